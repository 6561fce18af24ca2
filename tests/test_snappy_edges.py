"""K2 snappy at the decoder's own constants (pqg_snappy.hip): streams built
tag by tag (tests/snappy_build.py) that put tags on the parse window's ends,
the dense/sparse switch, the batch cut, the 4 KiB history ring's low edge,
every alignment of the literal writers, ragged output lengths and the 64 KiB /
4 KiB boundaries of the split decode, plus corruptions at the same places.

On the CPU: every valid case decodes in the oracle (decode_other.go restated)
and in pyarrow's snappy to the builder's plaintext; every property a case is
named for is recomputed from its tag log and the path model; every corrupt
case is an error in the oracle.  On the GPU: every case as a bare block and as
a page (V1 at device offsets 0, 1, 7, 15; V2 behind raw level bytes), with the
split decode required exactly for the block-shaped streams."""
import ctypes as C
import functools

import numpy as np
import pytest

import parity as P
import pqtest_util as U
import snappy_build as B
from oracle import pyoracle as O
from pqgpu import abi

SNAPPY, SIZE, CAPACITY = (abi.STATUS_CODES[k] for k in ("SNAPPY", "SIZE", "CAPACITY"))
SERIAL = 2  # PQG_PAGE_FLAG_SNAPPY_SERIAL
FLBA1 = dict(ptype=abi.FIXED_LEN_BYTE_ARRAY, type_length=1, codec=abi.CODEC_SNAPPY)


@functools.lru_cache(maxsize=None)
def valid():
    return B.valid_cases()


@functools.lru_cache(maxsize=None)
def corrupt():
    return B.corrupt_cases()


@functools.lru_cache(maxsize=None)
def oracle():
    """name -> (rc, bytes) of every case, computed once."""
    return {c.name: O.snappy_decode(c.comp, 1 << 20) for c in valid() + corrupt()}


def test_names_are_unique():
    names = [c.name for c in valid() + corrupt()]
    assert len(set(names)) == len(names)
    assert {c.family for c in valid()} == set("abcdefgh")


def test_valid_cases_decode_in_oracle():
    for c in valid():
        rc, out = oracle()[c.name]
        assert rc == 0 and out == c.plain, c.name


def test_valid_cases_decode_in_pyarrow():
    import pyarrow as pa
    for c in valid():
        if c.pyarrow:
            got = pa.decompress(c.comp, decompressed_size=len(c.plain), codec="snappy").to_pybytes()
            assert got == c.plain, c.name


def test_corrupt_cases_fail_in_oracle():
    for c in corrupt():
        assert oracle()[c.name][0] == SNAPPY, (c.name, oracle()[c.name][0])


def scan_block_shaped(log):
    """block_shaped() by a direct scan: vectors of each tag's first and last
    output byte and of each copy's first source byte, by their 64 KiB block."""
    if not log:
        return True
    d = np.array([t.d for t in log], np.int64)
    ln = np.array([t.ln for t in log], np.int64)
    src = np.array([t.d - t.off if t.kind == "C" else t.d for t in log], np.int64)
    return bool(np.all(d >> 16 == (d + ln - 1) >> 16) and np.all(src >> 16 == d >> 16))


def test_block_shaped_matches_scan():
    seen = set()
    for c in valid():
        assert c.b.block_shaped() == scan_block_shaped(c.log), c.name
        seen.add(c.b.block_shaped())
    assert seen == {True, False}


def check_claim(c, tr, claim):
    """One claimed property of case c, from its tag log and its trace."""
    kind, a = claim[0], claim[1:]
    log, st, hl = c.log, tr.steps, c.hl
    if kind == "rel":
        return st[a[0]].rel == a[1]
    if kind == "win_of":
        return st[a[0]].win == a[1]
    if kind == "path":
        return st[a[0]].path != "serial" if a[1] == "notserial" else st[a[0]].path == a[1]
    if kind == "writer":
        return st[a[0]].writer == a[1]
    if kind == "hdr_straddles":
        return st[a[0]].rel < B.K_POS <= st[a[0]].rel + log[a[0]].hdr  # its last byte is the window's, or past it
    if kind == "wintags":
        w = tr.windows[a[0]]
        return len(w["tags"]) == a[1] and (a[2] is None or all(log[i].kind == a[2] for i in w["tags"]))
    if kind == "winkind":
        return tr.windows[a[0]]["kind"] == a[1]
    if kind == "streak":
        return st[a[0]].path == "serial" and st[a[0]].streak == a[1]
    if kind == "serial_run":
        first, n = a
        return (all(st[first + k].path == "serial" and st[first + k].nth == k for k in range(n)) and
                st[first + n].path != "serial" and n in tr.serials)
    if kind == "span":  # tags first..last total 1024 - pre + delta from a batch's start at pre
        first, last, pre, delta = a
        bt = tr.batches[st[first].batch]
        total = sum(log[i].ln for i in range(first, last + 1))
        ok = bt["pre"] == pre and bt["tags"][0] == first and total == B.K_SPAN - pre + delta
        if delta <= 0:
            return ok and st[last].batch == st[first].batch and bt["filled"] == B.K_SPAN + delta
        return ok and st[last].batch == st[first].batch + 1 and st[last - 1].batch == st[first].batch
    if kind == "cut_tag":  # tag i is where its window was cut, the batch before it filled to a[1] bytes
        i, filled = a
        w = tr.windows[st[i - 1].win]
        return w["cut"] is not None and w["filled"] == filled and st[i].rel == 0 and st[i].batch == st[i - 1].batch + 1
    if kind == "winfilled":
        w, filled, joined = a
        return (tr.windows[w]["filled"] == filled and tr.windows[w]["cut"] is None and
                (tr.windows[w + 1]["batch"] == tr.windows[w]["batch"]) == joined)
    if kind == "batch":
        return tr.batches[a[0]][a[1]] == a[2]
    if kind == "cut0":
        return tr.batches[a[0]]["cut0"]
    if kind == "lit_end_minus_window":
        t = log[a[0]]
        return hl + t.next_s - (st[a[0]].in_base + B.K_WIN) == a[1]
    if kind == "same_batch_source":
        bt = tr.batches[st[a[0]].batch]
        return log[a[0]].d - log[a[0]].off >= bt["a0"] + bt["pre"]
    if kind == "copy_depth":  # a chain of a[1] copies, each reading the one before, all in one batch
        i, n = a
        return all(log[i - k].kind == "C" and log[i - k].d - log[i - k].off == log[i - k - 1].d and
                   st[i - k].batch == st[i].batch for k in range(n - 1))
    if kind == "source_straddles_batch_start":
        t, bt = log[a[0]], tr.batches[st[a[0]].batch]
        return t.d - t.off < bt["a0"] + bt["pre"] < t.d - t.off + t.ln
    if kind == "source_in_tag":
        t, u = log[a[0]], log[a[1]]
        return u.d <= t.d - t.off and t.d - t.off + min(t.ln, t.off) <= u.d + u.ln and st[a[0]].batch == st[a[1]].batch
    if kind == "below_ring":
        t = log[a[0]]
        return t.d - t.off + t.ln <= st[a[0]].ring_lo
    if kind == "src_minus_ring_lo":
        t = log[a[0]]
        return t.d - t.off - st[a[0]].ring_lo == a[1] and st[a[0]].ring_lo == B.ring_lo(t.d)
    if kind == "near_ring_edge":
        t = log[a[0]]
        return abs(t.d - t.off - B.ring_lo(t.d)) <= 1 and abs(t.d - t.off - st[a[0]].ring_lo) <= B.K_SPAN
    if kind == "off_is_d":
        return log[a[0]].off == log[a[0]].d
    if kind == "crosses":
        t = log[a[0]]
        return t.d < a[1] < t.d + t.ln
    if kind == "pre_salign":  # block offsets are addresses mod 16 when the block is aligned
        t = log[a[0]]
        return t.d % 16 == a[1] and (hl + t.s + t.hdr) % 16 == a[2]
    if kind == "pre":
        return log[a[0]].d % 16 == a[1]
    if kind == "slen_mod16":
        return len(c.comp) % 16 == a[0] and log[-1].kind == "L"
    if kind == "dlen":
        return len(c.plain) == a[0]
    if kind == "hl":
        return hl == a[0]
    if kind == "shaped":
        return c.b.block_shaped() == a[0]
    if kind == "ends_at":
        return log[a[0]].d + log[a[0]].ln == a[1]
    if kind == "starts_at":
        return log[a[0]].d == a[1]
    if kind == "src_minus_base":
        t = log[a[0]]
        return t.d - t.off - t.d // B.K_SUB * B.K_SUB == a[1] and t.d >= B.K_SUB
    if kind == "seg_rel":  # segments count from the first tag
        return log[a[0]].s % B.K_SEG == a[1] and log[a[0] - 1].kind == "L" and log[a[0] - 1].ln > B.K_SEG
    if kind == "seg_jump":
        t = log[a[0]]
        return t.next_s // B.K_SEG - t.s // B.K_SEG == a[1] and t.next_s % B.K_SEG < 64 and t.kind == "L"
    if kind == "clen_minus_hdr_mod":
        return (len(c.comp) - hl) % B.K_SEG == a[0] and len(c.plain) > B.K_SUB
    raise KeyError(kind)


def test_cases_have_their_properties():
    bad = []
    n = 0
    for c in valid():
        assert c.claims, c.name
        tr = B.trace(c.log, c.hl)
        for claim in c.claims:
            n += 1
            if not check_claim(c, tr, claim):
                bad.append((c.name, claim))
    assert not bad, bad[:10]
    assert n > 1000


def test_model_reaches_every_path():
    """Every family names at least one tag on each path it was built for."""
    want = {"a": {"dense"}, "b": {"dense", "sparse", "serial", "first"}, "c": {"dense", "first"},
            "d": {"dense"}, "e": {"dense", "serial"}, "f": {"serial", "sparse", "first"}, "g": {"dense", "sparse", "serial"},
            "h": {"dense", "sparse", "serial", "first"}}
    seen = {k: set() for k in want}
    for c in valid():
        seen[c.family] |= {s.path for s in B.trace(c.log, c.hl).steps}
    for k in want:
        assert want[k] <= seen[k], (k, seen[k])


# ---- mutations -----------------------------------------------------------
MUT_BASES = ("c_three_windows_of_2_byte_tags", "e_copies_along_ring_edge", "f_padded_headers_between_long_literals",
             "h_two_sub_blocks_of_copies")
MUT_PER_BASE = 500


def mutants(name):
    """MUT_PER_BASE seeded single-byte mutations of the named valid case."""
    base = {c.name: c for c in valid()}[name].comp
    rng = np.random.default_rng(sum(name.encode()))
    out = []
    for _ in range(MUT_PER_BASE):
        m = bytearray(base)
        i = int(rng.integers(0, len(m)))
        m[i] ^= int(rng.integers(1, 256))
        out.append(bytes(m))
    return out


@functools.lru_cache(maxsize=None)
def mutant_verdicts(name):
    return [O.snappy_decode(m, 1 << 20) for m in mutants(name)]


def test_mutation_bases_have_both_verdicts():
    """Each base leaves at least 5 % of its mutants decodable and at least 5 % in error."""
    for name in MUT_BASES:
        ok = sum(1 for rc, _ in mutant_verdicts(name) if rc == 0)
        print(name, "ok", ok, "errors", MUT_PER_BASE - ok)
        assert MUT_PER_BASE // 20 <= ok <= MUT_PER_BASE - MUT_PER_BASE // 20, (name, ok)


# ---- GPU -----------------------------------------------------------------
@pytest.fixture(scope="module")
def dec():
    import pqgpu
    d = pqgpu.GpuDecoder(0)
    yield d
    d.close()


def gpu_block(dec, src, dst):
    n = C.c_int64(0)
    rc = dec.L.pqg_block_decompress(dec.ctx, abi.CODEC_SNAPPY, src, len(src), dst.ctypes.data, len(dst), C.byref(n))
    return rc, dst[:n.value].tobytes() if rc == 0 else b""


@pytest.mark.gpu
def test_edges_block(dec):
    dst = np.zeros(1 << 20, np.uint8)
    bad = []
    for c in valid():
        rc, got = gpu_block(dec, c.comp, dst)
        if rc != 0 or got != c.plain:
            bad.append((c.name, abi.status_name(rc)))
    for c in corrupt():
        rc_o = oracle()[c.name][0]
        rc, _ = gpu_block(dec, c.comp, dst)
        if rc_o in (SIZE, CAPACITY):  # a changed varint: the buffer is sized from it
            rc_o = rc if rc != 0 else rc_o
        if rc != rc_o:
            bad.append((c.name, abi.status_name(rc), abi.status_name(rc_o)))
    assert not bad, bad


def v1_page(c):
    return U.page_header_v1(len(c.plain), len(c.comp), len(c.plain), 0) + c.comp


def def_levels(n, nbytes=6):
    """n definition levels of 1 (max_def 1) as RLE runs filling exactly six
    bytes: a run of m values is varint(m << 1) and the value byte, so 2, 3 or
    4 bytes for m up to 63, 8 191 and 2^20 - 1."""
    assert nbytes == 6
    lo, hi = {1: 1, 2: 64, 3: 8192}, {1: 63, 2: 8191, 3: (1 << 20) - 1}
    for hs in ((3, 1), (2, 2), (1, 1, 1)):
        if sum(lo[h] for h in hs) <= n <= sum(hi[h] for h in hs):
            ms = [lo[h] for h in hs]
            for k, h in enumerate(hs):
                ms[k] += min(hi[h] - lo[h], n - sum(ms))
            out = b"".join(U.uvarint(m << 1) + b"\x01" for m in ms)
            assert sum(ms) == n and len(out) == nbytes
            return out
    raise ValueError(n)


def v2_page(c, levels):
    n = len(c.plain)
    return U.page_header_v2(len(levels) + n, len(levels) + len(c.comp), n, 0, n, 0, len(levels), 0) + levels + c.comp


@functools.lru_cache(maxsize=None)
def v1_chunk():
    """The valid cases that hold a value as V1 pages of one chunk, and the oracle's decode of it."""
    cs = [c for c in valid() if c.plain]
    chunk = b"".join(v1_page(c) for c in cs)
    job, _ = U.chunk_job(chunk, keep=[], **FLBA1)
    return cs, chunk, O.decode_chunk(job)


def test_pages_decode_in_oracle():
    cs, chunk, exp = v1_chunk()
    assert exp.status == 0 and len(exp.pages) == len(cs)
    assert exp.values.tobytes() == b"".join(c.plain for c in cs)


def check_serial_flags(cs, pages):
    wrong = [(c.name, p.flags >> 8) for c, p in zip(cs, pages) if bool(p.flags & SERIAL) != (not c.b.block_shaped())]
    assert not wrong, wrong


@pytest.mark.gpu
@pytest.mark.parametrize("offset", [0, 1, 7, 15])
def test_edges_pages(dec, offset):
    cs, chunk, exp = v1_chunk()
    _, got = P.compare_chunk_bytes(chunk, dec, offset=offset, exp=exp, **FLBA1)
    assert got.status == 0 and len(got.pages) == len(cs)
    check_serial_flags(cs, got.pages)


V2_CASES = ("e_tag_d1_len64_ring_lo-1", "e_dense_d15_len64_ring_lo-1", "e_offset_65535_dense")


@pytest.mark.gpu
@pytest.mark.parametrize("nlevels", [1, 6])
def test_edges_pages_v2(dec, nlevels):
    """V2 pages keep their level bytes raw in front of the block: the block's
    source offset and alignment move by them.  Six bytes are two RLE runs of
    definition level 1 (max_def 1).  No level stream of one byte decodes, so
    the one-byte front is a definition-level byte of a required column
    (max_def 0), which the reader skips unread."""
    cs = [c for c in valid() if c.family == "h" or c.name in V2_CASES]
    assert len(cs) >= 20 + len(V2_CASES)
    chunk = b"".join(v2_page(c, def_levels(len(c.plain), nlevels) if nlevels > 1 else b"\x03") for c in cs)
    exp, got = P.compare_chunk_bytes(chunk, dec, max_def=int(nlevels > 1), **FLBA1)
    assert exp.status == 0 and exp.values.tobytes() == b"".join(c.plain for c in cs)
    check_serial_flags(cs, got.pages)


@pytest.mark.gpu
def test_edges_corrupt_pages(dec):
    """Each corrupt block as the third page of a chunk among valid pages, all
    chunks and one all-valid sibling in one decode call: every chunk fails at
    that page with the oracle's status, the pages before it are clean, and the
    sibling decodes exactly."""
    by = {c.name: c for c in valid()}
    v = [by[n] for n in ("e_dense_d8_len64_ring_lo+0", "h_len_65537", "d_period_17")]
    chunks = [b"".join(v1_page(c) for c in v)]
    for c in corrupt():
        hdr = U.page_header_v1(_declared(c), len(c.comp), _declared(c), 0)
        chunks.append(v1_page(v[0]) + v1_page(v[1]) + hdr + c.comp + v1_page(v[2]))
    keep, jobs, exps, offs = [], [], [], []
    at = 0
    for ch in chunks:
        job, buf = U.chunk_job(ch, keep=keep, **FLBA1)
        exps.append(O.decode_chunk(job))
        jobs.append(job)
        offs.append(at)
        at += (len(buf) + 63) & ~63
    big = np.zeros(at, np.uint8)
    for o, buf in zip(offs, keep):
        big[o:o + len(buf)] = buf
    dev = dec.upload(big)
    try:
        for job, o in zip(jobs, offs):
            job.data = dev + o
        res = dec.decode_jobs(jobs)
        for i, (r, exp) in enumerate(zip(res, exps)):
            got = dec.download(r, i)
            if i == 0:
                assert exp.status == 0
            else:
                c = corrupt()[i - 1]
                rc_o = oracle()[c.name][0]
                assert exp.status != 0 and exp.error_page == 2, c.name
                if _declared(c) == _varint(c):
                    assert exp.status == rc_o, c.name
                assert [p.status for p in got.pages[:3]] == [0, 0, exp.status], c.name
            P.compare_chunk(exp, got, "chunk %d" % i)
    finally:
        dec.free(dev)


def _varint(c):
    v, sft = 0, 0
    for b in c.comp:
        v |= (b & 0x7F) << sft
        sft += 7
        if b < 0x80:
            break
    return v


def _declared(c):
    """The page's uncompressed size: what the block's varint says, where a page header can say it."""
    v = _varint(c)
    return v if 0 < v < 1 << 20 else 7


@pytest.mark.gpu
def test_edge_mutations(dec):
    """2 000 single-byte mutations of four directed cases: the oracle's status
    (but CAPACITY for a changed varint) and, where it decodes, its bytes."""
    dst = np.zeros(1 << 20, np.uint8)
    bad = []
    for name in MUT_BASES:
        for k, (m, (rc_o, exp)) in enumerate(zip(mutants(name), mutant_verdicts(name))):
            rc, got = gpu_block(dec, m, dst)
            if rc_o in (SIZE, CAPACITY) and rc != 0:
                continue  # a changed varint: the buffer is sized from it
            if rc != rc_o or (rc == 0 and got != exp):
                bad.append((name, k, abi.status_name(rc), abi.status_name(rc_o)))
    assert not bad, bad[:10]
