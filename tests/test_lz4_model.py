"""The LZ4 block decoder of pqg_lz4.h on the host (tools/lz4_model.cpp: the
walk of LZ4_decompress_safe that k_lz4 runs) against liblz4 itself, reached
through ctypes: a compressed corpus, hand-built layouts at every boundary of
the format, invalid blocks, and 2 000 seeded mutations, as pages (a stated
size) and as bare blocks.  The verdict must be the library's by the rule of
lz4_util.reference: OK with its bytes, PQG_ERR_SIZE for a well-formed block of
another length, PQG_ERR_LZ4 for the rest.  The same inputs run through the
model built with AddressSanitizer / UBSan as a stand-alone program."""
import collections

import pytest

import lz4_util as Z
from pqgpu import abi

pa = pytest.importorskip("pyarrow")

needs_liblz4 = pytest.mark.skipif(Z.liblz4() is None, reason="liblz4 not found (ctypes.util.find_library('lz4'))")


def _same(z, u):
    """The model's and the library's verdict on z as a page of u bytes (None: bare): a mismatch, or None."""
    st, out = Z.reference(z, u)
    for step_a in (False, True):  # parsed in batches (step B) and one sequence at a time (step A)
        r = Z.model(z, u, step_a=step_a)
        if r["status"] != st or (st == 0 and (r["bytes"] != out or r["len"] != len(out))):
            return (step_a, st, r["status"], r["len"], None if out is None else len(out))
        assert r["guard"] == 0 and (r["batch"] == 0 or not step_a)
    return None


@pytest.fixture(scope="module")
def corpus_runs():
    return {name: Z.model(Z.compress(raw)) for name, raw in Z.corpus().items()}


@pytest.fixture(scope="module")
def hand_runs():
    return {name: Z.model(z) for name, (z, _) in Z.hand_blocks().items()}


def test_model_corpus_roundtrip(corpus_runs):
    for name, raw in Z.corpus().items():
        r = corpus_runs[name]
        assert r["status"] == 0 and r["len"] == len(raw) and r["bytes"] == raw and r["fnv"] == Z.fnv(raw), name
        assert r["guard"] == 0


@needs_liblz4
def test_model_corpus_matches_liblz4():
    for name, raw in Z.corpus().items():
        z = Z.compress(raw)
        for u in (None, len(raw), len(raw) + 1, max(len(raw) - 1, 0), len(raw) + 13):
            assert _same(z, u) is None, (name, u, _same(z, u))


@needs_liblz4
@pytest.mark.parametrize("name", sorted(Z.hand_blocks().keys()))
def test_model_hand_blocks(name):
    z, raw = Z.hand_blocks()[name]
    assert Z.reference(z) == (0, raw) and Z.reference(z, len(raw)) == (0, raw)
    # the sizes around the block's own: the end-of-block rules move with the buffer's end
    for u in [None] + [len(raw) + k for k in (-13, -12, -6, -5, -1, 0, 1, 5, 12, 13, 64) if len(raw) + k >= 0]:
        assert _same(z, u) is None, (name, u, _same(z, u))


@needs_liblz4
@pytest.mark.parametrize("name", sorted(Z.bad_blocks().keys()))
def test_model_bad_blocks(name):
    z, u = Z.bad_blocks()[name]
    st, _ = Z.reference(z, u)
    assert st != 0
    for v in (None, u, u + 1, max(u - 1, 0)):
        assert _same(z, v) is None, (name, v, _same(z, v))


@needs_liblz4
def test_liblz4_verdicts_pinned():
    """What the library (1.9.3) says where the format's description and its code part ways."""
    B = Z.bad_blocks()
    assert Z.reference(b"")[0] == Z.LZ4 and Z.reference(b"", 0)[0] == Z.LZ4
    assert Z.reference(b"\x00") == (0, b"") and Z.reference(b"\x00", 0) == (0, b"")
    assert Z.reference(*B["trailing_byte"])[0] == Z.LZ4
    assert Z.reference(*B["offset_past_start"])[0] == Z.LZ4
    # a match that ends 4 bytes before the end of a page: rejected; as a bare block (a far end) it decodes
    z, u = B["match_ends_4_before_end"]
    assert Z.reference(z, u)[0] == Z.LZ4 and Z.reference(z)[0] == 0
    # offset 0 is no error to the library: the match is zero bytes
    z, raw = Z.hand_blocks()["off0"]
    assert Z.reference(z) == (0, raw) and raw[20:50] == bytes(30)


@pytest.mark.parametrize("name", sorted(Z.huge_blocks().keys()))
def test_model_extension_runs_of_2g(name):
    """A run of extension bytes that claims 2^31 bytes ends in a verdict (64-bit lengths)."""
    z, u, want = Z.huge_blocks()[name]
    assert Z.model(z, u, want_bytes=False)["status"] == want
    if want == Z.LZ4:  # (the bare block of the other one decodes, to 2 GiB)
        assert Z.model(z, want_bytes=False)["status"] == Z.LZ4
    if Z.liblz4() is not None:
        assert Z.decompress_safe(z, u)[0] < 0


@pytest.mark.parametrize("cell", Z.CELLS)
def test_model_cells_covered(corpus_runs, hand_runs, cell):
    """The corpus (compressed inputs and hand-built layouts) reaches every cell the model counts."""
    assert sum(r[cell] for r in corpus_runs.values()) + sum(r[cell] for r in hand_runs.values()) > 0, cell


@pytest.mark.parametrize("want", [1, 63, 64, 65, 127, 128, 129])
def test_model_sequence_counts(hand_runs, want):
    r = hand_runs["seqs%d" % want]
    assert r["seqs"] == want and (r["seqs_gt64"] == 1) == (want > 64)


@needs_liblz4
def test_model_mutations_match_liblz4():
    """2 000 mutations of 1-3 bytes of one block: the library's class and bytes,
    and the library alone puts at least 50 cases in each of the three classes."""
    raw, z = Z.mutation_block()
    assert len(raw) == 20000 and 2500 < len(z) < 3000
    muts = Z.mutations(2000)
    for u, step_a in ((len(raw), False), (None, False), (len(raw), True), (None, True)):
        res, _ = Z.model_corpus([(u, m) for m in muts], step_a=step_a)
        classes, bad = collections.Counter(), []
        for i, (m, (rc, ln, h)) in enumerate(zip(muts, res)):
            st, out = Z.reference(m, u)
            classes[st] += 1
            if st != rc or (st == 0 and (ln != len(out) or Z.fnv(out) != h)):
                bad.append((i, st, rc, ln))
        assert not bad, (u, bad[:10])
        if u is not None:
            assert min(classes[0], classes[Z.SIZE], classes[Z.LZ4]) >= 50, classes
        else:
            assert min(classes[0], classes[Z.LZ4]) >= 50, classes


def test_model_sanitizer_clean():
    """The model built with -fsanitize=address,undefined (a stand-alone program)
    over the mutations, the hand-built and the invalid blocks, as pages of
    several sizes and as bare blocks."""
    raw, _ = Z.mutation_block()
    muts = Z.mutations(2000)
    cases = [(len(raw), m) for m in muts] + [(None, m) for m in muts] + [(0, m) for m in muts[:50]]
    for z, content in Z.hand_blocks().values():
        cases += [(None, z)] + [(max(len(content) + k, 0), z) for k in (-12, -5, -1, 0, 1, 64)]
    for z, u in Z.bad_blocks().values():
        cases += [(None, z), (u, z), (u + 1, z)]
    cases += [(u, z) for z, u, _ in Z.huge_blocks().values()]
    for step_a in (False, True):
        res, err = Z.model_corpus(cases, sanitize=True, step_a=step_a)
        assert len(res) == len(cases)
        assert "Sanitizer" not in err and "runtime error" not in err, err[-3000:]


def test_abi_constants():
    import ctypes as C
    import pqgpu
    assert abi.CODEC_LZ4_RAW == 7
    assert abi.STATUS[-17] == "LZ4" and abi.STATUS_CODES["LZ4"] == -17 == Z.LZ4 and abi.STATUS_CODES["SIZE"] == Z.SIZE
    hdr = open(Z.os.path.join(Z.ROOT, "include", "pqgpu.h")).read()
    assert "PQG_CODEC_LZ4_RAW = 7" in hdr and "PQG_ERR_LZ4 = -17" in hdr
    L = pqgpu._lib.lib()
    L.pqg_status_string.restype = C.c_char_p
    assert b"lz4" in L.pqg_status_string(-17)
