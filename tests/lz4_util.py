"""Helpers of the LZ4_RAW tests: liblz4 through ctypes (the judge of what is
accepted), the compressor (pyarrow's lz4_raw codec), a builder of hand-made
blocks, the corpus, the seeded mutations, and the host model
(tools/lz4_model.cpp, built once per session)."""
import ctypes as C
import ctypes.util
import functools
import os
import struct
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LZ4, SIZE = -17, -4
WINDOW = 1024  # k_lz4's LDS window of compressed bytes (pqg_lz4.hip kLz4Win), refilled in 16-byte granules

# every cell of the format the model counts (tools/lz4_model.cpp), but its bounds guard
CELLS = ["ll_0", "ll_short", "ll_15", "ll_ext1", "ll_ext255", "ml_0", "ml_short", "ml_15", "ml_ext1", "ml_ext255",
         "match_overlap", "off_1", "off_far", "off_0", "last_only", "empty", "seqs_gt64", "batch"]


@functools.lru_cache(maxsize=None)
def liblz4():
    """liblz4, or None when this machine has none."""
    name = ctypes.util.find_library("lz4")
    if not name:
        return None
    try:
        L = C.CDLL(name)
    except OSError:
        return None
    L.LZ4_decompress_safe.restype = C.c_int
    L.LZ4_decompress_safe.argtypes = [C.c_char_p, C.c_void_p, C.c_int, C.c_int]
    L.LZ4_versionNumber.restype = C.c_int
    return L


def decompress_safe(z, cap):
    """LZ4_decompress_safe(z, dst, len(z), cap): (r, the r bytes when r >= 0)."""
    buf = (C.c_ubyte * max(cap, 1))()
    C.memset(buf, 0xA5, max(cap, 1))
    r = liblz4().LZ4_decompress_safe(bytes(z), buf, len(z), cap)
    return r, (bytes(buf[:r]) if r >= 0 else None)


def max_output(n):
    return 255 * n + 64


def reference(z, u=None):
    """The library's verdict by the project's rule: (status, bytes or None).
    u: a page that must decode to u bytes; None: a bare block."""
    if u is None:
        r, out = decompress_safe(z, max_output(len(z)))
        return (0, out) if r >= 0 else (LZ4, None)
    r, out = decompress_safe(z, u)
    if r == u:
        return 0, out
    big, _ = decompress_safe(z, max_output(len(z)))
    return (SIZE if big >= 0 and big != u else LZ4), None


def compress(raw):
    import pyarrow as pa
    return pa.Codec("lz4_raw").compress(raw, asbytes=True)


def _length(v):
    """The extension bytes of a length field whose nibble is 15."""
    return b"\xff" * (v // 255) + bytes([v % 255])


def block(seqs, last=b""):
    """The block of [(literals, offset, match_len), ...] and the last literals."""
    out = bytearray()
    for lit, off, ml in list(seqs) + [(last, None, None)]:
        ll = len(lit)
        m = 0 if ml is None else ml - 4
        assert m >= 0
        out.append(min(ll, 15) << 4 | min(m, 15))
        if ll >= 15:
            out += _length(ll - 15)
        out += lit
        if ml is not None:
            out += struct.pack("<H", off)
            if m >= 15:
                out += _length(m - 15)
    return bytes(out)


def expand(seqs, last=b""):
    """What block(seqs, last) decodes to (offset 0: zero bytes, as liblz4 writes them)."""
    out = bytearray()
    for lit, off, ml in seqs:
        out += lit
        for _ in range(ml):
            out.append(out[-off] if off else 0)
    return bytes(out + last)


def fnv(data):
    h = 0xcbf29ce484222325
    for b in data:
        h = ((h ^ b) * 0x100000001b3) & 0xFFFFFFFFFFFFFFFF
    return h


@functools.lru_cache(maxsize=None)
def corpus():
    rng = np.random.default_rng(2025)
    words = [b"w%x" % i for i in range(3000)]
    text = b" ".join(words[int(i) % 3000] for i in rng.zipf(1.3, 60000))[:200_000]
    far = rng.integers(0, 256, 40000, dtype=np.uint8).tobytes()
    return {
        "text": text,
        "text300": text[:300],
        "random": rng.integers(0, 256, 5000, dtype=np.uint8).tobytes(),
        "constant": b"\x5a" * 100_000,
        "arange": np.arange(20000, dtype=np.int64).tobytes(),
        "div9": (np.arange(5000, dtype=np.int32) // 9).tobytes(),
        "small_range": rng.integers(0, 50, 8000).astype(np.int64).tobytes(),
        "far": far + rng.integers(0, 256, 3000, dtype=np.uint8).tobytes() + far[:20000],
        "runs": b"".join(bytes([int(b)]) * int(k) for b, k in zip(rng.integers(0, 256, 300), rng.integers(1, 700, 300))),
        "empty": b"",
        "tiny": b"abc",
    }


def _lits(rng, n):
    return rng.integers(0, 256, n, dtype=np.uint8).tobytes()


TAIL = b"the-last-literals"  # 17 bytes: clear of every end-of-block rule


@functools.lru_cache(maxsize=None)
def hand_blocks():
    """name -> (block, what it decodes to): valid layouts, each field at and around its boundaries."""
    rng = np.random.default_rng(7)
    out = {}

    def add(name, seqs, last=TAIL):
        out[name] = (block(seqs, last), expand(seqs, last))

    for ll in (0, 1, 14, 15, 16, 269, 270, 271, 524, 525, 526, WINDOW - 1, WINDOW, WINDOW + 1):
        add("ll%d" % ll, [(_lits(rng, 8), 3, 5), (_lits(rng, ll), 2, 6)])
    for ml in (4, 5, 18, 19, 20, 273, 274, 275, 528, 529, 530):
        add("ml%d" % ml, [(_lits(rng, 40), 33, ml)])
    for off in (1, 2, 3, 4, 5, 7, 8, 63, 64, 65, 255, 256):
        add("off%d" % off, [(_lits(rng, 300), off, 21), (_lits(rng, 3), off, 300)])
    add("off65535", [(_lits(rng, 65535), 65535, 100), (b"xy", 65535, 4)])
    add("off65535_first_byte", [(_lits(rng, 65600), 65535, 9)])
    for off in range(1, 10):
        for ml in (63, 64, 65, 255, 256, 257):
            add("overlap_o%d_m%d" % (off, ml), [(_lits(rng, 11), off, ml)])
    # destination alignment x source alignment, literals (source: the input) and matches (source: the output)
    for d in range(4):
        for s in range(4):
            pre = _lits(rng, 16 + d)  # the second sequence's literals land at output 16 + d + 4
            # ... and start at input position 1 + (16 + d) + 2 + 1 + pad: pad literal bytes shift the source
            add("align_lit_d%d_s%d" % (d, s), [(pre, 5, 4), (_lits(rng, 37 + s), 9, 4 + s), (_lits(rng, 41), 30 + s, 50)])
            add("align_match_d%d_s%d" % (d, s), [(_lits(rng, 64 + d), 40 + ((d - s) % 4), 45)])
    # the same sweep through the copies by aligned dwords (pqg_wavecopy.h): literal runs longer than the
    # window, a match further back than k_lz4's LDS ring; s moves the destinations against the sources
    for d in range(4):
        for s in range(4):
            add("align_far_d%d_s%d" % (d, s), [(_lits(rng, 9), 3, 5 + s), (_lits(rng, 4200 + d), 4100 + (d - s) % 4, 300),
                                               (_lits(rng, WINDOW + 6), 4500, 70)])
    # k_lz4_batch takes a sequence into a batch only far from both ends of the block: the same boundaries
    # with 40 small sequences behind them.  Its own limits: literal runs of 32 bytes, grouped matches of 64,
    # and a match that reads the bytes of the match before it (offset 8: all of it, 15: its last byte,
    # 16 and 17: none; the one before and after may go in one pass only then)
    pad = [(b"pq", 4, 5)] * 40
    for ll in (0, 1, 15, 31, 32, 33, 270):
        add("batch_ll%d" % ll, [(_lits(rng, 8), 3, 5), (_lits(rng, ll), 2, 6)] + pad)
    for ml in (4, 19, 63, 64, 65, 274):
        add("batch_ml%d" % ml, [(_lits(rng, 300), 5, 4), (_lits(rng, 3), 290, ml), (_lits(rng, 1), 280, 8)] + pad)
    for off in (8, 15, 16, 17):
        add("batch_dep_off%d" % off, [(_lits(rng, 50), 20, 8), (b"", off, 8), (b"x", off + 9, 8)] + pad)
    add("batch_off0", [(_lits(rng, 20), 3, 5), (_lits(rng, 3), 0, 9)] + pad)
    for k in (1, 63, 64, 65, 127, 128, 129):
        add("seqs%d" % k, [(_lits(rng, 1 + i % 5), 1 + i % 3, 4 + i % 7) for i in range(k)])
    # fields across the window's refill boundary at WINDOW: after the first literal run the offset sits at p,
    # the match extension at p + 2, the next token at p + 4, its extension at p + 5, its literals at p + 7
    for p in range(WINDOW - 8, WINDOW + 2):
        ll = next(k for k in range(p - 8, p) if 1 + len(_length(k - 15)) + k == p)
        add("straddle_p%d" % p, [(_lits(rng, ll), 7, 4 + 15 + 255 + 9), (_lits(rng, 15 + 255 + 20), 400, 4 + 15 + 300)])
    add("empty", [], b"")
    add("literals_only", [], _lits(rng, 100))
    add("literals_only_long", [], _lits(rng, 3000))
    add("out_128k_plus_1", [(_lits(rng, 50), 50, 131072 - 50 - 5)], b"sixby" + b"!")
    add("off0", [(_lits(rng, 20), 0, 30)])  # the library writes zeros
    add("many_far", [(_lits(rng, 33000), 32768, 40)] + [(_lits(rng, 2), 32768 + i, 5) for i in range(70)])
    for name, (z, raw) in out.items():
        assert raw is not None
    assert out["off0"][1][20:50] == bytes(30)
    assert len(out["out_128k_plus_1"][1]) == 131073
    return out


@functools.lru_cache(maxsize=None)
def bad_blocks():
    """name -> (block, u): invalid layouts; u is the page size to try them with."""
    rng = np.random.default_rng(8)
    a = _lits(rng, 30)
    good = block([(a, 10, 20), (a[:3], 4, 300)], TAIL)
    u = len(expand([(a, 10, 20), (a[:3], 4, 300)], TAIL))
    out = {
        "offset_past_start": (block([(a, 31, 8)], TAIL), 30 + 8 + 17),
        "offset_past_start_far": (block([(a, 65535, 8)], TAIL), 30 + 8 + 17),
        "trailing_byte": (good + b"\x00", u),
        "match_ends_4_before_end": (block([(a, 10, 20)], b"1234"), 54),
        "no_last_literals": (block([(a, 10, 20)], b"")[:-1], 50),
        "n0": (b"", 0),
        "n0_u8": (b"", 8),
        # truncation inside each field: literal extension, literals, offset, match extension, last literals
        "cut_in_literal_ext": (block([(a * 10, 10, 20)], TAIL)[:2], 300),
        "cut_in_literals": (good[:10], u),
        "cut_in_literals_last_byte": (good[:31], u),
        "cut_after_literals": (good[:32], u),  # a literals-only block: well-formed, of another length
        "cut_in_offset": (good[:33], u),
        "cut_after_offset": (good[:34], u),
        "cut_in_match_ext": (good[:-len(TAIL) - 3], u),
        "cut_in_last_literals": (good[:-2], u),
    }
    return out


@functools.lru_cache(maxsize=None)
def huge_blocks():
    """name -> (block, u, status as a page of u bytes): extension runs that claim 2^31 bytes (8 MiB of
    0xff each; too large an output bound for the library's int, so the model alone judges them).  The
    literal run has no such input behind it; the match of 2 GiB at offset 3 is a well-formed block."""
    a = _lits(np.random.default_rng(9), 30)
    ff = b"\xff" * ((1 << 31) // 255 + 1)
    return {
        "ext_2g": (b"\xf0" + ff + b"\x00" + a, 1 << 20, LZ4),
        "match_ext_2g": (bytes([12 << 4 | 15]) + a[:12] + b"\x03\x00" + ff + b"\x00" + block([], TAIL), 1 << 20, SIZE),
    }


def mutation_block():
    raw = (np.arange(5000, dtype=np.int32) // 9).tobytes()
    return raw, compress(raw)


def mutations(count=2000, seed=1):
    """[bytes]: `count` mutations of 1-3 bytes each of the mutation block."""
    raw, z = mutation_block()
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(count):
        m = bytearray(z)
        for _ in range(int(rng.integers(1, 4))):
            m[int(rng.integers(0, len(m)))] = int(rng.integers(0, 256))
        out.append(bytes(m))
    return out


# ---- the host model
_BUILT = {}


def build_model(sanitize=False):
    if sanitize not in _BUILT:
        d = tempfile.mkdtemp(prefix="lz4_model_")
        exe = os.path.join(d, "lz4_model_san" if sanitize else "lz4_model")
        flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2"]
        subprocess.run([os.environ.get("CXX", "g++"), "-std=c++17", "-Wall", *flags,
                        "-I", os.path.join(ROOT, "parquet-go_amd", "csrc"),
                        os.path.join(ROOT, "tools", "lz4_model.cpp"), "-o", exe], check=True)
        _BUILT[sanitize] = exe
    return _BUILT[sanitize]


def model(z, u=None, want_bytes=True, step_a=False):
    """Run the model on z (a page of u bytes, or a bare block): dict(status, len, fnv, bytes, <counters>).
    It parses in batches as k_lz4's step B does; step_a: one sequence at a time."""
    exe = build_model()
    with tempfile.TemporaryDirectory() as d:
        src, dst = os.path.join(d, "in.lz4"), os.path.join(d, "out.bin")
        with open(src, "wb") as f:
            f.write(z)
        cmd = [exe] + (["-a"] if step_a else []) + (["-u", str(u)] if u is not None else []) + (["-o", dst] if want_bytes else []) + [src]
        r = subprocess.run(cmd, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        tok = r.stdout.split()
        res = {"status": int(tok[1]), "len": int(tok[3]), "fnv": int(tok[5], 16)}
        for t in tok[6:]:
            k, v = t.split("=")
            res[k] = int(v)
        res["bytes"] = open(dst, "rb").read() if want_bytes and res["status"] == 0 else None
        return res


def model_corpus(cases, sanitize=False, step_a=False):
    """Run the model over [(u or None, bytes)] in one process: [(status, len, fnv)], and the process's stderr."""
    exe = build_model(sanitize)
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "corpus.bin")
        with open(src, "wb") as f:
            f.write(struct.pack("<I", len(cases)))
            for u, z in cases:
                f.write(struct.pack("<II", 0xffffffff if u is None else u, len(z)) + z)
        r = subprocess.run([exe] + (["-a"] if step_a else []) + ["-m", src], capture_output=True, text=True)
        assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
        rows = [ln.split() for ln in r.stdout.splitlines()]
        return [(int(a), int(b), int(c, 16)) for a, b, c in rows], r.stderr
