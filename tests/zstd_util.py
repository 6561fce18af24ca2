"""Helpers of the ZSTD tests: the input corpus, hand-built frames (raw / RLE
blocks, skippable frames, checksums), XXH64, the seeded mutations, and the
host model (tools/zstd_model.cpp, built once per session)."""
import functools
import os
import struct
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEVELS = (-5, 1, 3, 9, 19, 22)
MAGIC = 0xFD2FB528

# every format feature the model counts (tools/zstd_model.cpp)
CELLS = ["blk_raw", "blk_rle", "blk_comp",
         "frame_single", "frame_window", "fcs1", "fcs2", "fcs4", "frame_one_block", "frame_multi_block",
         "lit_raw", "lit_rle", "lit_huf1", "lit_huf4", "lit_treeless1", "lit_treeless4",
         "huf_direct", "huf_fse",
         "seq_none", "seq_short", "seq_mid", "seq_long",
         "ll_predef", "ll_rle", "ll_fse", "ll_repeat",
         "of_predef", "of_rle", "of_fse", "of_repeat",
         "ml_predef", "ml_rle", "ml_fse", "ml_repeat"]


def compress(raw, level):
    import pyarrow as pa
    return pa.Codec("zstd", compression_level=level).compress(raw, asbytes=True)


def libzstd(z, n):
    """libzstd's verdict on z for an output of n bytes: the bytes, or None."""
    import pyarrow as pa
    try:
        out = pa.Codec("zstd").decompress(z, decompressed_size=n, asbytes=True)
    except Exception:
        return None
    return out if len(out) == n else None


@functools.lru_cache(maxsize=None)
def corpus():
    rng = np.random.default_rng(2024)
    words = [b"w%x" % i for i in range(6000)]
    text = b" ".join(words[int(i) % 6000] for i in rng.zipf(1.25, 400000))[:850_000]
    assert len(text) == 850_000
    c = {
        "text": text,
        "text3000": text[:3000],
        "text200": text[:200],
        "random": rng.integers(0, 256, 65536, dtype=np.uint8).tobytes(),
        "constant": b"\x5a" * 300_000,
        "arange": np.arange(40000, dtype=np.int64).tobytes(),
        "small_range": rng.integers(0, 50, 30000).astype(np.int64).tobytes(),
        "coin": (rng.integers(0, 2, 100000, dtype=np.uint8) * 65).tobytes(),
    }
    # RLE literals: 5 000 random 12-byte patterns, each followed by a random
    # non-zero byte, padded with random bytes to one block; then every pattern
    # once in shuffled order, each followed by \0
    pats = [rng.integers(0, 256, 12, dtype=np.uint8).tobytes() for _ in range(5000)]
    first = b"".join(p + bytes([int(rng.integers(1, 256))]) for p in pats)
    first += rng.integers(0, 256, 131072 - len(first), dtype=np.uint8).tobytes()
    order = rng.permutation(5000)
    c["rle_literals"] = first + b"".join(pats[int(i)] + b"\0" for i in order)
    # direct Huffman weights: three symbols, probabilities ~ 0.6^i
    pr = np.array([0.6 ** i for i in range(3)])
    c["three_symbols"] = rng.choice(3, 4000, p=pr / pr.sum()).astype(np.uint8).tobytes()
    # long sequence count: 80 000 x (one of 64 random 3-byte tokens + a random byte)
    toks = [rng.integers(0, 256, 3, dtype=np.uint8).tobytes() for _ in range(64)]
    c["tokens"] = b"".join(toks[int(t)] + bytes([int(b)]) for t, b in
                           zip(rng.integers(0, 64, 80000), rng.integers(0, 256, 80000)))
    # a second block with few literals: treeless literals in one stream
    r2 = np.random.default_rng(5)
    c["two_blocks"] = text[:131072] + b"".join(
        text[int(q):int(q) + 300] + text[400000 + 37 * i:400000 + 37 * i + 8]
        for i, q in enumerate(r2.integers(0, 130000, 60)))
    return c


def fnv(data):
    h = 0xcbf29ce484222325
    for b in data:
        h = ((h ^ b) * 0x100000001b3) & 0xFFFFFFFFFFFFFFFF
    return h


# ---- XXH64 (seed 0)
_P1, _P2, _P3, _P4, _P5 = (0x9E3779B185EBCA87, 0xC2B2AE3D27D4EB4F, 0x165667B19E3779F9, 0x85EBCA77C2B2AE63,
                           0x27D4EB2F165667C5)
_M = 0xFFFFFFFFFFFFFFFF


def _rotl(x, r):
    return ((x << r) | (x >> (64 - r))) & _M


def _round(acc, x):
    return (_rotl((acc + x * _P2) & _M, 31) * _P1) & _M


def xxh64(data):
    n, i = len(data), 0
    if n >= 32:
        v = [(_P1 + _P2) & _M, _P2, 0, (-_P1) & _M]
        while i + 32 <= n:
            for k in range(4):
                v[k] = _round(v[k], int.from_bytes(data[i + 8 * k:i + 8 * k + 8], "little"))
            i += 32
        h = (_rotl(v[0], 1) + _rotl(v[1], 7) + _rotl(v[2], 12) + _rotl(v[3], 18)) & _M
        for k in range(4):
            h = (((h ^ _round(0, v[k])) * _P1) + _P4) & _M
    else:
        h = _P5
    h = (h + n) & _M
    while i + 8 <= n:
        h = (_rotl(h ^ _round(0, int.from_bytes(data[i:i + 8], "little")), 27) * _P1 + _P4) & _M
        i += 8
    if i + 4 <= n:
        h = (_rotl(h ^ ((int.from_bytes(data[i:i + 4], "little") * _P1) & _M), 23) * _P2 + _P3) & _M
        i += 4
    while i < n:
        h = (_rotl(h ^ ((data[i] * _P5) & _M), 11) * _P1) & _M
        i += 1
    h ^= h >> 33
    h = (h * _P2) & _M
    h ^= h >> 29
    h = (h * _P3) & _M
    h ^= h >> 32
    return h


# ---- hand-built frames of raw / RLE blocks
def block(kind, payload, last, size=None):
    """kind 0 raw (payload: its bytes), 1 RLE (payload: one byte, size: the run), 2 / 3: payload as is."""
    n = len(payload) if size is None else size
    return ((n << 3) | (kind << 1) | (1 if last else 0)).to_bytes(3, "little") + payload


def frame(blocks, content, fcs_bytes=0, single=False, checksum=False, window=0x50, dict_id=None, reserved=False,
          bad_checksum=False):
    """blocks: [(kind, payload, size or None)]; content: what they decode to (FCS, checksum)."""
    fid = {0: 0, 1: 0, 2: 1, 4: 2, 8: 3}[fcs_bytes]
    assert fcs_bytes != 1 or single
    fhd = fid << 6 | (0x20 if single else 0) | (8 if reserved else 0) | (4 if checksum else 0) | \
        (0 if dict_id is None else 1)
    out = struct.pack("<IB", MAGIC, fhd)
    if not single:
        out += bytes([window])
    if dict_id is not None:
        out += bytes([dict_id])
    if fcs_bytes == 2:
        out += (len(content) - 256).to_bytes(2, "little")
    elif fcs_bytes:
        out += len(content).to_bytes(fcs_bytes, "little")
    for i, (kind, payload, size) in enumerate(blocks):
        out += block(kind, payload, i == len(blocks) - 1, size)
    if checksum:
        out += ((xxh64(content) ^ (1 if bad_checksum else 0)) & 0xFFFFFFFF).to_bytes(4, "little")
    return out


def skippable(payload, nibble=3):
    return struct.pack("<II", 0x184D2A50 | nibble, len(payload)) + payload


def hand_frames():
    """name -> (frame bytes, the content a valid one decodes to)."""
    rng = np.random.default_rng(77)
    a = rng.integers(0, 256, 700, dtype=np.uint8).tobytes()
    b = bytes(rng.integers(0, 4, 300, dtype=np.uint8))
    raw = lambda x: (0, x, None)
    fa = frame([raw(a)], a, fcs_bytes=2)
    fb = frame([raw(b[:100]), (1, b"q", 50), raw(b[100:])], b[:100] + b"q" * 50 + b[100:], fcs_bytes=4)
    cb = b[:100] + b"q" * 50 + b[100:]
    big = bytes(rng.integers(0, 256, 131073, dtype=np.uint8))
    return {
        "checksum_ok": (frame([raw(a)], a, fcs_bytes=2, checksum=True), a),
        "checksum_bad": (frame([raw(a)], a, fcs_bytes=2, checksum=True, bad_checksum=True), a),
        "no_fcs_window": (frame([raw(a)], a), a),
        "single_fcs1": (frame([raw(a[:200])], a[:200], fcs_bytes=1, single=True), a[:200]),
        "fcs8": (frame([raw(a)], a, fcs_bytes=8), a),
        "skip_first": (skippable(b"hello") + fa, a),
        "skip_between": (fa + skippable(b"", 0xF) + fb, a + cb),
        "skip_last": (fa + skippable(b"x" * 40), a),
        "two_frames": (fa + fb, a + cb),
        "three_frames": (fb + fa + fb, cb + a + cb),
        "empty_frame": (frame([raw(b"")], b"", fcs_bytes=1, single=True), b""),
        "empty_last_block": (frame([raw(a), raw(b"")], a, fcs_bytes=2), a),
        "rle_only": (frame([(1, b"\x07", 5000)], b"\x07" * 5000, fcs_bytes=2), b"\x07" * 5000),
        "dict_id": (frame([raw(a)], a, fcs_bytes=2, dict_id=5), a),
        "dict_id_zero": (frame([raw(a)], a, fcs_bytes=2, dict_id=0), a),
        "reserved_bit": (frame([raw(a)], a, fcs_bytes=2, reserved=True), a),
        "block_type3": (frame([(3, a, None)], a, fcs_bytes=2), a),
        "block_128k_plus_1": (frame([raw(big)], big, fcs_bytes=4, window=0x58), big),
        "fcs_mismatch": (frame([raw(a)], a + b"z", fcs_bytes=2), a),
        "window_too_large": (frame([raw(a)], a, window=0xB0), a),
        "trailing1": (fa + b"\x00", a),
        "trailing2": (fa + b"\x28\xb5", a),
        "trailing3": (fa + b"\x28\xb5\x2f", a),
        "truncated_header": (fa[:6], a),
        "truncated_block": (fa[:-10], a),
        "bad_magic": (b"\x27" + fa[1:], a),
    }


# ---- shapes at which lanes and batches can go wrong (level 3)
def _no_repeats(n, rng):
    """n bytes over 24 symbols of skewed frequencies in which no 3 bytes occur twice (no match to find)."""
    pr = np.array([0.8 ** i for i in range(24)])
    pr /= pr.sum()
    out, seen = [0, 1], set()
    while len(out) < n:
        for s in list(rng.choice(24, 40, p=pr)) + list(range(24)):
            g = (out[-2], out[-1], int(s))
            if g not in seen:
                seen.add(g)
                out.append(int(s))
                break
        else:
            raise AssertionError("no unused 3-gram")
    return bytes(b + 97 for b in out[:n])


def lane_shapes():
    rng = np.random.default_rng(91)
    out = {}
    for n in range(1021, 1028):  # n literals and no match: four Huffman streams, a ragged fourth
        out["lits%d" % n] = _no_repeats(n, rng)
    for off in (1, 2, 3, 7):  # overlapping matches
        seed = rng.integers(0, 256, off, dtype=np.uint8).tobytes()
        out["overlap%d" % off] = rng.integers(0, 256, 100, dtype=np.uint8).tobytes() + seed * (700 // off) + b"end"
    out["block131072"] = (b" ".join(b"%d" % int(i) for i in rng.integers(0, 3000, 40000)))[:131072]
    assert len(out["block131072"]) == 131072
    return out


def seq_input(k, rng):
    """An input that compresses (level 3) to about k sequences: k repeats of
    16-byte strings seen before, separated by fresh random bytes."""
    pool = [rng.integers(0, 256, 16, dtype=np.uint8).tobytes() for _ in range(8)]
    parts = list(pool)
    for i in range(k):
        parts.append(rng.integers(0, 256, 6, dtype=np.uint8).tobytes())
        parts.append(pool[i % 8])
    return b"".join(parts)


@functools.lru_cache(maxsize=None)
def seq_count_frame(want):
    """(frame, raw) of one block with exactly `want` sequences (read from the model's counters)."""
    for k in range(max(want - 12, 1), want + 12):
        raw = seq_input(k, np.random.default_rng(1000 + k))
        z = compress(raw, 3)
        if model(z, want_bytes=False)["seqs"] == [want]:
            return z, raw
    raise AssertionError("no input with %d sequences" % want)


# ---- seeded mutations
def mutation_frames():
    c = corpus()
    srcs = [(c["text3000"], 3), (c["text200"], 3), (c["three_symbols"], 3), (c["small_range"][:8192], 19),
            (c["coin"][:8192], 1)]
    return [(raw, compress(raw, lvl)) for raw, lvl in srcs]


def mutations(count=2000, frames=None, seed=123):
    """[(frame index, mutated bytes)]: single-byte changes and truncations."""
    frames = frames if frames is not None else mutation_frames()
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(count):
        f = int(rng.integers(0, len(frames)))
        z = bytearray(frames[f][1])
        if rng.integers(0, 5) == 0:
            z = z[:int(rng.integers(0, len(z)))]
        else:
            i = int(rng.integers(0, len(z)))
            z[i] ^= int(rng.integers(1, 256))
        out.append((f, bytes(z)))
    return out


# ---- the host model
_BUILT = {}


def build_model(sanitize=False):
    if sanitize not in _BUILT:
        d = tempfile.mkdtemp(prefix="zstd_model_")
        exe = os.path.join(d, "zstd_model_san" if sanitize else "zstd_model")
        flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2"]
        subprocess.run([os.environ.get("CXX", "g++"), "-std=c++17", "-Wall", *flags,
                        "-I", os.path.join(ROOT, "parquet-go_amd", "csrc"),
                        os.path.join(ROOT, "tools", "zstd_model.cpp"), "-o", exe], check=True)
        _BUILT[sanitize] = exe
    return _BUILT[sanitize]


def model(z, cap=None, want_bytes=True):
    """Run the model on z: dict(status, len, fnv, bytes, seqs, <counters>)."""
    exe = build_model()
    with tempfile.TemporaryDirectory() as d:
        src, dst = os.path.join(d, "in.zst"), os.path.join(d, "out.bin")
        with open(src, "wb") as f:
            f.write(z)
        cmd = [exe] + (["-c", str(cap)] if cap is not None else []) + (["-o", dst] if want_bytes else []) + [src]
        r = subprocess.run(cmd, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        tok = r.stdout.split()
        res = {"status": int(tok[1]), "len": int(tok[3]), "fnv": int(tok[5], 16)}
        for t in tok[6:]:
            k, v = t.split("=")
            res[k] = [int(x) for x in v.split(",") if x] if k == "seqs" else int(v)
        res["bytes"] = open(dst, "rb").read() if want_bytes and res["status"] == 0 else None
        return res


def model_corpus(cases, sanitize=False):
    """Run the model over [(cap, bytes)] in one process: [(status, len, fnv)], and the process's stderr."""
    exe = build_model(sanitize)
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "corpus.bin")
        with open(src, "wb") as f:
            f.write(struct.pack("<I", len(cases)))
            for cap, z in cases:
                f.write(struct.pack("<II", cap, len(z)) + z)
        r = subprocess.run([exe, "-m", src], capture_output=True, text=True)
        assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
        rows = [ln.split() for ln in r.stdout.splitlines()]
        return [(int(a), int(b), int(c, 16)) for a, b, c in rows], r.stderr
