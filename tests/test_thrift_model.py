"""K1's PageHeader reader without a GPU: pqg_thrift.h run on the host by tools/thrift_model.cpp,
with the serial walk's capacity and with the limits of one candidate-scan lane (the kCand*
constants of pqg_common.h behind a byte source like CandSrc), against the oracle's reader
(pqo_read_page_header) on generated and damaged headers (hdr_util.random_header / mutate).

  (a) the full parse is the oracle's: status, bytes consumed, every field both keep
      (the oracle's num_nulls, num_rows and is_compressed have no counterpart in PageHdr);
  (b) a bounded parse that reports neither `overflow` nor `hit` is the full parse, number for number;
  (c) so a bounded parse that differs has a flag set (the kernel turns either into kCOMPLEX, and
      the serial walk redoes the chunk) — and the run holds such headers;
  (d) `hit` is set exactly when the header does not end inside the candidate window;
  (e) `overflow` is set exactly past kCandSteps steps / kCandFrames frames / kCandLast entries.
"""
import os
import random
import re
import shutil
import subprocess

import pytest

import hdr_util as H
from oracle import pyoracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_HEADERS = 100_000
FIELDS = 16  # after status and consumed


def _consts():
    src = open(os.path.join(ROOT, "parquet-go_amd", "csrc", "pqg_common.h")).read()
    return {k: int(re.search(r"\b%s = (\d+)" % k, src).group(1))
            for k in ("kCandFrames", "kCandLast", "kCandSteps", "kCandWin", "kCandParseBytes")}


K = _consts()
WIN = 16 * K["kCandWin"]


def build_model(tmp, sanitize, source=None):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = os.path.join(str(tmp), "thrift_model_san" if sanitize else "thrift_model")
    cmd = [cxx, "-O1", "-g", "-std=c++17", "-Wno-unknown-pragmas", "-I", os.path.join(ROOT, "parquet-go_amd", "csrc"),
           source or os.path.join(ROOT, "tools", "thrift_model.cpp"), "-o", exe]
    if sanitize:
        cmd[1:1] = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    subprocess.run(cmd, check=True)
    return exe


def run_model(exe, items):
    """items: (alignment, bytes).  Per item (full, bounded, overflow, hit, pre): full and bounded
    are tuples (status, consumed, 16 fields)."""
    text = "".join("%d %s\n" % (a, b.hex()) for a, b in items)
    r = subprocess.run([exe], input=text, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    out = []
    lines = r.stdout.splitlines()
    assert len(lines) == len(items)
    for ln in lines:
        t = ln.split()
        assert t[0] == "F" and t[3 + FIELDS] == "B" and len(t) == 2 * (3 + FIELDS) + 3, ln
        f = tuple(int(x) for x in t[1:3 + FIELDS])
        b = tuple(int(x) for x in t[4 + FIELDS:6 + 2 * FIELDS])
        out.append((f, b) + tuple(int(x) for x in t[-3:]))
    return out


def oracle_tuple(b):
    """The oracle's result in the model's order."""
    rc, n, h = O.read_page_header(b)
    return (rc, n, h.type, h.uncompressed_size, h.compressed_size, h.dph_num_values, h.dph_encoding,
            h.dph_def_encoding, h.dph_rep_encoding, h.dict_num_values, h.dict_encoding, h.v2_num_values,
            h.v2_encoding, h.v2_def_len, h.v2_rep_len, h.has_dph, h.has_dict, h.has_v2)


@pytest.fixture(scope="module")
def headers():
    """(alignment, bytes) of N_HEADERS headers from a fixed seed — generated ones as they are, and
    damaged copies — each followed by some payload bytes, and the oracle's result for each."""
    rng = random.Random(20240521)
    items = []
    while len(items) < N_HEADERS:
        b = H.random_header(rng)
        if len(items) % 5 >= 3:
            b = H.mutate(rng, b)
            if rng.random() < 0.3 and b:
                b = H.mutate(rng, b)
        tail = bytes(rng.randrange(256) for _ in range(rng.randrange(0, 24))) if rng.random() < 0.8 else b""
        items.append((rng.randrange(16), b + tail))
    return items, [oracle_tuple(b) for _, b in items]


@pytest.fixture(scope="module")
def models(tmp_path_factory):
    d = tmp_path_factory.mktemp("thrift_model")
    return {False: build_model(d, False), True: build_model(d, True)}


def check_properties(items, exp, got):
    """Properties (a) to (c) over one run; returns the counts the caller bounds."""
    valid = flagged = differ = 0
    for (a, b), e, (f, bd, ovf, hit, pre) in zip(items, exp, got):
        assert f == e, "(a) full parse vs oracle: %s\n model  %s\n oracle %s" % (b.hex(), f, e)
        valid += e[0] == 0
        if not (ovf or hit):
            assert bd == f, "(b) bounded parse without a flag differs: a=%d %s\n bounded %s\n full    %s" % (
                a, b.hex(), bd, f)
        else:
            flagged += 1
        if bd != f:
            differ += 1
            assert ovf or hit, "(c) a differing bounded parse without a flag: a=%d %s" % (a, b.hex())
    return valid, flagged, differ


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_generated_headers(headers, models, sanitize):
    items, exp = headers
    assert len(items) >= 100_000
    got = run_model(models[sanitize], items)
    valid, flagged, differ = check_properties(items, exp, got)
    assert valid * 3 >= len(items), valid          # not all error paths
    assert (len(items) - valid) * 10 >= len(items)  # nor all valid
    assert flagged >= 1000 and differ >= 1000       # (c) is exercised


def _window_items():
    items = []
    pay = H.plain_i32(range(12))
    for n in range(120, 181):
        for kind in (1, 2):
            _, hb = H.pad_to(n, len(pay), len(pay), H.Hdr(kind, nvals=12))
            for a in range(16):
                items.append((a, hb + pay, n))
    return items


def test_window_edge(models):
    """(d): headers of 120..180 bytes (a Statistics binary as the filler, V1 and V2) at each start
    alignment a: the window holds WIN - a bytes of the header's granules."""
    items = _window_items()
    got = run_model(models[True], [(a, b) for a, b, _ in items])
    for (a, b, n), (f, bd, ovf, hit, pre) in zip(items, got):
        assert f[0] == 0 and f[1] == n and pre == 1
        assert not ovf
        assert hit == (n > WIN - a), (n, a, hit)
        if not hit:
            assert bd == f


def test_window_edge_at_the_chunk_end(models):
    """The last page's header in a chunk that ends inside the window: bytes past the chunk are EOF,
    not `hit`."""
    _, hb = H.pad_to(100, 0, 0, H.Hdr(1, nvals=0))
    (f, bd, ovf, hit, pre), = run_model(models[True], [(3, hb)])
    assert f[0] == 0 and bd == f and not hit and not ovf
    (f, bd, ovf, hit, pre), = run_model(models[True], [(3, hb[:-10])])
    assert f[0] != 0 and bd == f and not hit and not ovf


def test_parse_bytes_limit(models):
    """kCandParseBytes is never the limit while the window is shorter (both are asserted here so
    that a larger window brings this case back to mind)."""
    assert WIN < K["kCandParseBytes"] == 1024 and WIN == 160


def _limit_items():
    pay = H.plain_i32(range(12))
    items = []
    # steps: 3 top-level fields, K bools, the struct's field, its 4 fields and STOP, the STOP: K + 10
    for k in range(20, 41):
        spec = H.Hdr(1, nvals=12, order=[1, 2, 3, ("x", lambda w, k=k: w.bools(20, k)), "5"])
        items.append(("steps", k + 10 > K["kCandSteps"], spec))
    # frames: an unknown struct nested d deep holds d frames
    for d in range(1, 9):
        spec = H.Hdr(1, nvals=12, order=[1, 2, 3, "5", ("x", lambda w, d=d: w.nested(9, d))])
        items.append(("frames", d > K["kCandFrames"], spec))
    # lastField entries: PageHeader, DataPageHeader, Statistics and d nested unknown structs: 3 + d
    # (the frames run out first: kCandLast cannot be reached with kCandFrames = 4)
    for d in range(1, 9):
        st = H.stats_fields(null_count=1, extra=lambda w, d=d: w.nested(9, d))
        items.append(("last", d > K["kCandFrames"] or 3 + d > K["kCandLast"], H.Hdr(1, nvals=12, stats=st)))
    # a list of n lists of two i32: 2 frames.  Steps: 11 for the header (the list's field among them)
    # + per inner list 1 (the element starts) + 2 (its elements) + 1 (it closes) + 1 to close the
    # outer list + 1 that finds no frame left; n = 15, 16: the size as a varint
    for n in (5, 6, 7, 14, 15, 16):
        fn = lambda w, n=n: w.list_of(9, H.C_LIST, [bytes([0x25, 2, 4])] * n)  # noqa: E731
        items.append(("list", 11 + 4 * n + 2 > K["kCandSteps"], H.Hdr(1, nvals=12, order=[1, 2, 3, "5", ("x", fn)])))
    return [(what, over, spec.build(len(pay), len(pay)) + pay) for what, over, spec in items]


def test_overflow_edges(models):
    """(e): `overflow` exactly past the step budget and the frame stack; no `hit` (all these headers
    are shorter than the window); without overflow the bounded parse is the full one."""
    assert (K["kCandSteps"], K["kCandFrames"], K["kCandLast"]) == (40, 4, 8)
    items = _limit_items()
    got = run_model(models[True], [(0, b) for _, _, b in items])
    seen = set()
    for (what, over, b), (f, bd, ovf, hit, pre) in zip(items, got):
        assert f[0] == 0 and not hit, what
        assert bool(ovf) == over, (what, b.hex())
        if not ovf:
            assert bd == f
        seen.add((what, bool(ovf)))
    assert {(w, o) for w in ("steps", "frames", "last", "list") for o in (False, True)} <= seen


def test_hdr_util_round_trips():
    """Every valid built header reads back through the oracle with the fields written, and pad_to
    hits its length exactly."""
    pay = 48
    for n in list(range(30, 300)) + list(range(1000, 1040)) + list(range(2030, 2060)) + [16500]:
        for kind in (1, 2):
            _, hb = H.pad_to(n, pay, pay, H.Hdr(kind, nvals=12, enc=0))
            assert len(hb) == n
            e = oracle_tuple(hb + b"\x00" * pay)
            assert e[:5] == (0, n, 0 if kind == 1 else 3, pay, pay)
            assert (e[5] if kind == 1 else e[11]) == 12
    shapes = dict(
        plain=H.Hdr(1, nvals=9, enc=0),
        long2=H.Hdr(1, nvals=9, long=(2,)),
        wrap=H.Hdr(1, nvals=9, wrap=(1, 3)),
        pad1=H.Hdr(1, nvals=9, pad={1: 1}),
        pad_past10=H.Hdr(1, nvals=9, pad={2: 12}),
        usize5=H.Hdr(1, nvals=9, pad={2: 4}),
        wide=H.Hdr(1, nvals=9, wide=(2, 3)),
        order=H.Hdr(1, nvals=9, order=["5", 3, 1, 2]),
        repeat=H.Hdr(1, nvals=9, order=[1, 2, 3, 2, "5", 3, 1]),
        index=H.Hdr(1, nvals=9, order=[1, 2, 3, 6, "5"]),
        every=H.Hdr(1, nvals=9, order=[1, 2, 3, "5", ("x", lambda w: w.every_type(20))]),
        inner=H.Hdr(2, nvals=9, inner=lambda w: w.every_type(20), def_len=0),
        v2stats=H.Hdr(2, nvals=9, stats=H.stats_fields(b"a" * 70, b"z" * 70, 0, 3, b"q", b"r",
                                                       extra=lambda w: w.every_type(9))),
        crc=H.Hdr(1, nvals=9, crcs=[0xDEADBEEF, 7], order=[1, 2, 3, 4, "5", 4], long=(4,)),
        dict=H.Hdr("dict", nvals=9, enc=2),
    )
    for name, spec in shapes.items():
        hb = spec.build(36, 36)
        e = oracle_tuple(hb)
        assert e[:2] == (0, len(hb)), name
        assert e[3:5] == (36, 36), name
        nv = {1: e[5], 2: e[11], "dict": e[9]}[spec.kind]
        assert nv == 9, name
    # both structs: each keeps its own fields
    e = oracle_tuple(H.Hdr(1, nvals=9, enc=0, second=(8, 77, 5)).build(36, 36))
    assert e[0] == 0 and (e[5], e[6], e[11], e[12], e[15], e[17]) == (9, 0, 77, 5, 1, 1)
    # a known id with the wrong type is skipped: the required field is missing
    hb = H.Hdr(1, nvals=9, wrong=(3,)).build(36, 36)
    assert oracle_tuple(hb)[:2] == (-2, len(hb))
    # chunk(): offsets of the pages
    data, at = H.chunk([(H.Hdr(1, nvals=3), H.plain_i32([1, 2, 3]))] * 3)
    assert [oracle_tuple(data[h:])[1] for h, _ in at] == [p - h for h, p in at]
    assert at[1][0] == at[0][1] + 12
