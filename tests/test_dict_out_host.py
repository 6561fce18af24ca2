"""Host side of the keep-dictionary decode (PQG_COL_KEEP_DICT, K4i), no GPU: the ABI additions
(pqg_get_dictionary, PQG_ERR_NOT_DICT, pqg_dictionary's layout against its ctypes mirror) and
DecodedColumn.materialize(), the host gather dictionary[keys], against the oracle's decode of small
dictionary files."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import pqgpu
from gen import pqwrite as W
from oracle import pyoracle as O
from pqgpu import _lib, abi
from pqgpu.reader import DecodedColumn, Dictionary

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "pqgpu.h")


def test_abi_declares_and_exports_dictionary_entry():
    text = open(HEADER).read()
    assert re.search(r"\bint\s+pqg_get_dictionary\s*\(\s*pqg_ctx\s*\*[^,]*,\s*int\s+\w+,\s*pqg_dictionary\s*\*", text)
    assert re.search(r"\bPQG_COL_KEEP_DICT\s*=\s*2\b", text)
    assert re.search(r"\bPQG_ERR_NOT_DICT\s*=\s*-19\b", text)
    L = _lib.lib()
    assert hasattr(L, "pqg_get_dictionary") and "pqg_get_dictionary" in _lib.EXPORTED
    assert abi.STATUS_CODES["NOT_DICT"] == -19 and abi.COL_KEEP_DICT == 2
    msg = L.pqg_status_string(-19)
    others = {L.pqg_status_string(c) for c in range(-40, 1) if c != -19}
    assert msg and msg != b"unknown" and msg not in others


def test_dictionary_struct_layout(tmp_path):
    """sizeof / offsetof of pqg_dictionary as a C compiler lays it out from the header."""
    fields = [f for f, _ in abi.Dictionary._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "pqgpu.h"\nint main(void) {\n'
                   '  printf("%zu\\n", sizeof(pqg_dictionary));\n'
                   + "".join('  printf("%%zu\\n", offsetof(pqg_dictionary, %s));\n' % f for f in fields)
                   + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    cc = next((c for c in ("cc", "gcc", "clang", "/opt/rocm/llvm/bin/clang")
               if subprocess.run(["sh", "-c", "command -v " + c], capture_output=True).returncode == 0), None)
    assert cc, "no C compiler"
    subprocess.run([cc, "-std=c99", "-I", os.path.dirname(HEADER), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got[0] == C.sizeof(abi.Dictionary)
    assert got[1:] == [getattr(abi.Dictionary, f).offset for f in fields]


# ---- materialize() ---------------------------------------------------------------------------------
N = 700


def _opt_levels(rng, n, nn):
    d = np.zeros(n, np.uint8)
    d[rng.choice(n, nn, replace=False)] = 1
    return d


def _files():
    """name -> (file bytes, value width): small dictionary files of the synthetic writer, several pages."""
    rng = np.random.default_rng(11)
    out = {}
    out["int32"] = (W.Column("v", W.INT32, rng.integers(-50, 50, N).astype(np.int32), encoding=W.RLE_DICTIONARY,
                             rows_per_page=300), 4)
    out["int64"] = (W.Column("v", W.INT64, rng.integers(-2 ** 40, 2 ** 40, 9)[rng.integers(0, 9, N)],
                             encoding=W.RLE_DICTIONARY, rows_per_page=256), 8)
    out["double"] = (W.Column("v", W.DOUBLE, rng.standard_normal(13)[rng.integers(0, 13, N)],
                              encoding=W.RLE_DICTIONARY, rows_per_page=300), 8)
    pool5 = rng.integers(0, 256, (17, 5), dtype=np.uint8)
    out["flba5"] = (W.Column("v", W.FLBA, pool5[rng.integers(0, 17, N)].reshape(-1), type_length=5,
                             encoding=W.RLE_DICTIONARY, rows_per_page=300), 5)
    pool12 = rng.integers(0, 256, (6, 12), dtype=np.uint8)
    out["int96"] = (W.Column("v", W.INT96, pool12[rng.integers(0, 6, N)].reshape(-1), encoding=W.RLE_DICTIONARY,
                             rows_per_page=300), 12)
    # byte arrays with empty strings, and nulls
    words = [b"", b"a", b"parquet", b"", b"x" * 40, b"dictionary"]
    nn = N - 90
    pick = rng.integers(0, len(words), nn)
    lens = np.array([len(words[k]) for k in pick], np.int64)
    offs = np.zeros(nn + 1, np.int64)
    np.cumsum(lens, out=offs[1:])
    chars = np.frombuffer(b"".join(words[k] for k in pick), np.uint8)
    out["bytes_nulls"] = (W.Column("v", W.BYTE_ARRAY, chars, offsets=offs, encoding=W.RLE_DICTIONARY,
                                   repetition=W.OPTIONAL, def_levels=_opt_levels(rng, N, nn), rows_per_page=300), 0)
    out["int32_nulls"] = (W.Column("v", W.INT32, rng.integers(0, 5, nn).astype(np.int32), encoding=W.RLE_DICTIONARY,
                                   repetition=W.OPTIONAL, def_levels=_opt_levels(rng, N, nn), rows_per_page=300), 4)
    return {k: (W.write_file([c], N), w) for k, (c, w) in out.items()}


@pytest.fixture(scope="module")
def oracle_chunks():
    res = {}
    for name, (data, w) in _files().items():
        pf = pqgpu.ParquetFile(data)
        ch = O.decode_chunk(pf.host_job(0, 0)[0])
        assert ch.status == 0 and ch.value_width == w and ch.num_values > 0
        assert any(p.encoding == 8 for p in ch.pages), "not a dictionary chunk"
        res[name] = ch
    return res


def _split(ch):
    """The oracle's values as np.unique leaves them: (Dictionary, int32 keys)."""
    n, w = ch.num_values, ch.value_width
    if w > 0:
        rows = np.asarray(ch.values, np.uint8).reshape(n, w)
        table, keys = np.unique(rows, axis=0, return_inverse=True)
        return Dictionary(table.reshape(-1).copy(), None, len(table), w), keys.reshape(-1).astype(np.int32)
    b, o = np.asarray(ch.values, np.uint8).tobytes(), np.asarray(ch.offsets)
    vals = [b[o[i]:o[i + 1]] for i in range(n)]
    uniq = sorted(set(vals))
    index = {v: k for k, v in enumerate(uniq)}
    doffs = np.zeros(len(uniq) + 1, np.int64)
    np.cumsum([len(v) for v in uniq], out=doffs[1:])
    d = Dictionary(np.frombuffer(b"".join(uniq), np.uint8), doffs, len(uniq), 0)
    return d, np.array([index[v] for v in vals], np.int32)


def _kept(ch, d, keys):
    return DecodedColumn(0, -1, ch.num_slots, ch.num_values, 4, ch.def_levels, ch.rep_levels,
                         np.ascontiguousarray(keys, "<i4").view(np.uint8), ch.pages, None, dictionary=d)


@pytest.mark.parametrize("name", ["int32", "int64", "double", "flba5", "int96", "bytes_nulls", "int32_nulls"])
def test_materialize_matches_oracle(oracle_chunks, name):
    ch = oracle_chunks[name]
    d, keys = _split(ch)
    col = _kept(ch, d, keys)
    assert col.dictionary is d and col.value_width == 4 and col.offsets is None
    assert np.array_equal(col.keys(), keys)
    m = col.materialize()
    assert m.dictionary is None and m.value_width == ch.value_width
    assert (m.num_slots, m.num_values) == (ch.num_slots, ch.num_values)
    assert m.values.dtype == np.uint8 and m.values.tobytes() == np.asarray(ch.values).tobytes()
    if ch.value_width == 0:
        assert m.offsets.dtype == np.int64 and np.array_equal(m.offsets, ch.offsets)
    else:
        assert m.offsets is None
    if ch.def_levels is not None:
        assert np.array_equal(m.def_levels, ch.def_levels)
    assert m.materialize() is m  # already materialised


def test_materialize_nil_entry():
    """A truncated INT96 dictionary: the last entry has 5 of its 12 bytes and reads as zeros (Q8)."""
    raw = np.arange(2 * 12 + 5, dtype=np.uint8) + 1
    d = Dictionary(raw, None, 3, 12, nil_entry=2)
    keys = np.array([2, 0, 1, 2, 2, 0], np.int32)
    col = DecodedColumn(0, -1, 6, 6, 4, None, None, keys.view(np.uint8), None, None, dictionary=d)
    exp = np.zeros((6, 12), np.uint8)
    exp[1], exp[5], exp[2] = raw[:12], raw[:12], raw[12:24]
    m = col.materialize()
    assert m.value_width == 12 and np.array_equal(m.values, exp.reshape(-1))
    assert d.pylist(abi.INT96)[2] == bytes(12)


def test_materialize_rejects_bad_key_and_empty():
    d = Dictionary(np.zeros(8, np.uint8), None, 2, 4)
    bad = DecodedColumn(0, -1, 1, 1, 4, None, None, np.array([2], np.int32).view(np.uint8), None, None, dictionary=d)
    with pytest.raises(IndexError):
        bad.materialize()
    # an all-null column: no keys, an empty dictionary
    e = Dictionary(np.zeros(0, np.uint8), np.zeros(1, np.int64), 0, 0)
    col = DecodedColumn(0, -1, 5, 0, 4, np.zeros(5, np.uint8), None, np.zeros(0, np.uint8), None, None, dictionary=e)
    m = col.materialize()
    assert m.values.nbytes == 0 and np.array_equal(m.offsets, [0]) and m.value_width == 0


def test_mutation_seed_rarely_leaves_the_dictionary():
    """The GPU test's 200 mutations (dictout_util): from the oracle's page tables alone, at most 10 % of
    them show a data page of another encoding, the only way a flagged decode may end NOT_DICT."""
    import dictout_util as D
    ms = D.mutations()
    assert len(ms) == D.MUTATIONS == 200 and len(set(ms)) > 150
    hit = 0
    for data in ms:
        pf = pqgpu.ParquetFile(data)
        hit += any(D.other_encoding_page(O.decode_chunk(pf.host_job(0, c)[0], D.PAGE_CAP))
                   for c in range(pf.num_columns))
    assert hit <= D.MUTATIONS // 10, hit
