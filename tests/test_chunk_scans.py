"""The per-chunk bookkeeping kernels (k_tile_scan, k_page_chain, k_page_list,
k_nn_scan*, k_finalize*) work in blocks of 1024 pages (or tiles) of a chunk,
one workgroup each, and chunks of more than 32 page blocks are walked by one
workgroup: chunks at the block edges, across them, and past the 32, against
the oracle (values, levels, offsets, per-page fields, status, error page).

A 16 KiB scan tile holds at most 64 header candidates and a data page header
gives about four (its inner `15 00 15` / `15 06 15` fields match the prefix
too), so chunks of 7-row pages take the serial header walk and exercise the
kernels after it; pages of more than 1 KiB stay on the candidate scan and
k_page_chain (asserted: serial_walk == 0).
"""
import os

import numpy as np
import pytest

import parity as P
import pqgpu
from gen import pqwrite as W

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dec_scan():
    """A decoder without the K1 stride walk (PQG_STRIDE=0, read at context
    creation): chunks of equal PLAIN pages take the candidate scan."""
    old = os.environ.get("PQG_STRIDE")
    os.environ["PQG_STRIDE"] = "0"
    try:
        d = pqgpu.GpuDecoder(0)
    finally:
        if old is None:
            os.environ.pop("PQG_STRIDE", None)
        else:
            os.environ["PQG_STRIDE"] = old
    yield d
    d.close()


def _plain_int64(pages, rpp):
    n = rpp * pages - (rpp // 2 if pages > 1 else 0)  # the last page short
    v = np.arange(n, dtype=np.int64) * 3 - 11
    return W.write_file([W.Column("x", W.INT64, v, rows_per_page=rpp)], n)


def _check(dec, data, pages=None, walk=None):
    P.compare_file(data, dec)
    got_walk, _, got_pages = dec.debug_job(0)[:3]
    if pages is not None:
        assert got_pages == pages
    if walk is not None:
        assert got_walk == walk


@pytest.mark.parametrize("pages", [1, 1023, 1024, 1025, 2049, 3073, 12289])
def test_page_counts_tiny_pages(dec_scan, pages):
    _check(dec_scan, _plain_int64(pages, 7), pages=pages)


@pytest.mark.parametrize("pages", [1023, 1024, 1025, 2049, 3073, 12289, 32 * 1024 + 1])
def test_page_counts_candidate_chain(dec_scan, pages):
    # 32 * 1024 + 1 pages: more blocks than a chunk is spread over
    _check(dec_scan, _plain_int64(pages, 160), pages=pages, walk=0)


def _optional_int64(pages, rpp, codec, seed=7):
    n = rpp * pages
    rng = np.random.default_rng(seed)
    d = (rng.random(n) >= 0.3).astype(np.uint8)
    v = rng.integers(-2**62, 2**62, size=int(d.sum()), dtype=np.int64)
    col = W.Column("x", W.INT64, v, repetition=W.OPTIONAL, def_levels=d, rows_per_page=rpp, codec=codec)
    return W.write_file([col], n)


@pytest.mark.parametrize("codec", [W.UNCOMPRESSED, W.SNAPPY])
@pytest.mark.parametrize("rpp", [7, 220])
def test_unequal_pages_with_nulls(dec_scan, rpp, codec):
    # not_null and the page lengths vary; SNAPPY: the scratch offsets
    _check(dec_scan, _optional_int64(2049, rpp, codec), pages=2049, walk=0 if rpp == 220 else None)


@pytest.mark.parametrize("rpp", [7, 1500])
def test_dictionary_pages_run_tables(dec_scan, rpp):
    # run_off / blk_off -> the walk -> k_dict4
    data, _ = W.config_c2(rows=rpp * 2049, bits=8, rows_per_page=rpp)
    _check(dec_scan, data, pages=2049 + 1, walk=0 if rpp == 1500 else None)


def _strings(pages, rpp, seed=9):
    n = rpp * pages
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, 12, size=n)
    offs = np.zeros(n + 1, dtype=np.int64)
    offs[1:] = np.cumsum(lens)
    chars = rng.integers(97, 123, size=int(offs[-1]), dtype=np.uint8)
    return W.write_file([W.Column("s", W.BYTE_ARRAY, chars, offsets=offs, rows_per_page=rpp)], n)


@pytest.mark.parametrize("rpp", [7, 130])
def test_string_offsets_across_blocks(dec_scan, rpp):
    _check(dec_scan, _strings(2049, rpp), pages=2049, walk=0 if rpp == 130 else None)


def test_several_chunks_in_one_call(dec_scan):
    # chunks of fewer pages than one block next to chunks of several; list offsets across chunks
    n = 2 * 7 * 1500
    rng = np.random.default_rng(11)
    d = (rng.random(n) >= 0.2).astype(np.uint8)
    cols = [W.Column("a", W.INT64, np.arange(n, dtype=np.int64), rows_per_page=7),
            W.Column("b", W.INT32, rng.integers(0, 1000, size=int(d.sum())).astype(np.int32), repetition=W.OPTIONAL,
                     def_levels=d, rows_per_page=50),
            W.Column("c", W.DOUBLE, rng.standard_normal(n), rows_per_page=5000)]
    data = W.write_file(cols, n, row_groups=2)
    res = P.compare_file(data, dec_scan)
    assert len(res) == 6
    assert [dec_scan.debug_job(i)[2] for i in range(6)] == [1500, 210, 3] * 2


def _oracle_pages(data):
    pf = pqgpu.ParquetFile(data)
    return pf.chunk_meta(0, 0).start, list(P.oracle_chunk(pf, 0, 0).pages)


def _expect_error(dec, data, page):
    res = P.compare_file(bytes(data), dec)  # status and error page are the oracle's
    assert res[0].status != 0 and res[0].error_page == page


@pytest.mark.parametrize("rpp", [7, 220])
def test_errors_across_block_edges(dec_scan, rpp):
    base = _optional_int64(2049, rpp, W.UNCOMPRESSED)
    start, pages = _oracle_pages(base)
    assert len(pages) == 2049
    for k in (1500, 2048):  # a damaged header
        b = bytearray(base)
        b[start + pages[k].header_offset + 4] ^= 0xFF
        _expect_error(dec_scan, b, k)
    b = bytearray(base)  # damaged level bytes on two pages: the first one counts
    for k in (1500, 300):
        at = start + pages[k].payload_offset
        b[at:at + 4] = b"\xff\xff\xff\x7f"
    _expect_error(dec_scan, b, 300)


@pytest.mark.parametrize("rpp", [7, 1400])
def test_dictionary_index_out_of_range_past_a_block(dec_scan, rpp):
    n = rpp * 2049
    rng = np.random.default_rng(13)
    v = rng.integers(0, 200, size=n).astype(np.int32) * 1000  # 200 entries: 8-bit indices, 200..255 out of range
    base = W.write_file([W.Column("x", W.INT32, v, encoding=W.RLE_DICTIONARY, rows_per_page=rpp)], n)
    start, pages = _oracle_pages(base)
    assert len(pages) == 2050  # the dictionary page first
    b = bytearray(base)
    b[start + pages[1031].payload_offset + 4] = 0xFF  # data page 1030: an index of its first bit-packed run
    _expect_error(dec_scan, b, 1031)


def test_tile_scan_past_one_block(dec_scan):
    # > 1024 scan tiles of 16 KiB in one chunk
    n = 2_200_000
    v = np.arange(n, dtype=np.int64) * 5
    data = W.write_file([W.Column("x", W.INT64, v, rows_per_page=20000)], n)
    assert len(data) > 1024 * 16384
    _check(dec_scan, data, pages=110, walk=0)
