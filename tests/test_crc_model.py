"""Page checksums without a GPU: k_page_crc's tile and combine code (pqg_crc.h) run on the host by
tools/crc_model.cpp, the shared CRC arithmetic against zlib, and the yardstick the GPU tests judge by.

The last test passes with or without the feature: it pins that PageHeader.crc of a pyarrow file is
zlib.crc32 of the page's compressed_size bytes at payload_offset (V1 and V2, dictionary pages too),
and that crc_util reads and rewrites the field."""
import os
import shutil
import subprocess
import zlib

import numpy as np
import pytest

import crc_util as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(tmp_path, sanitize):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / ("crc_model_san" if sanitize else "crc_model"))
    cmd = [cxx, "-O1", "-g", "-std=c++17", "-Wno-unknown-pragmas", "-I", os.path.join(ROOT, "parquet-go_amd", "csrc"),
           os.path.join(ROOT, "tools", "crc_model.cpp"), "-o", exe]
    if sanitize:
        cmd[1:1] = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    subprocess.run(cmd, check=True)
    return exe


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_host_model_of_the_kernel(tmp_path, sanitize):
    """Lengths 0..600 at every start alignment, every length within 17 of a lane slice, a wave row,
    one, two and three tiles at 4 alignments, and 4 MiB + 5 bytes (a combine over more than 256
    tiles): every load aligned and inside the range's granules, every result the plain CRC."""
    exe = _build(tmp_path, sanitize)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("ok "), r.stdout + r.stderr[-3000:]
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    cases = int(r.stdout.split()[1])
    assert cases >= 16 * 601 + 5 * 4 * 35 + 1


def test_combine_identity_against_zlib(tmp_path):
    """crc32(A || B) from crc32(A), crc32(B) and |B| by the shared multmodp / x8nmodp."""
    exe = _build(tmp_path, False)
    rng = np.random.default_rng(5)
    buf = rng.integers(0, 256, 1 << 20, dtype=np.uint8).tobytes()
    lines, want = [], []
    for n in [0, 1, 2, 3, 15, 16, 17, 255, 4096, 65537, 1 << 20] + [int(x) for x in rng.integers(0, 1 << 20, 40)]:
        for cut in sorted({0, n, n // 2, int(rng.integers(0, n + 1))}):
            a, b = buf[:cut], buf[cut:n]
            lines.append("%d %d %d" % (zlib.crc32(a), zlib.crc32(b), len(b)))
            want.append(zlib.crc32(buf[:n]))
    r = subprocess.run([exe, "combine"], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert r.returncode == 0
    got = [int(x) for x in r.stdout.split()]
    assert got == want


pa = pytest.importorskip("pyarrow")


@pytest.mark.parametrize("compression", ["none", "snappy"])
@pytest.mark.parametrize("version", ["1.0", "2.0"])
def test_pyarrow_page_crc_is_zlib_crc32_of_the_stored_bytes(version, compression):
    import pqgpu
    import parity as P
    table, kw = K.four_columns(2000)
    data = K.write_table(table, version, compression, **kw)
    pf = pqgpu.ParquetFile(data)
    seen = dict(dict_pages=0, data_pages=0)
    for col in range(pf.num_columns):
        m = pf.chunk_meta(0, col)
        chunk = bytes(pf.data[m.start:m.start + m.total_compressed_size])
        exp = P.oracle_chunk(pf, 0, col)
        assert exp.status == 0
        pages = K.split_pages(chunk, exp.pages)
        assert len(pages) >= 2
        for p, info in zip(pages, exp.pages):
            assert p.crc is not None and p.crc == K.crc32(p.payload), (col, info.page_type)
            assert K.header_crc(p.header)[1] == len(p.header)
            seen["dict_pages" if info.page_type == 2 else "data_pages"] += 1
            # the helper's rewrites: the same value gives the same bytes; any other value, also with
            # the top bit set, reads back; without the field nothing is read
            assert K.with_crc(p.header, p.crc) == p.header
            for v in (0, 1, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF, p.crc ^ 0x80000000):
                assert K.header_crc(K.with_crc(p.header, v))[0] == v
            bare = K.with_crc(p.header, None)
            assert K.header_crc(bare) == (None, len(bare)) and len(bare) < len(p.header)
        # a chunk rebuilt from its pages is the chunk
        again, dpo = K.join_pages(pages)
        assert again == chunk and dpo == m.data_page_offset - m.start
    assert seen["dict_pages"] == 1 and seen["data_pages"] > 8
    # the same file without checksums carries no field
    plain = pqgpu.ParquetFile(K.write_table(table, version, compression, checksum=False, **kw))
    m = plain.chunk_meta(0, 0)
    chunk = bytes(plain.data[m.start:m.start + m.total_compressed_size])
    assert all(p.crc is None for p in K.split_pages(chunk, P.oracle_chunk(plain, 0, 0).pages))


def test_abi_constants():
    from pqgpu import abi
    import pqgpu
    assert abi.STATUS[-18] == "CRC" and abi.STATUS_CODES["CRC"] == -18
    hdr = open(os.path.join(ROOT, "include", "pqgpu.h")).read()
    assert "PQG_ERR_CRC = -18" in hdr
    L = pqgpu._lib.lib()
    assert L.pqg_status_string(-18) == b"page checksum mismatch"
    import ctypes as C
    assert C.sizeof(abi.PageCrc) == 16
