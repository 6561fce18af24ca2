"""K2 snappy (decode_other.go:14-101) through pqg_block_decompress, on streams
built tag by tag so that every tag form and every hard case of the batched
decoder is present: literal headers 60..63, copy-1/2/4, overlapping
(run-length) copies, copies chained inside one batch, copies reaching past
the LDS history ring into L2, long literals crossing batches, blocks ending
mid-batch — plus corruptions.  The expected output is the oracle's
(oracle/pq_oracle.cpp pqo_snappy_decode) and, for valid streams, the
plaintext the generator tracked.  The generator itself is checked on CPU
against the oracle and pyarrow's snappy."""
import ctypes as C

import numpy as np
import pytest

from oracle import pyoracle as O
from pqgpu import abi
from snappy_build import copy, lit, stream, uvarint


def cases():
    rng = np.random.default_rng(11)
    cs = [stream(rng, 300_000), stream(rng, 120_000, far_frac=0.5), stream(rng, 70_000, lit_max=8),
          stream(rng, 5000), stream(rng, 40, lit_max=3)]
    # long literals (>= one batch) at every header size, then copies back into them
    big = rng.integers(0, 256, 70_000, dtype=np.uint8).tobytes()
    cs.append((uvarint(70_000 + 64 + 30) + lit(big) + copy(65535, 64, 2) + copy(69_000, 30, 4), None))
    cs.append((uvarint(3000) + lit(big[:1]) + copy(1, 64, 2) * 46 + copy(1, 55, 2), None))  # run-length chain
    cs.append((uvarint(1) + lit(b"q"), None))
    return cs


def test_generator_matches_oracle_and_pyarrow():
    import pyarrow as pa
    for src, plain in cases():
        rc, out = O.snappy_decode(src)
        assert rc == 0
        if plain is not None:
            assert out == plain
        assert pa.decompress(src, decompressed_size=len(out), codec="snappy").to_pybytes() == out


def _gpu(dec, src, cap=1 << 21):
    dst = np.zeros(cap, np.uint8)
    n = C.c_int64(0)
    rc = dec.L.pqg_block_decompress(dec.ctx, abi.CODEC_SNAPPY, src, len(src), dst.ctypes.data, cap, C.byref(n))
    return rc, dst[:n.value].tobytes()


@pytest.fixture(scope="module")
def dec():
    import pqgpu
    d = pqgpu.GpuDecoder(0)
    yield d
    d.close()


@pytest.mark.gpu
def test_snappy_tag_forms(dec):
    for src, plain in cases():
        rc, got = _gpu(dec, src)
        rc_o, exp = O.snappy_decode(src)
        assert rc == 0 and got == exp


BAD = [uvarint(10) + copy(1, 4, 1),                      # copy before any output
       uvarint(10) + lit(b"abc") + copy(4, 4, 1),        # offset > d
       uvarint(5) + lit(b"abc") + copy(1, 5, 2),         # past the declared length
       uvarint(10) + lit(b"abc"),                        # short output
       uvarint(3) + bytes([61 << 2, 2]),                 # truncated literal header
       uvarint(3) + bytes([8]) + b"ab",                  # literal past the block end
       uvarint(4) + lit(b"ab") + copy(0, 2, 2),          # zero offset
       uvarint(2) + lit(b"ab") + bytes([3])]             # truncated copy-4


def mutants():
    """60 seeded mutations (a changed byte, a truncation, an inserted byte) of each of two random streams."""
    rng = np.random.default_rng(12)
    base = [stream(rng, 20_000)[0], stream(rng, 3000, lit_max=5)[0]]
    out = []
    for s in base:
        for _ in range(60):
            m = bytearray(s)
            k = int(rng.integers(0, 3))
            if k == 0:
                i = int(rng.integers(len(uvarint(0)), len(m)))
                m[i] = int(rng.integers(0, 256))
            elif k == 1:
                m = m[:int(rng.integers(1, len(m)))]
            else:
                i = int(rng.integers(3, len(m)))
                m[i:i] = bytes([int(rng.integers(0, 256))])
            out.append((k, bytes(m)))
    return out


def oracle_decodes():
    """How many of the mutants the oracle alone decodes."""
    return sum(1 for _, m in mutants() if O.snappy_decode(m)[0] == 0)


def test_mutants_have_both_verdicts():
    n = len(mutants())
    assert n // 20 <= oracle_decodes() <= n - n // 20


@pytest.mark.gpu
def test_snappy_corruptions(dec):
    """Byte flips, truncations and bad offsets: the GPU and the oracle agree on
    success/failure (on the hand-written ones, on the status) and, on success,
    on every byte."""
    n = 0
    for s in BAD:
        rc, _ = _gpu(dec, s)
        rc_o = O.snappy_decode(s)[0]
        assert rc != 0 and rc == rc_o, (s, rc, rc_o)
    for k, m in mutants():
        rc, got = _gpu(dec, m)
        rc_o, exp = O.snappy_decode(m)
        assert (rc == 0) == (rc_o == 0), (k, rc, rc_o)
        if rc == 0:
            assert got == exp
            n += 1
    assert n == oracle_decodes()
