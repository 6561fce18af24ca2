"""The Zstandard decoder of pqg_zstd.h on the host (tools/zstd_model.cpp: the
parsers, table builds, repeat-offset rule and XXH64 that k_zstd runs) against
libzstd, reached through pyarrow.Codec('zstd'): a corpus at six levels that
passes through every feature of the format its encoder emits, hand-built
frames, the shapes at which lanes and batches can go wrong, 2 000 seeded
mutations (the verdict must be libzstd's), and the same run under
AddressSanitizer / UBSan as a stand-alone program."""
import numpy as np
import pytest

import zstd_util as Z
from pqgpu import abi

pa = pytest.importorskip("pyarrow")


@pytest.fixture(scope="module")
def corpus_runs():
    """(name, level) -> model result, over the corpus x levels."""
    out = {}
    for name, raw in Z.corpus().items():
        for lvl in Z.LEVELS:
            out[(name, lvl)] = Z.model(Z.compress(raw, lvl))
    return out


def test_model_corpus_roundtrip(corpus_runs):
    c = Z.corpus()
    want = {name: Z.fnv(raw) for name, raw in c.items()}
    for (name, lvl), r in corpus_runs.items():
        assert r["status"] == 0, (name, lvl, r["status"])
        assert r["len"] == len(c[name]) and r["fnv"] == want[name] and r["bytes"] == c[name], (name, lvl)


@pytest.mark.parametrize("cell", Z.CELLS)
def test_model_corpus_covers(corpus_runs, cell):
    """libzstd's encoder reaches every cell of the format on this corpus: a
    libzstd that stops emitting one fails here by name."""
    assert sum(r[cell] for r in corpus_runs.values()) > 0, cell


def test_model_rare_cells_where_expected(corpus_runs):
    assert corpus_runs[("rle_literals", 19)]["lit_rle"] or corpus_runs[("rle_literals", 22)]["lit_rle"]
    assert corpus_runs[("three_symbols", 3)]["huf_direct"]
    assert corpus_runs[("tokens", 19)]["seq_long"] or corpus_runs[("tokens", 22)]["seq_long"]
    assert corpus_runs[("arange", 19)]["ll_rle"] and corpus_runs[("arange", 1)]["of_rle"]


@pytest.mark.parametrize("name", sorted(Z.hand_frames().keys()))
def test_model_hand_frames(name):
    z, content = Z.hand_frames()[name]
    ref = Z.libzstd(z, len(content))
    r = Z.model(z, cap=len(content))
    mine = r["bytes"] if r["status"] == 0 and r["len"] == len(content) else None
    assert mine == ref, (name, r["status"], r["len"], None if ref is None else len(ref))
    if ref is None:
        assert r["status"] in (abi.STATUS_CODES["ZSTD"], 0)
    else:
        assert ref == content
    invalid = {"checksum_bad", "dict_id", "reserved_bit", "block_type3", "fcs_mismatch", "window_too_large", "trailing1",
               "trailing2", "trailing3", "truncated_header", "truncated_block", "bad_magic"}
    # libzstd's own verdicts, pinned: raw blocks past 128 KiB and a dictionary ID of 0 decode
    assert (ref is None) == (name in invalid), name


def test_model_checksum_counter():
    z, content = Z.hand_frames()["checksum_ok"]
    r = Z.model(z)
    assert r["frame_checksum"] == 1 and r["bytes"] == content
    z, content = Z.hand_frames()["skip_between"]
    assert Z.model(z)["frame_skip"] == 1


@pytest.mark.parametrize("name", sorted(Z.lane_shapes().keys()))
def test_model_lane_shapes(name):
    raw = Z.lane_shapes()[name]
    r = Z.model(Z.compress(raw, 3))
    assert r["status"] == 0 and r["bytes"] == raw
    if name.startswith("lits"):
        # no sequences: every byte is a literal, four Huffman streams with a ragged fourth
        assert r["lit_bytes"] == len(raw) and r["lit_huf4"] == 1 and r["seqs"] == [0]
    if name.startswith("overlap"):
        assert r["match_overlap"] >= 1


@pytest.mark.parametrize("want", [63, 64, 65, 127, 128, 129])
def test_model_sequence_counts(want):
    z, raw = Z.seq_count_frame(want)
    r = Z.model(z)
    assert r["status"] == 0 and r["bytes"] == raw and r["seqs"] == [want]


def test_model_mutations_match_libzstd():
    """2 000 single-byte and truncation mutations of five frames: ok with
    identical bytes, or both fail.  libzstd's laxities that show here, and that
    the model follows: Huffman streams decoded by its fast loop (four streams
    of >= 8 bytes each) need not be consumed exactly."""
    frames = Z.mutation_frames()
    assert all(len(raw) <= 8192 for raw, _ in frames)
    muts = Z.mutations(2000, frames)
    res, _ = Z.model_corpus([(len(frames[f][0]), z) for f, z in muts])
    bad, n_ok = [], 0
    for i, ((f, z), (rc, ln, h)) in enumerate(zip(muts, res)):
        ref = Z.libzstd(z, len(frames[f][0]))
        mine_ok = rc == 0 and ln == len(frames[f][0])
        n_ok += ref is not None
        if (ref is not None) != mine_ok or (mine_ok and Z.fnv(ref) != h):
            bad.append((i, f, rc, ln, ref is not None))
    assert not bad, bad[:10]
    assert 50 < n_ok < 1950  # both verdicts occur


def test_model_sanitizer_clean():
    """The model built with -fsanitize=address,undefined (a stand-alone
    program) over the mutation corpus and the hand-built frames."""
    frames = Z.mutation_frames()
    cases = [(len(frames[f][0]), z) for f, z in Z.mutations(2000, frames)]
    cases += [(len(content), z) for z, content in Z.hand_frames().values()]
    cases += [(0, z) for _, z in frames]  # no room at all
    res, err = Z.model_corpus(cases, sanitize=True)
    assert len(res) == len(cases)
    assert "Sanitizer" not in err and "runtime error" not in err, err[-3000:]


def test_abi_constants():
    import pqgpu
    assert abi.CODEC_ZSTD == 6
    assert abi.STATUS[-16] == "ZSTD" and abi.STATUS_CODES["ZSTD"] == -16
    hdr = open(Z.os.path.join(Z.ROOT, "include", "pqgpu.h")).read()
    assert "PQG_CODEC_ZSTD = 6" in hdr and "PQG_ERR_ZSTD = -16" in hdr
    L = pqgpu._lib.lib()
    import ctypes as C
    L.pqg_status_string.restype = C.c_char_p
    assert b"zstd" in L.pqg_status_string(-16)
