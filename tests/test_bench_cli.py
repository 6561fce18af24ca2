"""bench.py's command line: a plain run times the headline and nothing else,
--dump-outputs writes the timed path's last outputs, and the threaded C2
generation writes the files the one-thread generation writes."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench
from gen import pqwrite as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_c2_family_workers_write_the_same_files():
    for rh in (False, True):
        one = list(W.config_c2_family(rows=50_000, bits_list=(1, 4, 12), seed=3, run_heavy=rh))
        par = list(W.config_c2_family(rows=50_000, bits_list=(1, 4, 12), seed=3, run_heavy=rh, workers=3))
        assert [b for b, _, _ in par] == [1, 4, 12]
        for (_, d1, (l1, v1)), (_, d2, (l2, v2)) in zip(one, par):
            assert d1 == d2
            assert np.array_equal(l1, l2) and np.array_equal(v1, v2)


class _HostDecoder:
    """dump_outputs' view of a decoder, over host arrays."""

    def d2h(self, ptr, nbytes, dtype=np.uint8):
        return np.frombuffer(C.string_at(ptr, nbytes), dtype=np.uint8).view(dtype).copy()


def _fake_chunk(defs, vals):
    import pqgpu
    from pqgpu import abi
    data, _ = W.config_c2(rows=100, bits=1)
    r = abi.ChunkResult()
    r.status, r.value_width = 0, 4
    r.num_slots, r.num_values, r.values_bytes = len(defs), len(vals), vals.nbytes
    r.def_levels, r.values = defs.ctypes.data, vals.ctypes.data
    return bench.Workload("c2", "", [(pqgpu.ParquetFile(data), [(0, 0)], None)], "int32"), [r]


def test_dump_outputs_whole_and_sampled(tmp_path, monkeypatch):
    rng = np.random.default_rng(5)
    defs = (rng.random(300_000) >= 0.1).astype(np.uint8)
    vals = rng.integers(-2**31, 2**31 - 1, size=int(defs.sum()), dtype=np.int64).astype(np.int32)
    wl, res = _fake_chunk(defs, vals)
    bench.dump_outputs(wl, _HostDecoder(), res, str(tmp_path / "whole"))
    got = {f[:-4]: np.load(str(tmp_path / "whole" / f)) for f in os.listdir(str(tmp_path / "whole"))}
    assert sorted(got) == ["chunk00_def_levels", "chunk00_shape", "chunk00_values"]
    assert got["chunk00_shape"].tolist() == [0, len(defs), len(vals), vals.nbytes]
    assert got["chunk00_def_levels"].dtype == np.float32 and np.array_equal(got["chunk00_def_levels"], defs)
    assert got["chunk00_values"].dtype == np.float64 and np.array_equal(got["chunk00_values"], vals)

    monkeypatch.setattr(bench, "DUMP_BUDGET", 2 * (bench.DUMP_BLOCKS * 8 + 80_000))
    for d in ("a", "b"):
        bench.dump_outputs(wl, _HostDecoder(), res, str(tmp_path / d))
    files = sorted(os.listdir(str(tmp_path / "a")))
    assert files == sorted(os.listdir(str(tmp_path / "b")))
    assert "chunk00_values_blocksum.npy" in files and "chunk00_def_levels_blocksum.npy" in files
    total = 0
    for f in files:
        a, b = np.load(str(tmp_path / "a" / f)), np.load(str(tmp_path / "b" / f))
        assert np.array_equal(a, b)
        total += a.nbytes
    assert total <= 2 * (bench.DUMP_BLOCKS * 8 + 80_000) + 4 * 8
    s = np.load(str(tmp_path / "a" / "chunk00_values.npy"))
    assert len(s) == 10_000
    idx = np.sort(np.random.default_rng(0).integers(0, len(vals), size=10_000))
    assert np.array_equal(s, vals[idx])
    bs = np.load(str(tmp_path / "a" / "chunk00_values_blocksum.npy"))
    assert 1 < len(bs) <= bench.DUMP_BLOCKS and bs.sum() == vals.astype(np.float64).sum()
    # one changed element shows in its block's sum
    vals[123_456] ^= 1
    bench.dump_outputs(wl, _HostDecoder(), res, str(tmp_path / "c"))
    assert (np.load(str(tmp_path / "c" / "chunk00_values_blocksum.npy")) != bs).sum() == 1


@pytest.mark.gpu
def test_plain_run_line_and_dump(tmp_path):
    """A plain run at a small size: the line holds the headline's fields and
    none of --full's, `steps` timed steps, and the dumped arrays are the
    generator's."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                          "--rows", "60000", "--bits", "1,12", "--dump-outputs", str(tmp_path / "out")],
                         capture_output=True, text=True, timeout=120, env=env, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [x for x in out.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == 1
    line = json.loads(lines[0])
    assert line["metric"] == bench.METRIC and line["unit"] == "GB/s" and line["higher_is_better"] is True
    assert line["dtype"] == "int32" and line["steps"] == 3 and line["n_gpus"] == 1
    assert line["ms_per_step"] > 0 and line["value"] > 0
    # value and ms_per_step are the same measurement (both rounded, to 1e-3 GB/s and 1e-4 ms)
    gbs = line["config"]["bytes_out"] / (line["ms_per_step"] * 1e-3) / 1e9
    assert abs(line["value"] - gbs) <= 1e-2 * line["value"]
    for k in ("roofline", "cpu_baseline", "cpu_baseline_all_cores", "verified_bit_exact", "k8_assemble", "configs"):
        assert k not in line
    b_out = 0
    for i, (_, _, (defs, vals)) in enumerate(W.config_c2_family(rows=60000, bits_list=(1, 12), seed=2)):
        assert np.array_equal(np.load(str(tmp_path / "out" / ("chunk%02d_def_levels.npy" % i))), defs)
        v = np.load(str(tmp_path / "out" / ("chunk%02d_values.npy" % i)))
        assert v.dtype == np.float64 and np.array_equal(v, vals)
        b_out += len(defs) + vals.nbytes
    assert line["config"]["bytes_out"] == b_out
