"""bench.py's one-line JSON contract on the GPU (the driver parses this line every round):
a short config-2 run in a child process must print exactly one JSON line carrying the
BASELINE metric and the whole-job value; with --full also the roofline object (HIP-event
kernel time against SURVEY §8d bytes) and the cpu_baseline object, with the sampled parity
clean.  A plain run measures nothing besides its steps, and --dump-outputs writes what its
last step computed."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(extra):
    cmd = [sys.executable, os.path.join(REPO, "bench.py"), "--units", "20000", "--steps", "2", "--warmup", "1"] + extra
    r = subprocess.run(cmd, cwd=REPO, capture_output=True, text=True, timeout=110)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip().startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    base = json.load(open(os.path.join(REPO, "BASELINE.json")))
    assert d["metric"] == base["metric"]
    for k in ("value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert k in d, k
    assert d["n_gpus"] == 1 and d["steps"] == 2 and d["warmup"] == 1
    assert d["value"] > 0 and d["ms_per_step"] > 0 and d["higher_is_better"] is True
    assert d["value"] == pytest.approx(20000 * 4608 / (d["ms_per_step"] * 1e-3), rel=1e-9)
    assert "workload" in d["config"]
    return d


@pytest.mark.gpu
def test_bench_json_line_contract():
    d = _run(["--full", "--cpu-seconds", "0.5", "--parity-units", "16", "--no-frames", "--e2e-units", "0"])
    assert d["full"] is True
    roof = d["roofline"]
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert k in roof, k
    assert roof["bound"] == "hbm" and roof["unit"] == "GB/s"
    assert 0 < roof["frac"] < 1 and abs(roof["achieved"] / roof["peak"] - roof["frac"]) < 1e-6
    cpu = d["cpu_baseline"]
    for k in ("value", "unit", "cores", "kind", "sample"):
        assert k in cpu, k
    assert cpu["kind"] in ("port", "reference") and cpu["value"] > 0 and cpu["cores"] >= 1
    assert d["parity"]["mismatches"] == 0 and d["parity"]["units_checked"] > 0


@pytest.mark.gpu
def test_bench_plain_run_and_dump_outputs(tmp_path):
    """Without --full none of the legs runs (their keys are null), and --dump-outputs writes
    the last step's outputs of a seeded sample of units as float .npy files of at most 64 MB
    in all, consistent with one another and with the stream totals of the result line."""
    out = tmp_path / "dump"
    d = _run(["--dump-outputs", str(out)])
    assert d["full"] is False
    for k in ("roofline", "kernels", "cpu_baseline", "frame_writer", "end_to_end", "parity"):
        assert d[k] is None, k
    assert d["stream_stats"]["units"] == 20000 and d["stream_stats"]["samples"] == 20000 * 4608
    assert d["stream_stats"]["errors"] == 0
    files = sorted(p.name for p in out.iterdir())
    assert files == ["meta.npy", "residual.npy", "rice_params.npy", "stream_stats.npy", "units.npy"]
    assert sum(p.stat().st_size for p in out.iterdir()) <= 64 * 1000 * 1000
    a = {p.name[:-4]: np.load(p) for p in out.iterdir()}
    assert all(v.dtype in (np.float32, np.float64) and np.isfinite(v).all() for v in a.values())
    k = len(a["units"])
    assert k > 0 and np.all(np.diff(a["units"]) > 0) and 0 <= a["units"][0] and a["units"][-1] < 20000
    assert a["meta"].shape[0] == a["residual"].shape[0] == a["rice_params"].shape[0] == k
    assert a["residual"].shape[1] >= 4608
    from flac_amd import abi
    cols = [f for f in abi.META_DTYPE.names if f not in ("coefs", "lpc_tiers")]
    m = {f: a["meta"][:, i] for i, f in enumerate(cols)}
    assert np.all(m["status"] == 0)
    assert np.all(m["res_len"] > 0) and np.all(m["res_offset"] + m["res_len"] <= 4608)
    assert np.all(m["n_parts"] == 2 ** m["part_order"])
    assert a["residual"].any() and a["stream_stats"][0] == 20000 and np.all(m["rice_bits"] > 0)
