"""-m gpu: bench.py as it is run from the command line, in a fresh process.  A plain run prints the headline line and nothing that needs a run of
its own; --full adds those legs (here the roofline leg alone: --no-cpu-baseline --no-extras keep it short)."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL_ONLY = ("roofline", "cpu_baseline", "ap_delta", "sustained", "fed", "plugin_api", "v99",
             "split_gemm", "split_direct3x3", "split_gemm_v99", "split_direct3x3_v99")


def _bench(*args):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", *args],
                       cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    lines = p.stdout.decode().strip().splitlines()
    assert len(lines) == 1, lines
    return json.loads(lines[0])


def test_bench_plain_run_is_the_headline_only(dev, tmp_path):
    import numpy as np
    d = _bench("--dump-outputs", str(tmp_path / "dump"))
    assert d["metric"] == "images/sec whole-node (V2-39-eSE 3x800x1280)" and d["unit"] == "images/sec"
    assert d["higher_is_better"] is True and d["dtype"] == "f32" and d["steps"] == 2 and d["warmup"] == 1
    assert d["value"] > 0 and d["ms_per_step"] > 0
    assert abs(d["value"] - 8 * 1e3 / d["ms_per_step"]) <= 1e-2 * d["value"]
    assert not [k for k in FULL_ONLY if k in d]
    arrays = d["dump_outputs"]["arrays"]
    assert "records" in arrays and "counts" in arrays
    for name, shape in arrays.items():
        assert list(np.load(str(tmp_path / "dump" / (name + ".npy"))).shape) == shape, name


def test_bench_full_adds_the_roofline_leg(dev):
    d = _bench("--full", "--no-cpu-baseline", "--no-extras")
    assert d["value"] > 0 and d["ms_per_step"] > 0
    assert d["roofline"]["kernel"] in d["roofline"]["per_kernel"] and d["roofline"]["frac"] > 0
    assert not [k for k in FULL_ONLY if k in d and k != "roofline"]
