"""bench.py command-line contract: --dump-outputs writes what the timed
path returned in its last step, --full gates the secondary
measurements, --steps sets the number of timed steps."""
import importlib.util
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from tfservingcache_amd.wire import messages as m
from tfservingcache_amd.wire.tensor import numpy_to_tensorproto

REPO = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def bench():
    spec = importlib.util.spec_from_file_location("tfsc_bench",
                                                  REPO / "bench.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _resp(value, shape=(2, 5)):
    return m.PredictResponse(outputs={
        "probs": numpy_to_tensorproto(np.full(shape, value, np.float32))})


def test_dump_outputs_request_order_and_dtype(bench, tmp_path):
    # captured out of order, half as decoded messages and half as bytes
    captured = {}
    for i in (7, 3, 5, 4, 6):
        r = _resp(float(i))
        captured[i] = r if i % 2 else r.encode()
    bench._dump_outputs(str(tmp_path), captured, "native", 0, 1)
    arr = np.load(tmp_path / "probs.npy")
    assert arr.dtype == np.float32 and arr.shape == (5, 2, 5)
    assert arr[:, 0, 0].tolist() == [3.0, 4.0, 5.0, 6.0, 7.0]


def test_dump_outputs_rest_bodies(bench, tmp_path):
    captured = {i: json.dumps({"predictions": [[i, 2.5]]}).encode()
                for i in range(3)}
    bench._dump_outputs(str(tmp_path), captured, "native-rest", 0, 1)
    arr = np.load(tmp_path / "predictions.npy")
    # JSON numbers decode as doubles and are kept as such
    assert arr.dtype == np.float64 and arr.shape == (3, 1, 2)
    assert arr[:, 0, 0].tolist() == [0.0, 1.0, 2.0]


def test_dump_outputs_size_cap_is_seeded_sample(bench, tmp_path,
                                                monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BYTES_MAX", 64)
    full = np.arange(40, dtype=np.float32).reshape(4, 10)
    captured = {i: m.PredictResponse(outputs={
        "x": numpy_to_tensorproto(full[i])}) for i in range(4)}
    bench._dump_outputs(str(tmp_path / "a"), captured, "inproc", 0, 1)
    bench._dump_outputs(str(tmp_path / "b"), captured, "inproc", 0, 1)
    a = np.load(tmp_path / "a" / "x.npy")
    b = np.load(tmp_path / "b" / "x.npy")
    assert a.nbytes <= 64 and a.size == 16
    assert np.array_equal(a, b)                 # same sample every run
    assert np.isin(a, full).all()


@pytest.mark.gpu
def test_bench_plain_run_dumps_last_step(tmp_path):
    out = tmp_path / "dump"
    run = subprocess.run(
        [sys.executable, str(REPO / "bench.py"), "--gpus", "1",
         "--steps", "2", "--warmup", "1", "--models", "12",
         "--pool-size", "3", "--image-size", "64", "--batch", "2",
         "--dump-outputs", str(out)],
        capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stderr[-3000:]
    res = json.loads(run.stdout.strip().splitlines()[-1])
    for key in ("metric", "value", "unit", "higher_is_better", "dtype",
                "ms_per_step"):
        assert key in res, key
    assert res["steps"] == 2 and res["ms_per_step"] > 0
    # value and ms_per_step describe the same 2 timed steps
    reqs = 2 * res["config"]["requests_per_step"]
    assert res["value"] == pytest.approx(
        reqs / (2 * res["ms_per_step"] / 1e3), rel=1e-3)
    # plain run: the warm-cache half is behind --full
    assert res["config"]["full"] is False
    assert res["config"]["warm_req_per_sec"] is None
    probs = np.load(out / "probs.npy")
    assert probs.dtype == np.float32
    assert probs.shape == (res["config"]["requests_per_step"], 2, 1000)
    assert np.isfinite(probs).all()
    # bf16 softmax rows sum to 1 within bf16 rounding of 1000 terms
    assert np.abs(probs.sum(-1) - 1.0).max() < 0.05
