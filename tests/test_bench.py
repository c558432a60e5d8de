"""bench.py's options beside the timing: --dump-outputs (what the timed learner
holds after its last step, as .npy under a byte budget) and --full (the legs
beside the headline figure).  The GPU cases run the benchmark itself on the
ML-100k-shaped synthetic set, K=8: a fraction of a second of sweeps."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench
from conftest import REPO

HEADLINE_KEYS = {"metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup"}


def test_dump_outputs_small_arrays_whole_large_ones_sampled(tmp_path, monkeypatch):
    """Budget 4 MB: the two 2.4 MB arrays share what the small one leaves, as whole rows at
    sorted sampled positions; a second dump of the same shapes takes the same rows."""
    monkeypatch.setattr(bench, "DUMP_BUDGET", 4_000_000)
    big = np.arange(300_000, dtype=np.float64).reshape(3000, 100)
    vec = np.arange(300_000, dtype=np.float32)
    small = np.array([1.0, np.nan, 3.0])
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"big": big, "vec": vec, "small": small})
    got = {n: np.load(str(tmp_path / "a" / (n + ".npy"))) for n in ("big", "vec", "small")}
    assert all(a.dtype == np.float64 for a in got.values())
    assert np.array_equal(got["small"], small, equal_nan=True)
    total = sum(os.path.getsize(str(tmp_path / "a" / f)) for f in os.listdir(str(tmp_path / "a")))
    assert total <= 4_000_000 + 3 * 128  # payload budget + the .npy headers
    cap = (4_000_000 - small.nbytes) // 2
    assert got["big"].shape == (cap // 800, 100) and got["vec"].shape == (cap // 8,)
    rows = got["big"][:, 0].astype(np.int64) // 100  # row r of `big` starts with 100 r
    assert np.all(np.diff(rows) > 0) and np.array_equal(got["big"], big[rows])
    assert np.all(np.diff(got["vec"]) > 0)
    for n in got:
        assert np.array_equal(got[n], np.load(str(tmp_path / "b" / (n + ".npy"))), equal_nan=True)


def test_dump_outputs_within_budget_is_verbatim(tmp_path):
    a = np.random.default_rng(0).normal(size=(200_000, 2))  # 3.2 MB: above the 1 MB mark, below the budget
    bench.dump_outputs(str(tmp_path), {"a": a})
    assert np.array_equal(np.load(str(tmp_path / "a.npy")), a)


def _bench(tmp_path, *args):
    cmd = [sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--shape", "ml-100k", "--K", "8", *args]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1, r.stdout  # one JSON result line
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_dumps_what_the_timed_learner_holds(tmp_path):
    """--steps sets the timed steps; the plain line carries no extra leg; the dump equals the
    state of a learner configured and driven as bench.py's (1 warm-up call, one 3-sweep run)."""
    from sbmf import Data, FMLearnSBPMF, synth
    out = _bench(tmp_path, "--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path / "dump"))
    assert HEADLINE_KEYS <= set(out) and out["steps"] == 3 and out["warmup"] == 1
    assert out["config"]["sweeps_run"] == 4
    assert out["ms_per_step"] > 0 and out["value"] == pytest.approx(90_000 * 1e3 / out["ms_per_step"], rel=1e-9)
    assert "cpu_baseline" not in out and "f32_value" not in out
    assert out["config"]["time_to_test_rmse_0.85"] == [] and out["config"]["load"] is None
    assert not any("ms_standalone" in b for b in out["roofline"]["bins"].values())
    got = {f[:-4]: np.load(str(tmp_path / "dump" / f)) for f in os.listdir(str(tmp_path / "dump"))}
    assert {"U", "V", "predict", "tau", "sigma_u", "mu_u", "sigma_v", "mu_v", "rmse_avg", "rmse_this"} == set(got)
    assert all(a.dtype == np.float64 for a in got.values())
    train, test, dims = synth.generate("ml-100k")
    L = FMLearnSBPMF(num_factor=8, seed=2015, rng="philox", precision="f64", quirks="final", recompute_every=0,
                     eval_train=False, pipeline=1)
    L.set_data(Data(*train), Data(*test))
    L.learn(sweeps=1)
    L.learn(sweeps=3)
    U, V = L.factors()
    want = dict(L.hyper(), U=U, V=V, predict=L.predict(), rmse_avg=L.rmse_trajectory[-3:],
                rmse_this=[h["rmse_this"] for h in L.history[-3:]])
    L.close()
    assert got["U"].shape == (dims[0], 8) and got["V"].shape == (dims[1], 8) and got["predict"].shape == (10_000,)
    for name, w in want.items():  # the same kernels on the same inputs in the same order: the same bits
        assert np.array_equal(got[name], np.atleast_1d(np.asarray(w, dtype=np.float64))), name
    assert out["config"]["test_rmse_after"] == got["rmse_avg"][-1]


@pytest.mark.gpu
def test_long_run_restarts_the_chain_on_fresh_learners(tmp_path):
    """50 timed sweeps after 3 warm-up ones: no learner runs more than CHAIN_SWEEPS = 24 sweeps,
    so the first times 21, a second 23 after one warm-up sweep, a third the last 6: 3 learners,
    3 + 21 + 1 + 23 + 1 + 6 sweeps.  Every output is finite, each of the 50 timed steps has its
    RMSE, and the dump is the state of a fresh learner after learn(1), learn(6)."""
    from sbmf import Data, FMLearnSBPMF, synth
    assert bench.CHAIN_SWEEPS == 24
    out = _bench(tmp_path, "--steps", "50", "--warmup", "3", "--dump-outputs", str(tmp_path / "dump"))
    assert out["steps"] == 50 and out["config"]["learners"] == 3 and out["config"]["sweeps_run"] == 55
    assert out["ms_per_step"] > 0 and out["value"] == pytest.approx(90_000 * 1e3 / out["ms_per_step"], rel=1e-9)
    got = {f[:-4]: np.load(str(tmp_path / "dump" / f)) for f in os.listdir(str(tmp_path / "dump"))}
    assert all(np.all(np.isfinite(a)) for a in got.values())
    assert got["rmse_avg"].shape == (50,) and got["rmse_this"].shape == (50,)
    train, test, _ = synth.generate("ml-100k")
    L = FMLearnSBPMF(num_factor=8, seed=2015, rng="philox", precision="f64", quirks="final", recompute_every=0,
                     eval_train=False, pipeline=1)
    L.set_data(Data(*train), Data(*test))
    L.learn(sweeps=1)
    L.learn(sweeps=6)
    U, V = L.factors()
    want = dict(L.hyper(), U=U, V=V, predict=L.predict(), rmse_avg_tail=L.rmse_trajectory[-6:])
    L.close()
    assert np.array_equal(got["rmse_avg"][-6:], want.pop("rmse_avg_tail"))
    assert np.array_equal(got["rmse_avg"][21:27], got["rmse_avg"][44:])  # the same chain again: sweeps 1..6
    for name, w in want.items():
        assert np.array_equal(got[name], np.atleast_1d(np.asarray(w, dtype=np.float64))), name


@pytest.mark.gpu
def test_full_run_adds_the_other_legs(tmp_path):
    out = _bench(tmp_path, "--steps", "3", "--warmup", "1", "--full", "--cpu-seconds", "1")
    assert HEADLINE_KEYS <= set(out) and out["steps"] == 3
    assert out["f32_value"] > 0 and out["f32_ms_per_step"] > 0
    assert out["cpu_baseline"]["value"] > 0 and out["cpu_baseline"]["all_cores"]["value"] > 0
    assert [(t["quirks"], t["burnin"]) for t in out["config"]["time_to_test_rmse_0.85"]] == [
        ("final", 0), ("final", 50), ("bias2", 0), ("bias2", 50)]
    assert out["config"]["load"]["n"] == 90_000
    assert any("ms_standalone" in b for b in out["roofline"]["bins"].values())
