"""The general libFM MCMC / ALS learner (csrc/fmg.hip + fmg.cpp: cases with any number of
features, exact by ranges) on the GPU, against
  1. libFM itself, compiled from its own sources, on the four-field set fm4
     (tests/golden/ref_libfm_*_fm4_*, written by tests/make_fm_golden.py),
  2. the pinned oracle on the two-attribute sets, sent through the general learner,
  3. a serial numpy restatement of libFM's ALS in float64 and longdouble,
and for what the design promises: ranges are exact (bit for bit against one attribute per
launch), chunked long rows agree with unchunked ones, reruns are bit-identical, nothing leaks."""
import gzip
import os
import subprocess

import numpy as np
import pytest

import fm_cases
import oracle
from conftest import GOLD, gpu_available
from sbmf import Cases, Data, FMLearnSBPMF, SBMFError, device_usage
from sbmf._lib import CLI_PATH, SBMF_E_STATE
from test_gpu_libfm import _within_printed
from test_oracle_libfm import RUNS, golden_name

pytestmark = pytest.mark.gpu

FM4_RUNS = [("mcmc", (0.0, 0.0, 0.0)), ("als", (0.0, 0.0, 10.0))]


def _learner(method, regular, K=8, seed=1, rng="ref"):
    return FMLearnSBPMF(num_factor=K, seed=seed, rng=rng, method="als" if method == "als" else "mcmc", order="libfm",
                        k0=1, k1=1, regular=regular, init_stdev=0.1)


def _run(train, test, method, regular, iters, K=8, seed=1, rng="ref"):
    L = _learner(method, regular, K, seed, rng)
    L.set_data(train, test)
    L.learn(sweeps=iters)
    return L


def _golden(method):
    name = "ref_libfm_%s_fm4_d118_s1_i10" % method
    with open(os.path.join(GOLD, name + ".txt")) as f:
        lines = f.read().splitlines()
    with gzip.open(os.path.join(GOLD, name + "_pred.txt.gz"), "rt") as f:
        pred = np.array([float(x) for x in f.read().split()])
    train = [float(l.split("Train=")[1].split()[0]) for l in lines]
    test = [float(l.split("Test=")[1]) for l in lines]
    return lines, train, test, pred


# ---- 1. against libFM
@pytest.mark.parametrize("method,regular", FM4_RUNS, ids=["mcmc", "als"])
def test_fm4_python_matches_libfm(method, regular, ml100k):
    assert gpu_available()
    tr, te = fm_cases.fm4(ml100k)[:2]
    L = _run(tr, te, method, regular, 10)
    _, ref_train, ref_test, ref_pred = _golden(method)
    train = [h["rmse_train"] for h in L.history]
    test = [h["rmse_avg"] for h in L.history]
    print("train", train, "\ntest", test)
    assert _within_printed(train, ref_train) and _within_printed(test, ref_test)
    pred = L.predict()
    assert pred.shape == ref_pred.shape and _within_printed(pred, ref_pred)
    info = L.fm_info()
    assert info["num_attr"] == max(tr.num_attr, te.num_attr) + 1 and info["nranges"] == 8
    L.close()


@pytest.mark.parametrize("method,regular", FM4_RUNS, ids=["mcmc", "als"])
def test_fm4_cli_matches_libfm(method, regular, ml100k, tmp_path):
    assert gpu_available()
    trf, tef = fm_cases.write_fm4(ml100k, tmp_path)
    cmd = [CLI_PATH, "-task", "r", "-train", trf, "-test", tef, "-dim", "1,1,8", "-iter", "10", "-method", method,
           "-out", "pred.txt"]
    if method == "als":
        cmd += ["-regular", "0,0,10"]
    r = subprocess.run(cmd, cwd=str(tmp_path), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    lines = [l for l in r.stdout.splitlines() if l.startswith("#Iter=")]
    ref_lines, _, _, ref_pred = _golden(method)
    assert lines == ref_lines
    pred = np.array([float(x) for x in open(os.path.join(str(tmp_path), "pred.txt")).read().split()])
    assert pred.shape == ref_pred.shape and _within_printed(pred, ref_pred)
    assert "#attributes=" in r.stdout and "#ranges=8" in r.stdout


# ---- 2. the two-attribute sets through the general learner, against the pinned oracle
@pytest.mark.parametrize("run", RUNS, ids=[golden_name(*r[:5]) for r in RUNS])
def test_general_learner_matches_oracle_on_two_attribute_sets(run, ml100k, ragged, monkeypatch):
    assert gpu_available()
    method, dname, dim, seed, iters, reg = run
    tr, te = ml100k if dname == "ml100k" else ragged
    k0, k1, K = (int(x) for x in dim.split(","))
    regular = tuple(float(x) for x in reg.split(",")) if reg else (0.0, 0.0, 0.0)
    monkeypatch.setenv("SBMF_FMM_GENERAL", "1")
    L = FMLearnSBPMF(num_factor=K, seed=seed, method="als" if method == "als" else "mcmc", order="libfm", k0=k0,
                     k1=k1, regular=regular, init_stdev=0.1)
    L.set_data(Data(*tr), Data(*te))
    L.learn(sweeps=iters)
    monkeypatch.delenv("SBMF_FMM_GENERAL")
    assert L.fm_info()["nranges"] == 2
    o = oracle.run_fmm(tr, te, K=K, iters=iters, seed=seed, method=method, k0=k0, k1=k1, regular=regular)
    np.testing.assert_allclose([h["rmse_train"] for h in L.history], o["rmse_train"], rtol=1e-9, atol=0)
    np.testing.assert_allclose([h["rmse_avg"] for h in L.history], o["rmse_test"], rtol=1e-9, atol=0)
    U, V = L.factors()
    I = U.shape[0]
    np.testing.assert_allclose(U, o["v"][:, :I].T, rtol=0, atol=1e-8)
    np.testing.assert_allclose(V, o["v"][:, I:I + V.shape[0]].T, rtol=0, atol=1e-8)
    if k1:
        bu, bv, b0 = L.biases()
        np.testing.assert_allclose(np.concatenate([bu, bv]), o["w"][:len(bu) + len(bv)], rtol=0, atol=1e-8)
        assert abs(b0 - o["w0"]) <= 1e-8
    np.testing.assert_allclose(L.predict(), o["pred"], rtol=0, atol=1e-9)
    L.close()


# ---- 3. ALS against a serial restatement (float64, and longdouble for the restatement's own error)
_RESTATED = {}


def _restated(key, tr, te, K, seed, regular, record):
    if key not in _RESTATED:
        a = fm_cases.als_restatement(tr, te, K, max(record), seed, regular, np.float64, record=record)
        b = fm_cases.als_restatement(tr, te, K, max(record), seed, regular, np.longdouble, record=record)
        _RESTATED[key] = (a, b)
    return _RESTATED[key]


def _check_against_restatement(L, it, a, b):
    """Tolerance: the larger of the bars the project holds the two-attribute learner to (RMSE rtol
    1e-9, w / v atol 1e-8, predictions atol 1e-9) and 64 x the float64-longdouble gap of the
    restatement itself."""
    w0, w, v = L.fm()
    (aw0, aw, av, arm, apt), (bw0, bw, bv, brm, bpt) = a[it], b[it]
    gap = lambda x, y: float(np.max(np.abs(np.asarray(x, np.longdouble) - np.asarray(y, np.longdouble)))) if np.size(x) else 0.0
    g_w, g_v, g_p, g_r = max(gap(aw, bw), gap(aw0, bw0)), gap(av, bv), gap(apt, bpt), gap(arm, brm)
    print("iteration %d: f64-longdouble gap w %.3g v %.3g pred %.3g rmse %.3g; |gpu - f64| w %.3g v %.3g pred %.3g "
          "rmse %.3g" % (it, g_w, g_v, g_p, g_r, gap(w, aw), gap(v, av), gap(L.predict(), apt),
                         abs(L.history[-1]["rmse_train"] - float(arm))))
    assert abs(w0 - float(aw0)) <= max(1e-8, 64 * g_w)
    assert gap(w, aw) <= max(1e-8, 64 * g_w)
    assert gap(v, av) <= max(1e-8, 64 * g_v)
    assert gap(L.predict(), apt) <= max(1e-9, 64 * g_p)
    assert abs(L.history[-1]["rmse_train"] - float(arm)) <= max(1e-9 * float(arm), 64 * g_r)


def test_als_matches_serial_restatement_fm4(ml100k):
    assert gpu_available()
    tr, te = fm_cases.fm4(ml100k)[:2]
    a, b = _restated("fm4", tr, te, 8, 1, (0.0, 0.0, 10.0), (1, 2, 5))
    L = _learner("als", (0.0, 0.0, 10.0))
    L.set_data(tr, te)
    done = 0
    for it in (1, 2, 5):
        L.learn(sweeps=it - done)
        done = it
        _check_against_restatement(L, it, a, b)
    L.close()


def test_als_matches_serial_restatement_small():
    assert gpu_available()
    tr, te = fm_cases.small_cases()
    a, b = _restated("small", tr, te, 4, 3, (1.0, 2.0, 5.0), (1, 2, 5))
    L = _learner("als", (1.0, 2.0, 5.0), K=4, seed=3)
    L.set_data(tr, te)
    done = 0
    for it in (1, 2, 5):
        L.learn(sweeps=it - done)
        done = it
        _check_against_restatement(L, it, a, b)
    L.close()


# ---- 4. ranges are exact: one attribute per launch (libFM's loop, literally) gives the same bits
@pytest.mark.parametrize("method,rng", [("mcmc", "ref"), ("mcmc", "philox"), ("als", "ref")],
                         ids=["mcmc-ref", "mcmc-philox", "als"])
def test_ranges_are_exact(method, rng, ml100k, monkeypatch):
    assert gpu_available()
    tr, te = fm_cases.fm4(ml100k)[:2]
    regular = (0.0, 0.0, 10.0) if method == "als" else (0.0, 0.0, 0.0)
    A = _run(tr, te, method, regular, 3, rng=rng)
    monkeypatch.setenv("SBMF_FMG_SERIAL", "1")
    B = _run(tr, te, method, regular, 3, rng=rng)
    monkeypatch.delenv("SBMF_FMG_SERIAL")
    assert B.fm_info()["nranges"] == B.fm_info()["num_attr"] and A.fm_info()["nranges"] == 8
    (aw0, aw, av), (bw0, bw, bv) = A.fm(), B.fm()
    assert aw0 == bw0 and np.array_equal(aw, bw) and np.array_equal(av, bv)
    assert np.array_equal(A.predict(), B.predict())
    assert [h["rmse_train"] for h in A.history] == [h["rmse_train"] for h in B.history]
    A.close()
    B.close()


# ---- 5. chunk edges
@pytest.mark.parametrize("method", ["mcmc", "als"])
def test_chunked_long_rows_agree_with_unchunked(method, ml100k, monkeypatch):
    """fm4's field C rows (about 11 k cases) and tag rows run in chunks by default; with
    SBMF_FMM_LONG=256 / SBMF_FMM_CHUNK=64 so do the users and items above 256 cases.  Against
    the same chain with the chunks off (every long row on one 1024-thread workgroup)."""
    assert gpu_available()
    tr, te = fm_cases.fm4(ml100k)[:2]
    regular = (0.0, 0.0, 10.0) if method == "als" else (0.0, 0.0, 0.0)
    monkeypatch.setenv("SBMF_FMM_CHUNK", "0")
    A = _run(tr, te, method, regular, 5)
    monkeypatch.setenv("SBMF_FMM_LONG", "256")
    monkeypatch.setenv("SBMF_FMM_CHUNK", "64")
    B = _run(tr, te, method, regular, 5)
    monkeypatch.delenv("SBMF_FMM_LONG")
    monkeypatch.delenv("SBMF_FMM_CHUNK")
    assert B.fm_info()["launches_per_iter"] > A.fm_info()["launches_per_iter"]
    np.testing.assert_allclose([h["rmse_train"] for h in B.history], [h["rmse_train"] for h in A.history], rtol=1e-9)
    np.testing.assert_allclose([h["rmse_avg"] for h in B.history], [h["rmse_avg"] for h in A.history], rtol=1e-9)
    (aw0, aw, av), (bw0, bw, bv) = A.fm(), B.fm()
    assert abs(aw0 - bw0) <= 1e-8
    np.testing.assert_allclose(bw, aw, rtol=0, atol=1e-8)
    np.testing.assert_allclose(bv, av, rtol=0, atol=1e-8)
    np.testing.assert_allclose(B.predict(), A.predict(), rtol=0, atol=1e-9)
    A.close()
    B.close()


def test_row_lengths_at_every_edge_match_restatement(monkeypatch):
    assert gpu_available()
    tr, te = fm_cases.edge_set()
    assert sorted(np.bincount(tr.attr, minlength=9)[:9].tolist()) == sorted(fm_cases.EDGE_LENGTHS)
    a, b = _restated("edge", tr, te, 4, 2, (0.5, 1.0, 4.0), (1, 2, 5))
    monkeypatch.setenv("SBMF_FMM_LONG", "256")
    monkeypatch.setenv("SBMF_FMM_CHUNK", "64")
    L = _learner("als", (0.5, 1.0, 4.0), K=4, seed=2)
    L.set_data(tr, te)
    monkeypatch.delenv("SBMF_FMM_LONG")
    monkeypatch.delenv("SBMF_FMM_CHUNK")
    done = 0
    for it in (1, 2, 5):
        L.learn(sweeps=it - done)
        done = it
        _check_against_restatement(L, it, a, b)
    L.close()


# ---- 6. rerun and resources
def test_rerun_is_bit_identical_and_nothing_leaks(ml100k):
    assert gpu_available()
    tr, te = fm_cases.fm4(ml100k)[:2]
    before = device_usage()
    runs = []
    for _ in range(2):
        L = _run(tr, te, "mcmc", (0.0, 0.0, 0.0), 3, rng="philox")
        runs.append((L.fm(), L.predict(), [h["rmse_avg"] for h in L.history]))
        assert device_usage()["dev_allocs"] > before["dev_allocs"]
        L.close()
    (w0a, wa, va), pa, ha = runs[0]
    (w0b, wb, vb), pb, hb = runs[1]
    assert w0a == w0b and np.array_equal(wa, wb) and np.array_equal(va, vb) and np.array_equal(pa, pb) and ha == hb
    after = device_usage()
    for k in ("dev_bytes", "dev_allocs", "pinned_bytes", "pinned_allocs", "streams", "events", "contexts", "comms"):
        assert after[k] == before[k], (k, before[k], after[k])


# ---- 7. the two-attribute path is untouched, and the interfaces refuse what they do not offer
def test_two_feature_sets_take_the_two_attribute_learner(ml100k):
    assert gpu_available()
    tr, te = ml100k
    L = FMLearnSBPMF(num_factor=4, seed=1, method="mcmc", order="libfm", init_stdev=0.1)
    L.set_data(Data(*tr), Data(*te))
    L.learn(sweeps=1)
    with pytest.raises(SBMFError) as e:
        L.fm_info()
    assert e.value.code == SBMF_E_STATE
    with pytest.raises(SBMFError) as e:
        L.fm()
    assert e.value.code == SBMF_E_STATE
    L.close()


def test_cases_context_refuses_user_item_readers_and_other_methods(ml100k):
    assert gpu_available()
    tr, te = fm_cases.small_cases()
    L = _learner("als", (1.0, 2.0, 5.0), K=4)
    L.set_data(tr, te)
    L.learn(sweeps=1)
    for fn in (L.factors, L.biases):
        with pytest.raises(SBMFError) as e:
            fn()
        assert e.value.code == SBMF_E_STATE and "sbmf_get_fm" in str(e.value)
    assert L.hyper()["tau"] == 1.0 and L.timing().n_launch == L.fm_info()["launches_per_iter"] > 0
    L.close()
    for kw, name in ((dict(method="mcmc", order="sbpmf"), "SBPMF"), (dict(method="vb"), "VB")):
        M = FMLearnSBPMF(num_factor=4, **kw)
        with pytest.raises(SBMFError) as e:
            M.set_data(tr, te)
        assert e.value.code == SBMF_E_STATE and name in str(e.value)
        M.close()
