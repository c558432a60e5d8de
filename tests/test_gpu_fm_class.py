"""Binary classification (libFM's -task c, a probit model) in the two libFM MCMC / ALS learners on
the GPU.  Against
  1. libFM itself (libfm.cpp compiled from its sources and run with -task c; goldens written by
     tests/make_fm_class_golden.py) through the command line and through Python,
  2. a serial float64 numpy restatement of libFM's ALS classification (no random number at all:
     the device erf and the expected-value formula, case by case),
  3. the exact moments of the truncated normals, for the Philox draw of the latent targets, with
     its independence of the launch's size and of the cases' order,
  4. the reference's own spread over 16 seeds, for whole Philox chains,
and: reruns are bit-identical, nothing leaks, regression is untouched, and what is not offered is
refused."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import fm_cases
import fm_class
import fm_groups
from conftest import GOLD, REPO, gpu_available
from sbmf import Data, FMLearnSBPMF, SBMFError, comm_unique_id, device_usage, tgauss
from sbmf._lib import CLI_PATH, SBMF_E_ARG, SBMF_E_STATE
from test_gpu_libfm import _within_printed

pytestmark = pytest.mark.gpu


def _learner(method, regular=(0.0, 0.0, 0.0), K=8, seed=1, rng="ref", **kw):
    return FMLearnSBPMF(num_factor=K, seed=seed, rng=rng, method="als" if method == "als" else "mcmc", order="libfm",
                        k0=1, k1=1, regular=regular, init_stdev=0.1, task="c", **kw)


def _same_printed(x, ref):
    x, ref = np.asarray(x, float), np.asarray(ref, float)
    nan = np.isnan(ref)
    return x.shape == ref.shape and np.array_equal(np.isnan(x), nan) and _within_printed(x[~nan], ref[~nan])


# ---- 1. the command line against libFM
# (golden, learner): "two": the two-attribute learner on the two-feature text; "general": the same
# files through the general learner (SBMF_FMM_GENERAL=1; a -meta file would change the chain)
CLI_RUNS = [("ref_libfm_c_mcmc_m1m100k_i8", "two"), ("ref_libfm_c_als_m1m100k_i8", "two"),
            ("ref_libfm_c_mcmc_m1m100k_i8", "general"), ("ref_libfm_c_als_m1m100k_i8", "general"),
            ("ref_libfm_c_mcmc_fm4_i8", "general"), ("ref_libfm_c_als_fm4_i8", "general"),
            ("ref_libfm_c_mcmc_fm4_g4_i6", "general"), ("ref_libfm_c_mcmc_edge_i5", "general")]


def _write_set(dset, ml100k, dirpath):
    if dset == "m1m100k":
        return fm_class.write_m1m100k_class(dirpath)
    if dset == "fm4":
        return fm_class.write_cases(dirpath, *fm_class.fm4_class(ml100k))
    return fm_class.write_cases(dirpath, *fm_class.edge_class())


@pytest.mark.parametrize("name,learner", CLI_RUNS, ids=["%s-%s" % r for r in CLI_RUNS])
def test_cli_matches_libfm(name, learner, ml100k, tmp_path):
    assert gpu_available()
    dset, method, reg, iters, meta = fm_class.GOLDEN_RUNS[name]
    trf, tef = _write_set(dset, ml100k, tmp_path)
    cmd = [CLI_PATH, "-task", "c", "-train", trf, "-test", tef, "-dim", "1,1,8", "-iter", str(iters), "-method", method,
           "-out", "pred.txt", "-rlog", "rlog.txt"]
    if reg:
        cmd += ["-regular", reg]
    if meta:
        fm_groups.write_meta(os.path.join(str(tmp_path), "meta.txt"), fm_groups.fm4_groups(ml100k))
        cmd += ["-meta", "meta.txt"]
    env = dict(os.environ)
    if dset == "m1m100k" and learner == "general":
        env["SBMF_FMM_GENERAL"] = "1"
    r = subprocess.run(cmd, cwd=str(tmp_path), capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stderr
    assert ("#attributes=" in r.stdout) == (dset != "m1m100k")  # the CLI's own line of the general input
    lines = [l for l in r.stdout.splitlines() if l.startswith("#Iter=")]
    ref_lines, ref_pred, header, rows = fm_class.golden(name)
    print("\n".join(lines))
    assert lines == ref_lines
    pred = np.loadtxt(tmp_path / "pred.txt")
    assert pred.shape == ref_pred.shape and _within_printed(pred, ref_pred)
    assert pred.min() >= 0.0 and pred.max() <= 1.0
    t = open(os.path.join(str(tmp_path), "rlog.txt")).read().splitlines()
    ours = t[0].split("\t")
    assert ours[:len(header)] == header and all(c.startswith("sbmf_") for c in ours[len(header):])
    assert len(t) == iters + 1
    cols = [header.index(c) for c in fm_class.RLOG_COLUMNS] + list(range(header.index("wmu[0]"), len(header)))
    never = [header.index(c) for c in ("acc_mcmc_all_but5", "ll_mcmc_all", "ll_mcmc_all_but5")]
    for it in range(iters):
        got = [float(x) for x in t[1 + it].split("\t")]
        assert _same_printed([got[c] for c in cols], [rows[it][c] for c in cols]), (it, got, rows[it])
        assert all(math.isnan(got[c]) for c in never)  # libFM logs uninitialised variables there


# ---- 2. Python
def test_python_two_attribute_learner_matches_libfm(m1m100k):
    assert gpu_available()
    (tu, ti, ty), (su, si, sy) = fm_class.m1m100k_class(m1m100k)
    I = int(max(tu.max(), su.max())) + 1
    for method, name in (("mcmc", "ref_libfm_c_mcmc_m1m100k_i8"), ("als", "ref_libfm_c_als_m1m100k_i8")):
        ref_lines, ref_pred, header, rows = fm_class.golden(name)
        ref_train, ref_test = fm_class.iter_values(ref_lines)
        L = _learner(method, (0.0, 1.0, 10.0) if method == "als" else (0.0, 0.0, 0.0))
        L.set_data(Data(tu, ti - I, ty), Data(su, si - I, sy), num_users=I)
        L.learn(sweeps=8)
        h = L.history
        print(method, [x["acc_train"] for x in h], list(L.acc_trajectory))
        assert _within_printed([x["acc_train"] for x in h], ref_train) and _within_printed(L.acc_trajectory, ref_test)
        assert _within_printed([x["acc_this"] for x in h], [r[header.index("acc_mcmc_this")] for r in rows])
        assert _within_printed([x["ll_this"] for x in h], [r[header.index("ll_mcmc_this")] for r in rows])
        assert _within_printed([x["tau"] for x in h], [r[header.index("alpha")] for r in rows])
        assert all(math.isnan(x["rmse_avg"]) and math.isnan(x["rmse_this"]) and math.isnan(x["rmse_train"]) for x in h)
        pred = L.predict()
        assert pred.shape == ref_pred.shape and _within_printed(pred, ref_pred)
        assert pred.min() >= 0.0 and pred.max() <= 1.0
        L.close()


def test_python_cases_match_libfm_and_raw_targets_are_mapped(ml100k):
    """fm4 as Cases; the targets given as rating - 3.5 (any value <= 0 is the negative class)."""
    assert gpu_available()
    tr, te = fm_cases.fm4(ml100k)[:2]
    tr, te = fm_class.with_targets(tr, tr.target - 3.5), fm_class.with_targets(te, te.target - 3.5)
    ref_lines, ref_pred, _, _ = fm_class.golden("ref_libfm_c_mcmc_fm4_i8")
    ref_train, ref_test = fm_class.iter_values(ref_lines)
    L = _learner("mcmc")
    L.set_data(tr, te)
    L.learn(sweeps=8)
    assert _within_printed([x["acc_train"] for x in L.history], ref_train)
    assert _within_printed(L.acc_trajectory, ref_test)
    assert _within_printed(L.predict(), ref_pred)
    L.close()


# ---- 3. ALS draws nothing: the serial restatement
def _check_als(tr, te, K, seed, regular, iters, env=None):
    a = fm_class.als_class_restatement(tr, te, K, iters, seed, regular, np.float64)
    b = fm_class.als_class_restatement(tr, te, K, iters, seed, regular, np.longdouble)
    gap = lambda x, y: float(np.max(np.abs(np.asarray(x, np.longdouble) - np.asarray(y, np.longdouble)))) if np.size(x) else 0.0
    L = _learner("als", regular, K=K, seed=seed)
    L.set_data(tr, te)
    for it in range(1, iters + 1):
        L.learn(sweeps=1)
        (aat, aaa, aah, all_, apt, aw0, aw, av), (bat, baa, bah, bll, bpt, bw0, bw, bv) = a[it - 1], b[it - 1]
        w0, w, v = L.fm()
        h = L.history[-1]
        g_w, g_v, g_p = max(gap(aw, bw), gap(aw0, bw0)), gap(av, bv), gap(apt, bpt)
        print("iteration %d: f64-longdouble gap w %.3g v %.3g p %.3g; |gpu - f64| w %.3g v %.3g p %.3g; acc %r %r" % (
            it, g_w, g_v, g_p, gap(w, aw), gap(v, av), gap(L.predict(), apt), (h["acc_train"], h["acc_avg"], h["acc_this"]),
            (aat, aaa, aah)))
        # the tolerance of the ALS restatement tests of the general learner (test_gpu_fm_cases.py)
        assert abs(w0 - float(aw0)) <= max(1e-8, 64 * g_w)
        assert gap(w, aw) <= max(1e-8, 64 * g_w)
        assert gap(v, av) <= max(1e-8, 64 * g_v)
        assert gap(L.predict(), apt) <= max(1e-9, 64 * g_p)  # ALS predicts this iteration's probabilities
        # the votes are counts: equal, unless the restatement's own two precisions disagree on a case
        assert abs(h["acc_train"] - aat) <= max(1e-12, 64 * abs(aat - bat))
        assert abs(h["acc_avg"] - aaa) <= max(1e-12, 64 * abs(aaa - baa))
        assert abs(h["acc_this"] - aah) <= max(1e-12, 64 * abs(aah - bah))
        assert abs(h["ll_this"] - all_) <= max(1e-9 * abs(all_), 64 * abs(all_ - bll))
    L.close()


def test_als_matches_serial_restatement_small():
    assert gpu_available()
    tr, te = fm_cases.small_cases()
    tr, te = fm_class.with_targets(tr, tr.target - 3.0), fm_class.with_targets(te, te.target - 3.0)
    assert (tr.target <= 0).sum() >= 4 and (tr.target > 0).sum() >= 4
    _check_als(tr, te, 4, 3, (1.0, 2.0, 5.0), 5)


def test_als_matches_serial_restatement_edge(monkeypatch):
    assert gpu_available()
    tr, te = fm_class.edge_class()
    monkeypatch.setenv("SBMF_FMM_LONG", "256")
    monkeypatch.setenv("SBMF_FMM_CHUNK", "64")
    _check_als(tr, te, 4, 2, (0.5, 1.0, 4.0), 5)


# ---- 4. the Philox draw of the latent targets
MEANS = (-6.0, -2.0, -0.5, 0.0, 0.5, 2.0, 6.0)


@pytest.mark.parametrize("mode", ["device"])
def test_tgauss_sides_and_moments(mode):
    assert gpu_available()
    _check_tgauss_moments(mode)


def _check_tgauss_moments(mode):
    n = 65536
    for k, mean in enumerate(MEANS):
        for positive in (True, False):
            x = tgauss(np.full(n, mean), 1 if positive else -1, seed=11, it=2 * k + positive, mode=mode)
            assert np.all(x >= 0.0) if positive else np.all(x <= 0.0), (mean, positive)
            em, ev = fm_class.tgauss_moments(mean, positive)
            m4 = fm_class.tgauss_fourth_central(mean, positive)
            se_m, se_v = math.sqrt(ev / n), math.sqrt((m4 - ev * ev * (n - 3) / (n - 1)) / n)
            print("mean %g %s: sample mean %.6f (exact %.6f, se %.2g) variance %.6f (exact %.6f, se %.2g)" % (
                mean, "+" if positive else "-", x.mean(), em, se_m, x.var(ddof=1), ev, se_v))
            assert abs(x.mean() - em) <= 5 * se_m, (mean, positive)
            assert abs(x.var(ddof=1) - ev) <= 5 * se_v, (mean, positive)


def test_tgauss_depends_on_the_key_and_the_prediction_alone():
    assert gpu_available()
    n = 1000
    rs = np.random.RandomState(5)
    mean = rs.choice(MEANS, n) + rs.normal(0, 0.1, n)
    sign = np.where(rs.rand(n) < 0.5, 1, -1).astype(np.int32)
    full = tgauss(mean, sign, seed=9, it=3)
    for m in (1, 255, 256, 257):  # one block, a partial block, the block edge
        assert np.array_equal(tgauss(mean[:m], sign[:m], seed=9, it=3), full[:m]), m
    # the cases in another order, each keeping its place in the train file: the same draws, permuted
    perm = rs.permutation(n)
    assert np.array_equal(tgauss(mean[perm], sign[perm], seed=9, it=3, index=perm), full[perm])
    assert not np.array_equal(tgauss(mean, sign, seed=9, it=4), full)
    assert not np.array_equal(tgauss(mean, sign, seed=10, it=3), full)


# ---- 5. whole Philox chains
def test_rerun_is_bit_identical_and_nothing_leaks(ml100k):
    assert gpu_available()
    tr, te = fm_class.fm4_class(ml100k)
    before = device_usage()
    runs = []
    for _ in range(2):
        L = _learner("mcmc", rng="philox")
        L.set_data(tr, te)
        L.learn(sweeps=3)
        runs.append((L.fm(), L.predict(), [(h["acc_train"], h["acc_avg"], h["acc_this"], h["ll_this"]) for h in L.history]))
        assert device_usage()["dev_allocs"] > before["dev_allocs"]
        L.close()
    (w0a, wa, va), pa, ha = runs[0]
    (w0b, wb, vb), pb, hb = runs[1]
    assert w0a == w0b and np.array_equal(wa, wb) and np.array_equal(va, vb) and np.array_equal(pa, pb) and ha == hb
    after = device_usage()
    for k in ("dev_bytes", "dev_allocs", "pinned_bytes", "pinned_allocs", "streams", "events", "contexts", "comms"):
        assert after[k] == before[k], (k, before[k], after[k])


def test_philox_layouts_draw_the_same_targets(m1m100k, monkeypatch):
    """The two layouts keep the cases in different orders; the latent targets are keyed by the
    case's place in the train file, so both run the same chain (up to the layouts' rounding)."""
    assert gpu_available()
    (tu, ti, ty), (su, si, sy) = fm_class.m1m100k_class(m1m100k)
    I = int(max(tu.max(), su.max())) + 1
    out = []
    for general in (False, True):
        if general:
            monkeypatch.setenv("SBMF_FMM_GENERAL", "1")
        L = _learner("mcmc", rng="philox", seed=4)
        L.set_data(Data(tu, ti - I, ty), Data(su, si - I, sy), num_users=I)
        L.learn(sweeps=3)
        out.append((L.predict(), [h["acc_train"] for h in L.history]))
        L.close()
    monkeypatch.delenv("SBMF_FMM_GENERAL")
    np.testing.assert_allclose(out[0][0], out[1][0], rtol=0, atol=1e-9)
    np.testing.assert_allclose(out[0][1], out[1][1], rtol=0, atol=2e-5)  # a vote or two of 90 k at p = 0.5


def test_philox_chains_agree_with_the_reference_over_16_seeds(m1m100k):
    """Final Train and Test accuracy of m1m100k mcmc, 8 iterations, over 16 Philox seeds against the
    reference's 16 recorded seeds: |mean_gpu - mean_ref| <= 3 sqrt(s_g^2 / 16 + s_r^2 / 16).  The
    generator holds the reference's seeds 1-8 against its seeds 9-16 to the same bound."""
    assert gpu_available()
    (tu, ti, ty), (su, si, sy) = fm_class.m1m100k_class(m1m100k)
    I = int(max(tu.max(), su.max())) + 1
    tr, te = Data(tu, ti - I, ty), Data(su, si - I, sy)
    train, test = [], []
    for seed in range(1, 17):
        L = _learner("mcmc", rng="philox", seed=seed)
        L.set_data(tr, te, num_users=I)
        L.learn(sweeps=8)
        train.append(L.history[-1]["acc_train"])
        test.append(L.history[-1]["acc_avg"])
        L.close()
    ref = fm_class.seeds_golden()
    print("train gpu %.6f +- %.6f ref %.6f +- %.6f" % (np.mean(train), np.std(train, ddof=1), np.mean(ref["train"]),
                                                        np.std(ref["train"], ddof=1)))
    print("test  gpu %.6f +- %.6f ref %.6f +- %.6f" % (np.mean(test), np.std(test, ddof=1), np.mean(ref["test"]),
                                                        np.std(ref["test"], ddof=1)))
    assert len(ref["train"]) == 16 and len(ref["test"]) == 16
    assert fm_class.means_agree(train, ref["train"])
    assert fm_class.means_agree(test, ref["test"])


# ---- 6. regression is untouched
def test_regression_golden_is_unchanged_as_text(ml100k, tmp_path):
    assert gpu_available()
    trf, tef = fm_cases.write_fm4(ml100k, tmp_path)
    cmd = [CLI_PATH, "-task", "r", "-train", trf, "-test", tef, "-dim", "1,1,8", "-iter", "10", "-method", "mcmc"]
    r = subprocess.run(cmd, cwd=str(tmp_path), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    with open(os.path.join(GOLD, "ref_libfm_mcmc_fm4_d118_s1_i10.txt")) as f:
        assert [l for l in r.stdout.splitlines() if l.startswith("#Iter=")] == f.read().splitlines()
    tr, te = fm_cases.small_cases()
    L = FMLearnSBPMF(num_factor=4, method="als", regular=(1.0, 2.0, 5.0), init_stdev=0.1)  # task left at its default
    L.set_data(tr, te)
    L.learn(sweeps=1)
    h = L.history[-1]
    assert all(math.isnan(h[k]) for k in ("acc_train", "acc_avg", "acc_this", "ll_this")) and h["rmse_avg"] > 0
    L.close()


# ---- 7. what is not offered is refused
def test_other_methods_refuse_classification():
    assert gpu_available()
    for kw, name in ((dict(method="mcmc", order="sbpmf"), "SBPMF"), (dict(method="vb"), "VB")):
        L = FMLearnSBPMF(num_factor=4, task="c", **kw)
        with pytest.raises(SBMFError) as e:
            L.init()
        assert e.value.code == SBMF_E_ARG and name in str(e.value) and "classification" in str(e.value)


def test_several_ranks_refuse_classification(tmp_path):
    assert gpu_available()
    old = os.environ.get("SBMF_COMM")
    os.environ["SBMF_COMM"] = "host"
    try:
        uid = comm_unique_id()
    finally:
        if old is None:
            del os.environ["SBMF_COMM"]
        else:
            os.environ["SBMF_COMM"] = old
    worker = os.path.join(REPO, "tests", "workers", "fm_class_worker.py")
    procs = [subprocess.Popen([sys.executable, worker, str(r), "2", uid.hex()], stdout=subprocess.PIPE,
                              stderr=subprocess.STDOUT) for r in range(2)]
    for p in procs:
        try:
            o, _ = p.communicate(timeout=120)
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
        o = o.decode(errors="replace")
        assert p.returncode == 0, o[-2000:]
        assert "refused %d:" % SBMF_E_STATE in o and "classification" in o and "one rank" in o, o[-2000:]
