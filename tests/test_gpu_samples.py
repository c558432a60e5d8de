"""The posterior sample store (sbmf_keep_samples ... sbmf_load_samples, include/sbmf.h; kernels in
csrc/samples.hip): thinned samples of the SBPMF chain kept on the device, and top-N lists, full
rows and pair predictions formed from them after the run, also from a file.

The checker is numpy on what sbmf_get_sample returns: score_s = U_s[u] @ V_s.T (+ b0 + b_u + b_j
with biases), its mean and second moment over the samples.

Tolerance (tests/test_gpu_recommend.py's, derived, not fitted): the kernel and numpy each sum K
products in double, in different orders, so a score differs by at most 2 K eps sum_k |u_k v_jk|
(Higham, gamma_K per side); the bound used is twice that,
tol = 4 K eps max_j sum_k |u_k v_jk| (+ 4 eps (|b0| + |b_u| + |b_j|)), eps = 2^-52, taken as the
maximum over the samples.  Means are compared with tol, second moments (stdev^2 + mean^2) with
2 max|score| tol.  Each comparison prints the largest observed error next to its bound.

ML-100k is 943 x 1682 (1682 = 16 * 105 + 2: a ragged item tile, and 1682 = 128 * 13 + 18: a ragged
workgroup of 8 tiles); K = 20 gives Kp = 32 (padding in the K loop)."""
import subprocess

import numpy as np
import pytest

import sbmf
from sbmf import SBMF_E_ARG, SBMF_E_STATE, Communicator, Data, FMLearnSBPMF, SBMFError, device_usage, synth
from sbmf._lib import CLI_PATH, lib

from sample_files import expected_topn  # the selection's order: one copy for the list tests

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
COUNTS = ("dev_bytes", "dev_allocs", "pinned_bytes", "pinned_allocs", "streams", "events", "contexts", "comms")


def some_users(tr, num_users, n, seed=7):
    """ids 0 and num_users - 1, the users with the most and the fewest training ratings, the rest
    from a seeded permutation; n distinct ids."""
    deg = np.bincount(tr[0], minlength=num_users)
    out = []
    for u in [0, num_users - 1, int(np.argmax(deg)), int(np.argmin(deg))] + list(np.random.default_rng(seed).permutation(num_users)):
        if int(u) not in out:
            out.append(int(u))
        if len(out) == n:
            break
    return np.array(out, np.uint32)


def learner(ml, **kw):
    tr, te = ml
    kw.setdefault("num_factor", 20)
    kw.setdefault("seed", 3)
    L = FMLearnSBPMF(**kw)
    L.set_data(Data(*tr), Data(*te))
    return L


def clamp_of(L):
    return (0.5 if L.cfg.quirks in (sbmf.QUIRKS_SBPMF2, sbmf.QUIRKS_BIAS2) else 1.0, 5.0)


class Moments:
    """numpy sums of the users' scores over the stored samples, and the derived tolerance."""

    def __init__(self, L, users, clamp=False, bias=False):
        users = np.asarray(users, np.int64)
        K = L.cfg.num_factor
        self.n = L.samples_info()["count"]
        self.tol = self.smax = 0.0
        self.s1 = self.s2 = 0.0
        for s in range(self.n):
            x = L.sample(s)
            U, V = x["U"], x["V"]
            sc = U[users] @ V.T
            t = 4 * K * EPS * (np.abs(U[users]) @ np.abs(V).T).max()
            if bias:
                sc = ((x["b0"] + x["bu"][users])[:, None] + x["bv"][None, :]) + sc
                t += 4 * EPS * (abs(x["b0"]) + np.abs(x["bu"][users]).max() + np.abs(x["bv"]).max())
            if clamp:
                sc = np.clip(sc, *clamp_of(L))
            self.tol = max(self.tol, t)
            self.smax = max(self.smax, float(np.abs(sc).max()))
            self.s1 = self.s1 + sc
            self.s2 = self.s2 + sc * sc
        self.mean, self.m2 = self.s1 / self.n, self.s2 / self.n

    def check_rows(self, rows, what):
        """rows[w] = (mean, stdev) of user w against every item"""
        e1 = max(float(np.abs(m - self.mean[w]).max()) for w, (m, _) in enumerate(rows))
        e2 = max(float(np.abs(sd * sd + m * m - self.m2[w]).max()) for w, (m, sd) in enumerate(rows))
        b2 = 2 * self.smax * self.tol
        print("%s: %d samples  max|mean err| %.3e (bound %.3e)  max|2nd moment err| %.3e (bound %.3e)"
              % (what, self.n, e1, self.tol, e2, b2))
        assert e1 <= self.tol, (what, e1, self.tol)
        assert e2 <= b2, (what, e2, b2)

    def check_lists(self, items, mean, sd, what):
        """the values a top-N call returns beside its items, against numpy's at those items"""
        real = items >= 0
        w = np.nonzero(real)[0]
        e1 = float(np.abs(mean[real] - self.mean[w, items[real]]).max())
        e2 = float(np.abs(sd[real] ** 2 + mean[real] ** 2 - self.m2[w, items[real]]).max())
        b2 = 2 * self.smax * self.tol
        print("%s: %d list entries  max|mean err| %.3e (bound %.3e)  max|2nd moment err| %.3e (bound %.3e)"
              % (what, int(real.sum()), e1, self.tol, e2, b2))
        assert e1 <= self.tol and e2 <= b2, (what, e1, self.tol, e2, b2)


def check_against_numpy(L, users, what, clamp=False, bias=False):
    """every user's full row (one user per launch) and the multi-user launch's lists, against numpy"""
    M = Moments(L, users, clamp, bias)
    rows = [L.samples_scores(int(u), clamp=clamp) for u in users]
    M.check_rows(rows, what + " rows")
    items, mean, sd = L.samples_recommend(users, topn=1024, exclude_rated=False, clamp=clamp)
    assert (items >= 0).all()
    M.check_lists(items, mean, sd, what + " lists")
    # the lists hold exactly the rows' values
    for w in range(len(users)):
        assert np.array_equal(mean[w], rows[w][0][items[w]]) and np.array_equal(sd[w], rows[w][1][items[w]])
    return M, rows


# ---- 1. the store is the chain
@pytest.mark.parametrize("quirks", ["final", "bias2"])
@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("rng", ["ref", "philox"])
def test_the_store_is_the_chain(ml100k, rng, precision, quirks):
    L = learner(ml100k, rng=rng, precision=precision, quirks=quirks)
    L.keep_samples(every=1, cap=4)
    for s in range(3):
        L.learn(sweeps=1)
        info = L.samples_info()
        assert info["count"] == s + 1 and info["cap"] == 4 and info["every"] == 1
        x = L.sample(s)
        U, V = L.factors()
        assert x["sweep"] == s and np.array_equal(x["U"], U) and np.array_equal(x["V"], V)
        if quirks == "bias2":
            bu, bv, b0 = L.biases()
            assert np.array_equal(x["bu"], bu) and np.array_equal(x["bv"], bv) and x["b0"] == b0
            assert np.abs(bu).max() > 0
    ts = 4 if precision == "f32" else 8
    assert L.samples_info()["bytes"] == 4 * ((943 + 1682) * 32 * ts + (8 * (943 + 1682) if quirks == "bias2" else 0))
    L.close()


# ---- 2. thinning, the ring and burn-in
def test_thinning_ring_and_burnin(ml100k):
    kw = dict(rng="philox", burnin=2, seed=5)
    L = learner(ml100k, **kw)
    L.keep_samples(every=2, cap=3)
    L.learn(sweeps=11)  # 2 burn-in sweeps and 9 collected ones: 2, 4, 6, 8, 10 are kept, the last 3 stay
    assert L.samples_info() == {"count": 3, "cap": 3, "every": 2, "bytes": 3 * (943 + 1682) * 32 * 8}
    got = [L.sample(s) for s in range(3)]
    assert [x["sweep"] for x in got] == [6, 8, 10]
    twin = learner(ml100k, **kw)
    for s in range(11):
        twin.learn(sweeps=1)
        if s in (6, 8, 10):
            U, V = twin.factors()
            x = got[(s - 6) // 2]
            assert np.array_equal(x["U"], U) and np.array_equal(x["V"], V), s
    # registered between runs: the count starts at the first collected sweep after registration
    twin.keep_samples(every=3, cap=2)
    twin.learn(sweeps=5)  # sweeps 11..15: 11 and 14 are kept
    assert [twin.sample(s)["sweep"] for s in range(2)] == [11, 14]
    L.close()
    twin.close()


# ---- 3. scores against numpy
@pytest.mark.parametrize("precision,quirks", [("f64", "final"), ("f64", "bias2"), ("f32", "final")])
def test_scores_against_numpy(ml100k, precision, quirks):
    tr, _ = ml100k
    users = some_users(tr, 943, 37)  # not a multiple of 16; ids 0 and 942
    bias = quirks == "bias2"
    L = learner(ml100k, rng="philox", precision=precision, quirks=quirks)
    L.keep_samples(every=1, cap=4)
    L.learn(sweeps=1)
    _, rows = check_against_numpy(L, users, "%s/%s one sample" % (precision, quirks), bias=bias)
    for _, sd in rows:
        assert np.all(sd == 0.0), "one sample has no spread"
    items, _, sd = L.samples_recommend(users, topn=5)
    assert np.all(sd == 0.0)
    assert np.all(L.samples_predict(users, np.zeros(len(users), np.uint32))[1] == 0.0)
    L.learn(sweeps=3)
    for clamp in (False, True):
        M, rows = check_against_numpy(L, users, "%s/%s clamp=%s" % (precision, quirks, clamp), clamp=clamp, bias=bias)
        assert max(sd.max() for _, sd in rows) > 0
    L.close()


# ---- 4. agreement with the watch list
@pytest.mark.parametrize("quirks", ["final", "bias2"])
def test_agrees_with_the_watch_list(ml100k, quirks):
    tr, _ = ml100k
    users = some_users(tr, 943, 37)
    L = learner(ml100k, rng="philox", quirks=quirks)
    L.watch(users)
    L.keep_samples(every=1, cap=8)
    L.learn(sweeps=4)
    M = Moments(L, users, bias=quirks == "bias2")
    e1 = e2 = 0.0
    same = True
    for w, u in enumerate(users):
        a, b = L.watch_scores(w), L.samples_scores(int(u))
        same = same and np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        e1 = max(e1, float(np.abs(a[0] - b[0]).max()))
        e2 = max(e2, float(np.abs((a[1] ** 2 + a[0] ** 2) - (b[1] ** 2 + b[0] ** 2)).max()))
    print("watch list vs store (%s): bits equal: %s  max|mean diff| %.3e (bound %.3e)  max|2nd moment diff| %.3e "
          "(bound %.3e)" % (quirks, same, e1, 2 * M.tol, e2, 4 * M.smax * M.tol))
    assert e1 <= 2 * M.tol and e2 <= 2 * (2 * M.smax * M.tol)
    # the two kernels share the tile products and the sums' expressions (csrc/recommend_dev.h) and add the same
    # samples in the same order: the rows are the same bits
    assert same
    L.close()


# ---- 5. kernel shape edges
# Kp 112: 64 users per workgroup; Kp 128: 32; Kp 256: 16 -- with padding columns (120, 250) and without (128, 256)
@pytest.mark.parametrize("K", [100, 120, 128, 250, 256])
def test_wide_factors(ml100k, K):
    tr, _ = ml100k
    users = some_users(tr, 943, 37)
    L = learner(ml100k, num_factor=K, seed=1, rng="philox")
    L.keep_samples(every=1, cap=2)
    L.learn(sweeps=2)
    check_against_numpy(L, users, "K=%d" % K)
    L.close()


def test_several_blocks_each_way():
    tr, te, (I, J) = synth.generate("ml-2k")
    users = some_users(tr, I, 130)  # three workgroups of 64 users, 24 of 128 items
    L = FMLearnSBPMF(num_factor=100, seed=1, rng="philox")
    L.set_data(Data(*tr), Data(*te), num_users=I, num_items=J)
    L.keep_samples(every=1, cap=2)
    L.learn(sweeps=2)
    check_against_numpy(L, users, "ml-2k K=100")
    L.close()


def test_more_users_than_one_slice_and_the_per_sample_loop(ml100k):
    tr, _ = ml100k
    users = some_users(tr, 943, 150)
    L = learner(ml100k, rng="philox")
    L.keep_samples(every=1, cap=3)
    L.learn(sweeps=3)
    whole = L.samples_recommend(users, topn=20, risk=0.5)
    M = Moments(L, users)
    M.check_lists(*whole, "one slice")
    Jp = 1696
    assert lib.sbmf_test_samples_tune(L.ctx, 64 * 2 * Jp * 8, 0) == 0  # 64 users per slice: slices of 64, 64 and 22
    sliced = L.samples_recommend(users, topn=20, risk=0.5)
    for a, b in zip(whole, sliced):
        assert np.array_equal(a, b)
    assert lib.sbmf_test_samples_tune(L.ctx, 0, 1) == 0  # one launch of the watch list's kernel per sample
    loop = L.samples_recommend(users, topn=1024, exclude_rated=False)
    M.check_lists(*loop, "per-sample loop")
    assert lib.sbmf_test_samples_tune(L.ctx, 0, 0) == 0
    fused = L.samples_recommend(users, topn=1024, exclude_rated=False)
    print("fused kernel vs per-sample loop: bits equal: %s" % all(np.array_equal(a, b) for a, b in zip(fused, loop)))
    L.close()


# ---- 6. selection
@pytest.fixture(scope="module")
def store37(ml100k):
    tr, _ = ml100k
    users = some_users(tr, 943, 37)
    L = learner(ml100k, rng="philox")
    L.keep_samples(every=1, cap=4)
    L.learn(sweeps=4)
    rows = [L.samples_scores(int(u)) for u in users]
    yield L, users, tr, rows
    L.close()


@pytest.mark.parametrize("exclude", [True, False])
@pytest.mark.parametrize("risk", [0.0, 1.0])
@pytest.mark.parametrize("topn", [1, 10, 1024])
def test_selection_is_the_lexsort(store37, topn, risk, exclude):
    L, users, tr, rows = store37
    items, mean, sd = L.samples_recommend(users, topn=topn, exclude_rated=exclude, risk=risk)
    assert items.shape == mean.shape == sd.shape == (len(users), topn) and items.dtype == np.int64
    for w, u in enumerate(users):
        m, s = rows[w]
        rated = tr[1][tr[0] == u]
        want = expected_topn(m, s, rated, topn, risk, exclude)
        assert np.array_equal(items[w], want), (w, int(u), topn, risk, exclude)
        real = want >= 0
        assert np.array_equal(mean[w][real], m[want[real]]) and np.array_equal(sd[w][real], s[want[real]])
        assert np.all(np.isnan(mean[w][~real])) and np.all(np.isnan(sd[w][~real]))


# ---- 7. pair prediction
@pytest.mark.parametrize("precision,quirks", [("f64", "final"), ("f64", "bias2"), ("f32", "final")])
def test_pairs_against_numpy(ml100k, precision, quirks):
    L = learner(ml100k, rng="philox", precision=precision, quirks=quirks)
    L.keep_samples(every=1, cap=4)
    L.learn(sweeps=4)
    rng = np.random.default_rng(11)
    u = np.concatenate([rng.integers(0, 943, 1000), [0, 0, 942, 942]]).astype(np.uint32)
    i = np.concatenate([rng.integers(0, 1682, 1000), [0, 1681, 0, 1681]]).astype(np.uint32)
    for clamp in (False, True):
        s1 = s2 = tol = smax = 0.0
        for s in range(4):
            x = L.sample(s)
            sc = np.einsum("pk,pk->p", x["U"][u], x["V"][i])
            t = 4 * 20 * EPS * np.einsum("pk,pk->p", np.abs(x["U"][u]), np.abs(x["V"][i])).max()
            if quirks == "bias2":
                sc = ((x["b0"] + x["bu"][u]) + x["bv"][i]) + sc
                t += 4 * EPS * (abs(x["b0"]) + np.abs(x["bu"]).max() + np.abs(x["bv"]).max())
            if clamp:
                sc = np.clip(sc, *clamp_of(L))
            tol, smax = max(tol, t), max(smax, float(np.abs(sc).max()))
            s1, s2 = s1 + sc, s2 + sc * sc
        mean, sd = L.samples_predict(u, i, clamp=clamp)
        e1 = float(np.abs(mean - s1 / 4).max())
        e2 = float(np.abs(sd * sd + mean * mean - s2 / 4).max())
        print("pairs %s/%s clamp=%s: max|mean err| %.3e (bound %.3e)  max|2nd moment err| %.3e (bound %.3e)"
              % (precision, quirks, clamp, e1, tol, e2, 2 * smax * tol))
        assert e1 <= tol and e2 <= 2 * smax * tol
        assert sd.max() > 0
    L.close()


@pytest.mark.parametrize("quirks", ["final", "bias2"])
def test_pairs_agree_with_predict(ml100k, quirks):
    tr, te = ml100k
    L = learner(ml100k, rng="philox", quirks=quirks, burnin=0, average="collected")
    L.keep_samples(every=1, cap=5)
    L.learn(sweeps=5)
    mean, _ = L.samples_predict(te[0], te[1], clamp=True)
    tol = 0.0
    for s in range(5):
        x = L.sample(s)
        tol = max(tol, 4 * 20 * EPS * np.einsum("pk,pk->p", np.abs(x["U"][te[0]]), np.abs(x["V"][te[1]])).max()
                  + (4 * EPS * (abs(x["b0"]) + np.abs(x["bu"]).max() + np.abs(x["bv"]).max()) if quirks == "bias2" else 0.0))
    err = float(np.abs(mean - L.predict()).max())
    print("samples_predict vs predict (%s): max err %.3e (bound %.3e)" % (quirks, err, tol))
    assert err <= tol
    L.close()


# ---- 8. the chain is untouched; a rerun is bit-identical
@pytest.mark.parametrize("rng", ["ref", "philox"])
def test_chain_is_untouched(ml100k, rng):
    out = []
    for kept in (False, True):
        L = learner(ml100k, seed=11, rng=rng)
        if kept:
            L.keep_samples(every=2, cap=2)
        L.learn(sweeps=5)
        h = L.hyper()
        out.append((L.rmse_trajectory, *L.factors(), L.predict(), h["sigma_u"], h["mu_u"], h["sigma_v"], h["mu_v"],
                    np.array([h["tau"]])))
        L.close()
    for a, b in zip(*out):
        assert np.array_equal(a, b)


def test_rerun_is_bit_identical(ml100k):
    tr, _ = ml100k
    users = some_users(tr, 943, 37)
    out = []
    for _ in range(2):
        L = learner(ml100k, seed=9, rng="philox")
        L.keep_samples(every=1, cap=3)
        L.learn(sweeps=3)
        for _ in range(2):  # twice from one store, and from a second chain
            out.append(list(L.samples_recommend(users, topn=50, risk=0.5)) + list(L.samples_scores(17))
                       + list(L.samples_predict(users, users)))
        L.close()
    for other in out[1:]:
        for a, b in zip(out[0], other):
            assert np.array_equal(a, b, equal_nan=True)


# ---- 9. save and load
def _code(fn, *a, **k):
    with pytest.raises(SBMFError) as ei:
        fn(*a, **k)
    return ei.value.code, str(ei.value)


@pytest.mark.parametrize("precision,quirks", [("f64", "final"), ("f32", "final"), ("f64", "bias2")])
def test_save_and_load(ml100k, tmp_path, precision, quirks):
    tr, _ = ml100k
    users = some_users(tr, 943, 37)
    path = tmp_path / "samples.bin"
    L = learner(ml100k, rng="philox", precision=precision, quirks=quirks)
    L.keep_samples(every=1, cap=3)
    L.learn(sweeps=4)  # the ring has wrapped: sweeps 1, 2, 3
    L.save_samples(path)
    info = sbmf.samples_file_info(path)
    ts = 4 if precision == "f32" else 8
    bias = quirks == "bias2"
    assert info == {"version": 1, "precision": precision, "num_users": 943, "num_items": 1682, "num_factor": 20,
                    "count": 3, "bias": bias,
                    "bytes": 40 + 3 * 4 + 3 * ((943 + 1682) * 20 * ts + (8 * (1 + 943 + 1682) if bias else 0))}
    F = learner(ml100k, rng="philox", precision=precision, quirks=quirks)  # prepared, never run
    assert _code(F.samples_scores, 0)[0] == SBMF_E_STATE
    F.load_samples(path)
    assert F.samples_info()["count"] == 3 and F.samples_info()["cap"] == 3
    for s in range(3):
        a, b = L.sample(s), F.sample(s)
        assert a["sweep"] == b["sweep"] == s + 1 and a["b0"] == b["b0"]
        for k in ("U", "V", "bu", "bv"):
            assert np.array_equal(a[k], b[k])
    for u in (0, 17, 942):
        for a, b in zip(L.samples_scores(u), F.samples_scores(u)):
            assert np.array_equal(a, b)
    for a, b in zip(L.samples_recommend(users, topn=30, risk=1.0), F.samples_recommend(users, topn=30, risk=1.0)):
        assert np.array_equal(a, b)
    # loading into a larger store keeps its capacity; the chain of F is untouched and runs on
    F.keep_samples(every=1, cap=5)
    F.load_samples(path)
    assert F.samples_info()["count"] == 3 and F.samples_info()["cap"] == 5
    F.learn(sweeps=1)
    assert [F.sample(s)["sweep"] for s in range(4)] == [1, 2, 3, 0]
    F.close()
    L.close()
    if (precision, quirks) != ("f64", "final"):
        return
    for kw, words in ((dict(num_factor=8), ("num_factor K = 20", "K = 8")), (dict(precision="f32"), ("precision f64", "f32")),
                      (dict(quirks="bias2"), ("bias = 0", "biased"))):
        O = learner(ml100k, rng="philox", **kw)
        code, msg = _code(O.load_samples, path)
        assert code == SBMF_E_ARG and all(w in msg for w in words), (kw, msg)
        O.close()


# ---- 10. errors and resources
def test_errors_and_resources(ml100k):
    tr, te = ml100k
    base = {k: device_usage()[k] for k in COUNTS}
    L = learner(ml100k, rng="philox")
    held = {k: device_usage()[k] for k in COUNTS}
    for fn, args in ((L.samples_scores, (0,)), (L.samples_recommend, ([0],)), (L.samples_predict, ([0], [0])), (L.sample, (0,))):
        code, msg = _code(fn, *args)
        assert code == SBMF_E_STATE and "no sample kept yet" in msg
    assert _code(L.keep_samples, every=0, cap=4)[0] == SBMF_E_ARG
    assert _code(L.keep_samples, every=1, cap=65536)[0] == SBMF_E_ARG
    assert L.samples_info() == {"count": 0, "cap": 0, "every": 1, "bytes": 0}
    L.keep_samples(every=1, cap=2)
    assert device_usage()["dev_allocs"] == held["dev_allocs"] + 2
    code, msg = _code(L.samples_scores, 0)  # registered, nothing kept
    assert code == SBMF_E_STATE and "no sample kept yet" in msg
    L.learn(sweeps=2)
    assert _code(L.samples_scores, 943)[0] == SBMF_E_ARG
    assert _code(L.samples_recommend, [0, 943])[0] == SBMF_E_ARG
    assert _code(L.samples_recommend, [0], topn=0)[0] == SBMF_E_ARG
    assert _code(L.samples_recommend, [0], topn=1025)[0] == SBMF_E_ARG
    assert _code(L.samples_predict, [0], [1682])[0] == SBMF_E_ARG
    assert _code(L.samples_predict, [943], [0])[0] == SBMF_E_ARG
    assert _code(L.sample, 2)[0] == SBMF_E_ARG
    a, b = L.samples_recommend([5, 5], topn=3)[0]  # a repeated id gives the same list twice
    assert np.array_equal(a, b)
    t = L.samples_timing()
    assert t["ms_copy"] > 0 and t["ms_score"] > 0 and t["ms_select"] > 0
    before = dict(held)
    mid = {k: device_usage()[k] for k in COUNTS}
    assert mid["dev_allocs"] == before["dev_allocs"] + 2  # the calls' temporaries are freed
    L.keep_samples(every=1, cap=0)
    assert {k: device_usage()[k] for k in COUNTS} == held
    assert _code(L.samples_scores, 0)[0] == SBMF_E_STATE
    L.keep_samples(every=1, cap=3)  # closed with a live store
    L.learn(sweeps=1)
    L.close()
    assert {k: device_usage()[k] for k in COUNTS} == base
    for kw, word in ((dict(method="vb", num_factor=8), "online VB"), (dict(order="libfm", num_factor=8), "libFM MCMC"),
                     (dict(method="als", num_factor=8), "ALS")):
        O = FMLearnSBPMF(seed=1, **kw)
        O.set_data(Data(*tr), Data(*te))
        for fn, args in ((O.keep_samples, ()), (O.samples_scores, (0,)), (O.load_samples, ("/nonexistent",))):
            code, msg = _code(fn, *args)
            assert code == SBMF_E_STATE and "SBPMF sampler" in msg and word in msg, (kw, msg)
        O.close()
    comm = Communicator(1, 0, bytes(128))  # a context that joined a communicator, even one of a single rank
    N = FMLearnSBPMF(num_factor=8, seed=1, rng="philox")
    N.init(comm=comm)
    for fn, args in ((N.keep_samples, ()), (N.samples_info, ()), (N.samples_scores, (0,)), (N.samples_recommend, ([0],)),
                     (N.samples_predict, ([0], [0])), (N.sample, (0,)), (N.load_samples, ("/nonexistent",))):
        code, msg = _code(fn, *args)
        assert code == SBMF_E_STATE and "joined a communicator" in msg, msg
    N.close()
    comm.close()
    R = FMLearnSBPMF(num_factor=8, seed=1, rng="philox")
    R.init()
    assert lib.sbmf_test_virtual_rank(R.ctx, 2, 0) == 0
    R.set_data(Data(*tr), Data(*te))
    code, msg = _code(R.keep_samples)
    assert code == SBMF_E_STATE and "virtual rank" in msg
    R.close()
    assert {k: device_usage()[k] for k in COUNTS} == base


# ---- 11. the command line
def test_cli_writes_and_serves_a_sample_file(ml100k, tmp_path):
    tr, te = ml100k
    for name, d in (("train", tr), ("test", te)):
        with open(tmp_path / name, "w") as f:
            for u, i, r in zip(*d):
                f.write("%d %d %g\n" % (u, i, r))
    ids = [0, 17, 942]
    (tmp_path / "ids").write_text("".join("%d\n" % u for u in ids))
    common = [CLI_PATH, "-task", "r", "-train", str(tmp_path / "train"), "-test", str(tmp_path / "test"), "-dim", "0,0,8",
              "-rng", "philox", "-seed", "4"]
    sfile = tmp_path / "samples.bin"
    r = subprocess.run(common + ["-iter", "5", "-burnin", "1", "-samples_out", str(sfile), "-samples_every", "2"],
                       capture_output=True, text=True, timeout=120, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr
    info = sbmf.samples_file_info(sfile)
    assert (info["count"], info["num_users"], info["num_items"], info["num_factor"]) == (3, 943, 1682, 8)
    rec, out = tmp_path / "rec", tmp_path / "pred"
    r = subprocess.run(common + ["-samples_in", str(sfile), "-recommend", str(rec), "-rec_users", str(tmp_path / "ids"),
                                 "-rec_topn", "5", "-rec_risk", "0.5", "-out", str(out)],
                       capture_output=True, text=True, timeout=120, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr
    assert "#Iter=" not in r.stdout  # no sweep
    line = [l for l in r.stdout.splitlines() if l.startswith("#Samples=")]
    assert len(line) == 1 and line[0].startswith("#Samples=3\tTest=")
    # the same store in Python
    L = learner(ml100k, num_factor=8, rng="philox")
    L.load_samples(sfile)
    assert [L.sample(s)["sweep"] for s in range(3)] == [1, 3, 5]
    pred, _ = L.samples_predict(te[0], te[1], clamp=True)
    rmse = float(np.sqrt(np.mean((pred - te[2]) ** 2)))
    assert line[0] == "#Samples=3\tTest=%g" % rmse
    assert np.allclose(np.array([float(x) for x in out.read_text().split()]), pred, rtol=1e-5, atol=0)
    items, mean, sd = L.samples_recommend(ids, topn=5, risk=0.5)
    want = ["%d\t%d\t%.17g\t%.17g" % (u, items[k][j], mean[k][j], sd[k][j]) for k, u in enumerate(ids) for j in range(5)]
    assert rec.read_text().splitlines() == want
    L.close()
