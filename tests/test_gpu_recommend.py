"""Posterior top-N for a watch list of users (sbmf_watch_users / sbmf_watch_scores /
sbmf_recommend, include/sbmf.h; kernels in csrc/recommend.hip).

The reference has nothing of the kind, so the checker is numpy on the factors
the library itself returns after every sweep: score_s = U_s[w] @ V_s.T
(+ b0 + b_u + b_j with biases), its running mean and second moment.

Tolerance (derived, not fitted): the kernel and numpy each sum K products in
double, in different orders, so a score differs by at most 2 K eps sum_k |u_k v_jk|
(Higham, gamma_K per side); the bound used is twice that,
tol = 4 K eps max_j sum_k |u_k v_jk| (+ 4 eps (|b0| + |b_u| + |b_j|)), eps = 2^-52,
taken as the maximum over the sweeps accumulated so far.  Means are compared with
tol, second moments (stdev^2 + mean^2) with 2 max|score| tol.  Each comparison
prints the largest observed error next to its bound.

ML-100k is 943 x 1682 (1682 = 16 * 105 + 2: a ragged item tile); K = 20 gives
Kp = 32 (padding in the K loop)."""
import subprocess

import numpy as np
import pytest

from conftest import write_m1m100k_libfm
from sample_files import expected_topn  # the selection's order: one copy for the list tests
from sbmf import (SBMF_E_ARG, SBMF_E_STATE, Data, FMLearnSBPMF, SBMFError, device_usage, synth)
from sbmf._lib import CLI_PATH

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
COUNTS = ("dev_bytes", "dev_allocs", "pinned_bytes", "pinned_allocs", "streams", "events", "contexts", "comms")


def watch_ids(tr, num_users, n, seed=7):
    """ids 0 and num_users - 1, the users with the most and the fewest training ratings,
    the rest from a seeded permutation; n distinct ids."""
    deg = np.bincount(tr[0], minlength=num_users)
    ids = [0, num_users - 1, int(np.argmax(deg)), int(np.argmin(deg))]
    out = []
    for u in ids + list(np.random.default_rng(seed).permutation(num_users)):
        if int(u) not in out:
            out.append(int(u))
        if len(out) == n:
            break
    return np.array(out, np.uint32)


class Moments:
    """numpy running sums of the watched users' scores, and the derived tolerance."""

    def __init__(self, users, K):
        self.users, self.K = np.asarray(users, np.int64), K
        self.s1 = self.s2 = None
        self.n = 0
        self.tol = 0.0      # per score, max over the sweeps so far
        self.smax = 0.0     # max |score| over the sweeps so far

    def add(self, U, V, bias=None, clamp=None):
        s = U[self.users] @ V.T
        t = 4 * self.K * EPS * (np.abs(U[self.users]) @ np.abs(V).T).max()
        if bias is not None:
            bu, bv, b0 = bias
            s = ((b0 + bu[self.users])[:, None] + bv[None, :]) + s
            t += 4 * EPS * (abs(b0) + np.abs(bu[self.users]).max() + np.abs(bv).max())
        if clamp is not None:
            s = np.clip(s, clamp[0], clamp[1])
        self.tol = max(self.tol, t)
        self.smax = max(self.smax, float(np.abs(s).max()))
        self.s1 = s.copy() if self.s1 is None else self.s1 + s
        self.s2 = s * s if self.s2 is None else self.s2 + s * s
        self.n += 1

    def check(self, L, what):
        e1 = e2 = 0.0
        rows = []
        for w in range(len(self.users)):
            mean, sd = L.watch_scores(w)
            rows.append((mean, sd))
            e1 = max(e1, float(np.abs(mean - self.s1[w] / self.n).max()))
            e2 = max(e2, float(np.abs(sd * sd + mean * mean - self.s2[w] / self.n).max()))
        b2 = 2 * self.smax * self.tol
        print("%s: n_w=%d  max|mean err| %.3e (bound %.3e)  max|2nd moment err| %.3e (bound %.3e)"
              % (what, self.n, e1, self.tol, e2, b2))
        assert e1 <= self.tol, (what, e1, self.tol)
        assert e2 <= b2, (what, e2, b2)
        return rows


def step_and_check(L, M, sweeps, what, bias=False, clamp=None):
    rows = None
    for s in range(sweeps):
        L.learn(sweeps=1)
        U, V = L.factors()
        M.add(U, V, L.biases() if bias else None, clamp)
        rows = M.check(L, "%s sweep %d" % (what, s + 1))
        if s == 0:
            for _, sd in rows:
                assert np.all(sd == 0.0), "one sample has no spread"
    return rows


# ---- 1. the scores follow the chain
@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("rng", ["ref", "philox"])
def test_scores_follow_the_chain(ml100k, rng, precision):
    tr, te = ml100k
    users = watch_ids(tr, 943, 37)
    L = FMLearnSBPMF(num_factor=20, seed=3, rng=rng, precision=precision)
    L.set_data(Data(*tr), Data(*te))
    L.watch(users)
    step_and_check(L, Moments(users, 20), 4, "%s/%s" % (rng, precision))
    L.close()


# ---- 2. the overlapped schedule (the next sweep's user half must not overtake the scoring)
def test_overlapped_schedule(ml100k):
    tr, te = ml100k
    users = watch_ids(tr, 943, 37)
    kw = dict(num_factor=20, seed=5, rng="philox")
    L = FMLearnSBPMF(pipeline=1, **kw)
    L.set_data(Data(*tr), Data(*te))
    L.watch(users)
    L.learn(sweeps=4)
    twin, M = FMLearnSBPMF(**kw), Moments(users, 20)
    twin.set_data(Data(*tr), Data(*te))
    for _ in range(4):
        twin.learn(sweeps=1)
        M.add(*twin.factors())
    M.check(L, "pipeline=1, 4 sweeps in one run")
    assert np.array_equal(np.array(L.factors()[0]), np.array(twin.factors()[0]))
    L.close()
    twin.close()


# ---- 3. agreement with sbmf_predict (clamped watch; "bias2" covers the bias path)
@pytest.mark.parametrize("quirks", ["final", "bias2"])
def test_agrees_with_predict(ml100k, quirks):
    tr, _ = ml100k
    users = watch_ids(tr, 943, 3)
    J = 1682
    te = Data(np.repeat(users, J), np.tile(np.arange(J, dtype=np.uint32), 3), np.full(3 * J, 3.0))
    L = FMLearnSBPMF(num_factor=20, seed=2, quirks=quirks, burnin=0)
    L.set_data(Data(*tr), te)
    assert L.dims()[:2] == (943, J)
    L.watch(users, clamp=True)
    lo = 0.5 if quirks == "bias2" else 1.0
    M = Moments(users, 20)
    step_and_check(L, M, 5, "clamped/" + quirks, bias=quirks == "bias2", clamp=(lo, 5.0))
    pred = L.predict().reshape(3, J)
    mean = np.array([L.watch_scores(w)[0] for w in range(3)])
    err = float(np.abs(pred - mean).max())
    print("predict vs watch mean (%s): max err %.3e (bound %.3e)" % (quirks, err, M.tol))
    assert err <= M.tol
    L.close()


# ---- 4. selection
def check_selection(L, users, tr, topn, risk, exclude):
    items, mean, sd = L.recommend(topn=topn, exclude_rated=exclude, risk=risk)
    assert items.shape == mean.shape == sd.shape == (len(users), topn) and items.dtype == np.int64
    for w, u in enumerate(users):
        m, s = L.watch_scores(w)
        rated = tr[1][tr[0] == u]
        want = expected_topn(m, s, rated, topn, risk, exclude)
        assert np.array_equal(items[w], want), (w, int(u), topn, risk, exclude)
        real = want >= 0
        assert np.array_equal(mean[w][real], m[want[real]]) and np.array_equal(sd[w][real], s[want[real]])
        assert np.all(np.isnan(mean[w][~real])) and np.all(np.isnan(sd[w][~real]))
        if exclude:
            assert not np.intersect1d(items[w][real], rated).size


@pytest.fixture(scope="module")
def chain37(ml100k):
    tr, te = ml100k
    users = watch_ids(tr, 943, 37)
    L = FMLearnSBPMF(num_factor=20, seed=3, rng="philox")
    L.set_data(Data(*tr), Data(*te))
    L.watch(users)
    L.learn(sweeps=4)
    yield L, users, tr
    L.close()


@pytest.mark.parametrize("exclude", [True, False])
@pytest.mark.parametrize("risk", [0.0, 1.0])
@pytest.mark.parametrize("topn", [1, 10, 1024])
def test_selection_is_the_lexsort(chain37, topn, risk, exclude):
    L, users, tr = chain37
    check_selection(L, users, tr, topn, risk, exclude)


def test_selection_with_many_exact_ties(ml100k):
    tr, te = ml100k
    users = watch_ids(tr, 943, 37)
    L = FMLearnSBPMF(num_factor=20, seed=3, rng="philox", clamp_hi=3.0)
    L.set_data(Data(*tr), Data(*te))
    L.watch(users, clamp=True)
    L.learn(sweeps=3)
    ties = max(int((L.watch_scores(w)[0] == 3.0).sum()) for w in range(len(users)))
    print("largest number of items tied at the clamp: %d" % ties)
    assert ties > 1024 // 8
    for topn in (10, 1024):
        check_selection(L, users, tr, topn, 0.0, True)
    L.close()


def test_empty_slots_on_a_hand_made_set():
    tr = (np.array([0, 0, 0, 1, 2, 2], np.uint32), np.array([0, 1, 2, 3, 4, 0], np.uint32),
          np.array([5.0, 3.0, 4.0, 2.0, 1.0, 4.0]))
    L = FMLearnSBPMF(num_factor=8, seed=1)
    L.set_data(Data(*tr), Data(*tr))
    assert L.dims()[:2] == (3, 5)
    L.watch([0, 1, 2])
    L.learn(sweeps=2)
    items, mean, sd = L.recommend(topn=4)
    assert sorted(items[0][:2]) == [3, 4] and list(items[0][2:]) == [-1, -1]
    assert np.all(np.isfinite(mean[0][:2])) and np.all(np.isnan(mean[0][2:])) and np.all(np.isnan(sd[0][2:]))
    check_selection(L, np.array([0, 1, 2]), tr, 4, 0.0, True)
    L.close()


def test_selection_beyond_the_register_row(ml100k):
    """More than 32768 items: the selection forms its keys from memory on every pass."""
    tr, te = ml100k
    users = watch_ids(tr, 943, 5)
    L = FMLearnSBPMF(num_factor=8, seed=4, rng="philox")
    L.set_data(Data(*tr), Data(*te), num_items=33_001)
    L.watch(users)
    step_and_check(L, Moments(users, 8), 2, "J=33001")
    for topn, risk in ((10, 0.0), (1024, 1.0)):
        check_selection(L, users, tr, topn, risk, True)
    L.close()


# ---- 5. more than one block in both directions; the other users-per-workgroup shapes
def test_several_blocks_each_way():
    tr, te, (I, J) = synth.generate("ml-2k")
    users = watch_ids(tr, I, 130)
    L = FMLearnSBPMF(num_factor=100, seed=1, rng="philox")
    L.set_data(Data(*tr), Data(*te), num_users=I, num_items=J)
    L.watch(users)
    step_and_check(L, Moments(users, 100), 2, "ml-2k K=100")
    L.close()


@pytest.mark.parametrize("K", [120, 250])  # Kp 128: 32 users per workgroup; Kp 256: 16
def test_wide_factors(ml100k, K):
    tr, te = ml100k
    users = watch_ids(tr, 943, 37)
    L = FMLearnSBPMF(num_factor=K, seed=1, rng="philox")
    L.set_data(Data(*tr), Data(*te))
    L.watch(users)
    step_and_check(L, Moments(users, K), 2, "K=%d" % K)
    L.close()


# ---- 6. the chain is untouched
@pytest.mark.parametrize("rng", ["ref", "philox"])
def test_chain_is_untouched(ml100k, rng):
    tr, te = ml100k
    out = []
    for watched in (False, True):
        L = FMLearnSBPMF(num_factor=20, seed=11, rng=rng)
        L.set_data(Data(*tr), Data(*te))
        if watched:
            L.watch(watch_ids(tr, 943, 37))
        L.learn(sweeps=5)
        out.append((L.rmse_trajectory, *L.factors(), L.predict()))
        L.close()
    for a, b in zip(*out):
        assert np.array_equal(a, b)


# ---- 7. reproducible
def test_rerun_is_bit_identical(ml100k):
    tr, te = ml100k
    users = watch_ids(tr, 943, 37)
    out = []
    for _ in range(2):
        L = FMLearnSBPMF(num_factor=20, seed=9, rng="philox")
        L.set_data(Data(*tr), Data(*te))
        L.watch(users)
        L.learn(sweeps=3)
        rows = [np.stack(L.watch_scores(w)) for w in range(len(users))]
        out.append(rows + list(L.recommend(topn=50, risk=0.5)))
        L.close()
    for a, b in zip(*out):
        assert np.array_equal(a, b, equal_nan=True)


# ---- 8. errors and resources
def _code(fn, *a, **k):
    with pytest.raises(SBMFError) as ei:
        fn(*a, **k)
    return ei.value.code, str(ei.value)


def test_errors_and_resources(ml100k):
    tr, te = ml100k
    base = {k: device_usage()[k] for k in COUNTS}
    L = FMLearnSBPMF(num_factor=20, seed=1, rng="philox")
    L.set_data(Data(*tr), Data(*te))
    assert _code(L.watch, [0, 943])[0] == SBMF_E_ARG
    assert _code(L.recommend, topn=5)[0] == SBMF_E_STATE  # no list
    held0 = device_usage()["dev_allocs"]
    L.watch([1, 2, 2, 3])
    assert device_usage()["dev_allocs"] == held0 + 3
    assert _code(L.recommend, topn=5)[0] == SBMF_E_STATE  # no sweep accumulated
    assert _code(L.watch_scores, 0)[0] == SBMF_E_STATE
    L.learn(sweeps=2)
    assert _code(L.recommend, topn=0)[0] == SBMF_E_ARG
    assert _code(L.recommend, topn=1025)[0] == SBMF_E_ARG
    assert _code(L.watch_scores, 4)[0] == SBMF_E_ARG
    a, b = L.watch_scores(1), L.watch_scores(2)  # a duplicated id gives duplicate rows
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[1].max() > 0
    t = L.watch_timing()
    assert t["ms_score"] > 0 and t["ms_select"] == 0
    L.recommend(topn=5)
    assert L.watch_timing()["ms_select"] > 0
    # registering again zeroes the sums and the count
    L.watch([1, 2, 2, 3])
    L.learn(sweeps=1)
    U, V = L.factors()
    mean, sd = L.watch_scores(0)
    assert np.all(sd == 0.0) and np.abs(mean - U[1] @ V.T).max() <= 4 * 20 * EPS * (np.abs(U[1]) @ np.abs(V).T).max()
    L.watch([])
    assert device_usage()["dev_allocs"] == held0
    assert _code(L.recommend, topn=5)[0] == SBMF_E_STATE
    L.close()
    for kw in (dict(method="vb", num_factor=8), dict(order="libfm", num_factor=8)):
        O = FMLearnSBPMF(seed=1, **kw)
        O.set_data(Data(*tr), Data(*te))
        code, msg = _code(O.watch, [0])
        assert code == SBMF_E_STATE and "SBPMF sampler" in msg
        assert _code(O.recommend, topn=5)[0] == SBMF_E_STATE
        O.close()
    W = FMLearnSBPMF(num_factor=20, seed=1, rng="philox")  # closed with a live list
    W.set_data(Data(*tr), Data(*te))
    W.watch([5, 6])
    W.learn(sweeps=1)
    W.recommend(topn=3)
    W.close()
    assert {k: device_usage()[k] for k in COUNTS} == base


# ---- 9. the command line
def test_cli_recommend(tmp_path):
    trf, tef = write_m1m100k_libfm(tmp_path)
    ids = [0, 17, 942]
    (tmp_path / "ids").write_text("".join("%d\n" % u for u in ids))
    out = tmp_path / "out"
    r = subprocess.run([CLI_PATH, "-task", "r", "-train", trf, "-test", tef, "-method", "mcmc", "-order", "sbpmf",
                        "-dim", "0,0,8", "-iter", "3", "-recommend", str(out), "-rec_users", str(tmp_path / "ids"),
                        "-rec_topn", "5"], capture_output=True, text=True, timeout=120, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr
    rows = [l.split("\t") for l in out.read_text().splitlines()]
    assert len(rows) == 5 * len(ids) and all(len(x) == 4 for x in rows)
    train = set()
    with open(trf) as f:
        for line in f:
            p = line.split()
            train.add((int(p[1].split(":")[0]), int(p[2].split(":")[0])))
    for k, u in enumerate(ids):
        mine = rows[5 * k:5 * k + 5]
        assert [int(x[0]) for x in mine] == [u] * 5
        assert all(943 <= int(x[1]) < 943 + 1682 for x in mine)
        means = [float(x[2]) for x in mine]
        assert means == sorted(means, reverse=True) and all(float(x[3]) >= 0 for x in mine)
        assert not any((u, int(x[1])) in train for x in mine)
