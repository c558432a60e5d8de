"""The online VB learner's closed-form lists on the device: k_vb_score,
k_vb_pairs, k_vb_guest and the selection on given moments, through sbmf_vb_*.

Scoring, exact: the state comes from a numpy-written file of the exact construction
(tests/vb_posterior.py): every partial sum is exact in any order, so the MFMA's k permutation, the
three chains of k_vb_score, the 16-lane butterfly of k_vb_pairs and numpy agree bit for bit.
131 x 261 crosses one workgroup's 256 items and ends in a ragged tile of 5; K sits at the bounds
of vb_score_mu (Kp 32 | 48: 64 -> 32 rows a workgroup; 80 | 96: 32 -> 16), at the 64 KB of
dynamic LDS (Kp 160 | 176) and at one block of 16.

Guests: rows against the serial longdouble restatement; the allowance is 8 x the float64
restatement's own distance from it (the margin: the kernel's wave-partial sums against numpy's
serial ones), floored at 4 ulps of the row's largest entry.  Largest ratios seen: DESIGN.md 5.5."""
import numpy as np
import pytest

from conftest import gpu_available
from sample_files import expected_topn, same_bits
from sbmf import (SBMF_E_ARG, SBMF_E_STATE, Communicator, Data, FMLearnSBPMF, FMLearnVBOnline, SBMFError, device_usage)
from sbmf._lib import lib
from vb_posterior import (default_train, exact_state, guest_limit, guest_scan, make_guests, moments, open_with, smooth_state,
                          write_posterior)
import ctypes as C

pytestmark = pytest.mark.gpu

SEED = 41
EPS = 2.0 ** -52
KS = (1, 15, 16, 17, 32, 33, 80, 81, 100, 112, 113, 160, 161, 200, 240, 241, 256)
LENGTHS = (1, 15, 16, 17, 63, 64, 65, 131)
COUNTS = ("dev_bytes", "dev_allocs", "pinned_bytes", "pinned_allocs", "streams", "events", "contexts", "comms")


def _code(fn, *a, **kw):
    with pytest.raises(SBMFError) as ei:
        fn(*a, **kw)
    return ei.value.code, str(ei.value)


def usage():
    return {k: device_usage()[k] for k in COUNTS}


def kernel_moments(L, user, J):
    """one user's mean and variance as k_vb_score wrote them (sbmf_test_vb_moments)"""
    mean, var = np.zeros(J), np.zeros(J)
    dp = C.POINTER(C.c_double)
    L._check(lib.sbmf_test_vb_moments(L.ctx, int(user), mean.ctypes.data_as(dp), var.ctypes.data_as(dp)))
    return mean, var


def user_lists(I):
    """one list per length: ids 0 and I - 1 and a repeated id in each (from length 3 on)"""
    rng = np.random.default_rng([SEED, I, 2])
    out = []
    for n in LENGTHS:
        if n > I:
            continue
        ids = np.concatenate([[0, I - 1], 1 + rng.permutation(I - 2)])[:n] if n >= 2 else np.array([I - 1])
        if n >= 3:
            ids[-1] = ids[n // 2]
        out.append(ids.astype(np.uint32))
    return out


def check_lists(L, ids, mean, sd, rated, what, topns=(10, 1024), risks=(0.0, 0.5, 1.0)):
    for topn in topns:
        for exclude in (True, False):
            for risk in risks:
                it, m, s = L.vb_recommend(ids, topn=topn, exclude_rated=exclude, risk=risk)
                for w, u in enumerate(ids):
                    want = expected_topn(mean[u], sd[u], rated[u], topn, risk, exclude)
                    tag = "%s user %d topn %d exclude %s risk %g" % (what, u, topn, exclude, risk)
                    assert np.array_equal(it[w], want), tag
                    got = want >= 0
                    same_bits(m[w][got], mean[u][want[got]], tag + " mean")
                    same_bits(s[w][got], sd[u][want[got]], tag + " stdev")
                    assert np.isnan(m[w][~got]).all() and np.isnan(s[w][~got]).all(), tag


def scoring_case(I, J, K, full):
    assert gpu_available(), "these tests need a gfx950 device"
    base = usage()
    st = exact_state(I, J, K, SEED)
    train = default_train(I, J, SEED)
    rated = [train[1][train[0] == u] for u in range(I)]
    L = open_with(st, train)
    what = "I=%d J=%d K=%d" % (I, J, K)
    want_mean, want_var = moments(st, np.arange(I))
    mean, sd, ulp_used = np.zeros((I, J)), np.zeros((I, J)), False
    for u in range(I):
        km, kv = kernel_moments(L, u, J)
        same_bits(km, want_mean[u], what + " kernel mean of user %d" % u)
        same_bits(kv, want_var[u], what + " kernel variance of user %d" % u)
        mean[u], sd[u] = L.vb_scores(u)
        same_bits(mean[u], want_mean[u], what + " mean of user %d" % u)
        ref = np.sqrt(want_var[u])
        assert np.all(np.abs(sd[u] - ref) <= np.spacing(ref)), what
        ulp_used |= bool(np.any(sd[u] != ref))
    print("%s: the stdev's ulp was %s" % (what, "used" if ulp_used else "never used"))
    lists = user_lists(I)
    for ids in lists if full else lists[-1:]:
        check_lists(L, ids, mean, sd, rated, what)
    # pairs: 1,000 seeded ones and the four corners
    rng = np.random.default_rng(11)
    pu = np.concatenate([rng.integers(0, I, 1000), [0, 0, I - 1, I - 1]]).astype(np.uint32)
    pi = np.concatenate([rng.integers(0, J, 1000), [0, J - 1, 0, J - 1]]).astype(np.uint32)
    pm, ps = L.vb_predict(pu, pi)
    same_bits(pm, mean[pu, pi], what + " pair means")
    same_bits(ps, sd[pu, pi], what + " pair stdevs")
    # a second call is bit-identical
    ids = lists[-1]
    a, b = L.vb_recommend(ids, topn=10, risk=0.5), L.vb_recommend(ids, topn=10, risk=0.5)
    assert np.array_equal(a[0], b[0])
    same_bits(a[1], b[1], what + " rerun mean")
    same_bits(a[2], b[2], what + " rerun stdev")
    m2, s2 = L.vb_scores(I - 1)
    same_bits(m2, mean[I - 1], what + " rerun row")
    same_bits(s2, sd[I - 1], what + " rerun row stdev")
    if full and I > 128:  # sliced: a budget of 64 rows gives slices of 64 / 64 / 3
        assert lib.sbmf_test_vb_tune(L.ctx, 64 * 2 * ((J + 15) // 16 * 16) * 8) == 0
        c = L.vb_recommend(ids, topn=10, risk=0.5)
        assert lib.sbmf_test_vb_tune(L.ctx, 0) == 0
        assert len(ids) == 131 and np.array_equal(a[0], c[0])
        same_bits(a[1], c[1], what + " sliced mean")
        same_bits(a[2], c[2], what + " sliced stdev")
    t = L.vb_timing()
    assert t["ms_score"] > 0 and t["ms_select"] > 0 and t["ms_transpose"] > 0 and t["ms_guest"] == 0
    L.close()
    assert usage() == base


@pytest.mark.parametrize("K", KS)
def test_scoring_is_exact(K):
    scoring_case(131, 261, K, True)


@pytest.mark.parametrize("K", (16, 33))
def test_scoring_is_exact_on_a_small_shape(K):
    scoring_case(17, 129, K, False)


# ------------------------------------------------------------------ the selection on given moments
@pytest.mark.parametrize("J", (17, 1025, 32769))
def test_selection_ranks_by_the_given_variance(J):
    """K = 1, mu_u = 1, s_u = 0 and no bias or global spread: mean_j = mu_j and var_j = s_j exactly.
    Every item has var = 2^-40 mean^2 (sd = 2^-20 |mean|) but item B, whose mean is item A's and
    whose variance is four times A's: with risk 1, A (the higher id) has to come before B, decided
    by the variance alone.  k_watch_select's sums form would be fed s2 = var + mean^2 and take
    sd^2 = s2 - mean^2: at 2^-40 that difference keeps only the top 12 bits of the variance's 52
    (mean^2 (1 + 2^-40) rounds the rest away), so keys that differ below 2^-12 relative in sd tie; a
    second pair C, D sits at 2^-60 and 2^-58 of mean^2, below half an ulp of mean^2, where
    s2 == mean^2 in double and s2 - mean^2 returns 0 for both -- the order would fall to the ids."""
    assert gpu_available(), "these tests need a gfx950 device"
    I = 2
    rng = np.random.default_rng([SEED, J])
    mu = (16 + rng.integers(0, 64, J)) / 16.0  # in [1, 5)
    var = mu * mu * 2.0 ** -40
    A, B, Cc, D = J - 1, 3, J - 2, 5
    mu[A] = mu[B] = 6.0
    var[A], var[B] = 36.0 * 2.0 ** -40, 36.0 * 2.0 ** -38
    mu[Cc] = mu[D] = 5.5
    var[Cc], var[D] = 30.25 * 2.0 ** -60, 30.25 * 2.0 ** -58
    assert (var[Cc] + mu[Cc] ** 2) - mu[Cc] ** 2 == 0.0 and (var[D] + mu[D] ** 2) - mu[D] ** 2 == 0.0
    z = np.zeros
    st = dict(Um=np.ones((I, 1)), Us=z((I, 1)), Vm=mu[:, None], Vs=var[:, None], bum=z(I), bus=z(I), bvm=z(J), bvs=z(J),
              mu0=0.0, s0=0.0, alpha=1.0, sigma_0=1.0, sigma_w=1.0, sigma_v=np.ones(1))
    L = open_with(st, default_train(I, J, SEED))
    mean, sd = L.vb_scores(0)
    same_bits(mean, mu, "injected means")
    assert np.all(np.abs(sd - np.sqrt(var)) <= np.spacing(np.sqrt(var)))
    for topn in (4, 1024):
        it, m, s = L.vb_recommend([0, 0], topn=topn, exclude_rated=False, risk=1.0)
        want = expected_topn(mean, sd, [], topn, 1.0, False)
        assert np.array_equal(it[0], want) and np.array_equal(it[1], want)
        assert list(it[0][:4]) == [A, B, Cc, D]  # the smaller spread first, against the ids' order
        got = want >= 0
        same_bits(s[0][got], sd[want[got]], "selected stdevs")
    it, _, _ = L.vb_recommend([0], topn=4, exclude_rated=False, risk=0.0)
    assert list(it[0]) == [B, A, D, Cc]  # without the spread the ids decide
    L.close()


# ------------------------------------------------------------------ tied to the learner
def _learner(tr, te, K):
    L = FMLearnVBOnline(num_factor=K, seed=1)
    L.set_data(Data(*tr), Data(*te))
    return L


@pytest.mark.parametrize("K", (8, 20))
def test_lists_follow_the_learner(ml100k, tmp_path, K):
    assert gpu_available(), "these tests need a gfx950 device"
    base = usage()
    tr, te = ml100k
    plain = _learner(tr, te, K)
    plain.learn(sweeps=1)
    plain.learn(sweeps=1)
    L = _learner(tr, te, K)
    users = np.array([0, 5, 942, 5], np.uint32)
    before = L.vb_recommend(users, topn=5)  # before any epoch: the initial state, valid and repeatable
    again = L.vb_recommend(users, topn=5)
    assert np.array_equal(before[0], again[0]) and (before[0] >= 0).all() and np.isfinite(before[2]).all()
    L.learn(sweeps=1)
    L.vb_recommend(users, topn=5)
    L.vb_predict(te[0][:100], te[1][:100])
    L.vb_foldin_recommend([(tr[1][tr[0] == 0], tr[2][tr[0] == 0])], topn=5, scans=2)
    L.learn(sweeps=1)
    same_bits(L.rmse_trajectory, plain.rmse_trajectory, "RMSE trajectory with vb_* calls between the epochs")
    # the posterior against factors(), biases(), hyper()
    P = L.vb_posterior()
    U, V = L.factors()
    bu, bv, b0 = L.biases()
    hy = L.hyper()
    same_bits(P["U_mean"], U, "U means")
    same_bits(P["V_mean"], V, "V means")
    same_bits(P["bu_mean"], bu, "bu means")
    same_bits(P["bv_mean"], bv, "bv means")
    assert P["b0"][0] == b0 and P["alpha"] == hy["tau"] and np.array_equal(P["sigma_v"], hy["sigma_u"])
    for k in ("U_var", "V_var", "bu_var", "bv_var"):
        assert np.isfinite(P[k]).all() and (P[k] > 0).all(), k
    assert np.isfinite(P["b0"][1]) and P["b0"][1] > 0 and P["sigma_0"] > 0 and P["sigma_w"] > 0
    # the pair kernel against predict(): two summation orders of K products and three more terms
    lo, hi = float(np.float32(tr[2].min())), float(np.float32(tr[2].max()))
    pm, ps = L.vb_predict(te[0], te[1])
    bound = 4 * (K + 3) * EPS * ((np.abs(U[te[0]]) * np.abs(V[te[1]])).sum(axis=1) + np.abs(bu[te[0]]) + np.abs(bv[te[1]]) + abs(b0))
    err = np.abs(np.clip(pm, lo, hi) - L.predict())
    print("K=%d: max |clip(vb_predict) - predict| %.3e, its bound there %.3e" % (K, err.max(), bound[np.argmax(err)]))
    assert np.all(err <= bound)
    assert np.isfinite(ps).all() and (ps > 0).all()
    # rows against pairs
    m0, s0 = L.vb_scores(7)
    j = np.arange(V.shape[0], dtype=np.uint32)
    qm, qs = L.vb_predict(np.full(len(j), 7, np.uint32), j)
    tol = 4 * (K + 3) * EPS * ((np.abs(U[7]) * np.abs(V)).sum(axis=1) + abs(bu[7]) + np.abs(bv) + abs(b0))
    assert np.all(np.abs(m0 - qm) <= tol) and np.allclose(s0, qs, rtol=1e-12)
    # save, load into a fresh context with no epoch: the same lists, and no training from there
    path = tmp_path / "model.vb"
    L.save_vb_posterior(path)
    got = L.vb_recommend(users, topn=10, risk=0.5)
    guest = [(tr[1][tr[0] == 3], tr[2][tr[0] == 3])]
    gg = L.vb_foldin_recommend(guest, topn=10, scans=2)
    F = _learner(tr, te, K)
    F.load_vb_posterior(path)
    back = F.vb_recommend(users, topn=10, risk=0.5)
    assert np.array_equal(got[0], back[0])
    same_bits(got[1], back[1], "loaded model's means")
    same_bits(got[2], back[2], "loaded model's stdevs")
    gb = F.vb_foldin_recommend(guest, topn=10, scans=2)
    assert np.array_equal(gg[0], gb[0])
    same_bits(gg[1], gb[1], "loaded model's guest means")
    code, msg = _code(F.learn, sweeps=1)
    assert code == SBMF_E_STATE and "cannot resume" in msg
    # a guest whose ratings are a training user's: its list overlaps the user's
    urec = L.vb_recommend([3], topn=50)[0][0]
    grec = L.vb_foldin_recommend(guest, topn=50, scans=8)[0][0]
    overlap = len(set(urec) & set(grec))
    print("K=%d: user 3's top-50 and its guest twin's share %d items" % (K, overlap))
    assert overlap > 0
    for X in (plain, L, F):
        X.close()
    assert usage() == base


# ------------------------------------------------------------------ guests
GUEST_LENGTHS = (0, 1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1025)  # 256: one trip of the workgroup over the ratings
GUEST_J = 1100
_guest_cache = {}


def guest_setup(K):
    """per K: the state, the guests, the learner; the restatements once per (K, scans)"""
    if K not in _guest_cache:
        st = smooth_state(4, GUEST_J, K, 77)
        _guest_cache[K] = (st, make_guests(GUEST_J, GUEST_LENGTHS, K), {})
    return _guest_cache[K]


def ulps_of(x):
    return np.spacing(np.abs(x).max()) if np.abs(x).max() > 0 else 5e-324


@pytest.mark.parametrize("scans", (1, 2, 64))
@pytest.mark.parametrize("K", (1, 16, 17, 100, 200))
def test_guest_rows_follow_the_restatement(K, scans):
    assert gpu_available(), "these tests need a gfx950 device"
    base = usage()
    st, guests, refs = guest_setup(K)
    L = open_with(st, default_train(4, GUEST_J, SEED))
    rm, rv, bm, bv = L.vb_foldin_rows(guests, scans=scans)
    rm2, rv2, bm2, bv2 = L.vb_foldin_rows(guests, scans=scans)
    same_bits(rm, rm2, "rerun rows")
    same_bits(bm, bm2, "rerun biases")
    f64 = guest_scan(st, guests, scans)
    ld = guest_scan(st, guests, scans, np.longdouble)
    worst = 0.0
    for q, (it, r) in enumerate(guests):
        row = np.concatenate([[bm[q]], rm[q]]).astype(np.longdouble)
        ref = np.concatenate([[ld[2][q]], ld[0][q]])
        own = np.concatenate([[f64[2][q]], f64[0][q]]).astype(np.longdouble)
        allow = max(8 * float(np.abs(own - ref).max()), 4 * float(ulps_of(np.asarray(ref, np.float64))))
        err = float(np.abs(row - ref).max())
        worst = max(worst, err / allow)
        print("K=%d scans=%d n=%d: |row - longdouble| %.3e, allowance %.3e (ratio %.3f)" % (K, scans, len(it), err, allow, err / allow))
        assert err <= allow, (K, scans, len(it), err, allow)
        # variances: 1 / P within 2 ulps
        want_v = np.concatenate([[ld[3][q]], ld[1][q]]).astype(np.float64)
        got_v = np.concatenate([[bv[q]], rv[q]])
        assert np.all(np.abs(got_v - want_v) <= 2 * np.spacing(want_v)), (K, scans, len(it))
        if len(it) == 0:  # the prior exactly
            assert not rm[q].any() and bm[q] == 0.0
            same_bits(rv[q], 1 / st["sigma_v"], "prior variances")
            assert bv[q] == 1 / st["sigma_w"]
        if scans == 64:
            bl, gl = guest_limit(st, it, r)
            lim = np.concatenate([[bl], gl])
            assert np.abs(np.asarray(row, np.float64) - lim).max() <= 1e-10 * max(np.abs(lim).max(), 1e-300), (K, len(it))
    print("K=%d scans=%d: largest error / allowance %.3f" % (K, scans, worst))
    assert L.vb_timing()["ms_guest"] > 0
    L.close()
    assert usage() == base


def test_guest_lists_leave_out_the_guests_own_items():
    assert gpu_available(), "these tests need a gfx950 device"
    K = 17
    st, guests, _ = guest_setup(K)
    L = open_with(st, default_train(4, GUEST_J, SEED))
    it, m, s = L.vb_foldin_recommend(guests, topn=1024, scans=2)
    kept, km, ks = L.vb_foldin_recommend(guests, topn=1024, scans=2, exclude_rated=False)
    rm, rv, bm, bv = L.vb_foldin_rows(guests, scans=2)
    for q, (own, _) in enumerate(guests):
        assert not set(it[q][it[q] >= 0]) & set(int(x) for x in own), q
        mean, sd = L.vb_foldin_scores(own, guests[q][1], scans=2)
        assert np.array_equal(it[q], expected_topn(mean, sd, own, 1024, 0.0, True)), q
        assert np.array_equal(kept[q], expected_topn(mean, sd, own, 1024, 0.0, False)), q
        # the guest's row, scored on the host in the stated association
        gs = dict(st, Um=rm[q][None], Us=rv[q][None], bum=bm[q:q + 1], bus=bv[q:q + 1])
        wm, wv = moments(gs, [0])
        tol = 4 * (K + 3) * EPS * (np.abs(rm[q]) @ np.abs(st["Vm"]).T + abs(bm[q]) + np.abs(st["bvm"]) + abs(st["mu0"]))
        assert np.all(np.abs(mean - wm[0]) <= tol) and np.allclose(sd, np.sqrt(wv[0]), rtol=1e-12), q
    # sliced: 12 guests in one slice of 64 whatever the budget; the call is stateless
    again = L.vb_foldin_recommend(guests, topn=1024, scans=2)
    assert np.array_equal(again[0], it)
    same_bits(again[1], m, "rerun guest means")
    L.close()


# ------------------------------------------------------------------ refusals and resources
def test_refusals_and_resources(ml100k, tmp_path):
    assert gpu_available(), "these tests need a gfx950 device"
    base = usage()
    tr, te = ml100k
    guest = [([1, 2], [3.0, 4.0])]
    # a context that is not VB
    for kw in (dict(), dict(method="mcmc", order="libfm"), dict(method="als")):
        O = FMLearnSBPMF(num_factor=8, seed=1, **kw)
        O.set_data(Data(*tr), Data(*te))
        for fn, args in ((O.vb_posterior, ()), (O.vb_scores, (0,)), (O.vb_recommend, ([0],)), (O.vb_predict, ([0], [0])),
                         (O.vb_foldin_rows, (guest,)), (O.vb_foldin_scores, ([1], [3.0])), (O.vb_foldin_recommend, (guest,)),
                         (O.save_vb_posterior, (tmp_path / "x",)), (O.load_vb_posterior, (tmp_path / "x",)), (O.vb_timing, ())):
            code, msg = _code(fn, *args)
            assert code == SBMF_E_STATE and "online VB" in msg, (kw, msg)
        O.close()
    R = FMLearnSBPMF(num_factor=8, seed=1, rng="philox")  # a virtual rank is the SBPMF sampler's
    R.init()
    assert lib.sbmf_test_virtual_rank(R.ctx, 2, 0) == 0
    R.set_data(Data(*tr), Data(*te))
    code, msg = _code(R.vb_recommend, [0])
    assert code == SBMF_E_STATE
    R.close()
    comm = Communicator(1, 0, bytes(128))  # a context that joined a communicator, even one of a single rank
    N = FMLearnVBOnline(num_factor=8, seed=1)
    N.init(comm=comm)
    for fn, args in ((N.vb_scores, (0,)), (N.vb_recommend, ([0],)), (N.vb_predict, ([0], [0])), (N.vb_foldin_rows, (guest,)),
                     (N.vb_posterior, ()), (N.save_vb_posterior, (tmp_path / "x",))):
        code, msg = _code(fn, *args)
        assert code == SBMF_E_STATE and "joined a communicator" in msg, msg
    N.close()
    comm.close()
    U = FMLearnVBOnline(num_factor=8, seed=1)  # not prepared
    U.init()
    code, msg = _code(U.vb_recommend, [0])
    assert code == SBMF_E_STATE and "not prepared" in msg
    U.close()
    # argument errors on a VB context; the existing refusals, unchanged
    L = FMLearnVBOnline(num_factor=8, seed=1)
    L.set_data(Data(*tr), Data(*te))
    I, J = L.dims()[:2]
    for fn, args, kw, word in ((L.vb_recommend, ([0],), dict(topn=0), "topn"), (L.vb_recommend, ([0],), dict(topn=1025), "topn"),
                               (L.vb_recommend, ([I],), {}, "users[0]"), (L.vb_scores, (I,), {}, "users[0]"),
                               (L.vb_predict, ([I], [0]), {}, "users[0]"), (L.vb_predict, ([0], [J]), {}, "items[0]"),
                               (L.vb_foldin_rows, (guest,), dict(scans=0), "scans"), (L.vb_foldin_rows, (guest,), dict(scans=65), "scans"),
                               (L.vb_foldin_recommend, (guest,), dict(scans=65), "scans"),
                               (L.vb_foldin_recommend, (guest,), dict(topn=1025), "topn"),
                               (L.vb_foldin_recommend, ([([J], [3.0])],), {}, "items[0]"),
                               (L.vb_foldin_scores, ([J], [3.0]), {}, "items[0]"), (L.vb_foldin_scores, ([1], [3.0]), dict(scans=0), "scans")):
        code, msg = _code(fn, *args, **kw)
        assert code == SBMF_E_ARG and word in msg, msg
    ids = np.zeros(1, np.uint32)
    out_i, out_d = np.zeros(4, np.uint32), np.zeros(4)
    up, dp = C.POINTER(C.c_uint32), C.POINTER(C.c_double)
    for flags in (2, 3):  # a clamp bit is an argument error
        rc = lib.sbmf_vb_recommend(L.ctx, 1, ids.ctypes.data_as(up), 4, flags, 0.0, out_i.ctypes.data_as(up),
                                   out_d.ctypes.data_as(dp), None)
        assert rc == SBMF_E_ARG and b"no clamp" in lib.sbmf_last_error(L.ctx)
    for fn, args in ((L.watch, ([0],)), (L.foldin, (guest,)), (L.keep_samples, ())):
        code, msg = _code(fn, *args)
        assert code == SBMF_E_STATE and "online VB" in msg and "SBPMF sampler" in msg, msg
    code, msg = _code(L.set_factors, np.zeros((I, 8)), np.zeros((J, 8)))
    assert code == SBMF_E_STATE
    # files: other dims, a truncated file, a wrong magic -- and no partial load
    before = L.vb_recommend([0, 1], topn=5)
    write_posterior(tmp_path / "small.vb", exact_state(5, 9, 8, 1))
    code, msg = _code(L.load_vb_posterior, tmp_path / "small.vb")
    assert code == SBMF_E_ARG and "5 users, 9 items and 8 factors" in msg
    L.save_vb_posterior(tmp_path / "ok.vb")
    good = (tmp_path / "ok.vb").read_bytes()
    (tmp_path / "short.vb").write_bytes(good[:-8])
    (tmp_path / "magic.vb").write_bytes(b"SBMFSMP\n" + good[8:])
    for name, word in (("short.vb", "truncated"), ("magic.vb", "bad magic"), ("missing.vb", "cannot open")):
        code, msg = _code(L.load_vb_posterior, tmp_path / name)
        assert code != 0 and word in msg, msg
    after = L.vb_recommend([0, 1], topn=5)
    assert np.array_equal(before[0], after[0])
    same_bits(before[1], after[1], "means after refused loads")
    L.learn(sweeps=1)  # a refused load leaves training possible
    L.close()
    assert usage() == base


# ------------------------------------------------------------------ the association of the epilogue
@pytest.mark.parametrize("I,J", ((19, 37), (131, 261)))
def test_epilogue_follows_the_stated_association(I, J):
    """On the exact construction every association of the epilogue gives the same bits.  Here K = 1,
    the users' factor variance is 0 and every other number is continuous: d = mu_u mu_j and tv =
    (mu_u mu_u) s_j are one rounded product each (the MFMA adds them to 0), so the returned mean has
    to be ((d + bu) + bv) + mu0 and the variance ((tv + su) + sv) + s0 bit for bit; any other order
    of the three additions differs on most of these rows.  The pair kernel has to give the same bits."""
    assert gpu_available(), "these tests need a gfx950 device"
    rng = np.random.default_rng([SEED, I, J, 9])
    st = dict(Um=rng.standard_normal((I, 1)), Us=np.zeros((I, 1)), Vm=rng.standard_normal((J, 1)), Vs=rng.uniform(0.1, 2.0, (J, 1)),
              bum=rng.standard_normal(I), bus=rng.uniform(0.01, 1.0, I), bvm=rng.standard_normal(J), bvs=rng.uniform(0.01, 1.0, J),
              mu0=float(rng.standard_normal()) + 3.0, s0=float(rng.uniform(0.01, 1.0)), alpha=1.5, sigma_0=1.0, sigma_w=1.0,
              sigma_v=np.ones(1))
    want_mean, want_var = moments(st, np.arange(I))
    d = st["Um"] * st["Vm"].T  # [I][J]
    other = (d + (st["bum"][:, None] + st["bvm"][None, :])) + st["mu0"]
    assert np.mean(other != want_mean) > 0.05  # the inputs do tell the orders apart (about a tenth of the slots differ)
    L = open_with(st, default_train(I, J, SEED))
    for u in range(I):
        km, kv = kernel_moments(L, u, J)
        same_bits(km, want_mean[u], "mean of user %d" % u)
        same_bits(kv, want_var[u], "variance of user %d" % u)
        j = np.arange(J, dtype=np.uint32)
        pm, ps = L.vb_predict(np.full(J, u, np.uint32), j)
        same_bits(pm, want_mean[u], "pair means of user %d" % u)
        ref = np.sqrt(want_var[u])
        assert np.all(np.abs(ps - ref) <= np.spacing(ref))
    L.close()


# ------------------------------------------------------------------ the command line
def test_cli_writes_and_serves_the_model(ml100k, tmp_path):
    """-method vb with -vb_model_out and both lists, then -vb_model_in serving the same lists and -out
    with no epoch: every line equals the Python lists of a learner run alike, the '#Model' line's
    RMSE and -out are the clamped posterior-mean prediction."""
    import subprocess

    from sbmf import save_triples
    from sbmf._lib import CLI_PATH
    assert gpu_available(), "these tests need a gfx950 device"
    tr, te = ml100k
    K, topn, risk, scans = 8, 5, 0.5, 2
    save_triples(tmp_path / "train", Data(*tr))
    save_triples(tmp_path / "test", Data(*te))
    users = [0, 17, 942, 17]
    (tmp_path / "users").write_text("".join("%d\n" % u for u in users))
    guests = [(tr[1][tr[0] == 3][:40], tr[2][tr[0] == 3][:40]), (np.zeros(0, np.uint32), np.zeros(0)), (tr[1][tr[0] == 9], tr[2][tr[0] == 9])]
    (tmp_path / "guests").write_text("".join("%d %d %g\n" % (g, i, r) for g, (it, rt) in enumerate(guests) for i, r in zip(it, rt)))
    base = [CLI_PATH, "-task", "r", "-method", "vb", "-train", str(tmp_path / "train"), "-test", str(tmp_path / "test"), "-dim",
            "1,1,%d" % K, "-iter", "2", "-seed", "1", "-vb_users", str(tmp_path / "users"), "-vb_guests", str(tmp_path / "guests"),
            "-vb_topn", str(topn), "-vb_risk", str(risk), "-vb_scans", str(scans)]

    def lists(tag):
        return base + ["-vb_recommend", str(tmp_path / ("u_" + tag)), "-vb_recommend_guests", str(tmp_path / ("g_" + tag))]

    r1 = subprocess.run(lists("run") + ["-vb_model_out", str(tmp_path / "model")], capture_output=True, text=True, timeout=300, cwd=tmp_path)
    assert r1.returncode == 0, r1.stderr
    r2 = subprocess.run(lists("file") + ["-vb_model_in", str(tmp_path / "model"), "-out", str(tmp_path / "pred")], capture_output=True,
                        text=True, timeout=300, cwd=tmp_path)
    assert r2.returncode == 0, r2.stderr
    assert "#Iter" not in r2.stdout  # no epoch
    L = FMLearnVBOnline(num_factor=K, seed=1)
    L.set_data(Data(*tr), Data(*te))
    L.learn(sweeps=2)

    def want(rows, ids, out):
        it, m, s = out
        return ["%s\t%d\t%.17g\t%.17g" % (ids[w] if ids else w, it[w][k], m[w][k], s[w][k]) for w in range(rows)
                for k in range(topn) if it[w][k] >= 0]

    wu = want(len(users), users, L.vb_recommend(users, topn=topn, risk=risk))
    wg = want(len(guests), None, L.vb_foldin_recommend(guests, topn=topn, risk=risk, scans=scans))
    assert len(wu) == len(users) * topn and len(wg) == len(guests) * topn
    for tag in ("run", "file"):
        assert (tmp_path / ("u_" + tag)).read_text().splitlines() == wu, tag
        assert (tmp_path / ("g_" + tag)).read_text().splitlines() == wg, tag
    lo, hi = float(np.float32(tr[2].min())), float(np.float32(tr[2].max()))
    pred = np.clip(L.vb_predict(te[0], te[1])[0], lo, hi)
    got = np.array([float(x) for x in (tmp_path / "pred").read_text().split()])
    assert np.allclose(got, pred, rtol=1e-5, atol=0)  # -out prints six significant digits
    line = [x for x in r2.stdout.splitlines() if x.startswith("#Model\tTest=")]
    assert len(line) == 1
    assert abs(float(line[0].split("=")[1]) - np.sqrt(np.mean((pred - te[2]) ** 2))) < 1e-5
    info = __import__("sbmf").vb_posterior_file_info(tmp_path / "model")
    assert info["num_factor"] == K and info["num_users"] == 943 and info["num_items"] == 1682
    L.close()
