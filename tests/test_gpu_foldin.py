"""Fold-in users: posterior top-N for users outside the training set (sbmf_foldin_users /
sbmf_foldin_factors / sbmf_foldin_scores / sbmf_foldin_recommend, include/sbmf.h; the row
kernel in csrc/foldin.hip, scores and selection by the watch list's kernels).

The reference has nothing of the kind.  The checker of the draw is the header's coordinate
loop restated in numpy on what the library returns after every sweep: V (factors()),
sigma_u / mu_u / tau (hyper()), the rows the previous sweep left (foldin_factors()) and the
normals sbmf_philox_normals(seed, sweep, 7, g, K).  Restarting from the returned rows every
sweep keeps rounding from compounding.

Tolerance of the draw (derived, not fitted), per sweep:
  tol = max(64 * max|restatement in float64 - the same in np.longdouble|,
            K * n_max * 2^-52 * max|u|)          (+ 2^-24 max|u| in an F32 context: one rounding on store)
The first term measures the conditioning of the step on those very inputs; the factor 64
allows for the kernel's blocked summation order (Gram blocks of 16 columns, 16 waves);
n_max is the longest guest list.  The device's normals agree with the host's to the last
bits of log / sincos, far inside the floor.  Each comparison prints the observed error next
to its bound.

Scores use the tolerance of test_gpu_recommend.py (the same kernel): 4 K eps max sum|u v|.

ML-100k is 943 x 1682; K = 20 gives Kp = 32 (padding inside the second block)."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from conftest import write_m1m100k_libfm
from edge_rows import restate_row as restate  # the header's coordinate loop for one row in a floating type
from sample_files import expected_topn  # the selection's order: one copy for the list tests
from sbmf import (SBMF_E_ARG, SBMF_E_STATE, Data, FMLearnSBPMF, SBMFError, device_usage, philox_normals)
from sbmf._lib import CLI_PATH, lib

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
J = 1682
TAG_GUEST = 7
COUNTS = ("dev_bytes", "dev_allocs", "pinned_bytes", "pinned_allocs", "streams", "events", "contexts", "comms")
# the vector (4), wave (64) and 256-rating boundaries, the Gram pass's trip (16 waves x 8 vectors
# of 4 = 512 ratings), the one-thread-per-rating passes' trip (1024), and n_g = J
LENGTHS = (0, 1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1025, J)
THIN = (0, 5, 65, 257, J)


def make_guests(tr, lengths, seed=5, repeats=True):
    """One guest per length (distinct items; the J-long one lists every item once), ratings
    drawn from the training set's values; then a guest whose list repeats an item, and one
    longer than J (every item, 18 of them twice)."""
    rng = np.random.default_rng(seed)
    out = []
    for n in lengths:
        items = rng.permutation(J)[:n].astype(np.uint32)
        out.append((items, rng.choice(tr[2], n)))
    if repeats:
        out.append((np.array([7, 100, 7, 1681, 7, 0], np.uint32), np.array([5.0, 3.0, 4.0, 1.0, 5.0, 2.0])))
        items = np.concatenate([rng.permutation(J), rng.permutation(J)[:18]]).astype(np.uint32)
        out.append((items, rng.choice(tr[2], len(items))))
    return out


def step_draw(L, guests, prev, sweep, seed, K, sd_is_var, f32, what):
    """One sweep, then the restated draw of every guest against foldin_factors()."""
    L.learn(sweeps=1)
    _, V = L.factors()
    h = L.hyper()
    G = L.foldin_factors()
    assert G.shape == (len(guests), K)
    want = np.zeros_like(G)
    cond = 0.0
    for g, (items, r) in enumerate(guests):
        z = philox_normals(seed, sweep, TAG_GUEST, g, K)
        a = restate(V, h["sigma_u"], h["mu_u"], h["tau"], prev[g], z, items, r, sd_is_var, np.float64)
        b = restate(V, h["sigma_u"], h["mu_u"], h["tau"], prev[g], z, items, r, sd_is_var, np.longdouble)
        cond = max(cond, float(np.abs(a - b.astype(np.float64)).max()))
        want[g] = a
    umax = float(np.abs(want).max())
    n_max = max(len(it) for it, _ in guests)
    tol = max(64 * cond, K * n_max * EPS * umax) + (2.0 ** -24 * umax if f32 else 0.0)
    err = float(np.abs(G - want).max())
    print("%s sweep %d: max|row err| %.3e (bound %.3e; 64 x conditioning %.3e, floor %.3e)"
          % (what, sweep, err, tol, 64 * cond, K * n_max * EPS * umax))
    assert err <= tol, (what, sweep, err, tol)
    return G


# ---- 1. the draw is the conditional
@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("rng", ["ref", "philox"])
@pytest.mark.parametrize("quirks", ["final", "none"])
def test_draw_is_the_conditional(ml100k, quirks, rng, precision):
    tr, te = ml100k
    guests = make_guests(tr, LENGTHS)
    L = FMLearnSBPMF(num_factor=20, seed=3, rng=rng, quirks=quirks, precision=precision, pipeline=0)
    L.set_data(Data(*tr), Data(*te))
    L.foldin(guests)
    prev = np.zeros((len(guests), 20))
    for s in range(3):
        prev = step_draw(L, guests, prev, s, 3, 20, quirks != "none", precision == "f32",
                         "%s/%s/%s" % (quirks, rng, precision))
        assert np.all(np.abs(prev).max(axis=1) > 0), "every guest, the one without ratings too, has a row"
    L.close()


# ---- 2. every K shape
@pytest.mark.parametrize("K", [100, 250])  # 7 blocks with padding in the last; Kp = 256, the most the kernel holds
def test_every_k_shape(ml100k, K):
    tr, te = ml100k
    guests = make_guests(tr, THIN, repeats=False)
    L = FMLearnSBPMF(num_factor=K, seed=2, rng="philox", pipeline=0)
    L.set_data(Data(*tr), Data(*te))
    L.foldin(guests)
    prev = np.zeros((len(guests), K))
    for s in range(2):
        prev = step_draw(L, guests, prev, s, 2, K, True, False, "K=%d" % K)
    L.close()


# ---- 3. the chain is untouched
@pytest.mark.parametrize("rng", ["ref", "philox"])
def test_chain_is_untouched(ml100k, rng):
    tr, te = ml100k
    watch = np.array([0, 942, 17, 400], np.uint32)
    out = []
    for folded in (False, True):
        L = FMLearnSBPMF(num_factor=20, seed=11, rng=rng)
        L.set_data(Data(*tr), Data(*te))
        L.watch(watch)
        if folded:
            L.foldin(make_guests(tr, LENGTHS))
        L.learn(sweeps=4)
        h = L.hyper()
        rows = [np.stack(L.watch_scores(w)) for w in range(len(watch))]
        out.append([L.rmse_trajectory, *L.factors(), L.predict(), h["sigma_u"], h["mu_u"], h["sigma_v"], h["mu_v"],
                    np.array([h["tau"]])] + rows + list(L.recommend(topn=20)))
        L.close()
    assert len(out[0]) == len(out[1])
    for a, b in zip(*out):
        assert np.array_equal(a, b, equal_nan=True)


# ---- 4. the overlapped schedule (the draw must see this sweep's hyperparameters, not the
# next sweep's, which the host stages into the shared device block while the evaluation runs)
def test_overlapped_schedule(ml100k):
    tr, te = ml100k
    guests = make_guests(tr, LENGTHS)
    kw = dict(num_factor=20, seed=5, rng="philox")
    L = FMLearnSBPMF(pipeline=1, **kw)
    L.set_data(Data(*tr), Data(*te))
    L.foldin(guests)
    L.learn(sweeps=4)
    twin = FMLearnSBPMF(pipeline=0, **kw)
    twin.set_data(Data(*tr), Data(*te))
    twin.foldin(guests)
    for _ in range(4):
        twin.learn(sweeps=1)
    assert np.array_equal(L.factors()[1], twin.factors()[1])
    assert np.array_equal(L.foldin_factors(), twin.foldin_factors())
    for g in range(len(guests)):
        a, b = L.foldin_scores(g), twin.foldin_scores(g)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), g
    L.close()
    twin.close()


# ---- 5. scores and selection
class Moments:
    """numpy running sums of the guests' scores and the tolerance of test_gpu_recommend.py."""

    def __init__(self, K):
        self.K, self.s1, self.s2, self.n, self.tol, self.smax = K, None, None, 0, 0.0, 0.0

    def add(self, G, V):
        s = G @ V.T
        self.tol = max(self.tol, 4 * self.K * EPS * float((np.abs(G) @ np.abs(V).T).max()))
        self.smax = max(self.smax, float(np.abs(s).max()))
        self.s1 = s.copy() if self.s1 is None else self.s1 + s
        self.s2 = s * s if self.s2 is None else self.s2 + s * s
        self.n += 1

    def check(self, L, what):
        e1 = e2 = 0.0
        for g in range(self.s1.shape[0]):
            mean, sd = L.foldin_scores(g)
            e1 = max(e1, float(np.abs(mean - self.s1[g] / self.n).max()))
            e2 = max(e2, float(np.abs(sd * sd + mean * mean - self.s2[g] / self.n).max()))
        b2 = 2 * self.smax * self.tol
        print("%s: n=%d  max|mean err| %.3e (bound %.3e)  max|2nd moment err| %.3e (bound %.3e)"
              % (what, self.n, e1, self.tol, e2, b2))
        assert e1 <= self.tol and e2 <= b2, (what, e1, self.tol, e2, b2)


@pytest.fixture(scope="module")
def scored(ml100k):
    """Four stepped sweeps with the moments checked after each; shared by the selection cases."""
    tr, te = ml100k
    guests = make_guests(tr, LENGTHS)
    L = FMLearnSBPMF(num_factor=20, seed=3, rng="philox")
    L.set_data(Data(*tr), Data(*te))
    L.foldin(guests)
    M = Moments(20)
    for s in range(4):
        L.learn(sweeps=1)
        M.add(L.foldin_factors(), L.factors()[1])
        M.check(L, "sweep %d" % s)
    yield L, guests
    L.close()


@pytest.mark.parametrize("exclude", [True, False])
@pytest.mark.parametrize("risk", [0.0, 1.0])
@pytest.mark.parametrize("topn", [1, 10, 1024])
def test_selection_is_the_lexsort(scored, topn, risk, exclude):
    L, guests = scored
    items, mean, sd = L.foldin_recommend(topn=topn, exclude_rated=exclude, risk=risk)
    assert items.shape == mean.shape == sd.shape == (len(guests), topn) and items.dtype == np.int64
    for g, (rated, _) in enumerate(guests):
        m, s = L.foldin_scores(g)
        want = expected_topn(m, s, rated, topn, risk, exclude)
        assert np.array_equal(items[g], want), (g, topn, risk, exclude)
        real = want >= 0
        assert np.array_equal(mean[g][real], m[want[real]]) and np.array_equal(sd[g][real], s[want[real]])
        assert np.all(np.isnan(mean[g][~real])) and np.all(np.isnan(sd[g][~real]))
        if exclude:
            assert not np.intersect1d(items[g][real], rated).size
            assert real.sum() == min(topn, J - len(np.unique(rated)))  # no ratings: nothing left out; all: nothing left
        else:
            assert real.all()


def test_clamped_scores(ml100k):
    tr, te = ml100k
    guests = make_guests(tr, (0, 65), repeats=False)
    L = FMLearnSBPMF(num_factor=20, seed=3, rng="philox")
    L.set_data(Data(*tr), Data(*te))
    L.foldin(guests, clamp=True)
    L.learn(sweeps=1)
    G, V = L.foldin_factors(), L.factors()[1]
    tol = 4 * 20 * EPS * float((np.abs(G) @ np.abs(V).T).max())
    for g in range(2):
        mean, sd = L.foldin_scores(g)
        assert np.abs(mean - np.clip(G[g] @ V.T, 1.0, 5.0)).max() <= tol and np.all(sd == 0.0)
    L.close()


def test_only_collected_sweeps_are_accumulated(ml100k):
    tr, te = ml100k
    guests = make_guests(tr, THIN, repeats=False)
    L = FMLearnSBPMF(num_factor=20, seed=4, rng="philox", burnin=2)
    L.set_data(Data(*tr), Data(*te))
    L.foldin(guests)
    rows = []
    for _ in range(2):
        L.learn(sweeps=1)
        rows.append(L.foldin_factors())
        with pytest.raises(SBMFError) as ei:
            L.foldin_scores(0)
        assert ei.value.code == SBMF_E_STATE and "accumulated" in str(ei.value)
    assert np.all(np.abs(rows[0]).max(axis=1) > 0) and not np.array_equal(rows[0], rows[1])  # the rows move in burn-in
    M = Moments(20)
    for s in range(2):
        L.learn(sweeps=1)
        M.add(L.foldin_factors(), L.factors()[1])
        M.check(L, "burnin=2, collected sweep %d" % s)
    L.close()


# ---- 6. rerun and lifecycle
def test_rerun_is_bit_identical(ml100k):
    tr, te = ml100k
    guests = make_guests(tr, LENGTHS)
    out = []
    for _ in range(2):
        L = FMLearnSBPMF(num_factor=20, seed=9, rng="philox")
        L.set_data(Data(*tr), Data(*te))
        L.foldin(guests)
        L.learn(sweeps=3)
        rows = [np.stack(L.foldin_scores(g)) for g in range(len(guests))]
        out.append([L.foldin_factors()] + rows + list(L.foldin_recommend(topn=50, risk=0.5)))
        L.close()
    for a, b in zip(*out):
        assert np.array_equal(a, b, equal_nan=True)


def _code(fn, *a, **k):
    with pytest.raises(SBMFError) as ei:
        fn(*a, **k)
    return ei.value.code, str(ei.value)


def test_lifecycle_errors_and_resources(ml100k):
    tr, te = ml100k
    base = {k: device_usage()[k] for k in COUNTS}
    guests = make_guests(tr, THIN, repeats=False)
    L = FMLearnSBPMF(num_factor=20, seed=1, rng="philox")
    L.set_data(Data(*tr), Data(*te))
    held = {k: device_usage()[k] for k in COUNTS}
    assert _code(L.foldin_recommend, topn=5)[0] == SBMF_E_STATE  # no list
    assert _code(L.foldin, [([J], [3.0])])[0] == SBMF_E_ARG  # a bad item id
    ptr, items, ratings = np.array([0, 2, 1], np.uint32), np.array([1, 2], np.uint32), np.array([3.0, 4.0])
    code, msg = _code(L.foldin, (ptr, items, ratings))
    assert code == SBMF_E_ARG and "decreases" in msg
    pu, pi, pr = (ptr.ctypes.data_as(C.POINTER(C.c_uint32)), items.ctypes.data_as(C.POINTER(C.c_uint32)),
                  ratings.ctypes.data_as(C.POINTER(C.c_double)))
    assert lib.sbmf_foldin_users(L.ctx, 1, pu, pi, pr, 2) == SBMF_E_ARG  # unknown flags
    assert {k: device_usage()[k] for k in COUNTS} == held  # a refused registration holds nothing
    L.foldin(guests)
    assert device_usage()["dev_allocs"] > held["dev_allocs"]
    for fn, a in ((L.foldin_factors, ()), (L.foldin_scores, (0,)), (L.foldin_recommend, ())):
        code, msg = _code(fn, *a)
        assert code == SBMF_E_STATE and "no sweep" in msg  # results before any sweep
    assert L.foldin_timing() == {"ms_draw": 0.0, "ms_score": 0.0, "ms_select": 0.0}
    L.learn(sweeps=2)
    assert _code(L.foldin_recommend, topn=0)[0] == SBMF_E_ARG
    assert _code(L.foldin_recommend, topn=1025)[0] == SBMF_E_ARG
    assert _code(L.foldin_scores, len(guests))[0] == SBMF_E_ARG
    t = L.foldin_timing()
    assert t["ms_draw"] > 0 and t["ms_score"] > 0 and t["ms_select"] == 0
    L.foldin_recommend(topn=5)
    assert L.foldin_timing()["ms_select"] > 0
    assert L.foldin_scores(1)[1].max() > 0
    # registering again (as a CSR) zeroes the rows and the counts
    ptr = np.cumsum([0] + [len(it) for it, _ in guests]).astype(np.uint32)
    L.foldin((ptr, np.concatenate([it for it, _ in guests]), np.concatenate([r for _, r in guests])))
    assert _code(L.foldin_factors)[0] == SBMF_E_STATE
    h0 = len(L.history)
    prev = step_draw(L, guests, np.zeros((len(guests), 20)), h0, 1, 20, True, False, "re-registered")
    mean, sd = L.foldin_scores(1)
    V = L.factors()[1]
    assert np.all(sd == 0.0) and np.abs(mean - prev[1] @ V.T).max() <= 4 * 20 * EPS * (np.abs(prev[1]) @ np.abs(V).T).max()
    L.foldin([])
    assert {k: device_usage()[k] for k in COUNTS} == held  # n = 0: everything the list held is back
    assert _code(L.foldin_recommend, topn=5)[0] == SBMF_E_STATE
    L.close()
    # out of scope: the biased quirk sets, the other learners, a virtual rank
    for kw, word in ((dict(quirks="bias2", num_factor=8), "bias"), (dict(quirks="bias22", num_factor=8), "bias"),
                     (dict(method="vb", num_factor=8), "SBPMF sampler"), (dict(order="libfm", num_factor=8), "SBPMF sampler"),
                     (dict(method="als", num_factor=8), "SBPMF sampler")):
        O = FMLearnSBPMF(seed=1, **kw)
        O.set_data(Data(*tr), Data(*te))
        code, msg = _code(O.foldin, guests)
        assert code == SBMF_E_STATE and word in msg, (kw, msg)
        assert _code(O.foldin_recommend, topn=5)[0] == SBMF_E_STATE
        O.close()
    R = FMLearnSBPMF(num_factor=8, seed=1, rng="philox")
    R.init()
    assert lib.sbmf_test_virtual_rank(R.ctx, 2, 0) == 0
    R.set_data(Data(*tr), Data(*te))
    code, msg = _code(R.foldin, guests)
    assert code == SBMF_E_STATE and "virtual rank" in msg
    R.close()
    W = FMLearnSBPMF(num_factor=20, seed=1, rng="philox")  # closed with a live list
    W.set_data(Data(*tr), Data(*te))
    W.foldin(guests)
    W.learn(sweeps=1)
    W.foldin_recommend(topn=3)
    W.close()
    assert {k: device_usage()[k] for k in COUNTS} == base


# ---- 7. the command line
def test_cli_guests(tmp_path, m1m100k):
    trf, tef = write_m1m100k_libfm(tmp_path)
    (tru, tri, trr), (teu, tei, ter) = m1m100k
    rng = np.random.default_rng(1)
    lists = [(rng.permutation(J)[:n], rng.choice(trr, n)) for n in (4, 0, 70)]  # guest 1 has no line: no ratings
    with open(tmp_path / "guests", "w") as f:
        f.write("# guest item rating\n")
        for g, (it, r) in enumerate(lists):
            for a, b in zip(it, r):
                f.write("%d %d %g\n" % (g, a + 943, b))
    out = tmp_path / "out"
    r = subprocess.run([CLI_PATH, "-task", "r", "-train", trf, "-test", tef, "-method", "mcmc", "-order", "sbpmf",
                        "-dim", "0,0,8", "-iter", "3", "-recommend_guests", str(out), "-rec_guests", str(tmp_path / "guests"),
                        "-rec_topn", "5", "-rec_risk", "0.5"], capture_output=True, text=True, timeout=120, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr
    rows = [l.split("\t") for l in out.read_text().splitlines()]
    assert len(rows) == 5 * 3 and all(len(x) == 4 for x in rows)
    L = FMLearnSBPMF(num_factor=8, seed=1, num_iter=3, eval_train=True, pipeline=1)  # the CLI's settings
    L.set_data(Data(tru, tri - 943, trr), Data(teu, tei - 943, ter))
    assert L.dims()[:2] == (943, J)
    L.foldin(lists)
    L.learn()
    items, mean, sd = L.foldin_recommend(topn=5, risk=0.5)
    L.close()
    for g in range(3):
        mine = rows[5 * g:5 * g + 5]
        assert [int(x[0]) for x in mine] == [g] * 5
        assert [int(x[1]) - 943 for x in mine] == list(items[g])
        assert [float(x[2]) for x in mine] == list(mean[g]) and [float(x[3]) for x in mine] == list(sd[g])
        assert not np.intersect1d(items[g], lists[g][0]).size
