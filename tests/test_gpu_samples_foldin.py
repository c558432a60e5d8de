"""Guests folded into the posterior sample store after the run (sbmf_samples_foldin_recommend /
_rows / _scores, sbmf_get_sample_hyper and the hyperparameters' companion file; the kernel in
csrc/samples_foldin.hip around the scan of csrc/foldin_dev.h, scores and selection by the store's
and the watch list's kernels).

The reference has nothing of the kind.  Two checkers:
  * the in-chain fold-in list (test_gpu_foldin.py): registered together with an every = 1 store
    before the first sweep, it draws the same rows from the same V, hyperparameters and normals,
    so rows, scores and lists must be equal bit for bit (==, never close);
  * the header's coordinate loop restated in numpy (edge_rows.restate_row) on what the library
    returns: V of sample s (sample()), its hyperparameters (sample_hyper()), the device's row of
    the previous sample and the normals philox_normals(seed, sweep_s, 7, g, 256 scans).

Tolerance of the restated draw, per sample (test_gpu_foldin.py's, derived, not fitted):
  tol = max(64 * max|restatement in float64 - the same in np.longdouble|, K * n_max * 2^-52 * max|u|)
        (+ 2^-24 max|u| in an F32 context: one rounding on store)
Each sample restarts from the device's previous row, so nothing compounds across samples.  With
`scans` > 1 the intermediate rows stay in the kernel's LDS; the restatement chains the scans in
both types, its float64 / longdouble difference then measures the conditioning of the whole chain
on those inputs, and each scan may add one step's bound: tol is multiplied by `scans`.

Scores use the tolerance of test_gpu_recommend.py (the same kernel): 4 K eps max sum|u v| per sample.

ML-100k is 943 x 1682; K = 20 gives Kp = 32 (padding inside the second block)."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import sbmf
from edge_rows import restate_row as restate
from sbmf import (SBMF_E_ARG, SBMF_E_STATE, Communicator, Data, FMLearnSBPMF, SBMFError, device_usage, philox_normals)
from sbmf._lib import CLI_PATH, lib
from test_gpu_foldin import LENGTHS, THIN, expected_topn, make_guests

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
J = 1682
TAG_GUEST = 7
COUNTS = ("dev_bytes", "dev_allocs", "pinned_bytes", "pinned_allocs", "streams", "events", "contexts", "comms")


def learner(ml, **kw):
    tr, te = ml
    kw.setdefault("num_factor", 20)
    kw.setdefault("seed", 3)
    L = FMLearnSBPMF(**kw)
    L.set_data(Data(*tr), Data(*te))
    return L


def _code(fn, *a, **k):
    with pytest.raises(SBMFError) as ei:
        fn(*a, **k)
    return ei.value.code, str(ei.value)


def same(a, b):
    return all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b)) and len(a) == len(b)


# ---- 1. agrees with the in-chain list, bit for bit
@pytest.mark.parametrize("pipeline", [0, 1])
@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("rng", ["ref", "philox"])
@pytest.mark.parametrize("quirks", ["final", "none"])
def test_agrees_with_the_in_chain_list(ml100k, quirks, rng, precision, pipeline):
    tr, _ = ml100k
    guests = make_guests(tr, LENGTHS)
    L = learner(ml100k, rng=rng, quirks=quirks, precision=precision, pipeline=pipeline)
    L.foldin(guests)
    L.keep_samples(every=1, cap=4)
    chain = []
    if pipeline:  # one call: the next sweep's hyperparameters are staged while a sweep is evaluated
        L.learn(sweeps=4)
    else:
        for _ in range(4):
            L.learn(sweeps=1)
            chain.append(L.foldin_factors())
    rows = L.samples_foldin_rows(guests)
    assert rows.shape == (4, len(guests), 20)
    for s, want in enumerate(chain):
        assert np.array_equal(rows[s], want), s
    assert np.array_equal(rows[3], L.foldin_factors())
    assert np.all(np.abs(rows).max(axis=2) > 0), "every guest, the one without ratings too, has a row at every sample"
    # a guest's scores are keyed by its number in the list: guest 0's are the one-guest call's
    assert same(L.samples_foldin_scores(*guests[0]), L.foldin_scores(0))
    for kw in (dict(topn=10), dict(topn=1024, exclude_rated=False, risk=1.0)):  # the second: 1024 of every row's scores
        assert same(L.samples_foldin_recommend(guests, **kw), L.foldin_recommend(**kw)), kw
    L.close()


# ---- 2. the draw is the conditional, per sample
def check_samples(L, guests, seed, K, sd_is_var, f32, scans, what):
    """Every sample's rows against the restatement started from the device's previous sample's."""
    rows = L.samples_foldin_rows(guests, scans=scans)
    n_max = max(len(it) for it, _ in guests)
    prev = np.zeros((len(guests), K))
    for s in range(rows.shape[0]):
        smp, h = L.sample(s), L.sample_hyper(s)
        want = np.zeros_like(prev)
        cond = 0.0
        for g, (items, r) in enumerate(guests):
            z = philox_normals(seed, smp["sweep"], TAG_GUEST, g, 256 * scans)
            a, b = prev[g], prev[g].astype(np.longdouble)
            for c in range(scans):
                zc = z[256 * c:256 * c + K]
                a = restate(smp["V"], h["sigma_u"], h["mu_u"], h["tau"], a, zc, items, r, sd_is_var, np.float64)
                b = restate(smp["V"], h["sigma_u"], h["mu_u"], h["tau"], b, zc, items, r, sd_is_var, np.longdouble)
            cond = max(cond, float(np.abs(a - b.astype(np.float64)).max()))
            want[g] = a
        umax = float(np.abs(want).max())
        tol = scans * max(64 * cond, K * n_max * EPS * umax) + (2.0 ** -24 * umax if f32 else 0.0)
        err = float(np.abs(rows[s] - want).max())
        print("%s sample %d (sweep %d): max|row err| %.3e (bound %.3e; 64 x conditioning %.3e, floor %.3e)"
              % (what, s, smp["sweep"], err, tol, 64 * cond, K * n_max * EPS * umax))
        assert err <= tol, (what, s, err, tol)
        prev = rows[s]
    return rows


@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("scans", [1, 3])
def test_draw_is_the_conditional(ml100k, scans, precision):
    tr, _ = ml100k
    guests = make_guests(tr, LENGTHS)
    L = learner(ml100k, rng="philox", quirks="none", precision=precision)
    L.keep_samples(every=1, cap=3)
    L.learn(sweeps=3)
    check_samples(L, guests, 3, 20, False, precision == "f32", scans, "scans=%d/%s" % (scans, precision))
    L.close()


def test_thinned_store_is_keyed_by_the_sweep(ml100k):
    tr, _ = ml100k
    guests = make_guests(tr, THIN)
    L = learner(ml100k, rng="philox")
    L.keep_samples(every=2, cap=4)
    L.learn(sweeps=4)
    assert [L.sample(s)["sweep"] for s in range(2)] == [0, 2]
    check_samples(L, guests, 3, 20, True, False, 1, "every=2")
    L.close()


def test_wrapped_ring(ml100k):
    tr, _ = ml100k
    guests = make_guests(tr, THIN)
    L = learner(ml100k, rng="philox")
    L.keep_samples(every=1, cap=2)
    L.learn(sweeps=3)  # slot 0 holds sweep 2, slot 1 sweep 1: the oldest sample is not in slot 0
    assert [L.sample(s)["sweep"] for s in range(2)] == [1, 2]
    rows = check_samples(L, guests, 3, 20, True, False, 1, "cap=2, 3 sweeps")
    # the scores read the rows and V of the same slot
    mean, sd = L.samples_foldin_scores(*guests[0])
    s = np.stack([rows[k][0] @ L.sample(k)["V"].T for k in range(2)])
    tol = 4 * 20 * EPS * max(float((np.abs(rows[k][0]) @ np.abs(L.sample(k)["V"]).T).max()) for k in range(2))
    assert np.abs(mean - s.mean(axis=0)).max() <= tol
    L.learn(sweeps=1)  # sweeps 2, 3: wrapped twice, the oldest in slot 0 again
    check_samples(L, guests, 3, 20, True, False, 2, "cap=2, 4 sweeps, scans=2")
    L.close()


@pytest.mark.parametrize("K", [100, 250])  # 7 blocks with padding in the last; Kp = 256, the most the kernel holds
def test_every_k_shape(ml100k, K):
    tr, _ = ml100k
    guests = make_guests(tr, THIN, repeats=False)
    L = learner(ml100k, num_factor=K, seed=2, rng="philox")
    L.keep_samples(every=1, cap=2)
    L.learn(sweeps=2)
    check_samples(L, guests, 2, K, True, False, 1, "K=%d" % K)
    L.close()


# ---- 3. sample_hyper is the sweep's
@pytest.mark.parametrize("quirks", ["final", "bias2"])
def test_sample_hyper_is_the_sweeps(ml100k, quirks):
    tr, _ = ml100k
    L = learner(ml100k, rng="philox", quirks=quirks, pipeline=0)
    L.keep_samples(every=1, cap=2)
    seen = []
    for s in range(3):
        L.learn(sweeps=1)
        h, mine = L.hyper(), L.sample_hyper(min(s, 1))  # the newest sample
        assert h["tau"] == mine["tau"]
        for k in ("sigma_u", "mu_u", "sigma_v", "mu_v"):
            assert np.array_equal(h[k], mine[k]), (s, k)
        seen.append(h)
    old = L.sample_hyper(0)  # sweep 1's, kept in its slot while sweep 2 was drawn
    assert old["tau"] == seen[1]["tau"] and np.array_equal(old["sigma_u"], seen[1]["sigma_u"])
    assert _code(L.sample_hyper, 2)[0] == SBMF_E_ARG
    if quirks == "bias2":  # the getter works with biases; the fold-in is what refuses them
        code, msg = _code(L.samples_foldin_rows, make_guests(tr, (5,), repeats=False))
        assert code == SBMF_E_STATE and "guest bias would need a draw of its own" in msg
    L.close()


# ---- 4. fused equals unfused
@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("scans", [1, 3])
def test_fused_equals_unfused(ml100k, scans, precision):
    tr, _ = ml100k
    guests = make_guests(tr, LENGTHS)
    L = learner(ml100k, rng="philox", precision=precision)
    L.keep_samples(every=1, cap=3)
    L.learn(sweeps=4)  # wrapped
    out = []
    for hook in (2, 0):  # bit 1: the one fused launch; 0: the default, one launch per sample and scan
        assert lib.sbmf_test_samples_tune(L.ctx, 0, hook) == 0
        out.append([L.samples_foldin_rows(guests, scans=scans), *L.samples_foldin_scores(*guests[5], scans=scans),
                    *L.samples_foldin_recommend(guests, topn=20, risk=0.5, scans=scans)])
    assert same(*out)
    assert np.abs(out[0][0]).max() > 0
    L.close()


# ---- 5. scores and selection
@pytest.fixture(scope="module")
def stored(ml100k):
    tr, _ = ml100k
    L = learner(ml100k, rng="philox")
    L.keep_samples(every=1, cap=4)
    L.learn(sweeps=4)
    yield L, make_guests(tr, LENGTHS)
    L.close()


@pytest.fixture(scope="module")
def full_rows(stored):
    L, guests = stored
    return [L.samples_foldin_scores(*g) for g in guests]


def test_moments_against_numpy(stored):
    L, guests = stored
    rows = L.samples_foldin_rows(guests)
    V = [L.sample(s)["V"] for s in range(4)]
    sc = np.stack([rows[s] @ V[s].T for s in range(4)])  # [sample][guest][item]
    tol = max(4 * 20 * EPS * float((np.abs(rows[s]) @ np.abs(V[s]).T).max()) for s in range(4))
    smax = float(np.abs(sc).max())
    items, mean, sd = L.samples_foldin_recommend(guests, topn=1024, exclude_rated=False)
    e1 = e2 = 0.0
    for g in range(len(guests)):
        m, d = mean[g], sd[g]
        e1 = max(e1, float(np.abs(m - sc[:, g, items[g]].mean(axis=0)).max()))
        e2 = max(e2, float(np.abs(d * d + m * m - (sc[:, g, items[g]] ** 2).mean(axis=0)).max()))
    print("max|mean err| %.3e (bound %.3e)  max|2nd moment err| %.3e (bound %.3e)" % (e1, tol, e2, 2 * smax * tol))
    assert e1 <= tol and e2 <= 2 * smax * tol
    # the one-guest call is keyed as guest 0 of a list: its full row against numpy on its own rows
    one = [guests[7]]
    r1 = L.samples_foldin_rows(one)
    m, d = L.samples_foldin_scores(*guests[7])
    s1 = np.stack([r1[s][0] @ V[s].T for s in range(4)])
    assert np.abs(m - s1.mean(axis=0)).max() <= tol and np.abs(d * d + m * m - (s1 ** 2).mean(axis=0)).max() <= 2 * smax * tol
    it1, m1, d1 = L.samples_foldin_recommend(one, topn=1024, exclude_rated=False)
    assert np.array_equal(m1[0], m[it1[0]]) and np.array_equal(d1[0], d[it1[0]])  # exactly the values the top-N ranks by


def test_one_sample_has_no_spread(ml100k):
    tr, _ = ml100k
    guests = make_guests(tr, THIN)
    L = learner(ml100k, rng="philox")
    L.keep_samples(every=1, cap=1)
    L.learn(sweeps=2)
    _, mean, sd = L.samples_foldin_recommend(guests, topn=50, exclude_rated=False)
    assert np.all(sd == 0.0) and np.all(np.isfinite(mean))
    assert np.all(L.samples_foldin_scores(*guests[2])[1] == 0.0)
    L.close()


@pytest.mark.parametrize("exclude", [True, False])
@pytest.mark.parametrize("risk", [0.0, 1.0])
@pytest.mark.parametrize("topn", [1, 10, 1024])
def test_selection_is_the_lexsort(stored, full_rows, topn, risk, exclude):
    """A guest's normals are keyed by its number in the list, and the full row is readable for a
    guest on its own (number 0): every guest is ranked as a list of one against its own full row.
    Lists of many guests are held to the in-chain list's (test 1) and to each other (the slices)."""
    L, guests = stored
    for g, (rated, _) in enumerate(guests):
        m, s = full_rows[g]
        items, mean, sd = L.samples_foldin_recommend([guests[g]], topn=topn, exclude_rated=exclude, risk=risk)
        assert items.shape == mean.shape == sd.shape == (1, topn) and items.dtype == np.int64
        want = expected_topn(m, s, rated, topn, risk, exclude)
        assert np.array_equal(items[0], want), (g, topn, risk, exclude)
        real = want >= 0
        assert np.array_equal(mean[0][real], m[want[real]]) and np.array_equal(sd[0][real], s[want[real]])
        assert np.all(np.isnan(mean[0][~real])) and np.all(np.isnan(sd[0][~real]))
        if exclude:
            assert not np.intersect1d(items[0][real], rated).size
            assert real.sum() == min(topn, J - len(np.unique(rated)))  # no ratings: nothing left out; all: nothing left
        else:
            assert real.all()


def test_clamped_scores(stored):
    L, guests = stored
    g = guests[5]
    rows = L.samples_foldin_rows([g])
    V = [L.sample(s)["V"] for s in range(4)]
    sc = np.stack([np.clip(rows[s][0] @ V[s].T, 1.0, 5.0) for s in range(4)])
    tol = max(4 * 20 * EPS * float((np.abs(rows[s][0]) @ np.abs(V[s]).T).max()) for s in range(4))
    mean, sd = L.samples_foldin_scores(*g, clamp=True)
    assert np.abs(mean - sc.mean(axis=0)).max() <= tol and mean.min() >= 1.0 and mean.max() <= 5.0
    assert not np.array_equal(mean, L.samples_foldin_scores(*g)[0])
    a = L.samples_foldin_recommend([g], topn=5, clamp=True)
    assert np.array_equal(a[1][0], mean[a[0][0]])


def test_slices_equal_the_unsliced_call(ml100k):
    tr, _ = ml100k
    rng = np.random.default_rng(11)
    guests = [(rng.permutation(J)[:n].astype(np.uint32), rng.choice(tr[2], n)) for n in rng.integers(0, 40, 150)]
    L = learner(ml100k, rng="philox")
    L.keep_samples(every=1, cap=2)
    L.learn(sweeps=2)
    whole = [L.samples_foldin_rows(guests), *L.samples_foldin_recommend(guests, topn=7, risk=0.5)]
    # 64 guests: two sums of [64][Jp = 1696] doubles and two samples' rows of Kp = 32 doubles
    assert lib.sbmf_test_samples_tune(L.ctx, 64 * (2 * 1696 * 8 + 2 * 32 * 8), 0) == 0
    sliced = [L.samples_foldin_rows(guests), *L.samples_foldin_recommend(guests, topn=7, risk=0.5)]
    assert same(whole, sliced)
    assert lib.sbmf_test_samples_tune(L.ctx, 1, 2) == 0  # a budget below one group: slices of 64 still; the fused launch
    assert same(whole, [L.samples_foldin_rows(guests), *L.samples_foldin_recommend(guests, topn=7, risk=0.5)])
    L.close()


def test_null_stdev_on_a_partial_last_slice(stored, ml100k):
    """Slices of 64, 64 and 22 rows with stdev = NULL: items and mean are those of the call that
    takes a stdev, for users and for guests (the one selection helper's offsets on the last slice)."""
    L, _ = stored
    tr, _ = ml100k
    rng = np.random.default_rng(12)
    users = rng.permutation(943)[:150].astype(np.uint32)
    n, ptr, gi, gr = sbmf._guest_csr([(rng.permutation(J)[:k].astype(np.uint32), rng.choice(tr[2], k))
                                      for k in rng.integers(0, 40, 150)])
    u32, f64 = C.POINTER(C.c_uint32), C.POINTER(C.c_double)
    p = lambda a: a.ctypes.data_as(u32 if a.dtype == np.uint32 else f64)
    # 64 rows: two sums of [64][Jp = 1696] doubles and four samples' rows of Kp = 32 doubles
    assert lib.sbmf_test_samples_tune(L.ctx, 64 * (2 * 1696 * 8 + 4 * 32 * 8), 0) == 0

    def call(who, with_sd):
        items, mean, sd = np.full((150, 3), 0xfffffffe, np.uint32), np.full((150, 3), -7e7), np.full((150, 3), -7e7)
        out = (p(items), p(mean), p(sd) if with_sd else None)
        rc = (lib.sbmf_samples_recommend(L.ctx, 150, p(users), 3, 0, 0.5, *out) if who == "users" else
              lib.sbmf_samples_foldin_recommend(L.ctx, n, p(ptr), p(gi), p(gr), 1, 3, 0, 0.5, *out))
        assert rc == 0, lib.sbmf_last_error(L.ctx)
        return items, mean, sd

    try:
        for who in ("users", "guests"):
            items, mean, sd = call(who, True)
            assert not np.any(items == 0xfffffffe) and not np.any(mean == -7e7) and not np.any(sd == -7e7)  # every slot written
            i0, m0, s0 = call(who, False)
            assert np.array_equal(i0, items) and np.array_equal(m0, mean, equal_nan=True), who
            assert np.all(s0 == -7e7)  # nothing written where no stdev was asked for
    finally:
        assert lib.sbmf_test_samples_tune(L.ctx, 0, 0) == 0


def test_guest_csr_that_does_not_start_at_zero(stored, ml100k):
    """ptr[0] = 5 with five junk entries in front, an empty guest and one that holds all the rest:
    the in-chain list and the stored samples' guests are the rebased CSR's, bit for bit."""
    L, _ = stored
    tr, _ = ml100k
    rng = np.random.default_rng(13)
    items = rng.permutation(J)[:43].astype(np.uint32)
    ratings = rng.choice(tr[2], 43)
    based = (np.array([0, 3, 3, 43], np.uint32), items, ratings)
    offset = (based[0] + 5, np.concatenate([np.full(5, 0xffffffff, np.uint32), items]),
              np.concatenate([np.full(5, np.nan), ratings]))
    assert np.array_equal(L.samples_foldin_rows(offset), L.samples_foldin_rows(based))
    assert same(L.samples_foldin_recommend(offset, topn=5), L.samples_foldin_recommend(based, topn=5))
    out = []
    for csr in (based, offset):
        C2 = learner(ml100k, rng="philox")
        C2.foldin(csr)
        C2.learn(sweeps=2)
        out.append([C2.foldin_factors(), *C2.foldin_recommend(topn=5), *C2.foldin_scores(2)])
        C2.close()
    assert same(*out) and np.all(np.isfinite(out[0][0]))


# ---- 6. nothing else moves
def test_nothing_else_moves(ml100k):
    tr, _ = ml100k
    guests = make_guests(tr, LENGTHS)
    out = []
    for called in (False, True):
        L = learner(ml100k, rng="philox", seed=11)
        L.keep_samples(every=1, cap=3)
        L.learn(sweeps=2)
        if called:
            held = {k: device_usage()[k] for k in COUNTS}
            calls = ((L.samples_foldin_rows, (guests,), {}), (L.samples_foldin_rows, (guests,), dict(scans=2)),
                     (L.samples_foldin_scores, guests[6], {}), (L.samples_foldin_recommend, (guests,), dict(topn=30, risk=0.5)))
            for fn, a, kw in calls:
                first = fn(*a, **kw)
                assert {k: device_usage()[k] for k in COUNTS} == held, fn.__name__  # the temporaries are freed
                again = fn(*a, **kw)  # a rerun is bit-identical
                assert same([first] if isinstance(first, np.ndarray) else first, [again] if isinstance(again, np.ndarray) else again)
            t = L.samples_foldin_timing()
            assert t["ms_draw"] > 0 and t["ms_score"] > 0 and t["ms_select"] > 0
        L.learn(sweeps=2)
        h = L.hyper()
        smp = L.sample(0)
        out.append([L.rmse_trajectory, *L.factors(), L.predict(), h["sigma_u"], h["mu_u"], h["sigma_v"], h["mu_v"],
                    np.array([h["tau"]]), smp["U"], smp["V"], *L.samples_recommend([0, 17, 942], topn=20)])
        L.close()
    assert same(*out)


# ---- 7. files
def test_files(ml100k, tmp_path):
    tr, _ = ml100k
    guests = make_guests(tr, THIN)
    sfile, hfile = tmp_path / "samples.bin", tmp_path / "samples.hyper"
    L = learner(ml100k, rng="philox")
    L.keep_samples(every=1, cap=3)
    L.learn(sweeps=4)  # wrapped: sweeps 1, 2, 3
    L.save_samples(sfile)
    L.save_samples_hyper(hfile)
    want = [L.samples_foldin_rows(guests), *L.samples_foldin_recommend(guests, topn=12, risk=0.5)]
    info = sbmf.samples_file_info(sfile)  # the sample file is the parent's: version 1, the slots' bytes alone
    assert info["version"] == 1 and info["bytes"] == 40 + 3 * 4 + 3 * (943 + 1682) * 20 * 8 == sfile.stat().st_size
    assert sbmf.samples_hyper_file_info(hfile) == {"version": 1, "num_factor": 20, "count": 3,
                                                   "bytes": 24 + 3 * 4 + 3 * 8 * 81}
    assert L.samples_info()["bytes"] == 3 * (943 + 1682) * 32 * 8  # the hyperparameters live on the host
    F = learner(ml100k, rng="philox")  # prepared, never run; the same seed and quirks
    F.load_samples(sfile)
    for fn, a in ((F.samples_foldin_rows, (guests,)), (F.samples_foldin_recommend, (guests,)), (F.samples_foldin_scores, guests[1]),
                  (F.sample_hyper, (0,))):
        code, msg = _code(fn, *a)
        assert code == SBMF_E_STATE and "sbmf_load_samples_hyper" in msg, msg
    F.load_samples_hyper(hfile)
    for s in range(3):
        a, b = L.sample_hyper(s), F.sample_hyper(s)
        assert a["tau"] == b["tau"] and all(np.array_equal(a[k], b[k]) for k in ("sigma_u", "mu_u", "sigma_v", "mu_v"))
    assert same(want, [F.samples_foldin_rows(guests), *F.samples_foldin_recommend(guests, topn=12, risk=0.5)])
    F.load_samples(sfile)  # replaces the samples: the mark is cleared again
    assert _code(F.samples_foldin_rows, guests)[0] == SBMF_E_STATE
    F.close()
    # a companion file of another count, K or sweep index
    L.keep_samples(every=1, cap=2)
    L.learn(sweeps=2)
    L.save_samples_hyper(tmp_path / "two.hyper")
    L.keep_samples(every=1, cap=3)
    L.learn(sweeps=3)  # sweeps 6, 7, 8
    L.save_samples_hyper(tmp_path / "later.hyper")
    L.close()
    O = learner(ml100k, rng="philox", num_factor=8)
    O.keep_samples(every=1, cap=3)
    O.learn(sweeps=4)
    O.save_samples_hyper(tmp_path / "k8.hyper")
    O.close()
    F = learner(ml100k, rng="philox")
    F.load_samples(sfile)
    for name, words in (("two.hyper", ("count = 2", "holds 3")), ("k8.hyper", ("K = 8", "K = 20")),
                        ("later.hyper", ("sweep index 6", "sample 0", "sweep 1"))):
        code, msg = _code(F.load_samples_hyper, tmp_path / name)
        assert code == SBMF_E_ARG and all(w in msg for w in words), (name, msg)
    assert _code(F.samples_foldin_rows, guests)[0] == SBMF_E_STATE  # a refused file sets nothing
    F.close()


# ---- 8. refusals
def test_refusals(ml100k):
    tr, te = ml100k
    guests = make_guests(tr, THIN, repeats=False)
    base = {k: device_usage()[k] for k in COUNTS}
    L = learner(ml100k, rng="philox")
    for fn, a in ((L.samples_foldin_rows, (guests,)), (L.samples_foldin_recommend, (guests,)), (L.samples_foldin_scores, guests[1]),
                  (L.sample_hyper, (0,)), (L.save_samples_hyper, ("/nonexistent/x",))):
        code, msg = _code(fn, *a)
        assert code == SBMF_E_STATE and "no sample kept yet" in msg, msg
    L.keep_samples(every=1, cap=2)
    L.learn(sweeps=1)
    held = {k: device_usage()[k] for k in COUNTS}
    for kw, word in ((dict(scans=0), "scans 0"), (dict(scans=65), "scans 65"), (dict(topn=0), "topn 0"), (dict(topn=1025), "topn 1025")):
        code, msg = _code(L.samples_foldin_recommend, guests, **kw)
        assert code == SBMF_E_ARG and word in msg, msg
    assert _code(L.samples_foldin_rows, guests, scans=0)[0] == SBMF_E_ARG
    assert _code(L.samples_foldin_scores, [1], [3.0], scans=65)[0] == SBMF_E_ARG
    code, msg = _code(L.samples_foldin_rows, [([J], [3.0])])
    assert code == SBMF_E_ARG and "is not below the 1682 items" in msg
    assert _code(L.samples_foldin_scores, [J], [3.0])[0] == SBMF_E_ARG
    ptr, items, ratings = np.array([0, 2, 1], np.uint32), np.array([1, 2], np.uint32), np.array([3.0, 4.0])
    code, msg = _code(L.samples_foldin_recommend, (ptr, items, ratings))
    assert code == SBMF_E_ARG and "decreases" in msg
    P = lambda a, t: a.ctypes.data_as(C.POINTER(t))
    one = np.array([0, 2], np.uint32)
    out_i, out_m = np.zeros(1, np.uint32), np.zeros(1)
    rc = lib.sbmf_samples_foldin_recommend(L.ctx, 1, P(one, C.c_uint32), P(items, C.c_uint32), P(ratings, C.c_double),
                                           1, 1, 4, 0.0, P(out_i, C.c_uint32), P(out_m, C.c_double), None)
    assert rc == SBMF_E_ARG and b"unknown flags" in lib.sbmf_last_error(L.ctx)
    mean = np.zeros(J)
    rc = lib.sbmf_samples_foldin_scores(L.ctx, 2, P(items, C.c_uint32), P(ratings, C.c_double), 1, 1,
                                        P(mean, C.c_double), None)
    assert rc == SBMF_E_ARG and b"unknown flags" in lib.sbmf_last_error(L.ctx)
    assert {k: device_usage()[k] for k in COUNTS} == held  # a refused call holds nothing
    assert L.samples_foldin_rows([]).shape == (1, 0, 20)  # no guest: nothing to do
    L.close()
    for kw, word in ((dict(method="vb", num_factor=8), "online VB"), (dict(order="libfm", num_factor=8), "libFM MCMC"),
                     (dict(method="als", num_factor=8), "ALS")):
        O = FMLearnSBPMF(seed=1, **kw)
        O.set_data(Data(*tr), Data(*te))
        for fn, a in ((O.samples_foldin_rows, (guests,)), (O.samples_foldin_recommend, (guests,)), (O.sample_hyper, (0,)),
                      (O.load_samples_hyper, ("/nonexistent",))):
            code, msg = _code(fn, *a)
            assert code == SBMF_E_STATE and "SBPMF sampler" in msg and word in msg, (kw, msg)
        O.close()
    B = learner(ml100k, rng="philox", quirks="bias2", num_factor=8)
    code, msg = _code(B.samples_foldin_recommend, guests)
    assert code == SBMF_E_STATE and "guest bias would need a draw of its own" in msg
    B.close()
    comm = Communicator(1, 0, bytes(128))
    N = FMLearnSBPMF(num_factor=8, seed=1, rng="philox")
    N.init(comm=comm)
    for fn, a in ((N.samples_foldin_rows, (guests,)), (N.samples_foldin_recommend, (guests,)), (N.samples_foldin_scores, guests[1]),
                  (N.samples_foldin_timing, ()), (N.sample_hyper, (0,))):
        code, msg = _code(fn, *a)
        assert code == SBMF_E_STATE and "joined a communicator" in msg, msg
    N.close()
    comm.close()
    R = FMLearnSBPMF(num_factor=8, seed=1, rng="philox")
    R.init()
    assert lib.sbmf_test_virtual_rank(R.ctx, 2, 0) == 0
    R.set_data(Data(*tr), Data(*te))
    code, msg = _code(R.samples_foldin_rows, guests)
    assert code == SBMF_E_STATE and "virtual rank" in msg
    R.close()
    assert {k: device_usage()[k] for k in COUNTS} == base


# ---- 9. the command line
def test_cli_serves_guests_from_the_files(ml100k, tmp_path):
    tr, te = ml100k
    for name, d in (("train", tr), ("test", te)):
        with open(tmp_path / name, "w") as f:
            for u, i, r in zip(*d):
                f.write("%d %d %g\n" % (u, i, r))
    rng = np.random.default_rng(1)
    lists = [(rng.permutation(J)[:n], rng.choice(tr[2], n)) for n in (4, 0, 70)]  # guest 1 has no line: no ratings
    with open(tmp_path / "guests", "w") as f:
        f.write("# guest item rating\n")
        for g, (it, r) in enumerate(lists):
            for a, b in zip(it, r):
                f.write("%d %d %g\n" % (g, a, b))
    common = [CLI_PATH, "-task", "r", "-train", str(tmp_path / "train"), "-test", str(tmp_path / "test"), "-dim", "0,0,8",
              "-rng", "philox", "-seed", "4"]
    sfile, hfile, out = tmp_path / "samples.bin", tmp_path / "samples.hyper", tmp_path / "out"
    r = subprocess.run(common + ["-iter", "5", "-samples_out", str(sfile), "-samples_every", "2", "-samples_hyper_out", str(hfile)],
                       capture_output=True, text=True, timeout=120, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr
    assert sbmf.samples_hyper_file_info(hfile)["count"] == sbmf.samples_file_info(sfile)["count"] == 3
    r = subprocess.run(common + ["-samples_in", str(sfile), "-samples_hyper_in", str(hfile), "-samples_guests", str(tmp_path / "guests"),
                                 "-samples_recommend_guests", str(out), "-samples_scans", "2", "-rec_topn", "5", "-rec_risk", "0.5"],
                       capture_output=True, text=True, timeout=120, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr
    assert "#Iter=" not in r.stdout  # no sweep
    L = learner(ml100k, num_factor=8, seed=4, rng="philox")
    L.load_samples(sfile)
    L.load_samples_hyper(hfile)
    assert [L.sample(s)["sweep"] for s in range(3)] == [0, 2, 4]
    items, mean, sd = L.samples_foldin_recommend(lists, topn=5, risk=0.5, scans=2)
    L.close()
    want = ["%d\t%d\t%.17g\t%.17g" % (g, items[g][j], mean[g][j], sd[g][j]) for g in range(3) for j in range(5)]
    assert out.read_text().splitlines() == want
