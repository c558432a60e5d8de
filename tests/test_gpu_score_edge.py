"""Scoring edge set: k_samples_score, k_watch_accum (both through
watch_tile_products, csrc/recommend_dev.h) and k_samples_pairs on samples whose sums are exact.

Factors and biases are multiples of 1/4 in [-2, 2] (exact in float32 too): every product is a
multiple of 1/16, every dot product, S1 and S2 is far below 2^53 in units of 1/256 -- exact in any
summation order.  The MFMA's k permutation, the 16-lane butterfly of k_samples_pairs and numpy have
to agree bit for bit; a lost or mispaired product is a mismatch, not a rounding question.

131 users x 261 items x 3 samples: 261 crosses the 128 items of a k_samples_score workgroup and the
256 of a k_watch_accum workgroup and ends in a ragged tile of 5; the list lengths sit at the
workgroups' 16 / 32 / 64 users.  K sits at the bounds of watch_mu (Kp 112 | 128: 64 -> 32 users
per workgroup; 240 | 256: 32 -> 16) and at one block of 16."""
import numpy as np
import pytest

from conftest import gpu_available
from sample_files import check_row, expected_topn, moments, open_with, same_bits, write_samples
from sbmf import device_usage
from sbmf._lib import lib

pytestmark = pytest.mark.gpu

SEED = 31
S = 3
KS = (1, 15, 16, 17, 112, 113, 128, 240, 241, 256)
LENGTHS = (1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 131)
COUNTS = ("dev_bytes", "dev_allocs", "pinned_bytes", "pinned_allocs", "streams", "events", "contexts", "comms")


def quarters(rng, *shape):
    return rng.integers(-8, 9, shape) / 4.0


def make(I, J, K, bias):
    """seeded by the shape alone: f64 and f32, and both quirk sets, see the same factors"""
    rng = np.random.default_rng([SEED, I, J, K])
    a = dict(U=quarters(rng, S, I, K), V=quarters(rng, S, J, K))
    b = dict(b0=quarters(rng, S), bu=quarters(rng, S, I), bv=quarters(rng, S, J))
    if bias:
        a.update(b)
    # the training set: user 0 rated nothing, the last user everything, the others a seeded part
    u, i = [], []
    for user in range(1, I):
        r = np.arange(J) if user == I - 1 else np.flatnonzero(rng.random(J) < rng.random())
        u.append(np.full(len(r), user, np.uint32))
        i.append(r.astype(np.uint32))
    u, i = np.concatenate(u), np.concatenate(i)
    return a, (u, i, np.full(len(u), 3.0))


def reference(a, clamp, lo, hi):
    """(mean, variance, sd) [I][J]: per sample ((b0 + b_u) + b_j) + dot, the clamp, then the moments"""
    sc = []
    for s in range(S):
        x = a["U"][s] @ a["V"][s].T
        if "b0" in a:
            x = ((a["b0"][s] + a["bu"][s])[:, None] + a["bv"][s][None, :]) + x
        if clamp:
            x = np.where(x < hi, x, hi)
            x = np.where(lo < x, x, lo)
        sc.append(x)
    return moments(np.stack(sc)), np.stack(sc)


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


def run(tmp_path, I, J, K, precision, quirks):
    assert gpu_available(), "these tests need a gfx950 device"
    base = {k: device_usage()[k] for k in COUNTS}
    bias = quirks == "bias2"
    a, train = make(I, J, K, bias)
    rated = [train[1][train[0] == u] for u in range(I)]
    write_samples(tmp_path / "exact.samples", precision=precision, **a)
    L = open_with(tmp_path / "exact.samples", train, I, J, quirks=quirks)
    what0 = "I=%d J=%d K=%d %s %s" % (I, J, K, precision, quirks)
    lo, hi = (0.5 if bias else 1.0), 5.0
    rng = np.random.default_rng(11)
    pu = np.concatenate([rng.integers(0, I, 1000), [0, 0, I - 1, I - 1]]).astype(np.uint32)
    pi = np.concatenate([rng.integers(0, J, 1000), [0, J - 1, 0, J - 1]]).astype(np.uint32)
    sd_same = True
    try:
        for clamp in (False, True):
            (m, v, s), sc = reference(a, clamp, lo, hi)
            if clamp and K >= 15:  # the scores lie on both sides of both bounds
                assert (sc == lo).any() and (sc == hi).any() and ((sc > lo) & (sc < hi)).any()
            got = {}
            for unfused in (0, 1):
                what = "%s clamp=%s %s" % (what0, clamp, "per-sample" if unfused else "fused")
                assert lib.sbmf_test_samples_tune(L.ctx, 0, unfused) == 0
                rows = [L.samples_scores(u, clamp=clamp) for u in range(I)]
                for u in range(I):
                    sd_same = check_row(rows[u][0], rows[u][1], (m[u], v[u], s[u]), "%s user %d" % (what, u)) and sd_same
                out = [np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows])]
                want = {}
                for users in user_lists(I):
                    for topn, exclude, risk in ((10, True, 0.5), (1024, False, 0.0)) + (((10, False, 1.0), (1024, True, 0.0)) if len(users) in (17, I) else ()):
                        items, mean, sd = L.samples_recommend(users, topn=topn, exclude_rated=exclude, risk=risk, clamp=clamp)
                        out += [items, mean, sd]
                        assert items.shape == (len(users), topn)
                        for w, u in enumerate(users):
                            k = (int(u), exclude, risk)
                            if k not in want:
                                want[k] = expected_topn(rows[u][0], rows[u][1], rated[u], 1024, risk, exclude)
                            e = want[k][:topn]
                            assert np.array_equal(items[w], e), (what, len(users), w, int(u), topn, exclude, risk)
                            real = e >= 0
                            same_bits(mean[w][real], rows[u][0][e[real]], "%s list of %d, user %d mean" % (what, len(users), u))
                            same_bits(sd[w][real], rows[u][1][e[real]], "%s list of %d, user %d stdev" % (what, len(users), u))
                            assert np.all(np.isnan(mean[w][~real])) and np.all(np.isnan(sd[w][~real]))
                            assert int(real.sum()) == min(topn, J - len(rated[u]) if exclude else J)
                got[unfused] = out
            assert lib.sbmf_test_samples_tune(L.ctx, 0, 0) == 0
            for x, y in zip(got[0], got[1]):  # the two routes: identical bits
                assert x.dtype == y.dtype
                if x.dtype == np.float64:
                    same_bits(y, x, "%s clamp=%s, the two routes" % (what0, clamp))
                else:
                    assert np.array_equal(x, y)
            pm, ps = L.samples_predict(pu, pi, clamp=clamp)
            sd_same = check_row(pm, ps, (m[pu, pi], v[pu, pi], s[pu, pi]), "%s clamp=%s pairs" % (what0, clamp)) and sd_same
    finally:
        L.close()
    print("%s: stdev bit-equal to numpy's sqrt on every slot: %s" % (what0, sd_same))
    assert {k: device_usage()[k] for k in COUNTS} == base


@pytest.mark.parametrize("quirks", ["final", "bias2"])
@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("K", KS)
def test_exact_sums(tmp_path, K, precision, quirks):
    run(tmp_path, 131, 261, K, precision, quirks)


# J = 129: the k_samples_score workgroup's 128 items with a single ragged tile behind them
@pytest.mark.parametrize("quirks", ["final", "bias2"])
@pytest.mark.parametrize("K", [16, 113])
def test_exact_sums_one_item_past_a_workgroup(tmp_path, K, quirks):
    run(tmp_path, 17, 129, K, "f64", quirks)


@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_bias_order_on_inexact_values(tmp_path, precision):
    """The exact sums cannot see the order in which a score's four terms are added -- every order
    gives the same bits.  K = 1 with continuous values can: the dot product is one correctly
    rounded product (plus zero padding), and ((b0 + b_u) + b_j) + dot rounds once per addition,
    which numpy restates exactly; any other association differs in the last bit on many slots.
    Only the mean is compared: S2 adds s * s to a sum, which the compiler may contract into one
    fused operation -- the same bits as two on the exact sets, not on these values."""
    assert gpu_available(), "these tests need a gfx950 device"
    I, J, n = 40, 300, 2
    rng = np.random.default_rng([SEED, 7])
    f = np.float32 if precision == "f32" else np.float64
    a = dict(U=rng.normal(size=(n, I, 1)).astype(f).astype(np.float64), V=rng.normal(size=(n, J, 1)).astype(f).astype(np.float64),
             b0=rng.normal(3.0, 1.0, n), bu=rng.normal(size=(n, I)), bv=rng.normal(size=(n, J)))
    write_samples(tmp_path / "inexact.samples", precision=precision, **a)
    L = open_with(tmp_path / "inexact.samples", (np.zeros(1, np.uint32), np.zeros(1, np.uint32), np.full(1, 3.0)), I, J, quirks="bias2")
    try:
        pu, pi = np.repeat(np.arange(I), 5).astype(np.uint32), rng.integers(0, J, 5 * I).astype(np.uint32)
        for clamp in (False, True):
            sc = np.stack([((a["b0"][s] + a["bu"][s])[:, None] + a["bv"][s][None, :]) + a["U"][s] * a["V"][s].T for s in range(n)])
            other = np.stack([(a["b0"][s] + a["bu"][s])[:, None] + (a["bv"][s][None, :] + a["U"][s] * a["V"][s].T) for s in range(n)])
            assert (sc != other).mean() > 0.1  # the order matters on these values
            want = moments(np.clip(sc, 0.5, 5.0) if clamp else sc)
            for unfused in (0, 1):
                assert lib.sbmf_test_samples_tune(L.ctx, 0, unfused) == 0
                for u in range(I):
                    mean, sd = L.samples_scores(u, clamp=clamp)
                    same_bits(mean, want[0][u], "%s clamp=%s unfused=%d user %d mean" % (precision, clamp, unfused, u))
            assert lib.sbmf_test_samples_tune(L.ctx, 0, 0) == 0
            pm, ps = L.samples_predict(pu, pi, clamp=clamp)
            same_bits(pm, want[0][pu, pi], "%s clamp=%s pairs mean" % (precision, clamp))
    finally:
        L.close()


def test_slices_give_the_unsliced_lists(tmp_path):
    """a budget of 64 rows (64 * 2 * Jp * 8 bytes) slices 131 users as 64 / 64 / 3"""
    assert gpu_available(), "these tests need a gfx950 device"
    I, J, K = 131, 261, 113
    a, train = make(I, J, K, True)
    write_samples(tmp_path / "exact.samples", precision="f64", **a)
    L = open_with(tmp_path / "exact.samples", train, I, J, quirks="bias2")
    try:
        users = user_lists(I)[-1]
        assert len(users) == 131
        Jp = (J + 15) // 16 * 16
        for topn, exclude, clamp in ((10, True, False), (1024, False, True), (1024, True, False)):
            whole = L.samples_recommend(users, topn=topn, exclude_rated=exclude, risk=0.5, clamp=clamp)
            assert lib.sbmf_test_samples_tune(L.ctx, 64 * 2 * Jp * 8, 0) == 0
            sliced = L.samples_recommend(users, topn=topn, exclude_rated=exclude, risk=0.5, clamp=clamp)
            assert lib.sbmf_test_samples_tune(L.ctx, 0, 0) == 0
            for x, y in zip(whole, sliced):
                assert np.array_equal(x, y, equal_nan=True)
            assert (whole[0][:, 0] >= 0).sum() >= 129  # real lists: every user but those who rated everything
    finally:
        L.close()
