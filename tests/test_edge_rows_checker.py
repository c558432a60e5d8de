"""The checker of tests/test_gpu_edge_rows.py, validated on the CPU before anything trusts it.

1. The set is what tests/edge_rows.py says: exact row lengths on both sides, every length the
   table names as the last of a kind, set or task with its successor.
2. The restatement is the sampler: sweep 0 of the whole set restated in float64 from the Philox
   init, with the oracle's hyperparameters and tau, is the oracle's U and V under the f64 bound.
3. The f32 bound can see a small error: at M = 64, the most the GPU test may allow, a row
   restated without its last rating, its last 4-vector or its last chunk is at least 8 bounds
   from the true one, for every edge row of 2 ratings or more, on the state sweep 0 starts
   from; what is left of that on the state the third sweep starts from is in the test's text."""
import numpy as np
import pytest

import oracle
from edge_rows import (F32_M, F32_M_MAX, LENGTHS, ROWS_PER_LENGTH, SIDES, TAG_INIT_U, TAG_INIT_V, TAG_ITEMS, TAG_USERS,
                       checked_rows, degrees, edge_set, f32_bound, f64_bound, restate_gathered, restate_row, row_lists,
                       table_edges, to_f32)
from sbmf import philox_normals

SET_SEED = 17
K = 20


def test_the_set_is_what_the_table_needs():
    train, test, dims, edge_rows = edge_set(SET_SEED)
    again = edge_set.__wrapped__(SET_SEED)
    for a, b in zip(train + test, again[0] + again[1]):
        assert np.array_equal(a, b)
    assert again[2] == dims and again[3] == edge_rows
    assert 95000 <= len(train[2]) <= 105000
    assert np.array_equal(np.round(2 * train[2]), 2 * train[2]) and train[2].min() >= 0.5 and train[2].max() <= 5.0
    assert len(np.unique(train[2])) >= 8  # not a constant
    assert len({(int(u), int(i)) for u, i in zip(train[0], train[1])}) == len(train[0])  # no pair twice
    for s, side in enumerate(SIDES):
        deg = degrees(SET_SEED, side)
        assert len(deg) == dims[s]
        assert sorted(edge_rows[side]) == sorted(LENGTHS)
        for n in LENGTHS:
            assert len(edge_rows[side][n]) == ROWS_PER_LENGTH
            assert [int(deg[r]) for r in edge_rows[side][n]] == [n, n], (side, n)
        assert min(edge_rows[side][0]) > int(train[s].max())  # the empty rows exist through dims alone
        only = np.setdiff1d(test[s], train[s])  # ids of the test set without a training rating
        assert any(int(x) not in [r for rows in edge_rows[side].values() for r in rows] for x in only)
        assert 4300 <= dims[s] - len(LENGTHS) * ROWS_PER_LENGTH - 1 <= 4500  # the filler pool
        assert len(checked_rows(SET_SEED, side)) == len(LENGTHS) * ROWS_PER_LENGTH + 200
    missing = [e for e in table_edges() if e not in LENGTHS or e + 1 not in LENGTHS]
    assert not missing, "edge list stale: the table's edges %s (or their successors) are not in LENGTHS" % missing
    assert F32_M <= F32_M_MAX == 64 and F32_M & (F32_M - 1) == 0


def _normals(seed, sweep, tag, rows, k):
    return np.stack([philox_normals(seed, sweep, tag, int(r), k) for r in rows])


def _restate_side(side, partner, own, sig, mu, tau, z, sd_is_var, dt):
    """Every row of the side, the rows of one length in one stack."""
    ptr, oth, rat = row_lists(SET_SEED)[side]
    n = np.diff(ptr)
    out = np.zeros(own.shape, dtype=dt)
    for length in np.unique(n):
        g = np.flatnonzero(n == length)
        idx = np.stack([oth[ptr[r]:ptr[r] + length] for r in g])
        r = np.stack([rat[ptr[q]:ptr[q] + length] for q in g])
        out[g] = restate_gathered(partner[idx], sig, mu, tau, own[g], z[g], r, sd_is_var, dt)
    return out, n


@pytest.mark.parametrize("quirks", ["final", "none"])
def test_the_restatement_is_the_sampler(quirks):
    train, test, dims, _ = edge_set(SET_SEED)
    seed = 5
    o = oracle.run(train, test, K=K, iters=1, seed=seed, quirks=quirks, rng="philox", num_users=dims[0], num_items=dims[1])
    h, tau = o["hyper"], o["tau"][0]
    U0 = 1.0 * _normals(seed, 0xffffffff, TAG_INIT_U, range(dims[0]), K)  # init_stdev 1 in both quirk sets
    V0 = 1.0 * _normals(seed, 0xffffffff, TAG_INIT_V, range(dims[1]), K)
    zu, zv = _normals(seed, 0, TAG_USERS, range(dims[0]), K), _normals(seed, 0, TAG_ITEMS, range(dims[1]), K)
    sd_is_var = quirks != "none"
    worst = 0.0
    for dt in (np.float64, np.longdouble):
        U1, nu = _restate_side("users", V0, U0, h[:K], h[K:2 * K], tau, zu, sd_is_var, dt)
        V1, nv = _restate_side("items", U1.astype(np.float64), V0, h[2 * K:3 * K], h[3 * K:], tau, zv, sd_is_var, dt)
        if dt is np.float64:
            U64, V64 = U1, V1
    for name, got, a64, ald, n in (("U", o["U"], U64, U1, nu), ("V", o["V"], V64, V1, nv)):
        err, bound = np.abs(got - a64).max(axis=1), f64_bound(a64, ald, n, K)
        w = np.argmax(err / bound)
        worst = max(worst, float(err[w] / bound[w]))
        print("%s/%s: restatement against the oracle, max|err| %.3e; worst row %d (n=%d): err %.3e, bound %.3e"
              % (quirks, name, err.max(), w, n[w], err[w], bound[w]))
        assert np.all(err <= bound), (name, int(w), float(err[w]), float(bound[w]))
    assert worst > 0  # the oracle's own sums run in another order: a zero would mean nothing was compared


def _left_out(n):
    """(what, ratings kept): the last rating, the last 4-vector, the last chunk of the host's
    split (build_stream_tasks: nch = ceil(n / task), chunks of ceil(n / nch)) at the f32 task of
    2048 ratings and at split_chunk = 64."""
    out = [("last rating", n - 1), ("last 4-vector", 4 * ((n - 1) // 4))]
    for task in (2048, 64):
        if n > task:
            nch = -(-n // task)
            out.append(("last chunk of %d" % task, (nch - 1) * -(-n // nch)))
    return out


@pytest.mark.parametrize("state", ["init", "after 2 sweeps"])
def test_the_f32_bound_sees_a_left_out_rating(state):
    """init: the state sweep 0 of the GPU test starts from; the condition holds for every edge row
    and every omission (measured: at least 57 bounds).  after 2 sweeps: the state its last sweep
    starts from, where the residuals are several times smaller while the sequential float32
    restatement's error, and with it the bound, has grown like sqrt(n).  There the condition
    still holds for every omission on the rows below 1023 ratings (at least 38 bounds) and for
    a left-out task of 2048 on the longer ones (at least 216 bounds); both are asserted.  One
    left-out rating, 4-vector or 64-rating chunk moves the rows of 1023 ratings and more by
    only 2.5 .. 8.4 bounds at M = 64: the reference does not have the margin of 8 there, so
    those are held to 2 bounds.  On the long rows it is sweep 0 that sees a single rating with
    room to spare."""
    train, test, dims, edge_rows = edge_set(SET_SEED)
    seed = 5
    if state == "init":
        o = oracle.run(train, test, K=K, iters=1, seed=seed, rng="philox", num_users=dims[0], num_items=dims[1])
        U = _normals(seed, 0xffffffff, TAG_INIT_U, range(dims[0]), K)
        V = _normals(seed, 0xffffffff, TAG_INIT_V, range(dims[1]), K)
        sweep = 0
    else:
        o = oracle.run(train, test, K=K, iters=2, seed=seed, rng="philox", num_users=dims[0], num_items=dims[1])
        U, V, sweep = o["U"], o["V"], 2
    U, V, h, tau = to_f32(U), to_f32(V), to_f32(o["hyper"]), float(to_f32(o["tau"][-1]))
    worst = {}
    fails = []
    for side, own, partner, sig, mu, tag in (("users", U, V, h[:K], h[K:2 * K], TAG_USERS),
                                             ("items", V, U, h[2 * K:3 * K], h[3 * K:], TAG_ITEMS)):
        ptr, oth, rat = row_lists(SET_SEED)[side]
        for n in LENGTHS:
            if n < 2:
                continue
            for row in edge_rows[side][n]:
                ids, r = oth[ptr[row]:ptr[row + 1]], rat[ptr[row]:ptr[row + 1]]
                z = to_f32(philox_normals(seed, sweep, tag, row, K))
                a = lambda m, dt, seq=False: restate_row(partner, sig, mu, tau, own[row], z, ids[:m], r[:m], True, dt, seq)
                a64 = a(n, np.float64)
                bound = float(f32_bound(a64, a(n, np.float32, True), F32_M_MAX))
                for what, keep in _left_out(n):
                    moved = float(np.abs(a(keep, np.float64) - a64).max())
                    key = (side, what, "n < 1023" if n < 1023 else "n >= 1023")
                    if key not in worst or moved / bound < worst[key][0]:
                        worst[key] = (moved / bound, n, moved, bound)
                    # the reference has no 8 bounds on the long rows of the later state: a shorter margin
                    margin = 8 if state == "init" or n < 1023 or "chunk of 2048" in what else 2
                    if not moved >= margin * bound:
                        fails.append((side, n, row, what, moved, bound))
    for (side, what, cls), (ratio, n, moved, bound) in sorted(worst.items()):
        print("%s, %s, %s, %s left out: least sensitivity %.1f bounds (n=%d: moved %.3e, bound at M=64 %.3e)"
              % (state, side, cls, what, ratio, n, moved, bound))
    assert not fails, fails
