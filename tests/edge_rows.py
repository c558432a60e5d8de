"""Per-row check of the sampler's row kernels (k_gblock, k_grow, k_gres, k_split_finish) on a
rating set whose rows sit on every length the host code dispatches on.

The set (edge_set): two user rows and two item rows of every length in LENGTHS, exact
because edge users rate only filler items and edge items are rated only by filler users.

The checker (check_half): the reference's coordinate loop restated in numpy (restate_row, the
loop test_gpu_foldin.py uses for the guests) on the state the library returns around one sweep:
factors() before, factors() after, that sweep's hyper(), and the row's own normals
philox_normals(seed, sweep, TAG_USERS | TAG_ITEMS, row, K).  The item half is restated from the
library's own new U, so every row is an independent check of one kernel invocation.

Which kernel a row length runs on at default settings (the table the binning assertion keeps
honest: expected_kinds() restates it, assert_binning() compares it with timing().kern_rows and
fails with "edge list stale" when a threshold moves).  Lines of csrc/ that decide each edge:
bins gk_maxdeg (kernels.h:46-52) through build_bins (prepare.cpp:133-151) and the stream threshold
(prepare.cpp:196-197); kernel of a bin run_half (sweep.cpp:319-333; k_grow's capacity grow_maxdeg,
kernels.hip:1951; its KL form kernels.hip:1948); streaming set of a row prepare.cpp:262; task size
gstream_cmax (kernels.hip:1961, prepare.cpp:268-269); chunks of a row build_stream_tasks
(prepare.cpp:515, 522).

  f64, users and items alike up to 256 ratings            kern_rows kind
    0..8        k_gblock, one quarter-wave row (GK_W4)        0 gblock_w4
    9..64       k_grow<double,1>, one wave (GK_W16 bin)       1 gblock_w16
    (GK_B2 is empty: the wide one-wave kind takes 33..64)     2 gblock_b2
    65..128     k_grow<double,1>, one wave (GK_B4 bin)        3 gblock_b4
    129..256    k_grow<double,2>, two waves (GK_B8 bin)       4 gblock_b8
    257..       k_gres, the streaming kind                    5 gres_stage
  f64 users   257..512    k_gres<double,4,0>, set 0, tasks of 512: whole rows
              513..1024   k_gres<double,8,0>, set 1, tasks of 1024: whole rows
              1025..2048  set 1, 2 chunks;  2049: 3;  4095, 4096: 4;  4097: 5 (k_split_finish)
  f64 items   257..1024   k_gres<double,8,1>, set 0, tasks of 1024: whole rows
              1025..2048  k_gres<double,16,1>, set 1, tasks of 2048: whole rows
              2049..4096  set 1, 2 chunks;  4097: 3 (k_split_finish)
  f32, users and items alike
    0..16       k_gblock, one quarter-wave row (GK_W4)        0 gblock_w4
    17..64      k_grow<float,1> (GK_W16 bin)                  1 gblock_w16
    65..128     k_grow<float,1> (GK_B2 bin)                   2 gblock_b2
    129..256    k_grow<float,1> (GK_B4 bin)                   3 gblock_b4
    257..512    k_grow<float,2> (GK_B8 bin)                   4 gblock_b8
    513..2048   k_gres<float,8,side>, tasks of 2048: whole    5 gres_stage
    2049..4096  2 chunks;  4097: 3 (k_split_finish)
  k_grow runs its KL = 128 form up to K = 128 and the KL = 256 form above (K = 130 here).
  tune 2048 keeps the f32 bins 1..4 on the multi-wave Gram-block kinds (k_gblock, 1..8 waves);
  tune 128 / 1 << 17 run every streaming row on 4- / 16-wave k_gres (tasks of 512 / 2048 in
  f64, 1024 / 4096 in f32); stream_threshold 40 with split_chunk 64 streams every row above 40
  ratings in tasks of 64: 512 / 513 / 1024 / 1025 / 2048 / 2049 / 4097 ratings are 8 / 9 / 16 /
  17 / 32 / 33 / 65 chunks, around the 8-deep batches of the split-row hand-off.
kern_rows carries the bin of a row, not the streaming set or the chunk count.

Bounds, per row (n ratings, u the restated row in float64):
  f64  max(64 * max|restate(float64) - restate(longdouble)|, K n 2^-52 max|u|): the fold-in
       test's bound with the row's own n.  An empty row, whose floor would be zero, has the floor
       of one term, K 2^-52 max|u| (its draw is the prior's term alone); the GPU test also holds
       it to the closed form mu + sd z.
  f32  max(M * max|restate(float32, strictly sequential sums) - restate(float64)|, 2^-24 max|u|)
       on inputs rounded to float32 (sigma, mu, tau, the normals; the factors and half-star
       ratings already are): the kernel may be M times as far from the exact row as a plain
       float32 loop is, the floor being the rounding of the store.
tests/test_edge_rows_checker.py shows on the CPU that at M = 64 (the most this check allows) a
row computed without its last rating, its last 4-vector or its last chunk is at least 8 bounds
away (57 and more) on the state sweep 0 starts from, for every edge row.  On the state the third
sweep starts from the residuals are smaller and the bound of a long row larger: rows below 1023
ratings keep 38 bounds and a left-out task of 2048 ratings 216, one left-out rating only 2.5 on
the rows of 1023 ratings and more (held there to 2 bounds).

M = F32_M below, from the first run of tests/test_gpu_edge_rows.py's cases on an MI355X (set seed 17,
learner seed 3: {K 20 final, K 20 none, K 100, K 130} x 6 variants x 3 sweeps).  Largest observed
ratio of kernel error to the float32 restatement's error of the same row (0 where the store floor
covers the row), per length class, the larger of users and items:
  0: 3.19, 1: 7.60, 2: 6.12, 7: 5.90, 8: 6.11, 9: 4.72, 15: 3.72, 16: 3.74, 17: 6.22,
  31: 2.76, 32: 3.91, 33: 3.66, 63: 4.36, 64: 2.52, 65: 3.40, 127: 2.57, 128: 3.72, 129: 2.82,
  255: 4.95, 256: 7.35, 257: 2.45, 511: 5.45, 512: 2.76, 513: 2.23, 1023: 2.09, 1024: 2.37, 1025: 3.02,
  2047: 2.84, 2048: 1.78, 2049: 1.78, 4095: 2.41, 4096: 3.53, 4097: 2.80, filler: 11.63
The largest, 11.63, is an item filler row (5..19 ratings, k_gblock / k_grow) at K = 20, quirks none,
sweep 0.
4 x 11.63 = 46.5, so F32_M = 64, the cap.  f64: every row within 0.078 of its bound.  The tables
of error, bound and ratio per (side, length) are in DESIGN.md 5.1.
"""
import functools

import numpy as np

LENGTHS = (0, 1, 2, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513,
           1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096, 4097)
ROWS_PER_LENGTH = 2
FILLERS = 4400
SAMPLE = 200  # filler rows restated beside the edge rows
TAG_USERS, TAG_ITEMS, TAG_INIT_U, TAG_INIT_V = 0, 1, 3, 4
SIDES = ("users", "items")
EPS64, EPS32 = 2.0 ** -52, 2.0 ** -24
F32_M_MAX = 64  # the most the f32 check may allow (a condition of the test)
F32_M = 64      # smallest power of two >= 4 x 11.63, the largest needed M observed (table above)

# the table above: largest row of the bins 0..4 (rows above the last stream), and the largest
# streaming task per (precision, side) and set at default settings
BIN_MAX = {"f64": (8, 64, 64, 128, 256), "f32": (16, 64, 128, 256, 512)}
KIND_NAMES = ("gblock_w4", "gblock_w16", "gblock_b2", "gblock_b4", "gblock_b8", "gres_stage")
STREAM_SETS = {("f64", "users"): ((512, 512), (None, 1024)), ("f64", "items"): ((1024, 1024), (None, 2048)),
               ("f32", "users"): ((None, 2048),), ("f32", "items"): ((None, 2048),)}  # (largest row, task) per set


# ------------------------------------------------------------------ the set
@functools.lru_cache(maxsize=4)
def edge_set(seed):
    """(train, test, dims, edge_rows): train / test are (user, item, rating) arrays, dims =
    (num_users, num_items) -- the two length-0 rows of a side are its last two ids and exist only
    through dims -- and edge_rows[side][length] the ids of the rows of that length.  Ratings are
    half stars in 0.5..5 from a planted rank-6 model plus noise.  One user and one item occur in
    the test set only.  Everything is drawn from `seed`; the arrays are read-only."""
    rng = np.random.default_rng(seed)
    n_edge = ROWS_PER_LENGTH * (len(LENGTHS) - 1)  # rows with ratings
    n_side = n_edge + 1 + FILLERS + ROWS_PER_LENGTH  # + the test-only row, the fillers, the empty rows
    edge_rows, filler, test_only = {}, {}, {}
    for side in SIDES:
        ids = rng.permutation(n_side - ROWS_PER_LENGTH)
        edge_rows[side] = {0: [n_side - 2, n_side - 1]}
        for j, n in enumerate(LENGTHS[1:]):
            edge_rows[side][n] = sorted(int(x) for x in ids[ROWS_PER_LENGTH * j:ROWS_PER_LENGTH * (j + 1)])
        test_only[side] = int(ids[n_edge])
        filler[side] = np.sort(ids[n_edge + 1:])
    A, B = 0.6 * rng.standard_normal((n_side, 6)), 0.6 * rng.standard_normal((n_side, 6))

    def rate(u, i):
        x = 3.3 + np.einsum("nk,nk->n", A[u], B[i]) + 0.4 * rng.standard_normal(len(u))
        return np.clip(np.round(2.0 * x) / 2.0, 0.5, 5.0)

    tu, ti = [], []
    for n in LENGTHS[1:]:
        for u in edge_rows["users"][n]:  # edge users rate filler items only
            tu.append(np.full(n, u))
            ti.append(rng.choice(filler["items"], n, replace=False))
        for i in edge_rows["items"][n]:  # edge items are rated by filler users only
            ti.append(np.full(n, i))
            tu.append(rng.choice(filler["users"], n, replace=False))
    tu, ti = np.concatenate(tu), np.concatenate(ti)
    order = rng.permutation(len(tu))  # file order: no side sorted
    tu, ti = tu[order], ti[order]
    # test: filler x filler and edge x edge pairs (none is in train), the test-only user and item
    eu = np.array([r for n in LENGTHS for r in edge_rows["users"][n]])
    ei = np.array([r for n in LENGTHS for r in edge_rows["items"][n]])
    pairs = {(int(rng.choice(filler["users"])), int(rng.choice(filler["items"]))) for _ in range(1500)}
    pairs |= {(int(rng.choice(eu)), int(rng.choice(ei))) for _ in range(200)}
    pairs |= {(test_only["users"], int(i)) for i in rng.choice(filler["items"], 20, replace=False)}
    pairs |= {(int(u), test_only["items"]) for u in rng.choice(filler["users"], 20, replace=False)}
    pairs.add((test_only["users"], test_only["items"]))
    su, si = (np.array(x) for x in zip(*sorted(pairs)))
    train = (tu.astype(np.uint32), ti.astype(np.uint32), rate(tu, ti))
    test = (su.astype(np.uint32), si.astype(np.uint32), rate(su, si))
    for a in train + test:
        a.setflags(write=False)
    return train, test, (n_side, n_side), edge_rows


@functools.lru_cache(maxsize=4)
def row_lists(seed):
    """Per side the CSR (ptr, partner ids, ratings) of edge_set(seed)'s training ratings, a row's
    ratings in file order."""
    (tu, ti, tr), _, dims, _ = edge_set(seed)
    out = {}
    for side, key, oth, rows in (("users", tu, ti, dims[0]), ("items", ti, tu, dims[1])):
        order = np.argsort(key, kind="stable")
        ptr = np.concatenate([[0], np.cumsum(np.bincount(key, minlength=rows))])
        out[side] = (ptr, oth[order].astype(np.int64), tr[order])
    return out


def degrees(seed, side):
    return np.diff(row_lists(seed)[side][0])


def checked_rows(seed, side):
    """Every edge row of the side plus a seeded sample of SAMPLE other rows."""
    _, _, dims, edge_rows = edge_set(seed)
    edge = sorted(r for rows in edge_rows[side].values() for r in rows)
    rest = np.setdiff1d(np.arange(dims[SIDES.index(side)]), edge)
    pick = np.random.default_rng([seed, SIDES.index(side)]).choice(rest, SAMPLE, replace=False)
    return np.array(edge + sorted(int(x) for x in pick))


# ------------------------------------------------------------------ the table as code
def kind_of(n, precision, stream_threshold=0):
    """kern_rows kind of a row of n ratings (sbmf_config.tune bits 3 / 8..11 change kernels or
    bins; of those the tests here use only bit 11, which keeps the bins)."""
    top = BIN_MAX[precision][-1]
    if n > (min(stream_threshold, top) if stream_threshold else top):
        return 5
    return next(k for k, m in enumerate(BIN_MAX[precision]) if n <= m)


def expected_kinds(seed, precision, stream_threshold=0):
    """[side][kind] row counts of edge_set(seed) as the table has them."""
    out = np.zeros((2, len(KIND_NAMES)), dtype=np.int64)
    for s, side in enumerate(SIDES):
        for n in degrees(seed, side):
            out[s, kind_of(int(n), precision, stream_threshold)] += 1
    return out


def assert_binning(learner, seed, precision, stream_threshold=0):
    """The rows of each side landed in the kinds the table says, as far as timing().kern_rows
    carries it: the bin of a row, not its streaming set or task size (STREAM_SETS is compared
    with LENGTHS only, by table_edges() in tests/test_edge_rows_checker.py).  Returns the kind
    name of every edge length."""
    t = learner.timing()
    got = np.array([[t.kern_rows[s][k] for k in range(len(KIND_NAMES))] for s in range(2)], dtype=np.int64)
    want = expected_kinds(seed, precision, stream_threshold)
    assert np.array_equal(got, want), (
        "edge list stale: %s rows per kind %s are users %s items %s, the table in tests/edge_rows.py has users %s "
        "items %s -- a binning threshold moved: revise BIN_MAX, LENGTHS and the table"
        % (precision, list(KIND_NAMES), got[0].tolist(), got[1].tolist(), want[0].tolist(), want[1].tolist()))
    return {n: KIND_NAMES[kind_of(n, precision, stream_threshold)] for n in LENGTHS}


def table_edges():
    """Every row length the table names as the last of its kind, set or task."""
    edges = set()
    for p in BIN_MAX:
        edges.update(BIN_MAX[p])
    for sets in STREAM_SETS.values():
        for top, task in sets:
            edges.update(x for x in (top, task, 2 * task) if x)
    return sorted(edges)


# ------------------------------------------------------------------ the restatement
def _total(x, dt, sequential):
    """Sum over the last axis in dt: numpy's pairwise sum, or one term after the other."""
    if not sequential:
        return x.sum(axis=-1, dtype=dt)
    if x.shape[-1] == 0:
        return np.zeros(x.shape[:-1], dtype=dt)
    return np.add.accumulate(x, axis=-1, dtype=dt)[..., -1]


def restate_gathered(Pg, sig, mu, tau, u_old, z, r, sd_is_var, dt, sequential=False):
    """The header's coordinate loop (include/sbmf.h; gibbs_sbpmf_final.cpp's row update) in the
    floating type dt for one row -- Pg [n, K] the partner rows of its ratings r [n], u_old and z
    [K] -- or for a stack of rows of one length (a leading axis on Pg, r, u_old and z)."""
    K = u_old.shape[-1]
    Pg = Pg.astype(dt)
    u = u_old.astype(dt).copy()
    sig, mu, z, tau = sig.astype(dt), mu.astype(dt), z.astype(dt), dt(tau)
    if sequential:
        e = r.astype(dt) - _total(Pg * u[..., None, :], dt, True)
    elif u.ndim == 1:
        e = r.astype(dt) - Pg @ u
    else:
        e = r.astype(dt) - np.matmul(Pg, u[..., None])[..., 0]
    for k in range(K):
        v = Pg[..., k]
        uk = u[..., k]
        P = _total(v * v, dt, sequential)
        Q = _total(v * (e + v * uk[..., None]), dt, sequential)
        var = dt(1) / (sig[k] + tau * P)
        mean = var * (tau * Q + sig[k] * mu[k])
        un = mean + (var if sd_is_var else np.sqrt(var)) * z[..., k]
        e = e + v * (uk - un)[..., None]
        u[..., k] = un
    return u


def restate_row(partner, sig, mu, tau, u_old, z, ids, r, sd_is_var, dt, sequential=False):
    """One row's draw from the partner table, the row's hyperparameters, its previous value and
    its K normals.  sequential: every sum strictly left to right in dt."""
    return restate_gathered(partner[np.asarray(ids).astype(np.int64)], sig, mu, tau, u_old, z, r, sd_is_var, dt,
                            sequential)


def to_f32(x):
    return np.asarray(x, dtype=np.float64).astype(np.float32).astype(np.float64)


def f64_bound(a64, ald, n, K):
    """Per row: a64 / ald [rows, K] the float64 and longdouble restatements, n [rows].  The floor
    counts an empty row as one term (the prior's): K n 2^-52 max|u| would be zero there."""
    cond = np.abs(a64 - ald.astype(np.float64)).max(axis=-1)
    return np.maximum(64.0 * cond, K * np.maximum(np.asarray(n), 1) * EPS64 * np.abs(a64).max(axis=-1))


def f32_bound(a64, a32, M):
    d = np.abs(a32.astype(np.float64) - a64).max(axis=-1)
    return np.maximum(M * d, EPS32 * np.abs(a64).max(axis=-1))


class HalfReport:
    """Per checked row of one half-sweep: id, ratings, kernel error, bound, and for f32 the error
    of the float32 restatement (ref_err) and the store floor."""

    def __init__(self, side, rows, n, err, bound, ref_err, floor, finite, edge):
        self.side, self.rows, self.n, self.err, self.bound = side, rows, n, err, bound
        self.ref_err, self.floor, self.finite, self.edge = ref_err, floor, finite, edge

    def need(self):
        """f32: the M each row would need (0 where the store floor covers the row)."""
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where(self.err > self.floor, self.err / self.ref_err, 0.0)

    def classes(self):
        """(label, rows, worst error, its bound, worst error / bound, largest needed M) per
        edge length, then the filler sample."""
        out = []
        need = self.need() if self.ref_err is not None else np.zeros(len(self.rows))
        labels = [(str(n), self.edge & (self.n == n)) for n in LENGTHS] + [("filler", ~self.edge)]
        for label, m in labels:
            if m.any():
                w = np.argmax(np.where(m, self.err / self.bound, -1.0))
                out.append((label, int(m.sum()), self.err[w], self.bound[w], self.err[w] / self.bound[w], need[m].max()))
        return out

    def table(self):
        head = "%-6s %-7s %4s %11s %11s %9s %8s" % ("side", "length", "rows", "max err", "its bound", "err/bound", "needs M")
        return "\n".join([head] + ["%-6s %-7s %4d %11.3e %11.3e %9.3f %8.2f" % ((self.side,) + c) for c in self.classes()])

    def bad(self):
        return [(self.side, int(r), int(n), float(e), float(b)) for r, n, e, b, f in
                zip(self.rows, self.n, self.err, self.bound, self.finite) if not (f and e <= b)]


def check_half(set_seed, side, partner, own_old, own_new, sig, mu, tau, seed, sweep, sd_is_var, f32, M=F32_M,
               quiet=False):
    """One half-sweep against its restatement.  partner: the other side's table the half read
    (users: V before the sweep; items: the library's new U); own_old / own_new: this side's
    table before and after; sig, mu, tau: the sweep's hyper() values of this side; seed, sweep:
    the learner's, for the rows' normals.  Returns a HalfReport and prints its table."""
    from sbmf import philox_normals
    K = own_old.shape[1]
    ptr, oth, rat = row_lists(set_seed)[side]
    _, _, _, edge_rows = edge_set(set_seed)
    edge_ids = {r for rows in edge_rows[side].values() for r in rows}
    rows = checked_rows(set_seed, side)
    n = (ptr[rows + 1] - ptr[rows]).astype(np.int64)
    tag = TAG_USERS if side == "users" else TAG_ITEMS
    z = np.stack([philox_normals(seed, sweep, tag, int(r), K) for r in rows])
    if f32:
        sig, mu, tau, z = to_f32(sig), to_f32(mu), float(to_f32(tau)), to_f32(z)
    want = np.zeros((len(rows), K))
    other = np.zeros((len(rows), K))  # longdouble (f64 runs) or sequential float32 (f32 runs)
    for length in np.unique(n):
        g = np.flatnonzero(n == length)
        idx = np.stack([oth[ptr[r]:ptr[r] + length] for r in rows[g]])
        Pg, r = partner[idx], np.stack([rat[ptr[q]:ptr[q] + length] for q in rows[g]])
        a = (Pg, sig, mu, tau, own_old[rows[g]], z[g], r, sd_is_var)
        want[g] = restate_gathered(*a, np.float64)
        other[g] = restate_gathered(*a, np.float32, True) if f32 else restate_gathered(*a, np.longdouble)
    err = np.abs(own_new[rows] - want).max(axis=1)
    umax = np.abs(want).max(axis=1)
    if f32:
        ref_err, floor = np.abs(other - want).max(axis=1), EPS32 * umax
        bound = np.maximum(M * ref_err, floor)
    else:
        ref_err = floor = None
        bound = f64_bound(want, other, n, K)
    rep = HalfReport(side, rows, n, err, bound, ref_err, floor, np.isfinite(own_new[rows]).all(axis=1),
                     np.array([int(r) in edge_ids for r in rows]))
    if not quiet:
        print("%s half, sweep %d, K=%d, %s%s" % (side, sweep, K, "f32" if f32 else "f64", ", M=%g" % M if f32 else ""))
        print(rep.table())
    return rep
