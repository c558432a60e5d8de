"""Fixtures of the general libFM learner's tests, derived by rule (integer arithmetic on the
committed ML-100k triples), so the libFM text is reproducible and need not be committed.

"fm4": four fields over the ML-100k (user, item, rating) cases --
  A  users, one-hot:   attribute u
  B  items, one-hot:   I + i
  C  (u + 3 i) mod 7, one-hot, x = 1: C0 + c for c < 3, C0 + c + 1 above (the id C0 + 3 is a gap,
     an attribute without any case).  Its seven rows of about 11 k cases exceed the chunk bound.
  D  five tags, multi-hot: tag t (D0 + t) is present when bit t of the item id is set, x = 1 for a
     single tag and 0.5 otherwise; every 97th case's first tag has x = -1.5, every 89th case's last
     tag x = 0.25.  A sixth tag D0 + 5 occurs in the test file only (cases with (u + i) mod 11 == 0,
     x = 0.5): a row drawn from its prior.
Every value is exactly representable in float32 and printed exactly by %g."""
import numpy as np

from sbmf import Cases


def fm4_layout(ml100k):
    (tu, ti, _), (su, si, _) = ml100k
    I = int(max(tu.max(), su.max())) + 1
    J = int(max(ti.max(), si.max())) + 1
    C0 = I + J
    D0 = C0 + 8
    return I, J, C0, D0


def _fm4_rows(u, i, r, layout, test):
    I, J, C0, D0 = layout
    rows = []
    for c, (uu, ii, rr) in enumerate(zip(u.tolist(), i.tolist(), r.tolist())):
        f = [(uu, 1.0), (I + ii, 1.0)]
        cv = (uu + 3 * ii) % 7
        f.append((C0 + cv + (1 if cv >= 3 else 0), 1.0))
        tags = [t for t in range(5) if (ii >> t) & 1]
        xs = [1.0 if len(tags) == 1 else 0.5] * len(tags)
        if tags and c % 97 == 0:
            xs[0] = -1.5
        if tags and c % 89 == 0:
            xs[-1] = 0.25
        f += [(D0 + t, x) for t, x in zip(tags, xs)]
        if test and (uu + ii) % 11 == 0:
            f.append((D0 + 5, 0.5))
        rows.append((rr, f))
    return rows


def rows_to_cases(rows):
    ptr = np.zeros(len(rows) + 1, np.uint64)
    attr, x, y = [], [], []
    for c, (t, f) in enumerate(rows):
        f = sorted(f, key=lambda e: e[0])
        attr += [a for a, _ in f]
        x += [v for _, v in f]
        y.append(t)
        ptr[c + 1] = len(attr)
    return Cases(ptr, np.array(attr, np.uint32), np.array(x, np.float32), np.array(y, np.float32))


def rows_to_text(rows):
    return "".join("%g %s\n" % (t, " ".join("%d:%g" % (a, v) for a, v in f)) for t, f in rows)


_CACHE = {}


def fm4(ml100k):
    """(train Cases, test Cases, train rows, test rows, layout) -- built once per session."""
    if "fm4" not in _CACHE:
        lay = fm4_layout(ml100k)
        tr = _fm4_rows(*ml100k[0], lay, False)
        te = _fm4_rows(*ml100k[1], lay, True)
        _CACHE["fm4"] = (rows_to_cases(tr), rows_to_cases(te), tr, te, lay)
    return _CACHE["fm4"]


def write_fm4(ml100k, dirpath):
    """fm4 as libFM text: <dirpath>/train.libfm and test.libfm; returns the two paths."""
    import os
    _, _, tr, te, _ = fm4(ml100k)
    out = []
    for nm, rows in (("train.libfm", tr), ("test.libfm", te)):
        p = os.path.join(str(dirpath), nm)
        with open(p, "w") as f:
            f.write(rows_to_text(rows))
        out.append(p)
    return out


# the hand-written 12-case file: a case without features, unsorted ids, a comment line, trailing
# blanks, leading blanks, a value that is not exactly representable, an empty line
SMALL_TEXT = """# twelve cases
4 0:1 5:1 9:0.5
3 1:1 6:1
 5 2:1 5:1 10:1
1.5
2 9:0.25 0:1 7:1
4 3:1 6:1 9:-1.5 10:0.5

3.5 1:1 5:1\t
1 4:1 8:0.1
5 0:1 6:1 10:1 # trailing comment
2 2:1 7:1 9:1
4 3:1 8:2
3 4:1 5:0.333333
"""
SMALL_TEST_TEXT = """4 0:1 6:1 9:0.5
2 1:1 5:1 11:1
3
5 2:1 8:1 10:0.25
"""


def parse_text(text):
    """A plain Python parse of libFM text: (ptr, attr, x float32, target float32), entries sorted
    by id within a case (stable)."""
    ptr, attr, x, y = [0], [], [], []
    for line in text.split("\n"):
        s = line.lstrip(" \t")
        if not s or s[0] == "#":
            continue
        s = s.split("#")[0]
        tok = s.split()
        y.append(np.float32(tok[0]))
        f = [(int(t.split(":")[0]), np.float32(t.split(":")[1])) for t in tok[1:]]
        f.sort(key=lambda e: e[0])
        attr += [a for a, _ in f]
        x += [v for _, v in f]
        ptr.append(len(attr))
    return (np.array(ptr, np.uint64), np.array(attr, np.uint32), np.array(x, np.float32), np.array(y, np.float32))


def small_cases():
    return Cases(*parse_text(SMALL_TEXT)), Cases(*parse_text(SMALL_TEST_TEXT))


EDGE_LENGTHS = [0, 1, 63, 64, 65, 255, 256, 257, 1025]


def edge_set():
    """A one-hot field whose nine attributes have exactly the EDGE_LENGTHS cases (the one-wave bin's
    end, the chunk size, the long-row bound, each +-1, and a row of 17 chunks), a 13-valued
    one-hot field with real values beside it, and a two-valued multi-hot field."""
    own = np.repeat(np.arange(len(EDGE_LENGTHS)), EDGE_LENGTHS)
    n = len(own)
    own = own[(np.arange(n) * 7919) % n]  # 7919 is prime to n = 1986: a permutation
    rows = []
    for c in range(n):
        f = [(int(own[c]), 1.0), (9 + c % 13, 0.5 + 0.25 * (c % 4))]
        if c % 3 == 0:
            f.append((22, 0.5))
        if c % 5 < 2:
            f.append((23, -0.75 if c % 7 == 0 else 1.0))
        rows.append((1.0 + (c * 7) % 5, f))
    test = [(1.0 + (c * 3) % 5, [(int(own[c * 17 % n]), 1.0), (9 + c % 13, 1.25), (24, 1.0)]) for c in range(64)]
    return rows_to_cases(rows), rows_to_cases(test)


# ---- libFM's ALS, restated serially in numpy (fm_learn_mcmc.h with do_sample = do_multilevel = 0):
# draw_w0 (:627-668), draw_w (:670-719), add_main_q (:384-409), draw_v (:780-835) and
# predict_data_and_write_to_eterms (:117-348), attribute by attribute in ascending order, in
# the float type `ft` (float64 or longdouble).  The initial model is the reference stream's
# (fm_model::init then w, libfm.cpp:412).
def _csc(cases, p):
    order = np.argsort(cases.attr, kind="stable")
    cid = np.repeat(np.arange(cases.num_cases), np.diff(cases.ptr.astype(np.int64)))
    cnt = np.bincount(cases.attr, minlength=p)
    ap = np.concatenate([[0], np.cumsum(cnt)])
    return ap, cid[order], cases.x[order]


def _predict(cases, w0, w, v, ft, k0=1, k1=1):
    n = cases.num_cases
    cid = np.repeat(np.arange(n), np.diff(cases.ptr.astype(np.int64)))
    x = cases.x.astype(ft)
    e = np.zeros(n, ft)
    q2 = np.zeros(n, ft)
    for f in range(v.shape[0]):
        vx = v[f][cases.attr] * x
        q = np.zeros(n, ft)
        np.add.at(q, cid, vx)
        e += ft(0.5) * q * q
        np.subtract.at(q2, cid, ft(0.5) * v[f][cases.attr] * v[f][cases.attr] * x * x)
    if k1:
        np.add.at(q2, cid, w[cases.attr] * x)
    e = e + q2
    if k0:
        e = e + w0
    return e


def als_restatement(train, test, K, iters, seed, regular, ft=np.float64, init_stdev=0.1, record=()):
    """Returns {iteration: (w0, w, v, train rmse, test predictions)} for the iterations in `record`."""
    with np.errstate(all="ignore"):  # 1 / 0 of an attribute without cases and without a prior precision
        return _als_restatement(train, test, K, iters, seed, regular, ft, init_stdev, record)


def _als_restatement(train, test, K, iters, seed, regular, ft, init_stdev, record):
    import sbmf
    p = max(train.num_attr, test.num_attr) + 1
    z = sbmf.ref_stream(seed, 1, K * p + p)
    v = (z[:K * p].reshape(K, p) * init_stdev).astype(ft)
    w = (z[K * p:] * init_stdev).astype(ft)
    w0 = ft(0.0)
    reg0, regw, regv = (ft(r) for r in regular)
    ap, cs, xs32 = _csc(train, p)
    xs = xs32.astype(ft)
    y = train.target.astype(ft)
    lo, hi = ft(train.target.min()), ft(train.target.max())
    n = train.num_cases
    ccid = np.repeat(np.arange(n), np.diff(train.ptr.astype(np.int64)))
    cx = train.x.astype(ft)
    e = _predict(train, w0, w, v, ft) - y
    alpha = ft(1.0)
    out = {}
    for it in range(1, iters + 1):
        # draw_w0
        m = np.sum(e - w0)
        s2 = ft(1.0) / (reg0 + alpha * n)
        new = -s2 * (alpha * m - ft(0.0) * reg0)
        e -= (w0 - new)
        w0 = new
        # draw_w (w_mu = 0, w_lambda = regw)
        for a in range(p):
            c, x = cs[ap[a]:ap[a + 1]], xs[ap[a]:ap[a + 1]]
            m = np.sum(x * (e[c] - w[a] * x))
            x32 = xs32[ap[a]:ap[a + 1]]  # :678: x_li * x_li is a product of two floats (FM_FLOAT)
            s2 = ft(1.0) / (regw + alpha * np.sum((x32 * x32).astype(ft)))
            new = -s2 * (alpha * m - ft(0.0) * regw) if np.isfinite(s2) else ft(0.0)  # :686-688
            if not np.isfinite(new):  # :697-710: the old value stays, no update
                continue
            e[c] -= x * (w[a] - new)
            w[a] = new
        for f in range(K):
            q = np.zeros(n, ft)
            np.add.at(q, ccid, v[f][train.attr] * cx)
            for a in range(p):
                c, x = cs[ap[a]:ap[a + 1]], xs[ap[a]:ap[a + 1]]
                h = x * (q[c] - x * v[f, a])
                s = np.sum(h * h)
                m = np.sum(h * e[c]) - v[f, a] * s
                s2 = ft(1.0) / (regv + alpha * s)
                new = -s2 * (alpha * m - ft(0.0) * regv) if np.isfinite(s2) else ft(0.0)  # :800-802
                if not np.isfinite(new):  # :811-824
                    continue
                d = v[f, a] - new
                q[c] -= x * d
                e[c] -= h * d
                v[f, a] = new
        pr = _predict(train, w0, w, v, ft)
        e = pr - y
        if it in record:
            rm = np.sqrt(np.mean((np.clip(pr, lo, hi) - y) ** 2))
            pt = np.clip(_predict(test, w0, w, v, ft), lo, hi)
            out[it] = (w0, w.copy(), v.copy(), rm, pt)
    return out
