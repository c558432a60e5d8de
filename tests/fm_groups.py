"""Fixtures of the attribute-group (-meta) tests of the general libFM learner: the group tables
of the three golden sets, the sets and tables written as libFM would read them, and the serial
numpy restatement of libFM's ALS (tests/fm_cases.py) with per-group precisions."""
import gzip
import os

import numpy as np

import fm_cases
from conftest import GOLD


# ---- the group tables (group[a] for every a < num_attribute = largest id over train and test + 2)
def num_attribute(train, test):
    return max(train.num_attr, test.num_attr) + 1


def fm4_groups(ml100k):
    """fm4 (tests/fm_cases.py) in four groups: users 0, items 1, field C with its gap id 2, the tags
    with the test-only tag and libFM's trailing attribute 3."""
    tr, te, _, _, (I, J, C0, D0) = fm_cases.fm4(ml100k)
    g = np.zeros(num_attribute(tr, te), np.uint32)
    g[I:C0] = 1
    g[C0:D0] = 2
    g[D0:] = 3
    return g


def m1m100k_groups(m1m100k):
    """The reference's own two-feature files: users 0, items (and the trailing attribute) 1."""
    (tu, ti, _), (su, si, _) = m1m100k
    I = int(max(tu.max(), su.max())) + 1
    g = np.ones(int(max(ti.max(), si.max())) + 2, np.uint32)
    g[:I] = 0
    return g


def edge_groups():
    """edge_set(): a % 2 over the nine rows at the bin and chunk edges (two interleaved groups),
    group 2 spans the 13-value field and attribute 22, no attribute carries group 3, and the last
    multi-hot attribute, the test-only one and the trailing one are group 4."""
    tr, te = fm_cases.edge_set()
    g = np.zeros(num_attribute(tr, te), np.uint32)
    g[:9] = np.arange(9) % 2
    g[9:23] = 2
    g[23:] = 4
    return g


def cases_to_text(c):
    """libFM text of a Cases set whose values %g prints exactly."""
    out = []
    for k in range(c.num_cases):
        b, e = int(c.ptr[k]), int(c.ptr[k + 1])
        out.append("%g %s\n" % (c.target[k], " ".join("%d:%g" % (a, v) for a, v in zip(c.attr[b:e], c.x[b:e]))))
    return "".join(out)


def write_meta(path, group):
    with open(path, "w") as f:
        f.write("\n".join(str(int(x)) for x in group) + "\n")
    return path


def write_edge(dirpath):
    tr, te = fm_cases.edge_set()
    out = []
    for nm, c in (("train.libfm", tr), ("test.libfm", te)):
        p = os.path.join(str(dirpath), nm)
        with open(p, "w") as f:
            f.write(cases_to_text(c))
        out.append(p)
    return out


# ---- the goldens tests/make_fm_groups_golden.py writes
GOLDEN_RUNS = {
    # name: (set, method, -regular, iterations)
    "ref_libfm_mcmc_fm4_g4_d118_s1_i10": ("fm4", "mcmc", None, 10),
    "ref_libfm_als_fm4_g4_d118_s1_i10": ("fm4", "als", "0,1,2,3,4,5,10,20,30", 10),
    "ref_libfm_mcmc_m1m100k_g2_d118_s1_i10": ("m1m100k", "mcmc", None, 10),
    "ref_libfm_mcmc_edge_g5_d118_s1_i5": ("edge", "mcmc", None, 5),
}


def golden(name):
    """(#Iter lines, predictions, rlog header, rlog rows as float arrays) of a golden run."""
    with open(os.path.join(GOLD, name + ".txt")) as f:
        lines = f.read().splitlines()
    with gzip.open(os.path.join(GOLD, name + "_pred.txt.gz"), "rt") as f:
        pred = np.array([float(x) for x in f.read().split()])
    header, rows = None, None
    rl = os.path.join(GOLD, name + "_rlog.txt.gz")
    if os.path.exists(rl):
        with gzip.open(rl, "rt") as f:
            t = f.read().splitlines()
        header = t[0].split("\t")
        rows = [[float(x) for x in l.split("\t") if x != ""] for l in t[1:]]
    return lines, pred, header, rows


# ---- libFM's ALS with per-group precisions, restated serially (fm_cases._als_restatement with
# w_lambda(g) / v_lambda(g, f) of the drawn attribute's group, fm_learn_mcmc.h:445-455, :565-577)
def als_restatement_groups(train, test, K, iters, seed, reg0, regw_g, regv_g, group, ft=np.float64, init_stdev=0.1,
                           record=()):
    with np.errstate(all="ignore"):
        return _als_groups(train, test, K, iters, seed, reg0, regw_g, regv_g, group, ft, init_stdev, record)


def _als_groups(train, test, K, iters, seed, reg0, regw_g, regv_g, group, ft, init_stdev, record):
    import sbmf
    p = num_attribute(train, test)
    assert len(group) == p
    z = sbmf.ref_stream(seed, 1, K * p + p)
    v = (z[:K * p].reshape(K, p) * init_stdev).astype(ft)
    w = (z[K * p:] * init_stdev).astype(ft)
    w0 = ft(0.0)
    reg0 = ft(reg0)
    regw = np.asarray(regw_g, ft)[group]
    regv = np.asarray(regv_g, ft)[group]
    ap, cs, xs32 = fm_cases._csc(train, p)
    xs = xs32.astype(ft)
    y = train.target.astype(ft)
    lo, hi = ft(train.target.min()), ft(train.target.max())
    n = train.num_cases
    ccid = np.repeat(np.arange(n), np.diff(train.ptr.astype(np.int64)))
    cx = train.x.astype(ft)
    e = fm_cases._predict(train, w0, w, v, ft) - y
    alpha = ft(1.0)
    out = {}
    for it in range(1, iters + 1):
        m = np.sum(e - w0)
        s2 = ft(1.0) / (reg0 + alpha * n)
        new = -s2 * (alpha * m - ft(0.0) * reg0)
        e -= (w0 - new)
        w0 = new
        for a in range(p):
            c, x = cs[ap[a]:ap[a + 1]], xs[ap[a]:ap[a + 1]]
            m = np.sum(x * (e[c] - w[a] * x))
            x32 = xs32[ap[a]:ap[a + 1]]
            s2 = ft(1.0) / (regw[a] + alpha * np.sum((x32 * x32).astype(ft)))
            new = -s2 * (alpha * m - ft(0.0) * regw[a]) if np.isfinite(s2) else ft(0.0)
            if not np.isfinite(new):
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
                s2 = ft(1.0) / (regv[a] + alpha * s)
                new = -s2 * (alpha * m - ft(0.0) * regv[a]) if np.isfinite(s2) else ft(0.0)
                if not np.isfinite(new):
                    continue
                d = v[f, a] - new
                q[c] -= x * d
                e[c] -= h * d
                v[f, a] = new
        pr = fm_cases._predict(train, w0, w, v, ft)
        e = pr - y
        if it in record:
            rm = np.sqrt(np.mean((np.clip(pr, lo, hi) - y) ** 2))
            pt = np.clip(fm_cases._predict(test, w0, w, v, ft), lo, hi)
            out[it] = (w0, w.copy(), v.copy(), rm, pt)
    return out
