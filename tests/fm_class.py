"""Fixtures of the classification (libFM's -task c) tests of the two libFM learners: the rating
sets of the other libFM tests with the target binarised (+1 for a rating >= 4, else -1), the edge
set with a fixed +- pattern, the table of golden runs tests/make_fm_class_golden.py writes, and a
serial numpy restatement of libFM's ALS classification."""
import gzip
import json
import math
import os

import numpy as np

import fm_cases
import fm_groups
from conftest import GOLD
from sbmf import Cases


def binarise(r):
    return np.where(np.asarray(r) >= 4, 1.0, -1.0)


def with_targets(c, y):
    return Cases(c.ptr, c.attr, c.x, np.asarray(y, np.float32))


def write_m1m100k_class(dirpath):
    """The reference's m1m100k libFM files with the binarised target, as train_libfm / test_libfm."""
    out = []
    for nm in ("train", "test"):
        p = os.path.join(str(dirpath), nm + "_libfm")
        with gzip.open(os.path.join(GOLD, "m1m100k_%s_libfm.gz" % nm), "rt") as f, open(p, "w") as g:
            for line in f:
                t = line.split()
                if t:
                    g.write(" ".join(["1" if float(t[0]) >= 4 else "-1"] + t[1:]) + "\n")
        out.append(p)
    return out


def m1m100k_class(m1m100k):
    """((user feature, item feature, +-1), the same of the test file) of the conftest fixture."""
    (tu, ti, tr), (su, si, sr) = m1m100k
    return (tu, ti, binarise(tr)), (su, si, binarise(sr))


def fm4_class(ml100k):
    tr, te = fm_cases.fm4(ml100k)[:2]
    return with_targets(tr, binarise(tr.target)), with_targets(te, binarise(te.target))


def write_cases(dirpath, tr, te):
    out = []
    for nm, c in (("train.libfm", tr), ("test.libfm", te)):
        p = os.path.join(str(dirpath), nm)
        with open(p, "w") as f:
            f.write(fm_groups.cases_to_text(c))
        out.append(p)
    return out


def edge_class():
    """edge_set() with the targets replaced by a fixed pattern: -1 where (5 c + c // 3) % 3 == 0, else
    +1; every case of attribute 2 (a row of 63 cases) positive; one more train case, without features,
    negative; the test targets alternate in pairs."""
    tr, te = fm_cases.edge_set()
    n = tr.num_cases
    c = np.arange(n)
    y = np.where((5 * c + c // 3) % 3 == 0, -1.0, 1.0)
    first = tr.attr[tr.ptr[:-1].astype(np.int64)]  # the one-hot field's attribute is a case's smallest id
    y[first == 2] = 1.0
    assert (first == 2).sum() == 63 and (y < 0).sum() > n // 4
    tr = Cases(np.concatenate([tr.ptr, tr.ptr[-1:]]), tr.attr, tr.x, np.concatenate([y, [-1.0]]).astype(np.float32))
    te = with_targets(te, np.where(np.arange(te.num_cases) % 4 < 2, 1.0, -1.0))
    return tr, te


# ---- the goldens tests/make_fm_class_golden.py writes
ALS_REG = "0,1,10"
GOLDEN_RUNS = {
    # name: (set, method, -regular, iterations, with -meta)
    "ref_libfm_c_mcmc_m1m100k_i8": ("m1m100k", "mcmc", None, 8, False),
    "ref_libfm_c_als_m1m100k_i8": ("m1m100k", "als", ALS_REG, 8, False),
    "ref_libfm_c_mcmc_fm4_i8": ("fm4", "mcmc", None, 8, False),
    "ref_libfm_c_als_fm4_i8": ("fm4", "als", ALS_REG, 8, False),
    "ref_libfm_c_mcmc_fm4_g4_i6": ("fm4", "mcmc", None, 6, True),
    "ref_libfm_c_mcmc_edge_i5": ("edge", "mcmc", None, 5, False),
}
SEEDS_GOLDEN = "ref_libfm_c_mcmc_m1m100k_i8_seeds.json"  # {"train": [16], "test": [16]}: the final lines at LIBFM_PIN_TIME 1..16
RLOG_COLUMNS = ("accuracy", "alpha", "acc_mcmc_this", "acc_mcmc_all", "ll_mcmc_this")


def strip_map(line):
    """A "#Iter=" line of the reference without its "\\tMAP@5= ..." field."""
    return line.split("\tMAP@")[0]


def golden(name):
    """(#Iter lines without MAP@5, predictions, rlog header, rlog rows) of a golden run."""
    lines, pred, header, rows = fm_groups.golden(name)
    return [strip_map(l) for l in lines], pred, header, rows


def seeds_golden():
    with open(os.path.join(GOLD, SEEDS_GOLDEN)) as f:
        return json.load(f)


def iter_values(lines):
    return ([float(l.split("Train=")[1].split()[0]) for l in lines],
            [float(l.split("Test=")[1].split()[0]) for l in lines])


def means_agree(a, b):
    """|mean a - mean b| <= 3 sqrt(s_a^2 / n_a + s_b^2 / n_b), sample variances."""
    a, b = np.asarray(a, float), np.asarray(b, float)
    return abs(a.mean() - b.mean()) <= 3.0 * math.sqrt(a.var(ddof=1) / len(a) + b.var(ddof=1) / len(b))


# ---- the truncated normals of the latent targets
def tgauss_moments(mean, positive):
    """Mean and variance of N(mean, 1) truncated to (0, inf) (positive) or (-inf, 0), with math.erfc."""
    m = mean if positive else -mean  # the negative side mirrors
    z = 0.5 * math.erfc(-m / math.sqrt(2.0))  # P(x > 0)
    lam = math.exp(-0.5 * m * m) / math.sqrt(2.0 * math.pi) / z
    ex = m + lam
    var = 1.0 - lam * (lam + m)
    return (ex if positive else -ex), var


def tgauss_fourth_central(mean, positive, n=200001):
    """The fourth central moment, by quadrature: the standard error of a sample variance needs it."""
    m = mean if positive else -mean
    x = np.linspace(0.0, max(m, 0.0) + 12.0, n)
    trapz = getattr(np, "trapezoid", None) or np.trapz
    pdf = np.exp(-0.5 * (x - m) ** 2)
    pdf /= trapz(pdf, x)
    ex = trapz(x * pdf, x)
    return float(trapz((x - ex) ** 4 * pdf, x))


# ---- the reference's own erf / cdf_gaussian (util/random.h:47-69) and libFM's ALS classification,
# restated serially (fm_cases._als_restatement with the evaluate step of
# fm_learn_mcmc_simultaneous.h:176-222 in place of e = prediction - y)
def ref_erf(x, ft):
    x = np.asarray(x, ft)
    t = ft(1.0) / (ft(1.0) + ft(0.3275911) * np.abs(x))
    r = ft(1.0) - (t * (ft(0.254829592) + t * (ft(-0.284496736) + t * (ft(1.421413741) + t * (
        ft(-1.453152027) + t * ft(1.061405429)))))) * np.exp(-x * x)
    return np.where(x >= 0, r, -r)


def ref_cdf(x, ft):
    return ft(0.5) + ft(0.5) * ref_erf(ft(0.707106781) * np.asarray(x, ft), ft)


def als_class_restatement(train, test, K, iters, seed, regular, ft=np.float64, init_stdev=0.1):
    """Per iteration 1..iters: (train accuracy, test accuracy of the running mean, of this iteration,
    ll of this iteration, test probabilities, w0, w, v)."""
    with np.errstate(all="ignore"):
        return _als_class(train, test, K, iters, seed, regular, ft, init_stdev)


def _als_class(train, test, K, iters, seed, regular, ft, init_stdev):
    import sbmf
    p = max(train.num_attr, test.num_attr) + 1
    z = sbmf.ref_stream(seed, 1, K * p + p)
    v = (z[:K * p].reshape(K, p) * init_stdev).astype(ft)
    w = (z[K * p:] * init_stdev).astype(ft)
    w0 = ft(0.0)
    reg0, regw, regv = (ft(r) for r in regular)
    ap, cs, xs32 = fm_cases._csc(train, p)
    xs = xs32.astype(ft)
    y = np.where(train.target <= 0, -1.0, 1.0).astype(ft)
    yt = np.where(test.target <= 0, -1.0, 1.0).astype(ft)
    n = train.num_cases
    ccid = np.repeat(np.arange(n), np.diff(train.ptr.astype(np.int64)))
    cx = train.x.astype(ft)
    e = fm_cases._predict(train, w0, w, v, ft) - y
    alpha = ft(1.0)
    vote = lambda pp, t: float(np.mean(((pp >= 0.5) & (t > 0)) | ((pp < 0.5) & (t < 0))))
    psum = np.zeros(test.num_cases, ft)
    out = []
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
            s2 = ft(1.0) / (regw + alpha * np.sum((x32 * x32).astype(ft)))
            new = -s2 * (alpha * m - ft(0.0) * regw) if np.isfinite(s2) else ft(0.0)
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
                s2 = ft(1.0) / (regv + alpha * s)
                new = -s2 * (alpha * m - ft(0.0) * regv) if np.isfinite(s2) else ft(0.0)
                if not np.isfinite(new):
                    continue
                d = v[f, a] - new
                q[c] -= x * d
                e[c] -= h * d
                v[f, a] = new
        # the evaluate step: test, then train with the expected value of the truncated normal
        pt = ref_cdf(fm_cases._predict(test, w0, w, v, ft), ft)
        psum += pt
        mu = fm_cases._predict(train, w0, w, v, ft)
        acc_train = vote(ref_cdf(mu, ft), y)
        phi = np.exp(-mu * mu / ft(2.0)) / np.sqrt(ft(3.141) * ft(2))
        Phi = ref_cdf(-mu, ft)
        target = np.where(y >= 0, mu + phi / (ft(1) - Phi), mu - phi / Phi)
        e = mu - target
        mm = (yt + ft(1.0)) * ft(0.5)
        pll = np.clip(pt, ft(0.01), ft(0.99))
        ll = float(np.mean(-(mm * np.log10(pll) + (ft(1) - mm) * np.log10(ft(1) - pll)))) if len(pt) else float("nan")
        out.append((acc_train, vote(psum * (ft(1.0) / ft(it)), yt), vote(pt, yt), ll, np.clip(pt, 0.0, 1.0).copy(),
                    w0, w.copy(), v.copy()))
    return out
