"""Hand-made sample files for the sample store, and the float64 restatement
of what the list kernels do with them.

Two constructions make the reference exact:

  injected scores   K = 1 and u = +-1: the score of item j is +-v_j, one true product plus zero
                    padding, so any finite double can be put into any slot of a row;
  exact sums        factors and biases that are multiples of 1/4 with every partial sum far below
                    2^53: every dot product, S1 and S2 is exact in any summation order.

write_samples writes the file from numpy, without the library; open_with loads it into a prepared
learner that has run no sweep; moments restates watch_moments (csrc/recommend_dev.h);
expected_topn is the order the selection has to return; key_families are the rows of scores of
the selection edge set (tests/test_gpu_select_edge.py)."""
import os
import struct
import tempfile

import numpy as np

MAGIC = b"SBMFSMP\n"
TINY = 5e-324  # the smallest denormal


# ------------------------------------------------------------------ the file
def write_samples(path, U, V, precision, sweeps=None, b0=None, bu=None, bv=None):
    """The sample file of INTEGRATION.md 3d from U [S][I][K] and V [S][J][K]: a 40-byte header
    (magic, version 1, precision 0 = f64 | 1 = f32, I, J, K, count, bias, reserved), the samples'
    sweep indices (uint32, oldest first), then per sample U, V without padding in the file's
    precision and, with biases, b0, bu [I], bv [J] as float64.  Little-endian."""
    U, V = np.asarray(U, np.float64), np.asarray(V, np.float64)
    assert U.ndim == 3 and V.ndim == 3 and U.shape[0] == V.shape[0] and U.shape[2] == V.shape[2]
    S, I, K = U.shape
    J = V.shape[1]
    assert precision in ("f64", "f32")
    ft = "<f4" if precision == "f32" else "<f8"
    bias = b0 is not None
    assert bias == (bu is not None) == (bv is not None)
    sweeps = np.arange(S) if sweeps is None else np.asarray(sweeps)
    assert sweeps.shape == (S,)
    if bias:
        b0, bu, bv = np.asarray(b0, np.float64), np.asarray(bu, np.float64), np.asarray(bv, np.float64)
        assert b0.shape == (S,) and bu.shape == (S, I) and bv.shape == (S, J)
    with open(path, "wb") as f:
        f.write(MAGIC + struct.pack("<8I", 1, 1 if precision == "f32" else 0, I, J, K, S, 1 if bias else 0, 0))
        f.write(sweeps.astype("<u4").tobytes())
        for s in range(S):
            f.write(U[s].astype(ft).tobytes())
            f.write(V[s].astype(ft).tobytes())
            if bias:
                f.write(b0[s:s + 1].astype("<f8").tobytes())
                f.write(bu[s].astype("<f8").tobytes())
                f.write(bv[s].astype("<f8").tobytes())


def open_with(path_or_arrays, train, num_users, num_items, **kw):
    """A prepared FMLearnSBPMF on the hand-made training set ``train`` = (user, item, rating) with
    the samples of a file -- or of write_samples' arguments as a dict -- loaded; no sweep is run.
    K, the precision and the bias-ness of the quirk set are the file's unless ``kw`` names them."""
    import sbmf

    tmp = None
    path = path_or_arrays
    if isinstance(path_or_arrays, dict):
        fd, tmp = tempfile.mkstemp(suffix=".samples")
        os.close(fd)
        path = tmp
        write_samples(path, **path_or_arrays)
    try:
        info = sbmf.samples_file_info(path)
        kw.setdefault("num_factor", info["num_factor"])
        kw.setdefault("precision", info["precision"])
        kw.setdefault("quirks", "bias2" if info["bias"] else "final")
        kw.setdefault("rng", "philox")
        L = sbmf.FMLearnSBPMF(**kw)
        try:
            L.set_data(sbmf.Data(*train), None, num_users=num_users, num_items=num_items)
            L.load_samples(path)
        except Exception:
            L.close()
            raise
        return L
    finally:
        if tmp is not None:
            os.unlink(tmp)


# ------------------------------------------------------------------ the restatement
def moments(scores):
    """watch_moments (csrc/recommend_dev.h) on scores [S][...] in float64, in the kernels' expression
    order: s1 and s2 start at 0 and take the samples oldest first (so a lone -0.0 sums to +0.0),
    mean = s1 / S, v = s2 / S - mean * mean, sd = sqrt(v > 0 ? v : 0).  Returns (mean, v, sd)."""
    scores = np.asarray(scores, np.float64)
    with np.errstate(all="ignore"):
        s1 = np.zeros(scores.shape[1:])
        s2 = np.zeros(scores.shape[1:])
        for s in scores:
            s1 = s1 + s
            s2 = s2 + s * s
        nw = float(len(scores))
        mean = s1 / nw
        mm = mean * mean
        v = s2 / nw - mm
        sd = np.sqrt(np.where(v > 0.0, v, 0.0))
    return mean, v, sd


def expected_topn(mean, sd, rated, topn, risk, exclude):
    """The selection's order: key = mean - risk * sd descending, then item ascending; rated items
    left out when ``exclude``; -1 in the slots past the candidates."""
    key = mean - risk * sd
    item = np.arange(len(mean))
    if exclude:
        keep = np.ones(len(mean), bool)
        keep[np.asarray(rated, np.int64)] = False
        item, key = item[keep], key[keep]
    order = item[np.lexsort((item, -key))][:topn]
    out = np.full(topn, -1, np.int64)
    out[:len(order)] = order
    return out


def key_image(key):
    """watch_key (csrc/recommend.hip) in numpy: the unsigned integer whose order is the key's, -0 as +0."""
    key = np.asarray(key, np.float64) + 0.0  # -0.0 + 0.0 = +0.0
    b = key.view(np.uint64)
    return np.where(b >> np.uint64(63), ~b, b | np.uint64(1 << 63))


# ------------------------------------------------------------------ exact comparisons
def bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


def same_bits(got, want, what):
    """Bit equality, the sign of a zero included; the first mismatch in words."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bg, bw = bits(got).reshape(got.shape), bits(want).reshape(got.shape)
    bad = np.flatnonzero(bg != bw)
    if len(bad):
        q = np.unravel_index(bad[0], got.shape)
        raise AssertionError("%s: %d of %d slots differ; first at %s: expected %r (bits %016x), got %r (bits %016x)"
                             % (what, len(bad), got.size, tuple(int(x) for x in q), float(want[q]), int(bw[q]), float(got[q]),
                                int(bg[q])))


def check_row(mean, sd, want, what):
    """A returned (mean, stdev) against ``want`` = moments(...) of the same slots: the mean bit for
    bit; stdev exactly +0.0 wherever the restated variance is not above 0 (inf - inf included) and
    within one ulp of numpy's sqrt of that variance elsewhere -- the variance is the same
    operations on the same exact sums, the ulp covers the device's sqrt alone.  Returns whether
    stdev was bit-equal on every slot."""
    m, v, s = want
    same_bits(mean, m, what + " mean")
    flat = ~(v > 0.0)
    same_bits(sd[flat], np.zeros(int(flat.sum())), what + " stdev where the variance is not above 0")
    err, ulp = np.abs(sd[~flat] - s[~flat]), np.spacing(s[~flat])
    if np.any(err > ulp):
        q = np.flatnonzero(~flat)[int(np.argmax(err > ulp))]
        raise AssertionError("%s stdev: slot %d variance %r: expected %r, got %r" % (what, q, v.flat[q], s.flat[q], sd.flat[q]))
    return bool(np.all(bits(sd) == bits(s)))


# ------------------------------------------------------------------ the selection's families
FAMILY_RISKS = {"spread": (0.0, 1.0, 0.5), "signed_zero": (0.0, 1.0)}  # every other family: (0.0,)
HIGH_RUNS = ((200, 301), (65500, 65601))  # two_values' high value sits here (where J allows)
ZERO_BLOCK = (224, 288)  # neighbours' block of alternating +0.0 / -0.0: 64 items across 255 | 256


def _chain(start, toward, steps):
    out = [start]
    for _ in range(steps):
        out.append(np.nextafter(out[-1], toward))
    return out


def key_families(J, seed):
    """{name: scores [S][J]} of the +1 users (a -1 user sees the negated row, which mirrors the
    order) -- finite, no NaN; the families of DESIGN.md 5.4 that fit J.  Seeded."""
    rng = np.random.default_rng([seed, J])
    j = np.arange(J)
    fam = {}
    fam["all_equal"] = np.full((1, J), 2.75)
    # a high and a low value; the short high run is HIGH_RUNS, the long one 1300 items and HIGH_RUNS
    if J >= 2:
        high = np.zeros(J, bool)
        if J > HIGH_RUNS[0][1]:
            for a, b in HIGH_RUNS:
                high[a:min(b, J)] = True
        else:
            high[J // 3:max(J // 3 + 1, 2 * J // 3)] = True
        fam["two_values"] = np.where(high, 4.5, -1.25)[None]
        if J >= 2048:
            long_ = high.copy()
            long_[J // 8:J // 8 + 1300] = True
            fam["two_values_long"] = np.where(long_, 4.5, -1.25)[None]
    # neighbouring doubles: chains of nextafter steps up and down from 1, -1, 2 (an exponent carry),
    # the smallest normal and 0 (denormals of both signs), scattered over the row; the slots left
    # repeat chain values (ties between distant items); +-0.0 alternate over ZERO_BLOCK
    if J >= 64:
        steps = min(300, max(4, (J - 64) // 12))
        vals = []
        for start in (1.0, -1.0, 2.0, np.finfo(np.float64).tiny, 0.0):
            vals += _chain(start, np.inf, steps) + _chain(start, -np.inf, steps)[1:]
        vals = np.array(vals)
        row = np.concatenate([vals, rng.choice(vals, J - len(vals))]) if J >= len(vals) else rng.choice(vals, J, replace=False)
        row = row[rng.permutation(J)]
        a, b = (ZERO_BLOCK if J >= ZERO_BLOCK[1] else (0, 64))
        row[a:b] = np.where(np.arange(a, b) % 2 == 0, 0.0, -0.0)
        fam["neighbours"] = row[None]
    # equal magnitudes with both signs
    fam["mirror"] = (rng.choice([-1.0, 1.0], J) * rng.integers(1, 50, J) / 4.0)[None]
    # +-10^e times a random mantissa: every key byte varies, squares underflow; a few slots whose
    # squares overflow (inf - inf: the variance's v > 0 ? v : 0 branch)
    wide = rng.choice([-1.0, 1.0], J) * rng.uniform(1.0, 10.0, J) * 10.0 ** rng.integers(-300, 151, J)
    if J >= 16:
        big = np.array([1.5e200, -1.5e200, 7.25e250, -7.25e250, 1e300, -1e300, 1.7e308, -1.7e308])
        wide[rng.choice(J, len(big), replace=False)] = big
    fam["wide"] = wide[None]
    fam["ascending"] = ((j - J // 2) * 0.25)[None]
    fam["descending"] = ((J // 2 - j) * 0.25)[None]
    # two samples m + d and m - d in small integers: mean m and variance d^2 exactly; many items
    # share a mean but not a spread
    m, d = rng.integers(-3, 4, J).astype(np.float64), rng.integers(0, 6, J).astype(np.float64)
    fam["spread"] = np.stack([m + d, m - d])
    # two samples whose sum is +-TINY or +-2 TINY: half of -TINY rounds to -0.0, a mean of -0.0
    # beside means of +0.0 (a lone sample cannot give one: 0.0 + -0.0 = +0.0 in the sums)
    first = rng.choice([TINY, -TINY, 0.0, 2 * TINY, -2 * TINY], J, p=[0.25, 0.35, 0.2, 0.1, 0.1])
    fam["signed_zero"] = np.stack([first, np.zeros(J)])
    for v in fam.values():
        assert v.shape[1] == J and np.isfinite(v).all()
    return fam


def rated_kinds(J, seed):
    """The rated-item sets of the selection edge set, one per kind: nothing, everything,
    everything but c items for every c that is topn - 1, topn or topn + 1 of a topn in {1, 2,
    1023, 1024}, only item 0 and only item J - 1 (the best item of the ascending, descending and
    tied rows), the mask-word edge 31 | 32 | 33 with J - 1, every second item."""
    rng = np.random.default_rng([seed, J, 1])
    every = np.arange(J)
    kinds = [("nothing", every[:0]), ("everything", every)]
    for c in (1, 2, 3, 1022, 1023, 1024, 1025):
        left = np.sort(rng.choice(J, c, replace=False)) if c < J else every
        kinds.append(("all_but_%d" % c, np.setdiff1d(every, left)))
    kinds.append(("only_first", every[:1]))
    kinds.append(("only_last", every[-1:]))
    kinds.append(("word_edge", np.unique([i for i in (31, 32, 33, J - 1) if i < J])))
    kinds.append(("every_second", every[::2]))
    return kinds
