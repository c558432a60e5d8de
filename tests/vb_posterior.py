"""Hand-made posteriors for the online VB lists, and the restatement of what
the list kernels do with them.

A state is a dict: Um, Us [I][K], Vm, Vs [J][K], bum, bus [I], bvm, bvs [J] (means, variances),
mu0, s0, alpha, sigma_0, sigma_w and sigma_v [K].

  write_posterior   the file of INTEGRATION.md 3f from numpy, without the library
  open_with         a prepared FMLearnVBOnline with the file loaded; no epoch is run
  exact_state       every mean a multiple of 1/4 in [-2, 2], every variance one in [1/4, 2]: each
                    product is a multiple of 1/64 below 8 in magnitude, a variance sum is below
                    20 K + 6, so every partial sum is an integer far below 2^53 in units of 1/64 --
                    exact in any summation order
  smooth_state      continuous and seeded, item variances near 1 and small means: the guests'
                    normal equations are strongly diagonally dominant, a scan converges fast
  moments           mean and variance of rows x all items in float64, in the stated association
  moments_fraction  the same for one pair in exact rational arithmetic
  guest_scan        the guests' coordinate scans, serially, in float64 or longdouble
  guest_limit       the scans' fixed point, A m = c solved directly

Top-N: sample_files.expected_topn (one copy)."""
import os
import struct
import tempfile
from fractions import Fraction

import numpy as np

MAGIC = b"SBMFVBP1"
ARRAYS = ("Um", "Us", "Vm", "Vs", "bum", "bus", "bvm", "bvs")


def file_bytes(I, J, K):
    return 24 + 8 * (5 + K) + 16 * (K + 1) * (I + J)


def write_posterior(path, st):
    """magic, uint32 version 1, I, J, K; float64 mu0, s0, alpha, sigma_0, sigma_w, sigma_v[K]; then
    U_mean, U_var, V_mean, V_var, bu_mean, bu_var, bv_mean, bv_var as float64.  Little-endian."""
    I, K = np.shape(st["Um"])
    J = np.shape(st["Vm"])[0]
    assert np.shape(st["Us"]) == (I, K) and np.shape(st["Vs"]) == (J, K) and np.shape(st["Vm"]) == (J, K)
    assert np.shape(st["bum"]) == np.shape(st["bus"]) == (I,) and np.shape(st["bvm"]) == np.shape(st["bvs"]) == (J,)
    assert np.shape(st["sigma_v"]) == (K,)
    with open(path, "wb") as f:
        f.write(MAGIC + struct.pack("<4I", 1, I, J, K))
        f.write(struct.pack("<5d", st["mu0"], st["s0"], st["alpha"], st["sigma_0"], st["sigma_w"]))
        f.write(np.asarray(st["sigma_v"], "<f8").tobytes())
        for k in ARRAYS:
            f.write(np.ascontiguousarray(st[k], "<f8").tobytes())


def default_train(I, J, seed):
    """user 0 rated nothing, the last user everything, the others a seeded part; ratings 3"""
    rng = np.random.default_rng([seed, I, J, 7])
    u, i = [], []
    for user in range(1, I):
        r = np.arange(J) if user == I - 1 else np.flatnonzero(rng.random(J) < rng.random())
        u.append(np.full(len(r), user, np.uint32))
        i.append(r.astype(np.uint32))
    u, i = np.concatenate(u), np.concatenate(i)
    return u, i, np.full(len(u), 3.0)


def open_with(state_or_path, train, **kw):
    """A prepared FMLearnVBOnline on the training set ``train`` = (user, item, rating) with the
    posterior of a file -- or of a state dict -- loaded; no epoch is run (one batch: a hand-made
    set is too small for thirty)."""
    import sbmf

    tmp, path = None, state_or_path
    if isinstance(state_or_path, dict):
        fd, tmp = tempfile.mkstemp(suffix=".vbpost")
        os.close(fd)
        path = tmp
        write_posterior(path, state_or_path)
    try:
        info = sbmf.vb_posterior_file_info(path)
        kw.setdefault("vb_batches", 1)
        kw.setdefault("rng", "philox")
        L = sbmf.FMLearnVBOnline(num_factor=info["num_factor"], **kw)
        try:
            L.set_data(sbmf.Data(*train), None, num_users=info["num_users"], num_items=info["num_items"])
            L.load_vb_posterior(path)
        except Exception:
            L.close()
            raise
        return L
    finally:
        if tmp is not None:
            os.unlink(tmp)


# ------------------------------------------------------------------ states
def exact_state(I, J, K, seed):
    rng = np.random.default_rng([seed, I, J, K])
    mean = lambda *s: rng.integers(-8, 9, s) / 4.0
    var = lambda *s: rng.integers(1, 9, s) / 4.0
    return dict(Um=mean(I, K), Us=var(I, K), Vm=mean(J, K), Vs=var(J, K), bum=mean(I), bus=var(I), bvm=mean(J), bvs=var(J),
                mu0=float(mean()), s0=float(var()), alpha=2.0, sigma_0=1.0, sigma_w=1.5, sigma_v=var(K))


def smooth_state(I, J, K, seed, scale=0.05):
    rng = np.random.default_rng([seed, I, J, K, 1])
    return dict(Um=scale * rng.standard_normal((I, K)), Us=rng.uniform(0.01, 0.03, (I, K)),
                Vm=scale * rng.standard_normal((J, K)), Vs=rng.uniform(0.5, 1.5, (J, K)),
                bum=0.1 * rng.standard_normal(I), bus=rng.uniform(0.01, 0.03, I), bvm=0.3 * rng.standard_normal(J),
                bvs=rng.uniform(0.01, 0.03, J), mu0=3.5, s0=0.001, alpha=1.25, sigma_0=1.0, sigma_w=1.5,
                sigma_v=rng.uniform(1.0, 2.0, K))


# ------------------------------------------------------------------ the moments
def moments(st, rows):
    """(mean, var) [len(rows)][J] in float64: d and tv summed over f in order, then
    mean = ((d + bum) + bvm) + mu0 and var = ((tv + bus) + bvs) + s0."""
    rows = np.asarray(rows, np.int64)
    um, us = np.asarray(st["Um"], np.float64)[rows], np.asarray(st["Us"], np.float64)[rows]
    vm, vs = np.asarray(st["Vm"], np.float64), np.asarray(st["Vs"], np.float64)
    d = np.zeros((len(rows), vm.shape[0]))
    tv = np.zeros_like(d)
    for f in range(vm.shape[1]):
        mu, su, mj, sj = um[:, f, None], us[:, f, None], vm[None, :, f], vs[None, :, f]
        d = d + mu * mj
        tv = tv + ((su * sj + su * (mj * mj)) + sj * (mu * mu))
    mean = ((d + np.asarray(st["bum"])[rows, None]) + np.asarray(st["bvm"])[None, :]) + st["mu0"]
    var = ((tv + np.asarray(st["bus"])[rows, None]) + np.asarray(st["bvs"])[None, :]) + st["s0"]
    return mean, var


def moments_fraction(st, u, j):
    F = lambda x: Fraction(float(x))
    K = np.shape(st["Um"])[1]
    d = sum(F(st["Um"][u, f]) * F(st["Vm"][j, f]) for f in range(K))
    tv = sum(F(st["Us"][u, f]) * F(st["Vs"][j, f]) + F(st["Us"][u, f]) * F(st["Vm"][j, f]) ** 2
             + F(st["Vs"][j, f]) * F(st["Um"][u, f]) ** 2 for f in range(K))
    return (d + F(st["bum"][u]) + F(st["bvm"][j]) + F(st["mu0"]),
            tv + F(st["bus"][u]) + F(st["bvs"][j]) + F(st["s0"]))


# ------------------------------------------------------------------ the guests
def _serial_sum(x):
    """left-to-right sums along the last axis (numpy's add.reduce is pairwise; cumsum is not)"""
    return np.cumsum(x, axis=-1)[..., -1] if x.shape[-1] else np.zeros(x.shape[:-1], x.dtype)


def guest_scan(st, guests, scans, dtype=np.float64, trace=None):
    """The guests' posterior after ``scans`` scans, every sum serial over the guest's ratings in
    their order, in ``dtype``: (row_mean [G][K], row_var [G][K], b_mean [G], b_var [G]).  guests:
    a list of (items, ratings).  The guests run side by side, padded with zero terms behind
    their ratings (x + 0 = x: a guest's numbers are those of a run alone).  trace: a list that
    receives (b, g) copies after every scan."""
    T = dtype
    G, K = len(guests), np.shape(st["Vm"])[1]
    nmax = max([len(it) for it, _ in guests] + [1])
    mu, s, e, m = np.zeros((G, nmax, K), T), np.zeros((G, nmax, K), T), np.zeros((G, nmax), T), np.zeros((G, nmax), T)
    n = np.zeros(G, T)
    for g, (it, r) in enumerate(guests):
        it = np.asarray(it, np.int64)
        k = len(it)
        mu[g, :k], s[g, :k] = np.asarray(st["Vm"], T)[it], np.asarray(st["Vs"], T)[it]
        e[g, :k] = (np.asarray(r, T) - T(st["mu0"])) - np.asarray(st["bvm"], T)[it]
        m[g, :k] = 1
        n[g] = k
    alpha = T(st["alpha"])
    Pb = T(st["sigma_w"]) + alpha * n
    P = np.asarray(st["sigma_v"], T)[None, :] + alpha * _serial_sum(np.swapaxes(mu * mu + s, 1, 2))  # [G][K]
    b, gr = np.zeros(G, T), np.zeros((G, K), T)
    for _ in range(scans):
        bn = alpha * _serial_sum((e + b[:, None]) * m) / Pb
        e = e - (bn - b)[:, None] * m
        b = bn
        for f in range(K):
            x = mu[:, :, f]
            gn = alpha * _serial_sum(x * (e + gr[:, f, None] * x)) / P[:, f]
            e = e - x * (gn - gr[:, f])[:, None]
            gr[:, f] = gn
        if trace is not None:
            trace.append((b.copy(), gr.copy()))
    return gr, 1 / P, b, 1 / Pb


def guest_limit(st, items, ratings):
    """The scans' fixed point of one guest: A m = c with x_j = [1, mu_j],
    A = diag(sigma_w, sigma_v) + alpha sum_j (x_j x_j^T + diag(0, s_j)), c = alpha sum_j x_j (r_j - mu0 - bvm_j);
    returns (b, g [K])."""
    it = np.asarray(items, np.int64)
    K = np.shape(st["Vm"])[1]
    X = np.concatenate([np.ones((len(it), 1)), np.asarray(st["Vm"], np.float64)[it]], axis=1)
    A = np.diag(np.concatenate([[st["sigma_w"]], st["sigma_v"]])) + st["alpha"] * (X.T @ X)
    A[np.arange(1, K + 1), np.arange(1, K + 1)] += st["alpha"] * np.asarray(st["Vs"])[it].sum(axis=0)
    c = st["alpha"] * (X.T @ ((np.asarray(ratings, np.float64) - st["mu0"]) - np.asarray(st["bvm"])[it]))
    sol = np.linalg.solve(A, c)
    return sol[0], sol[1:]


def make_guests(J, lengths, seed):
    """one guest per length: distinct seeded items, ratings in 1..5"""
    rng = np.random.default_rng([seed, J, 3])
    return [(rng.choice(J, n, replace=False).astype(np.uint32), rng.integers(1, 6, n).astype(np.float64)) for n in lengths]
