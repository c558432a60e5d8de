"""The row kernels (k_gblock, k_grow, k_gres, k_split_finish) row by row on the edge set of
tests/edge_rows.py: rows of 0 .. 4097 ratings on both sides, one of every length the host code
dispatches on and its neighbours (the table, the checker and both bounds are in that module's text;
tests/test_edge_rows_checker.py validates the checker on the CPU).

a. Per-row conditional, f32 and f64: Philox, pipeline 0, three sweeps, each half of each sweep
   restated from the state the library returned before it; every edge row and 200 filler rows per
   side inside their bound, every row finite, the empty rows equal to their prior draw; the rows of
   each side in the kinds the table says ("edge list stale" otherwise).
b. f64 parity of the set with the oracle under test_gpu_parity.py's bars.
c. f32 against the f64 oracle under the suite's f32 bars (RMSE 1e-3, factors 5e-2).

Observed on an MI355X: a. no row of any case outside its bound; f64 rows within 0.078 of theirs;
f32 rows need M <= 11.63 against the float32 restatement (edge rows <= 7.60), hence M = 64 (the
per-length ratios are in tests/edge_rows.py, the tables in DESIGN.md 5.1).  b. max|dU|, max|dV| <= 5.1e-14,
max|dRMSE| <= 1.6e-15, tau within 1.8e-14 relative.  c. max|dRMSE| <= 2.5e-8, factors within 2.6e-6.
The 69 cases take 39 s together, the slowest (f64, K = 130: the longdouble restatement) 1.7 s."""
import functools

import numpy as np
import pytest

import oracle
from edge_rows import LENGTHS, TAG_ITEMS, TAG_USERS, assert_binning, check_half, edge_set, to_f32
from sbmf import Data, FMLearnSBPMF, philox_normals

pytestmark = pytest.mark.gpu

SET_SEED = 17  # the set tests/test_edge_rows_checker.py validates
SPLIT = {"stream_threshold": 40, "split_chunk": 64}
VARIANTS = {
    "default": {},
    "carried": {"recompute_every": 0},   # the bench mode: residuals carried from sweep to sweep
    "gblock32": {"tune": 2048},          # f32 rows of 17..512 ratings on the multi-wave Gram-block kinds
    "gres16": {"tune": 1 << 17},         # 16-wave k_gres on both sides
    "gres4": {"tune": 128},              # 4-wave k_gres on both sides
    "split64": SPLIT,                    # 8 / 9 / 16 / 17 / 32 / 33 / 65 chunks
}


def _learner(**kw):
    train, test, dims, _ = edge_set(SET_SEED)
    L = FMLearnSBPMF(**kw)
    L.set_data(Data(*train), Data(*test), num_users=dims[0], num_items=dims[1])
    assert L.dims()[:2] == dims
    return L


# ---- a. the per-row conditional
@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("K,quirks", [(20, "final"), (20, "none"), (100, "final"), (130, "final")])
@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_every_row_is_its_conditional(precision, K, quirks, variant):
    kw = VARIANTS[variant]
    seed, f32, sd_is_var = 3, precision == "f32", quirks != "none"
    _, _, _, edge_rows = edge_set(SET_SEED)
    L = _learner(num_factor=K, seed=seed, rng="philox", quirks=quirks, precision=precision, pipeline=0, **kw)
    kinds = assert_binning(L, SET_SEED, precision, kw.get("stream_threshold", 0))
    print("%s %s: kind of each edge length, users and items: %s" % (precision, variant, kinds))
    U0, V0 = L.factors()
    bad = []
    for sweep in range(3):
        L.learn(sweeps=1)
        U1, V1 = L.factors()
        h = L.hyper()
        assert np.isfinite(U1).all() and np.isfinite(V1).all(), sweep
        for side, partner, old, new, tag in (("users", V0, U0, U1, TAG_USERS), ("items", U1, V0, V1, TAG_ITEMS)):
            key = {"users": "u", "items": "v"}[side]
            sig, mu = h["sigma_" + key], h["mu_" + key]
            rep = check_half(SET_SEED, side, partner, old, new, sig, mu, h["tau"], seed, sweep, sd_is_var, f32)
            bad += [(sweep,) + b for b in rep.bad()]
            for row in edge_rows[side][0]:
                # no ratings: the prior draw mu + sd z.  The kernels form it as old + (draw - old)
                # (the residual update needs the change), so its eight roundings in the row's type
                # are at the size of the old value too; and the device's normal r cos(t) is the
                # host's to the last bits of log / sincos, an absolute 2^-52 r with r = sqrt(-2 log u)
                # <= 8.6, whatever the size of z
                z = philox_normals(seed, sweep, tag, row, K)
                s, m, unit = (to_f32(sig), to_f32(mu), 2.0 ** -24) if f32 else (sig, mu, 2.0 ** -53)
                z = to_f32(z) if f32 else z
                sd = 1.0 / s if sd_is_var else np.sqrt(1.0 / s)
                tol = 8 * unit * (np.abs(m) + np.abs(sd * z) + np.abs(old[row])) + sd * 8.6 * 2.0 ** -52
                assert np.all(np.abs(new[row] - (m + sd * z)) <= tol), (side, row, sweep)
        U0, V0 = U1, V1
    L.close()
    assert not bad, "rows outside their bound (sweep, side, row, ratings, error, bound): %s" % bad[:20]


# ---- b. f64 parity with the oracle
@functools.lru_cache(maxsize=None)
def _oracle(K, iters, seed, rng, quirks="final"):
    train, test, dims, _ = edge_set(SET_SEED)
    return oracle.run(train, test, K=K, iters=iters, seed=seed, rng=rng, quirks=quirks, num_users=dims[0], num_items=dims[1])


def _by_length(side, err):
    """max error by (side, length) over the edge rows, then over every other row."""
    _, _, dims, edge_rows = edge_set(SET_SEED)
    rest = np.ones(len(err), bool)
    out = []
    for n in LENGTHS:
        out.append("%s %d: %.2e" % (side, n, err[edge_rows[side][n]].max()))
        rest[edge_rows[side][n]] = False
    return ", ".join(out + ["%s filler: %.2e" % (side, err[rest].max())])


def _parity(L, o, sweeps):
    L.learn(sweeps=sweeps)
    U, V = L.factors()
    du, dv = np.abs(U - o["U"]).max(axis=1), np.abs(V - o["V"]).max(axis=1)
    tau = L.hyper()["tau"]
    dr = np.abs(L.rmse_trajectory - o["rmse"]).max()
    if not (du.max() < 1e-7 and dv.max() < 1e-7):
        print(_by_length("users", du))
        print(_by_length("items", dv))
    print("max|dU| %.3e max|dV| %.3e max|dRMSE| %.3e dtau/tau %.3e" % (du.max(), dv.max(), dr, abs(tau / o["tau"][-1] - 1)))
    assert du.max() < 1e-7 and dv.max() < 1e-7
    assert abs(tau - o["tau"][-1]) < 1e-9 * o["tau"][-1]
    np.testing.assert_allclose(L.rmse_trajectory, o["rmse"], rtol=0, atol=1e-9)


@pytest.mark.parametrize("K", [8, 20, 100, 256])
@pytest.mark.parametrize("mode", ["ref", "philox", "tune2", "split64"])
def test_f64_parity_with_the_oracle(mode, K):
    rng = "philox" if mode == "philox" else "ref"
    kw = {"tune2": {"tune": 2}, "split64": SPLIT}.get(mode, {})
    L = _learner(num_factor=K, seed=6, rng=rng, **kw)
    _parity(L, _oracle(K, 2, 6, rng), 2)
    L.close()


def test_f64_biased_sampler_parity_with_the_oracle():
    o = _oracle(20, 2, 6, "ref", "bias2")
    L = _learner(num_factor=20, seed=6, quirks="bias2")
    _parity(L, o, 2)
    bu, bv, b0 = L.biases()
    assert np.abs(bu - o["bu"]).max() < 1e-7 and np.abs(bv - o["bv"]).max() < 1e-7 and abs(b0 - o["b0"]) < 1e-9
    L.close()


# ---- c. f32 under the suite's f32 bars
@pytest.mark.parametrize("K,kw", [(20, {}), (20, {"tune": 2048}), (20, SPLIT), (130, {})])
def test_f32_within_the_north_star_bars(K, kw):
    o = _oracle(K, 3, 6, "ref")
    L = _learner(num_factor=K, seed=6, precision="f32", **kw)
    L.learn(sweeps=3)
    U, V = L.factors()
    dr = np.abs(L.rmse_trajectory - o["rmse"]).max()
    print("f32 K=%d %s: max|dRMSE| %.3e max|dU| %.3e max|dV| %.3e" % (K, kw, dr, np.abs(U - o["U"]).max(), np.abs(V - o["V"]).max()))
    assert dr < 1e-3
    assert np.abs(U - o["U"]).max() < 5e-2 and np.abs(V - o["V"]).max() < 5e-2
    L.close()
