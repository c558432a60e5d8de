"""The online VB kernels at every row class (tests/vb_edge.py: orientation x lane-group size x
loop trips) against the oracle (oracle/vbo_oracle.c with its batch count passed through;
bit-identical to the compiled reference on this set, tests/test_vb_edge.py).

With vb_batches = 1 a batch row is an attribute's whole count, so the set's hubs are rows of
exactly cpl << lg and (cpl << lg) + 1 cases for every lg, rows that run the beyond-the-registers
loops once, twice and up to 16 times, and full and partial tasks of every lane-group size.  The
cases vary the batch count, the slice count (SBMF_VB_SLICES = 1 is the fused item path) and K
(1; 17 = a second, mostly padded 16-block; 256 = the cap).  Tolerances are those of
tests/test_gpu_vbo.py::test_vbo_means_match_oracle.  A failure prints the per-class table."""
import functools

import numpy as np
import pytest

import oracle
import vb_edge
from conftest import golden_rmse
from sbmf import Data, FMLearnVBOnline, SBMFError
from sbmf._lib import SBMF_E_ARG

pytestmark = pytest.mark.gpu
SEED = 3


@functools.lru_cache(maxsize=None)
def _oracle(nb, K, epochs):
    """One oracle run per (batches, K, epochs), shared by the cases that differ only in slices."""
    train, test, (I, J) = vb_edge.generate()
    o = oracle.run_vbo(train, test, K=K, epochs=epochs, seed=SEED, num_users=I, num_items=J, num_batch=nb)
    for a in (o["rmse"], o["pred"], o["mu_w"], o["mu_v"]):
        a.setflags(write=False)
    return o


def _learner(nb, K, monkeypatch, slices=8, rng="ref"):
    train, test, (I, J) = vb_edge.generate()
    if slices == 8:  # the default
        monkeypatch.delenv("SBMF_VB_SLICES", raising=False)
    else:
        monkeypatch.setenv("SBMF_VB_SLICES", str(slices))
    L = FMLearnVBOnline(num_factor=K, seed=SEED, rng=rng, vb_batches=nb)
    L.set_data(Data(*train), Data(*test), num_users=I, num_items=J)  # vbo_create reads the slice count here
    return L


# vb_batches, slices, K, epochs
CASES = [(1, 1, 8, 3),    # exact row lengths; fused item kernels; item loops of 1, 2 and more trips
         (1, 8, 8, 3),    # the default path: sub-rows per slice, masks, filler tasks
         (1, 3, 8, 3),    # a slice count that is no power of two
         (2, 1, 8, 3),    # batch-to-batch state (rho, t_w, t_v, pending D, hyper blends); the 3000 / 6000 hubs still loop
         (3, 8, 17, 2),   # Kp = 32 with 15 padded columns
         (30, 8, 8, 3),   # the reference's setting; also against the compiled reference's golden
         (1, 8, 1, 3),    # one factor
         (1, 1, 256, 1)]  # the KBMAX cap


@pytest.mark.parametrize("nb,slices,K,epochs", CASES)
def test_vb_edge_matches_oracle(monkeypatch, nb, slices, K, epochs):
    train, _, (I, J) = vb_edge.generate()
    o = _oracle(nb, K, epochs)
    L = _learner(nb, K, monkeypatch, slices)
    L.learn(sweeps=epochs)
    U, V = L.factors()
    bu, bv, b0 = L.biases()
    rmse, alpha, pred = L.rmse_trajectory.copy(), L.hyper()["tau"], L.predict()
    launches = L.timing().n_launch
    L.close()
    # the slice count took effect: an epoch's launches as csrc/vbo.cpp counts them per batch,
    # 2K + 12, and K + 1 combine launches (k_item_w, k_item_v) only when the item rows are sliced
    assert launches == nb * (2 * K + 12 + (K + 1 if slices > 1 else 0)), (launches, nb, slices, K)
    got = {"U": U, "V": V, "bu": bu, "bv": bv}
    want = {"U": o["mu_v"][:I], "V": o["mu_v"][I:], "bu": o["mu_w"][:I], "bv": o["mu_w"][I:]}
    d = {k: np.abs(got[k] - want[k]).max() for k in got}
    print("vb edge nb=%d slices=%d K=%d: max|dRMSE| %.2e max|dU| %.2e max|dV| %.2e max|dbu| %.2e max|dbv| %.2e "
          "|db0| %.2e rel|dalpha| %.2e max|dpred| %.2e" % (
              nb, slices, K, np.abs(rmse - o["rmse"]).max(), d["U"], d["V"], d["bu"], d["bv"], abs(b0 - o["mu0"]),
              abs(alpha - o["alpha"]) / o["alpha"], np.abs(pred - o["pred"]).max()))
    ok = (len(rmse) == epochs and np.abs(rmse - o["rmse"]).max() < 1e-9 and max(d.values()) < 1e-8
          and np.isfinite(U).all() and np.isfinite(V).all())
    if not ok:
        vb_edge.report(got, want, train, I, J)
    assert len(rmse) == epochs and np.abs(rmse - o["rmse"]).max() < 1e-9
    assert d["U"] < 1e-8 and d["V"] < 1e-8
    assert d["bu"] < 1e-8 and d["bv"] < 1e-8
    assert abs(b0 - o["mu0"]) < 1e-10
    assert abs(alpha - o["alpha"]) < 1e-9 * o["alpha"]
    np.testing.assert_allclose(pred, o["pred"], rtol=0, atol=1e-9)
    if nb == 30:
        assert np.abs(rmse - golden_rmse("ref_vbo_vbedge_k8_s3_e3.txt")).max() < 1e-9


def test_vb_edge_philox_repeatable(monkeypatch):
    """Every reduction has a fixed order at every class: two throughput-mode runs are bitwise equal."""
    runs = []
    for _ in range(2):
        L = _learner(2, 8, monkeypatch, rng="philox")
        L.learn(sweeps=2)
        runs.append((L.rmse_trajectory.copy(),) + tuple(L.factors()) + tuple(L.biases()[:2]))
        L.close()
    assert np.isfinite(runs[0][0]).all()
    for a, b in zip(*runs):
        assert np.array_equal(a, b)


def test_vb_edge_continues_across_learn_calls(monkeypatch):
    a = _learner(3, 8, monkeypatch)
    a.learn(sweeps=2)
    b = _learner(3, 8, monkeypatch)
    b.learn(sweeps=1)
    b.learn(sweeps=1)
    assert np.array_equal(a.rmse_trajectory, b.rmse_trajectory)
    for x, y in zip(a.factors() + a.biases()[:2], b.factors() + b.biases()[:2]):
        assert np.array_equal(x, y)
    a.close()
    b.close()


@pytest.mark.parametrize("n,nb", [(20, 30), (1, 2)])
def test_vb_empty_batch_is_an_argument_error(n, nb):
    """ceil(N / batches) cases per batch leave the last batch empty: the reference divides by zero
    there, the library refuses the data."""
    u = np.arange(n, dtype=np.uint32)
    r = 0.5 + 0.5 * (np.arange(n) % 10)
    L = FMLearnVBOnline(num_factor=4, seed=1, vb_batches=nb)
    with pytest.raises(SBMFError) as e:
        L.set_data(Data(u, u % 7, r), Data(u[:1], u[:1] % 7, r[:1]))
        L.learn(sweeps=1)
    assert e.value.code == SBMF_E_ARG and "empty" in str(e.value)
    L.close()
