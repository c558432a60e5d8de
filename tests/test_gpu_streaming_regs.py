"""The streaming row kernels (k_gres / k_grow) after their arguments were split into a small
by-value block and a cold block in device memory.

Against the oracle as test_gpu_parity.py does (factors within 1e-7, RMSE trajectory within
1e-9, reference RNG stream), on the paths the split touches: every workgroup shape on both
sides, one / two / seven k-blocks, split rows of few and of many chunks, and the fields that
moved to the cold block (train RMSE, e_from_dot, f32).  Then the Philox chain bit for bit
against the hashes of the commit before the split (tests/golden/streaming_chain_parent.json,
made by tests/workers/streaming_chain.py on that commit's build).

Every case is ML-100k for 3 sweeps."""
import json
import os

import numpy as np
import pytest

import oracle
from conftest import GOLD
from sbmf import Data, FMLearnSBPMF
from workers import streaming_chain

pytestmark = pytest.mark.gpu

SEED = 9
_ORACLE = {}


def _oracle(ml100k, K):
    if K not in _ORACLE:  # one oracle run per K, shared by every case
        tr, te = ml100k
        _ORACLE[K] = oracle.run(tr, te, K=K, iters=3, seed=SEED)
    return _ORACLE[K]


def _run(ml100k, K, **kw):
    tr, te = ml100k
    L = FMLearnSBPMF(num_factor=K, seed=SEED, **kw)
    L.set_data(Data(*tr), Data(*te))
    L.learn(sweeps=3)
    return L


@pytest.mark.parametrize("tune", [0, 128, 1 << 17, 1 << 23])
@pytest.mark.parametrize("chunk", [16, 64, 150])
@pytest.mark.parametrize("K", [16, 17, 100])
def test_streaming_shapes_match_oracle(ml100k, K, chunk, tune):
    """K = 16: one k-block (the first block is the last); 17: two blocks, one live column in
    the tail; 100: the flagship's seven.  split_chunk 16 gives the longest rows more than 30
    chunks (the 8-deep read loop with a remainder, every piece of the chunk sum), 64 and 150
    give 2..16 chunks and task lengths in every size class.  tune: default shapes, 4-wave,
    16-wave, 8-wave user rows -- each of the 4-, 8- and 16-wave kernels on both sides."""
    o = _oracle(ml100k, K)
    L = _run(ml100k, K, stream_threshold=40, split_chunk=chunk, tune=tune)
    U, V = L.factors()
    du, dv = np.abs(U - o["U"]).max(), np.abs(V - o["V"]).max()
    dr = np.abs(L.rmse_trajectory - o["rmse"]).max()
    print("K=%d chunk=%d tune=%d: max|dU|=%.2e max|dV|=%.2e max|dRMSE|=%.2e" % (K, chunk, tune, du, dv, dr))
    assert du < 1e-7
    assert dv < 1e-7
    assert dr < 1e-9


def test_train_rmse_of_split_rows_matches_oracle(ml100k):
    """eval_train with split rows: row_tr / chunk_tr / r_this / lo / hi, all read from the cold
    block in the epilogue.  The train RMSE of the last sweep against the one of the oracle's
    factors (the clamped prediction of every training rating).  Tolerance: the factors agree
    within 1e-7 per entry, so a K-term dot product of entries of magnitude <= m differs by at
    most 2 K m 1e-7 (+ second order); clamping and the RMSE are 1-Lipschitz in a uniform bound
    on the predictions."""
    K = 17
    tr, te = ml100k
    o = _oracle(ml100k, K)
    L = _run(ml100k, K, stream_threshold=40, split_chunk=16, eval_train=True)
    U, V = L.factors()
    assert np.abs(U - o["U"]).max() < 1e-7 and np.abs(V - o["V"]).max() < 1e-7
    np.testing.assert_allclose(L.rmse_trajectory, o["rmse"], rtol=0, atol=1e-9)
    u, i, r = tr[0].astype(np.int64), tr[1].astype(np.int64), tr[2]
    pred = np.clip(np.einsum("nk,nk->n", o["U"][u], o["V"][i]), r.min(), r.max())
    want = float(np.sqrt(np.mean((pred - r) ** 2)))
    got = L.history[-1]["rmse_train"]
    m = max(np.abs(o["U"]).max(), np.abs(o["V"]).max())
    tol = 2 * K * m * 1e-7
    print("train RMSE %.12f, oracle factors %.12f, |d| = %.2e (tol %.2e)" % (got, want, abs(got - want), tol))
    assert abs(got - want) < tol


@pytest.mark.parametrize("kw", [{}, {"stream_threshold": 40, "split_chunk": 16}])
def test_e_from_dot_matches_oracle(ml100k, kw):
    """tune bit 1: the staging's e0 = r - own.partner (r_this and own through the cold block)."""
    K = 17
    o = _oracle(ml100k, K)
    L = _run(ml100k, K, tune=2, **kw)
    U, V = L.factors()
    assert np.abs(U - o["U"]).max() < 1e-7
    assert np.abs(V - o["V"]).max() < 1e-7
    np.testing.assert_allclose(L.rmse_trajectory, o["rmse"], rtol=0, atol=1e-9)


def test_f32_split_rows_within_north_star(ml100k):
    """f32 (64 vectors per wave, its own size classes): RMSE within 1e-3, test_gpu_parity.py's f32 bar."""
    K = 100
    o = _oracle(ml100k, K)
    L = _run(ml100k, K, precision="f32", stream_threshold=40, split_chunk=16)
    err = np.abs(L.rmse_trajectory - o["rmse"]).max()
    print("f32 max |dRMSE| = %.3e" % err)
    assert err < 1e-3


@pytest.fixture(scope="module")
def parent_chain():
    with open(os.path.join(GOLD, "streaming_chain_parent.json")) as f:
        return json.load(f)


@pytest.mark.parametrize("K,name,kw,prec", streaming_chain.CASES,
                         ids=[streaming_chain.case_id(K, n, p) for K, n, _, p in streaming_chain.CASES])
def test_chain_identical_to_parent(ml100k, parent_chain, K, name, kw, prec):
    """Same seed, same bits as the commit before the argument split: U, V and the RMSE list of
    the Philox chain (seed 2015, 3 sweeps), f64 and f32, default settings and 30+-chunk rows."""
    tr, te = ml100k
    want = parent_chain[streaming_chain.case_id(K, name, prec)]
    got = streaming_chain.run_case(tr, te, K, kw, prec)
    assert got["U"] == want["U"]
    assert got["V"] == want["V"]
    assert got["rmse"] == want["rmse"]
