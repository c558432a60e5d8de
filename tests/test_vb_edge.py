"""CPU side of the online VB learner's row-class edge set (tests/vb_edge.py): the set is
pinned, it holds every class and edge the GPU tests (tests/test_gpu_vb_edge.py) rely on, and
the oracle with its batch count passed through still is the compiled reference on it."""
import hashlib
import os
import re

import numpy as np
import pytest

import oracle
import vb_edge
from conftest import PKG, golden_rmse

TRAIN_SHA256 = "3d8b7854766f1042729382cce2b134486fd05a63d9cb88456cf243bdc453c7b9"


@pytest.fixture(scope="module")
def edge():
    return vb_edge.generate()


def test_generate_is_pinned(edge):
    train, test, (I, J) = edge
    h = hashlib.sha256()
    for a, dt in zip(train, ("<u4", "<u4", "<f8")):
        h.update(np.ascontiguousarray(a, dtype=dt).tobytes())
    assert h.hexdigest() == TRAIN_SHA256
    assert len(train[0]) <= 70000 and I + J <= 12000
    assert int(train[0].max()) == I - 1 and int(train[1].max()) == J - 1  # num_attribute = I + J from the ids alone
    r2 = np.concatenate([train[2], test[2]]) * 2
    assert np.array_equal(r2, np.round(r2)) and r2.min() >= 1 and r2.max() <= 10
    pairs = set(zip(train[0].tolist(), train[1].tolist()))
    assert len(pairs) == len(train[0])
    tpairs = set(zip(test[0].tolist(), test[1].tolist()))
    assert len(tpairs) == len(test[0]) and 1900 <= len(tpairs) <= 2100 and not (pairs & tpairs)
    # the test set reaches the longest rows of both sides
    c = vb_edge.counts(train, I, J)
    assert c["users"][test[0]].max() == c["users"].max() and c["items"][test[1]].max() == c["items"].max()


def test_per_lane_constants_are_the_headers():
    """vb_edge.USER_CPL / ITEM_CPL restate csrc/vbo.h; every class below follows from them."""
    with open(os.path.join(PKG, "csrc", "vbo.h")) as f:
        src = f.read()
    assert int(re.search(r"VB_CASES_PER_LANE\s*=\s*(\d+)\s*;", src).group(1)) == vb_edge.USER_CPL
    assert int(re.search(r"#define\s+SBMF_VB_ITEM_CPL\s+(\d+)", src).group(1)) == vb_edge.ITEM_CPL
    assert re.search(r"VB_ITEM_CASES_PER_LANE\s*=\s*SBMF_VB_ITEM_CPL\s*;", src)


def test_row_class_restates_the_dispatch():
    for cpl in (vb_edge.USER_CPL, vb_edge.ITEM_CPL):
        assert [vb_edge.row_class(n, cpl) for n in (1, cpl, cpl + 1, 2 * cpl, 2 * cpl + 1)] == \
            [(0, 0), (0, 0), (1, 0), (1, 0), (2, 0)]
        full = cpl * 256
        assert vb_edge.row_class(full, cpl) == (8, 0) and vb_edge.row_class(full + 1, cpl) == (8, 1)
        assert vb_edge.row_class(full + 256, cpl) == (8, 1) and vb_edge.row_class(full + 257, cpl) == (8, 2)
        assert vb_edge.row_class(cpl * 128, cpl) == (7, 0) and vb_edge.row_class(cpl * 128 + 1, cpl) == (8, 0)


def test_coverage_holds_every_class_and_edge(edge):
    train, _, (I, J) = edge
    cov = vb_edge.coverage(train, I, J)
    print(vb_edge.coverage_table(cov))
    rows = cov["rows"]
    c = vb_edge.counts(train, I, J)
    for s in vb_edge.SIDES:
        cpl = vb_edge.CPL[s]
        per_lg = {lg: sum(n for (s_, lg_, _), n in rows.items() if s_ == s and lg_ == lg) for lg in range(9)}
        for lg in range(9):
            assert per_lg[lg] > 0, (s, lg)
            assert cov["full"][(s, lg)] >= 1, (s, lg)   # n == cpl << lg
            assert cov["over"][(s, lg)] >= 1, (s, lg)   # n == (cpl << lg) + 1
            if lg <= 7:  # one full task of 256 >> lg rows and a partial one
                assert per_lg[lg] >= (256 >> lg) + 1, (s, lg, per_lg[lg])
        trips = {t for (s_, lg_, t) in rows if s_ == s}
        assert {0, 1, 2} <= trips and max(trips) >= 8, (s, trips)
        # the loop's own edges: the last row of one trip, the first of two; rows of 1, 2, 3
        for n in (1, 2, 3, cpl * 256 + 256, cpl * 256 + 257, 2 * cpl * 256, 2 * cpl * 256 + 1, 750 * cpl):
            assert (c[s] == n).any(), (s, n)
        # mid-class rows for lg 2..7 (neither a full row nor one more)
        for lg in range(2, 8):
            mid = (c[s] > (cpl << (lg - 1)) + 1) & (c[s] < (cpl << lg))
            assert mid.sum() >= (256 >> lg) + 1, (s, lg)
    # the hubs' counts are exact because specials meet fillers only: a case never joins two long rows
    assert (np.minimum(c["users"][train[0]], c["items"][train[1]]) <= 4 * vb_edge.ITEM_CPL).all()


def _same(a, b):
    return (np.array_equal(a["rmse"], b["rmse"]) and np.array_equal(a["mu_v"], b["mu_v"])
            and np.array_equal(a["mu_w"], b["mu_w"]) and np.array_equal(a["pred"], b["pred"])
            and a["alpha"] == b["alpha"] and a["mu0"] == b["mu0"])


def test_num_batch_zero_is_the_references_thirty(edge, ml100k):
    train, test, (I, J) = edge
    kw = dict(K=8, epochs=2, seed=3, num_users=I, num_items=J)
    assert _same(oracle.run_vbo(train, test, **kw), oracle.run_vbo(train, test, num_batch=30, **kw))
    assert not _same(oracle.run_vbo(train, test, **kw), oracle.run_vbo(train, test, num_batch=29, **kw))
    tr, te = ml100k
    assert _same(oracle.run_vbo(tr, te, K=8, epochs=1, seed=1), oracle.run_vbo(tr, te, K=8, epochs=1, seed=1, num_batch=30))


def test_oracle_is_the_reference_on_the_edge_set(edge):
    """Bit for bit, as tests/test_oracle_golden.py has it on ML-100k: the compiled reference's
    printed "%.17g" test RMSE of 3 epochs at its 30 batches (oracle/make_golden.py vbo)."""
    train, test, (I, J) = edge
    gold = golden_rmse("ref_vbo_vbedge_k8_s3_e3.txt")
    o = oracle.run_vbo(train, test, K=8, epochs=3, seed=3, num_users=I, num_items=J, num_batch=30)
    assert len(gold) == 3 and np.array_equal(o["rmse"], gold), (o["rmse"], gold)


@pytest.mark.parametrize("nb", [1, 2, 3])
def test_oracle_finite_at_few_batches(edge, nb):
    train, test, (I, J) = edge
    o = oracle.run_vbo(train, test, K=8, epochs=3, seed=3, num_users=I, num_items=J, num_batch=nb)
    assert o["epochs"] == 3 and np.isfinite(o["rmse"]).all() and np.isfinite(o["alpha"])
    assert np.isfinite(o["mu_v"]).all() and np.isfinite(o["mu_w"]).all() and np.isfinite(o["pred"]).all()


def test_oracle_refuses_an_empty_batch():
    u, r = np.arange(20, dtype=np.uint32), np.full(20, 3.0)
    with pytest.raises(ValueError):
        oracle.run_vbo((u, u, r), (u[:2], u[:2], r[:2]), K=2, epochs=1, num_batch=30)
    with pytest.raises(ValueError):
        oracle.run_vbo((u[:1], u[:1], r[:1]), (u[:1], u[:1], r[:1]), K=2, epochs=1, num_batch=2)
