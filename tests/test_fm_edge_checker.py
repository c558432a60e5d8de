"""The bars of tests/test_gpu_fm_edge.py can see one lost case (CPU only).

For every edge length >= 1 of tests/fm_edge.py's set, both sides, MCMC and ALS at the GPU test's
settings (K = 8, seed 2, 3 iterations): the oracle on the set without the last case (file order) of
one edge row of that length, against the oracle on the full set.  That row's v must move by at
least 1,000 of the 1e-8 factor bar, and the train RMSE (the largest relative change over the
iterations) by at least 1,000 of the rtol 1e-9 bar: a kernel that drops a row's last case -- a
tail loop that ends one trip early, a chunk cut one case short -- is then three orders of
magnitude outside both.

Observed, with the first of the two rows of each length: least row move 11,200 bars (MCMC, users,
31), ALS >= 84,988 (items, 4095); least train-RMSE move 1,427 bars (MCMC, users, 63), ALS >= 3,901
(items, 511).  The 128 oracle runs take 9 s."""
import numpy as np
import pytest

import fm_edge
import oracle
from edge_rows import LENGTHS, row_lists

NEED = 1000.0  # bars


def _without_last_case(side, row):
    """The train triples without the last case, in file order, of the side's row."""
    (tu, ti, tr), _, _ = fm_edge.generate()
    key = tu if side == "users" else ti
    drop = np.flatnonzero(key == row)[-1]
    keep = np.ones(len(tu), bool)
    keep[drop] = False
    return tu[keep], ti[keep], tr[keep]


@pytest.mark.parametrize("side", ["users", "items"])
@pytest.mark.parametrize("method", ["mcmc", "als"])
def test_a_lost_last_case_is_a_thousand_bars_away(method, side):
    _, test, dims = fm_edge.generate()
    full = fm_edge.oracle_run(method)
    rows = fm_edge.rows_of(side)
    ptr = row_lists(fm_edge.SET_SEED)[side][0]
    low = []
    margins = []
    for n in LENGTHS[1:]:
        row = rows[n][0]
        assert ptr[row + 1] - ptr[row] == n
        o = oracle.run_fmm(_without_last_case(side, row), test, K=fm_edge.K, iters=fm_edge.ITERS, seed=fm_edge.SEED,
                           method=method, k0=1, k1=1, init_stdev=fm_edge.INIT_STDEV, regular=fm_edge.REGULAR[method],
                           num_users=dims[0])
        assert o["v"].shape == full["v"].shape
        at = row if side == "users" else dims[0] + row
        dv = np.abs(o["v"][:, at] - full["v"][:, at]).max() / fm_edge.ATOL_FACTOR
        dr = (np.abs(o["rmse_train"] - full["rmse_train"]) / full["rmse_train"]).max() / fm_edge.RTOL_RMSE
        margins.append((n, dv, dr))
        if not (dv >= NEED and dr >= NEED):
            low.append((n, dv, dr))
    print("%s %s: bars moved by the lost last case, per length (row v, train RMSE)" % (method, side))
    for n, dv, dr in margins:
        print("  %-5d %12.0f %12.0f" % (n, dv, dr))
    lv, lr = min(margins, key=lambda m: m[1]), min(margins, key=lambda m: m[2])
    print("%s %s: least row move %.0f bars (length %d), least train-RMSE move %.0f bars (length %d)"
          % (method, side, lv[1], lv[0], lr[2], lr[0]))
    assert not low, "lengths whose lost last case moves less than %g bars (length, row v, train RMSE): %s" % (NEED, low)
