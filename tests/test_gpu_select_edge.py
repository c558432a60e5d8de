"""Selection edge set: k_watch_select -- the one selection of the library
(select_topn, csrc/lists.cpp) -- on rows of hand-made scores, exact.

The samples come from a file written by numpy (tests/sample_files.py) with K = 1 and u = +-1, so
the score of item j is +-v_j: one true product plus zero padding, any finite double in any slot.
Users with an even id have u = +1, users with an odd id u = -1: every family also runs mirrored,
the bottom of the order on top and the winners through watch_key's negative branch.  Each kind of
rated-item set (sample_files.rated_kinds) belongs to one user of either sign.

Every comparison is exact.  The rows' mean must equal the restated moments bit for bit (the sign
of a zero included); stdev is exactly 0 wherever the restated variance is not above 0 and within
one ulp of numpy's sqrt of that (exact) variance elsewhere.  The lists must equal expected_topn of
the rows the library returned, with those rows' values beside the items."""
import numpy as np
import pytest

from conftest import gpu_available
from sample_files import (FAMILY_RISKS, check_row, expected_topn, key_families, key_image, moments, open_with,
                          rated_kinds, same_bits, write_samples)
from sbmf import device_usage
from sbmf._lib import lib

pytestmark = pytest.mark.gpu

SEED = 20
# J = 1 and one tile's edges; the mask word's; one slot per thread; the cached / uncached switch of
# k_watch_select (32 slots per thread); an uncached row with the third byte of ~item in play
SIZES = (1, 15, 16, 17, 31, 32, 33, 1023, 1024, 1025, 32767, 32768, 32769, 70001)
TOPNS = (1, 2, 1023, 1024)
ROUTE_SIZES = (1025, 32768)  # also through k_watch_accum (sbmf_test_samples_tune bit 0)
COUNTS = ("dev_bytes", "dev_allocs", "pinned_bytes", "pinned_allocs", "streams", "events", "contexts", "comms")
FAMILIES = {J: key_families(J, SEED) for J in SIZES}
CASES = [(J, name) for J in SIZES for name in FAMILIES[J]]


class Stores:
    """One prepared learner per J, kept while the cases of that J run (they are consecutive)."""

    def __init__(self):
        self.J = self.L = self.kinds = None

    def close(self):
        if self.L is not None:
            self.L.close()
        self.J = self.L = None

    def load(self, J, path):
        if self.J != J:
            self.close()
            self.kinds = rated_kinds(J, SEED)
            u, i = [], []
            for k, (_, r) in enumerate(self.kinds):
                for user in (2 * k, 2 * k + 1):
                    u.append(np.full(len(r), user, np.uint32))
                    i.append(r.astype(np.uint32))
            u, i = np.concatenate(u), np.concatenate(i)
            self.L = open_with(path, (u, i, np.full(len(u), 3.0)), 2 * len(self.kinds), J)
            self.J = J
        else:
            self.L.load_samples(path)
        return self.L

    def rated(self, w):
        return self.kinds[w // 2][1]


@pytest.fixture(scope="module")
def stores():
    assert gpu_available(), "these tests need a gfx950 device"
    base = {k: device_usage()[k] for k in COUNTS}
    st = Stores()
    yield st
    st.close()
    assert {k: device_usage()[k] for k in COUNTS} == base  # everything is back after close()


def load_family(stores, tmp_path, J, name):
    """The family's file into J's learner; (L, users, want) with want[sign] = (mean, variance, sd) restated"""
    sc = FAMILIES[J][name]
    S = len(sc)
    I = 2 * len(rated_kinds(J, SEED))
    sign = np.where(np.arange(I) % 2 == 0, 1.0, -1.0)
    path = tmp_path / "family.samples"
    write_samples(path, np.tile(sign[None, :, None], (S, 1, 1)), sc[:, :, None], "f64")
    L = stores.load(J, path)
    assert L.samples_info()["count"] == S
    return L, np.arange(I, dtype=np.uint32), {1.0: moments(sc), -1.0: moments(-1.0 * sc)}


def check_rows(L, users, want, what):
    """every user's full row against the restatement; returns the rows and whether stdev was bit-equal"""
    rows, sd_same = [], True
    for w in users:
        mean, sd = L.samples_scores(int(w))
        sd_same = check_row(mean, sd, want[1.0 if w % 2 == 0 else -1.0], "%s user %d" % (what, w)) and sd_same
        rows.append((mean, sd))
    return rows, sd_same


def describe(w, place, want, got, rows, risk):
    def one(j):
        if j < 0:
            return "none"
        key = rows[w][0][j] - risk * rows[w][1][j]
        return "item %d (key %r, image %016x, ~item %08x)" % (j, float(key), int(key_image(np.array([key]))[0]), ~int(j) & 0xffffffff)
    return "user %d place %d: expected %s, got %s" % (w, place, one(int(want)), one(int(got)))


def check_lists(stores, L, users, rows, risks, what, topns=TOPNS):
    """every list against expected_topn of the returned rows; returns every call's result"""
    out = []
    for risk in risks:
        for exclude in (True, False):
            cache = {}
            for topn in topns:
                items, mean, sd = L.samples_recommend(users, topn=topn, exclude_rated=exclude, risk=risk)
                out.append((items, mean, sd))
                assert items.shape == mean.shape == sd.shape == (len(users), topn) and items.dtype == np.int64
                for w in users:
                    ck = int(w) if exclude else int(w) % 2
                    if ck not in cache:
                        cache[ck] = expected_topn(rows[w][0], rows[w][1], stores.rated(w), 1024, risk, exclude)
                    want = cache[ck][:topn]
                    if not np.array_equal(items[w], want):
                        p = int(np.argmax(items[w] != want))
                        pytest.fail("%s risk %g exclude %s topn %d: %s" % (what, risk, exclude, topn,
                                                                           describe(w, p, want[p], items[w][p], rows, risk)))
                    real = want >= 0
                    same_bits(mean[w][real], rows[w][0][want[real]], "%s user %d list mean" % (what, w))
                    same_bits(sd[w][real], rows[w][1][want[real]], "%s user %d list stdev" % (what, w))
                    assert np.all(np.isnan(mean[w][~real])) and np.all(np.isnan(sd[w][~real]))
                    left = stores.J - len(stores.rated(w)) if exclude else stores.J
                    assert int(real.sum()) == min(topn, left), (what, w, topn, exclude)
                    if exclude:
                        assert not np.isin(items[w][real], stores.rated(w)).any(), (what, w)
                        if left == 0:
                            assert np.all(items[w] == -1)  # a user who rated everything
    return out


@pytest.mark.parametrize("J,name", CASES, ids=["%d-%s" % c for c in CASES])
def test_selection_on_hand_made_rows(stores, tmp_path, J, name):
    L, users, want = load_family(stores, tmp_path, J, name)
    what = "J=%d %s" % (J, name)
    rows, sd_same = check_rows(L, users, want, what)
    print("%s: %d users, %d samples; stdev bit-equal to numpy's sqrt on every slot: %s" % (what, len(users), len(FAMILIES[J][name]), sd_same))
    risks = FAMILY_RISKS.get(name, (0.0,))
    first = check_lists(stores, L, users, rows, risks, what)
    # a second identical call is bit-identical (rows and the widest lists)
    again = L.samples_recommend(users, topn=1024, exclude_rated=False, risk=risks[-1])
    for a, b in zip(first[-1], again):
        assert np.array_equal(a, b, equal_nan=True)
    for w in (0, 1):
        for a, b in zip(rows[w], L.samples_scores(w)):
            same_bits(b, a, "%s user %d, second call" % (what, w))


ROUTE_CASES = [(J, name) for J in ROUTE_SIZES for name in FAMILIES[J]]


@pytest.mark.parametrize("J,name", ROUTE_CASES, ids=["%d-%s" % c for c in ROUTE_CASES])
def test_watch_list_route_is_identical(stores, tmp_path, J, name):
    """the same samples through k_watch_accum, one launch per sample: the same rows, the same lists"""
    L, users, want = load_family(stores, tmp_path, J, name)
    what = "J=%d %s" % (J, name)
    risks = FAMILY_RISKS.get(name, (0.0,))
    rows, _ = check_rows(L, users, want, what + " fused")
    fused = check_lists(stores, L, users, rows, risks, what + " fused", topns=(2, 1024))
    assert lib.sbmf_test_samples_tune(L.ctx, 0, 1) == 0
    try:
        rows2, _ = check_rows(L, users, want, what + " per-sample")
        loop = check_lists(stores, L, users, rows2, risks, what + " per-sample", topns=(2, 1024))
    finally:
        assert lib.sbmf_test_samples_tune(L.ctx, 0, 0) == 0
    for w in users:
        same_bits(rows2[w][0], rows[w][0], "%s user %d mean, the two routes" % (what, w))
        same_bits(rows2[w][1], rows[w][1], "%s user %d stdev, the two routes" % (what, w))
    for a, b in zip(fused, loop):
        for x, y in zip(a, b):
            assert np.array_equal(x, y, equal_nan=True)
