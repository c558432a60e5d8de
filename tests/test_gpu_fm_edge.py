"""The two-attribute libFM learner (csrc/fmm.hip, fmm.cpp) on the row-form edge set of
tests/fm_edge.py: user and item rows of 0 .. 4097 cases, so that every instantiation of k_fmm_pass
runs its cached cases and both of its tail loops, the chunk path runs at its default bound (4097 =
2048 + 2049) and at 5 .. 65 chunks, and several ranks run the scatter form with a long row --
against the oracle (oracle/fmm_oracle.c, held to compiled libFM on this set by
tests/test_oracle_libfm.py) under tests/test_gpu_libfm.py's bars, which
tests/test_fm_edge_checker.py shows to be 1,000 times finer than one lost case.  The table of
forms per length and variant is in tests/fm_edge.py.

a. one rank against the oracle, {MCMC reference stream, ALS} x five bin / chunk variants
b. the table against timing().n_launch ("fm edge table stale")
c. the Philox stream: the variants against the default bounds, and a rerun bit for bit
d. the general learner (SBMF_FMM_GENERAL=1, csrc/fmg.hip) on the same triples
e. 2 and 3 ranks on one GPU against the oracle
The pins of these chains are in tests/test_gpu_fm_pins.py (two/edge/*)."""
import gzip
import os

import numpy as np
import pytest

import fm_edge
from conftest import GOLD, gpu_available
from edge_rows import degrees
from fm_edge import ATOL_BIAS, ATOL_FACTOR, ATOL_PRED, ITERS, K, REGULAR, RTOL_RMSE, SEED, VARIANTS
from sbmf import Data, FMLearnSBPMF, partition_rows
from test_gpu_libfm import _within_printed
from test_gpu_multirank import _run_ranks
from test_oracle_libfm import golden_name

pytestmark = pytest.mark.gpu

METHODS = ["mcmc", "als"]
_RUNS = {}  # (method, variant, rng, general) -> the arrays of that run, shared by the tests below


def _run(monkeypatch, method, variant, rng="ref", general=False, fresh=False):
    key = (method, variant, rng, general)
    if key in _RUNS and not fresh:
        return _RUNS[key]
    assert gpu_available()
    env = dict(VARIANTS[variant]) if variant in VARIANTS else {"SBMF_FMM_LONG": "8192", "SBMF_FMM_CHUNK": "0"}
    for k in ("SBMF_FMM_LONG", "SBMF_FMM_CHUNK", "SBMF_FMM_GENERAL"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    if general:
        monkeypatch.setenv("SBMF_FMM_GENERAL", "1")
    train, test, dims = fm_edge.generate()
    L = FMLearnSBPMF(num_factor=K, seed=SEED, rng=rng, method=method, order="libfm", k0=1, k1=1,
                     regular=REGULAR[method], init_stdev=fm_edge.INIT_STDEV)
    L.set_data(Data(*train), Data(*test), num_users=dims[0], num_items=dims[1])
    L.learn(sweeps=ITERS)
    U, V = L.factors()
    bu, bv, b0 = L.biases()
    out = {"rmse_train": np.array([h["rmse_train"] for h in L.history]),
           "rmse": np.array([h["rmse_avg"] for h in L.history]), "U": U, "V": V, "bu": bu, "bv": bv,
           "b0": np.array([b0]), "pred": L.predict(), "n_launch": int(L.timing().n_launch)}
    L.close()
    assert U.shape == (dims[0], K) and V.shape == (dims[1], K)
    _RUNS.setdefault(key, out)
    return out


def _oracle(method):
    o = fm_edge.oracle_run(method)
    U, V, bu, bv = fm_edge.oracle_tables(o)
    return {"rmse_train": o["rmse_train"], "rmse": o["rmse_test"], "U": U, "V": V, "bu": bu, "bv": bv,
            "b0": np.array([o["w0"]]), "pred": o["pred"]}


def _hold(label, got, want):
    """got against want under the bars; the observed maxima are printed beside each bar, and on a
    failure the factor errors per row class."""
    for k in ("U", "V", "bu", "bv", "pred", "rmse", "rmse_train"):
        assert np.isfinite(got[k]).all(), (label, k, "not finite")
    eu, ev = np.abs(got["U"] - want["U"]).max(axis=1), np.abs(got["V"] - want["V"]).max(axis=1)
    rel = lambda k: (np.abs(got[k] - want[k]) / np.abs(want[k])).max()  # noqa: E731
    obs = [("train RMSE rel", rel("rmse_train"), RTOL_RMSE), ("test RMSE rel", rel("rmse"), RTOL_RMSE),
           ("U", eu.max(), ATOL_FACTOR), ("V", ev.max(), ATOL_FACTOR),
           ("predict", np.abs(got["pred"] - want["pred"]).max(), ATOL_PRED),
           ("bu", np.abs(got["bu"] - want["bu"]).max(), ATOL_BIAS),
           ("bv", np.abs(got["bv"] - want["bv"]).max(), ATOL_BIAS),
           ("w0", np.abs(got["b0"] - want["b0"]).max(), ATOL_BIAS)]
    print("%s: %s" % (label, ", ".join("%s %.2e (bar %g)" % o for o in obs)))
    bad = [o for o in obs if not o[1] <= o[2]]
    fm_edge.by_length("users", eu)  # shown with a failure: it names the row class
    fm_edge.by_length("items", ev)
    assert not bad, (label, bad)
    return dict((o[0], o[1]) for o in obs)


def _hold_empty_rows(label, method, got, want):
    """The users and items without a case: drawn from the prior alone (MCMC: the oracle's prior
    draw of that attribute; ALS: the 1 / (lambda + 0) path, the value the oracle holds)."""
    what = "the oracle's prior draw" if method == "mcmc" else "the oracle's value"
    for side, key in (("users", "U"), ("items", "V")):
        empty = np.flatnonzero(degrees(fm_edge.SET_SEED, side) == 0)
        assert set(fm_edge.rows_of(side)[0]) <= set(empty.tolist())
        d = np.abs(got[key][empty] - want[key][empty]).max(axis=1)
        assert (d <= ATOL_FACTOR).all(), "%s: empty %s %s are not %s: max|d| %s" % (
            label, side, empty[d > ATOL_FACTOR].tolist(), what, d[d > ATOL_FACTOR].tolist())


def _hold_printed(label, method, got):
    """libFM's own lines and -out file for this chain (6 significant digits)."""
    name = golden_name(method, "edge", "1,1,%d" % K, SEED, ITERS)
    with open(os.path.join(GOLD, name + ".txt")) as f:
        lines = f.read().splitlines()
    assert _within_printed(got["rmse_train"], [float(l.split("Train=")[1].split()[0]) for l in lines]), label
    assert _within_printed(got["rmse"], [float(l.split("Test=")[1]) for l in lines]), label
    with gzip.open(os.path.join(GOLD, name + "_pred.txt.gz"), "rt") as f:
        assert _within_printed(got["pred"], np.array([float(x) for x in f.read().split()])), label


# ---- a. one rank against the oracle
@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("method", METHODS)
def test_one_rank_matches_oracle(method, variant, monkeypatch):
    label = "two/%s/%s" % (method, variant)
    longb, chunk = fm_edge.bounds(VARIANTS[variant])
    forms = fm_edge.expected_forms(longb, chunk)
    print("%s: lengths in chunks or with tail cases, length: (bin, NT, chunks, tail cases) %s"
          % (label, {n: f for n, f in forms.items() if f[2] or f[3]}))
    got, want = _run(monkeypatch, method, variant), _oracle(method)
    _hold(label, got, want)
    _hold_empty_rows(label, method, got, want)
    _hold_printed(label, method, got)


# ---- b. the table is honest
def test_launch_counts_follow_the_table(monkeypatch):
    """timing().n_launch is the launches of the last iteration (FMChain::run sets it to 0 at the
    start of each, fmc.cpp:257).  run_bins (fmm.cpp:109-138) counts 3 launches per pass and side
    for a chunked bin, 1 for another non-empty bin, none for an empty one, and an iteration runs
    1 + K passes.  Both sides of the set have rows above 4096 and none above 8192, so per
    iteration: default - chunk0 = 2 sides * (3 - 1) * (1 + K) = 36 (108 over the 3 iterations),
    chunk0 - (long8192 with chunk0) = 2 sides * 1 * (1 + K) = 18 (54 over the 3).  The numbers
    are from the code, and fm_edge.expected_pass_launches() must give the same from the table."""
    n = {v: _run(monkeypatch, "mcmc", v)["n_launch"] for v in ("default", "chunk0", "long8192-chunk0", "long8192",
                                                                 "long256-chunk64", "long256-chunk0")}
    table = {"default": fm_edge.expected_pass_launches(), "chunk0": fm_edge.expected_pass_launches(4096, 0),
             "long8192-chunk0": fm_edge.expected_pass_launches(8192, 0),
             "long8192": fm_edge.expected_pass_launches(8192),
             "long256-chunk64": fm_edge.expected_pass_launches(256, 64),
             "long256-chunk0": fm_edge.expected_pass_launches(256, 0)}
    print("n_launch per iteration", n, "launches per pass by the table", table)
    assert (table["default"], table["chunk0"], table["long8192-chunk0"]) == (10, 6, 4)
    stale = "fm edge table stale: n_launch %s, launches per pass by tests/fm_edge.py %s" % (n, table)
    assert n["default"] - n["chunk0"] == 2 * 2 * (1 + K) == 36, stale
    assert n["chunk0"] - n["long8192-chunk0"] == 2 * 1 * (1 + K) == 18, stale
    for v in n:  # every variant: its difference from the default is the table's
        assert n[v] - n["default"] == (1 + K) * (table[v] - table["default"]), stale


# ---- c. the Philox stream
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_philox_variants_agree_with_default(variant, monkeypatch):
    """oracle/fmm_oracle.c has no Philox stream, so this is weaker than (a): no independent
    reference.  A variant draws the same per-attribute normals as the default bounds by
    construction, so the two chains differ by the order of the sums only and must agree under
    (a)'s bars; the default bounds run again must give the same bits."""
    base = _run(monkeypatch, "mcmc", "default", rng="philox")
    got = _run(monkeypatch, "mcmc", variant, rng="philox", fresh=variant == "default")
    if variant == "default":
        assert got is not base
        for k in base:
            assert np.array_equal(got[k], base[k]), k
        return
    _hold("two/mcmc-philox/%s against default" % variant, got, base)
    _hold_empty_rows(variant, "mcmc", got, base)
    ref = _oracle("mcmc")  # another stream: the same data, so a chain that learns ends near it
    assert abs(got["rmse_train"][-1] - ref["rmse_train"][-1]) < 0.05


# ---- d. the general learner on the same triples
@pytest.mark.parametrize("variant", ["default", "chunk0"])
@pytest.mark.parametrize("method", METHODS)
def test_general_learner_matches_oracle(method, variant, monkeypatch):
    """SBMF_FMM_GENERAL=1: csrc/fmg.hip's NT = 256 form with up to 3,072 tail cases, and (chunk0)
    its NT = 1024 form with one."""
    label = "general/%s/%s" % (method, variant)
    got, want = _run(monkeypatch, method, variant, general=True), _oracle(method)
    _hold(label, got, want)
    _hold_empty_rows(label, method, got, want)
    _hold_printed(label, method, got)


# ---- e. several ranks
@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("nranks", [2, 3])
def test_ranks_match_oracle(nranks, method, tmp_path):
    train, _, dims = fm_edge.generate()
    # by construction: a user row lies whole inside one rank's range, the scatter form on
    # NT = 1024 with a tail case; a 1-case item is an empty row on the other R - 1 ranks
    udeg, ideg = degrees(fm_edge.SET_SEED, "users"), degrees(fm_edge.SET_SEED, "items")
    ub = np.asarray(partition_rows(np.concatenate([[0], np.cumsum(udeg)]).astype(np.uint64), nranks), np.int64)
    assert ub[0] == 0 and ub[-1] == dims[0] and (np.diff(ub) > 0).all(), ub
    case_rank = np.searchsorted(ub[1:-1], train[0].astype(np.int64), side="right")
    share = np.stack([np.bincount(train[1][case_rank == r], minlength=dims[1]) for r in range(nranks)])  # [rank, item]
    for u in fm_edge.rows_of("users")[4097]:
        owners = [r for r in range(nranks) if ub[r] <= u < ub[r + 1]]
        assert len(owners) == 1 and (case_rank[train[0] == u] == owners[0]).all() and udeg[u] == 4097
    for i in fm_edge.rows_of("items")[1]:
        assert ideg[i] == 1 and (share[:, i] == 0).sum() == nranks - 1
    bins = np.digitize(share, [257, 4097])  # an item row's bin on each rank
    print("%d ranks: user ranges %s, %d item rows sit in different bins on different ranks, shares of the 4097-case "
          "items %s" % (nranks, ub.tolist(), int((bins.max(axis=0) != bins.min(axis=0)).sum()),
                        [share[:, i].tolist() for i in fm_edge.rows_of("items")[4097]]))
    outs = _run_ranks(tmp_path, nranks, [str(K), str(ITERS), str(SEED), "ref", "0",
                                         "1,1;" + ",".join("%g" % x for x in REGULAR[method]),
                                         "als" if method == "als" else "libfm"], env={"SBMF_WORKER_DATA": "edge"})
    z0 = dict(np.load(outs[0]))
    for r in range(1, nranks):
        z = np.load(outs[r])
        for k in ("U", "V", "bu", "bv", "b0", "rmse", "rmse_train", "pred"):
            assert np.array_equal(z[k], z0[k]), (r, k)
    label = "two/%s/%d ranks" % (method, nranks)
    want = _oracle(method)
    _hold(label, z0, want)
    _hold_empty_rows(label, method, z0, want)
    _hold_printed(label, method, z0)
