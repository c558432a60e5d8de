"""The query list of libFM's MCMC / ALS learner on the GPU (sbmf_fm_query_cases, include/sbmf.h):
posterior scores of query cases against every block row of one relation.

Yardsticks: (1) numpy in long double on the model the library returns after every iteration --
fm_rel._rel_predict on the expanded (query, block row) cases, its running mean and second moment;
(2) the learner's own test frame: a twin context whose test set is those expanded cases.  The bound
is derived in tests/fm_query.py: 4 (K + entries + 4) eps A on the mean, 2 max|score| times that on
the second moment (stdev^2 + mean^2).  Every comparison prints the largest error beside its bound.

Observed on an MI355X, largest error as a fraction of its bound: numpy per iteration 0.0093 (mean;
nq = 130, K = 8) and 0.0021 (second moment; nq = 1, K = 8; 0.0019 at nq = 130), at K = 250 at most
0.00044 / 0.00018; a list registered midway 0.0089 / 0.0075 (the second moment of one iteration
alone); the twin's predict 0.012 (regression), 0.0071 (task c), 0.010 (groups); ALS 0.014; rel_edge
0.0021 / 0.0013."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import fm_class
import fm_query
import fm_rel
from conftest import gpu_available
from fm_query import EPS, Expanded, query_cases, rel2_queries
from sbmf import Cases, Communicator, Data, FMLearnSBPMF, SBMFError, _lib, device_usage
from sbmf._lib import CLI_PATH, SBMF_E_ARG, SBMF_E_NOMEM, SBMF_E_STATE

pytestmark = pytest.mark.gpu

COUNTS = ("dev_bytes", "dev_allocs", "pinned_bytes", "pinned_allocs", "streams", "events", "contexts", "comms")
MODES = {"als": ("als", "ref"), "ref": ("mcmc", "ref"), "philox": ("mcmc", "philox")}


def _open(S, mode, K=8, task="r", seed=1):
    """a learner on the block form of S, prepared, no iteration run"""
    method, rng = MODES[mode]
    L = FMLearnSBPMF(num_factor=K, seed=seed, rng=rng, method="als" if method == "als" else "mcmc", order="libfm",
                     k0=1, k1=1, regular=fm_rel.als_regular(S.num_groups) if method == "als" else (0.0, 0.0, 0.0),
                     init_stdev=0.1, task=task)
    if S.main_group is not None:
        L.set_groups(S.main_group)
    for R in S.relations:
        L.add_relation(R)
    L.set_data(S.train, S.test)
    return L


def _code(fn, *a, **k):
    with pytest.raises(SBMFError) as ei:
        fn(*a, **k)
    return ei.value.code, str(ei.value)


class Tally:
    """the yardstick's running sums over the iterations a callback sees"""

    def __init__(self, L, ex, task="r", clamp=None, skip=0):
        self.L, self.ex, self.task, self.clamp, self.skip = L, ex, task, clamp, skip
        self.n, self.s1, self.s2, self.bound, self.smax = 0, 0, 0, 0.0, 0.0

    def __call__(self, rec):
        if self.skip:
            self.skip -= 1
            return
        m = self.L.fm()
        s = self.ex.scores(m, self.task, self.clamp)
        self.s1, self.s2, self.n = self.s1 + s, self.s2 + s * s, self.n + 1
        self.bound = np.maximum(self.bound, self.ex.bound(m))
        self.smax = max(self.smax, float(np.abs(s).max()))

    def check(self, what=""):
        """the list's rows against the sums; returns (largest mean error / bound, same of the second moment)"""
        worst = [0.0, 0.0]
        for q in range(self.ex.nq):
            mean, sd = self.L.fm_query_scores(q)
            rm = (self.s1[q] / self.n).astype(np.float64)
            r2 = (self.s2[q] / self.n).astype(np.float64)
            e1 = np.abs(mean - rm).max() / self.bound[q]
            e2 = np.abs(sd * sd + mean * mean - r2).max() / (2.0 * self.smax * self.bound[q])
            worst = [max(worst[0], e1), max(worst[1], e2)]
        print("%s mean error / bound %.3g  second moment error / bound %.3g  (bound %.3g, max|score| %.3g)"
              % (what, worst[0], worst[1], float(np.max(self.bound)), self.smax))
        assert worst[0] <= 1.0 and worst[1] <= 1.0, worst
        return worst


# ---- 1. against numpy, per iteration
@pytest.mark.parametrize("nq,K", [(1, 8), (1, 250), (17, 8), (17, 20), (17, 100), (17, 120), (17, 250), (130, 8),
                                  (130, 20), (130, 120)])
def test_scores_match_numpy_per_iteration(nq, K, ml100k):
    assert gpu_available()
    S = fm_rel.rel2(ml100k)
    main, urow = rel2_queries(S, nq)
    ex = Expanded(S, 1, main, [urow, None])
    L = _open(S, "philox", K)
    L.fm_queries(1, query_cases(S, main), rows=[urow, None])
    t = Tally(L, ex)
    L.learn(sweeps=5, callback=t)
    assert t.n == 5
    t.check("nq=%d K=%d" % (nq, K))
    L.close()


# ---- 2. against the learner's own test frame
@pytest.mark.parametrize("name,mode,task", [("rel2", "ref", "r"), ("rel2", "philox", "c"), ("rel2g", "philox", "r")])
def test_clamped_mean_equals_the_twins_predict(name, mode, task, ml100k):
    assert gpu_available()
    S = fm_rel.rel2_grouped(ml100k) if name == "rel2g" else fm_rel.rel2(ml100k, binary=task == "c")
    main, urow = rel2_queries(S, 3, ids=S.p_main - 1)
    ex = Expanded(S, 1, main, [urow, None])
    T = _open(fm_query.twin_set(S, ex), mode, task=task)
    T.learn(sweeps=5)
    twin = T.predict().reshape(ex.nq, ex.nb)
    L = _open(S, mode, task=task)
    assert L.fm_relation_info()[0]["attr_offset"] == T.fm_relation_info()[0]["attr_offset"] == S.p_main
    L.fm_queries(1, query_cases(S, main), rows=[urow, None], clamp=True)
    bound = [0.0]
    L.learn(sweeps=5, callback=lambda rec: bound.__setitem__(0, np.maximum(bound[0], ex.bound(L.fm()))))
    key = "acc_train" if task == "c" else "rmse_train"
    assert [h[key] for h in L.history] == [h[key] for h in T.history]  # one chain: the test set is not part of it
    worst = 0.0
    for q in range(ex.nq):
        mean, _ = L.fm_query_scores(q)
        worst = max(worst, np.abs(mean - twin[q]).max() / bound[0][q])
    print("%s %s task %s: |mean - twin predict| / bound %.3g (bound %.3g)" % (name, mode, task, worst, np.max(bound[0])))
    assert worst <= 1.0
    L.close()
    T.close()


# ---- 3. ALS: the latest iteration's model, no spread
def test_als_holds_the_latest_iteration(ml100k):
    assert gpu_available()
    S = fm_rel.rel2(ml100k)
    main, urow = rel2_queries(S, 17)
    ex = Expanded(S, 1, main, [urow, None])
    L = _open(S, "als")
    L.fm_queries(1, query_cases(S, main), rows=[urow, None])
    # The count is not read back directly: a count other than 1 shows as a mean that is the latest
    # score divided by it (or an average over iterations), far outside the bound.  The third round
    # registers the list anew midway (after iteration 3) and reads iteration 4 alone.
    for sweeps in (1, 2, 1):  # after iterations 1, 3 and 4
        if len(L.history) == 3:
            L.fm_queries(1, query_cases(S, main), rows=[urow, None])
            assert _code(L.fm_query_scores, 0)[0] == SBMF_E_STATE
        L.learn(sweeps=sweeps)
        m = L.fm()
        ref, bound = ex.scores(m).astype(np.float64), ex.bound(m)
        worst = 0.0
        for q in range(ex.nq):
            mean, sd = L.fm_query_scores(q)
            assert np.all(sd == 0.0) and not np.any(np.signbit(sd))  # exactly 0.0
            worst = max(worst, np.abs(mean - ref[q]).max() / bound[q])
        print("ALS after %d iterations: error / bound %.3g" % (len(L.history), worst))
        assert worst <= 1.0  # the count is 1: the mean is this iteration's score, not an average
        rows, mean, sd = L.fm_query_recommend(topn=5, risk=1.0)
        assert np.all(sd == 0.0)
        for q in range(ex.nq):
            assert np.array_equal(rows[q], _expect(L.fm_query_scores(q)[0], np.zeros(ex.nb), 1.0, 5))
    L.close()


# ---- 4. rel_edge: one relation, queries with main features only
def _edge_queries(S, nq=5):
    return [[] if q == 0 else [((3 * q) % (S.p_main - 1), 1.0 if q % 2 else 0.5)] for q in range(nq)]


@pytest.mark.parametrize("env", [{}, {"SBMF_FMM_LONG": "256", "SBMF_FMM_CHUNK": "64"}])
def test_rel_edge_candidates(env, monkeypatch):
    assert gpu_available()
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    S = fm_rel.rel_edge()
    main = _edge_queries(S)
    ex = Expanded(S, 0, main, [None])
    L = _open(S, "philox")
    L.fm_queries(0, query_cases(S, main))
    t = Tally(L, ex)
    L.learn(sweeps=5, callback=t)
    t.check("rel_edge %s" % env)
    cnt = np.bincount(S.relations[0].train_row, minlength=ex.nb)
    assert ex.nb == 1401 and cnt[0] == 0 and cnt[1400] == 0 and cnt[8] == 1025  # unjoined rows, the 1,025-case row
    for q in range(ex.nq):  # the feature-less block rows score w0 + a_q: the same bits for both
        mean, sd = L.fm_query_scores(q)
        assert mean[1349] == mean[1399] and sd[1349] == sd[1399]
        assert abs(mean[1349] - float(t.s1[q][1349] / t.n)) <= t.bound[q]
    L.close()


# ---- 5. the selection
def _expect(mean, sd, risk, topn, excluded=()):
    key = mean - risk * sd
    order = np.lexsort((np.arange(len(key)), -key))
    order = order[~np.isin(order, np.asarray(excluded, np.int64))][:topn]
    rows = np.full(topn, -1, np.int64)
    rows[:len(order)] = order
    return rows


def test_selection_is_exact():
    assert gpu_available()
    S = fm_rel.rel_edge()
    main = _edge_queries(S, 6)
    nb = 1401
    excl = [[], list(range(nb)), list(range(0, nb, 2)), [1349], [7, 7, 1400], list(range(500))]
    L = _open(S, "philox")
    L.fm_queries(0, query_cases(S, main), exclude=excl, clamp=True)
    L.learn(sweeps=4)
    sc = [L.fm_query_scores(q) for q in range(6)]
    ties = sum(len(m) - len(np.unique(m)) for m, _ in sc)
    print("tied means under clamp:", ties)
    assert ties > 0  # at least the feature-less rows 1349 and 1399
    for topn in (1, 10, 1024):
        for risk in (0.0, 1.0):
            for keep in (False, True):
                rows, mean, sd = L.fm_query_recommend(topn=topn, risk=risk, keep_excluded=keep)
                for q in range(6):
                    want = _expect(sc[q][0], sc[q][1], risk, topn, () if keep else excl[q])
                    assert np.array_equal(rows[q], want), (topn, risk, keep, q)
                    ok = want >= 0
                    assert np.array_equal(mean[q][ok], sc[q][0][want[ok]]) and np.array_equal(sd[q][ok], sc[q][1][want[ok]])
                    assert np.all(np.isnan(mean[q][~ok])) and np.all(np.isnan(sd[q][~ok]))
    rows, _, _ = L.fm_query_recommend(topn=1024)
    assert np.all(rows[1] == -1) and (rows[5] >= 0).sum() == nb - 500 and (rows[0] >= 0).all()
    # the same list without an exclusion CSR, and with an empty one
    for ex_arg in (None, [[] for _ in range(6)]):
        L.fm_queries(0, query_cases(S, main), exclude=ex_arg, clamp=True)
        L.learn(sweeps=1)
        rows, _, _ = L.fm_query_recommend(topn=10)
        for q in range(6):
            m, s = L.fm_query_scores(q)
            assert np.array_equal(rows[q], _expect(m, s, 0.0, 10))
    L.close()


# ---- 6. the chain does not see the list; reruns; registration
def _state(L):
    w0, w, v = L.fm()
    keys = ("rmse_train", "rmse_avg", "rmse_this", "tau")
    return w0, w.tobytes(), v.tobytes(), [[h[k] for k in keys] for h in L.history], L.predict().tobytes()


@pytest.mark.parametrize("mode", ["ref", "philox"])
def test_chain_untouched_and_rerun_identical(mode, ml100k):
    assert gpu_available()
    S = fm_rel.rel2(ml100k)
    main, urow = rel2_queries(S, 17)
    runs = []
    for with_list in (False, True, True):
        L = _open(S, mode)
        if with_list:
            L.fm_queries(1, query_cases(S, main), rows=[urow, None])
        L.learn(sweeps=5)
        tables = [np.concatenate(L.fm_query_scores(q)).tobytes() for q in range(17)] if with_list else None
        runs.append((_state(L), tables, L.fm_query_recommend(topn=7, risk=0.5) if with_list else None))
        L.close()
    assert runs[0][0] == runs[1][0] == runs[2][0]  # w0, w, v, the #Iter quantities, the predictions: the same bits
    assert runs[1][1] == runs[2][1]
    for a, b in zip(runs[1][2], runs[2][2]):
        assert np.array_equal(a, b, equal_nan=True)


def test_registered_midway_and_again(ml100k):
    assert gpu_available()
    S = fm_rel.rel2(ml100k)
    main, urow = rel2_queries(S, 3)
    ex = Expanded(S, 1, main, [urow, None])
    L = _open(S, "philox")
    L.learn(sweeps=2)
    L.fm_queries(1, query_cases(S, main), rows=[urow, None])
    assert _code(L.fm_query_scores, 0)[0] == SBMF_E_STATE
    t = Tally(L, ex)
    L.learn(sweeps=3, callback=t)
    assert t.n == 3 and len(L.history) == 5
    t.check("iterations 3..5")
    # registering again replaces and zeroes the list
    L.fm_queries(1, query_cases(S, main[:2]), rows=[urow[:2], None])
    assert _code(L.fm_query_scores, 0)[0] == SBMF_E_STATE
    ex2 = Expanded(S, 1, main[:2], [urow[:2], None])
    t2 = Tally(L, ex2)
    L.learn(sweeps=1, callback=t2)
    t2.check("iteration 6 alone")
    assert _code(L.fm_query_scores, 2)[0] == SBMF_E_ARG
    L.close()


def test_nothing_leaks():
    assert gpu_available()
    S = fm_rel.one_to_one()
    main = [[(q % 5, 1.0)] for q in range(4)]
    base = {k: device_usage()[k] for k in COUNTS}
    L = _open(S, "philox", K=4)
    held = {k: device_usage()[k] for k in COUNTS}
    L.fm_queries(0, query_cases(S, main), exclude=[[1], [], [2, 3], []])
    assert device_usage()["dev_allocs"] > held["dev_allocs"]
    L.learn(sweeps=1)
    L.fm_queries(0, Cases([0], [], [], []))  # n == 0 frees the list
    assert {k: device_usage()[k] for k in COUNTS} == held
    assert _code(L.fm_query_recommend, topn=3)[0] == SBMF_E_STATE
    L.close()
    for _ in range(50):
        L = _open(S, "philox", K=4)
        L.fm_queries(0, query_cases(S, main), exclude=[[1], [], [2, 3], []])
        L.learn(sweeps=1)
        L.fm_query_recommend(topn=3)
        L.close()  # with a live list
    assert {k: device_usage()[k] for k in COUNTS} == base


# ---- 7. what is refused
def test_refusals(ml100k):
    assert gpu_available()
    tr, te = ml100k
    S = fm_rel.rel2(ml100k)
    main, urow = rel2_queries(S, 3)
    qc = query_cases(S, main)
    # another method
    for kw, word in ((dict(method="mcmc", order="sbpmf"), "SBPMF"), (dict(method="vb"), "VB")):
        M = FMLearnSBPMF(num_factor=4, seed=1, **kw)
        M.set_data(Data(*tr), Data(*te))
        code, msg = _code(M.fm_queries, 0, qc)
        assert code == SBMF_E_STATE and word in msg and "libFM" in msg, msg
        M.close()
    # no relations
    M = FMLearnSBPMF(num_factor=4, seed=1, order="libfm")
    M.set_data(S.train, S.test)
    code, msg = _code(M.fm_queries, 0, qc)
    assert code == SBMF_E_STATE and "no relations" in msg, msg
    M.close()
    # before prepare
    M = FMLearnSBPMF(num_factor=4, seed=1, order="libfm")
    M.init()
    code, msg = _code(M.fm_queries, 0, qc)
    assert code == SBMF_E_STATE and "not prepared" in msg, msg
    M.close()
    # a communicator, a virtual rank
    comm = Communicator(1, 0, bytes(128))
    M = FMLearnSBPMF(num_factor=4, seed=1, order="libfm")
    M.init(comm=comm)
    code, msg = _code(M.fm_queries, 0, qc)
    assert code == SBMF_E_STATE and "communicator" in msg, msg
    M.close()
    comm.close()
    M = FMLearnSBPMF(num_factor=4, seed=1)
    M.init()
    assert _lib.lib.sbmf_test_virtual_rank(M.ctx, 2, 0) == 0
    code, msg = _code(M.fm_queries, 0, qc)
    assert code == SBMF_E_STATE and "virtual rank" in msg, msg
    M.close()
    # the arguments
    L = _open(S, "philox", K=4)
    nu, ni = S.relations[0].block.num_cases, S.relations[1].block.num_cases
    assert _code(L.fm_query_recommend, topn=3)[0] == SBMF_E_STATE  # no list
    for args, kw, word in (((2, qc), dict(rows=[urow, None]), "relation 2"),
                           ((1, query_cases(S, [[(S.p_main, 1.0)]] * 3)), dict(rows=[urow, None]), "attr_offset_0"),
                           ((1, qc), dict(rows=[[0, nu, 0], None]), "block rows"),
                           ((1, qc), dict(rows=None), "rows[0] is missing"),
                           ((0, qc), dict(rows=[None, None]), "rows[1] is missing"),
                           ((1, qc), dict(rows=[urow, None], exclude=[[0], [ni], []]), "excl_rows"),
                           ((1, qc), dict(rows=[urow, None], exclude=(np.array([0, 2, 1, 2], np.uint32),
                                                                       np.array([0, 1], np.uint32))), "excl_ptr")):
        code, msg = _code(L.fm_queries, *args, **kw)
        assert code == SBMF_E_ARG and word in msg, msg
    c = qc._c()
    arr = (_lib._P_U32 * 2)(urow.ctypes.data_as(_lib._P_U32), None)
    assert _lib.lib.sbmf_fm_query_cases(L.ctx, 1, C.byref(c), arr, None, None, 2) == SBMF_E_ARG
    assert b"unknown flags" in _lib.lib.sbmf_last_error(L.ctx)
    L.fm_queries(1, qc, rows=[urow, None])
    for fn, a, k in ((L.fm_query_scores, (0,), {}), (L.fm_query_recommend, (), dict(topn=3))):
        code, msg = _code(fn, *a, **k)  # reading before any iteration
        assert code == SBMF_E_STATE and "no sweep accumulated" in msg, msg
    assert L.fm_query_timing() == {"ms_terms": 0.0, "ms_score": 0.0, "ms_select": 0.0}
    L.learn(sweeps=1)
    assert _code(L.fm_query_recommend, topn=0)[0] == SBMF_E_ARG
    assert _code(L.fm_query_recommend, topn=1025)[0] == SBMF_E_ARG
    assert _code(L.fm_query_scores, 3)[0] == SBMF_E_ARG
    L.fm_query_recommend(topn=3)
    tm = L.fm_query_timing()
    print(tm)
    assert tm["ms_terms"] > 0 and tm["ms_score"] > 0 and tm["ms_select"] > 0
    L.close()


def test_a_list_the_device_cannot_hold(ml100k):
    """SBMF_E_NOMEM: 2^25 feature-less queries against rel2's 1,683 item rows (1,696 padded) make each
    sum table 455 GB, above any one GPU's memory, so the first device allocation fails at once and
    nothing is held.  On the host the case costs the zero-filled ptr / target / row arrays the call
    reads once (0.5 GB)."""
    assert gpu_available()
    S = fm_rel.rel2(ml100k)
    L = _open(S, "philox")
    held = {k: device_usage()[k] for k in COUNTS}
    n, nbp = 1 << 25, 1696
    assert device_usage()["device_total"] < 8 * n * nbp
    qc = Cases(np.zeros(n + 1, np.uint64), [], [], np.zeros(n, np.float32))
    code, msg = _code(L.fm_queries, 1, qc, rows=[np.zeros(n, np.uint32), None])
    print(msg)
    assert code == SBMF_E_NOMEM and "%d queries against 1683 block rows" % n in msg, msg
    need = int(re.search(r"need (\d+) bytes of device memory", msg).group(1))
    assert 16 * n * nbp < need < 17 * n * nbp  # the two tables, and per query far less than a row of them
    assert {k: device_usage()[k] for k in COUNTS} == held
    assert _code(L.fm_query_recommend, topn=3)[0] == SBMF_E_STATE  # no list is left behind
    L.learn(sweeps=1)  # and the learner runs on without one
    assert len(L.history) == 1 and _code(L.fm_query_scores, 0)[0] == SBMF_E_STATE
    L.close()


# ---- 8. the command line
def test_cli_recommend_queries(ml100k, tmp_path):
    assert gpu_available()
    S = fm_rel.rel2(ml100k)
    stems = fm_rel.write_binary_set(S, tmp_path)
    main, urow = rel2_queries(S, 5)
    excl = [[], [3, 4], [], [0], []]
    d = str(tmp_path)
    with open(os.path.join(d, "queries.libfm"), "w") as f:
        f.write(fm_rel.cases_to_text(query_cases(S, main)))
    with open(os.path.join(d, stems[0] + ".queries"), "w") as f:
        f.write("".join("%d\n" % r for r in urow))
    with open(os.path.join(d, "exclude.txt"), "w") as f:
        f.write("".join("%d %d\n" % (q, r) for q, e in enumerate(excl) for r in e))
    cmd = [CLI_PATH, "-task", "r", "-format", "libfm", "-train", "train.libfm", "-test", "test.libfm", "-dim", "1,1,8",
           "-iter", "8", "-method", "mcmc", "-relation", ",".join(stems), "-recommend_queries", "top.txt",
           "-rec_queries", "queries.libfm", "-rec_relation", stems[1], "-rec_exclude", "exclude.txt", "-rec_topn", "6",
           "-rec_risk", "0.5"]
    r = subprocess.run(cmd, cwd=d, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    ref_lines, _, _ = fm_rel.golden("ref_libfm_rel_rel2_mcmc_i8")
    assert [l for l in r.stdout.splitlines() if l.startswith("#Iter=")] == [fm_class.strip_map(l) for l in ref_lines]
    L = _open(S, "ref")
    L.fm_queries(1, query_cases(S, main), rows=[urow, None], exclude=excl)
    L.learn(sweeps=8)
    rows, mean, sd = L.fm_query_recommend(topn=6, risk=0.5)
    want = ["%d\t%d\t%.17g\t%.17g" % (q, rows[q, k], mean[q, k], sd[q, k]) for q in range(5) for k in range(6)]
    assert open(os.path.join(d, "top.txt")).read().splitlines() == want
    L.close()
