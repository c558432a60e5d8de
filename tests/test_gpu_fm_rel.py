"""Block-structure relations (libFM's -relation) in the general libFM MCMC / ALS learner on the
GPU.  The yardstick here is this project's own general learner on the expanded twin of each set
(tests/fm_rel.py): the same chain with the block rows' features written out on every case and the
relations' groups in a -meta.  The block form sums per block row what the twin sums per case, so
the two agree to rounding, at the general learner's bars: RMSE rtol 1e-9, w / v atol 1e-8,
predictions atol 1e-9.  Also: reruns are bit-identical in both RNG modes, nothing leaks, a
relation joined one case per block row equals its twin, and what is not offered is refused."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import fm_class
import fm_rel
from conftest import PKG, gpu_available
from sbmf import Cases, Communicator, Data, FMLearnSBPMF, Relation, SBMFError, _lib, device_usage, load_libfm_relation
from sbmf._lib import CLI_PATH, SBMF_E_ARG, SBMF_E_STATE
from test_gpu_fm_cases import _check_against_restatement
from test_gpu_libfm import _within_printed

pytestmark = pytest.mark.gpu

K = 8
MODES = {"als": ("als", "ref"), "ref": ("mcmc", "ref"), "philox": ("mcmc", "philox")}


def _learner(method, rng, regular=(0.0, 0.0, 0.0), task="r", seed=1):
    return FMLearnSBPMF(num_factor=K, seed=seed, rng=rng, method="als" if method == "als" else "mcmc", order="libfm",
                        k0=1, k1=1, regular=regular, init_stdev=0.1, task=task)


_als_regular = fm_rel.als_regular


def _block(S, mode, iters, task="r", seed=1):
    method, rng = MODES[mode]
    L = _learner(method, rng, _als_regular(S.num_groups) if method == "als" else (0.0, 0.0, 0.0), task, seed)
    if S.main_group is not None:
        L.set_groups(S.main_group)
    for R in S.relations:
        L.add_relation(R)
    L.set_data(S.train, S.test)
    L.learn(sweeps=iters)
    return L


def _twin(S, mode, iters, task="r", seed=1):
    method, rng = MODES[mode]
    L = _learner(method, rng, _als_regular(S.num_groups) if method == "als" else (0.0, 0.0, 0.0), task, seed)
    L.set_groups(S.group)
    L.set_data(S.twin_train, S.twin_test)
    L.learn(sweeps=iters)
    return L


def _compare(A, B, S, task="r"):
    """the block form A against the twin B at the general learner's bars; every figure is printed first"""
    assert A.fm_info()["num_attr"] == B.fm_info()["num_attr"] == S.num_attribute
    (a0, aw, av), (b0, bw, bv) = A.fm(), B.fm()
    pa, pb = A.predict(), B.predict()
    key = "acc_train" if task == "c" else "rmse_train"
    ta, tb = np.array([h[key] for h in A.history]), np.array([h[key] for h in B.history])
    ea = np.array([h["acc_avg" if task == "c" else "rmse_avg"] for h in A.history])
    eb = np.array([h["acc_avg" if task == "c" else "rmse_avg"] for h in B.history])
    fa, fb = A.fm_groups(), B.fm_groups()
    print("|dw0| %.3g  max|dw| %.3g  max|dv| %.3g  max|dpred| %.3g  max rel d(train) %.3g  max rel d(test) %.3g"
          % (abs(a0 - b0), np.abs(aw - bw).max(), np.abs(av - bv).max(), np.abs(pa - pb).max(),
             np.max(np.abs(ta - tb) / np.abs(tb)), np.max(np.abs(ea - eb) / np.abs(eb))))
    assert fa["G"] == fb["G"] == S.num_groups and fa["cnt"].tolist() == fb["cnt"].tolist()
    assert abs(a0 - b0) <= 1e-8 and np.abs(aw - bw).max() <= 1e-8 and np.abs(av - bv).max() <= 1e-8
    assert np.abs(pa - pb).max() <= 1e-9
    assert np.all(np.abs(ta - tb) <= 1e-9 * np.abs(tb)) and np.all(np.abs(ea - eb) <= 1e-9 * np.abs(eb))
    for k in ("w_lambda", "w_mu", "v_lambda", "v_mu"):
        assert np.allclose(fa[k], fb[k], rtol=1e-8, atol=1e-8), k


# ---- 1. against libFM itself run with -relation (tests/make_fm_rel_golden.py)
@pytest.mark.parametrize("name", sorted(fm_rel.GOLDEN_RUNS))
def test_python_matches_libfm_with_relations(name, ml100k):
    assert gpu_available()
    dset, method, task, iters = fm_rel.GOLDEN_RUNS[name]
    S = fm_rel.golden_set(dset, ml100k)
    ref_lines, ref_pred, head = fm_rel.golden(name)
    L = _block(S, "als" if method == "als" else "ref", iters, task=task)
    ref_train = [float(l.split("Train=")[1].split()[0]) for l in ref_lines]
    ref_test = [float(l.split("Test=")[1].split()[0]) for l in ref_lines]
    kt, ke = ("acc_train", "acc_avg") if task == "c" else ("rmse_train", "rmse_avg")
    train, test = [h[kt] for h in L.history], [h[ke] for h in L.history]
    print("train", train, ref_train, "\ntest", test, ref_test)
    assert _within_printed(train, ref_train) and _within_printed(test, ref_test)
    pred = L.predict()
    print("max|dpred|", np.abs(pred - ref_pred).max())
    assert pred.shape == ref_pred.shape and _within_printed(pred, ref_pred)
    assert "#attr=%d\t#groups=%d" % (L.fm_info()["num_attr"], L.fm_groups()["G"]) in head
    for g, c in enumerate(L.fm_groups()["cnt"]):
        assert "#attr_in_group[%d]=%d" % (g, c) in head
    L.close()


@pytest.mark.parametrize("name", sorted(fm_rel.GOLDEN_RUNS))
def test_cli_matches_libfm_with_relations(name, ml100k, tmp_path):
    assert gpu_available()
    dset, method, task, iters = fm_rel.GOLDEN_RUNS[name]
    S = fm_rel.golden_set(dset, ml100k)
    stems = fm_rel.write_binary_set(S, tmp_path)
    # -format libfm: rel_edge's first case holds no feature, which the format guess reads as a triple file
    cmd = [CLI_PATH, "-task", task, "-format", "libfm", "-train", "train.libfm", "-test", "test.libfm", "-dim", "1,1,8",
           "-iter", str(iters), "-method", method, "-relation", ",".join(stems), "-out", "pred.txt", "-rlog", "rlog.txt", "-verbosity", "1"]
    if S.main_group is not None:
        cmd += ["-meta", "meta.txt"]
    if method == "als":
        cmd += ["-regular", ",".join("%g" % x for x in fm_rel.als_regular(S.num_groups))]
    r = subprocess.run(cmd, cwd=str(tmp_path), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    ref_lines, ref_pred, head = fm_rel.golden(name)
    lines = [l for l in r.stdout.splitlines() if l.startswith("#Iter=")]
    print("\n".join(lines))
    # as text; of the reference's classification lines without the always-zero MAP@5 field, which
    # this CLI leaves out (tests/fm_class.py)
    assert lines == [fm_class.strip_map(l) for l in ref_lines]
    pred = np.array([float(x) for x in open(os.path.join(str(tmp_path), "pred.txt")).read().split()])
    assert pred.shape == ref_pred.shape and _within_printed(pred, ref_pred)
    out = r.stdout.splitlines()
    for l in head:  # "#relations: n", "#attr=..\t#groups=..", "#attr_in_group[g]=.."
        if l.startswith("#"):
            assert l in out, l
    # the rlog carries every joined group's columns; their last row against the same chain through Python
    t = open(os.path.join(str(tmp_path), "rlog.txt")).read().splitlines()
    header, last = t[0].split("\t"), t[-1].split("\t")
    assert len(t) == iters + 1
    L = _block(S, "als" if method == "als" else "ref", iters, task=task)
    fg = L.fm_groups()
    for g in range(S.num_groups):
        want = {"wmu[%d]" % g: fg["w_mu"][g], "wlambda[%d]" % g: fg["w_lambda"][g]}
        for f in range(K):
            want["vmu[%d,%d]" % (g, f)] = fg["v_mu"][g, f]
            want["vlambda[%d,%d]" % (g, f)] = fg["v_lambda"][g, f]
        for name_, val in want.items():
            assert name_ in header, name_
            got = float(last[header.index(name_)])
            assert _within_printed([val], [got]), (name_, val, got)
    L.close()


@pytest.mark.parametrize("args,word", [(["-method", "mcmc", "-order", "sbpmf"], "SBPMF"), (["-method", "vb"], "-method vb")])
def test_cli_refuses_relations_for_the_other_methods(args, word, ml100k, tmp_path):
    assert gpu_available()
    S = fm_rel.one_to_one()
    stems = fm_rel.write_binary_set(S, tmp_path)
    r = subprocess.run([CLI_PATH, "-task", "r", "-train", "train.libfm", "-test", "test.libfm", "-dim", "1,1,4", "-iter", "1",
                        "-relation", ",".join(stems)] + args, cwd=str(tmp_path), capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "-relation" in r.stderr + r.stdout and word in r.stderr + r.stdout, r.stderr


def test_loaded_relation_runs_like_the_one_in_memory(ml100k, tmp_path):
    assert gpu_available()
    S = fm_rel.rel2_grouped(ml100k)
    stems = fm_rel.write_binary_set(S, tmp_path)
    T = fm_rel.RelSet.__new__(fm_rel.RelSet)
    T.__dict__.update(S.__dict__)
    T.relations = [load_libfm_relation(os.path.join(str(tmp_path), s)) for s in stems]
    A, B = _block(S, "philox", 3), _block(T, "philox", 3)
    assert np.array_equal(A.predict(), B.predict()) and np.array_equal(A.fm()[2], B.fm()[2])
    A.close()
    B.close()


# ---- 2. the block form against the general learner on the expanded twin
@pytest.mark.parametrize("mode", ["als", "ref", "philox"])
def test_rel2_equals_its_expanded_twin(mode, ml100k):
    assert gpu_available()
    S = fm_rel.rel2(ml100k)
    A, B = _block(S, mode, 5), _twin(S, mode, 5)
    info = A.fm_relation_info()
    print(info, A.fm_info())
    assert [r["attr_offset"] for r in info] == S.offsets and [r["group_offset"] for r in info] == S.group_offsets
    assert [r["num_attr"] for r in info] == [R.block.num_attr for R in S.relations]
    assert [r["block_rows"] for r in info] == [R.block.num_cases for R in S.relations]
    _compare(A, B, S)
    A.close()
    B.close()


@pytest.mark.parametrize("mode", ["als", "philox"])
def test_rel2_with_meta_and_relation_groups_equals_its_twin(mode, ml100k):
    assert gpu_available()
    S = fm_rel.rel2_grouped(ml100k)
    A, B = _block(S, mode, 5), _twin(S, mode, 5)
    _compare(A, B, S)
    A.close()
    B.close()


def test_rel2_classification_als_equals_its_twin(ml100k):
    assert gpu_available()
    S = fm_rel.rel2(ml100k, binary=True)
    A, B = _block(S, "als", 5, task="c"), _twin(S, "als", 5, task="c")
    _compare(A, B, S, task="c")
    A.close()
    B.close()


_EDGE_CHILD = """
import sys
sys.path[:0] = [%r, %r]
import fm_rel, test_gpu_fm_rel as t
S = fm_rel.rel_edge()
for mode in ("als", "ref", "philox"):
    A, B = t._block(S, mode, 5), t._twin(S, mode, 5)
    print(mode, A.fm_relation_info(), A.fm_info())
    t._compare(A, B, S)
    A.close(); B.close()
print("edge ok")
"""


@pytest.mark.parametrize("bins", ["default", "long256_chunk64"])
def test_rel_edge_equals_its_expanded_twin(bins):
    """rel_edge in both bin settings (the bounds are read from the environment at prepare: a child process)"""
    assert gpu_available()
    env = dict(os.environ)
    if bins != "default":
        env.update(SBMF_FMM_LONG="256", SBMF_FMM_CHUNK="64")
    here = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, "-c", _EDGE_CHILD % (here, PKG)], env=env, capture_output=True, text=True,
                       timeout=300)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and "edge ok" in r.stdout


# ---- 3. ALS against the serial numpy restatement (tests/fm_rel.py) in float64, and in longdouble for
# the restatement's own error, at iterations 1, 2 and 5
_RESTATED = {}


def _restated(key, S):
    if key not in _RESTATED:
        _RESTATED[key] = (fm_rel.als_restatement(S, K, 5, ft=np.float64, record=(1, 2, 5)),
                          fm_rel.als_restatement(S, K, 5, ft=np.longdouble, record=(1, 2, 5)))
    return _RESTATED[key]


@pytest.mark.parametrize("dset", ["rel2", "rel2g", "edge"])
def test_als_matches_serial_restatement(dset, ml100k):
    assert gpu_available()
    S = fm_rel.golden_set(dset, ml100k)
    a, b = _restated(dset, S)
    L = _block(S, "als", 0)
    done = 0
    for it in (1, 2, 5):
        L.learn(sweeps=it - done)
        done = it
        _check_against_restatement(L, it, a, b)
    L.close()


# ---- 4. reruns are bit-identical
@pytest.mark.parametrize("mode", ["ref", "philox"])
def test_reruns_are_bit_identical(mode, ml100k):
    assert gpu_available()
    S = fm_rel.rel2(ml100k)
    A, B = _block(S, mode, 3), _block(S, mode, 3)
    (a0, aw, av), (b0, bw, bv) = A.fm(), B.fm()
    assert a0 == b0 and np.array_equal(aw, bw) and np.array_equal(av, bv) and np.array_equal(A.predict(), B.predict())
    assert [h["rmse_train"] for h in A.history] == [h["rmse_train"] for h in B.history]
    A.close()
    B.close()


def test_classification_mcmc_runs_and_reruns_bit_identical(ml100k):
    assert gpu_available()
    S = fm_rel.rel2(ml100k, binary=True)
    A, B = _block(S, "philox", 3, task="c"), _block(S, "philox", 3, task="c")
    assert np.array_equal(A.predict(), B.predict()) and np.array_equal(A.fm()[2], B.fm()[2])
    acc = A.history[-1]["acc_avg"]
    print("acc", [h["acc_avg"] for h in A.history])
    assert 0.5 < acc <= 1.0 and np.all((A.predict() >= 0) & (A.predict() <= 1))
    A.close()
    B.close()


# ---- 5. nothing leaks
def test_device_usage_returns_to_its_counts_after_close():
    assert gpu_available()
    S = fm_rel.one_to_one()
    _block(S, "als", 1).close()  # the runtime's own first-use allocations
    before = device_usage()
    L = _block(S, "philox", 2)
    during = device_usage()
    L.close()
    after = device_usage()
    keys = ("dev_bytes", "dev_allocs", "pinned_bytes", "pinned_allocs", "streams", "events", "contexts")
    assert during["dev_allocs"] > before["dev_allocs"]
    assert {k: after[k] for k in keys} == {k: before[k] for k in keys}


# ---- 6. one case per block row
@pytest.mark.parametrize("mode", ["als", "philox"])
def test_one_case_per_block_row_equals_its_twin(mode):
    assert gpu_available()
    S = fm_rel.one_to_one()
    A, B = _block(S, mode, 5), _twin(S, mode, 5)
    _compare(A, B, S)
    A.close()
    B.close()


# ---- triples given a relation run through the general learner
def test_triples_with_a_relation_take_the_general_learner(ml100k):
    assert gpu_available()
    (tu, ti, tr), (su, si, sr) = ml100k
    tu, ti, tr, su, si, sr = tu[::8], ti[::8], tr[::8], su[::8], si[::8], sr[::8]
    I = int(max(tu.max(), su.max())) + 1
    rows = [[(u % 4, 1.0), (4 + u % 3, 0.5)] for u in range(I)] + [[(7, 1.0)]]
    R = Relation(fm_rel.rows_to_cases(rows, num_attr=8), tu, su)
    L = _learner("mcmc", "philox")
    L.add_relation(R)
    L.set_data(Data(tu, ti, tr), Data(su, si, sr))
    L.learn(sweeps=3)
    info = L.fm_relation_info()
    assert len(info) == 1 and info[0]["num_attr"] == 8 and L.fm_info()["num_attr"] == info[0]["attr_offset"] + 8
    assert L.fm_groups()["G"] == 2 and np.isfinite(L.history[-1]["rmse_avg"])
    L.close()


# ---- 7. refusals
def _raises(code, *words):
    class Ctx:
        def __enter__(self):
            self.cm = pytest.raises(SBMFError)
            self.e = self.cm.__enter__()

        def __exit__(self, *a):
            r = self.cm.__exit__(*a)
            assert self.e.value.code == code and all(w in str(self.e.value) for w in words), str(self.e.value)
            return r
    return Ctx()


def _small():
    rows = [[(0, 1.0)], [(1, 1.0), (2, 0.5)], [(2, 1.0)]]
    tr = fm_rel.rows_to_cases([[(0, 1.0)], [(1, 1.0)], [], [(0, 1.0)]], [1, 2, 3, 4])
    te = fm_rel.rows_to_cases([[(1, 1.0)], [(0, 1.0)]], [2, 3])
    return rows, tr, te


def test_bad_relations_are_refused_with_their_numbers():
    assert gpu_available()
    rows, tr, te = _small()
    blk = fm_rel.rows_to_cases(rows, num_attr=3)

    def attempt(R):
        L = _learner("als", "ref")
        L.add_relation(R)
        try:
            L.set_data(tr, te)
        finally:
            L.close()

    with _raises(SBMF_E_ARG, "block row 3", "3 rows"):  # a row index >= block->n
        attempt(Relation(blk, [0, 1, 3, 2], [0, 1]))
    with _raises(SBMF_E_ARG, "test case 1", "block row 7"):
        attempt(Relation(blk, [0, 1, 2, 2], [0, 7]))
    with _raises(SBMF_E_ARG, "train map", "3", "4 cases"):  # a map length different from the case count
        attempt(Relation(blk, [0, 1, 2], [0, 1]))
    with _raises(SBMF_E_ARG, "test map", "1", "2 cases"):
        attempt(Relation(blk, [0, 1, 2, 2], [0]))
    rep = Cases(np.array([0, 2, 3, 4], np.uint64), np.array([1, 1, 0, 2], np.uint32), np.ones(4, np.float32),
                np.zeros(3, np.float32), num_attr=3)
    with _raises(SBMF_E_ARG, "block row 0", "repeats attribute 1"):
        attempt(Relation(rep, [0, 1, 2, 2], [0, 1]))


def test_relations_are_refused_where_they_are_not_offered():
    assert gpu_available()
    rows, tr, te = _small()
    blk = fm_rel.rows_to_cases(rows, num_attr=3)
    c = blk._c()
    row = np.zeros(4, np.uint32)

    def add(M, ntr=4):
        return _lib.lib.sbmf_add_relation(M.ctx, C.byref(c), row.ctypes.data_as(C.POINTER(C.c_uint32)), ntr,
                                          row.ctypes.data_as(C.POINTER(C.c_uint32)), 0, None, 0)

    for kw, name in ((dict(method="mcmc", order="sbpmf"), "SBPMF"), (dict(method="vb"), "VB")):
        M = FMLearnSBPMF(num_factor=4, **kw)
        M.init()
        assert add(M) == SBMF_E_STATE
        msg = _lib.lib.sbmf_last_error(M.ctx).decode()
        assert name in msg and "sbmf_add_relation" in msg, msg
        M.close()
    comm = Communicator(1, 0, bytes(128))
    M = FMLearnSBPMF(num_factor=4, method="mcmc", order="libfm")
    M.init(comm=comm)
    assert add(M) == SBMF_E_STATE and b"joined a communicator" in _lib.lib.sbmf_last_error(M.ctx)
    M.close()
    comm.close()
    M = FMLearnSBPMF(num_factor=4, method="mcmc", order="sbpmf")
    M.init()
    assert _lib.lib.sbmf_test_virtual_rank(M.ctx, 2, 0) == 0
    assert add(M) == SBMF_E_STATE and b"virtual rank" in _lib.lib.sbmf_last_error(M.ctx)
    M.close()
    M = _learner("als", "ref")
    M.init()
    assert add(M) == SBMF_E_STATE and b"cases first" in _lib.lib.sbmf_last_error(M.ctx)  # no data yet
    M.close()
    # the per-group -regular speaks of the joined groups
    M = _learner("als", "ref", regular=(0.0, 1.0, 2.0, 3.0, 4.0, 5.0, 6.0))  # 1 + 2 * 3 for 2 groups
    M.add_relation(Relation(blk, [0, 1, 2, 2], [0, 1]))
    with pytest.raises(ValueError, match="1 \\+ 2G = 5"):
        M.set_data(tr, te)
    M.close()
