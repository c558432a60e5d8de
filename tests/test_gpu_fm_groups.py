"""Attribute groups (libFM's -meta) in the general libFM MCMC / ALS learner on the GPU: per-group
w_mu / w_lambda / v_mu / v_lambda drawn as fm_learn_mcmc.h:931-1089 draws them, every attribute
drawn from its own group's prior.  Against
  1. libFM itself (libfm.cpp compiled from its sources and run with -meta; goldens written by
     tests/make_fm_groups_golden.py) on fm4 in four groups, the reference's m1m100k files in two
     groups (triples, routed through the general learner) and edge_set() in five awkward groups,
  2. a sequential float64 loop, bit for bit, for the grouped column sums kernel,
  3. the ungrouped chain, bit for bit, for groups that change nothing,
  4. a serial numpy restatement of libFM's ALS with per-group precisions,
and: reruns are bit-identical in both RNG modes, nothing leaks, and what is not offered is refused."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import fm_cases
import fm_groups
from conftest import gpu_available, write_m1m100k_libfm
from sbmf import Cases, Communicator, Data, FMLearnSBPMF, SBMFError, _lib, device_usage
from sbmf._lib import CLI_PATH, SBMF_E_ARG, SBMF_E_STATE
from test_gpu_fm_cases import _check_against_restatement
from test_gpu_libfm import _within_printed

pytestmark = pytest.mark.gpu

ALS_REG = (0.0, 1.0, 2.0, 3.0, 4.0, 5.0, 10.0, 20.0, 30.0)
FM4 = {"mcmc": ("ref_libfm_mcmc_fm4_g4_d118_s1_i10", (0.0, 0.0, 0.0)),
       "als": ("ref_libfm_als_fm4_g4_d118_s1_i10", ALS_REG)}


def _learner(method, regular, K=8, seed=1, rng="ref", group=None):
    L = FMLearnSBPMF(num_factor=K, seed=seed, rng=rng, method="als" if method == "als" else "mcmc", order="libfm",
                     k0=1, k1=1, regular=regular, init_stdev=0.1)
    if group is not None:
        L.set_groups(group)
    return L


def _run(train, test, method, regular, iters, group=None, **kw):
    L = _learner(method, regular, group=group, **kw)
    L.set_data(train, test)
    L.learn(sweeps=iters)
    return L


def _iter_values(lines):
    return ([float(l.split("Train=")[1].split()[0]) for l in lines], [float(l.split("Test=")[1]) for l in lines])


def _hyper_row(fg, K):
    """fm_groups() in the order of the rlog's wmu[g] wlambda[g] vmu[g,f] vlambda[g,f] columns."""
    row = []
    for g in range(fg["G"]):
        row += [fg["w_mu"][g], fg["w_lambda"][g]]
        for f in range(K):
            row += [fg["v_mu"][g, f], fg["v_lambda"][g, f]]
    return np.array(row)


def _same_printed(x, ref):
    x, ref = np.asarray(x, float), np.asarray(ref, float)
    nan = np.isnan(ref)
    return x.shape == ref.shape and np.array_equal(np.isnan(x), nan) and _within_printed(x[~nan], ref[~nan])


# ---- 1. fm4 in four groups against libFM
@pytest.mark.parametrize("method", ["mcmc", "als"])
def test_fm4_python_matches_libfm(method, ml100k):
    assert gpu_available()
    name, regular = FM4[method]
    tr, te = fm_cases.fm4(ml100k)[:2]
    group = fm_groups.fm4_groups(ml100k)
    ref_lines, ref_pred, header, rows = fm_groups.golden(name)
    ref_train, ref_test = _iter_values(ref_lines)
    L = _learner(method, regular, group=group)
    L.set_data(tr, te)
    lead = header.index("wmu[0]")
    for it in range(10):  # the hyperparameters of every iteration, as libFM logged them
        L.learn(sweeps=1)
        fg = L.fm_groups()
        assert fg["G"] == 4 and fg["cnt"].tolist() == np.bincount(group, minlength=4).tolist()
        got = _hyper_row(fg, 8)
        print(it, np.max(np.abs(got - np.array(rows[it][lead:]))))
        assert _same_printed(got, rows[it][lead:]), it
    train = [h["rmse_train"] for h in L.history]
    test = [h["rmse_avg"] for h in L.history]
    print("train", train, "\ntest", test)
    assert _within_printed(train, ref_train) and _within_printed(test, ref_test)
    pred = L.predict()
    assert pred.shape == ref_pred.shape and _within_printed(pred, ref_pred)
    assert L.fm_info()["num_attr"] == len(group) and L.fm_info()["nranges"] == 8  # ranges do not depend on groups
    L.close()


@pytest.mark.parametrize("method", ["mcmc", "als"])
def test_fm4_cli_matches_libfm(method, ml100k, tmp_path):
    assert gpu_available()
    name, regular = FM4[method]
    trf, tef = fm_cases.write_fm4(ml100k, tmp_path)
    group = fm_groups.fm4_groups(ml100k)
    fm_groups.write_meta(os.path.join(str(tmp_path), "meta.txt"), group)
    cmd = [CLI_PATH, "-task", "r", "-train", trf, "-test", tef, "-dim", "1,1,8", "-iter", "10", "-method", method,
           "-meta", "meta.txt", "-out", "pred.txt", "-rlog", "rlog.txt", "-verbosity", "1"]
    if method == "als":
        cmd += ["-regular", ",".join("%g" % x for x in regular)]
    r = subprocess.run(cmd, cwd=str(tmp_path), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    lines = [l for l in r.stdout.splitlines() if l.startswith("#Iter=")]
    ref_lines, ref_pred, header, rows = fm_groups.golden(name)
    assert lines == ref_lines
    pred = np.array([float(x) for x in open(os.path.join(str(tmp_path), "pred.txt")).read().split()])
    assert pred.shape == ref_pred.shape and _within_printed(pred, ref_pred)
    # DataMetaInfo::debug's lines
    assert "#attr=%d\t#groups=4" % len(group) in r.stdout
    for g, c in enumerate(np.bincount(group, minlength=4)):
        assert "#attr_in_group[%d]=%d" % (g, c) in r.stdout
    # the rlog: libFM's columns lead, and the group columns agree at every iteration
    t = open(os.path.join(str(tmp_path), "rlog.txt")).read().splitlines()
    ours = t[0].split("\t")
    assert ours[:len(header)] == header and all(c.startswith("sbmf_") for c in ours[len(header):])
    lead = header.index("wmu[0]")
    assert len(t) == 11
    for it in range(10):
        got = [float(x) for x in t[1 + it].split("\t")[lead:len(header)]]
        assert _same_printed(got, rows[it][lead:]), it


# ---- 2. the reference's two-feature files with a users / items meta: routed through the general learner
def test_m1m100k_cli_with_meta_matches_libfm(m1m100k, tmp_path):
    assert gpu_available()
    write_m1m100k_libfm(tmp_path)
    group = fm_groups.m1m100k_groups(m1m100k)
    fm_groups.write_meta(os.path.join(str(tmp_path), "meta.txt"), group)
    cmd = [CLI_PATH, "-task", "r", "-train", "train_libfm", "-test", "test_libfm", "-dim", "1,1,8", "-iter", "10",
           "-method", "mcmc", "-meta", "meta.txt", "-out", "pred.txt"]
    r = subprocess.run(cmd, cwd=str(tmp_path), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    ref_lines, ref_pred, _, _ = fm_groups.golden("ref_libfm_mcmc_m1m100k_g2_d118_s1_i10")
    assert [l for l in r.stdout.splitlines() if l.startswith("#Iter=")] == ref_lines
    pred = np.loadtxt(tmp_path / "pred.txt")
    assert pred.shape == ref_pred.shape and _within_printed(pred, ref_pred)
    assert "#groups=2" in r.stdout and "#attributes=%d\t#ranges=2" % len(group) in r.stdout  # sbmf_fm_info succeeded


def test_triples_given_groups_take_the_general_learner(m1m100k):
    assert gpu_available()
    (tu, ti, tr_), (su, si, sr) = m1m100k
    I = int(max(tu.max(), su.max())) + 1
    group = fm_groups.m1m100k_groups(m1m100k)
    L = _learner("mcmc", (0.0, 0.0, 0.0), group=group)
    L.set_data(Data(tu, ti - I, tr_), Data(su, si - I, sr), num_users=I)
    L.learn(sweeps=10)
    assert L.fm_info()["num_attr"] == len(group) and L.fm_info()["nranges"] == 2
    ref_lines, ref_pred, _, _ = fm_groups.golden("ref_libfm_mcmc_m1m100k_g2_d118_s1_i10")
    ref_train, ref_test = _iter_values(ref_lines)
    assert _within_printed([h["rmse_train"] for h in L.history], ref_train)
    assert _within_printed([h["rmse_avg"] for h in L.history], ref_test)
    assert _within_printed(L.predict(), ref_pred)
    U, V = L.factors()  # the users-first view still reads back
    assert U.shape == (I, 8) and np.array_equal(U.T, L.fm()[2][:, :I])
    L.close()


# ---- 3. every pass kind reads a non-zero group: rows of 0, 1, 63, 64, 65, 255, 256, 257 and 1025 cases
@pytest.mark.parametrize("bins", ["default", "chunked"])
def test_edge_set_cli_matches_libfm(bins, tmp_path, monkeypatch):
    assert gpu_available()
    trf, tef = fm_groups.write_edge(tmp_path)
    group = fm_groups.edge_groups()
    assert group.max() == 4 and 3 not in group and group[:9].tolist() == [0, 1, 0, 1, 0, 1, 0, 1, 0]
    fm_groups.write_meta(os.path.join(str(tmp_path), "meta.txt"), group)
    env = dict(os.environ)
    if bins == "chunked":  # rows above 256 cases in chunks of 64: chunk sums, chunk draw and the replay
        env.update(SBMF_FMM_LONG="256", SBMF_FMM_CHUNK="64")
    cmd = [CLI_PATH, "-task", "r", "-train", trf, "-test", tef, "-dim", "1,1,8", "-iter", "5", "-method", "mcmc",
           "-meta", "meta.txt", "-out", "pred.txt", "-rlog", "rlog.txt"]
    r = subprocess.run(cmd, cwd=str(tmp_path), capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stderr
    ref_lines, ref_pred, header, rows = fm_groups.golden("ref_libfm_mcmc_edge_g5_d118_s1_i5")
    assert [l for l in r.stdout.splitlines() if l.startswith("#Iter=")] == ref_lines
    pred = np.loadtxt(tmp_path / "pred.txt")
    assert pred.shape == ref_pred.shape and _within_printed(pred, ref_pred)
    assert "#groups=5" in r.stdout
    t = open(os.path.join(str(tmp_path), "rlog.txt")).read().splitlines()
    lead = header.index("wmu[0]")
    for it in range(5):  # the empty group's draws included
        got = [float(x) for x in t[1 + it].split("\t")[lead:len(header)]]
        assert _same_printed(got, rows[it][lead:]), it


# ---- 4. the grouped sums are the host loop's, bit for bit
def _field_cases(p, n, seed):
    """n cases over three one-hot fields that split [0, p - 1) into thirds (three ranges)."""
    rs = np.random.RandomState(seed)
    q = p - 1  # the largest id is p - 2: num_attribute = p
    b = [0, q // 3, 2 * q // 3, q]
    attr = np.stack([b[j] + (np.arange(n) * pr + j) % (b[j + 1] - b[j]) for j, pr in enumerate((7, 13, 29))], 1)
    attr[0, 2] = q - 1
    x = rs.choice([0.5, 1.0, -1.5, 0.25], size=(n, 3)).astype(np.float32)
    return Cases(np.arange(n + 1, dtype=np.uint64) * 3, attr.ravel().astype(np.uint32), x.ravel(),
                 rs.randint(1, 6, n).astype(np.float32))


SIZES = [0, 1, 2047, 2048, 2049, 4097]  # contiguous groups: the staging chunk +-1 and a second full chunk


def _sums_groups(kind):
    if kind == "mod3":
        return np.arange(6200, dtype=np.uint32) % 3
    contiguous = np.repeat(np.arange(len(SIZES), dtype=np.uint32), SIZES)
    if kind == "contiguous":
        return contiguous
    return np.concatenate([np.arange(6200, dtype=np.uint32) % 3, 3 + contiguous])  # both in one table


@pytest.mark.parametrize("kind", ["mod3", "contiguous", "mod3+contiguous"])
def test_grouped_sums_are_the_host_loops(kind):
    assert gpu_available()
    group = _sums_groups(kind)
    p, K, G = len(group), 3, int(group.max()) + 1
    tr, te = _field_cases(p, 600, 5), _field_cases(p, 40, 6)
    assert fm_groups.num_attribute(tr, te) == p
    L = _run(tr, te, "mcmc", (0.0, 0.0, 0.0), 2, group=group, K=K)
    out = np.zeros((K + 1, G, 2))
    assert _lib.lib.sbmf_test_fm_group_sums(L.ctx, out.ctypes.data_as(C.POINTER(C.c_double))) == 0
    _, w, v = L.fm()
    fg = L.fm_groups()
    assert fg["cnt"].tolist() == np.bincount(group, minlength=G).tolist()
    bad = 0
    for c in range(K + 1):
        x = v[c] if c < K else w
        for g in range(G):
            mu = fg["v_mu"][g, c] if c < K else fg["w_mu"][g]
            xg = x[group == g]  # ascending attribute id
            d = xg - mu
            gm0 = 1.0 * (mu - 0.0) * (mu - 0.0) + 1.0  # beta_0 (mu - mu_0)^2 + gamma_0
            gm = np.add.accumulate(np.concatenate([[gm0], d * d]))[-1]
            m = np.add.accumulate(np.concatenate([[0.0], xg]))[-1]
            if not (out[c, g, 0] == gm and out[c, g, 1] == m):
                bad += 1
                print("column %d group %d (%d members): gm %r / %r, m %r / %r" % (c, g, len(xg), out[c, g, 0], gm,
                                                                                 out[c, g, 1], m))
    assert bad == 0
    L.close()


def test_group_sums_hook_serves_an_ungrouped_context():
    assert gpu_available()
    tr, te = fm_cases.small_cases()
    L = _run(tr, te, "mcmc", (0.0, 0.0, 0.0), 2, K=4, seed=3)
    out = np.zeros((5, 1, 2))
    assert _lib.lib.sbmf_test_fm_group_sums(L.ctx, out.ctypes.data_as(C.POINTER(C.c_double))) == 0
    _, w, v = L.fm()
    h = L.hyper()
    for c in range(5):
        x, mu = (v[c], h["mu_u"][c]) if c < 4 else (w, h["sigma_v"][1])  # sbmf_get_hyper: [v_lambda | v_mu | w_lambda, w_mu]
        d = x - mu
        assert out[c, 0, 0] == np.add.accumulate(np.concatenate([[1.0 * mu * mu + 1.0], d * d]))[-1]
        assert out[c, 0, 1] == np.add.accumulate(np.concatenate([[0.0], x]))[-1]
    L.close()


# ---- 5. groups that change nothing
def _state(L):
    w0, w, v = L.fm()
    return w0, w, v, L.predict(), [h["rmse_train"] for h in L.history], [h["rmse_avg"] for h in L.history]


def _assert_same_bits(a, b):
    assert a[0] == b[0] and all(np.array_equal(x, y) for x, y in zip(a[1:4], b[1:4])) and a[4:6] == b[4:6]


def test_als_groups_with_equal_precisions_change_nothing(ml100k):
    assert gpu_available()
    tr, te = fm_cases.fm4(ml100k)[:2]
    A = _run(tr, te, "als", (0.0, 2.0, 10.0), 3)
    B = _run(tr, te, "als", (0.0,) + (2.0,) * 4 + (10.0,) * 4, 3, group=fm_groups.fm4_groups(ml100k))
    assert B.fm_groups()["G"] == 4 and A.fm_groups()["G"] == 1
    _assert_same_bits(_state(A), _state(B))
    A.close()
    B.close()


@pytest.mark.parametrize("rng", ["ref", "philox"])
def test_one_explicit_group_is_the_ungrouped_chain(rng, ml100k):
    assert gpu_available()
    tr, te = fm_cases.fm4(ml100k)[:2]
    A = _run(tr, te, "mcmc", (0.0, 0.0, 0.0), 3, rng=rng)
    B = _run(tr, te, "mcmc", (0.0, 0.0, 0.0), 3, rng=rng, group=np.zeros(fm_groups.num_attribute(tr, te), np.uint32))
    _assert_same_bits(_state(A), _state(B))
    assert A.fm_info()["launches_per_iter"] == B.fm_info()["launches_per_iter"]
    ha, hb = A.hyper(), B.hyper()  # one group: sbmf_get_hyper as before
    assert all(np.array_equal(ha[k], hb[k]) for k in ha)
    A.close()
    B.close()


# ---- 6. ALS with distinct per-group precisions against the serial restatement
_RESTATED = {}


def _restated(key, tr, te, K, seed, reg0, gw, gv, group, record):
    if key not in _RESTATED:
        _RESTATED[key] = tuple(fm_groups.als_restatement_groups(tr, te, K, max(record), seed, reg0, gw, gv, group, ft,
                                                                record=record) for ft in (np.float64, np.longdouble))
    return _RESTATED[key]


def _check_als(key, tr, te, K, seed, regular, group, record):
    G = int(group.max()) + 1
    a, b = _restated(key, tr, te, K, seed, regular[0], regular[1:1 + G], regular[1 + G:], group, record)
    L = _learner("als", regular, K=K, seed=seed, group=group)
    L.set_data(tr, te)
    done = 0
    for it in record:
        L.learn(sweeps=it - done)
        done = it
        _check_against_restatement(L, it, a, b)
    fg = L.fm_groups()
    assert fg["w_lambda"].tolist() == list(regular[1:1 + G]) and np.all(fg["w_mu"] == 0.0)
    assert np.array_equal(fg["v_lambda"], np.repeat(np.array(regular[1 + G:])[:, None], K, 1))
    L.close()


def test_als_per_group_precisions_match_serial_restatement_small():
    assert gpu_available()
    tr, te = fm_cases.small_cases()
    group = np.array([0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 3, 2, 3], np.uint32)  # 2 and 3 interleaved
    assert len(group) == fm_groups.num_attribute(tr, te)
    _check_als("small", tr, te, 4, 3, (1.0, 2.0, 0.5, 4.0, 0.25, 5.0, 1.0, 8.0, 3.0), group, (1, 2, 5))


def test_als_per_group_precisions_match_serial_restatement_fm4(ml100k):
    assert gpu_available()
    tr, te = fm_cases.fm4(ml100k)[:2]
    _check_als("fm4", tr, te, 8, 1, ALS_REG, fm_groups.fm4_groups(ml100k), (1, 2))


# ---- 7. rerun and leaks
@pytest.mark.parametrize("rng", ["ref", "philox"])
def test_rerun_is_bit_identical_and_nothing_leaks(rng, ml100k):
    assert gpu_available()
    tr, te = fm_cases.fm4(ml100k)[:2]
    group = fm_groups.fm4_groups(ml100k)
    before = device_usage()
    runs = []
    for _ in range(2):
        L = _run(tr, te, "mcmc", (0.0, 0.0, 0.0), 3, rng=rng, group=group)
        runs.append(_state(L) + (_hyper_row(L.fm_groups(), 8),))
        assert device_usage()["dev_allocs"] > before["dev_allocs"]
        L.close()
    _assert_same_bits(runs[0], runs[1])
    assert np.array_equal(runs[0][-1], runs[1][-1])
    after = device_usage()
    for k in ("dev_bytes", "dev_allocs", "pinned_bytes", "pinned_allocs", "streams", "events", "contexts", "comms"):
        assert after[k] == before[k], (k, before[k], after[k])


# ---- 8. refusals
def _raises(code, *words):
    class Ctx:
        def __enter__(self):
            self.cm = pytest.raises(SBMFError)
            self.e = self.cm.__enter__()
            return self.e

        def __exit__(self, *a):
            r = self.cm.__exit__(*a)
            assert self.e.value.code == code and all(w in str(self.e.value) for w in words), str(self.e.value)
            return r
    return Ctx()


def test_groups_are_refused_where_they_are_not_offered():
    assert gpu_available()
    g = np.array([0, 1, 1], np.uint32)
    for kw, name in ((dict(method="mcmc", order="sbpmf"), "SBPMF"), (dict(method="vb"), "VB")):
        M = FMLearnSBPMF(num_factor=4, **kw)
        M.init()
        with _raises(SBMF_E_STATE, name, "sbmf_set_attr_groups"):
            M.set_groups(g)
        r = np.ones(2)
        assert _lib.lib.sbmf_set_group_regular(M.ctx, 2, r.ctypes.data_as(C.POINTER(C.c_double)),
                                               r.ctypes.data_as(C.POINTER(C.c_double))) == SBMF_E_STATE
        M.close()
    comm = Communicator(1, 0, bytes(128))
    M = FMLearnSBPMF(num_factor=4, method="mcmc", order="libfm")
    M.init(comm=comm)
    with _raises(SBMF_E_STATE, "joined a communicator"):
        M.set_groups(g)
    M.close()
    comm.close()
    M = FMLearnSBPMF(num_factor=4, method="mcmc", order="sbpmf")
    M.init()
    assert _lib.lib.sbmf_test_virtual_rank(M.ctx, 2, 0) == 0
    with _raises(SBMF_E_STATE, "virtual rank"):
        M.set_groups(g)
    M.close()


def test_group_count_and_regular_count_are_checked():
    assert gpu_available()
    tr, te = fm_cases.small_cases()
    p = fm_groups.num_attribute(tr, te)
    L = _learner("als", (0.0, 1.0, 1.0), K=4, group=np.zeros(p - 1, np.uint32))
    with _raises(SBMF_E_ARG, str(p - 1), str(p)):  # the count is checked at prepare when the data comes later
        L.set_data(tr, te)
    L.close()
    L = _learner("als", (0.0, 1.0, 1.0), K=4)
    L.init()
    c = tr._c()
    L._check(_lib.lib.sbmf_set_train_cases(L.ctx, C.byref(c)))
    c = te._c()
    L._check(_lib.lib.sbmf_set_test_cases(L.ctx, C.byref(c)))
    with _raises(SBMF_E_ARG, str(p + 1), str(p)):  # ... and at once when it is already there
        L.set_groups(np.zeros(p + 1, np.uint32))
    L.set_groups(np.arange(p) % 3)
    r = np.ones(2)
    rc = _lib.lib.sbmf_set_group_regular(L.ctx, 2, r.ctypes.data_as(C.POINTER(C.c_double)),
                                         r.ctypes.data_as(C.POINTER(C.c_double)))
    assert rc == SBMF_E_ARG and b"3" in _lib.lib.sbmf_last_error(L.ctx)
    L.set_groups([])  # n = 0 drops the groups
    L._check(_lib.lib.sbmf_prepare(L.ctx))
    assert L.fm_groups()["G"] == 1 and L.fm_groups()["cnt"].tolist() == [p]
    L.close()


def test_get_hyper_points_to_the_group_getter():
    assert gpu_available()
    tr, te = fm_cases.small_cases()
    L = _run(tr, te, "mcmc", (0.0, 0.0, 0.0), 1, K=4, group=np.arange(fm_groups.num_attribute(tr, te)) % 2)
    with _raises(SBMF_E_STATE, "sbmf_get_fm_groups"):
        L.hyper()
    tau = C.c_double()  # tau alone is still served (the -rlog line reads it)
    assert _lib.lib.sbmf_get_hyper(L.ctx, None, C.byref(tau)) == 0 and tau.value == L.history[-1]["tau"]
    L.close()
