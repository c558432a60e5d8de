"""The libFM learners' chains (csrc/fmc.cpp with the layouts of fmm.cpp and fmg.cpp), held to
the bits: per case the sha256 of the float64 bytes of the per-iteration rmse_train / rmse_avg /
rmse_this / tau, of predict(), of the model (fm() on the general learner, factors() + biases()
on the two-attribute one) and of hyper(), and timing().n_launch, against
tests/golden/fm_chain_pins.json.  The first values of every array are kept beside its digest, so
a mismatch can be read.  The other tests hold the learners to libFM's printed digits or to the
oracle within 1e-9: a changed Philox tag, a swapped host draw or a lost launch passes those; it
does not pass here.

The fixture was recorded from the build before the host chain of the two learners was merged,
through the Python interface alone; the grouped cases (groups5-*: k_fmg_gpass, k_fmg_gchunk_draw and
k_fmg_gsums inside a chain, fm_groups() in place of hyper(), which refuses G > 1) from the build
before the two kernel files took their shared code from csrc/fm_dev.h.  To record it again, run
this file on an MI355X with SBMF_FM_PINS_RECORD=1 in the environment: every case then writes its
entry instead of comparing.  Only a change that means to alter the learners' arithmetic, their
launch counts or the order of their draws may do so, and says so; recording twice must give the
same file.

num_factor = 0 (libFM's -dim 1,1,0) is refused by sbmf_create, so those cases pin the refusal."""
import hashlib
import json
import os

import numpy as np
import pytest

import fm_cases
import fm_edge
import fm_groups
from conftest import GOLD, gpu_available
from sbmf import Data, FMLearnSBPMF, SBMFError
from test_gpu_multirank import _run_ranks

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(GOLD, "fm_chain_pins.json")
RECORD = os.environ.get("SBMF_FM_PINS_RECORD") == "1"


def _digest(a):
    a = np.ascontiguousarray(a, np.float64)
    return {"sha256": hashlib.sha256(a.tobytes()).hexdigest(), "size": int(a.size),
            "head": [repr(float(x)) for x in a.ravel()[:4]]}


def _hyper(L):
    hy = L.hyper()
    return np.concatenate([hy["sigma_u"], hy["mu_u"], hy["sigma_v"], hy["mu_v"], [hy["tau"]]])


def _group_hyper(L):
    fg = L.fm_groups()
    return np.concatenate([np.ravel(fg[k]) for k in ("cnt", "w_lambda", "w_mu", "v_lambda", "v_mu")])


def _pins(L, general, grouped=False):
    rec = {k: _digest([h[k] for h in L.history]) for k in ("rmse_train", "rmse_avg", "rmse_this", "tau")}
    rec["predict"] = _digest(L.predict() if L._test is not None else np.zeros(0))
    if general:
        w0, w, v = L.fm()
        rec.update(w0=_digest([w0]), w=_digest(w), v=_digest(v))
    else:
        (U, V), (bu, bv, b0) = L.factors(), L.biases()
        rec.update(U=_digest(U), V=_digest(V), bu=_digest(bu), bv=_digest(bv), b0=_digest([b0]))
    if grouped:  # sbmf_get_hyper refuses G > 1: the group getter's arrays stand in its place
        rec["fm_groups"] = _digest(_group_hyper(L))
    else:
        rec["hyper"] = _digest(_hyper(L))
    rec["n_launch"] = int(L.timing().n_launch)
    return rec


def _check(case, rec):
    if RECORD:
        pins = {}
        if os.path.exists(FIXTURE):
            with open(FIXTURE) as f:
                pins = json.load(f)
        pins[case] = rec
        with open(FIXTURE, "w") as f:
            json.dump(pins, f, indent=1, sort_keys=True)
            f.write("\n")
        return
    with open(FIXTURE) as f:
        want = json.load(f)[case]
    for k in sorted(set(want) | set(rec)):
        print(case, k, "pinned", want.get(k), "now", rec.get(k))
    assert rec == want


def _learner(method="mcmc", rng="ref", dim=(1, 1, 4), regular=(0.0, 0.0, 0.0), seed=3):
    return FMLearnSBPMF(num_factor=dim[2], seed=seed, rng=rng, method=method, order="libfm", k0=dim[0], k1=dim[1],
                        regular=regular, init_stdev=0.1)


def _run(train, test, general, iters=3, stop_then_one=False, group=None, dims=(0, 0), **kw):
    """The pins of one run: `iters` iterations, or (stop_then_one) five iterations whose callback
    stops after the second, then one more learn(1) -- the break and the carried iteration count."""
    L = _learner(**kw)
    if group is not None:
        L.set_groups(group)
    try:
        L.set_data(train, test, num_users=dims[0], num_items=dims[1])
    except SBMFError as e:
        L.close()
        return {"error_code": int(e.code), "error": str(e)}
    if stop_then_one:
        L.learn(sweeps=5, callback=lambda _: len(L.history) >= 2)
        assert len(L.history) == 2
        L.learn(sweeps=1)
    else:
        L.learn(sweeps=iters)
    assert len(L.history) == 3
    rec = _pins(L, general, group is not None)
    L.close()
    return rec


# ---- the two-attribute learner
TWO = {"mcmc-ref": {}, "mcmc-philox": dict(rng="philox"),
       "als-stop2-then1": dict(method="als", regular=(0.5, 1.0, 4.0), stop_then_one=True),
       "dim004": dict(dim=(0, 0, 4)), "dim110": dict(dim=(1, 1, 0))}


@pytest.mark.parametrize("case", sorted(TWO))
def test_two_attribute_ragged(case, ragged):
    assert gpu_available()
    tr, te = ragged
    _check("two/ragged/" + case, _run(Data(*tr), Data(*te), False, **TWO[case]))


def test_two_attribute_ragged_without_test_set(ragged):
    assert gpu_available()
    _check("two/ragged/no-test", _run(Data(*ragged[0]), None, False))


@pytest.mark.parametrize("chunk", ["64", "0"])
def test_two_attribute_ml100k_long_rows(chunk, ml100k, monkeypatch):
    """Rows above 256 cases in chunks of 64, and on one 1024-thread workgroup each."""
    assert gpu_available()
    tr, te = ml100k
    monkeypatch.setenv("SBMF_FMM_LONG", "256")
    monkeypatch.setenv("SBMF_FMM_CHUNK", chunk)
    _check("two/ml100k/long256-chunk" + chunk, _run(Data(*tr), Data(*te), False, seed=1))


@pytest.mark.parametrize("method,regular", [("mcmc", "0,0,0"), ("als", "0.5,1,4")], ids=["mcmc", "als"])
def test_two_attribute_two_ranks(method, regular, tmp_path):
    """Two ranks on one GPU (host communicator): rank 0's arrays are pinned, every rank equals it."""
    assert gpu_available()
    outs = _run_ranks(tmp_path, 2, ["4", "3", "3", "ref", "0", "1,1;" + regular, "als" if method == "als" else "libfm"],
                      env={"SBMF_WORKER_DATA": "ragged"})
    z0, z1 = np.load(outs[0]), np.load(outs[1])
    keys = ("rmse_train", "rmse", "rmse_this", "tau", "pred", "U", "V", "bu", "bv", "b0", "hyper")
    for k in keys:
        assert np.array_equal(z1[k], z0[k], equal_nan=True), k
    rec = {k: _digest(z0[k]) for k in keys}
    rec["n_launch"] = int(z0["n_launch"][0])
    _check("two/ragged/2ranks-" + method, rec)


# the row-form edge set of tests/fm_edge.py at tests/test_gpu_fm_edge.py's settings: rows of 0 .. 4097
# cases on both sides, the 4097-case rows in two chunks or (chunk0) whole with a tail case
TWO_EDGE = {"mcmc-ref": {}, "mcmc-philox": dict(rng="philox"), "als": dict(method="als", regular=(0.5, 1.0, 4.0)),
            "chunk0-mcmc-ref": dict(env={"SBMF_FMM_CHUNK": "0"})}


@pytest.mark.parametrize("case", sorted(TWO_EDGE))
def test_two_attribute_edge_set(case, monkeypatch):
    assert gpu_available()
    kw = dict(TWO_EDGE[case])
    for k, v in kw.pop("env", {}).items():
        monkeypatch.setenv(k, v)
    tr, te, dims = fm_edge.generate()
    _check("two/edge/" + case, _run(Data(*tr), Data(*te), False, dims=dims, dim=(1, 1, 8), seed=2, **kw))


def test_two_attribute_edge_set_two_ranks(tmp_path):
    """The user rows of 4097 cases whole on their rank, the item rows by their share on each."""
    assert gpu_available()
    outs = _run_ranks(tmp_path, 2, ["8", "3", "2", "ref", "0", "1,1;0,0,0", "libfm"], env={"SBMF_WORKER_DATA": "edge"})
    z0, z1 = np.load(outs[0]), np.load(outs[1])
    keys = ("rmse_train", "rmse", "rmse_this", "tau", "pred", "U", "V", "bu", "bv", "b0", "hyper")
    for k in keys:
        assert np.array_equal(z1[k], z0[k], equal_nan=True), k
    rec = {k: _digest(z0[k]) for k in keys}
    rec["n_launch"] = int(z0["n_launch"][0])
    _check("two/edge/2ranks-mcmc", rec)


# ---- the general learner
EDGE = {"mcmc-ref-long256-chunk64": dict(env=True), "mcmc-philox": dict(rng="philox"), "dim004": dict(dim=(0, 0, 4)),
        "dim110": dict(dim=(1, 1, 0))}


@pytest.mark.parametrize("case", sorted(EDGE))
def test_general_edge_set(case, monkeypatch):
    assert gpu_available()
    kw = dict(EDGE[case])
    if kw.pop("env", False):
        monkeypatch.setenv("SBMF_FMM_LONG", "256")
        monkeypatch.setenv("SBMF_FMM_CHUNK", "64")
    tr, te = fm_cases.edge_set()
    _check("general/edge/" + case, _run(tr, te, True, seed=2, **kw))


# five group ids, one empty, two interleaved over the rows at the bin and chunk edges
# (fm_groups.edge_groups()); the ALS case's -regular is w0's, then the five groups' for w, then for v
GROUPS5 = {"mcmc-ref-long256-chunk64": dict(env=True), "mcmc-philox": dict(rng="philox"),
           "als": dict(method="als", regular=(0.25, 0.5, 1.0, 1.5, 2.0, 2.5, 3.0, 4.0, 5.0, 6.0, 7.0))}


@pytest.mark.parametrize("case", sorted(GROUPS5))
def test_general_edge_set_groups(case, monkeypatch):
    """k_fmg_gpass, k_fmg_gchunk_draw (the chunked case) and k_fmg_gsums inside a chain."""
    assert gpu_available()
    kw = dict(GROUPS5[case])
    if kw.pop("env", False):
        monkeypatch.setenv("SBMF_FMM_LONG", "256")
        monkeypatch.setenv("SBMF_FMM_CHUNK", "64")
    tr, te = fm_cases.edge_set()
    _check("general/edge/groups5-" + case, _run(tr, te, True, seed=2, group=fm_groups.edge_groups(), **kw))


def test_general_small_cases_als():
    assert gpu_available()
    tr, te = fm_cases.small_cases()
    _check("general/small/als-stop2-then1", _run(tr, te, True, method="als", regular=(1.0, 2.0, 5.0),
                                                 stop_then_one=True))


def test_general_user_item_view(ragged, monkeypatch):
    """SBMF_FMM_GENERAL=1: the triples through the general learner, read back by user and item."""
    assert gpu_available()
    tr, te = ragged
    monkeypatch.setenv("SBMF_FMM_GENERAL", "1")
    _check("general/ragged/user-item-view", _run(Data(*tr), Data(*te), False))


def test_general_without_test_set():
    assert gpu_available()
    _check("general/edge/no-test", _run(fm_cases.edge_set()[0], None, True, seed=2))
