"""Classification (libFM's -task c) without a GPU: the host restatement of the reference's
truncated normals (sbmf_test_tgauss, host mode) against the exact moments, the fixtures of the GPU
tests, and the refusals of the command line and of the C ABI that need no device."""
import ctypes as C
import math
import subprocess

import numpy as np
import pytest

import fm_class
import sbmf
from sbmf import _lib, tgauss
from sbmf._lib import CLI_PATH
from test_gpu_fm_class import MEANS, _check_tgauss_moments


def test_host_tgauss_sides_and_moments():
    _check_tgauss_moments("host")


def test_host_tgauss_is_the_reference_stream_in_order():
    """The draws consume one sequential stream: a prefix is a prefix, and the first draw of a positive
    case at mean 0 is the first Leva normal of the stream that is >= 0."""
    mean = np.array(MEANS + MEANS)
    sign = np.array([1] * 7 + [-1] * 7, np.int32)
    full = tgauss(mean, sign, seed=7, mode="host")
    assert np.array_equal(tgauss(mean[:5], sign[:5], seed=7, mode="host"), full[:5])
    z = sbmf.ref_stream(7, 1, 64)
    assert tgauss([0.0], 1, seed=7, mode="host")[0] == z[z >= 0][0]
    assert tgauss([0.0], -1, seed=7, mode="host")[0] == -z[z >= 0][0]


def test_exact_moments_helper():
    em, ev = fm_class.tgauss_moments(0.0, True)  # the half normal
    assert abs(em - math.sqrt(2 / math.pi)) < 1e-15 and abs(ev - (1 - 2 / math.pi)) < 1e-15
    assert fm_class.tgauss_moments(1.5, False) == (-fm_class.tgauss_moments(-1.5, True)[0],
                                                    fm_class.tgauss_moments(-1.5, True)[1])
    assert abs(fm_class.tgauss_fourth_central(0.0, True) - (3 - 4 / math.pi - 12 / math.pi ** 2) ) < 1e-6


def test_edge_class_fixture():
    tr, te = fm_class.edge_class()
    assert tr.ptr[-1] == tr.ptr[-2] and tr.target[-1] == -1.0  # the case without features
    assert set(np.unique(tr.target)) == {-1.0, 1.0} and set(np.unique(te.target)) == {-1.0, 1.0}


def test_task_is_checked_before_the_device():
    ctx = C.c_void_p()
    cfg = sbmf.config_default()
    assert cfg.task == _lib.TASK_REGRESSION
    cfg.task = 2
    assert _lib.lib.sbmf_create(C.byref(cfg), C.byref(ctx)) == sbmf.SBMF_E_ARG
    for method, name in ((_lib.METHOD_MCMC, "SBPMF"), (_lib.METHOD_VB, "VB")):
        cfg = sbmf.config_default()
        cfg.method, cfg.task = method, _lib.TASK_CLASSIFICATION
        assert _lib.lib.sbmf_create(C.byref(cfg), C.byref(ctx)) == sbmf.SBMF_E_ARG
        msg = _lib.lib.sbmf_last_global_error().decode()
        assert name in msg and "classification" in msg
    with pytest.raises(ValueError):
        sbmf.FMLearnSBPMF(task="p")
    assert _lib.lib.sbmf_test_tgauss(2, 0, 1, 0, 0, None, None, None, None) == sbmf.SBMF_E_ARG


@pytest.mark.parametrize("args", [["-method", "vb"], ["-order", "sbpmf"], ["-quirks", "none"], ["-format", "triple"], []])
def test_cli_keeps_its_refusal_for_the_other_learners(args, tmp_path):
    """-task c with a learner that has no classification: today's text, and no input file is needed
    to decide it (the files named here do not exist)."""
    r = subprocess.run([CLI_PATH, "-task", "c", "-train", "a", "-test", "b"] + args, cwd=str(tmp_path),
                       capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "only -task r" in r.stderr
    assert "Unable to open" not in r.stderr and "Loading" not in r.stdout


def test_cli_refuses_recommend_with_classification(tmp_path):
    r = subprocess.run([CLI_PATH, "-task", "c", "-method", "als", "-train", "a", "-test", "b", "-recommend", "x",
                        "-rec_users", "u"], cwd=str(tmp_path), capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "-recommend is offered by the SBPMF sampler" in r.stderr
    r = subprocess.run([CLI_PATH, "-task", "x", "-train", "a", "-test", "b"], cwd=str(tmp_path), capture_output=True,
                       text=True, timeout=60)
    assert r.returncode != 0 and "only -task r" in r.stderr
