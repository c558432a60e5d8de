"""Attribute groups (libFM's -meta) of the general libFM learner, the parts that need no GPU:
the meta-file loader against DVector<uint>::load's rule (the first num_attr whitespace-separated
unsigned integers; a short file or a non-number refused, naming the entry), the argument and
state errors of the group calls that are decided before any device work, and the two -regular
parsers (Python's and the command line's): 0 / 1 / 3 / 1 + 2G values and a wrong count."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import sbmf
from sbmf import SBMFError, _lib
from sbmf._lib import CLI_PATH, SBMF_E_ARG, SBMF_E_IO

lib = _lib.lib


# ---- the meta loader
def test_meta_loader_reads_the_first_num_attr_entries(tmp_path):
    p = tmp_path / "meta"
    p.write_text("0 0\t1\n\n 1   2\r\n2 7\n")  # blanks, tabs, CR LF, an empty line
    assert sbmf.load_libfm_meta(p, 7).tolist() == [0, 0, 1, 1, 2, 2, 7]
    assert sbmf.load_libfm_meta(p, 5).tolist() == [0, 0, 1, 1, 2]  # extra entries are ignored
    assert sbmf.load_libfm_meta(p, 0).tolist() == []


def test_meta_loader_reports_the_group_count_with_an_empty_group_id(tmp_path):
    p = tmp_path / "meta"
    p.write_text("0\n3\n0\n")  # no attribute carries 1 or 2: they are groups all the same
    g, G = np.zeros(3, np.uint32), C.c_uint32()
    assert lib.sbmf_load_libfm_meta(str(p).encode(), 3, g.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(G)) == 0
    assert G.value == 4 and g.tolist() == [0, 3, 0]


def test_meta_loader_refuses_a_short_file(tmp_path):
    p = tmp_path / "meta"
    p.write_text("0 1 1\n")
    with pytest.raises(SBMFError) as e:
        sbmf.load_libfm_meta(p, 4)
    assert e.value.code == SBMF_E_IO and "3 group ids" in str(e.value) and "entry 4" in str(e.value)


@pytest.mark.parametrize("text,entry", [("0 1 x 1", 3), ("0 -1 1 1", 2), ("0 1 1 1.5", 4), ("0 1 99999999999 1", 3),
                                        ("2a 1 1 1", 1)])
def test_meta_loader_refuses_a_non_number(tmp_path, text, entry):
    p = tmp_path / "meta"
    p.write_text(text)
    with pytest.raises(SBMFError) as e:
        sbmf.load_libfm_meta(p, 4)
    assert e.value.code == SBMF_E_IO and "entry %d" % entry in str(e.value)


def test_meta_loader_refuses_a_missing_file_and_null_arguments(tmp_path):
    with pytest.raises(SBMFError) as e:
        sbmf.load_libfm_meta(tmp_path / "nothing", 2)
    assert e.value.code == SBMF_E_IO
    assert lib.sbmf_load_libfm_meta(None, 2, None, None) == SBMF_E_ARG
    assert lib.sbmf_load_libfm_meta(b"x", 2, None, None) == SBMF_E_ARG


# ---- the group calls' errors that need no context
def test_group_calls_refuse_a_null_context():
    g = np.zeros(3, np.uint32)
    r = np.zeros(1)
    assert lib.sbmf_set_attr_groups(None, 3, g.ctypes.data_as(C.POINTER(C.c_uint32))) == SBMF_E_ARG
    assert lib.sbmf_set_group_regular(None, 1, r.ctypes.data_as(C.POINTER(C.c_double)),
                                      r.ctypes.data_as(C.POINTER(C.c_double))) == SBMF_E_ARG
    assert lib.sbmf_get_fm_groups(None, None, None, None, None, None, None) == SBMF_E_ARG
    assert lib.sbmf_test_fm_group_sums(None, None) == SBMF_E_ARG
    assert b"null" in lib.sbmf_last_global_error()


# ---- -regular: Python
def test_parse_regular_forms():
    assert sbmf.parse_regular(()) == (0.0, 0.0, 0.0, None, None)
    assert sbmf.parse_regular((), 4) == (0.0, 0.0, 0.0, None, None)
    assert sbmf.parse_regular(2.5) == (2.5, 2.5, 2.5, None, None)
    assert sbmf.parse_regular((2.5,), 3) == (2.5, 2.5, 2.5, None, None)
    assert sbmf.parse_regular((0, 1, 10), 4) == (0.0, 1.0, 10.0, None, None)
    assert sbmf.parse_regular((0, 1, 2, 3, 4, 5, 10, 20, 30), 4) == (0.0, 0.0, 0.0, [1.0, 2.0, 3.0, 4.0],
                                                                     [5.0, 10.0, 20.0, 30.0])
    assert sbmf.parse_regular((7, 1, 2, 3, 4), 2) == (7.0, 0.0, 0.0, [1.0, 2.0], [3.0, 4.0])
    # one group: three values read either way give the same precisions
    assert sbmf.parse_regular((0.5, 1, 10), 1) == (0.5, 1.0, 10.0, None, None)


@pytest.mark.parametrize("values,G", [((0, 1), 1), ((0, 1, 2, 3, 4), 1), ((0, 1, 2, 3, 4), 3), ((0, 1, 2, 3), 2),
                                      ((0,) * 9, 3)])
def test_parse_regular_refuses_a_wrong_count(values, G):
    with pytest.raises(ValueError) as e:
        sbmf.parse_regular(values, G)
    assert "%d given" % len(values) in str(e.value)


def test_learner_keeps_the_group_form_of_regular_until_the_groups_are_known():
    L = sbmf.FMLearnSBPMF(num_factor=4, method="als", regular=(0.5, 1, 2, 3, 4))
    assert (L.cfg.reg0, L.cfg.regw, L.cfg.regv) == (0.0, 0.0, 0.0) and L.ctx is None
    M = sbmf.FMLearnSBPMF(num_factor=4, method="als", regular=(0.5, 1, 2))
    assert (M.cfg.reg0, M.cfg.regw, M.cfg.regv) == (0.5, 1.0, 2.0)


# ---- -regular: the command line parses it once the -meta groups are known and before the device is opened
FILES = {"train": "4 0:1 3:1\n3 1:1 4:1 5:0.5\n5 2:1 3:1\n", "test": "4 0:1 4:1\n", "meta": "0 0 0 1 1 2 2\n"}


def _cli(tmp_path, *extra):
    for nm, text in FILES.items():
        (tmp_path / nm).write_text(text)
    return subprocess.run([CLI_PATH, "-task", "r", "-train", "train", "-test", "test", "-method", "als", "-dim", "1,1,2",
                           "-iter", "1", *extra], capture_output=True, text=True, timeout=60, cwd=str(tmp_path))


@pytest.mark.parametrize("extra,count", [(["-regular", "0,1"], 2), (["-regular", "0,1,2,3,4"], 5),
                                         (["-meta", "meta", "-regular", "0,1,2,3,4"], 5),
                                         (["-meta", "meta", "-regular", "0,1,2,3,4,5,6,7"], 8)])
def test_cli_refuses_a_wrong_regular_count(tmp_path, extra, count):
    r = _cli(tmp_path, *extra)
    assert r.returncode == 1 and "-regular takes" in r.stderr and "%d given" % count in r.stderr
    if "-meta" in extra:
        assert "7 values" in r.stderr  # 1 + 2 * 3 groups


@pytest.mark.parametrize("extra", [[], ["-regular", "2"], ["-regular", "0,1,10"], ["-meta", "meta"],
                                   ["-meta", "meta", "-regular", "2"], ["-meta", "meta", "-regular", "0,1,10"],
                                   ["-meta", "meta", "-regular", "0,1,2,3,4,5,6"]])
def test_cli_accepts_the_regular_forms(tmp_path, extra):
    r = _cli(tmp_path, *extra)  # without a GPU the run ends at the device, past the parser
    assert "-regular takes" not in r.stderr and "-meta" not in r.stderr
    assert r.returncode == 0 or "no HIP device" in r.stderr


def test_cli_refuses_a_short_or_broken_meta_file(tmp_path):
    FILES2 = dict(FILES, meta="0 0 0 1\n")
    for nm, text in FILES2.items():
        (tmp_path / nm).write_text(text)
    r = subprocess.run([CLI_PATH, "-task", "r", "-train", "train", "-test", "test", "-method", "mcmc", "-meta", "meta"],
                       capture_output=True, text=True, timeout=60, cwd=str(tmp_path))
    assert r.returncode == 1 and "-meta" in r.stderr and "entry 5" in r.stderr and "7 attributes" in r.stderr


def test_help_says_where_meta_is_honoured():
    r = subprocess.run([CLI_PATH, "-help"], capture_output=True, text=True, timeout=60)
    line = [l for l in r.stdout.splitlines() if l.startswith("-meta")][0]
    assert "als" in line and "ignored by the SBPMF sampler" in line and "vb" in line
