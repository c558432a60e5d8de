"""The watch-list entry points (sbmf_watch_users, sbmf_watch_scores, sbmf_recommend,
sbmf_watch_timing) at the ABI and command-line level, without a GPU: the symbols
and their ctypes signatures, the header as C, the unchanged ABI version, and the
CLI's -recommend grammar."""
import ctypes as C
import re
import subprocess

import pytest

from conftest import REPO
from sbmf import _lib
from sbmf._lib import CLI_PATH

NEW = {
    "sbmf_watch_users": "int sbmf_watch_users(sbmf_ctx* ctx, uint32_t n, const uint32_t* users, uint32_t flags);",
    "sbmf_watch_scores": "int sbmf_watch_scores(sbmf_ctx* ctx, uint32_t w, double* mean, double* stdev);",
    "sbmf_recommend": "int sbmf_recommend(sbmf_ctx* ctx, uint32_t topn, uint32_t flags, double risk, uint32_t* items, "
                      "double* mean, double* stdev);",
    "sbmf_watch_timing": "int sbmf_watch_timing(sbmf_ctx* ctx, double* ms_score, double* ms_select);",
}
CTYPE = {"sbmf_ctx*": C.c_void_p, "uint32_t": C.c_uint32, "double": C.c_double,
         "const uint32_t*": C.POINTER(C.c_uint32), "uint32_t*": C.POINTER(C.c_uint32), "double*": C.POINTER(C.c_double)}


def run(*args):
    return subprocess.run([CLI_PATH, *args], capture_output=True, text=True, timeout=60)


def test_symbols_resolve_with_the_lib_signatures():
    header = re.sub(r"\s+", " ", open(REPO + "/include/sbmf.h").read())
    for name, proto in NEW.items():
        assert proto in header, name  # the prototype the signature below is read from
        args = proto[proto.index("(") + 1:proto.rindex(")")].split(", ")
        want = [CTYPE[a.rsplit(" ", 1)[0]] for a in args]
        res, have = _lib.SIGNATURES[name]
        assert res is C.c_int and have == want, name
        fn = getattr(_lib.lib, name)
        assert fn.restype is C.c_int and list(fn.argtypes) == want


def test_null_context_is_an_argument_error():
    assert _lib.lib.sbmf_watch_users(None, 0, None, 0) == _lib.SBMF_E_ARG
    assert _lib.lib.sbmf_watch_scores(None, 0, None, None) == _lib.SBMF_E_ARG
    assert _lib.lib.sbmf_recommend(None, 1, 0, 0.0, None, None, None) == _lib.SBMF_E_ARG
    assert _lib.lib.sbmf_watch_timing(None, None, None) == _lib.SBMF_E_ARG


def test_header_compiles_as_c_and_abi_version_stays(tmp_path):
    src = tmp_path / "proto.c"
    src.write_text('#include "sbmf.h"\n'
                   "int (*a)(sbmf_ctx*, uint32_t, const uint32_t*, uint32_t) = sbmf_watch_users;\n"
                   "int (*b)(sbmf_ctx*, uint32_t, double*, double*) = sbmf_watch_scores;\n"
                   "int (*c)(sbmf_ctx*, uint32_t, uint32_t, double, uint32_t*, double*, double*) = sbmf_recommend;\n"
                   "int (*d)(sbmf_ctx*, double*, double*) = sbmf_watch_timing;\n"
                   "int v = SBMF_ABI_VERSION;\n")
    subprocess.run(["cc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", REPO + "/include", "-c", str(src), "-o",
                    str(tmp_path / "proto.o")], check=True)
    assert _lib.lib.sbmf_abi_version() == 2


def test_help_lists_the_recommend_flags():
    r = run("-help")
    assert r.returncode == 0
    for flag in ("-recommend", "-rec_users", "-rec_topn", "-rec_risk"):
        assert flag in r.stdout


def test_recommend_needs_rec_users():
    r = run("-task", "r", "-train", "a", "-test", "b", "-recommend", "f")
    assert r.returncode == 1 and "ERROR:" in r.stderr and "-rec_users" in r.stderr


@pytest.mark.parametrize("method", ["als", "vb"])
def test_recommend_refused_for_other_learners_before_any_file_is_opened(method):
    r = run("-task", "r", "-train", "/nonexistent/train", "-test", "/nonexistent/test", "-method", method,
            "-recommend", "f", "-rec_users", "/nonexistent/ids")
    assert r.returncode == 1
    assert "-recommend is offered by the SBPMF sampler (-method mcmc -order sbpmf)" in r.stderr
    assert "open" not in r.stderr.lower()


def test_recommend_refused_for_the_libfm_order(tmp_path):
    tr = tmp_path / "train_libfm"
    tr.write_text("5 0:1 3:1\n3 1:1 4:1\n")  # libFM text: the default order is libfm
    r = run("-task", "r", "-train", str(tr), "-test", str(tr), "-recommend", "f", "-rec_users", "/nonexistent/ids")
    assert r.returncode == 1
    assert "-recommend is offered by the SBPMF sampler (-method mcmc -order sbpmf)" in r.stderr


def test_rec_topn_range():
    r = run("-task", "r", "-train", "a", "-test", "b", "-recommend", "f", "-rec_users", "u", "-rec_topn", "1025")
    assert r.returncode == 1 and "-rec_topn" in r.stderr
