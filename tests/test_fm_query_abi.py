"""The libFM learner's query-list entry points (sbmf_fm_query_cases, sbmf_fm_query_scores,
sbmf_fm_query_recommend, sbmf_fm_query_timing) at the ABI and command-line level, without a GPU:
the prototypes and their ctypes signatures, the header as C, the unchanged ABI version, and the
CLI's -recommend_queries grammar beside the untouched messages of -recommend."""
import ctypes as C
import re
import subprocess

import pytest

from conftest import REPO
from sbmf import _lib
from sbmf._lib import CLI_PATH

NEW = {
    "sbmf_fm_query_cases": "int sbmf_fm_query_cases(sbmf_ctx* ctx, uint32_t relation, const sbmf_cases* queries, "
                           "const uint32_t* const* rows, const uint32_t* excl_ptr, const uint32_t* excl_rows, uint32_t flags);",
    "sbmf_fm_query_scores": "int sbmf_fm_query_scores(sbmf_ctx* ctx, uint32_t q, double* mean, double* stdev);",
    "sbmf_fm_query_recommend": "int sbmf_fm_query_recommend(sbmf_ctx* ctx, uint32_t topn, uint32_t flags, double risk, "
                               "uint32_t* rows, double* mean, double* stdev);",
    "sbmf_fm_query_timing": "int sbmf_fm_query_timing(sbmf_ctx* ctx, double* ms_terms, double* ms_score, double* ms_select);",
}
P_U32 = C.POINTER(C.c_uint32)
CTYPE = {"sbmf_ctx*": C.c_void_p, "uint32_t": C.c_uint32, "double": C.c_double, "const uint32_t*": P_U32,
         "uint32_t*": P_U32, "double*": C.POINTER(C.c_double), "const sbmf_cases*": C.POINTER(_lib.CasesC),
         "const uint32_t* const*": C.POINTER(P_U32)}


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
    assert _lib.lib.sbmf_fm_query_cases(None, 0, None, None, None, None, 0) == _lib.SBMF_E_ARG
    assert _lib.lib.sbmf_fm_query_scores(None, 0, None, None) == _lib.SBMF_E_ARG
    assert _lib.lib.sbmf_fm_query_recommend(None, 1, 0, 0.0, None, None, None) == _lib.SBMF_E_ARG
    assert _lib.lib.sbmf_fm_query_timing(None, None, None, None) == _lib.SBMF_E_ARG


def test_header_compiles_as_c_and_abi_version_stays(tmp_path):
    src = tmp_path / "proto.c"
    src.write_text('#include "sbmf.h"\n'
                   "int (*a)(sbmf_ctx*, uint32_t, const sbmf_cases*, const uint32_t* const*, const uint32_t*, "
                   "const uint32_t*, uint32_t) = sbmf_fm_query_cases;\n"
                   "int (*b)(sbmf_ctx*, uint32_t, double*, double*) = sbmf_fm_query_scores;\n"
                   "int (*c)(sbmf_ctx*, uint32_t, uint32_t, double, uint32_t*, double*, double*) = sbmf_fm_query_recommend;\n"
                   "int (*d)(sbmf_ctx*, double*, double*, double*) = sbmf_fm_query_timing;\n"
                   "int v = SBMF_ABI_VERSION;\n")
    subprocess.run(["cc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", REPO + "/include", "-c", str(src), "-o",
                    str(tmp_path / "proto.o")], check=True)
    assert _lib.lib.sbmf_abi_version() == 2


def test_header_points_from_the_watch_list_to_the_query_list():
    header = re.sub(r"[\s*]+", " ", open(REPO + "/include/sbmf.h").read())
    assert "the VB, libFM-MCMC and ALS learners (the libFM learners have a list of their own" in header
    for word in ("score(q, j) = ((w0 + a_q) + y_j)", "stdev reads back as exactly 0", "16 n nBp bytes", "chain is untouched"):
        assert word in header, word


def test_help_lists_the_query_flags():
    r = run("-help")
    assert r.returncode == 0
    for flag in ("-recommend_queries", "-rec_queries", "-rec_relation", "-rec_exclude"):
        assert flag in r.stdout


BASE = ("-task", "r", "-train", "/nonexistent/train", "-test", "/nonexistent/test")


@pytest.mark.parametrize("flag", ["-rec_queries", "-rec_relation", "-rec_exclude"])
def test_query_flags_go_with_recommend_queries(flag):
    r = run(*BASE, flag, "x")
    assert r.returncode == 1 and "go with -recommend_queries" in r.stderr and flag in r.stderr
    assert "open" not in r.stderr.lower()


def test_recommend_queries_needs_its_files():
    r = run(*BASE, "-recommend_queries", "f", "-method", "als", "-relation", "a")
    assert r.returncode == 1 and "-recommend_queries needs -rec_queries" in r.stderr
    r = run(*BASE, "-recommend_queries", "f", "-rec_queries", "q", "-method", "als", "-relation", "a")
    assert r.returncode == 1 and "-recommend_queries needs -rec_relation" in r.stderr


def test_rec_relation_names_a_relation_stem():
    r = run(*BASE, "-method", "als", "-relation", "relu,reli", "-recommend_queries", "f", "-rec_queries", "q",
            "-rec_relation", "items")
    assert r.returncode == 1 and "-rec_relation items names none of -relation's stems (relu,reli)" in r.stderr
    assert "open" not in r.stderr.lower()


@pytest.mark.parametrize("args", [("-method", "vb", "-relation", "a"), ("-method", "als")])
def test_recommend_queries_refused_without_the_libfm_learner_and_a_relation(args):
    r = run(*BASE, *args, "-recommend_queries", "f", "-rec_queries", "q", "-rec_relation", "a")
    assert r.returncode == 1
    assert "-recommend_queries is offered by libFM's MCMC / ALS learner" in r.stderr and "-relation" in r.stderr
    assert "open" not in r.stderr.lower()


def test_rec_topn_range_with_queries():
    r = run(*BASE, "-method", "als", "-relation", "a", "-recommend_queries", "f", "-rec_queries", "q", "-rec_relation", "a",
            "-rec_topn", "1025")
    assert r.returncode == 1 and "-rec_topn must be in 1..1024" in r.stderr


def test_the_old_messages_stay():
    for method in ("als", "vb"):
        r = run(*BASE, "-method", method, "-recommend", "f", "-rec_users", "/nonexistent/ids")
        assert r.returncode == 1 and "-recommend is offered by the SBPMF sampler (-method mcmc -order sbpmf)" in r.stderr
        r = run(*BASE, "-method", method, "-recommend_guests", "f", "-rec_guests", "/nonexistent/g")
        assert r.returncode == 1
        assert ("-recommend_guests is offered by the SBPMF sampler (-method mcmc -order sbpmf) with the unbiased quirk "
                "sets (final, sbpmf2, none)") in r.stderr
    r = run(*BASE, "-rec_topn", "3")
    assert r.returncode == 1 and "-rec_users / -rec_topn / -rec_risk go with -recommend" in r.stderr
    r = run(*BASE, "-rec_guests", "g")
    assert r.returncode == 1 and "-rec_guests goes with -recommend_guests <file>" in r.stderr
