"""The online VB lists (sbmf_vb_get_posterior ... sbmf_vb_timing) at the ABI and command-line level,
without a GPU: the symbols and their ctypes signatures, the header as C, the unchanged ABI version,
the Python mirror, the new kernels' resource summary (no scratch, no spill), the scoring launch's
LDS by Kp, and the CLI's new flags as whole ERROR: lines decided by the flags alone."""
import ctypes as C
import os
import re
import subprocess

import pytest

import sbmf
from conftest import PKG, REPO
from sbmf import _lib
from sbmf._lib import CLI_PATH

GUESTS = "sbmf_ctx* ctx, uint32_t n, const uint32_t* ptr, const uint32_t* items, const double* ratings, uint32_t scans"
NEW = {
    "sbmf_vb_get_posterior": "int sbmf_vb_get_posterior(sbmf_ctx* ctx, double* U_mean, double* U_var, double* V_mean, "
                             "double* V_var, double* bu_mean, double* bu_var, double* bv_mean, double* bv_var, double* b0, "
                             "double* hyper);",
    "sbmf_vb_scores": "int sbmf_vb_scores(sbmf_ctx* ctx, uint32_t user, double* mean, double* stdev);",
    "sbmf_vb_recommend": "int sbmf_vb_recommend(sbmf_ctx* ctx, uint32_t n, const uint32_t* users, uint32_t topn, "
                         "uint32_t flags, double risk, uint32_t* items, double* mean, double* stdev);",
    "sbmf_vb_predict": "int sbmf_vb_predict(sbmf_ctx* ctx, uint64_t n, const uint32_t* users, const uint32_t* items, "
                       "double* mean, double* stdev);",
    "sbmf_vb_foldin_rows": "int sbmf_vb_foldin_rows(" + GUESTS + ", double* row_mean, double* row_var, double* b_mean, "
                           "double* b_var);",
    "sbmf_vb_foldin_scores": "int sbmf_vb_foldin_scores(sbmf_ctx* ctx, uint32_t len, const uint32_t* items, "
                             "const double* ratings, uint32_t scans, double* mean, double* stdev);",
    "sbmf_vb_foldin_recommend": "int sbmf_vb_foldin_recommend(" + GUESTS + ", uint32_t topn, uint32_t flags, double risk, "
                                "uint32_t* out_items, double* mean, double* stdev);",
    "sbmf_vb_save_posterior": "int sbmf_vb_save_posterior(sbmf_ctx* ctx, const char* path);",
    "sbmf_vb_load_posterior": "int sbmf_vb_load_posterior(sbmf_ctx* ctx, const char* path);",
    "sbmf_vb_posterior_file_info": "int sbmf_vb_posterior_file_info(const char* path, uint32_t* version, uint32_t* num_users, "
                                   "uint32_t* num_items, uint32_t* num_factor, uint64_t* bytes);",
    "sbmf_vb_timing": "int sbmf_vb_timing(sbmf_ctx* ctx, double* ms_transpose, double* ms_score, double* ms_select, "
                      "double* ms_guest);",
    "sbmf_test_vb_moments": "int sbmf_test_vb_moments(sbmf_ctx* ctx, uint32_t user, double* mean, double* var);",
    "sbmf_test_vb_tune": "int sbmf_test_vb_tune(sbmf_ctx* ctx, uint64_t budget_bytes);",
    "sbmf_test_vb_score_lds": "int sbmf_test_vb_score_lds(uint32_t Kp, uint32_t* rows, uint64_t* bytes);",
}
CTYPE = {"sbmf_ctx*": C.c_void_p, "uint32_t": C.c_uint32, "uint64_t": C.c_uint64, "double": C.c_double, "int": C.c_int,
         "const uint32_t*": C.POINTER(C.c_uint32), "uint32_t*": C.POINTER(C.c_uint32), "uint64_t*": C.POINTER(C.c_uint64),
         "double*": C.POINTER(C.c_double), "const double*": C.POINTER(C.c_double), "const char*": C.c_char_p}
C_NAME = {C.c_void_p: "sbmf_ctx*", C.c_uint32: "uint32_t", C.c_uint64: "uint64_t", C.c_double: "double"}


def run(*args):
    return subprocess.run([CLI_PATH, *args], capture_output=True, text=True, timeout=60)


def _args(proto):
    return proto[proto.index("(") + 1:proto.rindex(")")].split(", ")


def test_symbols_resolve_with_the_lib_signatures():
    header = re.sub(r"\s+", " ", open(REPO + "/include/sbmf.h").read())
    for name, proto in NEW.items():
        assert proto in header, name  # the prototype the signature below is read from
        want = [CTYPE[a.rsplit(" ", 1)[0]] for a in _args(proto)]
        res, have = _lib.SIGNATURES[name]
        assert res is C.c_int and have == want, name
        fn = getattr(_lib.lib, name)  # exported
        assert fn.restype is C.c_int and list(fn.argtypes) == want


def test_python_mirror_is_present():
    for name in ("vb_posterior", "vb_scores", "vb_recommend", "vb_predict", "vb_foldin_rows", "vb_foldin_scores",
                 "vb_foldin_recommend", "save_vb_posterior", "load_vb_posterior", "vb_timing"):
        assert callable(getattr(sbmf.FMLearnVBOnline, name)), name
    assert callable(sbmf.vb_posterior_file_info)


def test_null_context_is_an_argument_error():
    lib = _lib.lib
    assert lib.sbmf_vb_get_posterior(None, *([None] * 10)) == _lib.SBMF_E_ARG
    assert lib.sbmf_vb_scores(None, 0, None, None) == _lib.SBMF_E_ARG
    assert lib.sbmf_vb_recommend(None, 0, None, 1, 0, 0.0, None, None, None) == _lib.SBMF_E_ARG
    assert lib.sbmf_vb_predict(None, 0, None, None, None, None) == _lib.SBMF_E_ARG
    assert lib.sbmf_vb_foldin_rows(None, 0, None, None, None, 1, None, None, None, None) == _lib.SBMF_E_ARG
    assert lib.sbmf_vb_foldin_scores(None, 0, None, None, 1, None, None) == _lib.SBMF_E_ARG
    assert lib.sbmf_vb_foldin_recommend(None, 0, None, None, None, 1, 1, 0, 0.0, None, None, None) == _lib.SBMF_E_ARG
    assert lib.sbmf_vb_save_posterior(None, b"x") == _lib.SBMF_E_ARG
    assert lib.sbmf_vb_load_posterior(None, b"x") == _lib.SBMF_E_ARG
    assert lib.sbmf_vb_posterior_file_info(None, None, None, None, None, None) == _lib.SBMF_E_ARG
    assert lib.sbmf_vb_timing(None, None, None, None, None) == _lib.SBMF_E_ARG


def test_header_compiles_as_c_and_abi_version_stays(tmp_path):
    lines = ['#include "sbmf.h"']
    for k, (name, proto) in enumerate(NEW.items()):
        types = ", ".join(a.rsplit(" ", 1)[0] for a in _args(proto))
        lines.append("int (*f%d)(%s) = %s;" % (k, types, name))
    lines.append("int v = SBMF_ABI_VERSION;")
    src = tmp_path / "proto.c"
    src.write_text("\n".join(lines) + "\n")
    subprocess.run(["cc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", REPO + "/include", "-c", str(src), "-o",
                    str(tmp_path / "proto.o")], check=True)
    assert _lib.lib.sbmf_abi_version() == 2


def test_scoring_launch_lds_by_kp():
    """16 MU rows, three arrays of Kp + 2 doubles and the ids: MU 4 to Kp 32, 2 to Kp 80, then 1."""
    for Kp, rows in ((16, 64), (32, 64), (48, 32), (80, 32), (96, 16), (160, 16), (176, 16), (256, 16)):
        r, b = C.c_uint32(), C.c_uint64()
        assert _lib.lib.sbmf_test_vb_score_lds(Kp, C.byref(r), C.byref(b)) == 0
        assert r.value == rows and b.value == 3 * rows * (Kp + 2) * 8 + rows * 4, Kp
        assert b.value <= (65536 if Kp <= 160 else 160 * 1024), Kp


# ---- the kernels' resource summary (csrc/Makefile, the vb_lists_kernels.o rule): only the summary is read
FIELDS = r"(SGPRs Spill|VGPRs Spill|ScratchSize \[bytes/lane\]|VGPRs|AGPRs|LDS Size \[bytes/block\])"


def test_new_kernels_use_no_scratch_and_spill_nothing():
    res = os.path.join(PKG, "build", "vb_lists.resource.txt")
    if not os.path.exists(res):
        pytest.fail("%s is missing: rebuild csrc (make -C csrc clean all)" % res)
    kernels, cur = {}, None
    for line in open(res):
        m = re.search(r"remark: Function Name: \S*?(k_vb_[a-z]+)(ILi(\d)E)?", line)
        if m:
            cur = kernels.setdefault(m.group(1) + (m.group(3) or ""), {})
            continue
        m = re.search(r"remark:\s+" + FIELDS + r": (\d+)", line)
        if m and cur is not None:
            cur[m.group(1).split(" [")[0]] = int(m.group(2))
    assert set(kernels) == {"k_vb_score4", "k_vb_score2", "k_vb_score1", "k_vb_pairs", "k_vb_sd", "k_vb_guest"}
    for name, v in sorted(kernels.items()):
        print(name, v)
        assert v["ScratchSize"] == 0 and v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0, (name, v)
    assert kernels["k_vb_guest"]["LDS Size"] <= 65536
    assert kernels["k_vb_guest"]["VGPRs"] + kernels["k_vb_guest"]["AGPRs"] <= 128  # 16 waves a workgroup


# ---- the command line: decided by the flags alone, nothing opened
BASE = ("-task", "r", "-train", "/nonexistent/train", "-test", "/nonexistent/test")
VB = ("-method", "vb")
NOT_VB = "ERROR: -%s is offered by the online VB learner: use -method vb"
ROWS = [((f, "x"), NOT_VB % f[1:]) for f in ("-vb_recommend", "-vb_users", "-vb_recommend_guests", "-vb_guests", "-vb_topn",
                                             "-vb_risk", "-vb_scans", "-vb_model_out", "-vb_model_in")]
ROWS += [(("-method", "als", "-vb_model_out", "x"), NOT_VB % "vb_model_out"),
         (("-method", "mcmc", "-order", "libfm", "-vb_recommend", "o", "-vb_users", "u"), NOT_VB % "vb_recommend")]
ROWS += [
    ((*VB, "-vb_recommend"), "ERROR: -vb_recommend needs a file name"),
    ((*VB, "-vb_recommend", "o"), "ERROR: -vb_recommend needs -vb_users <file> (one user id per line)"),
    ((*VB, "-vb_users", "u"), "ERROR: -vb_users goes with -vb_recommend <file>"),
    ((*VB, "-vb_recommend_guests", "-vb_guests", "g"), "ERROR: -vb_recommend_guests needs a file name"),
    ((*VB, "-vb_recommend_guests", "o"), "ERROR: -vb_recommend_guests needs -vb_guests <file> ('guest item rating' per line)"),
    ((*VB, "-vb_guests", "g"), "ERROR: -vb_guests goes with -vb_recommend_guests <file>"),
    ((*VB, "-vb_scans", "2"), "ERROR: -vb_scans goes with -vb_recommend_guests <file>"),
    ((*VB, "-vb_recommend", "o", "-vb_users", "u", "-vb_scans", "2"), "ERROR: -vb_scans goes with -vb_recommend_guests <file>"),
    ((*VB, "-vb_topn", "5"), "ERROR: -vb_topn / -vb_risk go with -vb_recommend or -vb_recommend_guests"),
    ((*VB, "-vb_risk", "1"), "ERROR: -vb_topn / -vb_risk go with -vb_recommend or -vb_recommend_guests"),
    ((*VB, "-vb_recommend", "o", "-vb_users", "u", "-vb_topn", "0"), "ERROR: -vb_topn must be in 1..1024"),
    ((*VB, "-vb_recommend", "o", "-vb_users", "u", "-vb_topn", "1025"), "ERROR: -vb_topn must be in 1..1024"),
    ((*VB, "-vb_recommend_guests", "o", "-vb_guests", "g", "-vb_scans", "0"), "ERROR: -vb_scans must be in 1..64"),
    ((*VB, "-vb_recommend_guests", "o", "-vb_guests", "g", "-vb_scans", "65"), "ERROR: -vb_scans must be in 1..64"),
    ((*VB, "-vb_model_out"), "ERROR: -vb_model_out needs a file name"),
    ((*VB, "-vb_model_in"), "ERROR: -vb_model_in needs a file name"),
    ((*VB, "-vb_model_in", "a", "-vb_model_out", "b"), "ERROR: -vb_model_in runs no epoch: it does not go with -vb_model_out or -rlog"),
    ((*VB, "-vb_model_in", "a", "-rlog", "b"), "ERROR: -vb_model_in runs no epoch: it does not go with -vb_model_out or -rlog"),
]


@pytest.mark.parametrize("flags,line", ROWS, ids=[" ".join(f) for f, _ in ROWS])
def test_cli_refusals_are_whole_lines_with_nothing_opened(flags, line):
    r = run(*BASE, *flags)
    assert r.returncode == 1
    assert r.stderr.strip().splitlines() == [line]
    assert "open" not in r.stderr.lower() and "Loading" not in r.stdout


def test_existing_messages_of_method_vb_stay():
    r = run(*BASE, *VB, "-recommend", "f", "-rec_users", "u")
    assert r.stderr.strip() == "ERROR: -recommend is offered by the SBPMF sampler (-method mcmc -order sbpmf)"
    r = run(*BASE, *VB, "-recommend_guests", "f", "-rec_guests", "g")
    assert r.stderr.strip() == ("ERROR: -recommend_guests is offered by the SBPMF sampler (-method mcmc -order sbpmf) with "
                                "the unbiased quirk sets (final, sbpmf2, none)")
    r = run(*BASE, *VB, "-samples_out", "f")
    assert r.stderr.strip() == "ERROR: -samples_out / -samples_in are offered by the SBPMF sampler (-method mcmc -order sbpmf)"
    # the existing refusals come first, with the new flags beside them
    r = run(*BASE, *VB, "-rec_topn", "5", "-vb_model_out", "m")
    assert r.stderr.strip() == "ERROR: -rec_users / -rec_topn / -rec_risk go with -recommend"
    # a complete set of the new flags gets as far as the (missing) train file
    r = run(*BASE, *VB, "-vb_recommend", "o", "-vb_users", "u", "-vb_recommend_guests", "p", "-vb_guests", "g", "-vb_topn", "5",
            "-vb_risk", "0.5", "-vb_scans", "3", "-vb_model_out", "m")
    assert r.returncode == 1 and "vb_" not in r.stderr


def test_help_lists_the_new_flags():
    r = run("-help")
    assert r.returncode == 0
    for flag in ("-vb_recommend", "-vb_users", "-vb_recommend_guests", "-vb_guests", "-vb_topn", "-vb_risk", "-vb_scans",
                 "-vb_model_out", "-vb_model_in"):
        assert flag in r.stdout
