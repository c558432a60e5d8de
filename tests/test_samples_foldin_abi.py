"""Guests folded into the sample store after the run (sbmf_get_sample_hyper ...
sbmf_samples_foldin_timing) at the ABI and command-line level, without a GPU: the symbols and their
ctypes signatures, the header as C, the unchanged ABI version, sbmf_samples_hyper_file_info on
hand-written companion files (one per named error), and the CLI's new flags as whole ERROR: lines."""
import ctypes as C
import re
import struct
import subprocess

import pytest

import sbmf
from conftest import REPO
from sbmf import _lib
from sbmf._lib import CLI_PATH

GUESTS = "sbmf_ctx* ctx, uint32_t n, const uint32_t* ptr, const uint32_t* items, const double* ratings, uint32_t scans"
NEW = {
    "sbmf_get_sample_hyper": "int sbmf_get_sample_hyper(sbmf_ctx* ctx, uint32_t s, double* hyper4k, double* tau);",
    "sbmf_save_samples_hyper": "int sbmf_save_samples_hyper(sbmf_ctx* ctx, const char* path);",
    "sbmf_load_samples_hyper": "int sbmf_load_samples_hyper(sbmf_ctx* ctx, const char* path);",
    "sbmf_samples_hyper_file_info": "int sbmf_samples_hyper_file_info(const char* path, uint32_t* version, "
                                    "uint32_t* num_factor, uint32_t* count, uint64_t* bytes);",
    "sbmf_samples_foldin_recommend": "int sbmf_samples_foldin_recommend(" + GUESTS + ", uint32_t topn, uint32_t flags, "
                                     "double risk, uint32_t* out_items, double* mean, double* stdev);",
    "sbmf_samples_foldin_rows": "int sbmf_samples_foldin_rows(" + GUESTS + ", double* rows);",
    "sbmf_samples_foldin_scores": "int sbmf_samples_foldin_scores(sbmf_ctx* ctx, uint32_t len, const uint32_t* items, "
                                  "const double* ratings, uint32_t scans, uint32_t flags, double* mean, double* stdev);",
    "sbmf_samples_foldin_timing": "int sbmf_samples_foldin_timing(sbmf_ctx* ctx, double* ms_draw, double* ms_score, "
                                  "double* ms_select);",
}
CTYPE = {"sbmf_ctx*": C.c_void_p, "uint32_t": C.c_uint32, "uint64_t": C.c_uint64, "double": C.c_double, "int": C.c_int,
         "const uint32_t*": C.POINTER(C.c_uint32), "uint32_t*": C.POINTER(C.c_uint32), "uint64_t*": C.POINTER(C.c_uint64),
         "double*": C.POINTER(C.c_double), "const double*": C.POINTER(C.c_double), "const char*": C.c_char_p}


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
        fn = getattr(_lib.lib, name)  # exported
        assert fn.restype is C.c_int and list(fn.argtypes) == want


def test_python_mirror_is_present():
    for name in ("sample_hyper", "save_samples_hyper", "load_samples_hyper", "samples_foldin_recommend",
                 "samples_foldin_rows", "samples_foldin_scores", "samples_foldin_timing"):
        assert callable(getattr(sbmf.FMLearnSBPMF, name)), name
    assert callable(sbmf.samples_hyper_file_info) and "samples_hyper_file_info" in sbmf.__all__


def test_null_context_is_an_argument_error():
    lib = _lib.lib
    assert lib.sbmf_get_sample_hyper(None, 0, None, None) == _lib.SBMF_E_ARG
    assert lib.sbmf_save_samples_hyper(None, b"x") == _lib.SBMF_E_ARG
    assert lib.sbmf_load_samples_hyper(None, b"x") == _lib.SBMF_E_ARG
    assert lib.sbmf_samples_hyper_file_info(None, None, None, None, None) == _lib.SBMF_E_ARG
    assert lib.sbmf_samples_foldin_recommend(None, 0, None, None, None, 1, 1, 0, 0.0, None, None, None) == _lib.SBMF_E_ARG
    assert lib.sbmf_samples_foldin_rows(None, 0, None, None, None, 1, None) == _lib.SBMF_E_ARG
    assert lib.sbmf_samples_foldin_scores(None, 0, None, None, 1, 0, None, None) == _lib.SBMF_E_ARG
    assert lib.sbmf_samples_foldin_timing(None, None, None, None) == _lib.SBMF_E_ARG


def test_header_compiles_as_c_and_abi_version_stays(tmp_path):
    src = tmp_path / "proto.c"
    src.write_text('#include "sbmf.h"\n'
                   "int (*a)(sbmf_ctx*, uint32_t, double*, double*) = sbmf_get_sample_hyper;\n"
                   "int (*b)(sbmf_ctx*, const char*) = sbmf_save_samples_hyper;\n"
                   "int (*c)(sbmf_ctx*, const char*) = sbmf_load_samples_hyper;\n"
                   "int (*d)(const char*, uint32_t*, uint32_t*, uint32_t*, uint64_t*) = sbmf_samples_hyper_file_info;\n"
                   "int (*e)(sbmf_ctx*, uint32_t, const uint32_t*, const uint32_t*, const double*, uint32_t, uint32_t, "
                   "uint32_t, double, uint32_t*, double*, double*) = sbmf_samples_foldin_recommend;\n"
                   "int (*f)(sbmf_ctx*, uint32_t, const uint32_t*, const uint32_t*, const double*, uint32_t, double*) "
                   "= sbmf_samples_foldin_rows;\n"
                   "int (*g)(sbmf_ctx*, uint32_t, const uint32_t*, const double*, uint32_t, uint32_t, double*, double*) "
                   "= sbmf_samples_foldin_scores;\n"
                   "int (*h)(sbmf_ctx*, double*, double*, double*) = sbmf_samples_foldin_timing;\n"
                   "int v = SBMF_ABI_VERSION;\n")
    subprocess.run(["cc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", REPO + "/include", "-c", str(src), "-o",
                    str(tmp_path / "proto.o")], check=True)
    assert _lib.lib.sbmf_abi_version() == 2


# ---- sbmf_samples_hyper_file_info on hand-written files (the format: INTEGRATION.md 3e)
MAGIC = b"SBMFSHP\n"


def hyper_file(version=1, K=4, count=2, reserved=0, magic=MAGIC):
    head = magic + struct.pack("<4I", version, K, count, reserved)
    return head + bytes(4 * count + 8 * count * (4 * K + 1))


def info_error(tmp_path, data):
    p = tmp_path / "h.bin"
    p.write_bytes(data)
    with pytest.raises(sbmf.SBMFError) as ei:
        sbmf.samples_hyper_file_info(p)
    assert ei.value.code == sbmf.SBMF_E_IO
    return str(ei.value)


@pytest.mark.parametrize("K,count", [(1, 1), (3, 4), (20, 2), (256, 1), (4, 0)])
def test_file_info_reads_a_good_file(tmp_path, K, count):
    p = tmp_path / "h.bin"
    data = hyper_file(K=K, count=count)
    p.write_bytes(data)
    assert len(data) == 24 + 4 * count + 8 * count * (4 * K + 1)
    assert sbmf.samples_hyper_file_info(p) == {"version": 1, "num_factor": K, "count": count, "bytes": len(data)}


def test_file_info_names_each_error(tmp_path):
    assert "bad magic" in info_error(tmp_path, hyper_file(magic=b"SBMFSMP\n"))  # a sample file's magic is not this one
    msg = info_error(tmp_path, hyper_file(version=2))
    assert "unknown format version 2" in msg and "reads version 1" in msg
    msg = info_error(tmp_path, hyper_file()[:23])
    assert "truncated in its header" in msg and "23 bytes" in msg and "header has 24" in msg
    good = hyper_file()
    msg = info_error(tmp_path, good[:-1])
    assert "truncated in its body" in msg and "%d bytes, its header implies %d" % (len(good) - 1, len(good)) in msg
    msg = info_error(tmp_path, good + b"\0\0\0")
    assert "3 trailing bytes" in msg and "its header implies %d" % len(good) in msg
    assert "bad header" in info_error(tmp_path, hyper_file(K=0))
    assert "bad header" in info_error(tmp_path, hyper_file(K=257))
    assert "bad header" in info_error(tmp_path, hyper_file(reserved=1))
    with pytest.raises(sbmf.SBMFError) as ei:
        sbmf.samples_hyper_file_info(tmp_path / "missing")
    assert ei.value.code == sbmf.SBMF_E_IO and "cannot open" in str(ei.value)


def test_file_info_whole_messages(tmp_path):
    """Every refusal of the header reader, the whole text (the sample file's: test_samples_abi.py)."""
    p, good = tmp_path / "h.bin", hyper_file()
    n = len(good)
    cases = [(good[:23], "is truncated in its header: 23 bytes, a sample hyperparameter file's header has 24"),
             (hyper_file(magic=b"SBMFSMP\n"), "is not a sample hyperparameter file (bad magic)"),
             (hyper_file(version=2), "has the unknown format version 2; this build reads version 1"),
             (hyper_file(K=257, count=65536, reserved=1), "has a bad header (K 257, count 65536, reserved 1)"),
             (good[:-1], "is truncated in its body: %d bytes, its header implies %d" % (n - 1, n)),
             (good + b"\0\0\0", "has 3 trailing bytes: %d bytes, its header implies %d" % (n + 3, n))]
    for data, text in cases:
        assert info_error(tmp_path, data) == "sbmf error -4: sbmf_samples_hyper_file_info: %s %s" % (p, text)
    with pytest.raises(sbmf.SBMFError) as ei:
        sbmf.samples_hyper_file_info(tmp_path / "missing")
    assert str(ei.value) == "sbmf error -4: sbmf_samples_hyper_file_info: cannot open %s" % (tmp_path / "missing")


# ---- the command line: decided by the flags alone, nothing opened
BASE = ("-task", "r", "-train", "/nonexistent/train", "-test", "/nonexistent/test")
SERVE = ("-samples_in", "f", "-samples_hyper_in", "h", "-samples_recommend_guests", "o", "-samples_guests", "g")
ROWS = [
    (("-samples_hyper_out", "x"), "ERROR: -samples_hyper_out goes with -samples_out <file>"),
    (("-samples_hyper_in", "x"), "ERROR: -samples_hyper_in goes with -samples_in <file>"),
    (("-samples_in", "f", "-samples_hyper_out", "x"), "ERROR: -samples_hyper_out goes with -samples_out <file>"),
    (("-samples_out", "f", "-samples_hyper_in", "x"), "ERROR: -samples_hyper_in goes with -samples_in <file>"),
    (("-samples_out", "f", "-samples_hyper_out"), "ERROR: -samples_hyper_out needs a file name"),
    (("-samples_in", "f", "-samples_hyper_in"), "ERROR: -samples_hyper_in needs a file name"),
    (("-samples_guests", "g"), "ERROR: -samples_guests goes with -samples_recommend_guests <file>"),
    (("-samples_in", "f", "-samples_hyper_in", "h", "-samples_guests", "g"),
     "ERROR: -samples_guests goes with -samples_recommend_guests <file>"),
    (("-samples_scans", "2"), "ERROR: -samples_scans goes with -samples_recommend_guests <file>"),
    (("-samples_recommend_guests", "o", "-samples_guests", "g"), "ERROR: -samples_recommend_guests goes with -samples_in <file>"),
    (("-samples_in", "f", "-samples_hyper_in", "h", "-samples_recommend_guests", "-samples_guests", "g"),
     "ERROR: -samples_recommend_guests needs a file name"),
    (("-samples_in", "f", "-samples_recommend_guests", "o", "-samples_guests", "g"),
     "ERROR: -samples_recommend_guests needs -samples_hyper_in <file> (the samples' hyperparameters, written by "
     "-samples_hyper_out)"),
    (("-samples_in", "f", "-samples_hyper_in", "h", "-samples_recommend_guests", "o"),
     "ERROR: -samples_recommend_guests needs -samples_guests <file> ('guest item rating' per line)"),
    ((*SERVE, "-samples_scans", "0"), "ERROR: -samples_scans must be in 1..64"),
    ((*SERVE, "-samples_scans", "65"), "ERROR: -samples_scans must be in 1..64"),
    ((*SERVE, "-rec_topn", "1025"), "ERROR: -rec_topn must be in 1..1024"),
    ((*SERVE, "-quirks", "bias2", "-dim", "1,1,8"),
     "ERROR: -samples_recommend_guests is offered for samples of the unbiased quirk sets (final, sbpmf2, none): a guest "
     "bias would need a draw of its own"),
]


@pytest.mark.parametrize("flags,line", ROWS, ids=[" ".join(f) for f, _ in ROWS])
def test_cli_refusals_are_whole_lines_with_nothing_opened(flags, line):
    r = run(*BASE, *flags)
    assert r.returncode == 1
    assert r.stderr.strip().splitlines() == [line]
    assert "open" not in r.stderr.lower() and "Loading" not in r.stdout


def test_existing_refusals_come_first():
    # the sample store's own refusal of an in-chain guest list, with the new flags beside it
    r = run(*BASE, *SERVE, "-recommend_guests", "g", "-rec_guests", "h")
    assert r.returncode == 1
    assert r.stderr.strip() == "ERROR: -samples_in runs no sweep: it does not go with -samples_out, -recommend_guests or -rlog"
    r = run(*BASE, "-samples_hyper_out", "x", "-recommend", "f")
    assert r.stderr.strip() == "ERROR: -recommend needs -rec_users <file> (one user id per line)"
    r = run(*BASE, "-samples_scans", "2", "-samples_every", "2")
    assert r.stderr.strip() == "ERROR: -samples_every / -samples_max go with -samples_out <file>"
    # -rec_topn without any list stays refused; with the guests' list from the samples it applies
    r = run(*BASE, "-rec_topn", "5")
    assert r.stderr.strip() == "ERROR: -rec_users / -rec_topn / -rec_risk go with -recommend"
    r = run(*BASE, *SERVE, "-rec_topn", "5", "-rec_risk", "0.5")
    assert r.returncode == 1 and "rec_topn" not in r.stderr  # gets as far as the (missing) train file


def test_help_lists_the_new_flags():
    r = run("-help")
    assert r.returncode == 0
    for flag in ("-samples_hyper_out", "-samples_hyper_in", "-samples_guests", "-samples_recommend_guests", "-samples_scans"):
        assert flag in r.stdout
