"""The posterior sample store's entry points (sbmf_keep_samples ... sbmf_samples_file_info) at the
ABI and command-line level, without a GPU: the symbols and their ctypes signatures, the header
as C, the unchanged ABI version, sbmf_samples_file_info on hand-written files (one per named
error), and the CLI's -samples_* grammar as whole ERROR: lines."""
import ctypes as C
import re
import struct
import subprocess

import pytest

import sbmf
from conftest import REPO
from sbmf import _lib
from sbmf._lib import CLI_PATH

NEW = {
    "sbmf_keep_samples": "int sbmf_keep_samples(sbmf_ctx* ctx, uint32_t every, uint32_t cap);",
    "sbmf_samples_info": "int sbmf_samples_info(sbmf_ctx* ctx, uint32_t* count, uint32_t* cap, uint32_t* every, "
                         "uint64_t* bytes);",
    "sbmf_get_sample": "int sbmf_get_sample(sbmf_ctx* ctx, uint32_t s, uint32_t* sweep, double* U, double* V, double* bu, "
                       "double* bv, double* b0);",
    "sbmf_samples_recommend": "int sbmf_samples_recommend(sbmf_ctx* ctx, uint32_t n, const uint32_t* users, uint32_t topn, "
                              "uint32_t flags, double risk, uint32_t* items, double* mean, double* stdev);",
    "sbmf_samples_scores": "int sbmf_samples_scores(sbmf_ctx* ctx, uint32_t user, uint32_t flags, double* mean, "
                           "double* stdev);",
    "sbmf_samples_predict": "int sbmf_samples_predict(sbmf_ctx* ctx, uint64_t n, const uint32_t* users, "
                            "const uint32_t* items, uint32_t flags, double* mean, double* stdev);",
    "sbmf_samples_timing": "int sbmf_samples_timing(sbmf_ctx* ctx, double* ms_copy, double* ms_score, double* ms_select);",
    "sbmf_save_samples": "int sbmf_save_samples(sbmf_ctx* ctx, const char* path);",
    "sbmf_load_samples": "int sbmf_load_samples(sbmf_ctx* ctx, const char* path);",
    "sbmf_samples_file_info": "int sbmf_samples_file_info(const char* path, uint32_t* version, uint32_t* precision, "
                              "uint32_t* num_users, uint32_t* num_items, uint32_t* num_factor, uint32_t* count, "
                              "uint32_t* bias, uint64_t* bytes);",
    "sbmf_test_samples_lds": "int sbmf_test_samples_lds(uint32_t Kp, uint32_t* rows, uint64_t* bytes);",
    "sbmf_test_samples_tune": "int sbmf_test_samples_tune(sbmf_ctx* ctx, uint64_t budget_bytes, int unfused);",
}
CTYPE = {"sbmf_ctx*": C.c_void_p, "uint32_t": C.c_uint32, "uint64_t": C.c_uint64, "double": C.c_double, "int": C.c_int,
         "const uint32_t*": C.POINTER(C.c_uint32), "uint32_t*": C.POINTER(C.c_uint32), "uint64_t*": C.POINTER(C.c_uint64),
         "double*": C.POINTER(C.c_double), "const char*": C.c_char_p}


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


def test_null_context_is_an_argument_error():
    lib = _lib.lib
    assert lib.sbmf_keep_samples(None, 1, 4) == _lib.SBMF_E_ARG
    assert lib.sbmf_samples_info(None, None, None, None, None) == _lib.SBMF_E_ARG
    assert lib.sbmf_get_sample(None, 0, None, None, None, None, None, None) == _lib.SBMF_E_ARG
    assert lib.sbmf_samples_recommend(None, 0, None, 1, 0, 0.0, None, None, None) == _lib.SBMF_E_ARG
    assert lib.sbmf_samples_scores(None, 0, 0, None, None) == _lib.SBMF_E_ARG
    assert lib.sbmf_samples_predict(None, 0, None, None, 0, None, None) == _lib.SBMF_E_ARG
    assert lib.sbmf_samples_timing(None, None, None, None) == _lib.SBMF_E_ARG
    assert lib.sbmf_save_samples(None, b"x") == _lib.SBMF_E_ARG
    assert lib.sbmf_load_samples(None, b"x") == _lib.SBMF_E_ARG
    assert lib.sbmf_test_samples_tune(None, 0, 0) == _lib.SBMF_E_ARG
    assert lib.sbmf_samples_file_info(None, *[None] * 8) == _lib.SBMF_E_ARG


def test_header_compiles_as_c_and_abi_version_stays(tmp_path):
    src = tmp_path / "proto.c"
    src.write_text('#include "sbmf.h"\n'
                   "int (*a)(sbmf_ctx*, uint32_t, uint32_t) = sbmf_keep_samples;\n"
                   "int (*b)(sbmf_ctx*, uint32_t*, uint32_t*, uint32_t*, uint64_t*) = sbmf_samples_info;\n"
                   "int (*c)(sbmf_ctx*, uint32_t, uint32_t*, double*, double*, double*, double*, double*) = sbmf_get_sample;\n"
                   "int (*d)(sbmf_ctx*, uint32_t, const uint32_t*, uint32_t, uint32_t, double, uint32_t*, double*, double*) "
                   "= sbmf_samples_recommend;\n"
                   "int (*e)(sbmf_ctx*, uint32_t, uint32_t, double*, double*) = sbmf_samples_scores;\n"
                   "int (*f)(sbmf_ctx*, uint64_t, const uint32_t*, const uint32_t*, uint32_t, double*, double*) "
                   "= sbmf_samples_predict;\n"
                   "int (*g)(sbmf_ctx*, double*, double*, double*) = sbmf_samples_timing;\n"
                   "int (*h)(sbmf_ctx*, const char*) = sbmf_save_samples;\n"
                   "int (*i)(sbmf_ctx*, const char*) = sbmf_load_samples;\n"
                   "int (*j)(const char*, uint32_t*, uint32_t*, uint32_t*, uint32_t*, uint32_t*, uint32_t*, uint32_t*, "
                   "uint64_t*) = sbmf_samples_file_info;\n"
                   "int v = SBMF_ABI_VERSION;\n")
    subprocess.run(["cc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", REPO + "/include", "-c", str(src), "-o",
                    str(tmp_path / "proto.o")], check=True)
    assert _lib.lib.sbmf_abi_version() == 2


@pytest.mark.parametrize("Kp", range(16, 257, 16))
def test_scoring_launch_fits_the_lds(Kp):
    rows, nbytes = C.c_uint32(), C.c_uint64()
    assert _lib.lib.sbmf_test_samples_lds(Kp, C.byref(rows), C.byref(nbytes)) == 0
    assert rows.value in (16, 32, 64) and nbytes.value <= 64 * 1024
    assert nbytes.value == rows.value * ((Kp + 2) * 8 + 8 + 4)  # rows of Kp + 2 doubles, a bias and an id each


# ---- sbmf_samples_file_info on hand-written files (the format: INTEGRATION.md 3d)
MAGIC = b"SBMFSMP\n"


def sample_file(version=1, precision=0, I=3, J=2, K=4, count=2, bias=0, magic=MAGIC, body=None):
    head = magic + struct.pack("<8I", version, precision, I, J, K, count, bias, 0)
    ts = 4 if precision else 8
    size = count * 4 + count * ((I + J) * K * ts + (bias * (1 + I + J) * 8))
    return head + (bytes(size) if body is None else body)


def info_error(tmp_path, data):
    p = tmp_path / "s.bin"
    p.write_bytes(data)
    with pytest.raises(sbmf.SBMFError) as ei:
        sbmf.samples_file_info(p)
    assert ei.value.code == sbmf.SBMF_E_IO
    return str(ei.value)


@pytest.mark.parametrize("precision,bias", [(0, 0), (1, 0), (0, 1), (1, 1)])
def test_file_info_reads_a_good_file(tmp_path, precision, bias):
    p = tmp_path / "s.bin"
    data = sample_file(precision=precision, bias=bias, I=5, J=7, K=3, count=4)
    p.write_bytes(data)
    info = sbmf.samples_file_info(p)
    assert info == {"version": 1, "precision": "f32" if precision else "f64", "num_users": 5, "num_items": 7,
                    "num_factor": 3, "count": 4, "bias": bool(bias), "bytes": len(data)}
    ts = 4 if precision else 8
    assert len(data) == 40 + 4 * 4 + 4 * ((5 + 7) * 3 * ts + bias * (1 + 5 + 7) * 8)


def test_file_info_names_each_error(tmp_path):
    assert "bad magic" in info_error(tmp_path, sample_file(magic=b"SBMFSMQ\n"))
    msg = info_error(tmp_path, sample_file(version=2))
    assert "unknown format version 2" in msg and "reads version 1" in msg
    msg = info_error(tmp_path, sample_file()[:39])
    assert "truncated in its header" in msg and "39 bytes" in msg
    good = sample_file()
    msg = info_error(tmp_path, good[:-1])
    assert "truncated in its body" in msg and "%d bytes, its header implies %d" % (len(good) - 1, len(good)) in msg
    msg = info_error(tmp_path, good + b"\0\0\0")
    assert "3 trailing bytes" in msg and "its header implies %d" % len(good) in msg
    assert "bad header" in info_error(tmp_path, sample_file(precision=2))
    with pytest.raises(sbmf.SBMFError) as ei:
        sbmf.samples_file_info(tmp_path / "missing")
    assert ei.value.code == sbmf.SBMF_E_IO and "cannot open" in str(ei.value)


def test_file_info_whole_messages(tmp_path):
    """Every refusal of the header reader, the whole text (the companion file's: test_samples_foldin_abi.py)."""
    p, good = tmp_path / "s.bin", sample_file()
    n = len(good)
    cases = [(good[:39], "is truncated in its header: 39 bytes, a sample file's header has 40"),
             (sample_file(magic=b"SBMFSHP\n"), "is not a sample file (bad magic)"),
             (sample_file(version=2), "has the unknown format version 2; this build reads version 1"),
             (sample_file(precision=2, body=b""), "has a bad header (precision 2, bias 0, K 4, count 2)"),
             (sample_file(bias=2, K=257, count=65536, body=b""), "has a bad header (precision 0, bias 2, K 257, count 65536)"),
             (good[:-1], "is truncated in its body: %d bytes, its header implies %d" % (n - 1, n)),
             (good + b"\0\0\0", "has 3 trailing bytes: %d bytes, its header implies %d" % (n + 3, n))]
    for data, text in cases:
        assert info_error(tmp_path, data) == "sbmf error -4: sbmf_samples_file_info: %s %s" % (p, text)
    with pytest.raises(sbmf.SBMFError) as ei:
        sbmf.samples_file_info(tmp_path / "missing")
    assert str(ei.value) == "sbmf error -4: sbmf_samples_file_info: cannot open %s" % (tmp_path / "missing")


# ---- the command line: decided by the flags alone, nothing opened
BASE = ("-task", "r", "-train", "/nonexistent/train", "-test", "/nonexistent/test")
REFUSAL = "ERROR: -samples_out / -samples_in are offered by the SBPMF sampler (-method mcmc -order sbpmf)"
ROWS = [
    (("-samples_every", "2"), "ERROR: -samples_every / -samples_max go with -samples_out <file>"),
    (("-samples_max", "8"), "ERROR: -samples_every / -samples_max go with -samples_out <file>"),
    (("-samples_in", "f", "-samples_out", "g"),
     "ERROR: -samples_in runs no sweep: it does not go with -samples_out, -recommend_guests or -rlog"),
    (("-samples_in", "f", "-recommend_guests", "g", "-rec_guests", "h"),
     "ERROR: -samples_in runs no sweep: it does not go with -samples_out, -recommend_guests or -rlog"),
    (("-samples_in", "f", "-rlog", "g"),
     "ERROR: -samples_in runs no sweep: it does not go with -samples_out, -recommend_guests or -rlog"),
    (("-samples_out", "f", "-method", "als"), REFUSAL),
    (("-samples_out", "f", "-method", "vb"), REFUSAL),
    (("-samples_in", "f", "-method", "als"), REFUSAL),
    (("-samples_in", "f", "-method", "vb"), REFUSAL),
    (("-samples_out", "f", "-order", "libfm"), REFUSAL),
    (("-samples_in", "f", "-order", "libfm"), REFUSAL),
    (("-samples_out",), "ERROR: -samples_out needs a file name"),
    (("-samples_in",), "ERROR: -samples_in needs a file name"),
    (("-samples_out", "f", "-samples_every", "0"), "ERROR: -samples_every must be at least 1"),
    (("-samples_out", "f", "-samples_max", "65536"), "ERROR: -samples_max must be in 1..65535"),
]


@pytest.mark.parametrize("flags,line", ROWS, ids=[" ".join(f) for f, _ in ROWS])
def test_cli_refusals_are_whole_lines_with_nothing_opened(flags, line):
    r = run(*BASE, *flags)
    assert r.returncode == 1
    assert r.stderr.strip().splitlines() == [line]
    assert "open" not in r.stderr.lower() and "Loading" not in r.stdout


def test_existing_flag_checks_come_first():
    # an existing flags-only refusal wins over the new ones
    r = run(*BASE, "-samples_every", "2", "-recommend", "f")
    assert r.stderr.strip() == "ERROR: -recommend needs -rec_users <file> (one user id per line)"


def test_refused_for_the_libfm_order_of_libfm_input(tmp_path):
    tr = tmp_path / "train_libfm"
    tr.write_text("5 0:1 3:1\n3 1:1 4:1\n")  # libFM text: the default order is libfm
    r = run("-task", "r", "-train", str(tr), "-test", str(tr), "-samples_out", str(tmp_path / "s"))
    assert r.returncode == 1 and r.stderr.strip() == REFUSAL


def test_help_lists_the_sample_flags():
    r = run("-help")
    assert r.returncode == 0
    for flag in ("-samples_out", "-samples_every", "-samples_max", "-samples_in"):
        assert flag in r.stdout
