"""libFM cases with any number of features, without a GPU: the text loader
(sbmf_load_libfm_cases) against a plain Python parse, the ranges of mutually exclusive
attributes (sbmf_fm_ranges), the new entry points at the ABI level, and the command line's
refusals of what only libFM's own chain is defined for."""
import ctypes as C
import re
import subprocess

import numpy as np
import pytest

import fm_cases
import sbmf
from conftest import REPO
from sbmf import Cases, FMLearnSBPMF, SBMFError, _lib
from sbmf._lib import CLI_PATH, SBMF_E_ARG, SBMF_E_IO


def _same(c, ptr, attr, x, y):
    return (np.array_equal(c.ptr, ptr) and np.array_equal(c.attr, attr) and c.x.dtype == np.float32 and
            np.array_equal(c.x, x) and np.array_equal(c.target, y))


# ---- loader
def test_loader_small_file_equals_python_parse(tmp_path):
    p = tmp_path / "small.libfm"
    p.write_text(fm_cases.SMALL_TEXT)
    c = sbmf.load_libfm_cases(p)
    ptr, attr, x, y = fm_cases.parse_text(fm_cases.SMALL_TEXT)
    assert c.num_cases == 12 and _same(c, ptr, attr, x, y)
    assert c.num_attr == int(attr.max()) + 1
    assert 0 in np.diff(c.ptr.astype(np.int64))  # the case without features
    # a last line without a newline, and a file of one case without features
    p.write_text(fm_cases.SMALL_TEXT.rstrip("\n"))
    assert _same(sbmf.load_libfm_cases(p), ptr, attr, x, y)
    p.write_text("2.5\n")
    c = sbmf.load_libfm_cases(p)
    assert c.num_cases == 1 and c.num_attr == 0 and len(c.attr) == 0


def test_loader_fm4_equals_python_parse(ml100k, tmp_path, monkeypatch):
    trf, tef = fm_cases.write_fm4(ml100k, tmp_path)
    tr, te = fm_cases.fm4(ml100k)[:2]
    monkeypatch.setenv("SBMF_LOAD_CHUNK", "65536")  # many chunks on several threads
    monkeypatch.setenv("SBMF_LOAD_THREADS", "7")
    for path, want in ((trf, tr), (tef, te)):
        c = sbmf.load_libfm_cases(path)
        assert _same(c, want.ptr, want.attr, want.x, want.target) and c.num_attr == want.num_attr
    ptr, attr, x, y = fm_cases.parse_text(open(tef).read())
    assert _same(te, ptr, attr, x, y)


def test_loader_values_parse_to_float32_of_the_text(tmp_path):
    vals = ["0.1", "0.333333", "1e-3", "2.5E2", "-0.7", "+3", "16777217", "0.30000001192092896", "1.17549435e-38", ".5",
            "123456.789", "3.4028234e38"]
    p = tmp_path / "v.libfm"
    p.write_text("".join("%s %d:%s\n" % (v, k, v) for k, v in enumerate(vals)))
    c = sbmf.load_libfm_cases(p)
    want = np.array([np.float32(v) for v in vals], np.float32)
    assert np.array_equal(c.x, want) and np.array_equal(c.target, want)


@pytest.mark.parametrize("text,code,msg", [
    ("4 1:1 2:1\n3 5:1 2:0.5 5:2\n", SBMF_E_ARG, "repeated"),
    ("4 1:1 x:1\n", SBMF_E_IO, "cannot parse"),
    ("4 1:1 2\n", SBMF_E_IO, "cannot parse"),
    ("abc 1:1\n", SBMF_E_IO, "cannot parse"),
    ("4 -1:1\n", SBMF_E_IO, "out of range"),
])
def test_loader_refusals_name_the_line(tmp_path, text, code, msg):
    p = tmp_path / "bad.libfm"
    p.write_text("# head\n5 0:1\n" + text)
    with pytest.raises(SBMFError) as e:
        sbmf.load_libfm_cases(p)
    bad = 3 + [k for k, l in enumerate(text.splitlines()) if l != "4 1:1 2:1"][0]
    assert e.value.code == code and msg in str(e.value) and "line %d of" % bad in str(e.value)


def test_binary_stem_with_other_rows_keeps_its_refusal_and_names_the_limit(tmp_path):
    """A .x whose rows are not {user, item}: the two-feature loaders refuse it as before, and say
    that general cases come from libFM text."""
    import struct
    stem = str(tmp_path / "g")
    with open(stem + ".x", "wb") as f:
        f.write(struct.pack("<IIQII", 2, 4, 3, 1, 6))
        f.write(struct.pack("<I", 3) + b"".join(struct.pack("<If", a, 1.0) for a in (0, 3, 5)))
    with open(stem + ".y", "wb") as f:
        f.write(struct.pack("<IIIf", 1, 4, 1, 4.0))
    with pytest.raises(SBMFError) as e:
        sbmf.load_libfm_binary(stem)
    assert "one user and one item" in str(e.value) and "libFM text only" in str(e.value)


# ---- ranges
def test_ranges_of_fm4_cut_at_the_field_edges_and_between_co_occurring_tags(ml100k):
    tr, te, _, _, (I, J, C0, D0) = fm_cases.fm4(ml100k)
    p = max(tr.num_attr, te.num_attr) + 1
    cnt = np.bincount(tr.attr, minlength=p)
    assert cnt[C0 + 3] == 0 and cnt[D0 + 5] == 0 and np.bincount(te.attr, minlength=p)[D0 + 5] > 0  # gap, test-only tag
    b = sbmf.fm_ranges(tr, p)
    assert b.tolist() == [0, I, C0, D0, D0 + 1, D0 + 2, D0 + 3, D0 + 4, p]
    assert sbmf.fm_ranges(tr).tolist()[:-1] == b.tolist()[:-1]  # the train set's own attribute count


def _check_partition(c, b, p):
    assert b[0] == 0 and b[-1] == p and np.all(np.diff(b.astype(np.int64)) > 0)
    rng = np.searchsorted(b, c.attr, side="right") - 1
    ptr = c.ptr.astype(np.int64)
    sets = [set(c.attr[ptr[k]:ptr[k + 1]].tolist()) for k in range(c.num_cases)]
    for k in range(c.num_cases):  # no case holds two attributes of one range
        r = rng[ptr[k]:ptr[k + 1]]
        assert len(set(r.tolist())) == len(r)
    for j in range(1, len(b) - 1):  # minimal: a range's first attribute conflicts with the range before it
        first, lo = int(b[j]), int(b[j - 1])
        assert any(first in s and any(lo <= a < first for a in s) for s in sets), (j, b)


def test_ranges_property_on_random_small_sets():
    rs = np.random.RandomState(20150)
    for trial in range(60):
        p = int(rs.randint(1, 24))
        n = int(rs.randint(0, 30))
        rows = []
        for _ in range(n):
            m = int(rs.randint(0, min(p, 5) + 1))
            rows.append((1.0, [(int(a), 1.0) for a in rs.choice(p, m, replace=False)]))
        c = fm_cases.rows_to_cases(rows) if n else Cases(np.zeros(1, np.uint64), [], [], [])
        _check_partition(c, sbmf.fm_ranges(c, p), p)
    c = Cases(np.zeros(1, np.uint64), [], [], [])
    assert sbmf.fm_ranges(c, 0).tolist() == [0] and sbmf.fm_ranges(c, 5).tolist() == [0, 5]


def test_ranges_argument_errors():
    c = fm_cases.rows_to_cases([(1.0, [(0, 1.0), (4, 1.0)]), (2.0, [(4, 1.0)])])
    with pytest.raises(SBMFError) as e:
        sbmf.fm_ranges(c, 3)  # attribute 4 >= num_attr
    assert e.value.code == SBMF_E_ARG
    cc, nr = c._c(), C.c_uint32()
    out = np.zeros(1, np.uint32)
    assert _lib.lib.sbmf_fm_ranges(C.byref(cc), 5, out.ctypes.data_as(C.POINTER(C.c_uint32)), 1, C.byref(nr)) == SBMF_E_ARG
    assert nr.value == 2  # sized even when bounds is too small


# ---- ABI
NEW = {
    "sbmf_load_libfm_cases": "int sbmf_load_libfm_cases(const char* path, sbmf_cases* out);",
    "sbmf_free_cases": "void sbmf_free_cases(sbmf_cases* c);",
    "sbmf_fm_ranges": "int sbmf_fm_ranges(const sbmf_cases* train, uint32_t num_attr, uint32_t* bounds, uint32_t cap, "
                      "uint32_t* nranges);",
    "sbmf_set_train_cases": "int sbmf_set_train_cases(sbmf_ctx* ctx, const sbmf_cases* cases);",
    "sbmf_set_test_cases": "int sbmf_set_test_cases(sbmf_ctx* ctx, const sbmf_cases* cases);",
    "sbmf_get_fm": "int sbmf_get_fm(sbmf_ctx* ctx, double* w0, double* w, double* v);",
    "sbmf_fm_info": "int sbmf_fm_info(sbmf_ctx* ctx, uint32_t* num_attr, uint32_t* nranges, uint32_t* launches_per_iter);",
}
CTYPE = {"sbmf_ctx*": C.c_void_p, "uint32_t": C.c_uint32, "uint32_t*": C.POINTER(C.c_uint32), "double*": C.POINTER(C.c_double),
         "const char*": C.c_char_p, "sbmf_cases*": C.POINTER(_lib.CasesC), "const sbmf_cases*": C.POINTER(_lib.CasesC)}


def test_symbols_resolve_with_the_header_signatures():
    header = re.sub(r"\s+", " ", open(REPO + "/include/sbmf.h").read())
    for name, proto in NEW.items():
        assert proto in header, name
        args = proto[proto.index("(") + 1:proto.rindex(")")].split(", ")
        want = [CTYPE[a.rsplit(" ", 1)[0]] for a in args]
        res, have = _lib.SIGNATURES[name]
        assert res is (None if proto.startswith("void") else C.c_int) and have == want, name
        fn = getattr(_lib.lib, name)
        assert list(fn.argtypes) == want


def test_cases_struct_layout_matches_the_header(tmp_path):
    src = tmp_path / "lay.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "sbmf.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu %zu %zu %zu\\n", sizeof(sbmf_cases), offsetof(sbmf_cases, n), '
                   "offsetof(sbmf_cases, nnz), offsetof(sbmf_cases, num_attr), offsetof(sbmf_cases, ptr), "
                   "offsetof(sbmf_cases, attr), offsetof(sbmf_cases, x), offsetof(sbmf_cases, target)); return 0; }\n")
    exe = str(tmp_path / "lay")
    subprocess.run(["cc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", REPO + "/include", str(src), "-o", exe], check=True)
    got = [int(t) for t in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    S = _lib.CasesC
    assert got == [C.sizeof(S)] + [getattr(S, f).offset for f in ("n", "nnz", "num_attr", "ptr", "attr", "x", "target")]


def test_header_compiles_as_c_and_abi_version_stays(tmp_path):
    src = tmp_path / "proto.c"
    src.write_text('#include "sbmf.h"\n'
                   "int (*a)(const char*, sbmf_cases*) = sbmf_load_libfm_cases;\n"
                   "void (*b)(sbmf_cases*) = sbmf_free_cases;\n"
                   "int (*c)(const sbmf_cases*, uint32_t, uint32_t*, uint32_t, uint32_t*) = sbmf_fm_ranges;\n"
                   "int (*d)(sbmf_ctx*, const sbmf_cases*) = sbmf_set_train_cases;\n"
                   "int (*e)(sbmf_ctx*, const sbmf_cases*) = sbmf_set_test_cases;\n"
                   "int (*f)(sbmf_ctx*, double*, double*, double*) = sbmf_get_fm;\n"
                   "int (*g)(sbmf_ctx*, uint32_t*, uint32_t*, uint32_t*) = sbmf_fm_info;\n"
                   "int v = SBMF_ABI_VERSION;\n")
    subprocess.run(["cc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", REPO + "/include", "-c", str(src), "-o",
                    str(tmp_path / "proto.o")], check=True)
    assert _lib.lib.sbmf_abi_version() == 2


def test_null_context_is_an_argument_error_and_python_methods_exist():
    lib = _lib.lib
    assert lib.sbmf_set_train_cases(None, None) == SBMF_E_ARG
    assert lib.sbmf_set_test_cases(None, None) == SBMF_E_ARG
    assert lib.sbmf_get_fm(None, None, None, None) == SBMF_E_ARG
    assert lib.sbmf_fm_info(None, None, None, None) == SBMF_E_ARG
    assert lib.sbmf_fm_ranges(None, 0, None, 0, None) == SBMF_E_ARG
    assert lib.sbmf_load_libfm_cases(None, None) == SBMF_E_ARG
    for m in ("fm", "fm_info"):
        assert callable(getattr(FMLearnSBPMF, m)), m
    assert callable(sbmf.load_libfm_cases) and callable(sbmf.fm_ranges)


# ---- command line: a general file is refused, before any learning, by what cannot read it
GENERAL = "5 0:1 3:1 6:0.5\n3 1:1 4:1\n4 2:1 4:1 6:1 7:0.25\n"


def run(*args):
    return subprocess.run([CLI_PATH, *args], capture_output=True, text=True, timeout=60)


@pytest.mark.parametrize("extra,why", [
    (["-method", "mcmc", "-order", "sbpmf", "-dim", "0,0,8"], "-order sbpmf"),
    (["-method", "vb"], "-method vb"),
    (["-method", "mcmc", "-order", "sbpmf", "-dim", "0,0,8", "-recommend", "out", "-rec_users", "users"], "-recommend"),
    (["-method", "mcmc", "-order", "sbpmf", "-dim", "0,0,8", "-recommend_guests", "out", "-rec_guests", "guests"],
     "-recommend"),
])
def test_cli_refuses_general_files_for_the_other_learners(tmp_path, extra, why):
    tr = tmp_path / "general.libfm"
    tr.write_text(GENERAL)
    r = run("-task", "r", "-train", str(tr), "-test", str(tr), "-iter", "2", *extra)
    assert r.returncode == 1 and "ERROR:" in r.stderr
    assert "not one user and one item feature" in r.stderr and why in r.stderr and "-method als" in r.stderr
    assert "#Iter" not in r.stdout and "HIP" not in r.stderr  # refused before the device is asked for


def test_cli_general_file_reaches_the_learner_for_mcmc_and_als(tmp_path):
    """-method mcmc (libFM order) and -method als accept the file: on a machine without a GPU the
    first failure is the device's, on one with a GPU the run prints its iterations."""
    tr = tmp_path / "general.libfm"
    tr.write_text(GENERAL)
    for method in ("mcmc", "als"):
        r = run("-task", "r", "-train", str(tr), "-test", str(tr), "-iter", "2", "-method", method)
        assert "one user and one item" not in r.stderr
        assert (r.returncode == 1 and "no HIP device" in r.stderr) or (r.returncode == 0 and "#Iter=  1" in r.stdout)
