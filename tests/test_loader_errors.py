"""Every loader and writer of csrc/loader.cpp on the smallest files that reach each of its branches:
the return code, the whole text of sbmf_loader_error() and, where a call succeeds, the arrays it
loaded or the bytes it wrote.  No GPU is needed.

The return codes, messages and arrays are those of the library of the commit before loader.cpp was
rewritten around one reader per file format: every row here passed against that library (built from a
worktree of that commit, loaded through SBMF_LIB) before it was run against the new one.  Some rows
pin what that library does with a questionable input as it is (a libFM text id of 2^32 wraps to item
0 in sbmf_load_libfm): this file is about behaviour not moving.  The temporary directory inside a
message is replaced by <T> before comparing.  Every libFM text row runs with one thread and one chunk
and with eight threads and one-byte chunks, so the reported line is the file's."""
import ctypes as C
import os
import struct

import numpy as np
import pytest

from sbmf._lib import CasesC, Ratings, lib

OK, E_ARG, E_IO = 0, -1, -4
U32 = C.POINTER(C.c_uint32)


def f32(v):
    return float(np.float32(v))


# ---- the binary layouts, restated with struct (fmatrix.h:36-52, matrix.h:280-328)
def X(rows, num_cols, fid=2, fsize=4, nv=None):
    """a sparse matrix file from rows of (id, value)"""
    out = struct.pack("<IIQII", fid, fsize, sum(len(r) for r in rows) if nv is None else nv, len(rows), num_cols)
    for r in rows:
        out += struct.pack("<I", len(r)) + b"".join(struct.pack("<If", a, v) for a, v in r)
    return out


def Y(y, version=1, fsize=4, n=None):
    return struct.pack("<III", version, fsize, len(y) if n is None else n) + np.asarray(y, np.float32).tobytes()


def ones(cases):
    """rating cases (a list of feature ids each) as .x rows"""
    return [[(f, 1.0) for f in fs] for fs in cases]


def T(cases, nfeat):
    """... and as the rows of the transpose, one per feature"""
    return [[(c, 1.0) for c, fs in enumerate(cases) if f in fs] for f in range(nfeat)]


def DV(v, n=None):
    """a binary DVector<uint>"""
    return struct.pack("<III", 1, 4, len(v) if n is None else n) + np.asarray(v, np.uint32).tobytes()


PAIRS = [[0, 9], [1, 10]]  # two rating cases: users 0, 1 and items 0, 1 at offset 9
XV, XTV, YV = X(ones(PAIRS), 11), X(T(PAIRS, 11), 2), Y([4.0, 2.5])  # 64, 100 and 20 bytes
LOADED = ([0, 1], [0, 1], [4.0, 2.5])
OTHER = [[2, 12]]  # another set, to tell which of two pairs was read
XO, XTO, YO = X(ones(OTHER), 13), X(T(OTHER, 13), 1), Y([1.0])
LOADED_O = ([2], [3], [1.0])

NOT_X = "%s: not a libFM sparse matrix file (id 2, 4-byte values)"
NOT_Y = "<T>/s.y: not a libFM DVector<float> file (version 1, 4-byte values)"
TEXT_ONLY = "; cases with any other number of features are read from libFM text only (sbmf_load_libfm_cases)"
OFF = " (user id < item_offset <= item id)"


def bad_row(row, off=OFF):
    return "<T>/s.x row %d: the SBPMF sampler needs exactly one user and one item feature per row%s%s" % (row, off, TEXT_ONLY)


def bad_case(case, nf, off="; user id < item_offset <= item id)"):
    return ("<T>/s.xt case %d: the learners need exactly one user and one item feature per case (%d features%s%s"
            % (case, nf, off, TEXT_ONLY))


def row(id, call, files, rc, want, **kw):
    """want: the whole message of a failure; what a success loaded or wrote (None: not looked at)"""
    return dict(id=id, call=call, files=files, rc=rc, want=want, **kw)


def y_rows(name, ext):
    """the target file's faults, the same through either matrix"""
    call, x = (name, 9), {"s" + ext: XV if ext == ".x" else XTV}
    return [
        row(name + "_y_truncated_header", call, dict(x, **{"s.y": YV[:8]}), E_IO, "<T>/s.y: truncated header"),
        row(name + "_y_version", call, dict(x, **{"s.y": Y([4.0, 2.5], version=2)}), E_IO, NOT_Y),
        row(name + "_y_float_size", call, dict(x, **{"s.y": Y([4.0, 2.5], fsize=8)}), E_IO, NOT_Y),
        row(name + "_y_shorter_than_count", call, dict(x, **{"s.y": Y([4.0], n=2)}), E_IO, NOT_Y),
        row(name + "_truncated_header", call, {"s" + ext: XV[:20], "s.y": YV}, E_IO, "<T>/s%s: truncated header" % ext),
        row(name + "_wrong_id", call, {"s" + ext: X(ones(PAIRS), 11, fid=1), "s.y": YV}, E_IO, NOT_X % ("<T>/s" + ext)),
        row(name + "_float_size", call, {"s" + ext: X(ones(PAIRS), 11, fsize=8), "s.y": YV}, E_IO, NOT_X % ("<T>/s" + ext)),
    ]


def x_(cases, y=YV, tail=b"", **kw):
    return {"s.x": X(ones(cases), 11, **kw) + tail, "s.y": y}


def xt_(cases, y=YV, tail=b"", **kw):
    return {"s.xt": X(T(cases, 11), len(cases), **kw) + tail, "s.y": y}


BINARY = y_rows("binary", ".x") + y_rows("binary_t", ".xt") + [
    # ---- <stem>.x + <stem>.y
    row("x_missing_pair", ("binary", 9), {}, E_IO, "unable to open <T>/s.x/.y (or .data/.target)"),
    row("x_missing_y", ("binary", 9), {"s.x": XV}, E_IO, "unable to open <T>/s.x/.y (or .data/.target)"),
    row("x_rows_targets", ("binary", 9), x_(PAIRS, Y([4.0, 2.5, 1.0])), E_IO, "<T>/s.x: 2 rows but 3 targets"),
    row("x_truncated_in_size_word", ("binary", 9), {"s.x": XV[:46], "s.y": YV}, E_IO, "<T>/s.x: truncated at row 1"),
    row("x_truncated_in_entries", ("binary", 9), {"s.x": XV[:56], "s.y": YV}, E_IO, "<T>/s.x: truncated at row 1"),
    row("x_num_values_fixed_record_length", ("binary", 9), x_(PAIRS, nv=5), E_IO,
        "<T>/s.x: header says 5 values, rows hold 4"),
    row("x_num_values_other_length", ("binary", 9), x_(PAIRS, nv=5, tail=b"\0\0\0"), E_IO,
        "<T>/s.x: header says 5 values, rows hold 4"),
    row("x_one_feature", ("binary", 9), x_([[0], [1, 10]]), E_IO, bad_row(0)),
    row("x_three_features", ("binary", 0), x_([[0, 9], [1, 9, 10]]), E_IO, bad_row(1, "")),
    row("x_zero_features", ("binary", 9), x_([[], [1, 10]]), E_IO, bad_row(0)),
    row("x_item_below_offset", ("binary", 9), x_([[0, 9], [1, 8]]), E_IO, bad_row(1)),
    row("x_item_below_offset_scanned", ("binary", 9), x_([[0, 9], [1, 8]], tail=b"\0"), E_IO, bad_row(1)),
    row("x_user_at_offset", ("binary", 9), x_([[9, 10], [1, 10]]), E_IO, bad_row(0)),
    row("x_user_above_offset_0", ("binary", 0), x_([[9, 10], [1, 10]]), OK, ([9, 1], [10, 10], [4.0, 2.5])),
    row("x_bad_row_before_truncation", ("binary", 9), {"s.x": X(ones([[0], [1, 10]]), 11)[:40], "s.y": YV}, E_IO, bad_row(0)),
    row("x_empty_pair", ("binary", 9), {"s.x": X([], 0), "s.y": Y([])}, OK, ([], [], [])),
    row("x_valid", ("binary", 9), x_(PAIRS), OK, LOADED),
    row("x_valid_trailing_bytes_scanned", ("binary", 9), x_(PAIRS, tail=b"\0\0\0"), OK, LOADED),
    row("x_data_target_preferred", ("binary", 9), dict(x_(PAIRS), **{"s.data": XO, "s.target": YO}), OK, LOADED_O),
    row("x_data_without_target", ("binary", 9), dict(x_(PAIRS), **{"s.data": XO}), OK, LOADED),
    # ---- <stem>.xt + <stem>.y: 11 feature rows, the last one at byte 88
    row("xt_missing_pair", ("binary_t", 9), {}, E_IO, "unable to open <T>/s.xt/.y (or .datat/.target)"),
    row("xt_cases_targets", ("binary_t", 9), xt_(PAIRS, Y([4.0, 2.5, 1.0])), E_IO, "<T>/s.xt: 2 cases but 3 targets"),
    row("xt_truncated_in_size_word", ("binary_t", 9), {"s.xt": XTV[:90], "s.y": YV}, E_IO,
        "<T>/s.xt: truncated at feature row 10"),
    row("xt_truncated_in_entries", ("binary_t", 9), {"s.xt": XTV[:96], "s.y": YV}, E_IO,
        "<T>/s.xt: truncated at feature row 10"),
    row("xt_num_values", ("binary_t", 9), xt_(PAIRS, nv=5), E_IO, "<T>/s.xt: header says 5 values, rows hold 4"),
    row("xt_one_feature", ("binary_t", 9), xt_([[0, 9], [10]]), E_IO, bad_case(1, 1)),
    row("xt_three_features", ("binary_t", 0), xt_([[0, 1, 9], [1, 10]]), E_IO, bad_case(0, 3, ")")),
    row("xt_zero_features", ("binary_t", 9), xt_([[], [1, 10]]), E_IO, bad_case(0, 0)),
    row("xt_item_below_offset", ("binary_t", 9), xt_([[0, 9], [1, 8]]), E_IO, bad_case(1, 2)),
    row("xt_user_at_offset", ("binary_t", 9), xt_([[9, 10], [1, 10]]), E_IO, bad_case(0, 2)),
    row("xt_user_above_offset_0", ("binary_t", 0), xt_([[9, 10], [1, 10]]), OK, ([9, 1], [10, 10], [4.0, 2.5])),
    row("xt_case_id_past_targets", ("binary_t", 9), {"s.xt": X([[(0, 1.0)], [(2, 1.0)]] + T(PAIRS, 11)[2:], 2), "s.y": YV},
        E_IO, "<T>/s.xt feature row 1: case id past the 2 targets"),
    row("xt_empty_pair", ("binary_t", 9), {"s.xt": X([], 0), "s.y": Y([])}, OK, ([], [], [])),
    row("xt_valid", ("binary_t", 9), xt_(PAIRS), OK, LOADED),
    row("xt_valid_trailing_bytes", ("binary_t", 9), xt_(PAIRS, tail=b"\0\0\0"), OK, LOADED),
    row("xt_datat_target_preferred", ("binary_t", 9), dict(xt_(PAIRS), **{"s.datat": XTO, "s.target": YO}), OK, LOADED_O),
]

BOTH = {"s.data": XO, "s.datat": XTO, "s.target": YO, "s.x": XV, "s.xt": XTV, "s.y": YV}
OWN = {k: BOTH[k] for k in ("s.x", "s.xt", "s.y")}
KIND = [
    # ---- sbmf_libfm_binary_kind's four answers (the return code), and what sbmf_load_libfm_data reads then
    row("kind_1", ("kind", 1, 1), BOTH, 1, None),
    row("kind_1_transpose_alone", ("kind", 0, 1), {"s.datat": XTO, "s.target": YO}, 1, None),
    row("kind_2", ("kind", 1, 1), OWN, 2, None),
    row("kind_2_data_without_datat", ("kind", 1, 1), dict(OWN, **{"s.data": XO, "s.target": YO}), 2, None),
    row("kind_0", ("kind", 1, 1), {"s.x": XV, "s.xt": XTV}, 0, None),
    row("kind_no_orientation", ("kind", 0, 0), BOTH, E_ARG, None),
    row("data_kind_1_x", ("data", 1, 1, 9), BOTH, OK, LOADED_O),
    row("data_kind_1_xt", ("data", 0, 1, 9), dict(BOTH, **{"s.data": b"junk"}), OK, LOADED_O),
    row("data_kind_2_x", ("data", 1, 0, 9), dict(OWN, **{"s.xt": b"junk"}), OK, LOADED),
    row("data_kind_2_xt", ("data", 0, 1, 9), dict(OWN, **{"s.x": b"junk"}), OK, LOADED),
    row("data_kind_2_xt_faulty", ("data", 0, 1, 9), dict(OWN, **{"s.xt": XTV[:90]}), E_IO,
        "<T>/s.xt: truncated at feature row 10"),
    row("data_kind_0_text", ("data", 1, 1, 9), {"s": b"4 0:1 9:1\n2.5 1:1 10:1\n", "s.x": XV}, OK, LOADED),
    row("data_kind_0_nothing", ("data", 1, 1, 9), {"s.x": XV}, E_IO, "unable to open <T>/s"),
    row("data_no_orientation", ("data", 0, 0, 9), BOTH, E_ARG, None),
]

# ---- libFM text: two good lines, then the row's own; the same file through both text loaders
HEAD = b"5 0:1 3:1\n4 1:1 4:1\n"
HEAD_PAIRS = [(0, 3, 5.0), (1, 4, 4.0)]
HEAD_CASES = [(5.0, [(0, 1.0), (3, 1.0)]), (4.0, [(1, 1.0), (4, 1.0)])]
PARSE = "cannot parse libFM line %d of <T>/s"
PAIR = "the SBPMF sampler needs exactly one user and one item feature per line: libFM line %d of <T>/s"
PAIR_OFF = "the SBPMF sampler needs exactly one user and one item feature per line%s: libFM line %%d of <T>/s" % OFF
RANGE = "feature id out of range [0, 2^31) in libFM line %d of <T>/s"
REPEAT = "an attribute id is repeated inside one case (the learner writes one record per case of a row): line %d of <T>/s"


def text(id, tail, libfm, cases, offset=0):
    """libfm / cases: a message (E_IO), a (code, message), or the ratings / cases the tail adds to HEAD's"""
    return dict(id=id, tail=tail, libfm=libfm, cases=cases, offset=offset)


ONE = [(5.0, [(0, 1.0), (3, 1.0)])]
TEXT = [
    text("valid", b"", [], []),
    text("target", b"x 0:1 3:1\n", PARSE % 3, PARSE % 3),
    text("id_dash_value", b"5 0-1 3:1\n", PARSE % 3, PARSE % 3),
    text("missing_value", b"5 0:1 3:\n", PARSE % 3, PARSE % 3),
    text("missing_value_midline", b"5 0: 3:1\n", PARSE % 3, PARSE % 3),
    text("no_blank_between", b"5 0:1:1\n", PARSE % 3, PARSE % 3),
    text("negative_id", b"5 -1:1 3:1\n", PAIR % 3, RANGE % 3),
    text("id_2p31", b"5 0:1 2147483648:1\n", [(0, 2147483648, 5.0)], RANGE % 3),
    text("id_2p32", b"5 0:1 4294967296:1\n", [(0, 0, 5.0)], RANGE % 3),
    text("id_2p31_less_1", b"5 0:1 2147483647:1\n", [(0, 2147483647, 5.0)], [(5.0, [(0, 1.0), (2147483647, 1.0)])]),
    text("repeated_id", b"5 3:1 3:2\n", [(3, 3, 5.0)], (E_ARG, REPEAT % 3)),
    text("repeated_id_unsorted", b"5 3:1 0:1 3:2\n5 0:1 3:1\n", PAIR % 3, (E_ARG, REPEAT % 3)),
    text("unsorted_ids", b"5 3:1 0:2\n", [(3, 0, 5.0)], [(5.0, [(0, 2.0), (3, 1.0)])]),
    text("comment_after_features", b"5 0:1 3:1 # 7:1 x\n", [(0, 3, 5.0)], ONE),
    text("comment_after_target", b"5 # 0:1 3:1\n", PAIR % 3, [(5.0, [])]),
    text("crlf", b"5 0:1 3:1\r\n3 1:1 3:1\r\n", [(0, 3, 5.0), (1, 3, 3.0)], ONE + [(3.0, [(1, 1.0), (3, 1.0)])]),
    text("blank_lines", b"\n \t\n#c\n\r\n  5 0:1\t3:1  \n", [(0, 3, 5.0)], ONE),
    text("blank_lines_then_bad", b"\n \t\n#c\n\r\nx\n", PARSE % 7, PARSE % 7),
    text("bad_line_then_good", b"5 0:1 3\n5 0:1 3:1\n", PARSE % 3, PARSE % 3),
    text("two_bad_lines", b"5 0:1 3:1\n5 -1:1 3:1\nx\n", PAIR % 4, RANGE % 4),
    text("last_line_without_newline", b"5 0:1 3:1", [(0, 3, 5.0)], ONE),
    text("last_line_without_newline_bad", b"5 0:1 3", PARSE % 3, PARSE % 3),
    text("exponent", b"5e-1 0:1e0 3:2.5E1\n", [(0, 3, 0.5)], [(0.5, [(0, 1.0), (3, 25.0)])]),
    text("long_decimals", b"4.50000000000000000000001 0:0.3333333333333333333 3:1\n", [(0, 3, 4.5)],
         [(4.5, [(0, f32(1 / 3)), (3, 1.0)])]),
    text("one_feature", b"5 0:1\n", PAIR % 3, [(5.0, [(0, 1.0)])]),
    text("three_features", b"5 0:1 3:1 4:1\n", PAIR % 3, [(5.0, [(0, 1.0), (3, 1.0), (4, 1.0)])]),
    text("no_features", b"5\n", PAIR % 3, [(5.0, [])]),
    text("offset", b"5 2:1 3:1\n", [(2, 0, 5.0)], [(5.0, [(2, 1.0), (3, 1.0)])], offset=3),
    text("offset_item_below", b"5 0:1 2:1\n", PAIR_OFF % 3, [(5.0, [(0, 1.0), (2, 1.0)])], offset=3),
    text("offset_user_at", b"5 3:1 4:1\n", PAIR_OFF % 3, [(5.0, [(3, 1.0), (4, 1.0)])], offset=3),
]

# ---- -meta's group file
META = [
    row("meta_missing", ("meta", 3), {}, E_IO, "unable to open <T>/g"),
    row("meta_too_few", ("meta", 3), {"g": b"0 1\n"}, E_IO,
        "<T>/g holds 2 group ids; 3 attributes need one each (entry 3 is missing)"),
    row("meta_empty", ("meta", 3), {"g": b""}, E_IO, "<T>/g holds 0 group ids; 3 attributes need one each (entry 1 is missing)"),
    row("meta_not_a_number", ("meta", 3), {"g": b"0 x 1\n"}, E_IO, "<T>/g: entry 2 is not a group id (an unsigned integer)"),
    row("meta_number_then_letters", ("meta", 3), {"g": b"0 1x 1\n"}, E_IO,
        "<T>/g: entry 2 is not a group id (an unsigned integer)"),
    row("meta_negative", ("meta", 3), {"g": b"-1 0 1\n"}, E_IO, "<T>/g: entry 1 is not a group id (an unsigned integer)"),
    row("meta_2p32_less_1", ("meta", 3), {"g": b"0 1 4294967295"}, E_IO, "<T>/g: entry 3 is not a group id (an unsigned integer)"),
    row("meta_2p32_less_2", ("meta", 3), {"g": b"0 1 4294967294"}, OK, ([0, 1, 4294967294], 4294967295)),
    row("meta_leading_zeros", ("meta", 1), {"g": b"00000000000000000000000000007"}, OK, ([7], 8)),
    row("meta_many_digits", ("meta", 1), {"g": b"99999999999999999999"}, E_IO,
        "<T>/g: entry 1 is not a group id (an unsigned integer)"),
    row("meta_extra_entries_ignored", ("meta", 3), {"g": b"0\t1\r\n\f1\v7 junk"}, OK, ([0, 1, 1], 2)),
    row("meta_num_attr_0", ("meta", 0), {"g": b"junk"}, OK, ([], 0)),
]

# ---- a relation: three block rows {0: 1.5, 2: 2.5}, {1: 3.5}, {} over three attributes
BLOCK_ROWS = [[(0, 1.5), (2, 2.5)], [(1, 3.5)], []]
BLOCK = dict(n=3, nnz=3, num_attr=3, ptr=[0, 2, 3, 3], attr=[0, 2, 1], x=[1.5, 2.5, 3.5])
BX = X(BLOCK_ROWS, 3)  # 24 + 20 + 12 + 4 bytes
BXT = X([[(0, 1.5)], [(1, 3.5)], [(0, 2.5)]], 3)  # by attribute, as transpose.cpp writes it
MAPS = {"s.train": b"0 1\n2\n", "s.test": DV([2, 0])}
REL = dict(block=BLOCK, train=[0, 1, 2], test=[2, 0], group=None, G=0)


def rel(id, files, rc, want):
    return row(id, ("relation",), files, rc, want)


RELATION = [
    rel("rel_neither", MAPS, E_IO, "unable to open <T>/s.xt (or .x)"),
    rel("rel_x", dict(MAPS, **{"s.x": BX}), OK, REL),
    rel("rel_xt_transposed_back", dict(MAPS, **{"s.xt": BXT}), OK, REL),
    rel("rel_xt_preferred", dict(MAPS, **{"s.xt": BXT, "s.x": b"junk"}), OK, REL),
    rel("rel_xt_more_columns", dict(MAPS, **{"s.xt": X([[(0, 1.5)], [(1, 3.5)], [(0, 2.5)]], 4)}), OK,
        dict(REL, block=dict(BLOCK, n=4, ptr=[0, 2, 3, 3, 3]))),
    rel("rel_truncated_header", dict(MAPS, **{"s.x": BX[:23]}), E_IO, "<T>/s.x: truncated header"),
    rel("rel_wrong_id", dict(MAPS, **{"s.xt": X(BLOCK_ROWS, 3, fid=3)}), E_IO, NOT_X % "<T>/s.xt"),
    rel("rel_float_size", dict(MAPS, **{"s.x": X(BLOCK_ROWS, 3, fsize=8)}), E_IO, NOT_X % "<T>/s.x"),
    rel("rel_id_past_columns", dict(MAPS, **{"s.x": X(BLOCK_ROWS, 2)}), E_IO,
        "<T>/s.x row 0: entry 1 has id 2; the file has 2 columns"),
    rel("rel_num_values", dict(MAPS, **{"s.x": X(BLOCK_ROWS, 3, nv=5)}), E_IO, "<T>/s.x: 3 entries read, the header says 5"),
    rel("rel_truncated_in_size_word", dict(MAPS, **{"s.x": BX[:58]}), E_IO, "<T>/s.x: truncated at row 2"),
    rel("rel_truncated_in_entries", dict(MAPS, **{"s.x": BX[:50]}), E_IO, "<T>/s.x: truncated at row 1"),
    rel("rel_trailing_bytes", dict(MAPS, **{"s.x": BX + b"\0\0"}), OK, REL),
    rel("rel_empty_block", dict(MAPS, **{"s.x": X([], 0), "s.train": b"", "s.test": DV([])}), OK,
        dict(block=dict(n=0, nnz=0, num_attr=0, ptr=[0], attr=[], x=[]), train=[], test=[], group=None, G=0)),
    rel("rel_train_missing", {"s.x": BX, "s.test": b"0"}, E_IO, "unable to open <T>/s.train"),
    rel("rel_test_missing", {"s.x": BX, "s.train": b"0"}, E_IO, "unable to open <T>/s.test"),
    rel("rel_map_binary_truncated", dict(MAPS, **{"s.x": BX, "s.train": DV([0, 1, 2], n=5)}), E_IO,
        "<T>/s.train: a binary DVector<uint> of 5 entries, truncated"),
    rel("rel_map_binary_header_alone", dict(MAPS, **{"s.x": BX, "s.test": DV([])[:8]}), E_IO,
        "<T>/s.test: a binary DVector<uint> of 0 entries, truncated"),
    rel("rel_map_text_bad_entry", dict(MAPS, **{"s.x": BX, "s.test": b"0 x 1\n"}), E_IO,
        "<T>/s.test: entry 2 is not a block-row index (an unsigned integer)"),
    rel("rel_map_text_2p32_less_1", dict(MAPS, **{"s.x": BX, "s.train": b"0\n4294967295\n"}), E_IO,
        "<T>/s.train: entry 2 is not a block-row index (an unsigned integer)"),
    rel("rel_groups", dict(MAPS, **{"s.x": BX, "s.groups": b"0 1 1\n"}), OK, dict(REL, group=[0, 1, 1], G=2)),
    rel("rel_groups_too_few", dict(MAPS, **{"s.xt": BXT, "s.groups": b"0 1\n"}), E_IO,
        "<T>/s.groups holds 2 group ids; 3 attributes need one each (entry 3 is missing)"),
]

# ---- the writers: what lies in the directory after the call
DATA = ([0, 1], [0, 1], [4.0, 2.5])  # PAIRS at item_offset 9
WRAP = "feature id past UINT32_MAX - 1 (item_offset + item id): not representable in the %s format"
SAVE = [
    row("save_triples", ("save_triples", DATA), {}, OK, {"s": b"0\t0\t4\n1\t1\t2.5\n"}),
    row("save_triples_numbers", ("save_triples", ([7], [4294967295], [-0.1])), {}, OK,
        {"s": b"7\t4294967295\t-0.10000000000000001\n"}),
    row("save_binary", ("save_binary", DATA, 9, 0), {}, OK, {"s.x": XV, "s.y": YV}),
    row("save_binary_num_cols", ("save_binary", DATA, 9, 13), {}, OK, {"s.x": X(ones(PAIRS), 13), "s.y": YV}),
    row("save_binary_t", ("save_binary_t", DATA, 9, 0), {}, OK, {"s.xt": XTV, "s.y": YV}),
    row("save_binary_empty", ("save_binary", ([], [], []), 9, 0), {}, OK, {"s.x": X([], 0), "s.y": Y([])}),
    row("save_binary_t_empty", ("save_binary_t", ([], [], []), 9, 2), {}, OK, {"s.xt": X([[], []], 0), "s.y": Y([])}),
    row("save_block", ("save_block", BLOCK), {}, OK, {"s": BX}),
    row("save_row_map_text", ("save_row_map", [2, 0, 4294967295], 0), {}, OK, {"s": b"2\n0\n4294967295\n"}),
    row("save_row_map_binary", ("save_row_map", [2, 0], 1), {}, OK, {"s": DV([2, 0])}),
    row("save_row_map_binary_empty", ("save_row_map", [], 1), {}, OK, {"s": DV([])}),
    row("save_triples_unwritable", ("save_triples", DATA), {}, E_IO, "unable to write <T>/none/s", stem="none/s"),
    row("save_binary_unwritable", ("save_binary", DATA, 9, 0), {}, E_IO, "unable to write <T>/none/s.x/.y", stem="none/s"),
    row("save_binary_t_unwritable", ("save_binary_t", DATA, 9, 0), {}, E_IO, "unable to write <T>/none/s.xt/.y",
        stem="none/s"),
    row("save_block_unwritable", ("save_block", BLOCK), {}, E_IO, "unable to open <T>/none/s for writing", stem="none/s"),
    row("save_row_map_unwritable", ("save_row_map", [2, 0], 0), {}, E_IO, "unable to open <T>/none/s for writing",
        stem="none/s"),
    row("save_binary_item_wraps", ("save_binary", ([0], [1], [4.0]), 4294967295, 0), {}, E_ARG, WRAP % ".x"),
    row("save_binary_t_item_wraps", ("save_binary_t", ([0], [1], [4.0]), 4294967295, 0), {}, E_ARG, WRAP % ".xt"),
    row("save_binary_user_wraps", ("save_binary", ([4294967295], [0], [4.0]), 0, 0), {}, E_ARG, WRAP % ".x"),
    row("save_binary_largest_id", ("save_binary", ([0], [4294967285], [4.0]), 9, 0), {}, OK,
        {"s.x": X([[(0, 1.0), (4294967294, 1.0)]], 4294967295), "s.y": Y([4.0])}),
    row("save_binary_t_ids_coincide", ("save_binary_t", ([0, 9], [0, 0], [4.0, 2.5]), 9, 0), {}, E_ARG,
        "case 1: user and item feature ids coincide"),
]


# ---- one call, and what it left, as plain Python data
def ratings(u, i, r):
    d = Ratings()
    keep = [np.asarray(u, np.uint32), np.asarray(i, np.uint32), np.asarray(r, np.float64)]
    d.n = len(keep[0])
    d.user, d.item, d.rating = keep[0].ctypes.data_as(U32), keep[1].ctypes.data_as(U32), keep[2].ctypes.data_as(
        C.POINTER(C.c_double))
    return d, keep


def cases_struct(b):
    d = CasesC()
    keep = [np.asarray(b["ptr"], np.uint64), np.asarray(b["attr"], np.uint32), np.asarray(b["x"], np.float32)]
    d.n, d.nnz, d.num_attr = b["n"], b["nnz"], b["num_attr"]
    d.ptr, d.attr, d.x = (keep[0].ctypes.data_as(C.POINTER(C.c_uint64)), keep[1].ctypes.data_as(U32),
                          keep[2].ctypes.data_as(C.POINTER(C.c_float)))
    return d, keep


def loaded_ratings(rc, d):
    if rc != OK:  # zeroed before anything is read, freed after
        assert (d.n, bool(d.user), bool(d.item), bool(d.rating)) == (0, False, False, False)
        return None
    out = (d.user[:d.n], d.item[:d.n], d.rating[:d.n])
    lib.sbmf_free_ratings(C.byref(d))
    return out


def loaded_cases(rc, d):
    if rc != OK:
        assert (d.n, d.nnz, d.num_attr, bool(d.ptr), bool(d.attr), bool(d.x), bool(d.target)) == (0, 0, 0) + (False,) * 4
        return None
    out = dict(n=d.n, nnz=d.nnz, num_attr=d.num_attr, ptr=d.ptr[:d.n + 1], attr=d.attr[:d.nnz], x=d.x[:d.nnz],
               target=d.target[:d.n])
    lib.sbmf_free_cases(C.byref(d))
    return out


def run(tmp, name, *args, stem="s"):
    stem = os.path.join(str(tmp), stem).encode()
    if name in ("binary", "binary_t", "libfm", "data"):
        d = Ratings()
        fn = {"binary": lib.sbmf_load_libfm_binary, "binary_t": lib.sbmf_load_libfm_binary_t, "libfm": lib.sbmf_load_libfm,
              "data": lib.sbmf_load_libfm_data}[name]
        rc = fn(stem, *args, C.byref(d))
        return rc, loaded_ratings(rc, d)
    if name == "kind":
        return lib.sbmf_libfm_binary_kind(stem, *args), None
    if name == "cases":
        d = CasesC()
        rc = lib.sbmf_load_libfm_cases(stem, C.byref(d))
        return rc, loaded_cases(rc, d)
    if name == "meta":
        group, G = (C.c_uint32 * max(args[0], 1))(), C.c_uint32(77)
        rc = lib.sbmf_load_libfm_meta(os.path.join(str(tmp), "g").encode(), args[0], group, C.byref(G))
        return rc, (group[:args[0]], G.value) if rc == OK else None
    if name == "relation":
        d, tr, te, gr = CasesC(), U32(), U32(), U32()
        ntr, nte, G = C.c_uint64(77), C.c_uint64(77), C.c_uint32(77)
        rc = lib.sbmf_load_libfm_relation(stem, C.byref(d), C.byref(tr), C.byref(ntr), C.byref(te), C.byref(nte),
                                          C.byref(gr), C.byref(G))
        if rc != OK:  # nothing is left to free
            assert not (bool(d.ptr) or bool(d.attr) or bool(d.x) or bool(d.target) or bool(tr) or bool(te) or bool(gr))
            return rc, None
        assert d.target[:d.n] == [0.0] * d.n
        out = dict(block=dict(n=d.n, nnz=d.nnz, num_attr=d.num_attr, ptr=d.ptr[:d.n + 1], attr=d.attr[:d.nnz], x=d.x[:d.nnz]),
                   train=tr[:ntr.value], test=te[:nte.value], group=gr[:d.num_attr] if gr else None, G=G.value)
        lib.sbmf_free_relation(C.byref(d), C.byref(tr), C.byref(te), C.byref(gr))
        return rc, out
    before = set(os.listdir(str(tmp)))
    if name == "save_block":
        d, keep = cases_struct(args[0])
        rc = lib.sbmf_save_libfm_block(stem, C.byref(d))
    elif name == "save_row_map":
        keep = np.asarray(args[0], np.uint32)
        rc = lib.sbmf_save_libfm_row_map(stem, keep.ctypes.data_as(U32), len(keep), args[1])
    else:
        d, keep = ratings(*args[0])
        fn = {"save_triples": lib.sbmf_save_triples, "save_binary": lib.sbmf_save_libfm_binary,
              "save_binary_t": lib.sbmf_save_libfm_binary_t}[name]
        rc = fn(stem, C.byref(d), *args[1:])
    wrote = {f: open(os.path.join(str(tmp), f), "rb").read() for f in set(os.listdir(str(tmp))) - before}
    return rc, wrote


def check(tmp, r, call=None, rc=None, want=None):
    call, rc, want = call or r["call"], r["rc"] if rc is None else rc, r["want"] if want is None else want
    for name, data in r.get("files", {}).items():
        (tmp / name).write_bytes(data)
    got_rc, got = run(tmp, *call, stem=r.get("stem", "s"))
    assert got_rc == rc, lib.sbmf_loader_error().decode()
    if rc in (OK, 1, 2):
        assert want is None or got == want
    elif want is not None:
        assert lib.sbmf_loader_error().decode().replace(str(tmp), "<T>") == want
        assert got in (None, {})  # a writer that fails leaves no file


@pytest.mark.parametrize("r", BINARY + KIND + META + RELATION + SAVE, ids=lambda r: r["id"])
def test_row(tmp_path, r):
    check(tmp_path, r)


def text_want(loader, r):
    """the row's expectation for one text loader as (rc, want)"""
    e = r[loader]
    if isinstance(e, str):
        return E_IO, e
    if isinstance(e, tuple):
        return e
    if loader == "libfm":
        t = [(u, i - r["offset"], y) for u, i, y in HEAD_PAIRS] + e
        return OK, tuple([list(c) for c in zip(*t)])
    t = HEAD_CASES + e
    attr = [a for _, fs in t for a, _ in fs]
    return OK, dict(n=len(t), nnz=len(attr), num_attr=max(attr) + 1, ptr=[0] + list(np.cumsum([len(fs) for _, fs in t])),
                    attr=attr, x=[v for _, fs in t for _, v in fs], target=[y for y, _ in t])


@pytest.mark.parametrize("threads,chunk", [(1, 2 ** 30), (8, 1)], ids=["serial", "chunks"])
@pytest.mark.parametrize("loader", ["libfm", "cases"])
@pytest.mark.parametrize("r", TEXT, ids=lambda r: r["id"])
def test_text(tmp_path, monkeypatch, r, loader, threads, chunk):
    monkeypatch.setenv("SBMF_LOAD_THREADS", str(threads))
    monkeypatch.setenv("SBMF_LOAD_CHUNK", str(chunk))
    (tmp_path / "s").write_bytes(HEAD + r["tail"])
    rc, want = text_want(loader, r)
    check(tmp_path, {}, call=(loader, r["offset"]) if loader == "libfm" else (loader,), rc=rc, want=want)


def test_text_missing_file(tmp_path):
    check(tmp_path, {}, call=("libfm", 0), rc=E_IO, want="unable to open <T>/s")
    check(tmp_path, {}, call=("cases",), rc=E_IO, want="unable to open <T>/s")
