"""Block-structure relations (libFM's -relation), the parts that need no GPU: the new kernels'
resource summary (csrc/fmg.hip: k_fmr_*; read from build/fmg.resource.txt as
tests/test_fmg_resources.py reads the passes'), the ranges of a block table, the composition of
ids and groups of the test sets (tests/fm_rel.py) by libFM's rule (libfm.cpp:328-364), and the
entry points' presence in the C ABI."""
import os
import re

import numpy as np
import pytest

import fm_rel
from conftest import PKG
from sbmf import Cases, Relation, SBMFError, _lib, fm_ranges, load_libfm_relation, save_libfm_relation
from sbmf._lib import SBMF_E_IO

FIELDS = r"(SGPRs Spill|VGPRs Spill|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|VGPRs|LDS Size \[bytes/block\])"


def _kernels():
    res = os.path.join(PKG, "build", "fmg.resource.txt")
    if not os.path.exists(res):
        pytest.fail("%s is missing: rebuild csrc (make -C csrc clean all)" % res)
    kernels, cur = {}, None
    with open(res) as f:
        for line in f:
            m = re.search(r"remark: Function Name: (\S+)", line)
            if m:
                k = re.search(r"\d+(k_fmr_[a-z_]+?)(?:ILi(\d+)(?:ELi(\d+))?E)?E", m.group(1))
                cur = kernels.setdefault(k.groups(), {}) if k else None
                continue
            m = re.search(r"remark:\s+" + FIELDS + r": (\d+)", line)
            if m and cur is not None:
                cur[m.group(1).split(" [")[0]] = int(m.group(2))
    return kernels


def test_relation_kernels_use_no_scratch_and_spill_nothing():
    kernels = _kernels()
    want = {(n, m, nt) for n in ("k_fmr_pass", "k_fmr_gpass", "k_fmr_gather") for m in ("0", "1")
            for nt in ("64", "256", "1024")}
    want |= {("k_fmr_sync", "0", None), ("k_fmr_sync", "1", None), ("k_fmr_q", None, None), ("k_fmr_addq", None, None),
             ("k_fmr_block_predict", None, None), ("k_fmr_predict_train", None, None), ("k_fmr_predict_test", None, None),
             ("k_fmr_class_test", None, None)}
    want |= {("k_fmr_class_train", m, None) for m in ("0", "1", "2")}
    assert want <= set(kernels), sorted(want - set(kernels), key=str)
    for k in sorted(want, key=str):
        v = kernels[k]
        print(k, v)
        assert v["ScratchSize"] == 0 and v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0, (k, v)
        # gathers and scatters: waves hide the latency (the bar test_fm_class_resources.py sets the
        # frames, whose rejection loops hold the most registers)
        assert v["Occupancy"] >= 4, (k, v)


def test_ranges_of_a_block_table():
    # a one-hot id, a one-hot bucket, then two co-occurring tags: id and bucket are one range each,
    # the tags one range per attribute
    rows = [[(j, 1.0), (4 + j % 2, 1.0)] + ([(6, 0.5), (7, 0.5)] if j == 1 else [(6 + j % 2, 1.0)]) for j in range(4)]
    blk = fm_rel.rows_to_cases(rows, num_attr=8)
    assert fm_ranges(blk).tolist() == [0, 4, 6, 7, 8]
    S = fm_rel.rel_edge()
    b = fm_ranges(S.relations[0].block).tolist()
    assert b[0] == 0 and b[-1] == 59 and 9 in b and b[-2] <= 58  # the bucket is one range


def test_ids_and_groups_compose_as_libfm_composes_them(ml100k):
    for S in (fm_rel.rel2(ml100k), fm_rel.rel2_grouped(ml100k), fm_rel.rel_edge(), fm_rel.one_to_one()):
        off = max(S.train.num_attr, S.test.num_attr) + 1  # libfm.cpp:328
        goff = 1 if S.main_group is None else int(S.main_group.max()) + 1
        for R, o, g in zip(S.relations, S.offsets, S.group_offsets):
            assert (o, g) == (off, goff)
            off += R.block.num_attr  # :340, no + 1
            goff += R.num_groups
        assert (S.num_attribute, S.num_groups) == (off, goff) and len(S.group) == off
        # the twin's own count (its num_attr + 1) is the same num_attribute
        assert max(S.twin_train.num_attr, S.twin_test.num_attr) + 1 == S.num_attribute
        # the trap: the last relation's highest id sits on a block row no case joins, and the id
        # below it on a joined one -- the layout libFM's count of the expanded file needs
        R = S.relations[-1]
        joined = set(R.train_row.tolist()) | set(R.test_row.tolist())
        blk = R.block
        holders = lambda a: {j for j in range(blk.num_cases) if a in blk.attr[int(blk.ptr[j]):int(blk.ptr[j + 1])]}
        assert holders(blk.num_attr - 1) and not (holders(blk.num_attr - 1) & joined)
        assert holders(blk.num_attr - 2) & joined
        assert int(S.twin_train.attr.max()) < S.num_attribute - 1
        # every case of the twin holds its main features and its block rows' features
        c = len(S.twin_train.target) // 2
        want = S.train.ptr[c + 1] - S.train.ptr[c]
        for R in S.relations:
            j = int(R.train_row[c])
            want += R.block.ptr[j + 1] - R.block.ptr[j]
        assert S.twin_train.ptr[c + 1] - S.twin_train.ptr[c] == want


def test_rel_edge_has_the_edges_it_names():
    S = fm_rel.rel_edge()
    R = S.relations[0]
    per_row = np.bincount(R.train_row, minlength=R.block.num_cases)
    assert set(fm_rel.COUNTS) <= set(per_row.tolist())
    per_attr = np.bincount(R.block.attr, minlength=R.block.num_attr)
    assert per_attr[:9].tolist() == list(fm_rel.COUNTS)
    assert np.any(np.diff(R.block.ptr.astype(np.int64))[:-1] == 0)  # a block row without features
    assert np.any(np.diff(S.train.ptr.astype(np.int64)) == 0)      # a case without main features
    assert 1 not in S.main_group.tolist() and S.main_group.max() == 2  # an empty group id


def test_relation_checks_its_arguments():
    blk = fm_rel.rows_to_cases([[(0, 1.0)], [(1, 1.0)]], num_attr=2)
    with pytest.raises(ValueError, match="block.num_attr = 2"):
        Relation(blk, [0, 1], [], group=[0, 1, 1])
    with pytest.raises(ValueError):
        Relation([[0]], [0], [])
    R = Relation(blk, [0, 1], [], group=[0, 2])
    assert R.num_groups == 3 and Relation(blk, [0], []).num_groups == 1
    assert hasattr(_lib.lib, "sbmf_add_relation") and hasattr(_lib.lib, "sbmf_fm_relation_info")


@pytest.mark.parametrize("name", sorted(fm_rel.GOLDEN_RUNS))
def test_ids_and_groups_are_the_numbers_libfm_prints(name, ml100k):
    S = fm_rel.golden_set(fm_rel.GOLDEN_RUNS[name][0], ml100k)
    lines, pred, head = fm_rel.golden(name)
    assert len(lines) == fm_rel.GOLDEN_RUNS[name][3] and len(pred) == S.test.num_cases
    assert "#relations: %d" % len(S.relations) in head
    assert "#attr=%d\t#groups=%d" % (S.num_attribute, S.num_groups) in head
    for g, c in enumerate(np.bincount(S.group, minlength=S.num_groups)):
        assert "#attr_in_group[%d]=%d" % (g, c) in head
    for R in S.relations:
        assert "num_cases=%d\tnum_values=%d\tnum_features=%d" % (R.block.num_cases, len(R.block.attr), R.block.num_attr) in head


# ---- the relation files: round trips through the library's own readers and writers
def _same_relation(A, B):
    return (np.array_equal(A.block.ptr, B.block.ptr) and np.array_equal(A.block.attr, B.block.attr)
            and np.array_equal(A.block.x, B.block.x) and A.block.num_attr == B.block.num_attr
            and np.array_equal(A.train_row, B.train_row) and np.array_equal(A.test_row, B.test_row)
            and ((A.group is None and B.group is None) or np.array_equal(A.group, B.group)))


def test_relation_files_round_trip(ml100k, tmp_path):
    for S in (fm_rel.rel2_grouped(ml100k), fm_rel.rel_edge()):
        d = tmp_path / ("s%d" % len(S.relations))
        d.mkdir()
        stems = fm_rel.write_binary_set(S, d)  # relation 0: .xt and binary maps; the others .x and text maps
        for k, (stem, R) in enumerate(zip(stems, S.relations)):
            assert os.path.exists(str(d / (stem + (".xt" if k == 0 else ".x"))))
            assert not os.path.exists(str(d / (stem + (".x" if k == 0 else ".xt"))))
            assert _same_relation(load_libfm_relation(d / stem), R)
    R = Relation(fm_rel.rows_to_cases([[(0, 1.0)], [], [(1, 0.5), (2, -1.5)]], num_attr=4), [2, 0, 0], [1])
    save_libfm_relation(tmp_path / "plain", R)  # text maps, no .groups, a row without features, an unused last id
    L = load_libfm_relation(tmp_path / "plain")
    assert _same_relation(L, R) and L.group is None
    with open(str(tmp_path / "plain.x"), "rb") as f:  # fmatrix.h's header: id 2, 4-byte values, values, rows, columns
        assert np.frombuffer(f.read(24), np.uint32).tolist() == [2, 4, 3, 0, 3, 4]


def test_relation_loader_errors_name_the_file_and_entry(tmp_path):
    R = Relation(fm_rel.rows_to_cases([[(0, 1.0)], [(1, 0.5)]], num_attr=2), [1, 0, 0], [1], group=[0, 1])
    save_libfm_relation(tmp_path / "r", R)

    def fails(*words):
        with pytest.raises(SBMFError) as e:
            load_libfm_relation(tmp_path / "r")
        assert e.value.code == SBMF_E_IO and all(w in str(e.value) for w in words), str(e.value)

    assert len(load_libfm_relation(tmp_path / "r").train_row) == 3  # a map's length is the caller's to check
    (tmp_path / "r.train").write_text("1\n0\nx\n")
    fails("r.train", "entry 3")
    (tmp_path / "r.train").write_text("1\n0\n0\n")
    (tmp_path / "r.groups").write_text("0\n")
    fails("r.groups", "entry 2")
    os.remove(str(tmp_path / "r.groups"))
    os.remove(str(tmp_path / "r.test"))
    fails("r.test")
    (tmp_path / "r.test").write_text("1\n")
    blob = (tmp_path / "r.x").read_bytes()
    (tmp_path / "r.x").write_bytes(blob[:-4])
    fails("r.x", "truncated at row 1")
    os.remove(str(tmp_path / "r.x"))
    fails("r.xt")


# ---- the serial restatement of libFM's ALS with relations against libFM itself
def test_restatement_matches_the_als_golden(ml100k):
    name = "ref_libfm_rel_rel2_als_i8"
    S = fm_rel.golden_set("rel2", ml100k)
    lines, pred, _ = fm_rel.golden(name)
    out = fm_rel.als_restatement(S, 8, 8, record=range(1, 9))
    train = [float(out[it][3]) for it in range(1, 9)]
    ref_train = [float(l.split("Train=")[1].split()[0]) for l in lines]
    p = np.asarray(ref_train)
    print(train, ref_train, np.abs(out[8][4] - pred).max())
    assert np.all(np.abs(np.asarray(train) - p) <= 0.5 * 10.0 ** (np.floor(np.log10(p)) - 5) + 1e-12)
    # libFM's -out of ALS is the last iteration's clamped prediction, printed with 6 significant digits
    assert np.all(np.abs(out[8][4].astype(np.float64) - pred) <= 0.5 * 10.0 ** (np.floor(np.log10(pred)) - 5) + 1e-12)
    # "Test=" is the RMSE of the running mean of the iterations' clamped predictions, in ALS too
    # (fm_learn_mcmc_simultaneous.h:134-245)
    ref_test = [float(l.split("Test=")[1].split()[0]) for l in lines]
    y = S.test.target.astype(np.float64)
    run = np.cumsum([out[it][4].astype(np.float64) for it in range(1, 9)], axis=0)
    test = [float(np.sqrt(np.mean((run[it - 1] / it - y) ** 2))) for it in range(1, 9)]
    q = np.asarray(ref_test)
    assert np.all(np.abs(np.asarray(test) - q) <= 0.5 * 10.0 ** (np.floor(np.log10(q)) - 5) + 1e-12)


def test_restatement_of_one_case_per_block_row_equals_the_plain_restatement():
    """with every block row joined by one case the relation form is the expanded cases: the
    restatement with relations against tests/fm_cases.py's restatement of the twin with groups"""
    import fm_groups
    S = fm_rel.one_to_one()
    reg = fm_rel.als_regular(S.num_groups)
    G = S.num_groups
    a = fm_rel.als_restatement(S, 4, 3, record=(3,))[3]
    b = fm_groups.als_restatement_groups(S.twin_train, S.twin_test, 4, 3, 1, reg[0], reg[1:1 + G], reg[1 + G:], S.group,
                                         record=(3,))[3]
    assert np.abs(a[1] - b[1]).max() < 1e-12 and np.abs(a[2] - b[2]).max() < 1e-12 and np.abs(a[4] - b[4]).max() < 1e-12
