"""Sets of the relation tests (libFM's -relation), derived by rule from the committed ML-100k
triples, each in two forms: the block form (main cases + Relations) and its expanded twin -- the
same cases with every joined block row's features written out, the relation's attribute ids
shifted by its offset, and a group table that puts the main ids first and each relation's groups
after them.  libFM's chain on the two forms is the same chain (the reference prints identical
lines for them); the block form only sums per block row what the twin sums per case.

Ids (libfm.cpp:328-341): attr_offset_0 = max(train, test num_attr) + 1, attr_offset_{r+1} =
attr_offset_r + num_attr_r, num_attribute = the final sum.  The twin's num_attribute is its own
num_attr + 1, so the twin is given num_attr = num_attribute - 1 explicitly; every set also keeps
the last relation's highest id on a block row no case joins, the layout for which libFM's own
count of the expanded file agrees.

"rel2" (every 4th ML-100k case):
  main   (u + 3 i) mod 7, one-hot, ids 0..6
  users  block row u: id u; bucket u mod 4 at UB0 + b (+ 1 from b = 2: UB0 + 2 is a gap); tags
         UT0 + t for the set bits t < 3 of u // 4 with x = 0.5 (0 to 3 tags, co-occurring).  Row I
         is a user of the test set only ((u + i) mod 37 == 0 test cases are re-mapped to it).
  items  block row i: id i; tags J + t for the set bits t < 4 of i, x = 1 for one tag, else 0.5.
         Row J is joined by nobody and holds the highest id J + 4.
"rel_edge": one relation of 1401 block rows joined by 0, 1, 63, 64, 65, 255, 256, 257 and 1025
  cases (the others by one); attributes 0..8 held by those same counts of block rows (staggered,
  so they co-occur), a 49-value bucket, two block rows without features, an unjoined last row with
  the highest id; main cases with an 11-value field, every 17th without main features; main meta
  with an empty group id, the relation in two groups."""
import numpy as np

from sbmf import Cases, Relation

COUNTS = (0, 1, 63, 64, 65, 255, 256, 257, 1025)


def rows_to_cases(rows, targets=None, num_attr=None):
    """rows: per case a list of (attr, x) -> Cases with the entries sorted by attribute"""
    ptr = np.zeros(len(rows) + 1, np.uint64)
    attr, x = [], []
    for c, f in enumerate(rows):
        f = sorted(f, key=lambda e: e[0])
        attr += [a for a, _ in f]
        x += [v for _, v in f]
        ptr[c + 1] = len(attr)
    y = np.zeros(len(rows), np.float32) if targets is None else np.asarray(targets, np.float32)
    return Cases(ptr, np.array(attr, np.uint32), np.array(x, np.float32), y, num_attr=num_attr)


class RelSet:
    """main_train / main_test: (rows, targets); rels: [(block rows, num_attr, train_row, test_row, group or None)];
    main_group: group ids of the main table's num_attribute ids, or None"""

    def __init__(self, main_train, main_test, rels, main_group=None):
        self.train = rows_to_cases(*main_train)
        self.test = rows_to_cases(*main_test)
        self.p_main = max(self.train.num_attr, self.test.num_attr) + 1
        self.main_group = None if main_group is None else np.asarray(main_group, np.uint32)
        assert self.main_group is None or len(self.main_group) == self.p_main
        self.relations, self.offsets, self.group_offsets = [], [], []
        off, goff = self.p_main, 1 if main_group is None else int(self.main_group.max()) + 1
        group = [np.zeros(self.p_main, np.uint32) if main_group is None else self.main_group]
        ex_train = [list(f) for f in main_train[0]]
        ex_test = [list(f) for f in main_test[0]]
        for rows, num_attr, train_row, test_row, g in rels:
            R = Relation(rows_to_cases(rows, num_attr=num_attr), train_row, test_row, g)
            self.relations.append(R)
            self.offsets.append(off)
            self.group_offsets.append(goff)
            for ex, rmap in ((ex_train, train_row), (ex_test, test_row)):
                for c, j in enumerate(rmap):
                    ex[c] += [(off + a, x) for a, x in rows[j]]
            group.append(goff + (np.zeros(num_attr, np.uint32) if g is None else np.asarray(g, np.uint32)))
            off += num_attr
            goff += R.num_groups
        self.num_attribute, self.num_groups = off, goff
        self.group = np.concatenate(group).astype(np.uint32)  # the joined table: the twin's -meta
        self.twin_train = rows_to_cases(ex_train, main_train[1], num_attr=off - 1)
        self.twin_test = rows_to_cases(ex_test, main_test[1], num_attr=off - 1)


_CACHE = {}


def rel2(ml100k, binary=False):
    key = ("rel2", binary)
    if key not in _CACHE:
        (tu, ti, tr), (su, si, sr) = ml100k
        I = int(max(tu.max(), su.max())) + 1
        J = int(max(ti.max(), si.max())) + 1
        tu, ti, tr = tu[::4].tolist(), ti[::4].tolist(), tr[::4]
        su, si, sr = su[::4].tolist(), si[::4].tolist(), sr[::4]
        if binary:  # -task c: ratings of 4 and 5 are the positive class
            tr, sr = np.where(tr >= 4, 1.0, -1.0), np.where(sr >= 4, 1.0, -1.0)
        main = lambda U, It: [[((u + 3 * i) % 7, 1.0)] for u, i in zip(U, It)]
        UB0 = I + 1
        UT0 = UB0 + 5
        urows = []
        for u in range(I + 1):
            b = u % 4 if u < I else 1
            tags = [t for t in range(3) if ((u // 4) >> t) & 1] if u < I else [0]
            urows.append([(u, 1.0), (UB0 + b + (1 if b >= 2 else 0), 1.0)] + [(UT0 + t, 0.5) for t in tags])
        irows = []
        for i in range(J):
            tags = [t for t in range(4) if (i >> t) & 1]
            irows.append([(i, 1.0)] + [(J + t, 1.0 if len(tags) == 1 else 0.5) for t in tags])
        irows.append([(J + 4, 1.0)])
        utest = [I if (u + i) % 37 == 0 else u for u, i in zip(su, si)]
        _CACHE[key] = RelSet((main(tu, ti), tr), (main(su, si), sr),
                             [(urows, UT0 + 3, tu, utest, None), (irows, J + 5, ti, si, None)])
    return _CACHE[key]


def rel2_grouped(ml100k):
    """rel2 with a main -meta (two groups) and the relations' own .groups (ids / bucket / tags; ids / tags)"""
    if "rel2g" not in _CACHE:
        base = rel2(ml100k)
        (tu, ti, tr), (su, si, sr) = ml100k
        I = int(max(tu.max(), su.max())) + 1
        J = int(max(ti.max(), si.max())) + 1
        ug = np.array([0] * (I + 1) + [1] * 5 + [2] * 3, np.uint32)
        ig = np.array([0] * J + [1] * 5, np.uint32)
        mg = np.array([0, 0, 0, 1, 1, 1, 1, 0], np.uint32)
        S = RelSet.__new__(RelSet)
        S.__dict__.update(base.__dict__)
        S.main_group = mg
        S.relations = [Relation(base.relations[0].block, base.relations[0].train_row, base.relations[0].test_row, ug),
                       Relation(base.relations[1].block, base.relations[1].train_row, base.relations[1].test_row, ig)]
        S.group_offsets = [2, 5]
        S.num_groups = 7
        S.group = np.concatenate([mg, 2 + ug, 5 + ig]).astype(np.uint32)
        _CACHE["rel2g"] = S
    return _CACHE["rel2g"]


def rel_edge():
    if "edge" not in _CACHE:
        nb = 1400
        cnt = list(COUNTS) + [1] * (nb - len(COUNTS))
        train_row = [j for j in range(nb) for _ in range(cnt[j])]
        # interleave, so that a block row's cases are not contiguous
        order = sorted(range(len(train_row)), key=lambda c: (c * 7919) % len(train_row))
        train_row = [train_row[c] for c in order]
        N, T = len(train_row), 300
        test_row = [(c * 13) % nb for c in range(T)]
        rows = []
        for j in range(nb):
            f = []
            for k, n in enumerate(COUNTS):
                if 5 * k <= j < 5 * k + n:
                    f.append((k, 1.0 if k % 2 == 0 else 0.5 + (j % 3) * 0.25))
            if not (j % 50 == 49 and j >= 1300):  # rows 1349 and 1399 hold no feature
                if j % 50 != 49:
                    f.append((9 + j % 50, 1.0))
                else:
                    f.append((9 + 48, 0.5))
            rows.append(f)
        rows.append([(58, 1.0)])  # the unjoined last row holds the highest id
        rgroup = np.array([0] * 9 + [1] * 50, np.uint32)
        main = lambda n, s: [[] if c % 17 == 0 else [((c + s) % 11, 1.0)] for c in range(n)]
        ytr = [1.0 + ((7 * c + 3 * j) % 9) * 0.5 for c, j in enumerate(train_row)]
        yte = [1.0 + ((5 * c + 3 * j) % 9) * 0.5 for c, j in enumerate(test_row)]
        mg = np.array([0] * 11 + [2], np.uint32)  # group 1 holds no attribute
        _CACHE["edge"] = RelSet((main(N, 0), ytr), (main(T, 3), yte), [(rows, 59, train_row, test_row, rgroup)], mg)
    return _CACHE["edge"]


def one_to_one(n=500):
    """every block row joined by exactly one train case"""
    key = ("one", n)
    if key not in _CACHE:
        rows = [[(j % 40, 1.0), (40 + j % 7, 0.5 + (j % 2))] for j in range(n)] + [[(47, 1.0)]]
        main = lambda m: [[(c % 5, 1.0)] for c in range(m)]
        perm = [(c * 37) % n for c in range(n)]  # 37 and 500 are coprime
        y = [1.0 + ((3 * c) % 9) * 0.5 for c in range(n)]
        test_row = [(c * 11) % n for c in range(60)]
        _CACHE[key] = RelSet((main(n), y), (main(60), y[:60]), [(rows, 48, perm, test_row, None)])
    return _CACHE[key]


# ---- the files bin/libFM reads, and the goldens its -relation runs left (tests/make_fm_rel_golden.py)
def cases_to_text(cases):
    out = []
    for c in range(cases.num_cases):
        b, e = int(cases.ptr[c]), int(cases.ptr[c + 1])
        out.append("%g %s\n" % (cases.target[c], " ".join("%d:%g" % (a, x) for a, x in zip(cases.attr[b:e], cases.x[b:e]))))
    return "".join(out)


def write_set(S, dirpath, stems=("relu", "reli")):
    """train.libfm / test.libfm, per relation <stem>.libfm (the block table as text, for libFM's convert
    tool), <stem>.train / <stem>.test (text maps) and <stem>.groups when the relation has groups,
    meta.txt when the main table has; returns the stems used"""
    d = str(dirpath)
    import os
    for nm, cs in (("train.libfm", S.train), ("test.libfm", S.test)):
        with open(os.path.join(d, nm), "w") as f:
            f.write(cases_to_text(cs))
    used = list(stems[:len(S.relations)])
    for stem, R in zip(used, S.relations):
        with open(os.path.join(d, stem + ".libfm"), "w") as f:
            f.write(cases_to_text(R.block))
        for ext, m in ((".train", R.train_row), (".test", R.test_row)):
            with open(os.path.join(d, stem + ext), "w") as f:
                f.write("".join("%d\n" % j for j in m))
        if R.group is not None:
            with open(os.path.join(d, stem + ".groups"), "w") as f:
                f.write("".join("%d\n" % g for g in R.group))
    if S.main_group is not None:
        with open(os.path.join(d, "meta.txt"), "w") as f:
            f.write("".join("%d\n" % g for g in S.main_group))
    return used


def als_regular(G):
    """distinct per-group precisions: r0, w_lambda[g], v_lambda[g]"""
    return (0.0,) + tuple(1.0 + g for g in range(G)) + tuple(10.0 + 5 * g for g in range(G))


# name -> (set, method, task, iterations); -dim 1,1,8, seed pinned; ALS with als_regular of the set's groups
GOLDEN_RUNS = {
    "ref_libfm_rel_rel2_mcmc_i8": ("rel2", "mcmc", "r", 8),
    "ref_libfm_rel_rel2_als_i8": ("rel2", "als", "r", 8),
    "ref_libfm_rel_rel2g_mcmc_i8": ("rel2g", "mcmc", "r", 8),
    "ref_libfm_rel_rel2b_mcmc_c_i8": ("rel2b", "mcmc", "c", 8),
    "ref_libfm_rel_edge_mcmc_i5": ("edge", "mcmc", "r", 5),
}


def golden_set(name, ml100k):
    return {"rel2": lambda: rel2(ml100k), "rel2g": lambda: rel2_grouped(ml100k),
            "rel2b": lambda: rel2(ml100k, binary=True), "edge": rel_edge}[name]()


def golden(name):
    """(#Iter lines, -out predictions, "num_attr / #relations / group" header lines) of a golden run"""
    import gzip
    import os
    from conftest import GOLD
    with open(os.path.join(GOLD, name + ".txt")) as f:
        lines = f.read().splitlines()
    with gzip.open(os.path.join(GOLD, name + "_pred.txt.gz"), "rt") as f:
        pred = np.array([float(x) for x in f.read().split()])
    return [l for l in lines if l.startswith("#Iter=")], pred, [l for l in lines if not l.startswith("#Iter=")]


def transpose_block(block):
    """the block table attribute-major, as Cases whose rows are attributes and whose entries are
    block rows: what libFM's transpose tool writes as <stem>.xt"""
    rows = [[] for _ in range(block.num_attr)]
    for j in range(block.num_cases):
        for k in range(int(block.ptr[j]), int(block.ptr[j + 1])):
            rows[int(block.attr[k])].append((j, float(block.x[k])))
    return rows_to_cases(rows, num_attr=block.num_cases)


def write_binary_set(S, dirpath, stems=("relu", "reli")):
    """write_set, then the block tables through the library's own writers: the first relation as
    <stem>.xt with binary maps, the others as <stem>.x with text maps"""
    import ctypes as C
    import os
    from sbmf import _lib, save_libfm_relation
    used = write_set(S, dirpath, stems)
    for k, (stem, R) in enumerate(zip(used, S.relations)):
        path = os.path.join(str(dirpath), stem)
        save_libfm_relation(path, R, binary_maps=(k == 0))
        if k == 0:
            bt = transpose_block(R.block)  # kept alive: _c() points into its arrays
            c = bt._c()
            assert _lib.lib.sbmf_save_libfm_block((path + ".xt").encode(), C.byref(c)) == 0
            os.remove(path + ".x")
    return used


# ---- libFM's ALS with relations, restated serially: draw_all (fm_learn_mcmc.h:411-623) with
# draw_w_rel (:721-777), draw_v_rel (:839-899) and predict_data_and_write_to_eterms (:117-348),
# attribute by attribute in ascending id, in the float type `ft`.  Per-group precisions
# (w_lambda[g], v_lambda[g]) from als_regular; w_mu = v_mu = 0, alpha = 1.  The per-block-row
# sums are added case by case in case order (np.add.at), as the reference's loops add them.
def _csr_csc(block, ft):
    nb, pa = block.num_cases, block.num_attr
    rid = np.repeat(np.arange(nb), np.diff(block.ptr.astype(np.int64)))
    order = np.argsort(block.attr, kind="stable")
    ap = np.concatenate([[0], np.cumsum(np.bincount(block.attr, minlength=pa))])
    return {"nb": nb, "pa": pa, "rid": rid, "attr": block.attr.astype(np.int64), "x": block.x.astype(ft),
            "ap": ap, "rows": rid[order], "xs32": block.x[order], "xs": block.x[order].astype(ft)}


def _rel_predict(cases, maps, B, offs, w0, w, v, ft):
    """(predictions of the cases, per relation the block rows' y)"""
    n = cases.num_cases
    cid = np.repeat(np.arange(n), np.diff(cases.ptr.astype(np.int64)))
    x = cases.x.astype(ft)
    e, q2 = np.zeros(n, ft), np.zeros(n, ft)
    yb = [np.zeros(b["nb"], ft) for b in B]
    qs = [np.zeros(b["nb"], ft) for b in B]
    for f in range(v.shape[0]):
        q = np.zeros(n, ft)
        np.add.at(q, cid, v[f][cases.attr] * x)
        for r, b in enumerate(B):
            vb = v[f][offs[r] + b["attr"]]
            qb = np.zeros(b["nb"], ft)
            np.add.at(qb, b["rid"], vb * b["x"])
            q = q + qb[maps[r]]
            yb[r] += ft(0.5) * qb * qb
            np.subtract.at(qs[r], b["rid"], ft(0.5) * vb * vb * b["x"] * b["x"])
        e += ft(0.5) * q * q
        np.subtract.at(q2, cid, ft(0.5) * v[f][cases.attr] * v[f][cases.attr] * x * x)
    np.add.at(q2, cid, w[cases.attr] * x)
    for r, b in enumerate(B):
        np.add.at(qs[r], b["rid"], w[offs[r] + b["attr"]] * b["x"])
        q2 = q2 + qs[r][maps[r]]
        yb[r] = yb[r] + qs[r]
    return e + q2 + w0, yb


def als_restatement(S, K, iters, seed=1, ft=np.float64, init_stdev=0.1, record=()):
    """Returns {iteration: (w0, w, v, train rmse, clamped test predictions)} for a RelSet S."""
    with np.errstate(all="ignore"):
        return _als_restatement(S, K, iters, seed, ft, init_stdev, record)


def _als_restatement(S, K, iters, seed, ft, init_stdev, record):
    import sbmf
    from fm_cases import _csc
    p, pm, G = S.num_attribute, S.p_main, S.num_groups
    reg = als_regular(G)
    reg0, regw, regv = ft(reg[0]), [ft(r) for r in reg[1:1 + G]], [ft(r) for r in reg[1 + G:]]
    grp = S.group
    z = sbmf.ref_stream(seed, 1, K * p + p)
    v = (z[:K * p].reshape(K, p) * init_stdev).astype(ft)
    w = (z[K * p:] * init_stdev).astype(ft)
    w0, alpha, zero = ft(0.0), ft(1.0), ft(0.0)
    train, test = S.train, S.test
    B = [_csr_csc(R.block, ft) for R in S.relations]
    offs = S.offsets
    mtr = [R.train_row.astype(np.int64) for R in S.relations]
    mte = [R.test_row.astype(np.int64) for R in S.relations]
    wnum = [np.bincount(m, minlength=b["nb"]).astype(ft) for m, b in zip(mtr, B)]
    ap, cs, xs32 = _csc(train, pm)
    xs = xs32.astype(ft)
    y = train.target.astype(ft)
    lo, hi = ft(train.target.min()), ft(train.target.max())
    n = train.num_cases
    ccid = np.repeat(np.arange(n), np.diff(train.ptr.astype(np.int64)))
    cx = train.x.astype(ft)
    pr, yb = _rel_predict(train, mtr, B, offs, w0, w, v, ft)
    e = pr - y

    def draw(m, s, old, lam):  # the posterior mean under {lambda, mu = 0}; None: the old value stays
        s2 = ft(1.0) / (lam + alpha * s)
        new = -s2 * (alpha * m - zero * lam) if np.isfinite(s2) else zero
        return new if np.isfinite(new) else None

    out = {}
    for it in range(1, iters + 1):
        m = np.sum(e - w0)
        s2 = ft(1.0) / (reg0 + alpha * n)
        new = -s2 * (alpha * m - zero * reg0)
        e -= (w0 - new)
        w0 = new
        for a in range(pm):  # draw_w over the main table, up to the first relation (:435-457)
            c, x, x32 = cs[ap[a]:ap[a + 1]], xs[ap[a]:ap[a + 1]], xs32[ap[a]:ap[a + 1]]
            new = draw(np.sum(x * (e[c] - w[a] * x)), np.sum((x32 * x32).astype(ft)), w[a], regw[grp[a]])
            if new is None:
                continue
            e[c] -= x * (w[a] - new)
            w[a] = new
        for r, b in enumerate(B):  # :458-491
            we = np.zeros(b["nb"], ft)
            np.add.at(we, mtr[r], e)
            e -= yb[r][mtr[r]]
            for a in range(b["pa"]):
                j, x, x32 = b["rows"][b["ap"][a]:b["ap"][a + 1]], b["xs"][b["ap"][a]:b["ap"][a + 1]], b["xs32"][b["ap"][a]:b["ap"][a + 1]]
                g = offs[r] + a
                s = np.sum((x32 * x32).astype(ft) * wnum[r][j])
                new = draw(np.sum(x * we[j]) - w[g] * s, s, w[g], regw[grp[g]])
                if new is None:
                    continue
                we[j] -= x * (w[g] - new) * wnum[r][j]
                yb[r][j] += (new - w[g]) * x
                w[g] = new
            e += yb[r][mtr[r]]
        for f in range(K):
            q = np.zeros(n, ft)
            np.add.at(q, ccid, v[f][train.attr] * cx)
            qb = []
            for r, b in enumerate(B):  # :521-552
                t = np.zeros(b["nb"], ft)
                np.add.at(t, b["rid"], v[f][offs[r] + b["attr"]] * b["x"])
                qb.append(t)
                q = q + t[mtr[r]]
            for a in range(pm):
                c, x = cs[ap[a]:ap[a + 1]], xs[ap[a]:ap[a + 1]]
                h = x * (q[c] - x * v[f, a])
                s = np.sum(h * h)
                new = draw(np.sum(h * e[c]) - v[f, a] * s, s, v[f, a], regv[grp[a]])
                if new is None:
                    continue
                d = v[f, a] - new
                q[c] -= x * d
                e[c] -= h * d
                v[f, a] = new
            for r, b in enumerate(B):  # :579-620
                mp, nb = mtr[r], b["nb"]
                q = q - qb[r][mp]
                we, weq, wc, wcs = (np.zeros(nb, ft) for _ in range(4))
                np.add.at(we, mp, e)
                np.add.at(weq, mp, e * q)
                np.add.at(wc, mp, q)
                np.add.at(wcs, mp, q * q)
                e -= yb[r][mp] + q * qb[r][mp]
                for a in range(b["pa"]):
                    sl = slice(b["ap"][a], b["ap"][a + 1])
                    j, x, x32 = b["rows"][sl], b["xs"][sl], b["xs32"][sl]
                    g = offs[r] + a
                    old = v[f, g]
                    h = x * (qb[r][j] - x * old)
                    xx = (x32 * x32).astype(ft)
                    s = np.sum(h * h * wnum[r][j] + 2 * wc[j] * x * h + xx * wcs[j])
                    new = draw(np.sum(h * we[j] + x * weq[j]) - old * s, s, old, regv[grp[g]])
                    if new is None:
                        continue
                    d = old - new
                    we[j] -= d * (h * wnum[r][j] + x * wc[j])
                    qb[r][j] -= d * x
                    weq[j] -= d * (h * wc[j] + x * wcs[j])
                    yb[r][j] += (new - old) * h
                    v[f, g] = new
                e += yb[r][mp] + q * qb[r][mp]
                q = q + qb[r][mp]
        pr, yb = _rel_predict(train, mtr, B, offs, w0, w, v, ft)
        e = pr - y
        if it in record:
            rm = np.sqrt(np.mean((np.clip(pr, lo, hi) - y) ** 2))
            pt = np.clip(_rel_predict(test, mte, B, offs, w0, w, v, ft)[0], lo, hi)
            out[it] = (w0, w.copy(), v.copy(), rm, pt)
    return out
