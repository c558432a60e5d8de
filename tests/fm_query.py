"""Helpers of the query-list tests (sbmf_fm_query_cases): query sets over the relation sets of
tests/fm_rel.py, their expansion into (query, block row) cases, the numpy yardstick and the bound.

The score of query q against block row j of the candidates' relation R is libFM's prediction of
the case "q's main features, q's block row of every other relation, block row j of R".  The
yardstick forms exactly that case for every (q, j) and hands it to fm_rel._rel_predict in long
double; the device multiplies the square out (include/sbmf.h), which reorders the sum.

The bound is derived, not measured: reordering a sum of m terms moves it by at most about
m eps sum|terms|.  A score has K factor sums over `entries` features each, the v^2 x^2 and w x
terms and w0; with A(q, j) the sum of the absolute values of every term,
    A = |w0| + sum_f 1/2 (sum_e |v_ef x_e|)^2 + sum_f sum_e 1/2 v_ef^2 x_e^2 + sum_e |w_e x_e|,
the mean may move by 4 (K + entries + 4) eps max_j A and the second moment by 2 max|score| times
that (d(s^2) = 2 s ds), as tests/test_gpu_recommend.py bounds its sums."""
import numpy as np

import fm_class
import fm_rel
from fm_rel import _csr_csc, _rel_predict, rows_to_cases
from sbmf import Relation

EPS = np.finfo(np.float64).eps


def case_rows(cases):
    """Cases -> per case a list of (attr, x)"""
    return [[(int(cases.attr[k]), float(cases.x[k])) for k in range(int(cases.ptr[c]), int(cases.ptr[c + 1]))]
            for c in range(cases.num_cases)]


def rel2_queries(S, nq, ids=None):
    """nq queries over rel2 (candidates: the item relation 1): (main rows, user block rows).  Query 0
    has no main feature, query 1 joins the last user row (no train case joins it), query 2 holds as many
    distinct main ids as the main id space has (p_main, fewer than 70; `ids` caps them), with uneven x."""
    nu = S.relations[0].block.num_cases
    main, urow = [], []
    for q in range(nq):
        if q == 0 and nq > 1:
            main.append([])
        elif q == 2:
            main.append([(a, 0.25 + 0.5 * (a % 3)) for a in range(min(70, ids or S.p_main))])
        else:
            main.append([((5 * q + 3) % (S.p_main - 1), 1.0)])
        urow.append(nu - 1 if q == 1 else (37 * q + 11) % (nu - 1))
    return main, np.array(urow, np.uint32)


def query_cases(S, main):
    return rows_to_cases(main)


class Expanded:
    """every (query, block row of relation `rel`) pair as cases: q-major, the block rows ascending"""

    def __init__(self, S, rel, main, rows):
        nb = S.relations[rel].block.num_cases
        nq = len(main)
        self.nq, self.nb, self.rel = nq, nb, rel
        self.cases = rows_to_cases([main[q] for q in range(nq) for _ in range(nb)])
        self.maps = []
        for r in range(len(S.relations)):
            if r == rel:
                self.maps.append(np.tile(np.arange(nb, dtype=np.int64), nq))
            else:
                self.maps.append(np.repeat(np.asarray(rows[r], np.int64), nb))
        self.B = [_csr_csc(R.block, np.longdouble) for R in S.relations]
        self.B64 = [_csr_csc(R.block, np.float64) for R in S.relations]
        self.offs = S.offsets
        # features of an expanded case: the query's, its other relations' block rows', the candidate's
        blen = [np.diff(R.block.ptr.astype(np.int64)) for R in S.relations]
        ent = np.array([len(m) for m in main], np.int64)
        for r in range(len(S.relations)):
            if r != rel:
                ent = ent + blen[r][np.asarray(rows[r], np.int64)]
        self.entries = ent + int(blen[rel].max())  # [nq]
        self.main, self.rows = main, rows

    def scores(self, model, task="r", clamp=None):
        """[nq, nb] long double: the predictions of the expanded cases (task "c": their probabilities)"""
        w0, w, v = model
        ft = np.longdouble
        p = _rel_predict(self.cases, self.maps, self.B, self.offs, ft(w0), w.astype(ft), v.astype(ft), ft)[0]
        if task == "c":
            p = fm_class.ref_cdf(p, ft)
        elif clamp is not None:
            p = np.clip(p, ft(clamp[0]), ft(clamp[1]))
        return p.reshape(self.nq, self.nb)

    def abs_terms(self, model):
        """[nq] float64: max over the candidates of A(q, j)"""
        w0, w, v = model
        K = v.shape[0]

        def parts(attr, x, rid, n, off):  # per row: sum_e |v x| by factor, sum 1/2 v^2 x^2, sum |w x|
            a = np.zeros((n, K))
            s, t = np.zeros(n), np.zeros(n)
            if len(attr):
                vx = np.abs(v[:, off + attr] * x)  # [K, nnz]
                for f in range(K):
                    np.add.at(a[:, f], rid, vx[f])
                np.add.at(s, rid, 0.5 * (vx * vx).sum(axis=0))
                np.add.at(t, rid, np.abs(w[off + attr] * x))
            return a, s, t

        qc = query_cases_of(self.main)
        qid = np.repeat(np.arange(self.nq), [len(m) for m in self.main])
        aq, sq, tq = parts(qc[0], qc[1], qid, self.nq, 0)
        cand = None
        for r, b in enumerate(self.B64):
            ab, sb, tb = parts(b["attr"], b["x"], b["rid"], b["nb"], self.offs[r])
            if r == self.rel:
                cand = (ab, sb, tb)
            else:
                rr = np.asarray(self.rows[r], np.int64)
                aq, sq, tq = aq + ab[rr], sq + sb[rr], tq + tb[rr]
        ab, sb, tb = cand
        A = abs(w0) + 0.5 * ((aq * aq).sum(1)[:, None] + (ab * ab).sum(1)[None, :] + 2.0 * aq @ ab.T) \
            + sq[:, None] + sb[None, :] + tq[:, None] + tb[None, :]
        return A.max(axis=1)

    def bound(self, model):
        """[nq]: the bound on one iteration's score"""
        K = model[2].shape[0]
        return 4.0 * (K + self.entries + 4) * EPS * self.abs_terms(model)


def query_cases_of(main):
    attr = np.array([a for m in main for a, _ in sorted(m)], np.int64)
    x = np.array([xx for m in main for _, xx in sorted(m)], np.float64)
    return attr, x


def twin_set(S, ex):
    """S with the expanded pairs as its test set (block form): the context whose sbmf_predict is the yardstick"""
    T = fm_rel.RelSet.__new__(fm_rel.RelSet)
    T.__dict__.update(S.__dict__)
    T.test = ex.cases
    assert max(S.train.num_attr, T.test.num_attr) + 1 == S.p_main
    T.relations = [Relation(R.block, R.train_row, ex.maps[r].astype(np.uint32), R.group) for r, R in enumerate(S.relations)]
    return T
