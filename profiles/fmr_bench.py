#!/usr/bin/env python3
"""Cost of block-structure relations (libFM's -relation) against the same cases
expanded, on the ML-20M-shaped synthetic, K = 100, f64, Philox normals, per MCMC iteration
(method as profiles/fmg_bench.py: host clock around --steps iterations after --warmup, and the
mean of the iterations' HIP-event times).

Side information that is a property of the user or of the item, in three sizes, each as the
expanded cases through the general learner (with the groups the block form has; the same model but
for one trailing attribute without a case, see below) and as its block form:
  b / bB  users | items                       bB: items in the main table, users in a relation
  c / cB  + per user a 24-value field ((5 u) mod 24) and 5 tags (the set bits of u, x = 1 for one
          tag, else 0.5)                      cB: id, field and tags in one user relation
  d / dB  + per item a 7-value field (i mod 7) and 5 tags (the set bits of i)
                                              dB: no main features; a user and an item relation
A block setting followed by 'r' (bBr, cBr, dBr) runs with the cases ordered by relation 0's block
row (the learner's default for a context with relations), the plain one with
SBMF_FMG_CASE_ORDER=attribute: by their first main attribute, as a context without relations.
Alternating runs (--reps of each).  One JSON line on stdout (progress lines start with '#');
--out also writes it to a file.  Needs an MI355X."""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "scalable-bayesian-matrix-factorization_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from watch_bench import device_sync  # noqa: E402


def entity_fields(n, nval, with_side):
    """Per entity e < n the columns (attribute id or -1, x) of: its id; with_side: a one-hot field of
    nval values and 5 tags.  Returns (ids [n, m], x [n, m], num_attr)."""
    e = np.arange(n, dtype=np.int64)
    cols, vals, base = [e], [np.ones(n, np.float32)], n
    if with_side:
        cols.append(base + (5 * e) % nval if nval == 24 else base + e % nval)
        vals.append(np.ones(n, np.float32))
        base += nval
        ntag = sum(((e >> t) & 1) for t in range(5))
        for t in range(5):
            cols.append(np.where((e >> t) & 1, base + t, -1))
            vals.append(np.where(ntag == 1, 1.0, 0.5).astype(np.float32))
        base += 5
    return np.stack(cols, axis=1), np.stack(vals, axis=1), base


def to_cases(A, X, y, num_attr):
    from sbmf import Cases
    keep = A >= 0
    ptr = np.concatenate([[0], np.cumsum(keep.sum(axis=1))]).astype(np.uint64)
    return Cases(ptr, A[keep].astype(np.uint32), X[keep], np.asarray(y, np.float32), num_attr=num_attr)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="ml-20m")
    ap.add_argument("--K", type=int, default=100)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--settings", default="b,bB,bBr,c,cB,cBr,d,dB,dBr")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    from sbmf import FMLearnSBPMF, Relation, synth
    train, test, dims = synth.generate(args.shape)
    I, J = int(dims[0]), int(dims[1])
    sets = {}

    def data(name):
        """(train Cases, test Cases, relations, main group table or None)"""
        if name in sets:
            return sets[name]
        size = name[0]
        UA, UX, pu = entity_fields(I, 24, size in "cd")
        IA, IX, pi = entity_fields(J, 7, size == "d")
        ublock, iblock = to_cases(UA, UX, np.zeros(I), pu), to_cases(IA, IX, np.zeros(J), pi)
        out = []
        if name.endswith("B"):
            rels = []
            for u, i, r in (train, test):
                if size == "d":  # no main features
                    out.append(to_cases(np.full((len(u), 1), -1, np.int64), np.zeros((len(u), 1), np.float32), r, 0))
                else:
                    out.append(to_cases(IA[i], IX[i], r, pi))
            rels.append(Relation(ublock, train[0], test[0]))
            if size == "d":
                rels.append(Relation(iblock, train[1], test[1]))
            sets[name] = (out[0], out[1], rels, None)
        else:
            # the expanded twin: the ids in the block form's order (main table, trailing id, relations)
            main_p = 1 if size == "d" else pi + 1
            for u, i, r in (train, test):
                parts_a, parts_x = [], []
                if size != "d":
                    parts_a.append(IA[i])
                    parts_x.append(IX[i])
                parts_a.append(np.where(UA[u] >= 0, UA[u] + main_p, -1))
                parts_x.append(UX[u])
                if size == "d":
                    parts_a.append(np.where(IA[i] >= 0, IA[i] + main_p + pu, -1))
                    parts_x.append(IX[i])
                p = main_p + pu + (pi if size == "d" else 0)
                out.append(to_cases(np.concatenate(parts_a, axis=1), np.concatenate(parts_x, axis=1), r, p))
            # (the highest id is on a joined block row here, so the twin counts one trailing attribute more than
            # the block form: a draw from the prior, no case -- the cost is the same, the chain is not)
            g = np.zeros(p + 1, np.uint32)
            g[main_p:] = 1
            if size == "d":
                g[main_p + pu:] = 2
            sets[name] = (out[0], out[1], [], g)
        return sets[name]

    def run(name):
        by_rel = name.endswith("r")
        name_d = name[:-1] if by_rel else name
        tr, te, rels, group = data(name_d)
        os.environ["SBMF_FMG_CASE_ORDER"] = "relation" if by_rel else "attribute"
        L = FMLearnSBPMF(num_factor=args.K, seed=2015, rng="philox", method="mcmc", order="libfm", init_stdev=0.1)
        if group is not None:
            L.set_groups(group)
        for R in rels:
            L.add_relation(R)
        L.set_data(tr, te)
        os.environ.pop("SBMF_FMG_CASE_ORDER", None)
        L.learn(sweeps=args.warmup)
        device_sync()
        n0 = len(L.history)
        t0 = time.perf_counter()
        L.learn(sweeps=args.steps)
        device_sync()
        info = L.fm_info()
        res = {"ms_per_iter_host": 1e3 * (time.perf_counter() - t0) / args.steps,
               "ms_per_iter_events": float(np.mean([h["ms_sweep"] + h["ms_eval"] for h in L.history[n0:]])),
               "ms_sweep_events": float(np.mean([h["ms_sweep"] for h in L.history[n0:]])),
               "ms_eval_events": float(np.mean([h["ms_eval"] for h in L.history[n0:]])),
               "launches_per_iter": info["launches_per_iter"], "num_attr": info["num_attr"], "nranges": info["nranges"],
               "rmse_test": L.history[-1]["rmse_avg"], "main_nnz": int(len(tr.attr)),
               "block_nnz": [int(len(R.block.attr)) for R in rels], "block_rows": [R.block.num_cases for R in rels],
               "relation_ranges": [r["nranges"] for r in L.fm_relation_info()], "groups": L.fm_groups()["cnt"].tolist()}
        L.close()
        print("# %s %s" % (name, json.dumps(res)), flush=True)
        return res

    names = [s for s in args.settings.split(",") if s]
    runs = {s: [] for s in names}
    for _ in range(args.reps):
        for s in names:
            runs[s].append(run(s))
    out = {"what": "libFM MCMC, %s K=%d f64 philox: user / item side information expanded on every case (b, c, d) and as "
                   "block-structure relations (bB, cB, dB)" % (args.shape, args.K),
           "num_users": I, "num_items": J, "n_train": int(len(train[0])), "steps": args.steps, "warmup": args.warmup,
           "runs": runs}
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
