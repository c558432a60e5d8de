#!/usr/bin/env python3
"""Cost of the libFM learner's query list (sbmf_fm_query_cases) on the ML-20M-shaped
synthetic, K = 100, f64, Philox normals, in profiles/fmr_bench.py's dBr setting: no main features, a
user relation (id, 24-value field, 5 tags) and an item relation (id, 7-value field, 5 tags; 26,744
block rows), the cases ordered by relation 0's block row.  --queries queries (a user block row each,
no main feature) against the item relation.

One context; after --warmup iterations the phases alternate, --reps times: --steps iterations
without a list, then --steps with it (registered anew, so every phase accumulates from zero).  Per
phase the mean of the iterations' HIP-event times (ms_sweep + ms_eval) and the host clock; with the
list also sbmf_fm_query_timing's launches: the terms and operand copy (two launches, one figure),
the scoring launch, and the selection of --topn.  A last phase registers ONE query: its terms
launch is a single wave, so its figure is the operand copy's.  One JSON line on stdout (progress
lines start with '#'); --out also writes it to a file.  Needs an MI355X."""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "scalable-bayesian-matrix-factorization_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from fmr_bench import entity_fields, to_cases  # noqa: E402
from watch_bench import device_sync  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="ml-20m")
    ap.add_argument("--K", type=int, default=100)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--queries", type=int, default=1024)
    ap.add_argument("--topn", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    from sbmf import Cases, FMLearnSBPMF, Relation, synth
    train, test, dims = synth.generate(args.shape)
    I, J = int(dims[0]), int(dims[1])
    UA, UX, pu = entity_fields(I, 24, True)
    IA, IX, pi = entity_fields(J, 7, True)
    ublock, iblock = to_cases(UA, UX, np.zeros(I), pu), to_cases(IA, IX, np.zeros(J), pi)
    empty = lambda n, y: to_cases(np.full((n, 1), -1, np.int64), np.zeros((n, 1), np.float32), y, 0)
    os.environ["SBMF_FMG_CASE_ORDER"] = "relation"
    L = FMLearnSBPMF(num_factor=args.K, seed=2015, rng="philox", method="mcmc", order="libfm", init_stdev=0.1)
    L.add_relation(Relation(ublock, train[0], test[0]))
    L.add_relation(Relation(iblock, train[1], test[1]))
    L.set_data(empty(len(train[0]), train[2]), empty(len(test[0]), test[2]))
    os.environ.pop("SBMF_FMG_CASE_ORDER", None)
    L.learn(sweeps=args.warmup)
    device_sync()

    def queries(n):
        rows = (np.arange(n, dtype=np.int64) * 7919 % I).astype(np.uint32)
        return Cases(np.zeros(n + 1, np.uint64), [], [], np.zeros(n, np.float32)), rows

    def phase(nq):
        if nq:
            qc, rows = queries(nq)
            L.fm_queries(1, qc, rows=[rows, None])
        else:
            L.fm_queries(1, Cases([0], [], [], []))
        device_sync()
        n0 = len(L.history)
        t0 = time.perf_counter()
        L.learn(sweeps=args.steps)
        device_sync()
        h = L.history[n0:]
        res = {"queries": nq, "ms_per_iter_host": 1e3 * (time.perf_counter() - t0) / args.steps,
               "ms_per_iter_events": float(np.mean([x["ms_sweep"] + x["ms_eval"] for x in h])),
               "ms_eval_events": float(np.mean([x["ms_eval"] for x in h])),
               "launches_per_iter": L.fm_info()["launches_per_iter"]}
        if nq:
            L.fm_query_recommend(topn=args.topn)
            res.update(L.fm_query_timing())
        print("# %s" % json.dumps(res), flush=True)
        return res

    runs = {"without": [], "with": []}
    for _ in range(args.reps):
        runs["without"].append(phase(0))
        runs["with"].append(phase(args.queries))
    one = phase(1)
    nbp = (J + 15) // 16 * 16
    out = {"what": "libFM MCMC, %s K=%d f64 philox, dBr: %d queries against the item relation's %d block rows"
                   % (args.shape, args.K, args.queries, J),
           "num_users": I, "num_items": J, "n_train": int(len(train[0])), "steps": args.steps, "warmup": args.warmup,
           "table_bytes_per_iter": 4 * args.queries * nbp * 8, "runs": runs, "one_query": one}
    L.close()
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
