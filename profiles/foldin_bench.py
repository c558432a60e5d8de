#!/usr/bin/env python3
"""Cost of a fold-in list (sbmf_foldin_users) on the ML-20M-shaped synthetic,
K = 100, f64, Philox, pipeline = 1 -- the learner bench.py times, with the same settings.

The --guests guests are copies of the rating lists of training users drawn at random, so
their lengths are a sample of the training users' degree distribution.  Reports ms per
sweep (host clock around a run of --steps sweeps ending in a device synchronise, after
--warmup sweeps) without a list and with the fold-in list, in alternating runs; the draw,
scoring and selection device times (sbmf_foldin_timing, HIP events; the median over the
timed sweeps); and the draw's algorithmic bytes -- per rating one residual and two passes
over the row's Kp / 16 slices of 16 doubles, sum_g n_g (1 + 2 Kp / 16) 16 8, plus the rows
read and written -- over its time as a fraction of the 8 TB/s HBM peak.  One JSON line on
stdout; --out also writes it to a file.  --bench-this / --bench-parent take files holding
bench.py result lines of this commit and of its parent (taken alternately in one session)
and record their ms_per_step beside it.  Needs an MI355X: there is no CPU path."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "scalable-bayesian-matrix-factorization_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from watch_bench import HBM_PEAK, bench_lines, device_sync  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="ml-20m")
    ap.add_argument("--K", type=int, default=100)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--guests", type=int, default=1024)
    ap.add_argument("--topn", type=int, default=100)
    ap.add_argument("--reps", type=int, default=3, help="alternating repetitions of the two timed runs")
    ap.add_argument("--out", default=None)
    ap.add_argument("--bench-this", nargs="*", default=None)
    ap.add_argument("--bench-parent", nargs="*", default=None)
    args = ap.parse_args()
    if args.warmup + args.steps > 24:  # the headline chain collapses from sweep 28 (bench.py CHAIN_SWEEPS)
        ap.error("warmup + steps must stay within 24 sweeps")

    from sbmf import Data, FMLearnSBPMF, synth
    train, test, dims = synth.generate(args.shape)
    order = np.argsort(train[0], kind="stable")
    start = np.concatenate([[0], np.cumsum(np.bincount(train[0], minlength=dims[0]))])
    src = np.random.default_rng(2015).choice(dims[0], args.guests, replace=False)
    rows = [order[start[u]:start[u + 1]] for u in src]
    ptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.uint32)
    sel = np.concatenate(rows)
    csr = (ptr, np.ascontiguousarray(train[1][sel], dtype=np.uint32), np.ascontiguousarray(train[2][sel], dtype=np.float64))
    Kp = (args.K + 15) // 16 * 16
    nnz = int(ptr[-1])
    draw_bytes = nnz * (1 + 2 * Kp // 16) * 16 * 8 + 2 * args.guests * Kp * 8

    def run(fold):
        L = FMLearnSBPMF(num_factor=args.K, seed=2015, rng="philox", precision="f64", recompute_every=0,
                         eval_train=False, pipeline=1)
        L.set_data(Data(*train), Data(*test))
        if fold:
            L.foldin(csr)
        L.learn(sweeps=args.warmup)
        device_sync()
        draw, score = [], []

        def cb(_rec):  # the events are the last finished sweep's
            if fold:
                t = L.foldin_timing()
                draw.append(t["ms_draw"])
                score.append(t["ms_score"])
            return False

        # (the callback's timing read waits for the queued sweep: ms_per_sweep is taken in a run without it)
        t0 = time.perf_counter()
        L.learn(sweeps=args.steps)
        device_sync()
        ms = 1e3 * (time.perf_counter() - t0) / args.steps
        res = {"ms_per_sweep": ms}
        if fold:
            L.learn(sweeps=3, callback=cb)
            res["ms_draw"] = statistics.median(draw)
            res["ms_score"] = statistics.median(score)
            s = []
            for _ in range(3):
                L.foldin_recommend(topn=args.topn)
                s.append(L.foldin_timing()["ms_select"])
            res["ms_select"] = statistics.median(s)
        L.close()
        return res

    plain, folded = [], []
    for _ in range(args.reps):
        plain.append(run(False))
        folded.append(run(True))
    ms_draw = statistics.median(r["ms_draw"] for r in folded)
    out = {
        "what": "fold-in list cost, %s K=%d f64 philox pipeline=1, %d guests" % (args.shape, args.K, args.guests),
        "num_users": dims[0], "num_items": dims[1], "Kp": Kp, "steps": args.steps, "warmup": args.warmup,
        "guest_ratings": nnz, "guest_len_min_median_max": [int(np.diff(ptr).min()), float(np.median(np.diff(ptr))),
                                                            int(np.diff(ptr).max())],
        "ms_per_sweep_no_list": [r["ms_per_sweep"] for r in plain],
        "ms_per_sweep_foldin": [r["ms_per_sweep"] for r in folded],
        "ms_draw": [r["ms_draw"] for r in folded],
        "ms_score": [r["ms_score"] for r in folded],
        "draw_bytes": draw_bytes,
        "draw_frac_of_8TBs": draw_bytes / (ms_draw * 1e-3) / HBM_PEAK,
        "topn": args.topn,
        "ms_select": [r["ms_select"] for r in folded],
        "bench_py_this_commit": bench_lines(args.bench_this),
        "bench_py_parent_commit": bench_lines(args.bench_parent),
    }
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
