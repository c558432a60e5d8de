#!/usr/bin/env python3
"""The posterior sample store (sbmf_keep_samples) on the ML-20M-shaped synthetic,
K = 100, f64, Philox.

1. Scoring: --users users against every item over --samples stored samples, by the fused kernel
   (k_samples_score: both sums in registers over the sample loop) and by the obvious alternative
   (test hook: one launch of the watch list's kernel per sample, the sums passing through memory),
   in alternating runs, device time by HIP events (sbmf_samples_timing).  The samples come from a
   chain of the quirk set `none` (the headline set `final` collapses from sweep 28, bench.py
   CHAIN_SWEEPS; the scoring reads the same tables either way).  The fused kernel's algorithmic
   bytes -- per sample V once and the users' rows, plus both sums written once -- over its time as
   a fraction of the 8 TB/s HBM peak; the loop's bytes add both sums read and written per sample.
2. The store's cost to the chain: the headline configuration (quirks final, pipeline = 1), ms per
   sweep (host clock around --steps sweeps ending in a device synchronise, after --warmup sweeps)
   with no store, with every = 10 and with every = 1, in alternating runs, and the copy's own
   device time.
One JSON line on stdout; --out also writes it to a file.  --bench-this / --bench-parent take files
holding bench.py result lines of this commit and of its parent (taken alternately in one session)
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
    ap.add_argument("--users", type=int, default=1024)
    ap.add_argument("--samples", type=int, default=32)
    ap.add_argument("--topn", type=int, default=100)
    ap.add_argument("--reps", type=int, default=3, help="alternating repetitions of the timed runs")
    ap.add_argument("--out", default=None)
    ap.add_argument("--bench-this", nargs="*", default=None)
    ap.add_argument("--bench-parent", nargs="*", default=None)
    args = ap.parse_args()
    if args.warmup + args.steps > 24:  # the headline chain collapses from sweep 28 (bench.py CHAIN_SWEEPS)
        ap.error("warmup + steps must stay within 24 sweeps")

    from sbmf import Data, FMLearnSBPMF, synth
    from sbmf._lib import lib
    train, test, dims = synth.generate(args.shape)
    I, J = dims
    Kp, Jp = (args.K + 15) // 16 * 16, (J + 15) // 16 * 16
    users = np.random.default_rng(2015).choice(I, args.users, replace=False).astype(np.uint32)

    # ---- 1. scoring
    L = FMLearnSBPMF(num_factor=args.K, seed=2015, rng="philox", precision="f64", quirks="none", recompute_every=0,
                     eval_train=False, pipeline=1)
    L.set_data(Data(*train), Data(*test))
    L.keep_samples(every=1, cap=args.samples)
    L.learn(sweeps=args.samples)
    info = L.samples_info()
    assert info["count"] == args.samples
    ms = {0: [], 1: []}
    select, lists = [], {}
    for rep in range(args.reps + 1):  # the first round warms both paths up
        for unfused in (0, 1):
            assert lib.sbmf_test_samples_tune(L.ctx, 0, unfused) == 0
            lists[unfused] = L.samples_recommend(users, topn=args.topn)
            t = L.samples_timing()
            if rep:
                ms[unfused].append(t["ms_score"])
                select.append(t["ms_select"])
    same = all(np.array_equal(a, b, equal_nan=True) for a, b in zip(lists[0], lists[1]))
    u16 = (np.arange(1 << 16) % I).astype(np.uint32)  # the pair kernel: 65,536 pairs (a first call warms it up)
    i16 = (np.arange(1 << 16) * 7919 % J).astype(np.uint32)
    L.samples_predict(u16, i16)
    t0 = time.perf_counter()
    L.samples_predict(u16, i16)
    ms_pairs_wall = 1e3 * (time.perf_counter() - t0)
    L.close()
    n, S = args.users, args.samples
    fused_bytes = S * (J * Kp * 8 + n * Kp * 8) + 2 * n * Jp * 8
    loop_bytes = S * (J * Kp * 8 + n * Kp * 8 + 4 * n * Jp * 8)

    # ---- 2. the store's cost to the chain
    def run(every):
        L = FMLearnSBPMF(num_factor=args.K, seed=2015, rng="philox", precision="f64", recompute_every=0,
                         eval_train=False, pipeline=1)
        L.set_data(Data(*train), Data(*test))
        if every:
            L.keep_samples(every=every, cap=4)
        L.learn(sweeps=args.warmup)
        device_sync()
        t0 = time.perf_counter()
        L.learn(sweeps=args.steps)
        device_sync()
        res = {"ms_per_sweep": 1e3 * (time.perf_counter() - t0) / args.steps}
        if every:
            res["ms_copy"] = L.samples_timing()["ms_copy"]
        L.close()
        return res

    cost = {0: [], 10: [], 1: []}
    for _ in range(args.reps):
        for every in cost:
            cost[every].append(run(every))
    out = {
        "what": "sample store, %s K=%d f64 philox: %d users x %d items over %d samples" % (args.shape, args.K, n, J, S),
        "num_users": I, "num_items": J, "Kp": Kp, "sample_bytes": info["bytes"] // info["cap"],
        "ms_score_fused": ms[0], "ms_score_per_sample_loop": ms[1], "lists_bit_identical": same,
        "fused_bytes": fused_bytes, "fused_frac_of_8TBs": fused_bytes / (statistics.median(ms[0]) * 1e-3) / HBM_PEAK,
        "loop_bytes": loop_bytes, "loop_frac_of_8TBs": loop_bytes / (statistics.median(ms[1]) * 1e-3) / HBM_PEAK,
        "topn": args.topn, "ms_select": select, "ms_predict_65536_pairs_wall": ms_pairs_wall,
        "steps": args.steps, "warmup": args.warmup,
        "ms_per_sweep_no_store": [r["ms_per_sweep"] for r in cost[0]],
        "ms_per_sweep_every_10": [r["ms_per_sweep"] for r in cost[10]],
        "ms_per_sweep_every_1": [r["ms_per_sweep"] for r in cost[1]],
        "ms_copy": [r["ms_copy"] for r in cost[1]],
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
