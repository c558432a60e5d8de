#!/usr/bin/env python3
"""Guests folded into the posterior sample store after the run (sbmf_samples_foldin_recommend,
DESIGN.md 4.8) on the ML-20M-shaped synthetic, K = 100, f64, Philox.

1. The call: --guests guests (copies of the rating lists of training users drawn at random, as
   foldin_bench.py draws them) against --samples stored samples of a chain of the quirk set `none`
   (the headline set `final` collapses from sweep 28, bench.py CHAIN_SWEEPS).  The draw by the fused
   kernel (k_samples_foldin: the sample loop inside one launch; test hook bit 1) and by its unfused
   twin (one launch of k_samples_foldin_step per sample and scan), scans = 1 and 4, in alternating runs
   after a warm-up round; device times by HIP events (sbmf_samples_foldin_timing), the call's wall
   clock beside them.  The draw's algorithmic bytes are the in-chain draw's per sample and scan --
   per rating one residual and two passes over the row's Kp / 16 slices of 16 doubles,
   sum_g n_g (1 + 2 Kp / 16) 16 8 -- plus the rows written once per sample; over its time as a
   fraction of the 8 TB/s HBM peak (a latency chain per guest: no roofline share is a target).
2. Cost to the chain of keeping the hyperparameters: the headline configuration (quirks final,
   pipeline = 1), ms per sweep (host clock around --steps sweeps ending in a device synchronise,
   after --warmup sweeps) with no store and with every = 1, in alternating runs.
One JSON line on stdout; --out also writes it to a file.  --bench-this / --bench-parent take files
holding bench.py result lines of this commit and of its parent (taken alternately in one session),
--chain-parent a file holding part 2's numbers taken with the parent's library (--chain-only
prints them; $SBMF_PKG names the package directory to import in place of this tree's), and record
them beside it.  Needs an MI355X: there is no CPU path."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.environ.get("SBMF_PKG", os.path.join(REPO, "scalable-bayesian-matrix-factorization_amd")))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from watch_bench import HBM_PEAK, bench_lines, device_sync  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="ml-20m")
    ap.add_argument("--K", type=int, default=100)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--guests", type=int, default=1024)
    ap.add_argument("--samples", type=int, default=32)
    ap.add_argument("--topn", type=int, default=100)
    ap.add_argument("--reps", type=int, default=3, help="alternating repetitions of the timed runs")
    ap.add_argument("--out", default=None)
    ap.add_argument("--chain-only", action="store_true", help="part 2 alone (runs with the parent's library too)")
    ap.add_argument("--chain-parent", default=None)
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

    # ---- 2. the cost to the chain
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
        ms = 1e3 * (time.perf_counter() - t0) / args.steps
        L.close()
        return ms

    cost = {0: [], 1: []}
    for _ in range(args.reps):
        for every in cost:
            cost[every].append(run(every))
    chain = {"steps": args.steps, "warmup": args.warmup, "ms_per_sweep_no_store": cost[0], "ms_per_sweep_every_1": cost[1]}
    if args.chain_only:
        line = json.dumps(chain)
        print(line, flush=True)
        if args.out:
            with open(args.out, "w") as f:
                f.write(line + "\n")
        return

    # ---- 1. the call
    order = np.argsort(train[0], kind="stable")
    start = np.concatenate([[0], np.cumsum(np.bincount(train[0], minlength=I))])
    src = np.random.default_rng(2015).choice(I, args.guests, replace=False)
    rows = [order[start[u]:start[u + 1]] for u in src]
    ptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.uint32)
    sel = np.concatenate(rows)
    csr = (ptr, np.ascontiguousarray(train[1][sel], dtype=np.uint32), np.ascontiguousarray(train[2][sel], dtype=np.float64))
    nnz, n, S = int(ptr[-1]), args.guests, args.samples
    L = FMLearnSBPMF(num_factor=args.K, seed=2015, rng="philox", precision="f64", quirks="none", recompute_every=0,
                     eval_train=False, pipeline=1)
    L.set_data(Data(*train), Data(*test))
    L.keep_samples(every=1, cap=S)
    L.learn(sweeps=S)
    assert L.samples_info()["count"] == S
    res, same = {}, True
    for scans in (1, 4):
        ms = {0: {"draw": [], "score": [], "select": [], "wall": []}, 1: {"draw": [], "score": [], "select": [], "wall": []}}
        lists = {}
        for rep in range(args.reps + 1):  # the first round warms both paths up
            for unfused in (0, 1):
                assert lib.sbmf_test_samples_tune(L.ctx, 0, 0 if unfused else 2) == 0
                device_sync()
                t0 = time.perf_counter()
                lists[unfused] = L.samples_foldin_recommend(csr, topn=args.topn, scans=scans)
                wall = 1e3 * (time.perf_counter() - t0)
                t = L.samples_foldin_timing()
                if rep:
                    for k, v in (("draw", t["ms_draw"]), ("score", t["ms_score"]), ("select", t["ms_select"]), ("wall", wall)):
                        ms[unfused][k].append(v)
        same = same and all(np.array_equal(a, b, equal_nan=True) for a, b in zip(lists[0], lists[1]))
        draw_bytes = S * (scans * nnz * (1 + 2 * Kp // 16) * 16 * 8 + n * Kp * 8)
        med, medu = statistics.median(ms[0]["draw"]), statistics.median(ms[1]["draw"])
        res["scans_%d" % scans] = {
            "ms_draw_fused": ms[0]["draw"], "ms_draw_unfused": ms[1]["draw"],
            "unfused_over_fused": medu / med,
            "ms_draw_fused_per_sample_and_scan": med / (S * scans),
            "ms_draw_unfused_per_sample_and_scan": medu / (S * scans),
            "draw_bytes": draw_bytes, "draw_frac_of_8TBs_fused": draw_bytes / (med * 1e-3) / HBM_PEAK,
            "draw_frac_of_8TBs_unfused": draw_bytes / (medu * 1e-3) / HBM_PEAK,
            "ms_score": ms[1]["score"], "ms_select": ms[1]["select"],
            "ms_call_wall_fused": ms[0]["wall"], "ms_call_wall_unfused": ms[1]["wall"],
        }
    assert lib.sbmf_test_samples_tune(L.ctx, 0, 0) == 0
    L.close()
    parent = None
    if args.chain_parent:
        with open(args.chain_parent) as f:
            parent = json.loads(f.read())
    out = {
        "what": "guests from the sample store, %s K=%d f64 philox: %d guests x %d items over %d samples"
                % (args.shape, args.K, n, J, S),
        "num_users": I, "num_items": J, "Kp": Kp, "Jp": Jp, "guest_ratings": nnz,
        "guest_len_min_median_max": [int(np.diff(ptr).min()), float(np.median(np.diff(ptr))), int(np.diff(ptr).max())],
        "topn": args.topn, "lists_bit_identical": same, **res,
        "chain_this_commit": chain, "chain_parent_commit": parent,
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
