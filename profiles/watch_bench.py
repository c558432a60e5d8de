#!/usr/bin/env python3
"""Cost of a watch list (sbmf_watch_users) on the ML-20M-shaped synthetic,
K = 100, f64, Philox -- the learner bench.py times, with the same settings.

Reports ms per sweep (host clock around a run of --steps sweeps ending in a device
synchronise, after --warmup sweeps) without a watch list and with --users watched users,
the scoring launch's device time (sbmf_watch_timing, HIP events; the median over the timed
sweeps), its accumulator traffic 4 n Jp 8 bytes (read + write of both sums) as a fraction
of the 8 TB/s HBM peak, and the selection's device time for --topn.  One JSON line on stdout;
--out also writes it to a file.  --bench-this / --bench-parent take files holding
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

HBM_PEAK = 8.0e12  # bytes/s


_HIP = None


def device_sync():
    """hipDeviceSynchronize through the HIP runtime libsbmf is bound to (as bench.py does)."""
    global _HIP
    if _HIP is None:
        import ctypes
        from sbmf import _lib  # noqa: F401  (binds libamdhip64.so.7)
        _HIP = ctypes.CDLL("libamdhip64.so.7")
    if _HIP.hipDeviceSynchronize() != 0:
        raise RuntimeError("hipDeviceSynchronize failed")


def bench_lines(paths):
    out = []
    for p in paths or []:
        with open(p) as f:
            for line in f:
                if line.startswith("{"):
                    r = json.loads(line)
                    out.append({"file": os.path.basename(p), "ms_per_step": r["ms_per_step"], "value": r["value"],
                                "steps": r["steps"], "warmup": r["warmup"]})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="ml-20m")
    ap.add_argument("--K", type=int, default=100)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--users", type=int, default=1024)
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
    users = np.random.default_rng(2015).choice(dims[0], args.users, replace=False).astype(np.uint32)
    Jp = (dims[1] + 15) // 16 * 16

    def run(watch):
        L = FMLearnSBPMF(num_factor=args.K, seed=2015, rng="philox", precision="f64", recompute_every=0,
                         eval_train=False, pipeline=1)
        L.set_data(Data(*train), Data(*test))
        if watch:
            L.watch(users)
        L.learn(sweeps=args.warmup)
        device_sync()
        score = []

        def cb(_rec):  # pipeline = 1: the callback reads no device state; the events are the last finished sweep's
            if watch:
                score.append(L.watch_timing()["ms_score"])
            return False

        t0 = time.perf_counter()
        L.learn(sweeps=args.steps, callback=cb)
        device_sync()
        ms = 1e3 * (time.perf_counter() - t0) / args.steps
        res = {"ms_per_sweep": ms}
        if watch:
            res["ms_score"] = statistics.median(score)
            sel = []
            for _ in range(3):
                L.recommend(topn=args.topn)
                sel.append(L.watch_timing()["ms_select"])
            res["ms_select"] = statistics.median(sel)
        L.close()
        return res

    plain, watched = [], []
    for _ in range(args.reps):
        plain.append(run(False))
        watched.append(run(True))
    nbytes = 4 * args.users * Jp * 8
    ms_score = statistics.median(r["ms_score"] for r in watched)
    out = {
        "what": "watch list cost, %s K=%d f64 philox, %d watched users" % (args.shape, args.K, args.users),
        "num_users": dims[0], "num_items": dims[1], "Jp": Jp, "steps": args.steps, "warmup": args.warmup,
        "ms_per_sweep_no_watch": [r["ms_per_sweep"] for r in plain],
        "ms_per_sweep_watch": [r["ms_per_sweep"] for r in watched],
        "ms_score": [r["ms_score"] for r in watched],
        "score_bytes": nbytes,
        "score_frac_of_8TBs": nbytes / (ms_score * 1e-3) / HBM_PEAK,
        "topn": args.topn,
        "ms_select": [r["ms_select"] for r in watched],
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
