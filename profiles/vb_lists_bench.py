#!/usr/bin/env python3
"""Cost of the online VB learner's closed-form lists (sbmf_vb_*) on the
Netflix-shaped synthetic set, K = 200, in the state after one epoch.

Device times are HIP events read through sbmf_vb_timing (the last launch of each kind), after
--warmup calls, in --reps alternating repetitions; every figure is reported as the list of its
repetitions (each the median of --calls calls), not as one value.

  score     k_vb_score, --users users x all items; flops = 3 products x 2 x users x Jp x Kp; also with
            SBMF_VB_SCORE_MU=2 (32 rows a workgroup in the default's place, 16 at Kp > 80)
  accum     k_watch_accum<double> (one product, read-modify-write epilogue) on the same shape,
            the same users and Kp, as the SBPMF sampler's watch list launches it: a sampler on a
            small training set of the same dimensions (the launch reads whole tables: its time
            does not depend on the ratings), sbmf_watch_timing's ms_score
  select    the selection on given moments, topn --topn
  transpose the two tables' transposes, made by the first call after the epoch
  pairs     sbmf_vb_predict on --pairs pairs: host clock around the call (uploads, kernel,
            downloads): no event pair brackets the pair kernel alone
  guest     k_vb_guest for --guests guests whose rating lists are those of training users drawn at
            random (their lengths a sample of the set's user-degree distribution), scans 1 and 8

One JSON line on stdout; --out also writes it to a file.  --bench-this / --bench-parent take files
holding `bench.py --method vb` result lines of this commit and of its parent (taken alternately
in one session) and record their ms_per_step beside it.  Needs an MI355X: there is no CPU path."""
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

from watch_bench import bench_lines, device_sync  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="netflix")
    ap.add_argument("--K", type=int, default=200)
    ap.add_argument("--users", type=int, default=1024)
    ap.add_argument("--guests", type=int, default=1024)
    ap.add_argument("--pairs", type=int, default=1_000_000)
    ap.add_argument("--topn", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3, help="alternating repetitions")
    ap.add_argument("--out", default=None)
    ap.add_argument("--bench-this", nargs="*", default=None)
    ap.add_argument("--bench-parent", nargs="*", default=None)
    args = ap.parse_args()

    from sbmf import Data, FMLearnSBPMF, FMLearnVBOnline, synth
    train, test, dims = synth.generate(args.shape)
    I, J = dims
    Kp, Jp = (args.K + 15) // 16 * 16, (J + 15) // 16 * 16
    rng = np.random.default_rng(2015)
    users = rng.choice(I, args.users, replace=False).astype(np.uint32)
    order = np.argsort(train[0], kind="stable")
    start = np.concatenate([[0], np.cumsum(np.bincount(train[0], minlength=I))])
    rows = [order[start[u]:start[u + 1]] for u in rng.choice(I, args.guests, replace=False)]
    ptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.uint32)
    sel = np.concatenate(rows)
    csr = (ptr, np.ascontiguousarray(train[1][sel], dtype=np.uint32), np.ascontiguousarray(train[2][sel], dtype=np.float64))
    pu = rng.integers(0, I, args.pairs).astype(np.uint32)
    pi = rng.integers(0, J, args.pairs).astype(np.uint32)

    L = FMLearnVBOnline(num_factor=args.K, seed=2015, rng="philox")
    L.set_data(Data(*train), Data(*test), num_users=I, num_items=J)
    L.learn(sweeps=1)
    L.vb_scores(0)
    ms_transpose = L.vb_timing()["ms_transpose"]
    # the sampler whose watch list launches k_watch_accum<double> on the same shape: a thin training set
    thin = rng.choice(len(train[0]), 2_000_000, replace=False)
    W = FMLearnSBPMF(num_factor=args.K, seed=2015, rng="philox", precision="f64", recompute_every=0, eval_train=False)
    W.set_data(Data(train[0][thin], train[1][thin], train[2][thin]), None, num_users=I, num_items=J)
    W.watch(users)
    W.learn(sweeps=args.warmup)

    def med(fn, key, timing):
        out = []
        for _ in range(args.calls):
            fn()
            out.append(timing()[key])
        return statistics.median(out)

    score, score_mu2, select, accum, guest1, guest8, pairs = [], [], [], [], [], [], []
    rec = lambda: L.vb_recommend(users, topn=args.topn)
    for _ in range(args.warmup):
        rec()
        L.vb_foldin_rows(csr, scans=1)
        L.vb_predict(pu, pi)
    for _ in range(args.reps):
        score.append(med(rec, "ms_score", L.vb_timing))
        os.environ["SBMF_VB_SCORE_MU"] = "2"  # 32 rows a workgroup where the default takes 16 (Kp > 80)
        score_mu2.append(med(rec, "ms_score", L.vb_timing))
        del os.environ["SBMF_VB_SCORE_MU"]
        accum.append(med(lambda: W.learn(sweeps=1), "ms_score", W.watch_timing))
        select.append(med(rec, "ms_select", L.vb_timing))
        guest1.append(med(lambda: L.vb_foldin_rows(csr, scans=1), "ms_guest", L.vb_timing))
        guest8.append(med(lambda: L.vb_foldin_rows(csr, scans=8), "ms_guest", L.vb_timing))
        t = []
        for _ in range(args.calls):
            device_sync()
            t0 = time.perf_counter()
            L.vb_predict(pu, pi)
            t.append(1e3 * (time.perf_counter() - t0))
        pairs.append(statistics.median(t))
    flops = 3 * 2.0 * args.users * Jp * Kp
    lens = np.diff(ptr)
    out = {
        "what": "online VB lists, %s K=%d after 1 epoch, %d users, %d guests" % (args.shape, args.K, args.users, args.guests),
        "num_users": I, "num_items": J, "Kp": Kp, "calls": args.calls, "warmup": args.warmup,
        "ms_score": score, "score_tflops": [flops / (m * 1e-3) / 1e12 for m in score],
        "ms_score_forced_mu2": score_mu2,
        "ms_watch_accum_f64": accum, "accum_tflops": [flops / 3 / (m * 1e-3) / 1e12 for m in accum],
        "score_over_accum": [a / b for a, b in zip(score, accum)],
        "topn": args.topn, "ms_select": select, "ms_transpose_first_call": ms_transpose,
        "pairs": args.pairs, "ms_pairs_host": pairs,
        "guest_ratings": int(ptr[-1]), "guest_len_min_median_max": [int(lens.min()), float(np.median(lens)), int(lens.max())],
        "ms_guest_scans1": guest1, "ms_guest_scans8": guest8,
        "bench_py_this_commit": bench_lines(args.bench_this),
        "bench_py_parent_commit": bench_lines(args.bench_parent),
    }
    L.close()
    W.close()
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
