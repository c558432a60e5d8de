#!/usr/bin/env python3
"""Cost of libFM's MCMC chain on cases with any number of features (the general learner,
DESIGN.md 4.3b) on the ML-20M-shaped synthetic, K = 100, f64, Philox normals.

Four settings, in alternating runs (--reps of each):
  (a) the two-attribute learner on the user / item cases (the line bench.py --method libfm times),
  (b) the same cases through the general learner (SBMF_FMM_GENERAL=1): the price of generality,
  (c) the cases with a 7-value and a 24-value one-hot field added ((u + 3 i) mod 7, (5 u + i) mod 24),
  (d) the same with a 5-tag multi-hot field (tag t present when bit t of the item id is set).
A setting followed by a digit runs the same cases with that many attribute groups (libFM's
-meta, set_groups): b2 = users | items through the general learner, c2 / d2 = users | everything
else, c4 = users | items | the 7-value field | the 24-value field with the trailing attribute,
d4 = users | items | the two one-hot fields | the tags.  (a has no grouped form: the
two-attribute kernels keep one group.)
--task c runs the same settings as binary classification (libFM's -task c): the
targets binarised at the train set's median rating (+1 above it, else -1), --method mcmc (Philox
draws of the latent targets in the train frame) or als (their expected values); a run then
reports the test accuracy in place of the RMSE.  The evaluate step (transpose, train and test
frames, their sums) is ms_eval_events, the draws' sweep ms_sweep_events.
Per run: ms per iteration from a host clock around --steps iterations ending in a device
synchronise, after --warmup iterations, and the mean of the iterations' HIP-event times
(sweep + evaluation); launches per iteration and the ranges from fm_info.  One JSON line on
stdout (progress lines start with '#'); --out also writes it to a file.  Needs an MI355X."""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "scalable-bayesian-matrix-factorization_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from watch_bench import bench_lines, device_sync  # noqa: E402


def build_cases(u, i, r, I, J, fields):
    """Cases with the fields 'u' 'i' (one-hot), 'c7' 'c24' (one-hot) and 'tags' (multi-hot), ids
    in that order so every case's entries are sorted."""
    from sbmf import Cases
    u, i = u.astype(np.int64), i.astype(np.int64)
    n = len(u)
    cols, vals, base = [u, I + i], [np.ones(n, np.float32)] * 2, I + J
    if "c7" in fields:
        cols.append(base + (u + 3 * i) % 7)
        vals.append(np.ones(n, np.float32))
        base += 7
    if "c24" in fields:
        cols.append(base + (5 * u + i) % 24)
        vals.append(np.ones(n, np.float32))
        base += 24
    if "tags" in fields:
        ntag = sum(((i >> t) & 1) for t in range(5))
        for t in range(5):
            cols.append(np.where((i >> t) & 1, base + t, -1))
            vals.append(np.where(ntag == 1, 1.0, 0.5).astype(np.float32))
        base += 5
    A = np.stack(cols, axis=1)
    X = np.stack(vals, axis=1)
    keep = A >= 0
    ptr = np.concatenate([[0], np.cumsum(keep.sum(axis=1))]).astype(np.uint64)
    return Cases(ptr, A[keep].astype(np.uint32), X[keep], r.astype(np.float32), num_attr=base)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="ml-20m")
    ap.add_argument("--K", type=int, default=100)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--settings", default="a,b,c,d")
    ap.add_argument("--task", default="r", choices=["r", "c"])
    ap.add_argument("--method", default="mcmc", choices=["mcmc", "als"])
    ap.add_argument("--out", default=None)
    ap.add_argument("--bench-this", nargs="*", default=None)
    ap.add_argument("--bench-parent", nargs="*", default=None)
    args = ap.parse_args()

    from sbmf import Data, FMLearnSBPMF, synth
    train, test, dims = synth.generate(args.shape)
    I, J = int(dims[0]), int(dims[1])
    if args.task == "c":  # binarised at the median of the train ratings
        med = float(np.median(train[2]))
        train = (train[0], train[1], np.where(train[2] > med, 1.0, -1.0))
        test = (test[0], test[1], np.where(test[2] > med, 1.0, -1.0))
        print("# task c: median %g, %.4f of the train cases positive" % (med, float(np.mean(train[2] > 0))), flush=True)
    sets = {}

    def groups(setting, p):
        """The group table of a grouped setting (None for a plain one)."""
        if len(setting) == 1:
            return None
        n = int(setting[1:])
        g = np.zeros(p, np.uint32)
        if setting[0] == "b":  # triples: the attributes are user u -> u, item i -> (largest user id + 1) + i
            g[int(max(train[0].max(), test[0].max())) + 1:] = 1
        elif n == 2:
            g[I:] = 1
        elif n == 4 and setting[0] in "cd":
            g[I:I + J] = 1
            g[I + J:] = 2
            g[I + J + (7 if setting[0] == "c" else 31):] = 3
        else:
            raise SystemExit("no %d-group form of setting %s" % (n, setting[0]))
        return g

    def data(setting):
        if setting not in sets:
            if setting in "ab":
                sets[setting] = (Data(*train), Data(*test))
            else:
                f = ("c7", "c24") if setting == "c" else ("c7", "c24", "tags")
                sets[setting] = tuple(build_cases(d[0], d[1], d[2], I, J, f) for d in (train, test))
        return sets[setting]

    def run(name):
        setting = name[0]
        tr, te = data(setting)
        if name == "b":
            os.environ["SBMF_FMM_GENERAL"] = "1"
        try:
            kw = {"task": "c"} if args.task == "c" else {}  # (a tree without the task runs regression)
            if args.method == "als":
                kw["regular"] = (0.0, 1.0, 10.0)
            L = FMLearnSBPMF(num_factor=args.K, seed=2015, rng="philox", method=args.method, order="libfm",
                             init_stdev=0.1, **kw)
            if len(name) > 1:
                L.set_groups(groups(name, int(max(train[0].max(), test[0].max())) + int(max(train[1].max(), test[1].max())) + 3
                                    if setting == "b" else max(tr.num_attr, te.num_attr) + 1))
            L.set_data(tr, te)
        finally:
            os.environ.pop("SBMF_FMM_GENERAL", None)
        L.learn(sweeps=args.warmup)
        device_sync()
        n0 = len(L.history)
        t0 = time.perf_counter()
        L.learn(sweeps=args.steps)
        device_sync()
        res = {"ms_per_iter_host": 1e3 * (time.perf_counter() - t0) / args.steps,
               "ms_per_iter_events": float(np.mean([h["ms_sweep"] + h["ms_eval"] for h in L.history[n0:]])),
               "ms_sweep_events": float(np.mean([h["ms_sweep"] for h in L.history[n0:]])),
               "ms_eval_events": float(np.mean([h["ms_eval"] for h in L.history[n0:]])),
               "launches_per_iter": int(L.timing().n_launch)}
        if args.task == "c":
            res.update(acc_test=L.history[-1]["acc_avg"], acc_train=L.history[-1]["acc_train"])
        else:
            res["rmse_test"] = L.history[-1]["rmse_avg"]
        if setting != "a":
            info = L.fm_info()
            res.update(num_attr=info["num_attr"], nranges=info["nranges"])
            res["nnz"] = 2 * tr.num_cases if setting == "b" else int(len(tr.attr))
        if len(name) > 1:
            res["groups"] = L.fm_groups()["cnt"].tolist()
        L.close()
        print("# %s %s" % (name, json.dumps(res)), flush=True)
        return res

    names = [s for s in args.settings.split(",") if s]
    runs = {s: [] for s in names}
    for _ in range(args.reps):
        for s in names:
            runs[s].append(run(s))
    out = {"what": "libFM %s%s, %s K=%d f64 philox: (a) two-attribute learner, (b) general learner on the same cases, "
                   "(c) + one-hot fields of 7 and 24 values, (d) + a 5-tag multi-hot field"
                   % (args.method.upper(), " classification (targets binarised at the median)" if args.task == "c" else "",
                      args.shape, args.K),
           "task": args.task, "method": args.method,
           "num_users": I, "num_items": J, "n_train": int(len(train[0])), "steps": args.steps, "warmup": args.warmup,
           "runs": runs,
           "bench_py_this_commit": bench_lines(args.bench_this), "bench_py_parent_commit": bench_lines(args.bench_parent)}
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
