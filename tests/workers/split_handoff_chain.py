"""The Philox chain of the split-row hand-off on ML-100k, as hashes.

chain() runs the cases of tests/test_gpu_split_handoff.py with whatever libsbmf.so the sbmf
package loads and returns, per case, the sha256 of the U and V bytes and the RMSE list after 8
sweeps (so every slab area is used by 16 launches, 15 of them on what an earlier one left).
A run whose split-row hand-off times out raises (learn() reports it).

Run as a script it writes that as JSON: tests/golden/split_handoff_parent.json was made this way
with SBMF_LIB pointing at a build of the commit before the hand-off lost its block counters, so
the test holds every later build to that commit's bits:

    SBMF_LIB=/path/to/parent/libsbmf.so python tests/workers/split_handoff_chain.py OUT.json
"""
import gzip
import hashlib
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
PKG = os.path.join(REPO, "scalable-bayesian-matrix-factorization_amd")
if PKG not in sys.path:
    sys.path.insert(0, PKG)

SEED = 2015
SWEEPS = 8
# tune: default shapes, 4-wave, 16-wave, 8-wave user rows -- each of the 4-, 8- and 16-wave
# kernels on both sides.  split_chunk 16: the longest rows have more than 30 chunks (the 8-deep
# read loop with a remainder, every piece of the chunk sum); 64: 2..16 chunks.
CASES = [(K, chunk, tune, "f64")
         for K in (17, 100)
         for chunk in (16, 64)
         for tune in (0, 128, 1 << 17, 1 << 23)] + [(100, 16, 0, "f32")]


def case_id(K, chunk, tune, prec):
    return "K%d-chunk%d-tune%d-%s" % (K, chunk, tune, prec)


def _triples(name):
    u, i, r = [], [], []
    with gzip.open(os.path.join(REPO, "tests", "golden", name), "rt") as f:
        for line in f:
            a = line.split()
            if len(a) >= 3:
                u.append(int(a[0])); i.append(int(a[1])); r.append(float(a[2]))
    return np.array(u, np.uint32), np.array(i, np.uint32), np.array(r, np.float64)


def run_case(train, test, K, chunk, tune, prec, stages=None):
    from sbmf import Data, FMLearnSBPMF
    old = os.environ.get("SBMF_STAGES")
    if stages is not None:
        os.environ["SBMF_STAGES"] = str(stages)
    try:
        L = FMLearnSBPMF(num_factor=K, seed=SEED, rng="philox", precision=prec, stream_threshold=40,
                         split_chunk=chunk, tune=tune)
        L.set_data(Data(*train), Data(*test))
    finally:
        if stages is not None:
            if old is None:
                del os.environ["SBMF_STAGES"]
            else:
                os.environ["SBMF_STAGES"] = old
    L.learn(sweeps=SWEEPS)
    U, V = L.factors()
    out = {"U": hashlib.sha256(np.ascontiguousarray(U).tobytes()).hexdigest(),
           "V": hashlib.sha256(np.ascontiguousarray(V).tobytes()).hexdigest(),
           "rmse": [float(x) for x in L.rmse_trajectory]}
    L.close()
    return out


def chain(train=None, test=None):
    if train is None:
        train, test = _triples("ml100k_train.tsv.gz"), _triples("ml100k_test.tsv.gz")
    return {case_id(*c): run_case(train, test, *c) for c in CASES}


if __name__ == "__main__":
    res = chain()
    with open(sys.argv[1], "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote %d cases to %s" % (len(res), sys.argv[1]))
