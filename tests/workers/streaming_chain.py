"""The Philox chain of the streaming row kernels on ML-100k, as hashes.

chain() runs the cases of tests/test_gpu_streaming_regs.py::test_chain_identical_to_parent
with whatever libsbmf.so the sbmf package loads and returns, per case, the sha256 of the U and
V bytes and the RMSE list after 3 sweeps.

Run as a script it writes that as JSON: tests/golden/streaming_chain_parent.json was made this
way with SBMF_LIB pointing at a build of the commit before the kernels' hot / cold argument
split, so the test holds every later build to that commit's bits:

    SBMF_LIB=/path/to/parent/libsbmf.so python tests/workers/streaming_chain.py OUT.json
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
SWEEPS = 3
CASES = [(K, name, kw, prec)
         for K in (16, 100)
         for name, kw in (("default", {}), ("split16", {"stream_threshold": 40, "split_chunk": 16}))
         for prec in ("f64", "f32")]


def case_id(K, name, prec):
    return "K%d-%s-%s" % (K, name, prec)


def _triples(name):
    u, i, r = [], [], []
    with gzip.open(os.path.join(REPO, "tests", "golden", name), "rt") as f:
        for line in f:
            a = line.split()
            if len(a) >= 3:
                u.append(int(a[0])); i.append(int(a[1])); r.append(float(a[2]))
    return np.array(u, np.uint32), np.array(i, np.uint32), np.array(r, np.float64)


def run_case(train, test, K, kw, prec):
    from sbmf import Data, FMLearnSBPMF
    L = FMLearnSBPMF(num_factor=K, seed=SEED, rng="philox", precision=prec, **kw)
    L.set_data(Data(*train), Data(*test))
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
    return {case_id(K, name, prec): run_case(train, test, K, kw, prec) for K, name, kw, prec in CASES}


if __name__ == "__main__":
    res = chain()
    with open(sys.argv[1], "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote %d cases to %s" % (len(res), sys.argv[1]))
