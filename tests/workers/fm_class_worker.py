"""One rank of a two-rank libFM MCMC learner asked for classification (spawned by
tests/test_gpu_fm_class.py): sbmf_prepare must refuse, on every rank, before anything is exchanged.

usage: python fm_class_worker.py <rank> <nranks> <id-hex>
Prints "refused <code>: <message>" and exits 0 when the learner refuses."""
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(REPO, "scalable-bayesian-matrix-factorization_amd"))


def main():
    rank, nranks, idhex = sys.argv[1:4]
    from sbmf import Data, FMLearnSBPMF, SBMFError
    n = 64
    u, i = np.arange(n, dtype=np.uint32) % 8, (np.arange(n, dtype=np.uint32) * 3) % 5
    y = np.where(np.arange(n) % 3 == 0, -1.0, 1.0)
    L = FMLearnSBPMF(num_factor=4, seed=1, method="mcmc", order="libfm", init_stdev=0.1, task="c", device=0)
    L.init(comm=(int(nranks), int(rank), bytes.fromhex(idhex)))
    try:
        L.set_data(Data(u, i, y), Data(u[:8], i[:8], y[:8]))
    except SBMFError as e:
        print("refused %d: %s" % (e.code, e))
        return 0
    print("not refused")
    return 1


if __name__ == "__main__":
    sys.exit(main())
