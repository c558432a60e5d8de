#!/usr/bin/env python3
"""Goldens of the classification (-task c) runs of the two libFM learners: bin/libFM (libfm.cpp
compiled unmodified into oracle/_ref/libFM, time() pinned by LIBFM_PIN_TIME, as
tests/make_fm_groups_golden.py runs it) with -task c -dim '1,1,8' on the sets of tests/fm_class.py:
  m1m100k binarised (rating >= 4):  -method mcmc -iter 8;  -method als -regular '0,1,10' -iter 8
  fm4 binarised:                    the same two
  fm4 binarised, the four groups of tests/fm_groups.py as -meta:  -method mcmc -iter 6
  edge_class():                     -method mcmc -iter 5
Stored under tests/golden per run of fm_class.GOLDEN_RUNS: <name>.txt (the "#Iter=" lines as
printed, with the reference's MAP@5 field), <name>_pred.txt.gz (-out), <name>_rlog.txt.gz (-rlog).
And the m1m100k mcmc run at LIBFM_PIN_TIME = 1..16: the final Train and Test accuracies alone
(fm_class.SEEDS_GOLDEN); the reference's seeds 1-8 and 9-16 must meet, against each other, the
bound the GPU's Philox chains are held to against all 16.  Data only; runnable where
oracle/_ref/libFM has been built."""
import json
import os
import shutil
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from conftest import GOLD, REPO, read_triples_text  # noqa: E402
from make_fm_groups_golden import _gz  # noqa: E402
import fm_class  # noqa: E402
import fm_groups  # noqa: E402

# the first lines of the two m1m100k runs, as the issue that asked for this feature quotes them
FIRST = {"ref_libfm_c_mcmc_m1m100k_i8": "#Iter=  0\tTrain=0.688396\tTest=0.675334\tMAP@5= 0",
         "ref_libfm_c_als_m1m100k_i8": "#Iter=  0\tTrain=0.725247\tTest=0.709235"}
LAST = {"ref_libfm_c_mcmc_m1m100k_i8": "#Iter=  7\tTrain=0.714884\tTest=0.711236",
        "ref_libfm_c_als_m1m100k_i8": "#Iter=  7\tTrain=0.78196\tTest=0.724886"}


def _libfm(cwd, trf, tef, method, reg, iters, meta, pin="1", out=True):
    cmd = [os.path.join(REPO, "oracle", "_ref", "libFM"), "-task", "c", "-train", os.path.basename(trf), "-test",
           os.path.basename(tef), "-dim", "1,1,8", "-iter", str(iters), "-method", method]
    if out:
        cmd += ["-out", "pred.txt", "-rlog", "rlog.txt"]
    if meta:
        cmd += ["-meta", "meta.txt"]
    if reg:
        cmd += ["-regular", reg]
    p = subprocess.run(cmd, cwd=cwd, env=dict(os.environ, LIBFM_PIN_TIME=pin), capture_output=True, text=True, check=True)
    lines = [l for l in p.stdout.splitlines() if l.startswith("#Iter=")]
    assert len(lines) == iters, p.stdout[-500:]
    return lines


def main():
    ml100k = (read_triples_text(os.path.join(GOLD, "ml100k_train.tsv.gz")),
              read_triples_text(os.path.join(GOLD, "ml100k_test.tsv.gz")))
    root = tempfile.mkdtemp(prefix="sbmf_fmclass_")
    sets = {}
    for nm in ("fm4", "m1m100k", "edge"):
        os.mkdir(os.path.join(root, nm))
    sets["m1m100k"] = fm_class.write_m1m100k_class(os.path.join(root, "m1m100k"))
    sets["fm4"] = fm_class.write_cases(os.path.join(root, "fm4"), *fm_class.fm4_class(ml100k))
    sets["edge"] = fm_class.write_cases(os.path.join(root, "edge"), *fm_class.edge_class())
    fm_groups.write_meta(os.path.join(root, "fm4", "meta.txt"), fm_groups.fm4_groups(ml100k))
    for name, (dset, method, reg, iters, meta) in fm_class.GOLDEN_RUNS.items():
        trf, tef = sets[dset]
        cwd = os.path.dirname(trf)
        lines = _libfm(cwd, trf, tef, method, reg, iters, meta)
        if name in FIRST:
            assert lines[0].startswith(FIRST[name]) and lines[-1].startswith(LAST[name]), (lines[0], lines[-1])
        with open(os.path.join(GOLD, name + ".txt"), "w") as f:
            f.write("\n".join(lines) + "\n")
        _gz(os.path.join(cwd, "pred.txt"), os.path.join(GOLD, name + "_pred.txt.gz"))
        _gz(os.path.join(cwd, "rlog.txt"), os.path.join(GOLD, name + "_rlog.txt.gz"))
        print("golden", name, lines[-1])
    trf, tef = sets["m1m100k"]
    train, test = [], []
    for pin in range(1, 17):
        tr, te = fm_class.iter_values(_libfm(os.path.dirname(trf), trf, tef, "mcmc", None, 8, False, str(pin), out=False))
        train.append(tr[-1])
        test.append(te[-1])
    # the criterion of the GPU's Philox chains, met by the reference against itself
    assert fm_class.means_agree(train[:8], train[8:]) and fm_class.means_agree(test[:8], test[8:]), (train, test)
    with open(os.path.join(GOLD, fm_class.SEEDS_GOLDEN), "w") as f:
        json.dump({"train": train, "test": test}, f)
        f.write("\n")
    print("seeds", train, test)
    shutil.rmtree(root)


if __name__ == "__main__":
    main()
