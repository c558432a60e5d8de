#!/usr/bin/env python3
"""Goldens of the general libFM learner: bin/libFM (libfm.cpp compiled unmodified into
oracle/_ref/libFM, time() pinned by LIBFM_PIN_TIME, as oracle/make_golden.py libfm runs it) on
the four-field set "fm4" of tests/fm_cases.py:
  -task r -dim '1,1,8' -iter 10 -method mcmc                      and
  -task r -dim '1,1,8' -iter 10 -method als -regular '0,0,10'.
Stored under tests/golden: ref_libfm_<method>_fm4_d118_s1_i10.txt (the "#Iter=" lines) and
ref_libfm_<method>_fm4_d118_s1_i10_pred.txt.gz (the -out file).  Data only; runnable where
oracle/_ref/libFM has been built."""
import gzip
import os
import shutil
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from conftest import GOLD, REPO, read_triples_text  # noqa: E402
import fm_cases  # noqa: E402

RUNS = [("mcmc", None), ("als", "0,0,10")]


def golden_name(method):
    return "ref_libfm_%s_fm4_d118_s1_i10" % method


def main():
    ml100k = (read_triples_text(os.path.join(GOLD, "ml100k_train.tsv.gz")),
              read_triples_text(os.path.join(GOLD, "ml100k_test.tsv.gz")))
    root = tempfile.mkdtemp(prefix="sbmf_fm4_")
    fm_cases.write_fm4(ml100k, root)
    for method, reg in RUNS:
        cmd = [os.path.join(REPO, "oracle", "_ref", "libFM"), "-task", "r", "-train", "train.libfm", "-test",
               "test.libfm", "-dim", "1,1,8", "-iter", "10", "-method", method, "-out", "pred.txt"]
        if reg:
            cmd += ["-regular", reg]
        p = subprocess.run(cmd, cwd=root, env=dict(os.environ, LIBFM_PIN_TIME="1"), capture_output=True, text=True,
                           check=True)
        lines = [l for l in p.stdout.splitlines() if l.startswith("#Iter=")]
        assert len(lines) == 10, p.stdout[-500:]
        with open(os.path.join(GOLD, golden_name(method) + ".txt"), "w") as f:
            f.write("\n".join(lines) + "\n")
        with open(os.path.join(root, "pred.txt"), "rb") as f, \
                gzip.GzipFile(os.path.join(GOLD, golden_name(method) + "_pred.txt.gz"), "wb", mtime=0) as g:
            g.write(f.read())
        print("golden", golden_name(method), lines[-1])
    shutil.rmtree(root)


if __name__ == "__main__":
    main()
