#!/usr/bin/env python3
"""Goldens of the attribute-group (-meta) runs of the general libFM learner: bin/libFM
(libfm.cpp compiled unmodified into oracle/_ref/libFM, time() pinned by LIBFM_PIN_TIME, as
tests/make_fm_golden.py runs it) with a -meta file, on
  fm4 in four groups (users, items, field C with its gap id, tags with the trailing attribute):
      -task r -dim '1,1,8' -iter 10 -method mcmc -rlog
      -task r -dim '1,1,8' -iter 10 -method als -regular '0,1,2,3,4,5,10,20,30' -rlog
  the reference's own m1m100k files in two groups (users, items):    -method mcmc -iter 10
  edge_set() (tests/fm_cases.py) in five awkward groups (tests/fm_groups.py): -method mcmc -iter 5
Stored under tests/golden per run of fm_groups.GOLDEN_RUNS: <name>.txt (the "#Iter=" lines),
<name>_pred.txt.gz (the -out file) and <name>_rlog.txt.gz (the -rlog file).  Data only; runnable
where oracle/_ref/libFM has been built."""
import gzip
import os
import shutil
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from conftest import GOLD, REPO, read_libfm_text, read_triples_text, write_m1m100k_libfm  # noqa: E402
import fm_cases  # noqa: E402
import fm_groups  # noqa: E402


def _gz(src, dst):
    with open(src, "rb") as f, gzip.GzipFile(dst, "wb", mtime=0) as g:
        g.write(f.read())


def main():
    ml100k = (read_triples_text(os.path.join(GOLD, "ml100k_train.tsv.gz")),
              read_triples_text(os.path.join(GOLD, "ml100k_test.tsv.gz")))
    m1m = (read_libfm_text(os.path.join(GOLD, "m1m100k_train_libfm.gz")),
           read_libfm_text(os.path.join(GOLD, "m1m100k_test_libfm.gz")))
    root = tempfile.mkdtemp(prefix="sbmf_fmgroups_")
    sets = {}
    for nm in ("fm4", "m1m100k", "edge"):
        os.mkdir(os.path.join(root, nm))
    sets["fm4"] = fm_cases.write_fm4(ml100k, os.path.join(root, "fm4")) + [fm_groups.fm4_groups(ml100k)]
    sets["m1m100k"] = write_m1m100k_libfm(os.path.join(root, "m1m100k")) + [fm_groups.m1m100k_groups(m1m)]
    sets["edge"] = fm_groups.write_edge(os.path.join(root, "edge")) + [fm_groups.edge_groups()]
    for name, (dset, method, reg, iters) in fm_groups.GOLDEN_RUNS.items():
        trf, tef, group = sets[dset]
        cwd = os.path.dirname(trf)
        fm_groups.write_meta(os.path.join(cwd, "meta.txt"), group)
        cmd = [os.path.join(REPO, "oracle", "_ref", "libFM"), "-task", "r", "-train", os.path.basename(trf), "-test",
               os.path.basename(tef), "-dim", "1,1,8", "-iter", str(iters), "-method", method, "-meta", "meta.txt",
               "-out", "pred.txt", "-rlog", "rlog.txt"]
        if reg:
            cmd += ["-regular", reg]
        p = subprocess.run(cmd, cwd=cwd, env=dict(os.environ, LIBFM_PIN_TIME="1"), capture_output=True, text=True,
                           check=True)
        lines = [l for l in p.stdout.splitlines() if l.startswith("#Iter=")]
        assert len(lines) == iters, p.stdout[-500:]
        with open(os.path.join(GOLD, name + ".txt"), "w") as f:
            f.write("\n".join(lines) + "\n")
        _gz(os.path.join(cwd, "pred.txt"), os.path.join(GOLD, name + "_pred.txt.gz"))
        _gz(os.path.join(cwd, "rlog.txt"), os.path.join(GOLD, name + "_rlog.txt.gz"))
        print("golden", name, lines[-1])
    shutil.rmtree(root)


if __name__ == "__main__":
    main()
