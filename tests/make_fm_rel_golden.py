#!/usr/bin/env python3
"""Goldens of the -relation runs: bin/libFM (libfm.cpp compiled unmodified into oracle/_ref/libFM,
time() pinned by LIBFM_PIN_TIME, as tests/make_fm_golden.py runs it) with -relation on the sets
of tests/fm_rel.py.  The block tables go through the reference's own convert and transpose tools
(oracle/_ref/convert, oracle/_ref/transpose) into <stem>.x / <stem>.xt; the maps are text.
Stored under tests/golden per run of fm_rel.GOLDEN_RUNS: <name>.txt (libFM's "#relations", "#attr"
and "#Iter=" lines) and <name>_pred.txt.gz (the -out file).  Data only; runnable where the
reference binaries have been built."""
import gzip
import os
import shutil
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from conftest import GOLD, REPO, read_triples_text  # noqa: E402
import fm_rel  # noqa: E402

REF = os.path.join(REPO, "oracle", "_ref")


def main():
    ml100k = (read_triples_text(os.path.join(GOLD, "ml100k_train.tsv.gz")),
              read_triples_text(os.path.join(GOLD, "ml100k_test.tsv.gz")))
    for name, (dset, method, task, iters) in fm_rel.GOLDEN_RUNS.items():
        S = fm_rel.golden_set(dset, ml100k)
        cwd = tempfile.mkdtemp(prefix="sbmf_fmrel_")
        stems = fm_rel.write_set(S, cwd)
        for s in stems:
            subprocess.run([os.path.join(REF, "convert"), "--ifile", s + ".libfm", "--ofilex", s + ".x", "--ofiley", s + ".y"],
                           cwd=cwd, check=True, capture_output=True)
            subprocess.run([os.path.join(REF, "transpose"), "--ifile", s + ".x", "--ofile", s + ".xt"], cwd=cwd, check=True,
                           capture_output=True)
        cmd = [os.path.join(REF, "libFM"), "-task", task, "-train", "train.libfm", "-test", "test.libfm", "-dim", "1,1,8",
               "-iter", str(iters), "-method", method, "-relation", ",".join(stems), "-out", "pred.txt", "-verbosity", "1"]
        if S.main_group is not None:
            cmd += ["-meta", "meta.txt"]
        if method == "als":
            cmd += ["-regular", ",".join("%g" % x for x in fm_rel.als_regular(S.num_groups))]
        p = subprocess.run(cmd, cwd=cwd, env=dict(os.environ, LIBFM_PIN_TIME="1"), capture_output=True, text=True)
        assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-2000:])
        keep = [l for l in p.stdout.splitlines() if l.startswith(("#Iter=", "#relations", "#attr", "num_cases="))]
        assert sum(l.startswith("#Iter=") for l in keep) == iters, p.stdout[-1000:]
        with open(os.path.join(GOLD, name + ".txt"), "w") as f:
            f.write("\n".join(keep) + "\n")
        with open(os.path.join(cwd, "pred.txt"), "rb") as f, gzip.GzipFile(os.path.join(GOLD, name + "_pred.txt.gz"), "wb",
                                                                         mtime=0) as g:
            g.write(f.read())
        print("golden", name, keep[-1])
        shutil.rmtree(cwd)


if __name__ == "__main__":
    main()
