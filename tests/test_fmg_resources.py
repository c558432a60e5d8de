"""The general libFM learner's pass kernels (csrc/fmg.hip: k_fmg_pass, k_fmg_chunk_draw, k_fmg_q)
use no scratch memory and spill no vector register: read from the compiler's resource summary
the build writes to build/fmg.resource.txt (csrc/Makefile, the fmg_kernels.o rule).  A row of
any length is looped over; only a lane's first four entries are held in registers.  Only the
summary is read, never the code."""
import os
import re

import pytest

from conftest import PKG

RES = os.path.join(PKG, "build", "fmg.resource.txt")
FIELDS = r"(SGPRs Spill|VGPRs Spill|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|VGPRs|LDS Size \[bytes/block\])"


def _parse():
    if not os.path.exists(RES):
        pytest.fail("%s is missing: rebuild csrc (make -C csrc clean all)" % RES)
    kernels, cur = {}, None
    with open(RES) as f:
        for line in f:
            m = re.search(r"remark: Function Name: (\S+)", line)
            if m:
                k = re.search(r"\d+(k_fmg_[a-z_]+?)(?:ILi(\d+)(?:ELi(\d+))?E)?E", m.group(1))
                cur = kernels.setdefault((k.group(1), k.group(2), k.group(3)), {}) if k else None
                continue
            m = re.search(r"remark:\s+" + FIELDS + r": (\d+)", line)
            if m and cur is not None:
                cur[m.group(1).split(" [")[0]] = int(m.group(2))
    return kernels


def test_pass_kernels_use_no_scratch_and_spill_nothing():
    kernels = _parse()
    passes = {k for k in kernels if k[0] == "k_fmg_pass"}
    assert passes == {("k_fmg_pass", m, nt) for m in ("0", "1") for nt in ("64", "256", "1024")}
    assert {k for k in kernels if k[0] == "k_fmg_chunk_draw"} == {("k_fmg_chunk_draw", "0", None), ("k_fmg_chunk_draw", "1", None)}
    assert ("k_fmg_q", None, None) in kernels
    for k, v in sorted(kernels.items(), key=str):
        print(k, v)
        assert v["ScratchSize"] == 0 and v["VGPRs Spill"] == 0, (k, v)
    for k in passes:  # a 1024-thread workgroup needs 16 waves on a CU: at least 4 per SIMD
        assert kernels[k]["Occupancy"] >= 4, (k, kernels[k])
