"""k_foldin (csrc/foldin.hip) uses no scratch memory: read from the compiler's resource summary
the build writes to build/foldin.resource.txt (csrc/Makefile, the foldin_kernels.o rule).
A row of any length is looped over, never held in registers, so no vector register may spill
and no lane may own scratch bytes.  (Scalar registers that do not fit are parked in VGPR
lanes, not in memory; their count is recorded in DESIGN.md 4.5, not held here.)  Only the
summary is read, never the code."""
import os
import re

import pytest

from conftest import PKG

RES = os.path.join(PKG, "build", "foldin.resource.txt")
FIELDS = r"(SGPRs Spill|VGPRs Spill|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|VGPRs|LDS Size \[bytes/block\])"


def _parse():
    if not os.path.exists(RES):
        pytest.fail("%s is missing: rebuild csrc (make -C csrc clean all)" % RES)
    kernels, cur = {}, None
    with open(RES) as f:
        for line in f:
            m = re.search(r"remark: Function Name: (\S+)", line)
            if m:
                k = re.search(r"k_foldinI([fd])E", m.group(1))
                cur = kernels.setdefault(k.group(1), {}) if k else None
                continue
            m = re.search(r"remark:\s+" + FIELDS + r": (\d+)", line)
            if m and cur is not None:
                cur[m.group(1).split(" [")[0]] = int(m.group(2))
    return kernels


def test_both_instantiations_use_no_scratch():
    kernels = _parse()
    assert set(kernels) == {"f", "d"}
    for t, v in sorted(kernels.items()):
        print("k_foldin<%s>: %s" % ("float" if t == "f" else "double", v))
        assert v["ScratchSize"] == 0 and v["VGPRs Spill"] == 0, (t, v)
        assert v["LDS Size"] <= 64 * 1024, (t, v)
