"""The classification frames of the two libFM learners (csrc/fm_dev.h, instantiated in fmm.hip and
fmg.hip: k_fm*_class_train in its three target modes, k_fm*_class_test, the count sums, the
target subtraction and the draw alone) use no scratch memory and spill no vector register: read
from the compiler's resource summaries the build writes to build/fmm.resource.txt and
build/fmg.resource.txt (csrc/Makefile).  Only the summaries are read, never the code."""
import os
import re

import pytest

from conftest import PKG

FIELDS = r"(SGPRs Spill|VGPRs Spill|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|VGPRs|LDS Size \[bytes/block\])"


def _parse(name):
    res = os.path.join(PKG, "build", name)
    if not os.path.exists(res):
        pytest.fail("%s is missing: rebuild csrc (make -C csrc clean all)" % res)
    kernels, cur = {}, None
    with open(res) as f:
        for line in f:
            m = re.search(r"remark: Function Name: (\S+)", line)
            if m:
                k = re.search(r"\d+(k_fm[mg]?_[a-z_]+?)(?:ILi(\d+)E)?E", m.group(1))
                cur = kernels.setdefault((k.group(1), k.group(2)), {}) if k else None
                continue
            m = re.search(r"remark:\s+" + FIELDS + r": (\d+)", line)
            if m and cur is not None:
                cur[m.group(1).split(" [")[0]] = int(m.group(2))
    return kernels


@pytest.mark.parametrize("layout", ["fmm", "fmg"])
def test_classification_frames_use_no_scratch_and_spill_nothing(layout):
    kernels = _parse(layout + ".resource.txt")
    want = {("k_%s_class_train" % layout, m) for m in ("0", "1", "2")} | {("k_%s_class_test" % layout, None),
                                                                          ("k_%s_sub" % layout, None)}
    if layout == "fmm":  # shared by both layouts
        want |= {("k_fm_count_sums", None), ("k_fm_tgauss", None)}
    assert want <= set(kernels), sorted(want - set(kernels))
    for k in sorted(want, key=str):
        v = kernels[k]
        print(k, v)
        assert v["ScratchSize"] == 0 and v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0, (k, v)
        assert v["Occupancy"] >= 4, (k, v)  # the rejection loops' registers leave the gathers their waves
