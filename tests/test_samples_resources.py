"""The sample store's kernels (csrc/samples.hip) use no scratch memory and spill no vector
register: read from the compiler's resource summary the build writes to
build/samples.resource.txt (csrc/Makefile, the samples_kernels.o rule).  k_samples_score keeps
8 MU SAMPLES_TW sums per lane in registers over the whole sample loop -- 64 doubles at MU = 4 --
beside the MFMA accumulators, so a spill is the way it would go wrong.  The static LDS is held to
64 KB here; the dynamic LDS the launch asks for is held to it in tests/test_samples_abi.py
(sbmf_test_samples_lds).  Only the summary is read, never the code."""
import os
import re

import pytest

from conftest import PKG

RES = os.path.join(PKG, "build", "samples.resource.txt")
FIELDS = r"(SGPRs Spill|VGPRs Spill|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|VGPRs|AGPRs|LDS Size \[bytes/block\])"


def _parse():
    if not os.path.exists(RES):
        pytest.fail("%s is missing: rebuild csrc (make -C csrc clean all)" % RES)
    kernels, cur = {}, None
    with open(RES) as f:
        for line in f:
            m = re.search(r"remark: Function Name: (\S+)", line)
            if m:
                k = re.search(r"k_samples_scoreI([fd])Li(\d)E|k_samples_pairsI([fd])E", m.group(1))
                name = None
                if k:
                    name = ("score", k.group(1), int(k.group(2))) if k.group(1) else ("pairs", k.group(3), 0)
                cur = kernels.setdefault(name, {}) if name else None
                continue
            m = re.search(r"remark:\s+" + FIELDS + r": (\d+)", line)
            if m and cur is not None:
                cur[m.group(1).split(" [")[0]] = int(m.group(2))
    return kernels


def test_every_instantiation_uses_no_scratch_and_spills_no_vector_register():
    kernels = _parse()
    want = {("score", t, mu) for t in "fd" for mu in (1, 2, 4)} | {("pairs", t, 0) for t in "fd"}
    assert set(kernels) == want
    for name, v in sorted(kernels.items()):
        print("%s<%s%s>: %s" % (name[0], "float" if name[1] == "f" else "double", ", %d" % name[2] if name[2] else "", v))
        assert v["ScratchSize"] == 0, (name, v)
        assert v["VGPRs Spill"] == 0, (name, v)
        assert v["LDS Size"] <= 65536, (name, v)
