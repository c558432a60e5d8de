"""The sample store's guest kernels (csrc/samples_foldin.hip) use no scratch memory and spill no
vector register: read from the compiler's resource summary the build writes to
build/samples_foldin.resource.txt (csrc/Makefile, the samples_foldin_kernels.o rule).
k_samples_foldin wraps k_foldin's scan (csrc/foldin_dev.h) in a loop over samples and scans inside
a 16-wave workgroup, whose 128 vector registers a lane the loop-invariant values compete for, so a
spill is the way it would go wrong.  The static LDS -- the scan's, 51,584 bytes -- is held to 64 KB.
The summaries of foldin.hip and samples.hip list the kernels they listed before this file existed.
Only the summaries are read, never the code."""
import os
import re

import pytest

from conftest import PKG

BUILD = os.path.join(PKG, "build")
FIELDS = r"(SGPRs Spill|VGPRs Spill|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|VGPRs|AGPRs|LDS Size \[bytes/block\])"


def _parse(name, pattern):
    res = os.path.join(BUILD, name)
    if not os.path.exists(res):
        pytest.fail("%s is missing: rebuild csrc (make -C csrc clean all)" % res)
    kernels, cur = {}, None
    with open(res) as f:
        for line in f:
            m = re.search(r"remark: Function Name: (\S+)", line)
            if m:
                k = re.search(pattern, m.group(1))
                cur = kernels.setdefault(k.groups(), {}) if k else None
                continue
            m = re.search(r"remark:\s+" + FIELDS + r": (\d+)", line)
            if m and cur is not None:
                cur[m.group(1).split(" [")[0]] = int(m.group(2))
    return kernels


def test_every_instantiation_uses_no_scratch_and_spills_no_vector_register():
    kernels = _parse("samples_foldin.resource.txt", r"(k_samples_foldin|k_samples_foldin_step)I([fd])E")
    assert set(kernels) == {(k, t) for k in ("k_samples_foldin", "k_samples_foldin_step") for t in "fd"}
    for name, v in sorted(kernels.items()):
        print("%s<%s>: %s" % (name[0], "float" if name[1] == "f" else "double", v))
        assert v["ScratchSize"] == 0, (name, v)
        assert v["VGPRs Spill"] == 0, (name, v)
        assert v["LDS Size"] <= 65536, (name, v)


def test_the_other_summaries_list_what_they_listed():
    every = r"Function Name: \S*?(k_[a-z_]+)I"
    for name, want in (("foldin.resource.txt", {"k_foldin"}), ("samples.resource.txt", {"k_samples_score", "k_samples_pairs"})):
        with open(os.path.join(BUILD, name)) as f:
            assert set(re.findall(every, f.read())) == want, name
