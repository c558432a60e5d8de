"""The query list's kernels (csrc/fmq.hip: k_fmq_terms, k_fmq_operands) and every instantiation of
the accumulation kernel it shares with the watch list (csrc/recommend.hip: k_watch_accum<T, MU,
EPI>) use no scratch memory and spill no vector register: read from the compiler's resource
summaries the build writes to build/fmq.resource.txt and build/recommend.resource.txt
(csrc/Makefile).  The accumulation kernel's LDS is dynamic -- 16 MU rows of Kp + 2 doubles and
their ids (recommend.hip) --: at Kp = 112 (MU = 4) two workgroups fit a CU's 160 KB, and the
kernel's registers leave room for their eight waves.  Only the summaries are read, never the code."""
import ctypes as C
import os
import re

import pytest

from conftest import PKG
from sbmf import lib

FIELDS = r"(SGPRs Spill|VGPRs Spill|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|VGPRs|LDS Size \[bytes/block\])"
LDS_PER_CU = 160 * 1024


def _parse(name, pattern):
    path = os.path.join(PKG, "build", name)
    if not os.path.exists(path):
        pytest.fail("%s is missing: rebuild csrc (make -C csrc clean all)" % path)
    kernels, cur = {}, None
    with open(path) as f:
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


def test_query_kernels_use_no_scratch_and_spill_nothing():
    kernels = _parse("fmq.resource.txt", r"\d+(k_fmq_[a-z]+)E")
    assert set(kernels) == {("k_fmq_terms",), ("k_fmq_operands",)}
    for k, v in sorted(kernels.items()):
        print(k, v)
        assert v["ScratchSize"] == 0 and v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0, (k, v)
        assert v["LDS Size"] == 0 and v["Occupancy"] >= 4, (k, v)


def test_accumulation_kernel_epilogues():
    kernels = _parse("recommend.resource.txt", r"\d+k_watch_accumI([df])Li(\d)ELi(\d)EE")
    # the lists' own (EPI 0, both table types) and the query list's epilogues (f64): cdf 1, overwrite 2, both 3
    want = {(t, mu, "0") for t in "df" for mu in "421"} | {("d", mu, e) for mu in "421" for e in "123"}
    assert set(kernels) == want
    for k, v in sorted(kernels.items()):
        print(k, v)
        assert v["ScratchSize"] == 0 and v["VGPRs Spill"] == 0, (k, v)
        assert v["LDS Size"] == 0, (k, v)  # static: none; the dynamic part is the launcher's
    # Kp = 112 runs MU = 4: the launch's dynamic LDS as the launcher itself sizes it (watch_lds_bytes,
    # recommend.h, through sbmf_test_watch_lds), twice, within a CU; two workgroups are 8 waves = 2 per SIMD
    rows, lds = C.c_uint32(), C.c_uint64()
    assert lib.sbmf_test_watch_lds(112, C.byref(rows), C.byref(lds)) == 0
    print("Kp = 112: %d rows a workgroup, %d bytes of LDS" % (rows.value, lds.value))
    assert rows.value == 64 and lds.value >= 64 * 112 * 8  # at least the rows themselves
    assert 2 * lds.value <= LDS_PER_CU
    for e in "0123":
        assert kernels[("d", "4", e)]["Occupancy"] >= 2, e
