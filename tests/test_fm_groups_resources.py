"""Register, LDS and scratch use of the attribute-group kernels of the general libFM learner
(csrc/fmg.hip), read from the compiler's resource summary of the gfx950 code object that the
build writes to build/fmg.resource.txt: the grouped column sums (k_fmg_gsums), the grouped
passes (k_fmg_gpass, k_fmg_gchunk_draw) and, beside them, the ungrouped passes they share their
body with (k_fmg_pass, k_fmg_chunk_draw).  The figures are printed; what is asserted is that no
kernel uses scratch or spills -- the ungrouped ones had none before the groups came --, that the
grouped passes keep the occupancy a 1024-thread workgroup needs, and that the sums kernel's
staging leaves room for four workgroups in a CU's 160 KiB of LDS.  Only the summary is read,
never the code."""
import re

from test_fmg_resources import FIELDS, RES


def _parse():
    kernels, cur = {}, None
    with open(RES) as f:
        for line in f:
            m = re.search(r"remark: Function Name: (\S+)", line)
            if m:
                k = re.search(r"\d+(k_fmg_[a-z_]+?)(?:ILi(\d+)(?:ELi(\d+))?E)?E", m.group(1))
                cur = kernels.setdefault((k.group(1), k.group(2), k.group(3)), {}) if k else None
                continue
            m = re.search(r"remark:\s+(TotalSGPRs|" + FIELDS[1:] + r": (\d+)", line)
            if m and cur is not None:
                cur[m.group(1).split(" [")[0]] = int(m.group(2))
    return kernels


def test_group_kernels_use_no_scratch_and_spill_nothing():
    kernels = _parse()
    gpass = {k for k in kernels if k[0] == "k_fmg_gpass"}
    assert gpass == {("k_fmg_gpass", m, nt) for m in ("0", "1") for nt in ("64", "256", "1024")}
    assert {k for k in kernels if k[0] == "k_fmg_gchunk_draw"} == {("k_fmg_gchunk_draw", "0", None),
                                                                  ("k_fmg_gchunk_draw", "1", None)}
    assert ("k_fmg_gsums", None, None) in kernels
    watched = [k for k in kernels if k[0] in ("k_fmg_gsums", "k_fmg_gpass", "k_fmg_gchunk_draw", "k_fmg_pass",
                                              "k_fmg_chunk_draw")]
    assert len(watched) == 17
    for k in sorted(watched, key=str):
        v = kernels[k]
        print(k, "VGPRs %d SGPRs %d LDS %d scratch %d occupancy %d" % (v["VGPRs"], v["TotalSGPRs"], v["LDS Size"],
                                                                       v["ScratchSize"], v["Occupancy"]))
        assert v["ScratchSize"] == 0 and v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0, (k, v)
    for k in gpass:  # a 1024-thread workgroup needs 16 waves on a CU: at least 4 per SIMD
        assert kernels[k]["Occupancy"] >= 4, (k, kernels[k])
        # the group's prior costs a few registers, never an occupancy step
        assert kernels[k]["Occupancy"] == kernels[("k_fmg_pass",) + k[1:]]["Occupancy"], k
    gs = kernels[("k_fmg_gsums", None, None)]
    assert gs["LDS Size"] * 4 <= 160 * 1024 and gs["Occupancy"] >= 4, gs
