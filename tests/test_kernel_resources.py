"""Register budget of the streaming row kernels (k_gres / k_grow), from the compiler's resource
summary the build writes to build/kernels.resource.txt (csrc/Makefile, the kernels.o rule).

The kernels are capped at 128 VGPRs for 4 waves per SIMD; what does not fit is spilled, SGPRs to
VGPR lanes and VGPRs to scratch memory, and the item stage has moved 5-10 % with a few spilled
registers more or fewer.  PARENT is the table of the commit before the kernels'
arguments were split into a by-value block and a cold block in device memory: no instantiation
may spill more than it did then.  FLAGSHIP holds the four kernels of the ML-20M K=100 f64 line to
what the split reached.  Only the summary is read, never the code."""
import os
import re

import pytest

from conftest import PKG

RES = os.path.join(PKG, "build", "kernels.resource.txt")

# (kernel, T, NW[, KL]) -> (spilled SGPRs, spilled VGPRs) before the argument split; the same for
# SIDE 0 and 1
PARENT = {
    ("k_gres", "d", 16): (80, 14), ("k_gres", "d", 8): (69, 15), ("k_gres", "d", 4): (44, 0),
    ("k_gres", "f", 16): (59, 23), ("k_gres", "f", 8): (75, 26), ("k_gres", "f", 4): (35, 1),
    ("k_grow", "d", 1, 128): (21, 0), ("k_grow", "d", 1, 256): (31, 2),
    ("k_grow", "d", 2, 128): (6, 0), ("k_grow", "d", 2, 256): (10, 0),
    ("k_grow", "f", 1, 128): (13, 0), ("k_grow", "f", 1, 256): (23, 0),
    ("k_grow", "f", 2, 128): (4, 0), ("k_grow", "f", 2, 256): (6, 0),
}
# (kernel, T, NW, SIDE) -> (spilled SGPRs, spilled VGPRs, scratch bytes per lane) reached by the
# split: the item sets (16- and 8-wave, SIDE 1) and the user sets (8- and 4-wave, SIDE 0).  The
# parent's scratch: 60, 64, 64, 0.
FLAGSHIP = {
    ("k_gres", "d", 16, 1): (10, 1, 8),
    ("k_gres", "d", 8, 1): (12, 0, 0),
    ("k_gres", "d", 8, 0): (12, 0, 0),
    ("k_gres", "d", 4, 0): (6, 0, 0),
}


def _parse():
    if not os.path.exists(RES):
        pytest.fail("%s is missing: rebuild csrc (make -C csrc clean all)" % RES)
    kernels, cur = {}, None
    with open(RES) as f:
        for line in f:
            m = re.search(r"remark: Function Name: (\S+)", line)
            if m:
                cur = None
                k = re.search(r"(k_gres|k_grow)I([fd])((?:Li\d+E)+)E", m.group(1))
                if k:
                    ints = tuple(int(x) for x in re.findall(r"Li(\d+)E", k.group(3)))
                    cur = kernels.setdefault((k.group(1), k.group(2)) + ints, {})
                continue
            m = re.search(r"remark:\s+(SGPRs Spill|VGPRs Spill|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]): (\d+)",
                          line)
            if m and cur is not None:
                cur[m.group(1).split(" [")[0]] = int(m.group(2))
    return kernels


@pytest.fixture(scope="module")
def kernels():
    return _parse()


def test_every_instantiation_is_in_the_summary(kernels):
    # k_gres<T, NW, SIDE>: 2 x 3 x 2; k_grow<T, NW, SIDE, KL>: 2 x 2 x 2 x 2
    assert sum(k[0] == "k_gres" for k in kernels) == 12
    assert sum(k[0] == "k_grow" for k in kernels) == 16
    for v in kernels.values():
        assert set(v) == {"SGPRs Spill", "VGPRs Spill", "ScratchSize", "Occupancy"}


def test_no_instantiation_spills_more_than_before_the_split(kernels):
    for key, v in sorted(kernels.items()):
        name, t, nw = key[0], key[1], key[2]
        base = PARENT[(name, t, nw) if name == "k_gres" else (name, t, nw, key[4])]
        print(key, v)
        assert v["SGPRs Spill"] <= base[0], key
        assert v["VGPRs Spill"] <= base[1], key
        assert v["Occupancy"] == 4, key


def test_flagship_kernels_keep_what_the_split_reached(kernels):
    for key, (sg, vg, scr) in FLAGSHIP.items():
        v = kernels[key]
        base = PARENT[key[:3]]
        assert sg < base[0] and (vg < base[1] or base[1] == 0), key  # the literals: strictly below the parent's
        assert v["SGPRs Spill"] <= sg, (key, v)
        assert v["VGPRs Spill"] <= vg, (key, v)
        assert v["ScratchSize"] <= scr, (key, v)
        assert v["Occupancy"] == 4, key
