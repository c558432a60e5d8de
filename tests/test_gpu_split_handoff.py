"""The split-row hand-off of the streaming kernels (k_gres): partials that are their own flags.

A chunk of a split row publishes its packed partial of a k-block with plain write-through stores
and every chunk reads all of them, taking a slab word as valid as soon as it no longer holds the
all-ones sentinel; the chunks and k_split_finish put the sentinel back, so a slab area is ready
for the next launch without a clear.  None of this may change a bit: every case is held to the
hashes of the commit before (tests/golden/split_handoff_parent.json, made by
tests/workers/split_handoff_chain.py on that commit's build, the counter hand-off).

Every case is ML-100k, stream_threshold 40, for 8 sweeps: each slab area is used by 16 launches.
The cases have far more chunks than resident workgroups, so the chunks of a row start unevenly.
A hand-off that times out makes learn() raise, which fails the case."""
import json
import os

import pytest

from conftest import GOLD
from workers import split_handoff_chain as shc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def parent_chain():
    with open(os.path.join(GOLD, "split_handoff_parent.json")) as f:
        return json.load(f)


def _same(got, want):
    assert got["U"] == want["U"]
    assert got["V"] == want["V"]
    assert got["rmse"] == want["rmse"]


@pytest.mark.parametrize("K,chunk,tune,prec", shc.CASES, ids=[shc.case_id(*c) for c in shc.CASES])
def test_chain_identical_to_parent(ml100k, parent_chain, K, chunk, tune, prec):
    """Same seed, same bits as the counter hand-off: U, V and the RMSE list of the Philox chain.
    K 17 (two k-blocks) and 100 (seven); 30+-chunk rows and 2..16-chunk rows; the 4-, 8- and
    16-wave kernels on both sides; f64 and one f32 case."""
    tr, te = ml100k
    _same(shc.run_case(tr, te, K, chunk, tune, prec), parent_chain[shc.case_id(K, chunk, tune, prec)])


REUSE = (100, 16, 0, "f64")


def test_second_learner_in_one_process(ml100k, parent_chain):
    """Two learners one after the other in one process: each fills its own slab areas, and the
    second gives the first's bits."""
    tr, te = ml100k
    first = shc.run_case(tr, te, *REUSE)
    second = shc.run_case(tr, te, *REUSE)
    _same(first, parent_chain[shc.case_id(*REUSE)])
    _same(second, first)


@pytest.mark.parametrize("case", [REUSE, (17, 64, 1 << 17, "f64")], ids=lambda c: shc.case_id(*c))
def test_two_stages_share_the_slab_areas(ml100k, parent_chain, case):
    """SBMF_STAGES=2: both stages' launches of a set use one slab area, one after the other, and
    give the one-stage bits."""
    tr, te = ml100k
    _same(shc.run_case(tr, te, *case, stages=2), parent_chain[shc.case_id(*case)])
