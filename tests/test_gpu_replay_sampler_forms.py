"""The replay store's device sampler (csrc/mzreplay.hip: sample_games_kernel, position_tables_kernel, sample_walk_kernel,
sample_finish_kernel, update_priorities_kernel / game_priority_kernel) on the MI355X against numpy's own
numpy.random.RandomState (tests/replay_sampler_reference.py), bit for bit: game ids, positions and absorbing actions as
integers, importance weights by their uint32 view, the stream's key block and position after every batch.

The cases (tests/replay_sampler_cases.py; held to numpy alone, and to the defects they are there for, by
tests/test_replay_sampler_reference.py) stand on both sides of every switch between two forms of a kernel:

* games G=12288 | 12289        game probabilities and running sum in LDS | in HBM; 1, 2, G - 1 and G games, a wrapped ring
* leaves n=65032..70001        512 parallel pairwise leaves | the one-lane sum at 513 and more (65 033, 65 537, 70 001),
                               back to 512 at 65 040 and 65 536
* positions L=18432 | 18433 | 27000   a sample's table built in LDS | in place; draws in the table's last entries
* walk U=5 (batch 3351 | 3352 | 4096), U=4 (batch 4096: exactly the budget)   table tails in LDS | read from HBM;
                               batch 4097 refused by name with the stream unmoved
* several batches              one store at batch 1, 129, 4096, 1: the per-batch scratch grows and is reused
* stream ...                   every start position 0..624 of a key block, so the 624-word turn-over falls inside every
                               draw of every loop once (U=121: inside a 64-word rejection round)
* chosen ...                   draws exactly on a table entry, at 0 and at 1 - 2**-53, over equal entries from zero
                               priorities, subnormal priorities, and a table whose last entry is not 1
and after a batch of each large store priorities are written back and the next batch is compared again.

Where it is cheap a host-sampled ReplayBuffer holds the same games: its priorities (the same priorities_kernel) are
compared for every game, the device sampler's for 64 of each bulk, and whole batches with assert_same_batch."""
import importlib

import pytest

import replay_sampler_cases as rc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mods(pkg):
    importlib.import_module("muzero-hypermodel_amd.build").build_native()
    return (importlib.import_module("muzero-hypermodel_amd.replay_buffer"),
            importlib.import_module("muzero-hypermodel_amd.self_play"))


@pytest.mark.parametrize("name", rc.CASE_NAMES)
def test_device_sampler_equals_numpy(mods, name):
    case = rc.case_named(name)
    run = rc.Run(case, mods)
    try:
        case.script(run)
        assert run.records
    finally:
        run.close()
