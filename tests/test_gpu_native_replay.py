"""Whole native lock-step searches replayed on the fp64 oracle, at every lane form.

expand_roots_kernel / expand_backup_kernel / expand_backup_select_kernel / select_kernel / select_queue_kernel
(csrc/mcts_kernels.hip, csrc/tree_device.h) in their native (INJECTED = false) instantiations -- the code objects every
actor launches -- search 19 trees x 32 simulations from seeded logits (tests/native_replay_cases.py: all eleven (G, CH),
support 10 and, on the strided side of F <= 4 G, 2 G; three-step loop, fused step, select queues of 40 and 256 trees over
57 envs; deep backups, repeated normaliser updates, tie-breaks after the first expansion, tie storms, both players,
four temperatures).  One statement, no tolerance:

    the native search == the oracle fed with the native search's own decoded outputs,

on every key of test_gpu_parity.EXACT_KEYS (noise, visits, value sums, priors, rewards, root sums, min-max, depths, paths,
tie lists, targets, the sampled action) and on the count of tie-break words.  The oracle takes stream row s at simulation
s whatever its path, so a mismatch cannot cancel out: sim_actions shows where it left the engine's path.  The same
streams through the INJECTED instantiations (run_injected_on_engine) must equal the native run too, which pins a
difference on one template argument.  With the decode bounds of test_gpu_lockstep_decode.py this holds a whole native
search to float64.

Reading used: the per-simulation one -- every tree is exported after every simulation (native_replay.decoded_streams:
value_sum / reward of the path's last edge, prior row of the node it created, each reading checked against the tree's own
visit counts and links); the 608 exports of a case cost well under a second (printed with -s, collected in
measure_out/native_replay_report.json)."""
import importlib
import json
import os
import time

import numpy as np
import pytest
import torch

from native_replay import (decoded_streams, dirichlet_words, native_root_priors, run_native_on_engine, search_config,
                           streams_for)
from native_replay_cases import QUEUE, REPEAT, S, T, case_id, cases, inputs
from parity_helpers import run_injected_on_engine, run_injected_on_oracle
from test_gpu_parity import EXACT_KEYS, assert_exact

pytestmark = pytest.mark.gpu

REPORT = {}


@pytest.fixture(scope="module")
def eng(pkg):
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    yield importlib.import_module("muzero-hypermodel_amd.engine")
    out_dir = os.environ.get("MZ_OUT_DIR") or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                          "measure_out")
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "native_replay_report.json"), "w") as f:
        json.dump(REPORT, f, indent=1, sort_keys=True)


CASES = cases()


@pytest.mark.parametrize("A,gw,G,CH,s,form", CASES, ids=[case_id(*c) for c in CASES])
def test_native_search_equals_oracle_fed_its_own_decoded_outputs(eng, oracle, A, gw, G, CH, s, form):
    started = time.perf_counter()
    case = inputs(A, gw, s)
    cfg = search_config(case)
    got, exports = run_native_on_engine(eng, case, form, G=G)
    searched = time.perf_counter() - started
    assert got["all_equal"], "copies of the same tree differ"
    value, reward, priors = decoded_streams(exports, got["sim_depth"], got["sim_actions"], case["legal"])
    streams = streams_for(case, native_root_priors(eng, case, G=G), value, reward, priors)
    storms = case["storm"]
    # a tie storm is one on the card: exact zeros, equal priors, bounds that never separated
    assert (value[storms] == 0).all() and (reward[storms] == 0).all()
    assert (priors[storms] == priors[storms][..., :1]).all()
    assert (got["min_max"][storms, 0] == got["min_max"][storms, 1]).all()

    want = run_injected_on_oracle(oracle, cfg, streams, temperature=case["temperature"])
    left = [(t, int(np.nonzero((got["sim_actions"][t] != want["sim_actions"][t]).any(axis=1))[0][0]))
            for t in range(T) if not np.array_equal(got["sim_actions"][t], want["sim_actions"][t])]
    assert not left, f"(tree, first simulation) where the oracle leaves the native search's path: {left}"
    assert_exact(got, want, where=f"{case_id(A, gw, G, CH, s, form)} native vs oracle: ")
    tie_words = want["rng_words_run"] - dirichlet_words(oracle, case)
    assert np.array_equal(got["tie_break_words"].astype(np.int64), tie_words), "tie-break words drawn"
    assert np.array_equal(got["depth_sum"], want["sim_depth"].sum(axis=1))

    injected = run_injected_on_engine(eng, cfg, streams, temperature=case["temperature"], group_width=gw,
                                      fused_step=form == "fused", select_queue=QUEUE.get(form, 0), repeat=REPEAT[form])
    assert injected["all_equal"]
    assert_exact(got, injected, where=f"{case_id(A, gw, G, CH, s, form)} native vs INJECTED kernels: ")
    assert np.array_equal(got["tie_break_words"], injected["tie_break_words"])
    assert np.array_equal(got["depth_sum"], injected["depth_sum"])

    deep = int((got["max_tree_depth"] >= 3).sum())
    elapsed = time.perf_counter() - started
    REPORT[case_id(A, gw, G, CH, s, form)] = dict(seconds=elapsed, native_search_and_exports_seconds=searched,
                                                  trees_with_depth_3=deep, tie_break_words=int(tie_words.sum()))
    print(f"\n{case_id(A, gw, G, CH, s, form)}: {elapsed:.2f} s ({searched:.2f} s the native search with its {T * S} "
          f"exports); depth >= 3 in {deep} of {T} trees, {int(tie_words.sum())} tie-break words")
