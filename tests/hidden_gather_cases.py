"""Inputs and the model of the hidden-state movement tests (test_gpu_hidden_gather.py on the card,
test_hidden_gather_reference.py on the CPU).

A lock-step search moves hidden states twice per simulation: the network's output goes into the pool f32[S+1][E][H]
(expand_roots_kernel writes slab 0, copy_slab_kernel slab s + 1) and the state of the leaf's parent comes out again as
the next inference batch, through one of the gathers of csrc/mcts_kernels.hip.  Nothing here computes: the pool holds
TAGS (every float distinct, so a row taken from a wrong slab, env or offset cannot compare equal), which slab a row
must come from is a dictionary walk over the recorded search paths, and every comparison is on the int32 views, bit for
bit.  The module imports no GPU code; `guarded` asks for torch when it is called."""
import numpy as np

from lockstep_decode_cases import SHAPES, players_for
from parity_helpers import make_search_config, random_streams

TAG_BASE = 0x3F000000     # 0.5f: tags run upwards from here through finite positive floats
CANARY = 0x7FC0DEAD       # a quiet NaN no copy produces: what nobody wrote still holds it
GUARD = 64                # floats before and after a guarded output (256 bytes: the interior keeps 16-byte alignment)

E_MAIN = 70               # ragged in every lane-group width (64 / G trees per wavefront) and in a select queue of 40
S_MAIN = 24
INACTIVE = (0, 33, -1)    # envs of the inactive runs (num_legal = 0); -1 is the last one


# ---- tags ---------------------------------------------------------------------------------------------------------
def tagged_pool(S, E, H):
    """f32[S+1, E, H] whose int32 view is TAG_BASE + arange: every element a distinct finite float."""
    n = (S + 1) * E * H
    assert TAG_BASE + n <= 0x7F800000, "tags would run into the infinities"
    return (np.int32(TAG_BASE) + np.arange(n, dtype=np.int32)).view(np.float32).reshape(S + 1, E, H)


def bits(a):
    """The int32 view every comparison is made on."""
    a = np.ascontiguousarray(a)
    assert a.dtype == np.float32
    return a.view(np.int32)


# ---- which slab a leaf's parent lives in ------------------------------------------------------------------------------
def parents_from_paths(depth, actions):
    """depth[S], actions[S, >= max depth]: the search paths of one tree as the oracle and last_paths() record them (the
    root's entry is the real action, deeper entries are child slots = actions).  Returns (parent[S], action[S]): the node
    whose hidden state simulation s needs -- 0 is the root, k the node simulation k - 1 expanded, which is also the pool
    slab its state lives in -- and the action select must report for it."""
    expanded = {}
    parents, picked = [], []
    for s, d in enumerate(depth):
        d = int(d)
        assert d >= 1
        node = 0
        for a in actions[s, :d - 1]:
            node = expanded[(node, int(a))]       # KeyError: a path through a node no earlier simulation expanded
        last = int(actions[s, d - 1])
        assert (node, last) not in expanded, f"simulation {s} expands ({node}, {last}) a second time"
        expanded[(node, last)] = s + 1
        parents.append(node)
        picked.append(last)
    return np.asarray(parents, dtype=np.int64), np.asarray(picked, dtype=np.int64)


def parents_of_envs(sim_depth, sim_actions):
    """[E, S] depths and [E, S, S] actions -> (parent[E, S], action[E, S])."""
    pairs = [parents_from_paths(sim_depth[e], sim_actions[e]) for e in range(len(sim_depth))]
    return np.stack([p for p, _ in pairs]), np.stack([a for _, a in pairs])


def coverage(parents):
    """parent[E, S] -> (share of (env, simulation) pairs with a parent other than the root, share of the pairs with
    s > 0 whose parent is the node expanded by the step just before, the set of slabs that are a parent somewhere)."""
    S = parents.shape[1]
    s = np.arange(S)[None, :]
    return float((parents != 0).mean()), float((parents[:, 1:] == s[:, 1:]).mean()), set(np.unique(parents).tolist())


# ---- expected rows ------------------------------------------------------------------------------------------------
def expected_hidden(pool, parents_s):
    """pool f32[S+1, E, H], parents_s[E] -> f32[E, H]: row e of slab parents_s[e]."""
    return pool[np.asarray(parents_s), np.arange(pool.shape[1])]


def expected_planes(pool, parents_s, action_s, plane, A):
    """The dynamics input rows: that row followed by `plane` copies of float32(action) / float32(A)."""
    fill = np.asarray(action_s).astype(np.float32) / np.float32(A)
    assert fill.dtype == np.float32
    return np.concatenate([expected_hidden(pool, parents_s), np.repeat(fill[:, None], plane, axis=1)], axis=1)


# ---- guarded outputs ----------------------------------------------------------------------------------------------
def guarded(E, width, device="cuda"):
    """(whole, interior): a canary-filled device tensor of GUARD + E * width + GUARD floats and its [E, width] middle."""
    import torch
    whole = torch.full((2 * GUARD + E * width,), CANARY, dtype=torch.int32, device=device).view(torch.float32)
    interior = whole[GUARD:GUARD + E * width].view(E, width)
    assert interior.data_ptr() % 16 == 0 and interior.is_contiguous()
    return whole, interior


def guards_intact(whole):
    import torch
    raw = whole.view(torch.int32)
    return bool((raw[:GUARD] == CANARY).all()) and bool((raw[-GUARD:] == CANARY).all())


# ---- streams and configs --------------------------------------------------------------------------------------------
TIES = (3, 9)             # action counts whose streams carry many exactly equal priors (tie-breaks on the device stream)


def discount_for(A):
    return 1 if players_for(A) == 2 else 0.997


def streams_for(A, E=E_MAIN, S=S_MAIN):
    return random_streams(E, A, S, seed=1000 + A, n_players=players_for(A), ties=A in TIES, min_legal=min(2, A))


def fc_config(A, H, S=S_MAIN):
    return make_search_config(A, S, players_for(A), discount_for(A), H=H)


def planes_config(A, channels, h, w, S=S_MAIN):
    """Only what BatchedMCTS reads of a residual-network config: the hidden state is [channels, h, w]."""
    cfg = make_search_config(A, S, players_for(A), discount_for(A))
    cfg.network, cfg.channels, cfg.observation_shape, cfg.downsample = "resnet", channels, (1, h, w), False
    del cfg.encoding_size
    return cfg


# ---- part A: mzmcts_select's gathers -----------------------------------------------------------------------------------
def shape_for(G, CH):
    """The (A, group_width argument) that reaches dispatch_group's (G, CH), preferring action counts the streams' own
    coverage is stated for."""
    preferred = {(1, 1): (1, 0), (1, 2): (2, 1), (2, 1): (2, 0), (4, 1): (3, 0), (4, 2): (5, 4), (8, 1): (7, 0),
                 (8, 2): (9, 8), (16, 1): (9, 0), (32, 1): (17, 0), (64, 1): (9, 64), (64, 4): (121, 0)}
    A, gw = preferred[(G, CH)]
    assert (A, gw, G, CH) in SHAPES
    return A, gw


GROUP_SHAPES = sorted({(G, CH) for _, _, G, CH in SHAPES})

# (A, group_width, G, CH, H)
FUSED_GATHER_CASES = ([shape_for(G, CH) + (G, CH, H) for G, CH in GROUP_SHAPES for H in (63, 64)]
                      + [shape_for(G, CH) + (G, CH, H) for G, CH in ((1, 1), (16, 1), (64, 4)) for H in (1, 3, 4)])
# gather_hidden_kernel: scalar | float4 | 257 float4 pieces, two blocks per row | 2049 pieces, nine blocks wanted and
# eight given: a second lap of the stride loop | scalar under the same cap
GATHER_HIDDEN_CASES = [(9, 0, 16, 1, H) for H in (65, 68, 1028, 8196, 8195)]
SELECT_CASES = FUSED_GATHER_CASES + GATHER_HIDDEN_CASES
QUEUES = (40, 256)        # trees per wavefront: a ragged refill and a ragged last wavefront | several refills per group
QUEUE_CASES = [c for c in SELECT_CASES if c[0] <= 64]     # (more than 64 actions: the request is ignored)
# one case per kernel for the inactive runs: (driver, case)
INACTIVE_SELECT_CASES = [("select", (9, 0, 16, 1, 64)), ("select", (9, 0, 16, 1, 63)), ("queue40", (9, 0, 16, 1, 64)),
                         ("queue40", (9, 0, 16, 1, 63)), ("fused", (9, 0, 16, 1, 64)), ("select", (9, 0, 16, 1, 68)),
                         ("queue40", (9, 0, 16, 1, 68)), ("fused", (9, 0, 16, 1, 65))]


def select_case_id(case):
    A, gw, G, CH, H = case
    return f"A{A}-gw{gw}-G{G}x{CH}-H{H}"


# ---- part B: dynamics-input rows -------------------------------------------------------------------------------------------
# (channels, h, w, A, E, S): row = channels * h * w + h * w.  The action counts are ones at which a / A and a * (1 / A)
# differ in float32 for some action (6, 7, 13, 121; not 3 or 9: test_hidden_gather_reference.py), so the plane tells a
# division from a multiplication by the reciprocal.
PLANES_CASES = [
    (1, 1, 1, 6, 1025, S_MAIN),      # row 2: short rows, 1024 envs per block, the last block holds one env
    (16, 3, 3, 13, E_MAIN, S_MAIN),  # row 153: short rows (TicTacToe)
    (72, 1, 7, 7, E_MAIN, S_MAIN),   # row 511: short rows, the tightest multiply-shift division
    (63, 2, 4, 7, E_MAIN, S_MAIN),   # row 512: the last short row
    (18, 3, 9, 7, E_MAIN, S_MAIN),   # row 513: long rows, H even, row odd: scalar
    (19, 3, 9, 13, E_MAIN, S_MAIN),  # row 540: long rows, H odd, row even: scalar
    (256, 1, 2, 6, E_MAIN, S_MAIN),  # row 514: long rows, float2
    (64, 6, 7, 7, E_MAIN, S_MAIN),   # row 2730: float2, capped grid (Connect4)
    (128, 11, 11, 121, E_MAIN, 12),  # row 15609: scalar, capped grid (Gomoku); 12 simulations keep the pool near 60 MB
]
FUSED_PLANES_ROWS = (153, 2730, 15609)
INACTIVE_PLANES_ROWS = (153, 514)


def planes_row(case):
    c, h, w = case[:3]
    return c * h * w + h * w


def planes_case_id(case):
    return f"row{planes_row(case)}-A{case[3]}-E{case[4]}"


# ---- part C: writes into the pool ----------------------------------------------------------------------------------------
# (E, H, S, floats the source starts past a 16-byte boundary)
COPY_SLAB_CASES = [
    (1, 3, 2, 0),          # n < 4
    (7, 3, 2, 0),          # n % 4 != 0 (and slabs 1, 2 start off a 16-byte boundary)
    (70, 64, 2, 0),        # float4
    (70, 64, 2, 1),        # a contiguous view one float into a larger tensor: the kernel's alignment test -> scalar loop
    (70, 30000, 2, 0),     # 2.1 M floats > 2048 * 256 * 4: the capped grid laps
]
ROOT_COPY_CASES = [(H, G) for H in (3, 64, 2688) for G in (1, 16, 64)]


def copy_slab_case_id(case):
    return f"E{case[0]}xH{case[1]}" + (f"-src+{case[3]}" if case[3] else "")

