"""A native lock-step search replayed on the fp64 oracle from its own decoded outputs.

Right after simulation s the tree states every number the decode of that simulation produced, widened to double
(mzmcts_export_tree): with (parent, a) the last edge of the simulation's path and node = child_node[parent, a],

    value   value_sum[parent, a]      the new node has been visited once, by its own value (both players' sign is +)
    reward  reward[parent, a]
    priors  prior[node, :]

Collected over a search these are the value [T, S], reward [T, S] and priors [T, S, A] streams the oracle and the
INJECTED instantiations of the kernels take (parity_helpers.run_injected_on_oracle / run_injected_on_engine), so a native
search must equal both, bit for bit: nothing in the tree arithmetic has a tolerance.

Indexing (tests/test_gpu_lockstep_decode.py): the ROOT row of an exported tree is indexed by child SLOT (the i-th legal
action the caller handed over), every other row by action.  No torch or HIP at module level."""
import numpy as np

from native_replay_cases import DISCOUNT, QUEUE, REPEAT, S, T
from parity_helpers import _result_arrays, make_search_config, softmax64, support_to_scalar64


def search_config(case, simulations=S):
    return make_search_config(case["A"], simulations, case["players"], DISCOUNT, support=case["support"], H=4)


# ---- reading the streams out of exported trees ---------------------------------------------------------------------
def _edge(tree, t, path, legal):
    """(parent node, index of the child record in the parent's row) of the last edge of `path`, walked from the root
    through child_node."""
    node = 0
    for d, action in enumerate(path):
        index = legal.index(int(action)) if node == 0 else int(action)
        if d == len(path) - 1:
            return node, index
        node = int(tree["child_node"][t, node, index])
        assert node > 0, f"tree {t}: the path {list(path)} leaves the expanded tree at depth {d}"
    raise AssertionError(f"tree {t}: empty path")


class StreamReader:
    """Reads the decoded outputs of one simulation after the other out of the trees exported after each (`read`, in
    order); `value` [T, S], `reward` [T, S] and `priors` [T, S, A] fill up.  The reading checks itself, so a wrong index
    fails instead of yielding plausible numbers: the edge was unexpanded before the simulation, its node is the one
    simulation s creates (s + 1), visited once, none of that node's children is visited or expanded, and every edge of
    the path above it leads to a node expanded earlier."""

    def __init__(self, legal, n_sims, A):
        self.legal = [[int(a) for a in row] for row in legal]
        n_trees = len(self.legal)
        self.value, self.reward = np.zeros((n_trees, n_sims)), np.zeros((n_trees, n_sims))
        self.priors = np.zeros((n_trees, n_sims, A))
        self.done, self.before = 0, None

    def read(self, tree, depth, actions):
        """tree: {key: [T, S + 1, A]} right after simulation `done`; depth [T], actions [T, >= depth]: its paths."""
        s, before = self.done, self.before
        for t, legal in enumerate(self.legal):
            d = int(depth[t])
            assert d >= 1 and (np.asarray(actions[t, :d]) >= 0).all(), (t, s, d)
            parent, index = _edge(tree, t, actions[t, :d], legal)
            node = int(tree["child_node"][t, parent, index])
            where = f"tree {t}, simulation {s}, edge ({parent}, {index})"
            assert node == s + 1, f"{where}: child_node is {node}, the node this simulation creates is {s + 1}"
            if before is not None:
                assert before["child_node"][t, parent, index] == -1 and before["visits"][t, parent, index] == 0, \
                    f"{where}: expanded before its simulation"
            assert tree["visits"][t, parent, index] == 1, f"{where}: visited {tree['visits'][t, parent, index]} times"
            assert (tree["visits"][t, node] == 0).all() and (tree["child_node"][t, node] == -1).all(), \
                f"{where}: the new node {node} already has visited or expanded children"
            self.value[t, s] = tree["value_sum"][t, parent, index]
            self.reward[t, s] = tree["reward"][t, parent, index]
            self.priors[t, s] = tree["prior"][t, node]
        self.done, self.before = s + 1, {k: tree[k] for k in ("child_node", "visits")}


def decoded_streams(exports, depth, actions, legal):
    """exports[s]: {key: [T, S + 1, A]} right after simulation s; depth [T, S], actions [T, S, >= depth] the path of every
    simulation; legal: per tree the root's actions in slot order.  Returns value [T, S], reward [T, S], priors [T, S, A]
    (StreamReader over the whole search)."""
    reader = StreamReader(legal, len(exports), exports[0]["visits"].shape[2])
    for s, tree in enumerate(exports):
        reader.read(tree, depth[:, s], actions[:, s])
    return reader.value, reader.reward, reader.priors


def export_trees(engine, n_trees):
    """mzmcts_export_tree of the first n_trees envs, stacked: {key: [n_trees, S + 1, A]}."""
    trees = [engine.export_tree(e) for e in range(n_trees)]
    return {k: np.stack([tree[k] for tree in trees]) for k in trees[0]}


def streams_for(case, root_priors, value, reward, priors):
    """The injected streams of a case (parity_helpers.random_streams layout).  The root's reward is exactly 0: its logits
    are the one-hot-centre row (native_replay_cases.log_onehot_centre)."""
    return dict(seeds=case["seeds"], legal=case["legal"], to_play=case["to_play"], root_reward=np.zeros(T),
                root_priors=np.asarray(root_priors, dtype=np.float64), value=value, reward=reward, priors=priors)


# ---- the same streams from the float64 reference: what the cases reach, without a GPU ------------------------------------
def _f32(x):
    return np.asarray(x, dtype=np.float32).astype(np.float64)


def decode64(logits, support):
    """support_to_scalar64 rounded to float32 (a storm tree's one-hot-centre rows give exactly 0: sign(0) = 0)."""
    return _f32(support_to_scalar64(logits, support))


def reference_streams(case):
    """The streams the float64 decode of the case's logits gives, every number rounded to float32 as the kernels' are."""
    A = case["A"]
    root_priors = np.zeros((T, A))
    for t, legal in enumerate(case["legal"]):
        root_priors[t, :len(legal)] = _f32(softmax64(case["root_policy_logits"][t][legal]))
    return streams_for(case, root_priors, decode64(case["value_logits"], case["support"]),
                       decode64(case["reward_logits"], case["support"]), _f32(softmax64(case["policy_logits"])))


def oracle_exports(oracle, cfg, streams, t):
    """Tree t of `streams` searched on the C oracle one simulation at a time; after each the whole tree as
    mzmcts_export_tree lays it out, built from Tree.node_stats along the oracle's own paths (node k is the one simulation
    k - 1 created).  Returns (exports [S] of {key: [1, S + 1, A]}, depth [1, S], actions [1, S, S + 1])."""
    ocfg = oracle.config_from_muzero(cfg)
    A, n_sims = ocfg.A, ocfg.S
    legal = streams["legal"][t]
    rng = oracle.Rng(streams["seeds"][t])
    tree = oracle.Tree(ocfg)
    tree.reset(rng, legal, streams["to_play"][t], 0.0, root_priors=streams["root_priors"][t][:len(legal)])
    node_paths, exports = [[]], []
    for s in range(n_sims):
        tree.simulate(rng, first=s, n=1, value=streams["value"][t], reward=streams["reward"][t], priors=streams["priors"][t])
        node_paths.append(tree.sim_actions[s, :tree.sim_depth[s]].tolist())
        index_of = {tuple(p): k for k, p in enumerate(node_paths)}
        out = dict(visits=np.zeros((1, n_sims + 1, A), np.int32), value_sum=np.zeros((1, n_sims + 1, A)),
                   prior=np.zeros((1, n_sims + 1, A)), reward=np.zeros((1, n_sims + 1, A)),
                   child_node=np.full((1, n_sims + 1, A), -1, np.int32))
        for k, path in enumerate(node_paths):
            for index, action in enumerate(legal if k == 0 else range(A)):
                st = tree.node_stats(path + [action])
                out["visits"][0, k, index], out["value_sum"][0, k, index] = st["visit"], st["value_sum"]
                out["prior"][0, k, index], out["reward"][0, k, index] = st["prior"], st["reward"]
                out["child_node"][0, k, index] = index_of.get(tuple(path + [action]), -1)
        exports.append(out)
    return exports, tree.sim_depth[None].copy(), tree.sim_actions[None].copy()


def dirichlet_words(oracle, case):
    """32-bit words the root noise takes from each tree's stream: what a search draws beyond them are tie-breaks."""
    cfg = search_config(case)
    words = np.zeros(T, np.int64)
    for t in range(T):
        rng = oracle.Rng(case["seeds"][t])
        rng.dirichlet(float(cfg.root_dirichlet_alpha), len(case["legal"][t]))
        words[t] = rng.words
    return words


# ---- the native search on the card ---------------------------------------------------------------------------------
def _tile(a, repeat):
    return np.concatenate([a] * repeat, axis=0)


def _device_inputs(case, repeat):
    import torch

    def cuda(a):
        return torch.from_numpy(np.ascontiguousarray(_tile(a, repeat))).cuda()

    return {k: cuda(case[k]) for k in ("value_logits", "reward_logits", "policy_logits", "root_value_logits",
                                       "root_reward_logits", "root_policy_logits")}


def native_root_priors(engine_mod, case, G=None):
    """The root's priors before the noise, by child slot: the same engine form with add_exploration_noise=False."""
    import torch
    dev = _device_inputs(case, 1)
    engine = engine_mod.BatchedMCTS(search_config(case), T, seeds=case["seeds"], group_width=case["gw"])
    try:
        assert G is None or engine.group_width() == G
        engine.begin_search(case["legal"], case["to_play"], False)
        engine.expand_roots(dev["root_value_logits"], dev["root_reward_logits"], dev["root_policy_logits"],
                            torch.zeros(T, 4, device="cuda"))
        return engine.readout()["child_prior"].copy()
    finally:
        engine.close()


def run_native_on_engine(engine_mod, case, form, G=None):
    """Drive a native search of `case` (logits in, the kernels decode) in one of native_replay_cases.FORMS; the trees are
    tiled REPEAT[form] times.  Returns (result arrays of the first T envs as run_injected_on_engine lays them out, with
    `all_equal` over the copies; exports [S] of {key: [T, S + 1, A]}, one per simulation)."""
    import torch
    repeat, queue, fused = REPEAT[form], QUEUE.get(form, 0), form == "fused"
    E, A = T * repeat, case["A"]
    dev = _device_inputs(case, repeat)
    hidden = torch.zeros(E, 4, device="cuda")
    engine = engine_mod.BatchedMCTS(search_config(case), E, seeds=case["seeds"] * repeat, group_width=case["gw"])
    try:
        assert G is None or engine.group_width() == G
        engine.set_debug_ties(True)
        if queue:
            engine.set_select_queue(queue)
        engine.begin_search(case["legal"] * repeat, case["to_play"] * repeat, True)
        out = _result_arrays(E, A, S)
        out["noise"][:] = engine.noise
        engine.expand_roots(dev["root_value_logits"], dev["root_reward_logits"], dev["root_policy_logits"], hidden)
        exports = []
        for s in range(S):
            if s == 0 or not fused:
                engine.select()
            depth, actions, ties = engine.last_paths(with_ties=True)
            out["sim_depth"][:, s], out["sim_actions"][:, s, :], out["sim_ties"][:, s, :] = depth, actions, ties
            step = engine.expand_backup_select if fused and s + 1 < S else engine.expand_backup
            step(dev["value_logits"][:, s], dev["reward_logits"][:, s], dev["policy_logits"][:, s], hidden)
            exports.append(export_trees(engine, T))
        st = engine.readout()
        for key in ("visits", "child_value_sum", "child_prior", "child_reward", "root_value_sum", "root_visits",
                    "max_tree_depth", "min_max"):
            out[key][:] = st[key]
        out["tie_break_words"] = st["tie_break_words"].copy()
        out["depth_sum"] = st["depth_sum"].copy()
        out["child_visits_target"][:], out["root_value_target"][:] = engine.search_statistics()
        out["action"][:] = engine.sample_actions(case["temperature"] * repeat)[0]
        torch.cuda.synchronize()
    finally:
        engine.close()
    all_equal = all(np.array_equal(arr[:T], arr[r * T:(r + 1) * T]) for arr in out.values() for r in range(1, repeat))
    result = {k: v[:T] for k, v in out.items()}
    result["all_equal"] = all_equal
    return result, exports
