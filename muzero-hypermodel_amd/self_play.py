"""Drop-in for the reference's self_play.py: SelfPlay, MCTS, Node, GameHistory, MinMaxStats.

Same class names, method names, signatures and return values (reference self_play.py:11-568), so
`muzero.py`-style orchestration, `diagnose_model.py`-style inspection and the replay buffer / trainer
keep working -- but the search itself runs on the MI355X:

  * `MCTS(config).run(...)` drives the HIP engine (engine.BatchedMCTS, one tree) and returns a `Node`
    tree materialised from the device pools plus the same `extra_info` dict;
  * `SelfPlay` is a plain class (no Ray): `.play_game`, `.continuous_self_play`, `.close_game`,
    `.select_opponent_action` and the static `.select_action`;
  * `BatchedSelfPlay` is the MI355X-native way to use the engine: E games in lock step, one actor per
    GPU, each env on the RNG stream of reference worker `config.seed + e`.

Randomness: the reference uses numpy's global legacy generator for everything.  The single-tree
facade hands that global state to the engine's stream before a search and hands it back afterwards
(`numpy.random.get_state/set_state`), so a run interleaves with any other user of `numpy.random`
(games, expert agents) exactly as the reference does.
"""
import dataclasses
import math
import time
import typing

import numpy
import torch

from . import _native, models
from .engine import BatchedMCTS


class SelfPlay:
    """Plays games with MCTS at every move and hands them to the replay buffer
    (reference self_play.py:11-246)."""

    def __init__(self, initial_checkpoint, Game, config, seed):
        self.config = config
        self.game = Game(seed)

        # Fix random generator seed (self_play.py:22-23)
        numpy.random.seed(seed)
        torch.manual_seed(seed)

        self.model = models.MuZeroNetwork(self.config)
        self.model.set_weights(initial_checkpoint["weights"])
        self.model.to(torch.device("cuda" if torch.cuda.is_available() else "cpu"))
        self.model.eval()
        self._mcts = None

    def _searcher(self):
        if self._mcts is None:
            self._mcts = MCTS(self.config)
        return self._mcts

    def continuous_self_play(self, shared_storage, replay_buffer, test_mode=False):
        """Game loop (self_play.py:31-108).  `shared_storage` / `replay_buffer` are any objects with
        `get_info` / `set_info` / `save_game` methods (called directly: there is no Ray here)."""
        while (shared_storage.get_info("training_step") < self.config.training_steps
               and not shared_storage.get_info("terminate")):
            self.model.set_weights(shared_storage.get_info("weights"))

            if not test_mode:
                game_history = self.play_game(
                    self.config.visit_softmax_temperature_fn(
                        trained_steps=shared_storage.get_info("training_step")),
                    self.config.temperature_threshold, False, "self", 0)
                replay_buffer.save_game(game_history, shared_storage)
            else:
                # Take the best action (no exploration) in test mode
                game_history = self.play_game(
                    0, self.config.temperature_threshold, False,
                    "self" if len(self.config.players) == 1 else self.config.opponent,
                    self.config.muzero_player)
                shared_storage.set_info({
                    "episode_length": len(game_history.action_history) - 1,
                    "total_reward": sum(game_history.reward_history),
                    "mean_value": numpy.mean([value for value in game_history.root_values if value]),
                })
                if 1 < len(self.config.players):
                    mine = self.config.muzero_player
                    shared_storage.set_info({
                        "muzero_reward": sum(
                            reward for i, reward in enumerate(game_history.reward_history)
                            if game_history.to_play_history[i - 1] == mine),
                        "opponent_reward": sum(
                            reward for i, reward in enumerate(game_history.reward_history)
                            if game_history.to_play_history[i - 1] != mine),
                    })

            # Managing the self-play / training ratio
            if not test_mode and self.config.self_play_delay:
                time.sleep(self.config.self_play_delay)
            if not test_mode and self.config.ratio:
                while (shared_storage.get_info("training_step")
                       / max(1, shared_storage.get_info("num_played_steps")) < self.config.ratio
                       and shared_storage.get_info("training_step") < self.config.training_steps
                       and not shared_storage.get_info("terminate")):
                    time.sleep(0.5)

        self.close_game()

    def play_game(self, temperature, temperature_threshold, render, opponent, muzero_player):
        """One game, MCTS at every move (self_play.py:110-184)."""
        game_history = GameHistory()
        observation = self.game.reset()
        game_history.action_history.append(0)
        game_history.observation_history.append(observation)
        game_history.reward_history.append(0)
        game_history.to_play_history.append(self.game.to_play())

        done = False
        if render:
            self.game.render()

        with torch.no_grad():
            while not done and len(game_history.action_history) <= self.config.max_moves:
                shape = numpy.array(observation).shape
                assert len(shape) == 3, (
                    f"Observation should be 3 dimensionnal instead of {len(shape)} dimensionnal. "
                    f"Got observation of shape: {shape}")
                assert shape == self.config.observation_shape, (
                    "Observation should match the observation_shape defined in MuZeroConfig. "
                    f"Expected {self.config.observation_shape} but got {shape}.")
                stacked_observations = game_history.get_stacked_observations(
                    -1, self.config.stacked_observations)

                # Choose the action
                if opponent == "self" or muzero_player == self.game.to_play():
                    root, mcts_info = self._searcher().run(
                        self.model, stacked_observations, self.game.legal_actions(),
                        self.game.to_play(), True)
                    action = self.select_action(
                        root,
                        temperature
                        if not temperature_threshold
                        or len(game_history.action_history) < temperature_threshold
                        else 0)
                    if render:
                        print(f'Tree depth: {mcts_info["max_tree_depth"]}')
                        print(f"Root value for player {self.game.to_play()}: {root.value():.2f}")
                else:
                    action, root = self.select_opponent_action(opponent, stacked_observations)

                observation, reward, done = self.game.step(action)

                if render:
                    print(f"Played action: {self.game.action_to_string(action)}")
                    self.game.render()

                game_history.store_search_statistics(root, self.config.action_space)

                # Next batch
                game_history.action_history.append(action)
                game_history.observation_history.append(observation)
                game_history.reward_history.append(reward)
                game_history.to_play_history.append(self.game.to_play())

        return game_history

    def close_game(self):
        self.game.close()
        if self._mcts is not None:
            self._mcts.close()
            self._mcts = None

    def select_opponent_action(self, opponent, stacked_observations):
        """Opponent move when evaluating MuZero (self_play.py:189-221)."""
        if opponent == "human":
            root, mcts_info = self._searcher().run(
                self.model, stacked_observations, self.game.legal_actions(), self.game.to_play(), True)
            print(f'Tree depth: {mcts_info["max_tree_depth"]}')
            print(f"Root value for player {self.game.to_play()}: {root.value():.2f}")
            print(f"Player {self.game.to_play()} turn. MuZero suggests "
                  f"{self.game.action_to_string(self.select_action(root, 0))}")
            return self.game.human_to_action(), root
        elif opponent == "expert":
            return self.game.expert_agent(), None
        elif opponent == "random":
            assert self.game.legal_actions(), (
                f"Legal actions should not be an empty array. Got {self.game.legal_actions()}.")
            assert set(self.game.legal_actions()).issubset(set(self.config.action_space)), (
                "Legal actions should be a subset of the action space.")
            return numpy.random.choice(self.game.legal_actions()), None
        else:
            raise NotImplementedError(
                'Wrong argument: "opponent" argument should be "self", "human", "expert" or "random"')

    @staticmethod
    def select_action(node, temperature):
        """Sample the played action from the root's visit counts (self_play.py:223-246).

        Uses the engine's numpy-legacy generator on numpy's global state, so the draw (and the number
        of random words consumed) is the reference's."""
        visit_counts = numpy.array([child.visit_count for child in node.children.values()], dtype="int32")
        actions = [action for action in node.children.keys()]
        if temperature == 0:
            return actions[numpy.argmax(visit_counts)]
        rng = _native.HostRng(0)
        rng.set_state(numpy.random.get_state())
        slot = rng.select_action(visit_counts, temperature)
        numpy.random.set_state(rng.get_state())
        return actions[slot]


# Game independent
class MCTS:
    """Monte-Carlo tree search (self_play.py:250-431), executed by the HIP engine.

    `run` keeps the reference signature.  `select_child`, `ucb_score` and `backpropagate` are kept
    for callers that drive a search by hand on `Node` objects (diagnose-style tooling); they are
    host-side conveniences and are not used by `run`."""

    def __init__(self, config):
        self.config = config
        self._engine = None

    def _get_engine(self, device, model):
        if self._engine is None:
            self._engine = BatchedMCTS(self.config, 1, device=device, seeds=[0],
                                       group_width=16 if len(self.config.action_space) <= 16 else 0)
            self._engine_model = None
        if self.config.network == "fullyconnected" and self._engine_model is not model:
            # fully-connected networks run the whole search in one fused HIP launch; the model's parameters
            # become views into one flat buffer (values unchanged, set_weights keeps working)
            try:
                self._engine.configure_fused_fc(model)
            except (NotImplementedError, RuntimeError):
                pass                                # shape outside the fused kernel's range: lock-step path
            self._engine_model = model
        return self._engine

    def close(self):
        if self._engine is not None:
            self._engine.close()
            self._engine = None

    def run(self, model, observation, legal_actions, to_play, add_exploration_noise,
            override_root_with=None):
        """Search from `observation`; returns (root Node, {"max_tree_depth", "root_predicted_value"})."""
        if override_root_with:
            return self._run_from_root(model, override_root_with, add_exploration_noise)
        device = next(model.parameters()).device
        if device.type != "cuda":
            raise RuntimeError("MCTS.run needs the model on a HIP device; the engine has no CPU fallback")
        assert legal_actions, f"Legal actions should not be an empty array. Got {legal_actions}."
        assert set(legal_actions).issubset(set(self.config.action_space)), (
            "Legal actions should be a subset of the action space.")
        engine = self._get_engine(device, model)
        engine.set_rng_state(0, numpy.random.get_state())
        obs = torch.tensor(numpy.asarray(observation)).float().unsqueeze(0)
        stats = engine.search(model, obs, [list(legal_actions)], [to_play], add_exploration_noise)
        numpy.random.set_state(engine.get_rng_state(0))

        root = Node._from_engine(engine, list(legal_actions), to_play, len(self.config.players))
        extra_info = {
            "max_tree_depth": int(stats["max_tree_depth"][0]),
            "root_predicted_value": float(stats["root_predicted_value"][0]),
        }
        return root, extra_info

    def _run_from_root(self, model, root_in, add_exploration_noise):
        """`run(..., override_root_with=root)` (self_play.py:276-278; diagnose_model.py builds such roots with
        Node(0).expand(...)): the given root's children (priors), reward, to_play and hidden state are uploaded as the
        search's root instead of being computed from an observation; root_predicted_value is None as in the reference.
        The root must be freshly expanded -- trees are rebuilt in the device pools per search, so visit counts of an
        earlier search cannot be continued."""
        if not root_in.expanded() or root_in.hidden_state is None:
            raise AssertionError("override_root_with must be an expanded node carrying a hidden state")
        if root_in.visit_count or any(c.visit_count or c.expanded() for c in root_in.children.values()):
            raise NotImplementedError("override_root_with: only a freshly expanded root (no visits yet) can be uploaded "
                                      "to the device engine")
        device = next(model.parameters()).device
        if device.type != "cuda":
            raise RuntimeError("MCTS.run needs the model on a HIP device; the engine has no CPU fallback")
        legal_actions = list(root_in.children.keys())
        assert set(legal_actions).issubset(set(self.config.action_space)), (
            "Legal actions should be a subset of the action space.")
        engine = self._get_engine(device, model)
        engine.set_rng_state(0, numpy.random.get_state())
        priors = numpy.zeros((1, engine.A), dtype=numpy.float64)
        priors[0, : len(legal_actions)] = [root_in.children[a].prior for a in legal_actions]
        with torch.no_grad(), torch.cuda.device(engine.device):
            engine.begin_search([legal_actions], [root_in.to_play], add_exploration_noise)
            engine.expand_roots_injected(numpy.array([float(root_in.reward)]), priors)
            engine.pool[0, 0].copy_(torch.as_tensor(root_in.hidden_state).to(engine.device, torch.float32).reshape(-1))
            engine._run_simulations(model)
            stats = engine.readout()
        numpy.random.set_state(engine.get_rng_state(0))
        root = Node._from_engine(engine, legal_actions, root_in.to_play, len(self.config.players))
        return root, {"max_tree_depth": int(stats["max_tree_depth"][0]), "root_predicted_value": None}

    def select_child(self, node, min_max_stats):
        """Child with the highest UCB score, ties broken like the reference (self_play.py:364-379)."""
        scored = [(self.ucb_score(node, child, min_max_stats), action)
                  for action, child in node.children.items()]
        top = max(score for score, _ in scored)
        action = numpy.random.choice([action for score, action in scored if score == top])
        return action, node.children[action]

    def ucb_score(self, parent, child, min_max_stats):
        """Prior exploration bonus + normalised value (self_play.py:381-405)."""
        c = self.config
        pb_c = math.log((parent.visit_count + c.pb_c_base + 1) / c.pb_c_base) + c.pb_c_init
        pb_c *= math.sqrt(parent.visit_count) / (child.visit_count + 1)
        score = pb_c * child.prior
        if child.visit_count > 0:
            q = child.value() if len(c.players) == 1 else -child.value()
            score += min_max_stats.normalize(child.reward + c.discount * q)
        return score

    def backpropagate(self, search_path, value, to_play, min_max_stats):
        """Propagate a leaf evaluation to the root (self_play.py:407-431)."""
        n_players = len(self.config.players)
        if n_players > 2:
            raise NotImplementedError("More than two player mode not implemented.")
        gamma = self.config.discount
        for node in reversed(search_path):
            if n_players == 1:
                node.value_sum += value
                node.visit_count += 1
                min_max_stats.update(node.reward + gamma * node.value())
                value = node.reward + gamma * value
            else:
                mine = node.to_play == to_play
                node.value_sum += value if mine else -value
                node.visit_count += 1
                min_max_stats.update(node.reward + gamma * -node.value())
                value = (-node.reward if mine else node.reward) + gamma * value


class Node:
    """Search-tree node with the reference's attributes (self_play.py:434-477).  Nodes returned by
    `MCTS.run` are views materialised from the engine's device pools after the search."""

    def __init__(self, prior):
        self.visit_count = 0
        self.to_play = -1
        self.prior = prior
        self.value_sum = 0
        self.children = {}
        self.hidden_state = None
        self.reward = 0

    def expanded(self):
        return len(self.children) > 0

    def value(self):
        if self.visit_count == 0:
            return 0
        return self.value_sum / self.visit_count

    def expand(self, actions, to_play, reward, policy_logits, hidden_state):
        """Give the node children with softmax priors over `actions` (self_play.py:452-466)."""
        self.to_play = to_play
        self.reward = reward
        self.hidden_state = hidden_state
        priors = torch.softmax(torch.tensor([policy_logits[0][a] for a in actions]), dim=0).tolist()
        for action, p in zip(actions, priors):
            self.children[action] = Node(p)

    def add_exploration_noise(self, dirichlet_alpha, exploration_fraction):
        """Mix Dirichlet noise into the children's priors (self_play.py:468-477)."""
        actions = list(self.children.keys())
        noise = numpy.random.dirichlet([dirichlet_alpha] * len(actions))
        frac = exploration_fraction
        for a, n in zip(actions, noise):
            self.children[a].prior = self.children[a].prior * (1 - frac) + n * frac

    @classmethod
    def _from_engine(cls, engine, legal_actions, to_play, n_players, env=0):
        """Rebuild the whole tree of `env` from the exported child-record pools."""
        tree = engine.export_tree(env)
        stats = engine.stats
        state_shape = engine.state_shape

        def hidden(k):
            return engine.pool[k, env].view(1, *state_shape)

        root = cls(0)
        root.visit_count = int(stats["root_visits"][env])
        root.value_sum = float(stats["root_value_sum"][env])
        root.to_play = to_play
        root.reward = 0.0
        root.hidden_state = hidden(0)
        stack = [(root, 0, 0)]  # (node, expanded-node index, tree depth)
        while stack:
            node, k, depth = stack.pop()
            actions = legal_actions if k == 0 else range(engine.A)
            for slot, action in enumerate(actions):
                child = cls(float(tree["prior"][k, slot]))
                child.visit_count = int(tree["visits"][k, slot])
                child.value_sum = float(tree["value_sum"][k, slot])
                child.reward = float(tree["reward"][k, slot])
                node.children[action] = child
                ck = int(tree["child_node"][k, slot])
                if ck >= 0:
                    child.to_play = (to_play + depth + 1) % n_players
                    child.hidden_state = hidden(ck)
                    stack.append((child, ck, depth + 1))
        return root


class GameHistory:
    """What is stored of a self-play game (self_play.py:480-548)."""

    def __init__(self):
        self.observation_history = []
        self.action_history = []
        self.reward_history = []
        self.to_play_history = []
        self.child_visits = []
        self.root_values = []
        self.reanalysed_predicted_root_values = None
        # For PER
        self.priorities = None
        self.game_priority = None

    def store_search_statistics(self, root, action_space):
        """Turn the root's visit counts into a policy target (self_play.py:497-512)."""
        if root is None:
            self.root_values.append(None)
            return
        total = sum(child.visit_count for child in root.children.values())
        self.child_visits.append(
            [root.children[a].visit_count / total if a in root.children else 0 for a in action_space])
        self.root_values.append(root.value())

    def get_stacked_observations(self, index, num_stacked_observations):
        """Observation at `index` followed by the previous observations, each with the plane of the
        action that led out of it; zero planes before the start of the game (self_play.py:514-548)."""
        index = index % len(self.observation_history)
        planes = [self.observation_history[index].copy()]
        like_plane = numpy.ones_like(planes[0][0])
        for past in range(index - 1, index - num_stacked_observations - 1, -1):
            if past >= 0:
                planes.append(self.observation_history[past])
                planes.append([like_plane * self.action_history[past + 1]])
            else:
                planes.append(numpy.zeros_like(self.observation_history[index]))
                planes.append([numpy.zeros_like(planes[0][0])])
        return numpy.concatenate(planes) if len(planes) > 1 else planes[0]


class MinMaxStats:
    """Running min / max of the values seen in one search tree (self_play.py:551-568)."""

    def __init__(self):
        self.maximum = -float("inf")
        self.minimum = float("inf")

    def update(self, value):
        self.maximum = max(self.maximum, value)
        self.minimum = min(self.minimum, value)

    def normalize(self, value):
        if self.maximum > self.minimum:
            # only once both bounds have been set
            return (value - self.minimum) / (self.maximum - self.minimum)
        return value


class ManyEnvLoop:
    """`continuous_self_play` for the many-env actors (BatchedSelfPlay, DeviceSelfPlay): the reference's loop
    (self_play.py:31-108) with one actor playing E games at once.

    One pass of the loop = the reference's pass for one game, in the same order of storage calls:
        loop condition   get_info("training_step"), get_info("terminate")
        weight pull      get_info("weights") -> set_weights           (self_play.py:37: before every game)
        training         temperature = visit_softmax_temperature_fn(get_info("training_step")), play until at
                         least one env finishes a game, replay_buffer.save_game(history, shared_storage) per game
        test mode        temperature 0; per finished game set_info({episode_length, total_reward, mean_value})
                         (+ {muzero_reward, opponent_reward} for two players)
        throttle         self_play_delay sleep, then the training_step / num_played_steps < ratio wait
    so with E == 1 the call sequence is the reference's own (fixture G15, tests/test_self_play_loop.py).  With E > 1
    every env that starts a game after a pull plays it with the pulled weights; envs in mid-game switch to them at
    that move boundary, and every game records the weight version (the training step of the
    pull) it started and ended with in `weights_version`.

    `moves_per_pass`: play exactly that many moves per pass instead of "until a game ends" -- required when the
    actors of several GPUs run this loop together (torch.distributed initialised): every rank then makes the same
    collective calls.  Rank 0 alone talks to `shared_storage`; the loop condition travels as a 2-word broadcast and
    the weights as one broadcast of the flat buffer (weights.FlatWeights, RCCL over xGMI) when their version moved."""

    # (opponent, muzero_player) the moves play when a call names none: class-level, because subclasses need not run a
    # base constructor
    _opponent = ("self", 0)
    _paired = False              # ... and whether the opponent replies inside MuZero's move (set_opponent(paired=True))

    def _build_search(self, initial_checkpoint, config, seed, num_envs, device, use_graph):
        """What a single-GPU actor starts from: the checkpoint's network on the device and a search engine of num_envs
        trees, env e on the RNG stream of reference worker seed + e (fully-connected networks: the fused whole-move
        kernel where the shape is in its range)."""
        self.config = config
        self.E = int(num_envs)
        self.device = torch.device(device if device is not None else "cuda")
        torch.manual_seed(seed)
        self.model = models.MuZeroNetwork(config)
        self.model.set_weights(initial_checkpoint["weights"])
        self.model.to(self.device)
        self.model.eval()
        fused = config.network == "fullyconnected"
        self.engine = BatchedMCTS(config, self.E, device=self.device, seeds=[seed + e for e in range(self.E)],
                                  use_graph=use_graph, group_width=16 if fused and len(config.action_space) <= 16 else 0)
        if fused:
            try:
                self.engine.configure_fused_fc(self.model)      # whole move in one HIP launch
            except (NotImplementedError, RuntimeError):
                pass

    def set_opponent(self, opponent, muzero_player=None, paired=False):
        """From now on a step() / play_moves() that names no opponent plays `opponent` ("self", "expert" or "random")
        with MuZero as `muzero_player` (None: the config's).  An opponent the actors cannot play is refused by the
        first move, not here.
        paired=True (device actors' move batches only): the opponent replies inside MuZero's move -- one environment
        launch plays MuZero's ply and the opponent's (games.device.DeviceEnvs.advance_paired), so that every env is
        searched in every move instead of sitting every other search out.  The games are the same games."""
        self._opponent = (opponent, self.config.muzero_player if muzero_player is None else muzero_player)
        self._paired = bool(paired)

    def _resolve_opponent(self, opponent, muzero_player, paired=None):
        """The (opponent, muzero_player, paired) one call plays: its own arguments, else what set_opponent stored."""
        if opponent is None:
            opponent, muzero_player = self._opponent
            paired = self._paired if paired is None else paired
        elif muzero_player is None:
            muzero_player = self.config.muzero_player
        if opponent not in ("self", "expert", "random"):
            raise NotImplementedError('many-env actors play opponent "self", "expert" or "random" ("human": use SelfPlay)')
        return (opponent, int(muzero_player), bool(paired)) if opponent != "self" else ("self", 0, False)

    def _loop_state(self):
        st = self.__dict__.get("_loop")
        if st is None:
            st = self.__dict__["_loop"] = dict(version=0, started=numpy.zeros(self.E, dtype=numpy.int64), flat=None)
        return st

    def _distributed(self):
        import torch.distributed as dist
        return dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1

    def _loop_control(self, shared_storage, training_steps):
        """(training_step, terminate) as every rank must see them."""
        if not self._distributed():
            step = shared_storage.get_info("training_step")
            return step, (step >= training_steps or shared_storage.get_info("terminate"))
        import torch.distributed as dist
        word = torch.zeros(2, dtype=torch.int64, device=self.device if dist.get_backend() == "nccl" else "cpu")
        if dist.get_rank() == 0:
            step = shared_storage.get_info("training_step")
            word[0], word[1] = int(step), int(step >= training_steps or bool(shared_storage.get_info("terminate")))
        dist.broadcast(word, src=0)
        return int(word[0]), bool(word[1])

    def _pull_weights(self, shared_storage, version):
        st = self._loop_state()
        if not self._distributed():
            self.set_weights(shared_storage.get_info("weights"))
        else:
            import torch.distributed as dist
            from .weights import FlatWeights
            if st["flat"] is None:
                st["flat"] = FlatWeights(self.model)
            if dist.get_rank() == 0:
                st["flat"].load_state_dict(shared_storage.get_info("weights"))
            st["flat"].broadcast(src=0)
        st["version"] = int(version)

    def _play_pass(self, temperature, temperature_threshold, moves_per_pass):
        """Play until a game ends (moves_per_pass None) or exactly moves_per_pass moves; returns the finished games
        as (env index, GameHistory) pairs in the order they ended."""
        finished = []
        moves = 0
        while True:
            self.step(temperature, temperature_threshold, on_game=lambda e, gh: finished.append((e, gh)))
            moves += 1
            if (moves_per_pass is None and finished) or (moves_per_pass is not None and moves >= moves_per_pass):
                return finished

    def _filed_counters(self):
        """(num_played_games, num_played_steps) of the replay store an actor files its games into itself, else None."""
        return None

    def continuous_self_play(self, shared_storage, replay_buffer, test_mode=False, moves_per_pass=None):
        cfg = self.config
        st = self._loop_state()
        if self._distributed() and moves_per_pass is None:
            raise ValueError("several ranks: give moves_per_pass so that every rank makes the same collective calls")
        # test mode against an opponent (self_play.py:65-90: play_game(0, threshold, False, config.opponent,
        # config.muzero_player) for games with several players): the actors whose step() takes an opponent play it
        if test_mode and len(cfg.players) > 1:
            self.set_opponent(cfg.opponent, cfg.muzero_player)
        else:
            self.set_opponent("self", 0)
        talker = not self._distributed() or torch.distributed.get_rank() == 0
        while True:
            step, stop = self._loop_control(shared_storage, cfg.training_steps)
            if stop:
                break
            self._pull_weights(shared_storage, step)
            if not test_mode:
                temperature = cfg.visit_softmax_temperature_fn(
                    trained_steps=shared_storage.get_info("training_step") if talker else step)
            else:
                temperature = 0                          # best action, no exploration noise in the sampling
            finished = self._play_pass(temperature, cfg.temperature_threshold, moves_per_pass)
            counters = self._filed_counters()
            if counters is not None and talker:
                # the pass filed its games on the device: they are in the store, only the counters travel
                shared_storage.set_info("num_played_games", counters[0])
                shared_storage.set_info("num_played_steps", counters[1])
            for e, game_history in finished:
                game_history.weights_version = (int(st["started"][e]), st["version"])
                st["started"][e] = st["version"]
                if not test_mode:
                    replay_buffer.save_game(game_history, shared_storage)
                elif talker:
                    shared_storage.set_info({
                        "episode_length": len(game_history.action_history) - 1,
                        "total_reward": sum(game_history.reward_history),
                        "mean_value": numpy.mean([value for value in game_history.root_values if value]),
                    })
                    if 1 < len(cfg.players):
                        mine = cfg.muzero_player
                        shared_storage.set_info({
                            "muzero_reward": sum(reward for i, reward in enumerate(game_history.reward_history)
                                                 if game_history.to_play_history[i - 1] == mine),
                            "opponent_reward": sum(reward for i, reward in enumerate(game_history.reward_history)
                                                   if game_history.to_play_history[i - 1] != mine),
                        })
            # Managing the self-play / training ratio (self_play.py:92-106)
            if not test_mode and cfg.self_play_delay:
                time.sleep(cfg.self_play_delay)
            if not test_mode and cfg.ratio and talker:
                while (shared_storage.get_info("training_step")
                       / max(1, shared_storage.get_info("num_played_steps")) < cfg.ratio
                       and shared_storage.get_info("training_step") < cfg.training_steps
                       and not shared_storage.get_info("terminate")):
                    time.sleep(0.5)
        self.close()


class BatchedSelfPlay(ManyEnvLoop):
    """E games in lock step on one GPU: the MI355X-native actor.

    Env e plays with `Game(seed + e)` and the RNG stream of reference worker `seed + e`
    (muzero.py:170-178), so with E == 1 it reproduces `SelfPlay.play_game`, and with E > 1 each env
    reproduces what the reference's e-th Ray worker would have played with the same weights.
    Finished games are handed to `on_game(env_index, GameHistory)` and their env restarts at once.
    """

    def __init__(self, initial_checkpoint, Game, config, seed, num_envs, device=None, use_graph=True):
        self.games = [Game(seed + e) for e in range(int(num_envs))]
        self._build_search(initial_checkpoint, config, seed, num_envs, device, use_graph)
        self.histories = [None] * self.E
        self.observations = [None] * self.E
        self.moves_played = 0
        self.games_finished = 0
        for e in range(self.E):
            self._restart(e)

    def _restart(self, e):
        gh = GameHistory()
        obs = self.games[e].reset()
        gh.action_history.append(0)
        gh.observation_history.append(obs)
        gh.reward_history.append(0)
        gh.to_play_history.append(self.games[e].to_play())
        self.histories[e] = gh
        self.observations[e] = obs

    def set_weights(self, weights):
        self.model.set_weights(weights)

    def step(self, temperature, temperature_threshold=None, on_game=None, opponent=None, muzero_player=None):
        """One move in every env (the body of play_game's loop, self_play.py:129-182).  `opponent` / `muzero_player`
        (default: what set_opponent stored, else "self"): in an env where it is not MuZero's turn the move comes from
        select_opponent_action (self_play.py:189-221) -- the plugin's expert_agent(), or
        numpy.random.choice over the legal actions drawn on THAT env's stream -- and no search statistics are stored
        for it (root None: store_search_statistics appends only a None root value, self_play.py:497-512)."""
        cfg = self.config
        opponent, muzero_player, paired = self._resolve_opponent(opponent, muzero_player)
        if paired:
            raise NotImplementedError("paired replies are played by the device environment kernels (DeviceSelfPlay move "
                                      "batches); host envs play the opponent's ply as a move of its own")
        searching = [opponent == "self" or muzero_player == self.games[e].to_play() for e in range(self.E)]
        stacked = numpy.stack([
            self.histories[e].get_stacked_observations(-1, cfg.stacked_observations)
            for e in range(self.E)]).astype(numpy.float32)
        legal = [self.games[e].legal_actions() if searching[e] else [] for e in range(self.E)]
        to_play = [self.games[e].to_play() for e in range(self.E)]
        self.engine.search(self.model, stacked, legal, to_play, True)     # (an empty legal set = env not searched)
        temps = numpy.array([
            temperature if not temperature_threshold
            or len(self.histories[e].action_history) < temperature_threshold else 0
            for e in range(self.E)], dtype=numpy.float64)
        actions, _ = self.engine.sample_actions(temps)
        child_visits, root_values = self.engine.search_statistics()
        for e in range(self.E):
            gh = self.histories[e]
            if searching[e]:
                action = int(actions[e])
                gh.child_visits.append([float(v) if a in legal[e] else 0 for a, v in enumerate(child_visits[e])])
                gh.root_values.append(float(root_values[e]))
            else:
                action = self._opponent_action(e, opponent)
                gh.root_values.append(None)
            observation, reward, done = self.games[e].step(action)
            gh.action_history.append(action)
            gh.observation_history.append(observation)
            gh.reward_history.append(reward)
            gh.to_play_history.append(self.games[e].to_play())
            self.observations[e] = observation
            if done or len(gh.action_history) > cfg.max_moves:
                self.games_finished += 1
                if on_game is not None:
                    on_game(e, gh)
                self._restart(e)
        self.moves_played += self.E

    def _opponent_action(self, e, opponent):
        """select_opponent_action (self_play.py:189-221) for env e.  The reference's opponents draw from numpy's GLOBAL
        generator, which in a reference worker is also the search's stream (expert agents start from a random legal move:
        games/tictactoe.py:307-312, games/connect4.py:306-343): env e's stream is lent to numpy for the call and handed
        back to the engine afterwards (host mirror and device copy move together)."""
        game = self.games[e]
        saved = numpy.random.get_state()
        numpy.random.set_state(self.engine.get_rng_state(e))
        try:
            if opponent == "expert":
                action = game.expert_agent()
            else:
                legal = game.legal_actions()
                assert legal, f"Legal actions should not be an empty array. Got {legal}."
                assert set(legal).issubset(set(self.config.action_space)), "Legal actions should be a subset of the action space."
                action = numpy.random.choice(legal)
            self.engine.set_rng_state(e, numpy.random.get_state())
        finally:
            numpy.random.set_state(saved)
        return int(action)

    def close(self):
        for g in self.games:
            g.close()
        self.engine.close()


class PackedGames:
    """A batch of finished games as arrays (what a device-side replay buffer would ingest directly).

    Game i has `length[i]` moves; row layouts follow GameHistory (reference self_play.py:116-121, 176-182):
      observations[i, 0..length]   observation_history (index 0 = reset observation)
      actions[i, 0..length]        action_history      (index 0 = the reference's dummy action 0)
      rewards[i, 0..length]        reward_history      (index 0 = 0)
      to_play[i, 0..length]        to_play_history
      child_visits[i, 0..length-1] visit-count targets, root_values[i, 0..length-1]
    Entries past a game's length are padding.  An opponent's ply of an evaluation game keeps its slot: its root value
    is NaN (the reference's None: store_search_statistics(None, ...), self_play.py:497-512) and its child_visits row is
    zero; `history(i)` turns the NaN into None and drops that row, as the reference appends none."""

    __slots__ = ("env_index", "length", "observations", "actions", "rewards", "to_play", "child_visits", "root_values")

    def __init__(self, **arrays):
        for k, v in arrays.items():
            setattr(self, k, v)

    def __len__(self):
        return len(self.env_index)

    def history(self, i):
        """Game i as a reference-shaped GameHistory (Python lists)."""
        n = int(self.length[i])
        gh = GameHistory()
        gh.observation_history = [o.copy() for o in self.observations[i, : n + 1]]   # (the batch may be a view)
        gh.action_history = self.actions[i, : n + 1].tolist()
        gh.reward_history = self.rewards[i, : n + 1].tolist()
        gh.to_play_history = self.to_play[i, : n + 1].tolist()
        root_values = self.root_values[i, :n]
        opponent_ply = numpy.isnan(root_values)
        if opponent_ply.any():
            if self.child_visits[i, :n][opponent_ply].any():
                # (an opponent's ply has a zero row as well: this NaN came out of a search)
                raise ValueError(f"game {i}: a searched ply has a NaN root value")
            gh.child_visits = self.child_visits[i, :n][~opponent_ply].tolist()
            gh.root_values = [None if o else v for v, o in zip(root_values.tolist(), opponent_ply.tolist())]
        else:
            gh.child_visits = self.child_visits[i, :n].tolist()
            gh.root_values = root_values.tolist()
        return gh


class HistoryFiler:
    """Host-side filing of whole move batches into per-env history rows in native code (include/mzhist.h): the rows of
    the running games live here and nowhere else; M moves are filed at once on the library's worker pool
    (tests/test_history_filer.py holds the one-move-at-a-time numpy filing it must equal).  Finished games come back
    as PackedGames whose arrays are views of the library's buffers, valid until the next `file` call."""

    def __init__(self, num_envs, max_moves, observation_shape, num_actions):
        import ctypes
        from . import _native
        self._ct, self._native = ctypes, _native
        self._lib = _native.load()
        self.E, self.L, self.A = int(num_envs), int(max_moves), int(num_actions)
        self.observation_shape = tuple(int(v) for v in observation_shape)
        self.obs_floats = int(numpy.prod(self.observation_shape))
        handle = ctypes.c_void_p()
        if self._lib.mzhist_create(self.E, self.L, self.obs_floats, self.A, ctypes.byref(handle)) != 0:
            raise RuntimeError("mzhist_create failed")
        self._h = handle

    def close(self):
        if getattr(self, "_h", None):
            self._lib.mzhist_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def begin(self, first_observations, first_to_play=None):
        obs = numpy.ascontiguousarray(first_observations, dtype=numpy.float32).reshape(self.E, self.obs_floats)
        tp = None if first_to_play is None else numpy.ascontiguousarray(first_to_play, dtype=numpy.int32)
        self._lib.mzhist_begin(self._h, self._native.ptr(obs, self._native.c_f32_p),
                               None if tp is None else self._native.ptr(tp, self._native.c_i32_p))

    def searched_moves(self):
        """Plies filed so far that were searched (a non-empty legal set): all of them in self-play, MuZero's in
        evaluation games."""
        return int(self._lib.mzhist_searched_moves(self._h))

    def lengths(self):
        """Moves filed so far in every env's running game: an int32 [E] view of the library's own counters, which
        `file` and `begin` update in place (valid as long as this filer)."""
        addr = self._lib.mzhist_lengths(self._h)
        return numpy.ctypeslib.as_array(self._ct.cast(addr, self._ct.POINTER(self._ct.c_int32)), shape=(self.E,))

    def file(self, out, legal, num_legal, num_simulations, rewards, done, obs_after, obs_next, to_play_after=None,
             to_play_next=None, played=None, slots=1, reset_obs=None):
        """out: engine.moves_collect() result (copies or ring views); legal [E,A] / num_legal [E] for the whole batch or
        [M,E,A] / [M,E] per move (engine.moves_inputs); rewards f32 [M,E], done u8 [M,E],
        obs_after / obs_next f32 [M,E,...] host arrays; to_play_after / to_play_next [M,E] for two-player games.
        played int32 [M,E] (evaluation games: the actions the environment kernels actually played): a ply whose legal
        set is empty is then an opponent's -- its action comes from `played`, its root value is NaN, its child_visits
        row zero (include/mzhist.h).
        slots > 1 (a paired batch, games.device.DeviceEnvs.advance_paired): rewards, done, obs_after, to_play_after and
        played carry the slot axis, [M, slots, E, ...]; a move files up to `slots` plies in up to two games of an env --
        slot 0 from the search's blocks, the later slots as opponent plies, an empty slot (played < 0) nothing -- and a game
        that ends inside a move is followed by one that starts from `reset_obs` (f32 observation) with player 0 to move.
        Returns PackedGames of the games that ended, or None."""
        ct = self._ct
        M = int(out["actions"].shape[0])
        def per_move_rows(a):
            # a per-move array whose rows are contiguous goes as it is (ring views: rows a block stride apart)
            a = numpy.asarray(a)
            inner = numpy.empty(a.shape[1:], dtype=numpy.int32).strides
            return a if a.dtype == numpy.int32 and a.ndim >= 2 and a.strides[1:] == inner else numpy.ascontiguousarray(a, dtype=numpy.int32)
        keep = [numpy.ascontiguousarray(out["moves_done"], dtype=numpy.int32),
                per_move_rows(legal) if numpy.ndim(legal) == 3 else numpy.ascontiguousarray(legal, dtype=numpy.int32),
                per_move_rows(num_legal) if numpy.ndim(legal) == 3 else numpy.ascontiguousarray(num_legal, dtype=numpy.int32),
                numpy.ascontiguousarray(rewards, dtype=numpy.float32), numpy.ascontiguousarray(done, dtype=numpy.uint8),
                numpy.ascontiguousarray(obs_after, dtype=numpy.float32), numpy.ascontiguousarray(obs_next, dtype=numpy.float32)]
        mv = self._native.MzHistMoves()
        mv.n_moves, mv.num_simulations = M, int(num_simulations)
        mv.moves_done = keep[0].ctypes.data
        for name, key in (("actions", "actions"), ("visits", "visits"), ("root_value_sum", "root_value_sum")):
            a = out[key]
            setattr(mv, name, a.ctypes.data)
            setattr(mv, name + "_stride", int(a.strides[0]) if M else 0)
        mv.legal, mv.num_legal = keep[1].ctypes.data, keep[2].ctypes.data
        per_move = keep[1].ndim == 3                      # legal [M, E, A], num_legal [M, E]: one set per move
        mv.legal_stride = int(keep[1].strides[0]) if per_move else 0
        mv.num_legal_stride = int(keep[2].strides[0]) if per_move else 0
        mv.rewards, mv.done, mv.obs_after, mv.obs_next = (k.ctypes.data for k in keep[3:7])
        mv.to_play_after = mv.to_play_next = None
        if to_play_after is not None:
            # (a paired batch starts every game with player 0 to move and reads no to_play_next)
            assert to_play_next is not None or slots > 1
            keep += [numpy.ascontiguousarray(to_play_after, dtype=numpy.int32),
                     numpy.ascontiguousarray(to_play_after if to_play_next is None else to_play_next, dtype=numpy.int32)]
            mv.to_play_after, mv.to_play_next = keep[7].ctypes.data, keep[8].ctypes.data
        if played is not None:
            keep.append(numpy.ascontiguousarray(played, dtype=numpy.int32))
            assert keep[-1].shape == ((M, self.E) if slots <= 1 else (M, slots, self.E))
            mv.played = keep[-1].ctypes.data
        if slots > 1:
            keep.append(numpy.ascontiguousarray(reset_obs, dtype=numpy.float32).reshape(self.obs_floats))
            assert keep[3].shape == keep[4].shape == (M, slots, self.E) and keep[5].shape[:3] == (M, slots, self.E)
            assert to_play_after is None or keep[7].shape == (M, slots, self.E)
            mv.slots, mv.reset_obs = int(slots), keep[-1].ctypes.data
        n = ct.c_int32()
        if self._lib.mzhist_file(self._h, ct.byref(mv), ct.byref(n)) != 0:
            raise RuntimeError(self._lib.mzhist_last_error(self._h).decode())
        if n.value == 0:
            return None
        ptrs = [ct.c_void_p() for _ in range(8)]
        row = ct.c_int32()
        count = self._lib.mzhist_finished(self._h, *[ct.byref(p) for p in ptrs], ct.byref(row))
        W = row.value

        def arr(p, ctype, shape):
            return numpy.ctypeslib.as_array(ct.cast(p, ct.POINTER(ctype)), shape=shape)
        return PackedGames(env_index=arr(ptrs[0], ct.c_int32, (count,)), length=arr(ptrs[1], ct.c_int32, (count,)),
                           observations=arr(ptrs[2], ct.c_float, (count, W + 1) + self.observation_shape),
                           actions=arr(ptrs[3], ct.c_int32, (count, W + 1)), rewards=arr(ptrs[4], ct.c_float, (count, W + 1)),
                           to_play=arr(ptrs[5], ct.c_int32, (count, W + 1)),
                           child_visits=arr(ptrs[6], ct.c_double, (count, W, self.A)),
                           root_values=arr(ptrs[7], ct.c_double, (count, W)))


class FiledGames(typing.NamedTuple):
    """The games a move batch finished when the actor files on the device (DeviceSelfPlay.file_to): they are in the replay
    store already; what comes back is 4 bytes per game and the ids the store gave them.  Host arrays, in the order
    PackedGames would have had (env-major, then in move order)."""
    env_index: numpy.ndarray     # int32 [n]
    length: numpy.ndarray        # int32 [n] moves
    game_id: numpy.ndarray       # int64 [n] ascending (consecutive while one actor files into the store)

    def __len__(self):
        return len(self.env_index)


class GameOutcomes(typing.NamedTuple):
    """What finished games report to a training loop's log (the numbers of reference self_play.py:65-90), computed on the
    device where the games lie (csrc/game_outcomes.h): DeviceSelfPlay.take_outcomes() after file_to(outcomes=True), or
    ReplayBuffer.game_outcomes(game_ids) for stored games.  Host arrays, one entry per game."""
    env_index: numpy.ndarray         # int32 [n] (-1: the store does not keep it)
    length: numpy.ndarray            # int32 [n] moves
    game_id: numpy.ndarray           # int64 [n]
    total_reward: numpy.ndarray      # float64 [n] sum(reward_history)
    reward_of_player: numpy.ndarray  # float64 [n, 2] rewards earned on player p's moves ([:, 1] is 0 in one-player games)
    value_sum: numpy.ndarray         # float64 [n] numpy's sum of the non-zero root values
    value_count: numpy.ndarray       # int32 [n] how many those are

    def __len__(self):
        return len(self.env_index)

    @property
    def mean_value(self):
        """numpy.mean([value for value in root_values if value]) per game, bit for bit; nan where no value counts."""
        with numpy.errstate(divide="ignore", invalid="ignore"):
            return self.value_sum / self.value_count

    @classmethod
    def from_records(cls, env_index, length, game_id, records):
        """`records`: a _native.GAME_OUTCOME_DTYPE array parallel to the three lists."""
        return cls(numpy.asarray(env_index, dtype=numpy.int32), numpy.asarray(length, dtype=numpy.int32),
                   numpy.asarray(game_id, dtype=numpy.int64), records["total_reward"].copy(),
                   records["reward_of_player"].reshape(-1, 2).copy(), records["value_sum"].copy(),
                   records["value_count"].copy())

    @classmethod
    def concatenate(cls, parts):
        parts = list(parts)
        if not parts:
            return cls.from_records([], [], [], numpy.zeros(0, dtype=_native.GAME_OUTCOME_DTYPE))
        return cls(*(numpy.concatenate(column) for column in zip(*parts)))


ENV_OUTPUTS = ("reward", "done", "obs_after", "obs_next")    # what the environment kernels return for a move of a batch


class UnfiledBatch(typing.NamedTuple):
    """A collected move batch that HostRows.flush has yet to file: HistoryFiler.file's arguments, as views of the
    engine's download ring and of the rows' pinned host sets (nothing is copied until the filer reads them)."""
    out: dict                                               # engine.moves_collect(copy=False)
    host: dict                                              # ENV_OUTPUTS -> [M, E, ...] host arrays
    legal: numpy.ndarray                                    # [E, A] for the whole batch or [M, E, A] per move
    num_legal: numpy.ndarray                                # [E] or [M, E]
    to_play_after: typing.Optional[numpy.ndarray] = None    # [M, E]; None: player 0 throughout
    to_play_next: typing.Optional[numpy.ndarray] = None
    played: typing.Optional[numpy.ndarray] = None           # [M, E] evaluation games: what the environment kernels played
    slots: int = 1                                          # > 1: a paired batch, host / to_play_after / played [M, slots, E, ...]


@dataclasses.dataclass(slots=True)
class DeviceBatch:
    """A device-input move batch between DeviceSelfPlay._device_batch_begin and _device_batch_end."""
    n_moves: int
    ring: dict                   # the environment kernels' outputs on the device, [n_moves, E, ...] each
    obs_in: torch.Tensor         # what the next move's search reads (the move before's next observation, where it lies)
    threshold: int               # play_game's temperature threshold (0 / None: none)
    pinned: typing.Optional[dict]    # the host set the outputs are downloaded into, move by move (HostRows.next_set)
    opponent: bool               # evaluation games: the kernels also return the played actions and the words drawn
    paired: bool = False         # ... and reply inside MuZero's move (advance_paired): the ring's ply outputs carry a slot axis
    settled: typing.Optional[numpy.ndarray] = None    # plies per env the settle launch in front of the batch played

    @property
    def keys(self):
        return ENV_OUTPUTS + (("played", "words") if self.opponent else ())


class HostRows:
    """Where DeviceSelfPlay's games go by default: the rows of the running games on the host (HistoryFiler), with all a
    move batch needs on its way there -- the two alternating pinned host sets its env outputs are downloaded into, the
    copy stream of those downloads, and the collected batch that waits to be filed.  The actor holds one rows owner and
    never asks which; StoreRows answers the same calls."""

    def __init__(self, engine, envs, config, device, first):
        self.engine, self.envs, self.config, self.device = engine, envs, config, device
        # the running games: one packed row per env in the native filer, long enough for a game of config.max_moves moves
        self.filer = HistoryFiler(envs.E, int(config.max_moves) + 1, envs.observation_shape, envs.A)
        self.filer.begin(first["obs"], first["to_play"])
        self.lengths = self.filer.lengths()     # moves played in env e's current game (the filer's own counters)
        self.pending = None                     # UnfiledBatch: collected, not filed yet
        self._copy_stream = torch.cuda.Stream(device=device)    # downloads of a batch's env outputs
        self._sets, self._flip = {}, 0          # their two alternating host sets (next_set), per ring form
        self._reset_obs = None                  # the observation every game of a board game starts from (paired batches)

    def admit(self, step=False, on_game=None, opponent="self", batched_pass=True):
        pass                                    # host rows take every way of playing

    def per_game(self, on_game):
        return on_game

    def counters(self):
        return None                             # (no store of its own: the loop's replay buffer counts)

    def searched_moves(self, moves_played):
        return self.filer.searched_moves()

    def ring_resized(self, ring, paired=False):
        self._sets[paired] = [{k: torch.zeros(v.shape, dtype=v.dtype).pin_memory() for k, v in ring.items()} for _ in range(2)]

    def next_set(self, paired=False):
        """The host set a batch's env outputs are downloaded into (after ring_resized): two alternate, so that the batch
        waiting to be filed keeps its own.  A paired batch's ring has a form of its own (a slot axis), and so have its sets."""
        self._flip ^= 1
        return self._sets[paired][self._flip]

    def _file_kwargs(self, slots):
        """What a paired batch's filing needs beyond the batch: the slot count and the observation games start from."""
        if slots <= 1:
            return {}
        if self._reset_obs is None:
            self._reset_obs = self.envs.reset_observation()
        return dict(slots=slots, reset_obs=self._reset_obs)

    def file_settled(self, host):
        """The plies of a settle launch (advance_paired with no action: the opponent's pending plies, e.g. its openings)
        are plies of the games: filed as a paired move whose searched slot is empty.  host: the launch's outputs,
        [slots, E, ...] host arrays.  Returns the games they finished (PackedGames or None)."""
        E, A, slots = self.envs.E, self.envs.A, host["played"].shape[0]
        assert not (host["played"][0] >= 0).any()
        none = {"actions": numpy.full((1, E), -1, dtype=numpy.int32), "visits": numpy.zeros((1, E, A), dtype=numpy.int32),
                "root_value_sum": numpy.zeros((1, E), dtype=numpy.float64), "moves_done": numpy.ones(E, dtype=numpy.int32)}
        self.engine.rng_consumed(host["words"].view(numpy.uint32).sum(axis=0, dtype=numpy.uint64))
        mzp = int(self.envs.opponent[1])
        return self.filer.file(none, numpy.zeros((E, A), dtype=numpy.int32), numpy.zeros(E, dtype=numpy.int32),
                               self.config.num_simulations, host["reward"][None], host["done"][None], host["obs_after"][None],
                               host["obs_after"][None, 0], to_play_after=numpy.full((1, slots, E), mzp, dtype=numpy.int32),
                               played=host["played"][None], **self._file_kwargs(slots))

    def download_move(self, b, m):
        # the env outputs of a move (reward, done, the observations the history rows need) go to pinned host memory on a
        # copy stream as soon as the move's env kernel has run: the downloads ride under the batch's remaining searches
        ran = torch.cuda.Event()
        ran.record(torch.cuda.current_stream(self.device))
        self._copy_stream.wait_event(ran)
        with torch.cuda.stream(self._copy_stream):
            for k in b.keys:
                b.pinned[k][m].copy_(b.ring[k][m], non_blocking=True)

    def file_move(self, one, legal, num_legal, reward, over, after, nxt):
        # step_end's move, filed natively (include/mzhist.h, the library's worker pool): a batch of one move whose legal
        # sets are this move's
        return self.filer.file(one, legal, num_legal, self.config.num_simulations, reward[None], over.astype(numpy.uint8)[None],
                               after["obs"][None], nxt["obs"][None], to_play_after=after["to_play"][None],
                               to_play_next=nxt["to_play"][None])

    def queue(self):
        pass

    def flush(self):
        """File the batch that waits (native code, one pass on the library's worker pool): the games it finished as
        PackedGames, or None."""
        u, self.pending = self.pending, None
        if u is None:
            return None
        return self.filer.file(u.out, u.legal, u.num_legal, self.config.num_simulations, u.host["reward"], u.host["done"],
                               u.host["obs_after"], u.host["obs_next"], to_play_after=u.to_play_after,
                               to_play_next=u.to_play_next, played=u.played, **self._file_kwargs(u.slots))

    # the batch before's games leave once the current batch has been enqueued, so that host filing runs under the GPU,
    # and before moves_collect overwrites the engine ring the UnfiledBatch views
    games_before_collect = flush

    def games_after_collect(self):
        return None

    def keep_predrawn(self, out, ring, n_moves, cur):
        """A collected batch of the pre-drawn form becomes the batch that waits; returns the envs' current observations."""
        # env outputs of the batch: one asynchronous copy each into pinned host buffers (alternating sets, so that
        # the batch waiting to be filed keeps its own), one wait
        pinned = self.next_set()
        for k in ENV_OUTPUTS:
            pinned[k][:n_moves].copy_(ring[k][:n_moves], non_blocking=True)
        torch.cuda.current_stream(self.device).synchronize()
        host = {k: pinned[k][:n_moves].numpy() for k in ENV_OUTPUTS}
        self.pending = UnfiledBatch(out=out, host=host, legal=cur["legal"], num_legal=cur["num_legal"])
        return host["obs_next"][n_moves - 1]

    def keep_device_inputs(self, out, b):
        """A collected batch of the device-input form becomes the batch that waits."""
        # (views of the engine's pinned rings, filled move by move while the batch ran: nothing is unpacked here; they
        # stay valid until the batch after the next one is prepared, and flush() files them before that)
        inputs = self.engine.moves_inputs(b.n_moves, copy=False)
        last_to_play = self.envs.to_play.cpu().numpy()
        self._copy_stream.synchronize()                  # (the last move's downloads)
        host = {k: b.pinned[k][:b.n_moves].numpy() for k in b.keys}
        played = None
        if b.opponent:
            # the opponents drew on the device copies of the streams: the host mirrors step over those words (a paired
            # batch: summed over the moves and their slots)
            played = host["played"]
            words = host["words"].view(numpy.uint32)
            self.engine.rng_consumed(words.reshape(-1, words.shape[-1]).sum(axis=0, dtype=numpy.uint64))
        two_players = len(self.config.players) > 1
        to_play = inputs["to_play"]
        to_play_after = (1 - to_play) if two_players else numpy.zeros_like(to_play)
        to_play_next = numpy.concatenate([to_play[1:], last_to_play[None]], axis=0)
        slots = 1
        if b.paired:
            # slot 0 is MuZero's ply, after which the opponent is to move; after an opponent's ply (slots 1, 2) MuZero is
            slots = played.shape[1]
            to_play_after = numpy.stack([to_play_after] + [to_play] * (slots - 1), axis=1)
        self.pending = UnfiledBatch(out=out, host=host, legal=inputs["legal"], num_legal=inputs["num_legal"],
                                    to_play_after=to_play_after, to_play_next=to_play_next, played=played, slots=slots)
        return (played >= 0).sum(axis=(0, 1)) if b.paired else None


class StoreRows:
    """Where DeviceSelfPlay's games go after file_to(): rows in `replay_buffer`'s store, filed on the device
    (include/mzreplay.h mzreplay_filer_*).  Owns the buffer's reference and the described batch that waits to be queued,
    with the ring it points into.  Nothing of a batch is downloaded; a batch's games reach the store, and on_games,
    exactly when HostRows would hand them out: its filing is queued at the start of the next play_moves -- behind the
    batch's last environment kernel, ahead of anything that rewrites the rings -- or in flush(), and its few bytes are
    synchronised right behind the current batch's moves_collect; the new batch is described only then."""

    def __init__(self, replay_buffer, engine, envs, config, outcomes=False):
        self.replay_buffer, self.engine, self.envs, self.config = replay_buffer, engine, envs, config
        # this actor's own: other actors may file into the same store
        self.filer = replay_buffer.attach_filer(envs.E, outcomes=outcomes)
        obs, _, _, to_play = envs.observe()
        self.filer.begin(obs, to_play)
        self.pending = None                     # (MzReplayFileMoves, ring): described, not queued yet (the ring stays alive with it)

    @property
    def lengths(self):
        return self.filer.lengths()                          # (a small download)

    def admit(self, step=False, on_game=None, opponent="self", batched_pass=True):
        """Evaluation games are never saved to a replay buffer, and the device filer takes whole move batches."""
        if not batched_pass:
            raise NotImplementedError("after file_to() a pass must run as one move batch on the device: give "
                                      "moves_per_pass, and a temperature and root_dirichlet_alpha play_moves accepts")
        what = "step()" if step else "on_game" if on_game is not None else "an opponent" if opponent != "self" else None
        if what is not None:
            raise NotImplementedError(f"{what} is not available after file_to(): the games are filed on the device from "
                                      "whole move batches (play_moves with on_games)")

    def per_game(self, on_game):
        return None                             # the games are in the store: none is rebuilt on the host

    def counters(self):
        return self.replay_buffer.num_played_games, self.replay_buffer.num_played_steps

    def searched_moves(self, moves_played):
        return moves_played                     # self-play only: every ply was searched

    def ring_resized(self, ring):
        pass                                    # (an actor that files on the device downloads none of it: no host sets)

    def next_set(self):
        return None

    def download_move(self, b, m):
        pass                                    # filed on the device: the env outputs stay where they are

    def queue(self):
        if self.pending is not None:
            self.filer.file(self.pending[0])
            self.pending = None

    def flush(self):
        self.queue()
        return self.games_after_collect()

    def games_before_collect(self):
        return None

    def games_after_collect(self):
        """The games of the filing queued last: their lengths and ids join the host bookkeeping (one small sync of every
        filer of the store that has a filing pending; what a sync another actor asked for fetched for this one waits in
        the filer)."""
        filed = FiledGames(*self.filer.take_filed())
        return filed if len(filed) else None

    def keep_predrawn(self, out, ring, n_moves, cur):
        self._describe(n_moves, ring, device_inputs=False)
        return None                             # (the observations stay on the device)

    def keep_device_inputs(self, out, b):
        self._describe(b.n_moves, b.ring, device_inputs=True)

    def _describe(self, n_moves, ring, device_inputs):
        """Describe the batch just collected for the device filer: the search results where the engine left them, the env
        outputs in the actor's ring, the legal sets and players to move from the envs' own arrays (a constant legal set)
        or from the engine's recorded-inputs ring (device-input batches)."""
        eng, envs = self.engine, self.envs
        out = eng.moves_device_ring()
        mv = _native.MzReplayFileMoves()
        mv.n_moves, mv.num_simulations = int(n_moves), int(self.config.num_simulations)
        mv.players = 2 if len(self.config.players) > 1 else 1
        for name in ("actions", "visits", "root_value_sum"):
            setattr(mv, name, out[name])
            setattr(mv, name + "_stride", out["stride"])
        if device_inputs:
            inputs = eng.moves_inputs_device_ring()
            for name in ("legal", "num_legal", "to_play"):
                setattr(mv, name, inputs[name])
                setattr(mv, name + "_stride", inputs["stride"])
            mv.to_play_last = envs.to_play.data_ptr()
        else:
            mv.legal, mv.num_legal, mv.legal_stride, mv.num_legal_stride = envs.legal.data_ptr(), envs.num_legal.data_ptr(), 0, 0
            mv.to_play, mv.to_play_stride, mv.to_play_last = None, 0, None
        mv.rewards, mv.done = ring["reward"].data_ptr(), ring["done"].data_ptr()
        mv.obs_after, mv.obs_next = ring["obs_after"].data_ptr(), ring["obs_next"].data_ptr()
        self.pending = (mv, ring)


def _device_store(replay_buffer):
    """file_to()'s sink is the device store of a replay_buffer.ReplayBuffer: nothing else can be filed into."""
    from .replay_buffer import ReplayBuffer
    if not isinstance(replay_buffer, ReplayBuffer):
        raise NotImplementedError(f"file_to() files into the device store of a replay_buffer.ReplayBuffer; a "
                                  f"{type(replay_buffer).__name__} is not one (hand other sinks the games through on_games)")


class DeviceSelfPlay(ManyEnvLoop):
    """Self-play with device-resident environments (games.device.DeviceEnvs): search, env step and
    observation all stay on the GPU; per move the host only draws the exploration noise, samples the
    actions (both on the per-env numpy-compatible RNG streams) and files the move into packed per-env
    history rows.

    Env e plays the game the host plugin `Game(seed + e)` would play with reference worker `seed + e`'s RNG
    stream -- the same games `BatchedSelfPlay` produces with host envs (tests/test_gpu_envs.py) -- without
    E Python `game.step` calls per move.  Finished games leave as one `PackedGames` batch per move through
    `on_games(batch)`; `on_game(env_index, GameHistory)` is the per-game compatibility callback (it rebuilds
    Python lists, which costs more than the search itself at thousands of envs)."""

    def __init__(self, initial_checkpoint, game_name, config, seed, num_envs, device=None, use_graph=True):
        from .games.device import DeviceEnvs, DeviceFrameStack
        self._build_search(initial_checkpoint, config, seed, num_envs, device, use_graph)
        E = self.E
        self.envs = DeviceEnvs(game_name, E, seeds=[seed + e for e in range(E)], device=self.device)
        assert self.envs.A == len(config.action_space) and self.envs.observation_shape == tuple(config.observation_shape)
        self.moves_played = 0
        self.games_finished = 0
        self._cur = self._observe_host()
        self._row_moves = int(config.max_moves)  # moves a running game's row holds, whoever owns the rows
        # where the games are filed: HostRows, until file_to() swaps StoreRows in; the rows of the running games, the
        # batch waiting to be filed and everything on the way there live in the owner and nowhere else
        self._rows = HostRows(self.engine, self.envs, config, self.device, self._cur)
        self._step_is_batch = False             # step_begin queued the whole move as a one-move batch (an opponent's turn)
        self._batch_ready = None                # (n_moves, temperature) of the batch drawn and uploaded ahead (play_moves)
        self._dev_batch = None                  # DeviceBatch being queued
        self._ring = None                       # env outputs of a batch on the device, sized by the first batch (_move_ring)
        self._paired_ring = None                # ... of a paired batch: the ply outputs carry a slot axis (_move_ring)
        self._paired_on = False                 # the envs are in paired mode: MuZero is to move in every env
        self._settle = None                     # the settle launch's outputs (paired mode taken up: _settle_paired)
        # config.stacked_observations = n > 0: the n previous frames of every env live in a device frame stack
        # (include/mzenv.h mzenv_stack_*).  The plain observations stay what is filed and stored everywhere; only what
        # the searches read changes: `_stacked`, which every move's push rewrites on the actor's stream.  n = 0: no
        # stack, no launch, today's code.
        self._stack = self._stacked = self._stack_ring = None
        if int(config.stacked_observations) > 0:
            self._stack = DeviceFrameStack(E, self.envs.observation_shape, int(config.stacked_observations), self.device)
            self._step_stacked = self._stack.new_output()    # step()'s search input (a batch's lie in _stack_ring)
            self._stacked = self._stack.reset(self._cur["obs_dev"], self._step_stacked)
            # step(): the frame a move is played from (the observe after the move rewrites the envs' own buffer),
            # and the done mask of a move that ends no game
            self._plain_before = torch.zeros_like(self._cur["obs_dev"])
            self._no_done = torch.zeros(E, dtype=torch.uint8, device=self.device)
            torch.cuda.current_stream(self.device).synchronize()    # (a pipelined actor moves to a stream of its own)

    def stacked_observation(self):
        """What the next search reads: the device tensor [E, C + n (C + 1), H, W] of every env's
        GameHistory.get_stacked_observations(-1, n) (n = config.stacked_observations); the plain observation [E, C, H, W]
        when n = 0.  Valid until the next move is queued."""
        return self._cur["obs_dev"] if self._stack is None else self._stacked

    def _frame_before(self, obs_in, obs_next_slot):
        """The frame a batch's move is played from, where the push can still read it after the move's env kernel has
        run: a batch that follows a one-move batch starts from the ring slot its own first move rewrites."""
        if self._stack is not None and obs_in.data_ptr() == obs_next_slot.data_ptr():
            return self._plain_before.copy_(obs_in)
        return obs_in

    @property
    def _len(self):
        """Moves played in every env's running game: the host filer's counters, or the device filer's (a small download)."""
        return self._rows.lengths

    def file_to(self, replay_buffer, shared=False, outcomes=False):
        """From now on finished games go into `replay_buffer`'s store on the device (include/mzreplay.h
        mzreplay_filer_file): play_moves queues the filing behind the batch's last environment kernel, no observation,
        policy row or value of a game visits the host, and `on_games` receives a FiledGames (env_index, length, game_id)
        instead of a PackedGames.  Before the first move only, same device only; step(), on_game and opponent modes are
        not available afterwards (evaluation games are never saved to a replay buffer).
        shared=True: the buffer may already receive another actor's games.  The store then numbers games in the order of
        the actors' play_moves / flush calls, and what the first actor's owner sees changes with it -- its ids are no
        longer consecutive, sync_filing() returns None and the buffer's filer_* calls want the filer named -- which is
        why joining a store is asked for and never happens by default.
        outcomes=True: the filer also reports what every finished game earned (total reward, reward per player, the sum
        and count of its non-zero root values: csrc/game_outcomes.h), computed where it finishes the game; take_outcomes()
        hands them out.  The store's contents and ids are the same either way."""
        if isinstance(self._rows, StoreRows):
            raise ValueError("file_to was called before")
        if self.moves_played or self._batch_ready or self._dev_batch is not None or self._rows.pending is not None:
            raise ValueError("file_to comes before the first move: the running games live in the host filer by now")
        _device_store(replay_buffer)
        if replay_buffer.filers and not shared:
            raise NotImplementedError("this replay buffer already receives the games of an actor that called file_to(); "
                                      "sharing a store is not the default: pass file_to(replay_buffer, shared=True) to join "
                                      "it (ids then follow the order of the actors' calls), or use on_games -> save_games")
        store_device = torch.device(replay_buffer.device)
        mine = self.device if self.device.index is not None else torch.device("cuda", torch.cuda.current_device())
        if store_device != mine:
            raise ValueError(f"file_to: the replay buffer lives on {store_device}, the actor on {mine}")
        if (replay_buffer.L != int(self.config.max_moves) or replay_buffer.A != self.envs.A
                or (replay_buffer.C, replay_buffer.H, replay_buffer.W) != tuple(self.envs.observation_shape)):
            raise ValueError("file_to: the replay buffer was built for another game shape or move limit")
        self._rows = StoreRows(replay_buffer, self.engine, self.envs, self.config, outcomes=outcomes)

    def take_outcomes(self):
        """The GameOutcomes of the games handed out (on_games) since the last take, in that order.  Needs
        file_to(replay_buffer, outcomes=True)."""
        if not isinstance(self._rows, StoreRows) or not self._rows.filer.outcomes:
            raise RuntimeError("take_outcomes: the actor reports no outcomes: turn them on when it starts filing on the "
                               "device, file_to(replay_buffer, outcomes=True)")
        return self._rows.filer.take_outcomes()

    def _filed_counters(self):
        return self._rows.counters()

    def _observe_host(self):
        obs, legal, num_legal, to_play = self.envs.observe()
        return dict(obs=obs.cpu().numpy(), legal=legal.cpu().numpy(), num_legal=num_legal.cpu().numpy(),
                    to_play=to_play.cpu().numpy(), obs_dev=obs)

    def _current(self):
        """The envs' current positions on the host (what step() searches).  A device-input move batch leaves them on the
        device only: they are fetched when a step() next asks, not once per batch."""
        if self._cur.get("on_device_only"):
            self._cur = self._observe_host()
        return self._cur

    def set_weights(self, weights):
        self.model.set_weights(weights)

    def set_device_temperatures(self, enabled=True):
        """Move batches at any softmax temperature (engine.set_device_temperatures): play_moves, a step against an
        opponent, continuous_self_play(moves_per_pass=K) and evaluate() then run a config whose temperature is not 0,
        inf or 1 / k as batches too, the actions sampled on the GPU -- the games step() plays, bit for bit.  Off by
        default: such a config plays through step(), one host round trip per move."""
        self.engine.set_device_temperatures(enabled)

    def _device_samples(self, temperature):
        """Can a move batch sample at `temperature` (engine.moves_prepare* would accept it)?"""
        if temperature == 0 or _native.exact_inverse_temperature(temperature):
            return True
        # (1 / k whose powers leave the exact integers is refused by the engine unless the switch is on; not asked here)
        return bool(self.engine._device_temperatures) and 0.0 < float(temperature) < float("inf")

    def step(self, temperature, temperature_threshold=None, on_game=None, on_games=None, opponent=None,
             muzero_player=None):
        """One move in every env (the body of play_game's loop, self_play.py:129-182).  `opponent` / `muzero_player` as
        in BatchedSelfPlay.step (default: what set_opponent stored, else "self"): where it is not MuZero's turn the
        environment kernels play the opponent's move, drawn on that env's stream, and the ply is filed without search
        statistics.  Such a step is a one-move device-input batch (the opponent draws on the device copy of the stream,
        which a host-sampled step leaves behind its mirror)."""
        self.step_begin(on_game, on_games, opponent, muzero_player, temperature, temperature_threshold)
        self.step_end(temperature, temperature_threshold, on_game, on_games)

    def _set_env_mode(self, mode):
        """Before anything is queued: the envs end games at config.max_moves where that is shorter than the game itself
        (the environment kernels count the plies; read here because callers edit the config of a built actor), and
        switch between self-play and an opponent; the positions stay, the legal counts the searches read are observed
        again in the new mode."""
        limit = int(self.config.max_moves)
        if limit > self._row_moves:
            raise ValueError(f"config.max_moves was raised to {limit} on a built actor whose history rows hold "
                             f"{self._row_moves} moves; build a new actor")
        limit = limit if limit < self.envs.max_episode_steps else 0
        if self.envs.max_moves != limit:
            self.envs.set_max_moves(limit)
        paired_before, self._paired_on = self._paired_on, mode[2]
        if self.envs.opponent == mode[:2]:
            return mode[2] and not paired_before
        self.envs.set_opponent(mode[0], mode[1], self.engine)
        obs, _, _, _ = self.envs.observe()
        self._cur = dict(obs_dev=obs, on_device_only=True)
        return mode[2]      # paired mode taken up: the opponent's pending plies come first (_settle_paired)

    def _paired_check(self, temperature_threshold):
        """What a paired batch leaves out of scope: say which condition rules it out."""
        if temperature_threshold:
            raise NotImplementedError("paired mode with a non-zero temperature_threshold: the engine's per-game ply counter "
                                      "does not see the opponent's replies; play the sit-out mode (paired=False)")
        if self._stack is not None:
            raise NotImplementedError("paired mode with stacked_observations > 0: the frame stack pushes one ply per move; "
                                      "play the sit-out mode (paired=False)")

    def _settle_paired(self, on_game, on_games):
        """Paired mode was taken up (or the side MuZero plays changed): one advance_paired launch with no action plays the
        opponent's pending plies -- its openings after a reset when MuZero plays second -- so that MuZero is to move in
        every env.  The plies are filed like any other; returns (the observation the first search reads, plies per env)."""
        envs = self.envs
        if self._settle is None:
            self._settle = dict(envs.new_paired_outputs(), obs_next=torch.zeros_like(envs.obs),
                                actions=torch.full((self.E,), -1, dtype=torch.int32, device=self.device))
        st = self._settle
        envs.advance_paired(st["actions"], st["reward"], st["done"], st["obs_after"], st["obs_next"], st["played"], st["words"])
        host = {k: st[k].cpu().numpy() for k in ("reward", "done", "obs_after", "played", "words")}
        self._hand_out(self._rows.file_settled(host), on_game, on_games)
        plies = (host["played"] >= 0).sum(axis=0)
        self.moves_played += int(plies.sum())
        return st["obs_next"], plies

    def _opponent_step_check(self, temperature):
        """An opponent's plies exist in the device-input form of a move batch only: say what rules it out."""
        cfg = self.config
        if not 0.0 < float(cfg.root_dirichlet_alpha) <= 1.0:
            raise NotImplementedError("a step against an opponent runs as a device-input move batch, whose exploration "
                                      "noise is drawn on the GPU for 0 < root_dirichlet_alpha <= 1 only")
        if not (temperature == float("inf") or self._device_samples(temperature)):
            raise NotImplementedError("a step against an opponent runs as a device-input move batch, whose actions are "
                                      f"sampled on the GPU at temperature 0, inf or 1/k (k = 1..4) only; got {temperature}")

    def step_begin(self, on_game=None, on_games=None, opponent=None, muzero_player=None, temperature=None,
                   temperature_threshold=None):
        """First half of step(): queue the search of every env's current position on the engine's stream and return
        (the GPU works; `step_end` waits).  Two actors on streams of their own alternate their halves
        (PipelinedDeviceSelfPlay): one's host work runs under the other's search.  Against an opponent the whole move
        is queued here (search, action sampling, env step: a one-move batch), so the temperature is needed already."""
        self._rows.admit(step=True)
        mode = self._resolve_opponent(opponent, muzero_player)
        if mode[2]:
            raise NotImplementedError("step() in paired mode: a paired move exists as a move batch only; "
                                      "use play_moves(1, ...)")
        if mode[0] != "self":
            if temperature is None:
                raise ValueError("step_begin against an opponent samples the action on the device: pass temperature")
            self._opponent_step_check(temperature)
            self._device_batch_begin(1, temperature, on_game, on_games, temperature_threshold or 0, *mode)
            self._device_batch_move(0)
            self._step_is_batch = True
            return
        self.flush(on_game, on_games)      # first: the unfiled batch holds views of the download ring
        self._drop_batch()
        self._set_env_mode(mode)
        cur = self._current()
        search_input = cur["obs_dev"]
        if self._stack is not None:
            search_input = self._stacked
            self._plain_before.copy_(cur["obs_dev"])         # the frame step_end pushes
        if self.engine._fc_model is not None:
            self.engine.search_fused_begin(search_input.reshape(self.E, -1), cur["legal"], cur["to_play"], True,
                                           num_legal=cur["num_legal"])
        else:
            self.engine.search_begin(self.model, search_input, cur["legal"], cur["to_play"], True,
                                     num_legal=cur["num_legal"])

    def step_end(self, temperature, temperature_threshold=None, on_game=None, on_games=None):
        """Second half of step(): wait for the search, sample the actions, step the envs, file the move."""
        if self._step_is_batch:                          # against an opponent: step_begin queued the whole move
            self._step_is_batch = False
            self._device_batch_end(on_game, on_games)
            self.flush(on_game, on_games)
            return
        cur = self._cur
        self.engine.readout()
        if temperature_threshold:
            # play_game: temperature only while len(action_history) < threshold (self_play.py:163-170)
            temps = numpy.where(self._len + 1 < temperature_threshold, float(temperature), 0.0)
        else:
            temps = numpy.full(self.E, float(temperature))
        actions, _ = self.engine.sample_actions(numpy.ascontiguousarray(temps, dtype=numpy.float64))
        stats = self.engine.stats
        played = actions
        if self._stack is not None:                          # (the push reads the actions on the device as well)
            played = torch.from_numpy(numpy.ascontiguousarray(actions, dtype=numpy.int32)).to(self.device)
        reward, done = self.envs.step(played)
        after = self._observe_host()
        reward, done = reward.cpu().numpy(), done.cpu().numpy().astype(bool)
        over = done | (self._len + 2 > self.config.max_moves)   # len(action_history) > max_moves ends the game
        nxt = after
        over_dev = None
        if over.any():
            over_dev = torch.from_numpy(over.astype(numpy.uint8)).to(self.device)
            self.envs.reset(over_dev)
            nxt = self._observe_host()
        if self._stack is not None:
            # the games that are over -- by their rules or by play_game's move limit -- forget their frames; queued
            # here, ahead of the next step_begin on this stream
            self._stacked = self._stack.push(self._plain_before, played, self._no_done if over_dev is None else over_dev,
                                             nxt["obs_dev"], self._step_stacked)
        # child visits by action and root values as store_search_statistics computes them (self_play.py:497-512)
        one = {"actions": actions.astype(numpy.int32)[None], "visits": stats["visits"][None],
               "root_value_sum": stats["root_value_sum"][None], "moves_done": numpy.ones(self.E, dtype=numpy.int32)}
        self._hand_out(self._rows.file_move(one, cur["legal"], cur["num_legal"], reward, over, after, nxt), on_game, on_games)
        self._cur = nxt
        self.moves_played += self.E

    def _hand_out(self, batch, on_game, on_games):
        """The games a filing finished (PackedGames, FiledGames or None) leave: counted, then as one batch, then one by one."""
        if batch is None:
            return
        self.games_finished += len(batch)
        if on_games is not None:
            on_games(batch)
        if on_game is not None:
            for i, e in enumerate(batch.env_index):
                on_game(int(e), batch.history(i))

    # ---- whole batches of moves on the device (engine.moves_*, include/mzmcts.h) ---------------------------
    def play_moves(self, n_moves, temperature, on_game=None, on_games=None, temperature_threshold=None, opponent=None,
                   muzero_player=None, paired=None):
        """`n_moves` moves of every env with no host round trip in between: search (which samples the action),
        env step, terminal observation, reset of finished envs, next observation -- all queued on one stream.
        Fully-connected networks search in the fused whole-move kernel (games with a constant legal set: the exploration
        noise of the whole batch is drawn up front, and the next batch's while this one runs); residual networks search
        lock-step (engine.moves_enqueue_lockstep) with inputs, noise and action sampling on the device.
        `temperature_threshold` (default config.temperature_threshold) is play_game's rule, applied per env and move.
        An env may come back with fewer than n_moves moves played (it plays the rest next time).
        Games end where play_game ends them: by the game's rules or at config.max_moves plies, whichever comes first --
        the environment kernels apply both (DeviceEnvs.set_max_moves), so a limit costs a batch nothing.
        `opponent` / `muzero_player` as in step(): an opponent's plies are played by the environment kernels inside the
        batch (always its device-input form; every env then plays all n_moves plies).  `paired` (default: what
        set_opponent stored): the opponent replies inside MuZero's move, so every env is searched in every move and
        plays up to three plies per move; the return value then counts plies per env."""
        E, eng, envs, cfg = self.E, self.engine, self.envs, self.config
        mode = self._resolve_opponent(opponent, muzero_player, paired)
        self._rows.admit(on_game=on_game, opponent=mode[0])
        self._rows.queue()                                   # (store rows) the batch before: ahead of anything this one rewrites
        # Everything but a fused search of a game with a constant legal set takes the device-input form of the batch:
        # board games (legal sets change), residual networks (lock-step searches), and a temperature threshold
        # (play_game drops to temperature 0 once len(action_history) reaches it, self_play.py:152-158: a per-env, per-move
        # switch the kernels make from per-game move counters they keep on the device)
        if temperature_threshold is None:
            temperature_threshold = cfg.temperature_threshold
        if (not getattr(envs, "constant_legal_actions", False) or eng._fc_model is None or temperature_threshold
                or mode[0] != "self"):
            return self._play_moves_device_inputs(n_moves, temperature, on_game, on_games, temperature_threshold, *mode)
        self._set_env_mode(mode)
        cur = self._current()
        params = (int(n_moves), float(temperature))
        if self._batch_ready != params:
            self.flush(on_game, on_games)                    # (the unfiled batch holds views of the download ring)
            self._drop_batch()
            eng.moves_prepare(n_moves, cur["legal"], cur["to_play"], temperature, True, num_legal=cur["num_legal"])
        ring = self._move_ring(n_moves)
        obs_in = cur["obs_dev"]
        for m in range(n_moves):
            eng.moves_enqueue((obs_in if self._stack is None else self._stacked).reshape(E, -1))
            obs_in = self._frame_before(obs_in, ring["obs_next"][m])
            # step, terminal observation, reset of the finished envs, next observation: one call, one launch
            obs_next = envs.advance(eng.moves_actions(m), ring["reward"][m], ring["done"][m], ring["obs_after"][m],
                                    ring["obs_next"][m])
            if self._stack is not None:
                # (a stalled env's action reads -1: the env kernels left it alone and nothing is pushed)
                self._stacked = self._stack.push(obs_in, eng.moves_actions(m), ring["done"][m], obs_next,
                                                 self._stack_ring[m])
            obs_in = obs_next
        # host rows: the previous batch's games, while this one runs
        self._hand_out(self._rows.games_before_collect(), on_game, on_games)
        eng.moves_predraw_next(n_moves, cur["legal"], cur["to_play"], temperature, True, num_legal=cur["num_legal"])
        out = eng.moves_collect(copy=False)                  # views: kept by the rows, filed before the next collect
        # store rows: the batch before's games, filed ahead of this batch (collect() has waited for it: the RNG mirrors
        # need the engine's own ring); the filing's few bytes come back right behind it
        self._hand_out(self._rows.games_after_collect(), on_game, on_games)
        obs = self._rows.keep_predrawn(out, ring, n_moves, cur)
        eng.moves_submit_next()
        self._batch_ready = params
        self._cur = dict(cur, obs_dev=obs_in, obs=obs)
        self.moves_played += int(out["moves_done"].sum())
        return out["moves_done"].copy()

    def _play_moves_device_inputs(self, n_moves, temperature, on_game, on_games, temperature_threshold=None,
                                  opponent=None, muzero_player=None, paired=None):
        """play_moves with the batch's inputs on the device: the searches read the legal sets and players to move from the
        environment kernels' device outputs and draw their exploration noise on the device (engine.moves_prepare_device),
        so a whole batch -- games ending and restarting inside it -- is queued without the host; afterwards every move
        is filed with the legal set it was searched with.  The search of a move is the fused whole-move kernel
        (fully-connected networks) or the lock-step loop with this actor's network (residual networks)."""
        self._device_batch_begin(n_moves, temperature, on_game, on_games, temperature_threshold, opponent, muzero_player,
                                 paired)
        for m in range(n_moves):
            self._device_batch_move(m)
        return self._device_batch_end(on_game, on_games)

    # (the three phases are separate so that PipelinedDeviceSelfPlay can interleave the batches of its groups move by move)
    def _device_batch_begin(self, n_moves, temperature, on_game, on_games, temperature_threshold, opponent=None,
                            muzero_player=None, paired=None):
        eng, envs = self.engine, self.envs
        mode = self._resolve_opponent(opponent, muzero_player, paired)
        paired = mode[2]
        if paired:
            self._paired_check(temperature_threshold)
        if self._batch_ready or temperature_threshold:
            # a batch of the pre-drawn form is waiting to be filed / the threshold rule needs the games' current lengths
            self.flush(on_game, on_games)
        self._drop_batch()
        settled = None
        if self._set_env_mode(mode):
            self.flush(on_game, on_games)                    # (the settle launch's plies are filed behind all played so far)
            obs, settled = self._settle_paired(on_game, on_games)
            self._cur = dict(obs_dev=obs, on_device_only=True)
        eng.moves_prepare_device(n_moves, envs.legal, envs.num_legal, envs.to_play, temperature, True)
        if mode[0] != "self" and not paired:
            eng.moves_sit_out(True)        # the opponent's plies: played by the environment kernels, filed from `played`
        if temperature_threshold:
            eng.moves_temperature_threshold(temperature_threshold, self._len)
        ring = self._move_ring(n_moves, paired)
        self._dev_batch = DeviceBatch(n_moves=n_moves, ring=ring, obs_in=self._cur["obs_dev"], threshold=temperature_threshold,
                                      pinned=self._rows.next_set(paired) if paired else self._rows.next_set(),
                                      opponent=mode[0] != "self", paired=paired, settled=settled)

    def _device_batch_move(self, m):
        b, eng, envs = self._dev_batch, self.engine, self.envs
        ring = b.ring
        if b.threshold and m > 0:
            eng.moves_finished(ring["done"][m - 1])          # games that ended with the move before restart their count
        search_input = b.obs_in if self._stack is None else self._stacked
        if eng._fc_model is not None:
            eng.moves_enqueue(search_input.reshape(self.E, -1).contiguous())
        else:
            eng.moves_enqueue_lockstep(self.model, search_input)
        b.obs_in = self._frame_before(b.obs_in, ring["obs_next"][m])
        if b.paired:
            # MuZero's ply and the opponent's reply (and what follows a game's end) in one launch: MuZero is to move again
            obs_next = envs.advance_paired(eng.moves_actions(m), ring["reward"][m], ring["done"][m], ring["obs_after"][m],
                                           ring["obs_next"][m], ring["played"][m], ring["words"][m])
        else:
            obs_next = envs.advance(eng.moves_actions(m), ring["reward"][m], ring["done"][m], ring["obs_after"][m],
                                    ring["obs_next"][m], played=ring["played"][m] if b.opponent else None,
                                    words=ring["words"][m] if b.opponent else None)
        if self._stack is not None:
            # an opponent's ply is a ply of the game: the action the env kernels played, not the search's (-1 there:
            # a full board on the opponent's turn leaves the env alone)
            self._stacked = self._stack.push(b.obs_in, ring["played"][m] if b.opponent else eng.moves_actions(m),
                                             ring["done"][m], obs_next, self._stack_ring[m])
        b.obs_in = obs_next
        self._rows.download_move(b, m)

    def _device_batch_end(self, on_game, on_games):
        b, self._dev_batch = self._dev_batch, None
        # host rows: the previous batch's games, while this one runs
        self._hand_out(self._rows.games_before_collect(), on_game, on_games)
        out = self.engine.moves_collect(copy=False)
        # store rows: the batch before's games (filed ahead of this batch)
        self._hand_out(self._rows.games_after_collect(), on_game, on_games)
        plies = self._rows.keep_device_inputs(out, b)
        # the envs' current positions stay on the device: the next batch starts from the last move's observation (the
        # kernels' output, where it lies); a step() fetches what it needs first (_current)
        self._cur = dict(obs_dev=b.obs_in, on_device_only=True)
        if plies is None:
            self.moves_played += int(out["moves_done"].sum())
            return out["moves_done"].copy()
        # a paired batch: every env was searched in every move and played up to three plies per move (the plies of a
        # settle launch in front of the batch were counted there and are reported with it)
        self.moves_played += int(plies.sum())
        return (plies if b.settled is None else plies + b.settled).astype(out["moves_done"].dtype)

    def _batchable(self, temperature, temperature_threshold, moves_per_pass, device_inputs=None):
        """Can a pass of `moves_per_pass` moves run as one move batch on the device (play_moves)?"""
        if device_inputs is None:
            device_inputs = (not getattr(self.envs, "constant_legal_actions", False) or self.engine._fc_model is None
                             or bool(temperature_threshold) or self._opponent[0] != "self")
        return (moves_per_pass is not None
                and self._device_samples(temperature)
                # (a device-input batch draws its exploration noise on the GPU: the legacy gamma sampler for shapes <= 1)
                and (not device_inputs or 0.0 < float(self.config.root_dirichlet_alpha) <= 1.0))

    def _play_pass(self, temperature, temperature_threshold, moves_per_pass):
        """ManyEnvLoop's pass: whole move batches on the device when the game, the network and the temperature allow
        it (play_moves), else one move at a time (step)."""
        if not self._batchable(temperature, temperature_threshold, moves_per_pass):
            self._rows.admit(batched_pass=False)
            return ManyEnvLoop._play_pass(self, temperature, temperature_threshold, moves_per_pass)
        finished = []
        collect = self._rows.per_game(lambda e, gh: finished.append((e, gh)))
        self.play_moves(moves_per_pass, temperature, on_game=collect, temperature_threshold=temperature_threshold or 0)
        self.flush(on_game=collect)
        return finished

    def flush(self, on_game=None, on_games=None):
        """File the moves of the last play_moves batch into the histories (play_moves does this for the
        batch before while the GPU runs the current one; call it once at the end).  Host rows: native code
        (HistoryFiler, include/mzhist.h), one pass over the batch on the library's worker pool.  Store rows: the filing
        is queued and its games' lengths and ids join the host bookkeeping (one small sync per batch)."""
        self._rows.admit(on_game=on_game)
        self._hand_out(self._rows.flush(), on_game, on_games)

    @property
    def searched_moves(self):
        """Env-moves filed so far that ran a search (moves_played counts the opponent's plies too)."""
        return self._rows.searched_moves(self.moves_played)

    def _drop_batch(self):
        """Forget the batch that was drawn and uploaded ahead (its noise goes back into the RNG streams)."""
        if self._batch_ready:
            self.engine.moves_collect()
            self._batch_ready = None

    def _move_ring(self, n_moves, paired=False):
        if paired:
            # the same ring with a slot axis on what a ply produces; the sit-out ring keeps its shape
            ring = self._paired_ring
            if ring is None or ring["reward"].shape[0] < n_moves:
                ring = dict(self.envs.new_paired_outputs(n_moves),
                            obs_next=torch.zeros((n_moves, self.E) + self.envs.observation_shape, dtype=torch.float32,
                                                 device=self.device))
                self._rows.ring_resized(ring, paired=True)
                self._paired_ring = ring
            return ring
        ring = self._ring
        if ring is None or ring["reward"].shape[0] < n_moves:
            shape, dev = self.envs.observation_shape, self.device
            ring = dict(reward=torch.zeros((n_moves, self.E), dtype=torch.float32, device=dev),
                        done=torch.zeros((n_moves, self.E), dtype=torch.uint8, device=dev),
                        obs_after=torch.zeros((n_moves, self.E) + shape, dtype=torch.float32, device=dev),
                        obs_next=torch.zeros((n_moves, self.E) + shape, dtype=torch.float32, device=dev),
                        # evaluation games: the actions the environment kernels played, the stream words (u32 bits) the
                        # opponents consumed
                        played=torch.zeros((n_moves, self.E), dtype=torch.int32, device=dev),
                        words=torch.zeros((n_moves, self.E), dtype=torch.int32, device=dev))
            self._rows.ring_resized(ring)                    # (host rows: their host sets are sized with it)
            self._ring = ring
            if self._stack is not None:
                # every move's stacked search input, kept like its obs_next: the engine holds the tensors it was handed
                # until the batch is collected (never downloaded, so not part of `ring`, which sizes the host sets; an
                # earlier ring that `_stacked` still views stays alive through that reference)
                self._stack_ring = self._stack.new_output(n_moves)
        return ring

    def close(self):
        if self._stack is not None:
            self._stack.close()
        self.envs.close()
        self.engine.close()


class PipelinedDeviceSelfPlay(ManyEnvLoop):
    """`groups` DeviceSelfPlay actors of num_envs / groups envs each, on HIP streams of their own, alternating the halves
    of a move (step_begin / step_end): while the host samples, steps, observes and files one group's move, the GPU
    searches the other group's positions.  Env e keeps seed `seed + e`, so the groups together play the games one
    DeviceSelfPlay of num_envs envs plays (tests/test_gpu_envs.py).  Callbacks see global env indices.  Carries the
    reference's continuous_self_play loop (ManyEnvLoop): a weight pull reaches every group's network replica.
    file_to(replay_buffer) files every group's games into one store on the device, ids in the host path's order."""

    def __init__(self, initial_checkpoint, game_name, config, seed, num_envs, groups=2, device=None, use_graph=True):
        assert num_envs % groups == 0
        self.config = config
        self.groups, self.per_group, self.E = groups, num_envs // groups, num_envs
        self.actors, self.streams = [], []
        for g in range(groups):
            actor = DeviceSelfPlay(initial_checkpoint, game_name, config, seed + g * self.per_group, self.per_group,
                                   device=device, use_graph=use_graph)
            stream = torch.cuda.Stream(device=actor.device)
            actor.engine.stream = stream
            self.actors.append(actor)
            self.streams.append(stream)
        self._started = [False] * groups         # group g's next search is queued (step)
        self._batch_queued = [False] * groups    # group g's next move batch is queued (play_moves)
        self._filing = False                     # file_to(): every group files into one store on the device
        self.device, self.model = self.actors[0].device, self.actors[0].model   # (what ManyEnvLoop's weight pull addresses)

    def file_to(self, replay_buffer, shared=False, outcomes=False):
        """DeviceSelfPlay.file_to for every group: each group's actor files into the one store through a filer of its own,
        on the group's stream (shared=True: the store may already receive another actor's games).  The store numbers games in the order the filings are queued, whatever the streams do
        (include/mzreplay.h), and play_moves queues them in the order the host path hands the games out: per batch, group
        0, then group 1, and so on -- with and without prefetch.  `on_games` receives a FiledGames per group with global
        env indices.  What StoreRows.admit refuses holds for every group: no step(), no on_game, no opponent."""
        _device_store(replay_buffer)
        if self._filing:
            raise ValueError("file_to was called before")
        if any(self._started) or any(self._batch_queued):
            raise ValueError("file_to comes before the first move")
        for g, (actor, stream) in enumerate(zip(self.actors, self.streams)):
            with torch.cuda.stream(stream):
                # (the groups share the store among themselves)
                actor.file_to(replay_buffer, shared=shared or g > 0, outcomes=outcomes)
        self._filing = True

    def take_outcomes(self):
        """DeviceSelfPlay.take_outcomes of every group as one GameOutcomes with global env indices, merged by ascending
        game_id (the order the store numbered the games in, which is the order on_games saw them)."""
        if not self._filing:
            raise RuntimeError("take_outcomes: the actor reports no outcomes: turn them on when it starts filing on the "
                               "device, file_to(replay_buffer, outcomes=True)")
        parts = []
        for g, actor in enumerate(self.actors):
            part = actor.take_outcomes()
            # (built anew: a NamedTuple whose len() counts games cannot _replace)
            parts.append(GameOutcomes(part.env_index + numpy.int32(g * self.per_group), *part[1:]))
        merged = GameOutcomes.concatenate(parts)
        order = numpy.argsort(merged.game_id, kind="stable")
        return GameOutcomes(*(column[order] for column in merged))

    def _filed_counters(self):
        return self.actors[0]._filed_counters() if self._filing else None    # (one store: every group's rows count it)

    def _pull_weights(self, shared_storage, version):
        self._no_batch_queued("weight pull")
        ManyEnvLoop._pull_weights(self, shared_storage, version)     # group 0's model (all ranks: one flat broadcast)
        # the replicas take the parameters AND rebuild what they cache from them (folded batch norms, packed tower
        # weights): a replayed hipGraph reads those buffers without coming back to Python
        state = self.model.state_dict()
        current = torch.cuda.current_stream(self.device)
        for actor, stream in zip(self.actors[1:], self.streams[1:]):
            stream.wait_stream(current)
            with torch.cuda.stream(stream):
                actor.model.set_weights(state)

    def stacked_observation(self):
        """DeviceSelfPlay.stacked_observation of all groups, env-major (a copy, once every group's stream has run)."""
        for stream in self.streams:
            stream.synchronize()
        return torch.cat([a.stacked_observation() for a in self.actors])

    def set_device_temperatures(self, enabled=True):
        """DeviceSelfPlay.set_device_temperatures for every group's engine."""
        for a in self.actors:
            a.set_device_temperatures(enabled)

    @property
    def moves_played(self):
        return sum(a.moves_played for a in self.actors)

    @property
    def games_finished(self):
        return sum(a.games_finished for a in self.actors)

    @property
    def searched_moves(self):
        return sum(a.searched_moves for a in self.actors)

    def set_weights(self, weights):
        self._no_batch_queued("set_weights")
        for a in self.actors:
            a.set_weights(weights)

    def flush(self, on_game=None, on_games=None):
        for g, actor in enumerate(self.actors):
            one, many = self._callbacks(g, on_game, on_games)
            actor.flush(one, many)

    def _callbacks(self, g, on_game, on_games):
        base = g * self.per_group
        one = None if on_game is None else (lambda e, gh: on_game(base + e, gh))

        def many(batch):
            if isinstance(batch, FiledGames):                # (after file_to(): a tuple of host arrays)
                batch = FiledGames(batch.env_index + base, batch.length, batch.game_id)
            else:
                batch.env_index = batch.env_index + base
            on_games(batch)
        return one, (None if on_games is None else many)

    def step(self, temperature, temperature_threshold=None, on_game=None, on_games=None, prefetch=True, opponent=None,
             muzero_player=None):
        """One move in every env of every group (each group's search was queued during the previous call).
        prefetch=False leaves no search queued behind (the next call then starts them): what a caller wants before it
        changes the weights, so that no move is searched with the weights of the move before.
        Against an opponent (`opponent` / `muzero_player` as in DeviceSelfPlay.step) the move is a one-move batch of every
        group, queued on the groups' streams in turn; nothing is prefetched."""
        self._no_batch_queued("step")
        mode = self._resolve_opponent(opponent, muzero_player)
        if mode[2]:
            raise NotImplementedError("step() in paired mode: a paired move exists as a move batch only; "
                                      "use play_moves(1, ...)")
        if mode[0] != "self":
            if any(self._started):
                raise RuntimeError("step against an opponent: a search is queued ahead; call step(..., prefetch=False) first")
            for actor in self.actors:
                actor._opponent_step_check(temperature)
            self.play_moves(1, temperature, on_game, on_games, temperature_threshold or 0, opponent=mode[0],
                            muzero_player=mode[1])
            self.flush(on_game, on_games)
            return
        for g, actor in enumerate(self.actors):
            if not self._started[g]:
                with torch.cuda.stream(self.streams[g]):
                    actor.step_begin(*self._callbacks(g, on_game, on_games), *mode[:2])
                self._started[g] = True
        for g, actor in enumerate(self.actors):
            one, many = self._callbacks(g, on_game, on_games)
            with torch.cuda.stream(self.streams[g]):
                actor.step_end(temperature, temperature_threshold, one, many)
                self._started[g] = False
                if prefetch:
                    actor.step_begin(one, many, *mode[:2])   # the next move's search runs while the other groups are served
                    self._started[g] = True

    def play_moves(self, n_moves, temperature, on_game=None, on_games=None, temperature_threshold=None, prefetch=False,
                   opponent=None, muzero_player=None, paired=None):
        """`n_moves` moves of every env of every group with no host round trip (DeviceSelfPlay.play_moves in its
        device-input form): each group's batch is queued on the group's own stream, move by move in turn, so the
        kernels of the groups fill each other's gaps (a tower workgroup's fill / epilogue / export phases leave the matrix
        pipe idle).  Returns moves played per env.

        prefetch=True queues each group's NEXT batch (same parameters) as soon as its current one is collected, before
        anything is filed: collecting, filing and the callbacks of one group then run under the other group's kernels
        and the GPU never drains between calls -- the batch form of step()'s prefetch, with the same contract: the batch a
        call returns was queued by the call before (with that call's parameters and the weights of that time), and
        the last call before the weights change passes prefetch=False.
        `opponent` / `muzero_player` as in DeviceSelfPlay.play_moves (a prefetched batch plays what its call asked for)."""
        mode = self._resolve_opponent(opponent, muzero_player, paired)      # (the groups are told: they keep none of their own)
        if temperature_threshold is None:
            temperature_threshold = self.config.temperature_threshold
        queued = self._batch_queued
        fresh = [g for g in range(self.groups) if not queued[g]]
        for g in fresh:
            actor = self.actors[g]
            if self._started[g]:                             # (a search queued by step(): finish that move first)
                raise RuntimeError("play_moves: a step() is half done; call step(..., prefetch=False) before batches")
            one, many = self._callbacks(g, on_game, on_games)
            with torch.cuda.stream(self.streams[g]):
                self._queue_filing(actor, one, mode)
                actor._device_batch_begin(n_moves, temperature, one, many, temperature_threshold, *mode)
        for m in range(n_moves):
            for g in fresh:
                with torch.cuda.stream(self.streams[g]):
                    self.actors[g]._device_batch_move(m)
        for g in fresh:
            queued[g] = True
        played = []
        for g, actor in enumerate(self.actors):
            one, many = self._callbacks(g, on_game, on_games)
            with torch.cuda.stream(self.streams[g]):
                played.append(actor._device_batch_end(one, many))
                queued[g] = False
                if prefetch:
                    self._queue_filing(actor, one, mode)
                    actor._device_batch_begin(n_moves, temperature, one, many, temperature_threshold, *mode)
                    for m in range(n_moves):
                        actor._device_batch_move(m)
                    queued[g] = True
                    actor.flush(one, many)                   # the collected batch's games, while the GPU runs the next
        return numpy.concatenate(played)

    @staticmethod
    def _queue_filing(actor, on_game, mode):
        """What DeviceSelfPlay.play_moves does ahead of a batch: after file_to() the group's collected batch is filed on
        its stream, ahead of anything the next batch rewrites -- the groups in turn, so the store's ids follow the order
        the host path hands the games out.  (Host rows: nothing to do.)"""
        actor._rows.admit(on_game=on_game, opponent=mode[0])
        actor._rows.queue()

    def _no_batch_queued(self, what):
        if any(self._batch_queued):
            raise RuntimeError(f"{what}: a move batch is queued ahead; call play_moves(..., prefetch=False) first")

    def _play_pass(self, temperature, temperature_threshold, moves_per_pass):
        """ManyEnvLoop's pass: the groups' move batches on their streams when the pass can run as batches (always in their
        device-input form; nothing stays queued behind the pass: a weight pull follows), else move by move with the
        groups' halves alternating -- the last move of a pass queues nothing behind it either."""
        finished = []
        if self.actors[0]._batchable(temperature, temperature_threshold, moves_per_pass, device_inputs=True):
            # (after file_to() the games are in the store: none is rebuilt on the host)
            collect = None if self._filing else (lambda e, gh: finished.append((e, gh)))
            self.play_moves(moves_per_pass, temperature, on_game=collect, temperature_threshold=temperature_threshold or 0)
            self.flush(on_game=collect)
            return finished
        moves = 0
        while True:
            last = moves_per_pass is None or moves + 1 >= moves_per_pass
            self.step(temperature, temperature_threshold, on_game=lambda e, gh: finished.append((e, gh)), prefetch=not last)
            moves += 1
            if (moves_per_pass is None and finished) or (moves_per_pass is not None and moves >= moves_per_pass):
                return finished

    def close(self):
        torch.cuda.synchronize(self.device)      # (a queued search may still be running)
        for a in self.actors:
            a.close()


def evaluate(checkpoint, game_name, config, num_tests, opponent=None, muzero_player=None, num_envs=64, seed=0,
             device=None, moves_per_batch=8, groups=1, use_graph=True, warmup_batches=0, temperature=0,
             device_temperatures=False, paired=False):
    """`MuZero.test` (reference muzero.py:346-396) on device-resident envs: `num_tests` games at temperature 0 and
    temperature threshold 0 (play_game(0, 0, False, opponent, muzero_player)), `num_envs` of them at a time, env e on
    the game and RNG stream of reference worker `seed + e`.

    `opponent` "self", "expert" or "random", `muzero_player` the side MuZero plays; None means the config's value.
    (The reference tests `if muzero_player`, which also sends an explicit 0 to the config; here only None does.)
    One-player games have no opponent: they are played as "self".

    The games counted are the first `num_tests` games STARTED, ordered by (ply of their env at which they began, env
    index) -- not the first finished, which would over-represent short games.  Envs keep playing until those are over.

    `warmup_batches` (for rate measurements): that many batches (or single moves, where batches do not apply) are
    played on the same actor first -- its buffers, the captured hipGraph and the history filer exist afterwards --;
    games that began during them are not counted and `seconds` / the move counts start after them.  With 0 the games
    are those of a fresh actor (num_envs = 1: the consecutive games of one SelfPlay worker of that seed).

    `temperature` (MuZero.test plays at 0) samples MuZero's moves instead of taking the most visited one;
    `device_temperatures` switches set_device_temperatures on, so that a temperature other than 0, inf and 1 / k runs as
    batches (against an opponent it cannot run at all without it).

    `paired` (against an opponent only): the opponent replies inside MuZero's move (set_opponent(paired=True)), so that
    every env is searched in every move of a batch instead of sitting every other search out.  Every env plays the games
    it plays in the sit-out mode, so with warmup_batches = 0 everything below but `seconds`, `env_moves`, `searched_moves`
    and `simulations` (the envs run on until the counted games are over, which the two modes reach at different points)
    is the sit-out mode's; warm-up batches cover about twice the plies here, so the games counted after them begin at other
    points of each env's sequence.  Needs move batches.

    Returns a dict: `result` is MuZero.test's number (one player: mean total reward; otherwise the mean of the rewards
    earned on muzero_player's moves), `muzero_reward` / `opponent_reward` the means per side (two players),
    `mean_episode_length`, `wins` / `draws` / `losses` (by comparing the two sides' rewards; None for one player),
    `games`, and the timed region's totals, counted games or not: `env_moves` (plies played by all envs),
    `searched_moves` (those that ran a search, counted by the history filer), `simulations`, `seconds`."""
    cfg = config
    if opponent is None:
        opponent = cfg.opponent
    if muzero_player is None:
        muzero_player = cfg.muzero_player
    two_players = len(cfg.players) > 1
    if not two_players or opponent is None:
        opponent = "self"
    num_tests, E = int(num_tests), int(num_envs)
    if num_tests < 1:
        raise ValueError("evaluate: num_tests must be positive")
    if groups > 1:
        actor = PipelinedDeviceSelfPlay(checkpoint, game_name, cfg, seed, E, groups=groups, device=device, use_graph=use_graph)
        probe = actor.actors[0]
    else:
        actor = probe = DeviceSelfPlay(checkpoint, game_name, cfg, seed, E, device=device, use_graph=use_graph)
    paired = bool(paired) and opponent != "self"
    actor.set_opponent(opponent, muzero_player, paired=paired)
    if device_temperatures:
        actor.set_device_temperatures(True)
    clock = numpy.zeros(E, dtype=numpy.int64)          # plies of env e's finished games
    plies = numpy.zeros(E, dtype=numpy.int64)          # plies env e has played
    found = {k: [] for k in ("start", "env", "length", "mine", "theirs", "total")}

    def on_games(batch):
        n = len(batch)
        env = numpy.array(batch.env_index, dtype=numpy.int64)
        length = numpy.array(batch.length, dtype=numpy.int64)
        W = batch.rewards.shape[1] - 1
        # (a batch lists an env's games together, oldest first: each starts where the one before ended)
        before = numpy.cumsum(length) - length
        new_env = numpy.r_[True, env[1:] != env[:-1]]
        found["start"].append(clock[env] + before - before[numpy.flatnonzero(new_env)][numpy.cumsum(new_env) - 1])
        numpy.add.at(clock, env, length)
        valid = numpy.arange(1, W + 1)[None, :] <= length[:, None]
        rewards = numpy.where(valid, batch.rewards[:n, 1:], 0.0).astype(numpy.float64)
        mine = (batch.to_play[:n, :W] == muzero_player) & valid      # reward i belongs to the player of move i - 1
        found["env"].append(env)
        found["length"].append(length)
        found["mine"].append((rewards * mine).sum(axis=1))
        found["theirs"].append((rewards * ~mine).sum(axis=1))
        found["total"].append(rewards.sum(axis=1))

    # the pipelined actor's batches always take the device-input form
    batched = probe._batchable(temperature, 0, moves_per_batch, device_inputs=True if groups > 1 else None)
    if paired and not batched:
        raise NotImplementedError("evaluate(paired=True) plays move batches: give moves_per_batch, a temperature the batches "
                                  "sample on the device and 0 < root_dirichlet_alpha <= 1")

    def play():
        if batched:
            plies[:] += actor.play_moves(moves_per_batch, temperature, on_games=on_games, temperature_threshold=0)
            actor.flush(on_games=on_games)
        else:
            actor.step(temperature, 0, on_games=on_games)
            plies[:] += 1

    for _ in range(int(warmup_batches)):
        play()
    first_ply = plies.copy()                           # games that began before it are not counted

    def counted():
        """Indices (into the concatenated records) of the first num_tests games started, once they are all over."""
        if not found["start"]:
            return None
        start, env = numpy.concatenate(found["start"]), numpy.concatenate(found["env"])
        e = int(numpy.lexsort((numpy.arange(E), clock))[0])       # the oldest game still running: every game that
        running = (int(clock[e]), e)                              # starts from now on starts after it
        eligible = start >= first_ply[env]
        earlier = eligible & ((start < running[0]) | ((start == running[0]) & (env < running[1])))
        if int(earlier.sum()) < num_tests:
            return None
        order = numpy.lexsort((env, start))
        return order[eligible[order]][:num_tests]

    torch.cuda.synchronize(probe.device)
    began = time.perf_counter()
    moves0, searched0 = actor.moves_played, actor.searched_moves
    while True:
        play()
        pick = counted()
        if pick is not None:
            break
    seconds = time.perf_counter() - began
    env_moves, searched = actor.moves_played - moves0, actor.searched_moves - searched0
    actor.close()
    col = {k: numpy.concatenate(v)[pick] for k, v in found.items()}
    out = dict(games=int(len(pick)), mean_episode_length=float(col["length"].mean()), env_moves=int(env_moves),
               searched_moves=int(searched), simulations=int(searched) * int(cfg.num_simulations), seconds=seconds,
               opponent=opponent, muzero_player=int(muzero_player), num_envs=E, paired=paired)
    if two_players:
        out.update(result=float(col["mine"].mean()), muzero_reward=float(col["mine"].mean()),
                   opponent_reward=float(col["theirs"].mean()), wins=int((col["mine"] > col["theirs"]).sum()),
                   draws=int((col["mine"] == col["theirs"]).sum()), losses=int((col["mine"] < col["theirs"]).sum()))
    else:
        out.update(result=float(col["total"].mean()), muzero_reward=float(col["total"].mean()), opponent_reward=0.0,
                   wins=None, draws=None, losses=None)
    return out
