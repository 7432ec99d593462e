"""The closed MuZero loop on one GPU, for every device game: self-play in move batches (DeviceSelfPlay.play_moves) ->
finished games filed into the replay store on the device (file_to, with their outcomes) -> replay batches drawn on the
device (ReplayBuffer(device_sampling=True)) -> training steps queued without a host trip (Trainer.train_steps) ->
an optional batched Reanalyse pass -> weights published back into the actors' flat buffers (Trainer.publish) -> every few
iterations an evaluation against the config's opponent (self_play.evaluate).

What tools/train_cartpole.py hard-wires for CartPole -- the config, the fused engine's flat buffer, the fc_* trainer
flags, "the reward sum is the length" -- is here a matter of the config alone: the network is whatever it says, the
learning curve comes from what the filer reports about every finished game (self_play.GameOutcomes: total reward, reward
per player, mean root value; csrc/game_outcomes.h), and no game is downloaded to log it.

One JSON-serialisable row per iteration (TrainingLoop.iterate):
    iteration, training_step, num_played_games, num_played_steps, num_reanalysed_games, lr, temperature,
    total_loss, value_loss, reward_loss, policy_loss (the last step of the iteration; None before the first step),
    games_finished, and over the last 50 outcomes mean_total_reward, max_total_reward, mean_length, mean_value,
    mean_reward_player0, mean_reward_player1 (None while no game has finished), eval (MuZero.test's numbers under the
    reference's names -- total_reward, episode_length, muzero_reward, opponent_reward -- with the games counted and the
    opponent; evaluation games are played through the host path, which reports no root values; or None), seconds.
"""
import collections
import importlib
import math
import time

import numpy
import torch

from . import models, replay_buffer as replay_buffer_module, self_play, trainer as trainer_module
from .weights import FlatWeights

DEVICE_GAMES = ("cartpole", "tictactoe", "connect4", "gomoku", "twentyone", "simple_grid")
RECENT_GAMES = 50      # outcomes a row averages over (the reference's tensorboard smoothing is the reader's business)
TEMPERATURE_SCAN = 100000   # iterations of the schedule looked at for a temperature the batches refuse


def game_config(game_name, overrides=None):
    """games.<game_name>.MuZeroConfig() with `overrides` (a dict of attribute -> value) applied; unknown attributes are an
    error, so that a typo does not silently train the default."""
    if game_name not in DEVICE_GAMES:
        raise ValueError(f"no device game {game_name!r}: one of {', '.join(DEVICE_GAMES)}")
    config = importlib.import_module(f"{__package__}.games.{game_name}").MuZeroConfig()
    for key, value in (overrides or {}).items():
        if not hasattr(config, key):
            raise AttributeError(f"MuZeroConfig of {game_name} has no attribute {key!r}")
        setattr(config, key, value)
    return config


class TrainingLoop:
    def __init__(self, game_name, config, envs, moves_per_iteration, train_steps_per_iteration, seed, reanalyse_games=0,
                 eval_every=0, eval_games=0, eval_opponent=None, groups=1, trainer_flags=None, device_filing=True,
                 log=None, eval_paired=False):
        """`config`: a games.*.MuZeroConfig (game_config()).  `envs` device envs play `moves_per_iteration` plies each per
        iteration, then `train_steps_per_iteration` steps are trained.  `groups` > 1: a PipelinedDeviceSelfPlay.
        `trainer_flags`: Trainer's keyword flags verbatim (default: graph=True, and fc_step / fc_optimizer for a
        fully-connected network); what the trainer refuses it says itself.  device_filing=False plays the same games
        through on_games -> save_games and asks the store for their outcomes (ReplayBuffer.game_outcomes): the twin the
        tests compare against.  eval_paired=True: evaluation games against an opponent let it reply inside MuZero's move
        (self_play.evaluate(paired=True)): the same games and `eval` numbers in less GPU time; off by default.  `log`: called with a line of text for the few things the loop decides on its own."""
        if game_name not in DEVICE_GAMES:
            raise ValueError(f"no device game {game_name!r}: one of {', '.join(DEVICE_GAMES)}")
        self.game_name, self.config, self.seed = game_name, config, int(seed)
        self.moves, self.steps = int(moves_per_iteration), int(train_steps_per_iteration)
        self.reanalyse_games, self.device_filing = int(reanalyse_games), bool(device_filing)
        self.eval_every, self.eval_games = int(eval_every), int(eval_games)
        self.eval_paired = bool(eval_paired)
        self._say = log or (lambda line: None)
        config.seed = self.seed
        fully_connected = config.network == "fullyconnected"
        two_players = len(config.players) > 1
        # evaluation: the opponent asked for, else the config's; one-player games have none
        self.eval_opponent = None
        if two_players:
            self.eval_opponent = eval_opponent if eval_opponent is not None else config.opponent
            if self.eval_opponent == "expert" and game_name == "gomoku":
                self._say('gomoku has no expert agent: evaluating against "random"')
                self.eval_opponent = "random"
        torch.manual_seed(self.seed)
        weights = models.MuZeroNetwork(config).get_weights()
        checkpoint = {"weights": weights}
        if groups > 1:
            self.actor = self_play.PipelinedDeviceSelfPlay(checkpoint, game_name, config, self.seed, envs, groups=groups)
            actors = self.actor.actors
        else:
            self.actor = self_play.DeviceSelfPlay(checkpoint, game_name, config, self.seed, envs)
            actors = [self.actor]
        # where Trainer.publish puts the weights: the flat buffer the fused engine reads (fully-connected networks), else one
        # laid under the actor's model
        if fully_connected:
            for actor in actors:
                actor.engine.set_fused_options("auto", publish_tree=False)
            self.flats = [actor.engine._fc_flat for actor in actors]
        else:
            self.flats = [FlatWeights(actor.model) for actor in actors]
        if any(flat is None for flat in self.flats):
            raise RuntimeError("the actor's engine holds no flat weight buffer for this fully-connected network")
        self.replay = replay_buffer_module.ReplayBuffer({"num_played_games": 0, "num_played_steps": 0}, {}, config,
                                                        device_sampling=True)
        if trainer_flags is None:
            trainer_flags = dict(graph=True, **(dict(fc_step=True, fc_optimizer=True) if fully_connected else {}))
        self.trainer = trainer_module.Trainer({"weights": weights, "training_step": 0, "optimizer_state": None}, config,
                                              device="cuda", **trainer_flags)
        self.reanalyse = None
        if self.reanalyse_games > 0:
            self.reanalyse = replay_buffer_module.Reanalyse(checkpoint, config, flat=self.flats[0] if fully_connected else None)
        if self.device_filing:
            self.actor.file_to(self.replay, outcomes=True)
        # a temperature of the schedule that the batches refuse as they are: sampled on the GPU from the start
        probe = actors[0]
        steps = range(0, int(config.training_steps) + 1, max(1, self.steps))[:TEMPERATURE_SCAN]
        if any(not probe._device_samples(config.visit_softmax_temperature_fn(step)) for step in steps):
            self._say("the temperature schedule leaves 0 and 1 / k: set_device_temperatures() is on")
            self.actor.set_device_temperatures(True)
        self.iteration = 0
        self.games_finished = 0
        self.recent = collections.deque(maxlen=RECENT_GAMES)   # (total reward, length, mean value, reward 0, reward 1)
        self._host_outcomes = []
        self._began = time.perf_counter()

    # ---- finished games ---------------------------------------------------------------------------------------------
    def _on_games_host(self, batch):
        """device_filing=False: the games go through the host into the store, which is then asked what they report."""
        first = self.replay.num_played_games
        self.replay.save_games(batch)
        got = self.replay.game_outcomes(range(first, first + len(batch)))
        self._host_outcomes.append(self_play.GameOutcomes(numpy.asarray(batch.env_index, dtype=numpy.int32), *got[1:]))

    def _take_outcomes(self):
        if self.device_filing:
            return self.actor.take_outcomes()
        taken, self._host_outcomes = self._host_outcomes, []
        return self_play.GameOutcomes.concatenate(taken)

    def _book(self, outcomes):
        self.games_finished += len(outcomes)
        mean_value = outcomes.mean_value
        for i in range(max(0, len(outcomes) - RECENT_GAMES), len(outcomes)):
            self.recent.append((float(outcomes.total_reward[i]), int(outcomes.length[i]), float(mean_value[i]),
                                float(outcomes.reward_of_player[i, 0]), float(outcomes.reward_of_player[i, 1])))

    # ---- one iteration ----------------------------------------------------------------------------------------------
    def iterate(self):
        config, trainer, replay = self.config, self.trainer, self.replay
        temperature = config.visit_softmax_temperature_fn(trainer.training_step)
        self.actor.play_moves(self.moves, temperature, on_games=None if self.device_filing else self._on_games_host)
        self._book(self._take_outcomes())
        losses = None
        if replay.num_played_games > 0:
            losses = trainer.train_steps(replay, self.steps)
        if self.reanalyse is not None:
            if config.network != "fullyconnected" and replay.num_played_games > 0:
                self.reanalyse.model.set_weights(trainer.model.state_dict())   # (the pass runs on a model of its own)
            self.reanalyse.reanalyse_games(replay, self.reanalyse_games)
        if losses is not None:
            for flat in self.flats:
                trainer.publish(flat)                        # fresh weights for the next batch of searches
        row = dict(iteration=self.iteration, training_step=int(trainer.training_step),
                   num_played_games=int(replay.num_played_games), num_played_steps=int(replay.num_played_steps),
                   num_reanalysed_games=int(self.reanalyse.num_reanalysed_games) if self.reanalyse is not None else 0,
                   lr=float(getattr(trainer, "_lr_host", config.lr_init)), temperature=float(temperature))
        for name, value in zip(("total_loss", "value_loss", "reward_loss", "policy_loss"), losses or (None,) * 4):
            row[name] = value
        row["games_finished"] = self.games_finished
        row.update(self._recent_means())
        row["eval"] = None
        self.iteration += 1
        if self.eval_every > 0 and self.eval_games > 0 and self.iteration % self.eval_every == 0:
            row["eval"] = self.evaluate()
        row["seconds"] = time.perf_counter() - self._began
        return row

    def _recent_means(self):
        if not self.recent:
            return dict.fromkeys(("mean_total_reward", "max_total_reward", "mean_length", "mean_value", "mean_reward_player0",
                                  "mean_reward_player1"))
        total, length, value, first, second = (numpy.array(column, dtype=numpy.float64) for column in zip(*self.recent))
        counted = value[~numpy.isnan(value)]                 # (a game whose every root value is zero has no mean)
        return dict(mean_total_reward=float(total.mean()), max_total_reward=float(total.max()),
                    mean_length=float(length.mean()), mean_value=float(counted.mean()) if len(counted) else None,
                    mean_reward_player0=float(first.mean()), mean_reward_player1=float(second.mean()))

    def evaluate(self):
        """self_play.evaluate with the trainer's weights: the reference's five test metrics."""
        weights = {k: v.detach().cpu().clone() for k, v in self.trainer.model.state_dict().items()}
        out = self_play.evaluate({"weights": weights}, self.game_name, self.config, self.eval_games,
                                 opponent=self.eval_opponent, num_envs=min(64, self.eval_games), seed=self.seed,
                                 paired=self.eval_paired and self.eval_opponent not in (None, "self"))
        return dict(total_reward=out["result"], episode_length=out["mean_episode_length"],
                    muzero_reward=out["muzero_reward"], opponent_reward=out["opponent_reward"], games=out["games"],
                    opponent=out["opponent"])

    def run(self, iterations, on_row=None):
        rows = []
        for _ in range(int(iterations)):
            rows.append(self.iterate())
            if on_row is not None:
                on_row(rows[-1])
        return rows

    def close(self):
        """The last batch's games are filed and booked, then everything is released; returns their outcomes' count."""
        self.actor.flush(on_games=None if self.device_filing else self._on_games_host)
        last = self._take_outcomes()
        self._book(last)
        self.actor.close()
        self.replay.close()
        return len(last)


def finite(row):
    """True when every loss of a row that has losses is a finite number."""
    return all(row[k] is None or math.isfinite(row[k]) for k in ("total_loss", "value_loss", "reward_loss", "policy_loss"))
