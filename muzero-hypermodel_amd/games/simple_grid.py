"""SimpleGrid plugin (reference games/simple_grid.py): config :10-121, rules :190-227, wrapper :124-188.

One player walks a 3 x 3 grid from (0, 0) to (2, 2): action 0 moves down, action 1 right.  `Game.legal_actions()` is
[0, 1] in every state -- the wrapper does not forward `GridEnv.legal_actions()` -- and a move the grid does not allow
moves nothing, so the game's own rules may never end it: play that dawdles ends at `config.max_moves` = 6.  Reward 10
and done exactly when the position becomes (2, 2) (recorded games: tests/golden/g23_simple_grid_env.npz; the same
rules for host and device: csrc/solo_rules.h).
"""
import numpy

from ._config import BaseMuZeroConfig
from .abstract_game import AbstractGame


class MuZeroConfig(BaseMuZeroConfig):
    GAME = "simple_grid"
    OVERRIDES = dict(
        observation_shape=(1, 1, 9), action_space=list(range(2)), players=[0], max_moves=6, num_simulations=10,
        discount=0.978, encoding_size=5, fc_representation_layers=[16], training_steps=30000, batch_size=32,
        lr_init=0.0064, lr_decay_rate=1, replay_buffer_size=5000, num_unroll_steps=7, td_steps=7,
        self_play_delay=0.2, ratio=None)

    def visit_softmax_temperature_fn(self, trained_steps):
        return 1


class GridEnv:
    def __init__(self, size=3):
        self.size = size
        self.position = [0, 0]

    def legal_actions(self):
        return [axis for axis in (0, 1) if self.position[axis] != self.size - 1]

    def step(self, action):
        if action in self.legal_actions():
            self.position[action] += 1
        reward = 1 if self.position == [self.size - 1, self.size - 1] else 0
        return self.get_observation(), reward, bool(reward)

    def reset(self):
        self.position = [0, 0]
        return self.get_observation()

    def render(self):
        picture = numpy.full((self.size, self.size), "-")
        picture[self.size - 1, self.size - 1] = "1"
        picture[self.position[0], self.position[1]] = "x"
        print(picture)

    def get_observation(self):
        observation = numpy.zeros(self.size * self.size)
        observation[self.size * self.position[0] + self.position[1]] = 1
        return observation


class Game(AbstractGame):
    def __init__(self, seed=None):
        self.env = GridEnv()

    def step(self, action):
        observation, reward, done = self.env.step(action)
        return [[observation]], reward * 10, done

    def legal_actions(self):
        return list(range(2))

    def reset(self):
        return [[self.env.reset()]]

    def render(self):
        self.env.render()
        input("Press enter to take a step ")

    def action_to_string(self, action_number):
        names = {0: "Down", 1: "Right"}
        return f"{action_number}. {names[action_number]}"
