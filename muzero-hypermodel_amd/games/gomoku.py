"""Gomoku plugin (reference games/gomoku.py): config :10-116, rules :219-291, letter-pair actions :309-328.

11 x 11 board, action = cell = 11 * row + column.  Same observations (planes [first player's stones, second
player's, side to move as +1 / -1]), rewards (1 for the ply that ends the game, a full-board draw included),
legal-action order (ascending cells) and end-of-game test as the reference (recorded games:
tests/golden/g18_gomoku_env.npz).  The end-of-game test is the reference's whole-board one -- any stone of
either colour that starts five equal stones down-left, down, down-right or right -- done here with shifted
views of a zero-bordered board instead of a walk per stone.  There is no expert agent, as in the reference.
"""
import numpy

from ._config import BaseMuZeroConfig
from .abstract_game import AbstractGame

SIZE = 11
# (row, column) steps of the four scanned directions
DIRECTIONS = ((1, -1), (1, 0), (1, 1), (0, 1))


class MuZeroConfig(BaseMuZeroConfig):
    GAME = "gomoku"
    OVERRIDES = dict(
        observation_shape=(3, SIZE, SIZE), action_space=list(range(SIZE * SIZE)), players=[0, 1], opponent="random",
        num_workers=2, max_moves=121, num_simulations=400, discount=1, root_dirichlet_alpha=0.3, network="resnet",
        blocks=6, channels=128, reduced_channels_reward=2, reduced_channels_value=2, reduced_channels_policy=4,
        resnet_fc_reward_layers=[64], resnet_fc_value_layers=[64], resnet_fc_policy_layers=[64], encoding_size=32,
        fc_dynamics_layers=[64], fc_reward_layers=[64], fc_value_layers=[], fc_policy_layers=[],
        training_steps=10000, batch_size=512, checkpoint_interval=50, value_loss_weight=1, lr_init=0.002,
        lr_decay_rate=0.9, lr_decay_steps=10000, replay_buffer_size=10000, num_unroll_steps=121, td_steps=121,
        use_last_model_value=False, ratio=1)

    def visit_softmax_temperature_fn(self, trained_steps):
        if trained_steps < 0.5 * self.training_steps:
            return 1.0
        elif trained_steps < 0.75 * self.training_steps:
            return 0.5
        return 0.25


class Gomoku:
    def __init__(self):
        self.board_size = SIZE
        self.board = numpy.zeros((SIZE, SIZE), dtype="int32")
        self.player = 1
        self.board_markers = [chr(ord("A") + i) for i in range(SIZE)]

    def to_play(self):
        return 0 if self.player == 1 else 1

    def reset(self):
        self.board = numpy.zeros((SIZE, SIZE), dtype="int32")
        self.player = 1
        return self.get_observation()

    def step(self, action):
        self.board[action // SIZE, action % SIZE] = self.player
        done = self.is_finished()
        self.player *= -1
        return self.get_observation(), 1 if done else 0, done

    def get_observation(self):
        first = numpy.where(self.board == 1, 1.0, 0.0)
        second = numpy.where(self.board == -1, 1.0, 0.0)
        turn = numpy.full((SIZE, SIZE), self.player, dtype="int32")
        return numpy.array([first, second, turn])

    def legal_actions(self):
        return [int(cell) for cell in numpy.flatnonzero(self.board == 0)]

    def is_finished(self):
        """Five equal stones in a line anywhere on the board, whoever they belong to, or no empty cell left."""
        bordered = numpy.zeros((SIZE + 4, SIZE + 8), dtype="int32")   # 4 rows below, 4 columns either side
        bordered[:SIZE, 4:4 + SIZE] = self.board
        start = bordered[:SIZE, 4:4 + SIZE]
        for dr, dc in DIRECTIONS:
            run = start != 0
            for k in range(1, 5):
                run = run & (bordered[k * dr:k * dr + SIZE, 4 + k * dc:4 + k * dc + SIZE] == start)
            if run.any():
                return True
        return not (self.board == 0).any()

    def render(self):
        print("  " + "".join(marker + " " for marker in self.board_markers))
        for row in range(SIZE):
            print(self.board_markers[row] + " " + "".join(".XO"[self.board[row, col]] + " " for col in range(SIZE)))

    def human_input_to_action(self):
        text = input("Enter an action: ")
        if len(text) == 2 and text[0] in self.board_markers and text[1] in self.board_markers:
            row, col = ord(text[0]) - ord("A"), ord(text[1]) - ord("A")
            if self.board[row, col] == 0:
                return True, row * SIZE + col
        return False, -1

    def action_to_human_input(self, action):
        return chr(ord("A") + action // SIZE) + chr(ord("A") + action % SIZE)


class Game(AbstractGame):
    def __init__(self, seed=None):
        self.env = Gomoku()

    def step(self, action):
        return self.env.step(action)

    def to_play(self):
        return self.env.to_play()

    def legal_actions(self):
        return self.env.legal_actions()

    def reset(self):
        return self.env.reset()

    def render(self):
        self.env.render()
        input("Press enter to take a step ")

    def human_to_action(self):
        valid = False
        while not valid:
            valid, action = self.env.human_input_to_action()
        return action

    def action_to_string(self, action):
        return self.env.action_to_human_input(action)
