"""TwentyOne plugin (reference games/twentyone.py): config :17-133, rules :227-299, wrapper :136-224.

A simplified twenty-one against a dealer: an ace always counts 1, so there is no two-card 21.  The player hits
(action 0) or stands (action 1); a stand, a bust or a hand of exactly 21 ends the game, and unless the player is busted
the dealer then draws until its hand exceeds 16.  A card is `RandomState(seed).randint(1, 13)` on the game's own
stream, 10 and above counting 10 -- the one stochastic transition among the games here (recorded games with their
stream positions: tests/golden/g23_twentyone_env.npz; the same rules for host and device: csrc/solo_rules.h).
`Game(seed)` deals two cards in its constructor that `reset()` replaces, as the reference does.
"""
import numpy

from ._config import BaseMuZeroConfig
from .abstract_game import AbstractGame


class MuZeroConfig(BaseMuZeroConfig):
    GAME = "twentyone"
    OVERRIDES = dict(
        observation_shape=(3, 3, 3), action_space=list(range(2)), players=[0], num_workers=4, max_moves=21,
        num_simulations=21, discount=1, network="resnet", blocks=2, channels=32, reduced_channels_reward=32,
        reduced_channels_value=32, reduced_channels_policy=32, resnet_fc_reward_layers=[16],
        resnet_fc_value_layers=[16], resnet_fc_policy_layers=[16], encoding_size=32, fc_representation_layers=[16],
        training_steps=15000, batch_size=64, value_loss_weight=0.25, optimizer="SGD", lr_init=0.03,
        lr_decay_rate=0.75, lr_decay_steps=150000, replay_buffer_size=10000, num_unroll_steps=20, td_steps=50,
        ratio=None)

    def visit_softmax_temperature_fn(self, trained_steps):
        if trained_steps < 500e3:
            return 1.0
        elif trained_steps < 750e3:
            return 0.5
        return 0.25


class TwentyOne:
    def __init__(self, seed):
        self.random = numpy.random.RandomState(seed)
        self.player_hand = self.card()
        self.dealer_hand = self.card()
        self.player = 1

    def card(self):
        return min(self.random.randint(1, 13), 10)

    def to_play(self):
        return 0 if self.player == 1 else 1

    def reset(self):
        self.player_hand = self.card()
        self.dealer_hand = self.card()
        self.player = 1
        return self.get_observation()

    def step(self, action):
        if action == 0:
            self.player_hand += self.card()
        busted = self.player_hand > 21
        done = busted or action == 1 or self.player_hand == 21
        if done and not busted:
            while self.dealer_hand <= 16:
                self.dealer_hand += self.card()
        return self.get_observation(), self.reward(done), done

    def reward(self, done):
        if not done:
            return 0
        if self.player_hand > 21:
            return -1
        if self.dealer_hand < self.player_hand or self.dealer_hand > 21:
            return 1
        return 0 if self.dealer_hand == self.player_hand else -1

    def get_observation(self):
        # (the third plane is an integer array, as the reference's is: numpy.array(observation) is float64)
        return [numpy.full((3, 3), self.player_hand, dtype="float32"),
                numpy.full((3, 3), self.dealer_hand, dtype="float32"),
                numpy.full((3, 3), 0)]

    def legal_actions(self):
        return [0, 1]

    def render(self):
        print("Dealer hand: " + str(self.dealer_hand))
        print("Player hand: " + str(self.player_hand))


class Game(AbstractGame):
    def __init__(self, seed=None):
        self.env = TwentyOne(seed)

    def step(self, action):
        observation, reward, done = self.env.step(action)
        return observation, reward * 10, done

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
        choice = input(f"Enter the action (0) Hit, or (1) Stand for the player {self.to_play()}: ")
        while choice not in [str(action) for action in self.legal_actions()]:
            choice = input("Enter either (0) Hit or (1) Stand : ")
        return int(choice)

    def action_to_string(self, action_number):
        names = {0: "Hit", 1: "Stand"}
        return f"{action_number}. {names[action_number]}"
