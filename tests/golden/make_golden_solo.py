#!/usr/bin/env python3
"""Generate the fixtures of the two numpy-only one-player games (G23) under tests/golden/ by RUNNING the reference's
games/twentyone.py and games/simple_grid.py.

Build-container only, like make_golden.py (whose helpers it imports and which stays as it is): the reference is
imported from its checkout, inputs and expected outputs are recorded as .npz files, and nothing but data is written.

    python tests/golden/make_golden_solo.py

g23_twentyone_env.npz -- 64 envs, env e = the reference's Game(e), 400 plies each, the action of ply t drawn with
numpy.random.RandomState(9000 + e).randint(2); a finished game is reset in place.  No observation is stored: the
generator checks at every point that the reference's observation is [full(player_hand), full(dealer_hand), zeros] with
dtypes float32 / float32 / int64, and stores the hands.
  seed [64]                         Game(seed)
  ctor_hands [64,2], ctor_pos [64]  hands and stream position (RandomState.get_state()[2]) after the constructor
  ctor_words [64]                   32-bit words the constructor's two cards consumed
  first_hands, first_pos, first_words   the same after the first reset()
  action, reward, done [64,400]     the ply; reward is the Game wrapper's (x10)
  hands [64,400,2]                  player_hand, dealer_hand after the ply (the terminal position where done)
  pos, words [64,400]               stream position after the ply, words the ply consumed
  ply [64,400]                      plies of the env's current game, this one included
  next_hands [64,400,2], next_pos, reset_words [64,400]   after the reset that follows a finished game (elsewhere
                                    equal to hands / pos, 0)
Coverage, asserted here so that a numpy that draws differently fails loudly: EVERY env reaches a hit to exactly 21, a
bust, a dealer bust, a dealer win, a win on the higher hand, a dealer that stops at 17 and a dealer that draws two or
more cards; 62 of the 64 reach a tie; every env consumes more than 1000 words in its first 300 plies (its stream is
regenerated at least once); the longest game has 6 plies.

g23_simple_grid_env.npz -- one row per ply: seq, step, action, row, col (after the ply), reward, done; `length[seq]`.
Sequences 0..63 are all 2^6 action sequences of length 6 from the start (bit t of the sequence number is ply t's
action), cut where the game ends; sequence 64 goes down twice, then plays 12 illegal moves along the bottom row (six
"down" at (2, 0), one legal "right", six "down" at (2, 1)) and never ends.  Observations are checked to be the one-hot
of 3 * row + col (float64, wrapped in two lists) and not stored.

Both files carry the reference's MuZeroConfig field by field as `cfg_*` (None stored as the string "None"; results_path
and train_on_gpu left out) and `cfg_temperatures`, visit_softmax_temperature_fn at 0, 499999, 500000, 749999, 750000
and 1000000 trained steps.
"""
import sys

import numpy

import make_golden as mg

ENVS, PLIES = 64, 400
TEMPERATURE_STEPS = (0, 499999, 500000, 749999, 750000, 1000000)


def full_config(config):
    out = {}
    for key, value in sorted(vars(config).items()):
        if key in ("results_path", "train_on_gpu"):      # a path with a time stamp; a property of the machine
            continue
        out["cfg_" + key] = numpy.array("None" if value is None else value)
    out["cfg_temperatures"] = numpy.array([float(config.visit_softmax_temperature_fn(t)) for t in TEMPERATURE_STEPS])
    return out


def words_between(before, after):
    """Stream positions are 1..624 once a word was drawn (624 right after seeding); fewer than 624 words lie between."""
    return int(after - before) if after >= before else int(624 - before + after)


def check_t21_observation(obs, env):
    assert len(obs) == 3 and [str(o.dtype) for o in obs] == ["float32", "float32", "int64"]
    assert all(o.shape == (3, 3) for o in obs)
    assert (obs[0] == env.player_hand).all() and (obs[1] == env.dealer_hand).all() and (obs[2] == 0).all()
    assert numpy.array(obs).shape == (3, 3, 3)


def g23_twentyone(twentyone):
    a = dict(seed=numpy.arange(ENVS), ctor_hands=numpy.zeros((ENVS, 2), "int32"), ctor_pos=numpy.zeros(ENVS, "int32"),
             ctor_words=numpy.zeros(ENVS, "int32"), first_hands=numpy.zeros((ENVS, 2), "int32"),
             first_pos=numpy.zeros(ENVS, "int32"), first_words=numpy.zeros(ENVS, "int32"))
    for name in ("action", "reward", "done", "pos", "words", "ply", "next_pos", "reset_words"):
        a[name] = numpy.zeros((ENVS, PLIES), "int32")
    a["hands"] = numpy.zeros((ENVS, PLIES, 2), "int32")
    a["next_hands"] = numpy.zeros((ENVS, PLIES, 2), "int32")
    ties, longest = 0, 0
    for e in range(ENVS):
        game = twentyone.Game(e)
        env = game.env
        position = lambda: int(env.random.get_state()[2])
        a["ctor_hands"][e] = env.player_hand, env.dealer_hand
        a["ctor_pos"][e] = a["ctor_words"][e] = position()      # (the first draw regenerates the block: position = words)
        check_t21_observation(game.reset(), env)
        a["first_hands"][e] = env.player_hand, env.dealer_hand
        a["first_pos"][e] = position()
        a["first_words"][e] = position() - a["ctor_pos"][e]
        cards = [0]
        deal = env.deal_card_value

        def counting_deal():
            cards[0] += 1
            return deal()

        env.deal_card_value = counting_deal
        seen = set()
        actions = numpy.random.RandomState(9000 + e)
        ply, words_300 = 0, 0
        for t in range(PLIES):
            action = int(actions.randint(2))
            before, cards[0] = position(), 0
            obs, reward, done = game.step(action)
            assert type(reward) is int and type(done) is bool and game.legal_actions() == [0, 1] and game.to_play() == 0
            check_t21_observation(obs, env)
            ply += 1
            player, dealer = env.player_hand, env.dealer_hand
            a["action"][e, t], a["reward"][e, t], a["done"][e, t], a["ply"][e, t] = action, reward, done, ply
            a["hands"][e, t] = player, dealer
            a["pos"][e, t] = position()
            a["words"][e, t] = words_between(before, position())
            assert a["words"][e, t] >= cards[0]
            if done:
                dealer_cards = cards[0] - (action == 0)
                if action == 0 and player == 21:
                    seen.add("hit21")
                if player > 21:
                    seen.add("bust")
                    assert reward == -10 and dealer_cards == 0
                else:
                    assert dealer > 16
                    seen.add("dealer_bust" if dealer > 21 else "tie" if dealer == player else
                             "higher_hand" if dealer < player else "dealer_win")
                    assert reward == (10 if dealer > 21 or dealer < player else 0 if dealer == player else -10)
                    if dealer == 17 and dealer_cards >= 1:
                        seen.add("dealer17")
                    if dealer_cards >= 2:
                        seen.add("dealer_two_cards")
                longest = max(longest, ply)
                before = position()
                check_t21_observation(game.reset(), env)
                a["reset_words"][e, t] = words_between(before, position())
                ply = 0
            else:
                assert reward == 0
            a["next_hands"][e, t] = env.player_hand, env.dealer_hand
            a["next_pos"][e, t] = position()
            if t < 300:
                words_300 += a["words"][e, t] + a["reset_words"][e, t]
        need = {"hit21", "bust", "dealer_bust", "dealer_win", "higher_hand", "dealer17", "dealer_two_cards"}
        assert need <= seen, (e, need - seen)
        assert words_300 > 1000, (e, words_300)
        ties += "tie" in seen
    assert ties == 62 and longest == 6, (ties, longest)
    total = a["words"].sum() + a["reset_words"].sum()
    print(f"   twentyone: {int(a['done'].sum())} games, {total / (ENVS * PLIES):.2f} words per ply, ties in {ties} envs")
    a.update(full_config(twentyone.MuZeroConfig()))
    mg.save("g23_twentyone_env", **a)


def g23_simple_grid(simple_grid):
    rows = dict(seq=[], step=[], action=[], row=[], col=[], reward=[], done=[])
    lengths = []
    sequences = [[(s >> t) & 1 for t in range(6)] for s in range(64)]
    sequences.append([0, 0] + [0] * 6 + [1] + [0] * 6)

    def check(obs, env):
        assert len(obs) == 1 and len(obs[0]) == 1 and obs[0][0].dtype == numpy.float64 and obs[0][0].shape == (9,)
        want = numpy.zeros(9)
        want[3 * env.position[0] + env.position[1]] = 1
        assert numpy.array_equal(obs[0][0], want)

    for s, actions in enumerate(sequences):
        game = simple_grid.Game(s)
        check(game.reset(), game.env)
        assert game.env.position == [0, 0]
        t = 0
        for action in actions:
            legal = action in game.env.legal_actions()
            before = list(game.env.position)
            obs, reward, done = game.step(action)
            assert type(reward) is int and type(done) is bool and game.legal_actions() == [0, 1]
            check(obs, game.env)
            assert legal or game.env.position == before
            t += 1
            rows["seq"].append(s); rows["step"].append(t); rows["action"].append(action)
            rows["row"].append(game.env.position[0]); rows["col"].append(game.env.position[1])
            rows["reward"].append(reward); rows["done"].append(done)
            if done:
                break
        lengths.append(t)
    arrays = {k: numpy.array(v, dtype="int32") for k, v in rows.items()}
    arrays["length"] = numpy.array(lengths, dtype="int32")
    assert lengths[64] == 15 and not arrays["done"][arrays["seq"] == 64].any()
    assert sorted(set(lengths[:64])) == [4, 5, 6] and int(arrays["done"].sum()) == 50
    print("   simple_grid:", len(arrays["seq"]), "plies,", int(arrays["done"].sum()), "sequences reach the goal")
    arrays.update(full_config(simple_grid.MuZeroConfig()))
    mg.save("g23_simple_grid_env", **arrays)


def main():
    mg.import_reference()
    import games.simple_grid as simple_grid
    import games.twentyone as twentyone
    g23_twentyone(twentyone)
    g23_simple_grid(simple_grid)


if __name__ == "__main__":
    sys.exit(main())
