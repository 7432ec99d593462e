"""The history filer's paired batches (include/mzhist.h mzhist_moves.slots), which need no GPU: a move carries up to
three plies in up to two games of an env; the packed games must equal a numpy restatement ply by ply."""
import importlib

import numpy as np
import pytest


def test_history_filer_files_paired_moves(pkg):
    """Random paired batches -- slot 0 searched or empty, slots 1 and 2 opponent plies or empty, games ending in any slot
    -- filed in two calls: every game equals the plies in (move, slot) order, a game that follows another inside a move
    starts from the reset observation with player 0 to move, empty slots file nothing, history(i) has None exactly on
    the opponent's plies, and searched_moves counts slot 0's."""
    sp = importlib.import_module("muzero-hypermodel_amd.self_play")
    E, M, A, S, L, slots = 7, 10, 4, 10, 8, 3
    obs_shape = (3, 2, 2)
    rs = np.random.RandomState(5)
    reset_obs = rs.randn(*obs_shape).astype(np.float32)
    filer = sp.HistoryFiler(E, L, obs_shape, A)
    filer.begin(np.tile(reset_obs, (E, 1, 1, 1)), np.zeros(E, np.int32))
    running = [[] for _ in range(E)]              # the plies of env e's running game: (action, reward, obs, to_play, cv, rv)
    want = [[] for _ in range(E)]
    got = [[] for _ in range(E)]
    searched = 0
    for call in range(2):
        out = dict(actions=rs.randint(0, A, (M, E)).astype(np.int32), visits=rs.randint(0, S, (M, E, A)).astype(np.int32),
                   root_value_sum=rs.randn(M, E), moves_done=np.full(E, M, np.int32))
        num_legal = rs.randint(1, A + 1, (M, E)).astype(np.int32)
        legal = np.stack([np.stack([rs.permutation(A) for _ in range(E)]) for _ in range(M)]).astype(np.int32)
        played = rs.randint(0, A, (M, slots, E)).astype(np.int32)
        played[:, 0] = out["actions"]
        played[rs.rand(M, slots, E) < 0.3] = -1
        done = (rs.rand(M, slots, E) < 0.3).astype(np.uint8)
        rewards = rs.randn(M, slots, E).astype(np.float32)
        obs_after = rs.randn(M, slots, E, *obs_shape).astype(np.float32)
        obs_next = rs.randn(M, E, *obs_shape).astype(np.float32)       # (not read in a paired batch)
        tp_after = rs.randint(0, 2, (M, slots, E)).astype(np.int32)
        # no game outgrows the row: force an end where a game would reach L plies
        length = [len(r) for r in running]
        for m in range(M):
            for s in range(slots):
                for e in range(E):
                    if played[m, s, e] < 0:
                        continue
                    length[e] += 1
                    if length[e] >= L - 1:
                        done[m, s, e] = 1
                    if done[m, s, e]:
                        length[e] = 0
        assert ((played >= 0) & (done == 1))[:, 0].any() and ((played >= 0) & (done == 1))[:, 1].any()
        assert ((played[:, 1] >= 0) & (done[:, 1] == 1) & (played[:, 2] >= 0)).any()     # an opening in slot 2
        batch = filer.file(out, legal, num_legal, S, rewards, done, obs_after, obs_next, to_play_after=tp_after,
                           played=played, slots=slots, reset_obs=reset_obs)
        for i in range(len(batch)):
            got[int(batch.env_index[i])].append(batch.history(i))
        for e in range(E):
            for m in range(M):
                for s in range(slots):
                    if played[m, s, e] < 0:
                        continue
                    if s == 0:
                        cv = np.zeros(A)
                        cv[legal[m, e, : num_legal[m, e]]] = out["visits"][m, e, : num_legal[m, e]] / S
                        ply = (int(out["actions"][m, e]), float(rewards[m, s, e]), obs_after[m, s, e], int(tp_after[m, s, e]),
                               cv.tolist(), out["root_value_sum"][m, e] / S)
                        searched += 1
                    else:
                        ply = (int(played[m, s, e]), float(rewards[m, s, e]), obs_after[m, s, e], int(tp_after[m, s, e]),
                               None, None)
                    running[e].append(ply)
                    if done[m, s, e]:
                        want[e].append(running[e])
                        running[e] = []
    assert sum(len(g) for g in want) > 3 * E
    for e in range(E):
        assert len(got[e]) == len(want[e]), e
        for gh, plies in zip(got[e], want[e]):
            assert gh.action_history == [0] + [p[0] for p in plies]
            assert gh.reward_history == [0.0] + [p[1] for p in plies]
            assert gh.to_play_history == [0] + [p[3] for p in plies]
            assert np.array_equal(np.array(gh.observation_history), np.stack([reset_obs] + [p[2] for p in plies]))
            assert gh.root_values == [p[5] for p in plies]
            assert gh.child_visits == [p[4] for p in plies if p[4] is not None]
    assert filer.searched_moves() == searched
    assert np.array_equal(filer.lengths(), [len(r) for r in running])
    # a paired batch without the played actions or the reset observation is refused
    with pytest.raises((RuntimeError, AssertionError, TypeError)):
        filer.file(out, legal, num_legal, S, rewards, done, obs_after, obs_next, to_play_after=tp_after, slots=slots,
                   reset_obs=reset_obs)
