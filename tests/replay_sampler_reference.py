"""The sampling of one replay batch with numpy's own legacy generator: the yardstick the device sampler (csrc/mzreplay.hip,
arithmetic in csrc/replay_sampler.h) is held to, bit for bit, by tests/test_gpu_replay_sampler_forms.py.

It follows the order named in the header comment of csrc/replay_sampler.h and nothing else: numpy.sum, numpy's float32
division, numpy.random.RandomState.choice and Python's sum do the arithmetic -- none of it is restated here.  (The
restated copy, with one switch per way of getting it wrong, is in tests/test_replay_sampler_reference.py.)

`ModelStore` is the bookkeeping around it: which games a ring of `capacity` slots holds, oldest to newest, with their
priorities, and update_priorities as a sequential loop."""
import numpy as np


def sample_batch(rs, game_priority, lengths, priorities, batch, unroll, num_actions, per, total_samples):
    """One batch from `rs` (numpy.random.RandomState), which is left where the batch leaves it.

    game_priority  float32 [n], stored games oldest to newest        lengths  int [n]
    priorities     sequence of n float32 arrays (read where per)     total_samples  Python int: sum of the lengths
    Returns dict(game_index i64[B], position i64[B], absorbing i64[B, unroll + 1] (zero where nothing is drawn),
    weight f32[B] or None, state = rs.get_state())."""
    n = len(lengths)
    if per:
        game_probs = np.array(game_priority, dtype="float32")
        game_probs /= np.sum(game_probs)                       # numpy's pairwise float32 sum, float32 quotients
        game_index = rs.choice(n, batch, p=game_probs)
    else:
        game_index = np.array([rs.choice(n) for _ in range(batch)], dtype=np.int64)
    position = np.zeros(batch, dtype=np.int64)
    absorbing = np.zeros((batch, unroll + 1), dtype=np.int64)
    weights = []
    for b, g in enumerate(game_index):
        length = int(lengths[g])
        if per:
            row = priorities[g]
            assert row.dtype == np.float32 and len(row) == length
            position_probs = row / sum(row)                    # Python's sum over float32 scalars, left to right
            position[b] = rs.choice(length, p=position_probs)
            weights.append(1 / (total_samples * game_probs[g] * position_probs[position[b]]))
        else:
            position[b] = rs.choice(length)
        for u in range(unroll + 1):                            # make_target: a random action per step past the end
            if position[b] + u > length:
                absorbing[b, u] = rs.choice(num_actions)
    weight = np.array(weights, dtype="float32") / max(weights) if per else None
    return dict(game_index=np.asarray(game_index, dtype=np.int64), position=position, absorbing=absorbing, weight=weight,
                state=rs.get_state())


class ModelStore:
    """The games a replay ring holds, as plain Python: ids run from 0, the oldest leave when the ring is full."""

    def __init__(self, capacity):
        self.capacity = int(capacity)
        self.first_id = 0               # id of the oldest stored game
        self.lengths, self.priorities, self.game_priority = [], [], []

    def __len__(self):
        return len(self.lengths)

    @property
    def total_samples(self):
        return int(sum(self.lengths))

    def add(self, rows):
        """rows: float32 priorities of each new game (its length is the row's)."""
        for row in rows:
            row = np.array(row, dtype=np.float32)
            self.lengths.append(len(row))
            self.priorities.append(row)
            self.game_priority.append(np.max(row))
        extra = len(self.lengths) - self.capacity
        if extra > 0:
            del self.lengths[:extra], self.priorities[:extra], self.game_priority[:extra]
            self.first_id += extra

    def load(self, game_id, row):
        g = game_id - self.first_id
        row = np.array(row, dtype=np.float32)
        assert len(row) == self.lengths[g]
        self.priorities[g], self.game_priority[g] = row, np.max(row)

    def snapshot(self):
        """(game_priority, lengths, priorities, total_samples) as they stand: later updates leave them alone."""
        return (np.array(self.game_priority, dtype=np.float32), np.array(self.lengths, dtype=np.int64),
                list(self.priorities), self.total_samples)

    def update(self, game_ids, positions, fresh):
        """update_priorities as the sequential loop it is: batch order, rows clipped at the end of the game, games that
        have left skipped, the game priority the maximum of what the game then holds.  Returns the touched ids."""
        touched = []
        for i in range(len(game_ids)):
            g = int(game_ids[i]) - self.first_id
            if g < 0:
                continue
            row = self.priorities[g].copy()
            end = min(int(positions[i]) + fresh.shape[1], len(row))
            row[int(positions[i]): end] = fresh[i, : end - int(positions[i])]
            self.priorities[g], self.game_priority[g] = row, np.max(row)
            touched.append(int(game_ids[i]))
        return touched
