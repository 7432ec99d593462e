"""Host time of the end of a device-input move batch, phase by phase, with the GPU already idle (so no phase's time is a
wait for kernels): what a single-group DeviceSelfPlay.play_moves exposes per batch.

    python tools/batch_end_phases.py [game=tictactoe] [envs=65536] [moves=20]"""
import importlib, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
sp = importlib.import_module("muzero-hypermodel_amd.self_play")
models = importlib.import_module("muzero-hypermodel_amd.models")
game = sys.argv[1] if len(sys.argv) > 1 else "tictactoe"
E = int(sys.argv[2]) if len(sys.argv) > 2 else 65536
M = int(sys.argv[3]) if len(sys.argv) > 3 else 20
config = importlib.import_module(f"muzero-hypermodel_amd.games.{game}").MuZeroConfig()
torch.manual_seed(0)
actor = sp.DeviceSelfPlay({"weights": models.MuZeroNetwork(config).get_weights()}, game, config, 0, E)
games = [0]
cb = dict(on_games=lambda b: games.__setitem__(0, games[0] + len(b)))
for _ in range(3):
    actor.play_moves(M, 1.0, **cb)
phases = {}
def add(name, seconds):
    phases[name] = phases.get(name, 0.0) + seconds
def timed(name, fn):
    def call(*args, **kwargs):
        t = time.perf_counter()
        try:
            return fn(*args, **kwargs)
        finally:
            add(name, time.perf_counter() - t)
    return call
def batch_end():
    """The actor's own _device_batch_end, with the calls it makes timed where it makes them."""
    eng = actor.engine
    inside = {"flush previous batch": (actor, "flush"), "moves_collect": (eng, "moves_collect"), "moves_inputs": (eng, "moves_inputs")}
    before = sum(phases.get(k, 0.0) for k in inside)
    for name, (owner, method) in inside.items():
        setattr(owner, method, timed(name, getattr(owner, method)))
    t = time.perf_counter()
    try:
        actor._device_batch_end(None, cb["on_games"])
    finally:
        whole = time.perf_counter() - t
        for owner, method in inside.values():
            delattr(owner, method)
    # what is left: the last to_play download, the copy stream's wait, the to_play arrays, the unfiled batch's record
    add("rest of batch end", whole - (sum(phases.get(k, 0.0) for k in inside) - before))
reps = 4
for _ in range(reps):
    timed("begin", actor._device_batch_begin)(M, 1.0, None, cb["on_games"], config.temperature_threshold)
    t = time.perf_counter()
    for m in range(M):
        actor._device_batch_move(m)
    add("enqueue moves (host)", time.perf_counter() - t)
    timed("gpu wait", torch.cuda.synchronize)()
    batch_end()
actor.flush(**cb)
print(json.dumps({"game": game, "envs": E, "moves_per_batch": M, "ms_per_batch": {k: round(1e3 * v / reps, 2) for k, v in phases.items()}}))
actor.close()
