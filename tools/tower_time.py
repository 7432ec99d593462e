"""Time of one recurrent-inference tower launch (all 3x3 convolutions of the dynamics and prediction networks) for a
game's network at a given batch, from a hipGraph of 10 launches; environment variables select kernel variants
(MZ_TOWER_COLS=off: the row-tile kernel for 3x3 boards; MZ_BOARD_CONV_PRECISION=fp32; MZ_SPLIT_FALLBACK=off).

    python tools/tower_time.py [game=tictactoe] [batch=65536]        -> one JSON line
    python tools/tower_time.py wide-layer [batch=256]                -> one JSON line

wide-layer: Gomoku's two layer shapes on 11 x 11 boards -- 129 -> 128 (the dynamics input) and 128 -> 128 with a skip --
through mzmcts_board_conv_wide and through the path it replaces (torch's convolution + mzmcts_affine_act), 20 eager
launches of each after a warm-up (what a `rocprofv3 --kernel-trace --stats` run averages per kernel name) and the time
per layer from events around them."""
import importlib, json, os, sys, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")]
from parity_helpers import synthetic_model
game = sys.argv[1] if len(sys.argv) > 1 else "tictactoe"
b = int(sys.argv[2]) if len(sys.argv) > 2 else (256 if game == "wide-layer" else 65536)
models = importlib.import_module("muzero-hypermodel_amd.models")
if game == "wide-layer":
    torch.manual_seed(0)
    result = {"mode": game, "batch": b}
    with torch.no_grad():
        for name, cin, skip in (("129->128", 129, False), ("128->128+skip", 128, True)):
            conv, bn = models.conv3x3(cin, 128).cuda().eval(), models.BatchNorm2d(128).cuda().eval()
            x = torch.rand(b, cin, 11, 11, device="cuda")
            res = torch.rand(b, 128, 11, 11, device="cuda") if skip else None
            for path in ("wide", "torch"):
                os.environ["MZ_BOARD_CONV_WIDE"] = "on" if path == "wide" else "off"
                assert conv.takes_wide_path(x) == (path == "wide")
                run = (lambda: conv.fused(x, bn, residual=res)) if path == "wide" else (lambda: models.conv_epilogue(conv(x), bn, residual=res))
                for _ in range(5):
                    run()
                torch.cuda.synchronize()
                a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(20):
                    run()
                e.record(); torch.cuda.synchronize()
                result[f"{name} {path}_us"] = 1e3 * a.elapsed_time(e) / 20
    result["algorithmic_TFLOPs_128_wide"] = 2 * 9 * 121 * 128 * 128 * b / result["128->128+skip wide_us"] / 1e6
    print(json.dumps(result))
    sys.exit(0)
engine = importlib.import_module("muzero-hypermodel_amd.engine")
if game == "atari84":
    config = importlib.import_module("muzero-hypermodel_amd.games.breakout").atari84_config()
else:
    config = importlib.import_module(f"muzero-hypermodel_amd.games.{game}").MuZeroConfig()
model, _ = synthetic_model(models, config, "cuda")
c, h, w = engine.hidden_state_shape(config)
A = len(config.action_space)
state = torch.rand(b, c, h, w, device="cuda")
action = torch.randint(0, A, (b, 1), device="cuda")
planes = models.state_action_planes(state, action, A)
with torch.no_grad():
    for _ in range(3):
        assert model._recurrent_tower(planes, None) is not None
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(10):
            model._recurrent_tower(planes, None)
    g.replay(); torch.cuda.synchronize()
    a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(5):
        g.replay()
    e.record(); torch.cuda.synchronize()
us = 1e3 * a.elapsed_time(e) / 50
layers = 1 + 4 * config.blocks
flops = 2 * 9 * h * w * c * (c + 1 + (layers - 1) * c) * b          # direct-convolution count, every tap at every position
print(json.dumps({"game": game, "batch": b, "tower_us": us, "algorithmic_TFLOPs": flops / us / 1e6,
                  "env": {k: os.environ.get(k) for k in ("MZ_TOWER_COLS", "MZ_BOARD_CONV_PRECISION", "MZ_SPLIT_FALLBACK") if os.environ.get(k)}}))
