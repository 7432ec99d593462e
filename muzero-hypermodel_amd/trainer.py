"""Trainer with the reference's interface (trainer.py:11-298), SURVEY.md section 8(f) row 4: the unroll that
turns a replay batch into a gradient step, and the producer side of the weight hand-over to the actors.

The arithmetic is PyTorch-ROCm (fp32, the reference's operation order) -- or, for fully-connected networks with
Trainer(fc_step=True), four HIP launches per step (include/mztrain.h mztrain_fc_*), with fc_optimizer=True the optimizer as
a HIP launch too (mztrain_opt_step), and for residual networks with Trainer(native_epilogue=True) every
relu(batch_norm(x) [+ residual]) as one HIP launch each way (mztrain_epilogue_*), with Trainer(native_conv=True) their 3 x 3
convolutions and both gradients as HIP launches (mztrain_conv_*), with Trainer(native_heads=True) their reward, value and
policy heads as HIP launches (mztrain_heads_*), with Trainer(native_rescale=True) the hidden state's min-max rescale as one
HIP launch each way (mzmcts_unit_rescale, mztrain_rescale_backward), with Trainer(native_optimizer=True) the weight gradients
of all uses of a parameter folded and Adam or SGD applied in one HIP launch (mztrain_fold_step); what changes is the plumbing
around it:
batches arrive as CUDA tensors from the device replay store (replay_buffer.ReplayBuffer.get_batch) and never
visit the host, the new priorities are computed on the device and copied back once per step, and fresh weights
leave through `publish` into the flat buffer the actors alias (weights.FlatWeights) -- one RCCL broadcast
instead of a state_dict through shared storage.

There is one training step, Trainer._queue_step: produce the gradients, step the optimizer, build the report of the four
losses.  Three things produce gradients -- the four fc_step launches (_fc_queue), autograd under the loss launch
(_loss_native) and autograd under the torch expression (_loss_torch: on the CPU, or with native_loss = False) -- and
update_weights, train_steps and graph mode's warm-up and capture (_capture) all run that one body; _step replays a
captured one.  A non-zero status of a mztrain_* call is raised by _native.check_train.
"""
import copy
import ctypes
import time
import weakref

import numpy
import torch

from . import _native, models


def _scale_gradient(tensor, divisor):
    """Leaves `tensor` as it is and divides the gradient flowing back through it by `divisor` (a number or a
    per-sample tensor).  A tensor hook, not an autograd node: the graph -- and with it the order in which the
    shared parameters accumulate their gradients -- stays the reference's, which one-step Adam parity needs."""
    tensor.register_hook(lambda grad: grad / divisor)
    return tensor


def _loss_outputs(size, steps, device):
    """What a loss launch fills: per-sample loss [B], per-sample head sums [3, B], priorities [B, K+1]."""
    return (torch.empty(size, device=device), torch.empty((3, size), device=device),
            torch.empty((size, steps), device=device))


class _UnrollLoss(torch.autograd.Function):
    """The loss of one training step over all unrolled positions as ONE HIP launch (include/mztrain.h
    mztrain_unroll_loss, csrc/trainer_kernels.hip): two-hot value / reward targets, the three cross-entropies per step,
    their sums over the steps in the reference's order, the per-sample total, the new PER priorities, and -- kept for
    backward -- the gradient of the per-sample total with respect to every logit (gradient scales folded in).
    Forward returns (per-sample loss [B], per-sample head sums [3, B], priorities [B, K+1]); only the first is
    differentiable.  CUDA tensors only: on the CPU the trainer keeps the torch expression."""

    @staticmethod
    def forward(ctx, value_logits, reward_logits, policy_logits, batch, support_size, value_loss_weight, per_alpha):
        lib = _native.load()      # raises when the HIP library is missing: no silent fallback on a GPU box
        steps, size, full = value_logits.shape
        actions = policy_logits.shape[2]
        assert full == 2 * support_size + 1 and reward_logits.shape == value_logits.shape
        v, r, p = (t.detach().contiguous().float() for t in (value_logits, reward_logits, policy_logits))
        tv, tr, tp, gs = (batch[key].contiguous() for key in ("values", "rewards", "policies", "gradient_scales"))
        weight = batch["weights"].contiguous() if batch["weights"] is not None else None
        sample_loss, head_sums, priorities = _loss_outputs(size, steps, v.device)
        grads = (torch.empty_like(v), torch.empty_like(r), torch.empty_like(p))
        args = _native.MzTrainLossArgs(
            value_logits=v.data_ptr(), reward_logits=r.data_ptr(), policy_logits=p.data_ptr(), target_value=tv.data_ptr(),
            target_reward=tr.data_ptr(), target_policy=tp.data_ptr(), gradient_scale=gs.data_ptr(),
            weight=weight.data_ptr() if weight is not None else None, batch=size, steps=steps, support_size=support_size,
            actions=actions, value_loss_weight=float(value_loss_weight), per_alpha=float(per_alpha),
            sample_loss=sample_loss.data_ptr(), head_sums=head_sums.data_ptr(), priorities=priorities.data_ptr(),
            grad_value=grads[0].data_ptr(), grad_reward=grads[1].data_ptr(), grad_policy=grads[2].data_ptr())
        rc = lib.mztrain_unroll_loss(ctypes.byref(args), torch.cuda.current_stream(v.device).cuda_stream)
        _native.check_train(lib, rc, "mztrain_unroll_loss", reason=False)
        ctx.save_for_backward(*grads)
        ctx.mark_non_differentiable(head_sums, priorities)
        return sample_loss, head_sums, priorities

    @staticmethod
    def backward(ctx, grad_loss, _grad_sums, _grad_priorities):
        g = grad_loss.reshape(1, -1, 1)
        gv, gr, gp = ctx.saved_tensors
        return gv * g, gr * g, gp * g, None, None, None, None


class FlatOptimizer:
    """Adam or SGD on a fully-connected network's flat weight and gradient buffers as HIP launches (include/mztrain.h
    mztrain_opt_step, csrc/fc_optimizer.h): what Trainer(fc_step=True, fc_optimizer=True) holds in place of a torch.optim
    object.  Owns two flat moment tensors (Adam's exp_avg / SGD's momentum buffer, and Adam's exp_avg_sq), the learning
    rate as a device float64 and the count of steps done as a device int64 the launches advance.  state_dict() and
    load_state_dict() speak the format of torch.optim.Adam / torch.optim.SGD of the same configuration."""

    def __init__(self, lib, model, flat_weights, flat_grad, kind, lr, weight_decay, momentum=0.0, parameters_only=True):
        self._lib = lib
        self.kind = kind
        names = [name for name, _ in model.named_parameters()]
        if parameters_only and names != list(flat_weights.float_keys):
            raise NotImplementedError("Trainer(fc_optimizer=True): the flat buffer must hold the parameters and nothing else "
                                      "(a network with batch-norm statistics keeps torch's optimizer)")
        self._slices = [(flat_weights.offsets[name], parameter.numel(), tuple(parameter.shape))
                        for name, parameter in model.named_parameters()]
        self._weights, self._grads = flat_weights.flat, flat_grad
        device = self._weights.device
        self.n = int(flat_weights.numel)
        self.moment1 = torch.zeros(self.n, dtype=torch.float32, device=device)
        self.moment2 = torch.zeros(self.n if kind == "Adam" else 0, dtype=torch.float32, device=device)
        self.lr = torch.full((1,), float(lr), dtype=torch.float64, device=device)
        self.steps_done = torch.zeros(1, dtype=torch.int64, device=device)
        self._lr_filled = float(lr)
        # torch's own param-group keys for this configuration (nothing is allocated before a step)
        if kind == "Adam":
            template = torch.optim.Adam(model.parameters(), lr=float(lr), weight_decay=weight_decay)
        else:
            template = torch.optim.SGD(model.parameters(), lr=float(lr), momentum=momentum, weight_decay=weight_decay)
        group = dict(template.state_dict()["param_groups"][0])
        group["lr"] = float(lr)
        self.param_groups = [group]

    def zero_grad(self, set_to_none=True):
        """Nothing to do: the gradient buffer is overwritten by every step's launches."""

    def set_lr(self, lr):
        self.param_groups[0]["lr"] = float(lr)
        self.lr.fill_(float(lr))
        self._lr_filled = float(lr)

    def _opt_args(self):
        """mztrain_opt_args of this step (the learning rate is brought up to the param group's first)."""
        group = self.param_groups[0]
        if float(group["lr"]) != self._lr_filled:
            self.set_lr(group["lr"])
        adam = self.kind == "Adam"
        beta1, beta2 = group["betas"] if adam else (0.0, 0.0)
        momentum = 0.0 if adam else float(group["momentum"])
        return _native.MzTrainOptArgs(
            kind=_native.OPT_ADAM if adam else _native.OPT_SGD, n=self.n, weights=self._weights.data_ptr(),
            grads=self._grads.data_ptr(), moment1=self.moment1.data_ptr() if adam or momentum != 0.0 else None,
            moment2=self.moment2.data_ptr() if adam else None, lr=self.lr.data_ptr(), steps_done=self.steps_done.data_ptr(),
            beta1=float(beta1), beta2=float(beta2), eps=float(group["eps"]) if adam else 0.0,
            weight_decay=float(group["weight_decay"]), momentum=momentum)

    def step(self):
        args = self._opt_args()
        rc = self._lib.mztrain_opt_step(ctypes.byref(args), torch.cuda.current_stream(self._weights.device).cuda_stream)
        _native.check_train(self._lib, rc, "mztrain_opt_step")

    # ---- what a capture's warm-up puts back ---------------------------------------------------------------
    def snapshot(self):
        return self.moment1.clone(), self.moment2.clone(), self.steps_done.clone()

    def restore(self, saved):
        self.moment1.copy_(saved[0])
        self.moment2.copy_(saved[1])
        self.steps_done.copy_(saved[2])

    # ---- torch's state-dict format ------------------------------------------------------------------------
    def state_dict(self):
        done = int(self.steps_done.item())
        group = dict(self.param_groups[0])
        group["params"] = list(range(len(self._slices)))
        state = {}
        with_buffer = self.kind == "SGD" and float(group["momentum"]) != 0.0
        if done > 0 and (self.kind == "Adam" or with_buffer):
            for index, (at, count, shape) in enumerate(self._slices):
                first = self.moment1[at: at + count].view(shape).clone()
                if self.kind == "Adam":
                    state[index] = {"step": torch.tensor(float(done), dtype=torch.float32), "exp_avg": first,
                                    "exp_avg_sq": self.moment2[at: at + count].view(shape).clone()}
                else:
                    state[index] = {"momentum_buffer": first}
        return {"state": state, "param_groups": [group]}

    def load_state_dict(self, state_dict, steps_hint=0):
        """Takes torch's state dict, one without state and an SGD one without momentum buffers included.  SGD's state holds
        no step count: where it holds momentum buffers, the count becomes `steps_hint` (at least 1)."""
        groups = state_dict["param_groups"]
        if len(groups) != 1 or len(groups[0]["params"]) != len(self._slices):
            raise ValueError("FlatOptimizer.load_state_dict: one parameter group over the model's parameters is expected")
        saved = groups[0]
        if saved.get("amsgrad") or saved.get("maximize") or saved.get("nesterov") or saved.get("dampening") \
                or saved.get("decoupled_weight_decay"):
            raise ValueError("FlatOptimizer.load_state_dict: amsgrad, maximize, nesterov, dampening and decoupled weight "
                             "decay are not what mztrain_opt_step computes")
        group = self.param_groups[0]
        for key in ("lr", "betas", "eps", "weight_decay", "momentum"):
            if key in group and key in saved:
                value = saved[key]
                group[key] = tuple(float(v) for v in value) if key == "betas" else float(value)
        self.set_lr(group["lr"])
        self.moment1.zero_()
        self.moment2.zero_()
        done = 0
        for index, entry in state_dict["state"].items():
            at, count, shape = self._slices[saved["params"].index(index)]
            names = ("exp_avg", "exp_avg_sq") if self.kind == "Adam" else ("momentum_buffer",)
            for name, flat in zip(names, (self.moment1, self.moment2)):
                value = entry.get(name)
                if value is not None:
                    flat[at: at + count].copy_(torch.as_tensor(value).reshape(-1))
            if "step" in entry:
                done = max(done, int(float(entry["step"])))
            elif self.kind == "SGD" and entry.get("momentum_buffer") is not None:
                done = max(done, int(steps_hint), 1)
        self.steps_done.fill_(done)


class FoldOptimizer(FlatOptimizer):
    """FlatOptimizer for a residual network under Trainer(native_optimizer=True): the flat buffers hold the batch-norm
    statistics beside the parameters, the HIP training Functions write every use's weight gradient into a slot of one staging
    buffer (models.GradientSink), and step() queues ONE launch that folds each parameter's slots in autograd's order into the
    flat gradient buffer and applies Adam or SGD to exactly the parameters (include/mztrain.h mztrain_fold_step,
    csrc/grad_fold.h).  Moments, learning rate, step count and torch's state-dict format are the base class's."""

    def __init__(self, lib, model, flat_weights, flat_grad, kind, lr, weight_decay, momentum, capacity):
        super().__init__(lib, model, flat_weights, flat_grad, kind, lr, weight_decay, momentum=momentum, parameters_only=False)
        device = self._weights.device
        self._device = device if device.index is not None else torch.device("cuda", torch.cuda.current_device())
        names = [name for name, _ in model.named_parameters()]
        segments = (_native.MzTrainFoldSegment * len(names))()
        total = 0
        for index, (at, count, _) in enumerate(self._slices):
            stride = -(-count // _native.FOLD_SLOT_ALIGN) * _native.FOLD_SLOT_ALIGN
            segments[index] = _native.MzTrainFoldSegment(offset=at, count=count, slot_base=total, slot_stride=stride,
                                                         capacity=capacity)
            total += stride * capacity
        self.segments = segments
        self.staging = torch.zeros(total, dtype=torch.float32, device=device)
        views = [[self.staging[s.slot_base + k * s.slot_stride: s.slot_base + k * s.slot_stride + s.count].view(shape)
                  for k in range(capacity)] for s, (_, _, shape) in zip(segments, self._slices)]
        self.sink = models.GradientSink(names, views)
        self.uploaded_uses = None
        handle = ctypes.c_void_p()
        with torch.cuda.device(self._device):
            rc = lib.mztrain_fold_create(segments, len(names), self.n, total, self._device.index, ctypes.byref(handle))
        _native.check_train(lib, rc, "mztrain_fold_create", refusal="Trainer(native_optimizer=True)")
        self._live = [handle]
        weakref.finalize(self, self._destroy, lib, self._live, self._device)

    @staticmethod
    def _destroy(lib, live, device):
        if live[0] is not None:
            torch.cuda.synchronize(device)
            lib.mztrain_fold_destroy(live[0])
            live[0] = None

    def set_uses(self, uses):
        """Upload the slots written per parameter; synchronous, not for a capture."""
        uses = [int(u) for u in uses]
        with torch.cuda.device(self._device):
            rc = self._lib.mztrain_fold_set_uses(self._live[0], (ctypes.c_int32 * len(uses))(*uses), len(uses))
        _native.check_train(self._lib, rc, "mztrain_fold_set_uses")
        self.uploaded_uses = uses

    def step(self):
        args = _native.MzTrainFoldArgs(opt=self._opt_args(), staging=self.staging.data_ptr(),
                                       staging_floats=self.staging.numel())
        with torch.cuda.device(self._device):
            rc = self._lib.mztrain_fold_step(self._live[0], ctypes.byref(args),
                                             torch.cuda.current_stream(self._device).cuda_stream)
        _native.check_train(self._lib, rc, "mztrain_fold_step")


class Trainer:
    native_loss = True      # on the GPU: the loss of a step as one HIP launch (False: the torch expression, for timing)

    def __init__(self, initial_checkpoint, config, device=None, graph=False, fc_step=False, fc_optimizer=False,
                 native_epilogue=False, native_conv=False, native_heads=False, native_rescale=False, native_optimizer=False):
        """The flags choose what produces a step's gradients and what applies them; the step itself is one (_queue_step).

        graph=True (GPU, Adam): the whole step -- unroll, loss launch, backward, optimizer -- is captured into a
        hipGraph at the first update_weights and replayed afterwards (the step is launch-bound: ~1 500 launches of
        microsecond kernels for the CartPole network); batches are copied into the capture's static buffers.

        fc_step=True (GPU, fully-connected networks): forward, loss, backward and weight gradients are four HIP launches
        (include/mztrain.h mztrain_fc_step) that differentiate the arithmetic the search evaluates; the parameters are
        views of one flat buffer (weights.FlatWeights, `self.flat_weights`), every p.grad a view of one flat gradient buffer
        the launches overwrite whole, and the optimizer stays torch's.  Combines with graph=True.

        fc_optimizer=True (with fc_step=True): the optimizer is a HIP launch on the two flat buffers too (FlatOptimizer,
        include/mztrain.h mztrain_opt_step), Adam or SGD; the step is HIP launches only, eager and captured steps give the
        same bits, graph=True takes SGD as well, and checkpoints keep torch's optimizer format.

        native_epilogue=True (GPU, residual networks): every relu(batch_norm(x) [+ residual]) of the network in training is
        one HIP launch forward and one backward (include/mztrain.h mztrain_epilogue_*, models._TrainingEpilogue) instead of
        torch's batch norm, add and ReLU with their autograd nodes; convolutions, heads and the optimizer stay torch's.
        Combines with graph=True; checkpoints, publish and update_lr are untouched.

        native_conv=True (GPU, residual networks): every 3 x 3 convolution the launches cover (boards 3 x 3, 6 x 6, 6 x 7; 16
        or 64 output channels; stride 1) runs its forward, data gradient and weight gradient as HIP launches (include/mztrain.h
        mztrain_conv_*, models._TrainingConv3x3) instead of the convolution library's; every step first queues one pack
        launch per such module, so a captured step repacks on replay.  Other convolutions stay torch's.  Combines with
        native_epilogue, graph=True and train_steps.

        native_heads=True (GPU, residual networks): every reward, value and policy head the launches cover (one hidden
        layer, ELU with alpha 1, a convolution bias) runs as one HIP launch forward per call and two backward
        (include/mztrain.h mztrain_heads_*, models._TrainingHeads) instead of the torch modules with their autograd nodes;
        value and policy share a call.  Other heads stay torch's.  Combines with native_epilogue, native_conv, graph=True and
        train_steps.

        native_rescale=True (GPU, residual networks, hidden-state planes of at most 128 positions): the per-plane min-max
        rescale of the hidden state, after the representation network and after every dynamics step, runs the inference
        launch forward and one HIP launch backward (include/mztrain.h mztrain_rescale_backward, models._TrainingRescale)
        instead of torch's eight launches with their autograd nodes; ties at a plane's minimum or maximum share the gradient
        evenly, as torch's amin and amax do.  Combines with native_epilogue, native_conv, native_heads, graph=True and
        train_steps.

        native_optimizer=True (with native_epilogue, native_conv and native_heads; every parameter must belong to a module
        they cover): the parameters and batch-norm statistics live in one flat buffer (`self.flat_weights`), every use's weight
        gradient is written into a slot of one staging buffer instead of being summed into p.grad by one launch per
        parameter and use, and ONE HIP launch per step folds the slots in autograd's order and applies Adam or SGD
        (FoldOptimizer, include/mztrain.h mztrain_fold_step).  The folded gradients are bit for bit the four-flag trainer's
        (`gradients()`), eager and captured steps give the same bits, graph=True takes SGD as well, and checkpoints keep
        torch's optimizer format.  p.grad stays None; a call that falls back to torch's path raises after the backward."""
        if fc_optimizer and not fc_step:
            raise NotImplementedError("Trainer(fc_optimizer=True) updates the flat buffers of Trainer(fc_step=True): pass "
                                      "fc_step=True as well")
        self.config = config
        self._fc = None
        self._graph_mode = bool(graph)
        self._graph = None
        numpy.random.seed(self.config.seed)
        torch.manual_seed(self.config.seed)
        self.model = models.MuZeroNetwork(self.config)
        self.model.set_weights(copy.deepcopy(initial_checkpoint["weights"]))
        device = torch.device(device if device is not None else "cuda" if self.config.train_on_gpu else "cpu")
        self.model.to(device)
        self.model.train()
        self._fold = None
        if native_optimizer:
            missing = [name for name, on in (("native_epilogue", native_epilogue), ("native_conv", native_conv),
                                             ("native_heads", native_heads)) if not on]
            if missing:
                raise NotImplementedError(f"Trainer(native_optimizer=True) folds the gradients the HIP training launches "
                                          f"write: pass {', '.join(name + '=True' for name in missing)} as well")
            if self.config.network != "resnet":
                raise NotImplementedError(f"Trainer(native_optimizer=True) folds the gradients of residual networks; "
                                          f"config.network is {self.config.network!r}")
            if device.type != "cuda":
                raise NotImplementedError(f"Trainer(native_optimizer=True) runs HIP kernels: the model must be on the GPU, "
                                          f"not on {device}")
            if fc_step:
                raise NotImplementedError("Trainer(native_optimizer=True) is the residual networks' way; fc_step=True has "
                                          "fc_optimizer=True")
        # each flag's refusals stand at the head of what sets it up, in this order: native_epilogue, native_conv, native_heads,
        # native_rescale, fc_step
        # (_fc_setup), then the optimizer's and graph's (_make_optimizer)
        if native_epilogue:
            if self.config.network != "resnet":
                raise NotImplementedError(f"Trainer(native_epilogue=True) fuses the batch norms of residual networks; "
                                          f"config.network is {self.config.network!r}")
            if device.type != "cuda":
                raise NotImplementedError(f"Trainer(native_epilogue=True) runs HIP kernels: the model must be on the GPU, "
                                          f"not on {device}")
            self.model.native_training_epilogue(True)
        self._native_norms = [m for m in self.model.modules() if isinstance(m, models.BatchNorm2d)] if native_epilogue else []
        self._native_conv = bool(native_conv)
        if native_conv:
            if self.config.network != "resnet":
                raise NotImplementedError(f"Trainer(native_conv=True) runs the 3 x 3 convolutions of residual networks; "
                                          f"config.network is {self.config.network!r}")
            if not any(isinstance(m, models.BoardConv2d) and m.training_covered() for m in self.model.modules()):
                raise NotImplementedError("Trainer(native_conv=True) found no 3 x 3 convolution its launches cover (16 or 64 "
                                          "output channels, at most 80 input channels, stride 1) in this network")
            if device.type != "cuda":
                raise NotImplementedError(f"Trainer(native_conv=True) runs HIP kernels: the model must be on the GPU, "
                                          f"not on {device}")
            self.model.native_training_conv(True)
        if native_heads:
            if self.config.network != "resnet":
                raise NotImplementedError(f"Trainer(native_heads=True) runs the heads of residual networks; "
                                          f"config.network is {self.config.network!r}")
            if not any(models._head_covered(conv, fc) for conv, fc in self.model.training_heads()):
                raise NotImplementedError("Trainer(native_heads=True) found no head its launches cover (one hidden layer, "
                                          "ELU with alpha 1, a convolution bias, at most 256 channels, 128 positions, 16 "
                                          "reduced channels, 128 hidden units and 256 outputs) in this network")
            if device.type != "cuda":
                raise NotImplementedError(f"Trainer(native_heads=True) runs HIP kernels: the model must be on the GPU, "
                                          f"not on {device}")
            self.model.native_training_heads(True)
        if native_rescale:
            if self.config.network != "resnet":
                raise NotImplementedError(f"Trainer(native_rescale=True) runs the hidden-state rescale of residual networks; "
                                          f"config.network is {self.config.network!r}")
            if self.model.hidden_plane > 128:
                raise NotImplementedError(f"Trainer(native_rescale=True) covers hidden-state planes of at most 128 positions; "
                                          f"this network's have {self.model.hidden_plane}")
            if device.type != "cuda":
                raise NotImplementedError(f"Trainer(native_rescale=True) runs HIP kernels: the model must be on the GPU, "
                                          f"not on {device}")
            self.model.native_training_rescale(True)
        if native_optimizer:
            owned = set(self.model.training_owned_parameters())
            for name, _ in self.model.named_parameters():
                if name not in owned:
                    raise NotImplementedError(f"Trainer(native_optimizer=True): no HIP training launch covers the module of "
                                              f"parameter {name}, its gradient would stay with autograd")
            self._fold_setup(device)    # before the optimizer, like fc_step
        if fc_step:
            self._fc_setup(device)      # before the optimizer: it must hold the re-pointed parameters
        self.training_step = initial_checkpoint["training_step"]
        self._fc_opt = bool(fc_optimizer) or bool(native_optimizer)      # the optimizer is a FlatOptimizer
        self.optimizer = self._make_optimizer(device)
        self._lr_host = float(self.config.lr_init)
        if initial_checkpoint.get("optimizer_state") is not None:
            self._load_optimizer_state(initial_checkpoint["optimizer_state"])

    def _make_optimizer(self, device):
        """FlatOptimizer (fc_optimizer=True), or torch's SGD / Adam -- in graph mode the capturable Adam."""
        cfg = self.config
        if cfg.optimizer not in ("SGD", "Adam"):
            raise NotImplementedError(
                f"{cfg.optimizer} is not implemented. You can change the optimizer manually in trainer.py.")
        if self._graph_mode and not self._fc_opt and (cfg.optimizer != "Adam" or device.type != "cuda"):
            raise NotImplementedError("Trainer(graph=True) captures an Adam step on the GPU")
        if self._fold:
            optimizer = FoldOptimizer(self._fc_lib, self.model, self.flat_weights, self._flat_grad, cfg.optimizer, cfg.lr_init,
                                      cfg.weight_decay, cfg.momentum if cfg.optimizer == "SGD" else 0.0,
                                      capacity=int(cfg.num_unroll_steps) + 1)
            self.model.install_gradient_sink(optimizer.sink)
            return optimizer
        if self._fc_opt:
            return FlatOptimizer(self._fc_lib, self.model, self.flat_weights, self._flat_grad, cfg.optimizer, cfg.lr_init,
                                 cfg.weight_decay, momentum=cfg.momentum if cfg.optimizer == "SGD" else 0.0)
        if cfg.optimizer == "SGD":
            return torch.optim.SGD(self.model.parameters(), lr=cfg.lr_init, momentum=cfg.momentum,
                                   weight_decay=cfg.weight_decay)
        if not self._graph_mode:
            return torch.optim.Adam(self.model.parameters(), lr=cfg.lr_init, weight_decay=cfg.weight_decay)
        # step counter and learning rate live on the device, so a replay can move them
        self._lr = torch.tensor(float(cfg.lr_init), device=device)
        return torch.optim.Adam(self.model.parameters(), lr=self._lr, capturable=True, weight_decay=cfg.weight_decay)

    def _load_optimizer_state(self, state):
        """A checkpoint's optimizer state, eager or graphed, torch's or FlatOptimizer's (they share a format)."""
        portable = copy.deepcopy(self._portable_optimizer_state(state))
        if self._fc_opt:
            self.optimizer.load_state_dict(portable, steps_hint=self.training_step)
        else:
            self.optimizer.load_state_dict(portable)
        self._lr_host = float(self.optimizer.param_groups[0]["lr"])
        if self._graph_mode and not self._fc_opt:
            # load_state_dict replaced every param group's settings with the checkpoint's: put the device-resident
            # learning rate and the capturable flag back (an eager checkpoint carries a float lr, capturable False and
            # CPU step counters; a graphed one a tensor lr), or update_lr() would fill an orphaned tensor and the
            # capture of optimizer.step() would break / bake the learning rate in
            self._lr.fill_(self._lr_host)
            for group in self.optimizer.param_groups:
                group["lr"], group["capturable"] = self._lr, True
            for entry in self.optimizer.state.values():
                if "step" in entry:
                    entry["step"] = torch.as_tensor(entry["step"], dtype=torch.float32).to(self._lr.device).reshape(())

    # ---- gradients folded and the optimizer applied in one launch (include/mztrain.h mztrain_fold_*) -------
    def _fold_setup(self, device):
        """Parameters and batch-norm statistics into one flat buffer, and a flat gradient buffer indexed like it."""
        from . import weights
        self._fc_lib = _native.load()
        self.flat_weights = weights.FlatWeights(self.model)
        self._flat_grad = torch.zeros(self.flat_weights.numel, dtype=torch.float32, device=device)
        self._fold = True

    def _fold_after_backward(self):
        """What the host checks after every backward Python runs (eager, warm-up, capture): no gradient went to autograd,
        and the slots written are the ones the launch will read."""
        for name, parameter in self.model.named_parameters():
            if parameter.grad is not None:
                raise NotImplementedError(f"Trainer(native_optimizer=True): the gradient of {name} came through autograd -- a "
                                          f"call of its module fell back to torch's path; the fold launch would lose it")
        uses = list(self.optimizer.sink.arrivals)
        if uses != self.optimizer.uploaded_uses:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("Trainer(native_optimizer=True): the uses of the parameters changed while a capture is "
                                   f"open ({self.optimizer.uploaded_uses} -> {uses})")
            if self._graph is not None:
                raise RuntimeError("Trainer(native_optimizer=True): the captured step was recorded with other uses")
            self.optimizer.set_uses(uses)

    def _fold_mark_moved(self):
        """The fold launch writes the parameters through raw pointers: move their version counters on the host (no launch),
        so that every inference cache keyed by them (folded batch norms, packed and expanded convolutions) is rebuilt on its
        next use, as after a step of torch's optimizer."""
        for parameter in self.model.parameters():
            torch.autograd.graph.increment_version(parameter)

    def gradients(self):
        """{name: view into the flat gradient buffer}: the folded gradients of the last step (native_optimizer=True)."""
        if not self._fold:
            raise NotImplementedError("Trainer.gradients() reads the flat gradient buffer of Trainer(native_optimizer=True)")
        return {name: self._flat_grad[self.flat_weights.offsets[name]: self.flat_weights.offsets[name] + p.numel()].view(p.shape)
                for name, p in self.model.named_parameters()}

    # ---- the fully-connected step as HIP launches (include/mztrain.h mztrain_fc_*) -------------------------
    def _fc_setup(self, device):
        from . import weights
        cfg = self.config
        if cfg.network != "fullyconnected":
            raise NotImplementedError(f"Trainer(fc_step=True) differentiates fully-connected networks; config.network is "
                                      f"{cfg.network!r}")
        if device.type != "cuda":
            raise NotImplementedError(f"Trainer(fc_step=True) runs HIP kernels: the model must be on the GPU, not on {device}")
        layers = (cfg.fc_representation_layers, cfg.fc_dynamics_layers, cfg.fc_reward_layers, cfg.fc_policy_layers,
                  cfg.fc_value_layers)
        if any(len(widths) > 3 for widths in layers):
            raise NotImplementedError("Trainer(fc_step=True): layer sizes outside the supported range (<= 3 hidden layers "
                                      "per MLP, widths <= 256)")
        c, h, w = cfg.observation_shape
        desc = _native.MzFcDesc()
        desc.observation_floats = c * h * w * (cfg.stacked_observations + 1) + cfg.stacked_observations * h * w
        desc.encoding_size = int(cfg.encoding_size)
        for i, widths in enumerate(layers):
            desc.n_hidden[i] = len(widths)
            for k, width in enumerate(widths):
                desc.hidden[i][k] = int(width)
        self._fc_lib = _native.load()
        self._fc_desc = desc
        self._fc_device = device if device.index is not None else torch.device("cuda", torch.cuda.current_device())
        self.flat_weights = weights.FlatWeights(self.model)
        self._flat_grad = torch.zeros(self.flat_weights.numel, dtype=torch.float32, device=device)
        for name, parameter in self.model.named_parameters():
            at = self.flat_weights.offsets[name]
            parameter.grad = self._flat_grad[at: at + parameter.numel()].view(parameter.shape)
        self._fc_max = (0, 0)
        self._fc_live = [None]
        weakref.finalize(self, self._fc_destroy, self._fc_lib, self._fc_live, self._fc_device)
        self._fc_handle(int(cfg.batch_size), int(cfg.num_unroll_steps) + 1)

    def _fc_handle(self, batch, steps):
        """The handle, made again (outside any capture) when a batch is larger than the one it was sized for."""
        if self._fc is not None and batch <= self._fc_max[0] and steps <= self._fc_max[1]:
            return self._fc
        if self._graph is not None:
            raise RuntimeError("Trainer(fc_step=True, graph=True): the captured step was sized for a smaller batch")
        batch, steps = max(batch, self._fc_max[0]), max(steps, self._fc_max[1])
        handle = ctypes.c_void_p()
        with torch.cuda.device(self._fc_device):
            rc = self._fc_lib.mztrain_fc_create(
                ctypes.byref(self._fc_desc), len(self.config.action_space), int(self.config.support_size),
                self.flat_weights.flat.data_ptr(), self.flat_weights.numel, self._flat_grad.data_ptr(), batch, steps,
                self._fc_device.index, ctypes.byref(handle))
        _native.check_train(self._fc_lib, rc, "mztrain_fc_create", refusal="Trainer(fc_step=True)")
        self._fc_release()
        self._fc, self._fc_max = handle, (batch, steps)
        self._fc_live[0] = handle
        return handle

    def _fc_release(self):
        self._fc_destroy(self._fc_lib, self._fc_live, self._fc_device)
        self._fc = None

    @staticmethod
    def _fc_destroy(lib, live, device):
        """Free the handle in `live` (a one-entry list, so that the finalizer registered in _fc_setup sees a handle made
        later without holding the trainer)."""
        if live[0] is not None:
            torch.cuda.synchronize(device)
            lib.mztrain_fc_destroy(live[0])
            live[0] = None

    def _fc_queue(self, b):
        """Queue forward, loss, backward and weight gradients of batch `b` on the current stream: the flat gradient buffer
        is overwritten whole.  Returns (per-sample loss [B], head sums [3, B], priorities [B, K+1]) as device tensors."""
        values = b["values"]
        size, steps = values.shape
        handle = self._fc_handle(size, steps)
        dev = values.device
        obs = b["observations"].reshape(size, -1).contiguous().float()
        actions = b["actions"].reshape(size, steps).contiguous()
        assert actions.dtype == torch.int64 and obs.shape[1] == self._fc_desc.observation_floats
        tv, tr, tp, gs = (b[key].contiguous() for key in ("values", "rewards", "policies", "gradient_scales"))
        weight = b["weights"].contiguous() if b["weights"] is not None else None
        sample_loss, head_sums, priorities = _loss_outputs(size, steps, dev)
        args = _native.MzTrainFcArgs(
            observations=obs.data_ptr(), actions=actions.data_ptr(), target_value=tv.data_ptr(), target_reward=tr.data_ptr(),
            target_policy=tp.data_ptr(), gradient_scale=gs.data_ptr(),
            weight=weight.data_ptr() if weight is not None else None, batch=size, steps=steps,
            value_loss_weight=float(self.config.value_loss_weight), per_alpha=float(self.config.PER_alpha),
            sample_loss=sample_loss.data_ptr(), head_sums=head_sums.data_ptr(), priorities=priorities.data_ptr())
        rc = self._fc_lib.mztrain_fc_step(handle, ctypes.byref(args), torch.cuda.current_stream(dev).cuda_stream)
        _native.check_train(self._fc_lib, rc, "mztrain_fc_step")
        return sample_loss, head_sums, priorities

    @staticmethod
    def _portable_optimizer_state(state):
        """An optimizer state dict whose param groups hold plain numbers (a graphed trainer's learning rate is a device
        tensor shared by every group: a checkpoint must not alias it)."""
        out = dict(state)
        out["param_groups"] = [{k: (float(v) if torch.is_tensor(v) and v.numel() == 1 and k == "lr" else v)
                                for k, v in group.items()} for group in state["param_groups"]]
        return out

    def optimizer_state(self):
        """optimizer.state_dict() on the CPU with a float learning rate: what goes into a checkpoint (trainer.py:87-95)."""
        return copy.deepcopy(models.dict_to_cpu(self._portable_optimizer_state(self.optimizer.state_dict())))

    # ---- the loop (trainer.py:62-122) without Ray ----------------------------------------------------
    def continuous_update_weights(self, replay_buffer, shared_storage, max_steps=None):
        while shared_storage.get_info("num_played_games") < 1:
            time.sleep(0.1)
        done = 0
        while self.training_step < self.config.training_steps and not shared_storage.get_info("terminate"):
            if getattr(replay_buffer, "device_sampling", False):
                # one host synchronisation per step here (the losses are published after every step, as in the
                # reference); callers that want none between checkpoints call train_steps(replay_buffer, n) themselves
                total_loss, value_loss, reward_loss, policy_loss = self.train_steps(replay_buffer, 1)
            else:
                index_batch, batch = replay_buffer.get_batch()
                self.update_lr()
                priorities, total_loss, value_loss, reward_loss, policy_loss = self.update_weights(batch)
                if self.config.PER:
                    replay_buffer.update_priorities(priorities, index_batch)
            if self.training_step % self.config.checkpoint_interval == 0:
                shared_storage.set_info({"weights": copy.deepcopy(self.model.get_weights()),
                                         "optimizer_state": self.optimizer_state()})
                if self.config.save_model:               # trainer.py:96-97
                    shared_storage.save_checkpoint()
            shared_storage.set_info({"training_step": self.training_step, "lr": self._lr_host,
                                     "total_loss": total_loss, "value_loss": value_loss, "reward_loss": reward_loss,
                                     "policy_loss": policy_loss})
            done += 1
            if max_steps is not None and done >= max_steps:
                break
            if self.config.training_delay:
                time.sleep(self.config.training_delay)
            if self.config.ratio:
                while (self.training_step / max(1, shared_storage.get_info("num_played_steps")) > self.config.ratio
                       and self.training_step < self.config.training_steps and not shared_storage.get_info("terminate")):
                    time.sleep(0.5)

    def train_steps(self, replay_buffer, n):
        """`n` training steps on a device-sampling replay buffer (ReplayBuffer(device_sampling=True)): get_batch ->
        update_lr -> step -> update_priorities, queued back to back on the current stream with no synchronisation in
        between; in graph mode the batch is written straight into the capture's static buffers.  The step is
        update_weights' (_queue_step), so an eager trainer with native_loss = False takes the torch expression here too.
        Returns the last step's (total, value, reward, policy) losses, read back with one synchronisation at the end."""
        if not getattr(replay_buffer, "device_sampling", False):
            raise ValueError("train_steps needs a ReplayBuffer(device_sampling=True)")
        device = next(self.model.parameters()).device
        if device.type != "cuda":
            raise NotImplementedError("train_steps queues HIP work: the model must be on the GPU")
        report = None
        for _ in range(int(n)):
            if self._graph_mode and self._graph is not None:
                index_batch, _batch = replay_buffer.get_batch(out=self._static)
                b = None                                 # already where the capture reads it: nothing to copy
            else:
                index_batch, (obs, act, val, rew, pol, weights, scales) = replay_buffer.get_batch()
                b = {"observations": obs, "actions": act.unsqueeze(-1), "values": val, "rewards": rew, "policies": pol,
                     "weights": weights if self.config.PER else None, "gradient_scales": scales}
            self.update_lr()
            report, priorities = self._step(b)
            self.training_step += 1
            if self.config.PER:
                replay_buffer.update_priorities(priorities, index_batch)
        if report is None:
            return None
        return tuple(report.tolist())

    # ---- one training step (trainer.py:124-268) ---------------------------------------------------------
    def _batch_on_device(self, batch):
        """The seven batch entries as float32 tensors on the model's device (actions: int64 [B, K+1, 1]).  Lists and
        numpy arrays (the reference's replay buffer) and CUDA tensors (the device replay store) are both accepted."""
        device = next(self.model.parameters()).device

        def as_tensor(x):
            if torch.is_tensor(x):
                return x.to(device)
            if isinstance(x, numpy.ndarray):
                x = x.copy()
            return torch.tensor(numpy.asarray(x)).to(device)

        observations, actions, values, rewards, policies, weights, gradient_scales = batch
        return {"observations": as_tensor(observations).float(), "actions": as_tensor(actions).long().unsqueeze(-1),
                "values": as_tensor(values).float(), "rewards": as_tensor(rewards).float(),
                "policies": as_tensor(policies).float(),
                "weights": as_tensor(weights).float() if self.config.PER else None,
                "gradient_scales": as_tensor(gradient_scales).float()}

    def _unroll(self, observations, actions):
        """(value logits, reward logits, policy logits) per unroll step; the hidden state handed from step to step
        passes half of its gradient on (paper appendix "Training", trainer.py:171-173)."""
        if getattr(self, "_native_conv", False):     # (getattr: the tests unroll float64 twins through a bare namespace)
            self.model.pack_training_convs()         # once per step and module, queued with the step: a replay repacks
        if getattr(self, "_fold", None):
            self.optimizer.sink.reset()              # this step's first gradient of every parameter goes to slot 0
        out = self.model.initial_inference(observations)
        steps, hidden = [out[:3]], out[3]
        for k in range(1, actions.shape[1]):
            out = self.model.recurrent_inference(hidden, actions[:, k])
            hidden = _scale_gradient(out[3], 2.0)
            steps.append(out[:3])
        return steps

    def update_weights(self, batch):
        report, new_priorities = self._step(self._batch_on_device(batch))
        self.training_step += 1
        total_loss, value_loss, reward_loss, policy_loss = report.tolist()       # the step's one device-to-host report
        return new_priorities.cpu().numpy(), total_loss, value_loss, reward_loss, policy_loss

    def _step(self, b):
        """One step on the batch dict `b`, eager or (graph mode) as a hipGraph replay: (report, priorities) as device
        tensors, report = the (total, value, reward, policy) losses.  `b` None: the batch is in the static buffers."""
        if not self._graph_mode:
            return self._queue_step(b)
        if self._graph is None:
            self._capture(b)
        if b is not None:
            self._to_static(b)
        self._replay()
        return self._graph_out

    def _queue_step(self, b):
        """Queue one whole training step on the current stream -- what update_weights, train_steps, a capture's warm-up and
        the capture itself run.  The ways differ in what produces the gradients, nothing else."""
        if self._fc is not None:
            # four HIP launches overwrite the flat gradient buffer whole.  No zero_grad here, ever: with torch's optimizer
            # set_to_none would drop the p.grad views into that buffer
            sample_loss, head_sums, priorities = self._fc_queue(b)
            loss = sample_loss.mean()
        else:
            # autograd through the unroll, under the loss as one HIP launch or, on the CPU and with native_loss = False,
            # as the torch expression (a capture always takes the launch).  The gradients are None from here to backward,
            # so a capture's backward allocates them from the graph's pool
            if b["values"].is_cuda and (self.native_loss or self._graph_mode):
                sample_loss, head_sums, priorities = self._loss_native(b)
            else:
                sample_loss, head_sums, priorities = self._loss_torch(b)
            loss = sample_loss.mean()
            if self._fold:
                # p.grad is None and stays None: the Functions write every weight gradient into its slot
                loss.backward()
                self._fold_after_backward()
            else:
                self.optimizer.zero_grad(set_to_none=True)
                loss.backward()
        self.optimizer.step()
        if self._fold:
            self._fold_mark_moved()
        return torch.cat([loss.detach().reshape(1), head_sums.mean(dim=1)]), priorities

    def _loss_native(self, b):
        """Everything between the network's outputs and `loss.mean()` in one HIP launch (_UnrollLoss): the logits of all
        unrolled positions are stacked step-major, the kernel returns the per-sample loss and keeps its gradient for
        backward."""
        steps = self._unroll(b["observations"], b["actions"])
        cfg = self.config
        return _UnrollLoss.apply(torch.stack([s[0] for s in steps]), torch.stack([s[1] for s in steps]),
                                 torch.stack([s[2] for s in steps]), b, cfg.support_size, cfg.value_loss_weight,
                                 cfg.PER_alpha)

    def _loss_torch(self, b):
        """The reference's loss as a torch expression, in _loss_native's form: (per-sample loss [B], head sums, priorities
        [B, K+1]).  The head sums come back already averaged over the batch, as [3, 1], each by the reference's own
        `.mean()` of a [B] vector: the mean over that last axis of one entry is exact."""
        cfg = self.config
        steps = self._unroll(b["observations"], b["actions"])
        value_targets = models.scalar_to_support(b["values"], cfg.support_size)
        reward_targets = models.scalar_to_support(b["rewards"], cfg.support_size)
        priorities = torch.zeros_like(b["values"])
        sums = {"value": 0, "reward": 0, "policy": 0}
        for k, (value, reward, policy_logits) in enumerate(steps):
            per_head = dict(zip(("value", "reward", "policy"), self.loss_function(
                value.squeeze(-1), reward.squeeze(-1), policy_logits, value_targets[:, k], reward_targets[:, k],
                b["policies"][:, k])))
            if k == 0:
                del per_head["reward"]           # no reward is predicted for the root position (trainer.py:182-193)
            for head, term in per_head.items():
                if k > 0:                        # every unrolled step contributes 1 / (its gradient scale) of its gradient
                    term = _scale_gradient(term, b["gradient_scales"][:, k])
                sums[head] = sums[head] + term
            with torch.no_grad():                # new priorities: |predicted value - target| ** alpha (trainer.py:199-209)
                predicted = models.support_to_scalar(value, cfg.support_size).squeeze(-1)
                priorities[:, k] = torch.abs(predicted - b["values"][:, k]) ** cfg.PER_alpha

        loss = sums["value"] * cfg.value_loss_weight + sums["reward"] + sums["policy"]
        if cfg.PER:
            loss = loss * b["weights"]           # importance-sampling correction of the prioritised replay
        head_means = torch.stack([sums[head].mean().detach() for head in ("value", "reward", "policy")])
        return loss, head_means.unsqueeze(1), priorities

    # ---- graph mode: the step captured once, then replayed ----------------------------------------------
    def _to_static(self, b):
        for key, value in b.items():
            if value is not None:
                self._static[key].copy_(value)

    def _replay(self):
        self._graph.replay()
        for norm in self._native_norms:      # a replay runs no Python: drop the eval-mode constants the launches outdated
            norm._folded = None
        if self._fold:
            self._fold_mark_moved()

    def _capture(self, b):
        """Warm _queue_step up on a side stream (what stream capture requires) and capture it into a hipGraph on static
        copies of the batch `b`; the capture itself does not execute the step.  Every later step copies its batch in,
        replays, and reads report and priorities out of the capture's output tensors (_graph_out).  On the fc_step way
        the warm-up sizes the handle for this batch; a larger one after the capture is refused (_fc_handle)."""
        self._static = {k: (v.clone() if v is not None else None) for k, v in b.items()}
        dev = b["values"].device
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        weights, optimizer = copy.deepcopy(self.model.state_dict()), self._optimizer_snapshot()
        with torch.cuda.stream(side):
            for _ in range(3):                       # warm-up steps, undone below
                self._queue_step(self._static)
        torch.cuda.current_stream(dev).wait_stream(side)
        self.model.load_state_dict(weights)          # in place: fc_step's parameters stay views of the flat buffer
        self._optimizer_restore(optimizer)
        if self._fc is None:
            # the warm-up's gradients go before the capture begins, not at the zero_grad inside it: the capture's
            # backward allocates them anew from the graph's pool either way (same bits), but the allocator then enters
            # the capture with nothing of the warm-up alive, which the step times of the residual networks prefer
            self.optimizer.zero_grad(set_to_none=True)
        self._graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self._graph):
            self._graph_out = self._queue_step(self._static)

    def _optimizer_snapshot(self):
        return self.optimizer.snapshot() if self._fc_opt else copy.deepcopy(self.optimizer.state_dict())

    def _optimizer_restore(self, saved):
        """Undo a capture's warm-up steps on the optimizer, in place."""
        if self._fc_opt:
            return self.optimizer.restore(saved)     # the moments and the count of steps done, as they were
        # the optimizer's moments and step counters must exist BEFORE the capture (created inside it they would be
        # re-initialised by every replay): keep the tensors the warm-up made, put the saved values back in place
        for index, entry in self.optimizer.state_dict()["state"].items():
            before = saved["state"].get(index)
            for name, value in entry.items():
                if torch.is_tensor(value):
                    value.copy_(before[name]) if before is not None else value.zero_()

    def update_lr(self):
        lr = self.config.lr_init * self.config.lr_decay_rate ** (self.training_step / self.config.lr_decay_steps)
        self._lr_host = float(lr)              # what set_info publishes: a Python float, as in the reference
        if self._fc_opt:
            self.optimizer.set_lr(lr)
            return
        if self._graph_mode:
            self._lr.fill_(lr)
            return
        for param_group in self.optimizer.param_groups:
            param_group["lr"] = lr

    @staticmethod
    def loss_function(value, reward, policy_logits, target_value, target_reward, target_policy):
        value_loss = (-target_value * torch.nn.LogSoftmax(dim=1)(value)).sum(1)
        reward_loss = (-target_reward * torch.nn.LogSoftmax(dim=1)(reward)).sum(1)
        policy_loss = (-target_policy * torch.nn.LogSoftmax(dim=1)(policy_logits)).sum(1)
        return value_loss, reward_loss, policy_loss

    # ---- producer side of the weight hand-over -----------------------------------------------------------
    @torch.no_grad()
    def publish(self, flat):
        """Copy the trained parameters (and BN statistics) into an actor-side flat buffer (weights.FlatWeights):
        the actors' models alias it, so the next search -- or the next RCCL broadcast from this rank -- sees them."""
        flat.load_state_dict(self.model.state_dict())
