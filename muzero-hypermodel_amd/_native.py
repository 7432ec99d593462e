"""ctypes binding of libmzmcts.so (the C ABI of include/mzmcts.h).

There is NO Python / CPU fallback for the tree kernels: if the library is missing or no HIP device
is present, loading / engine creation raises.
"""
import ctypes
import os

import numpy as np

from .build import LIB_PATH

c_i32_p = ctypes.POINTER(ctypes.c_int32)
c_i64_p = ctypes.POINTER(ctypes.c_int64)
c_u32_p = ctypes.POINTER(ctypes.c_uint32)
c_u64_p = ctypes.POINTER(ctypes.c_uint64)
c_f64_p = ctypes.POINTER(ctypes.c_double)
c_f32_p = ctypes.POINTER(ctypes.c_float)
c_void = ctypes.c_void_p

ABI_VERSION = 2
ERR_INVALID, ERR_HIP, ERR_EMPTY_LEGAL, ERR_LEGAL_RANGE, ERR_PLAYERS = -1, -2, -3, -4, -5


class MzConfig(ctypes.Structure):
    _fields_ = [("num_envs", ctypes.c_int32), ("num_actions", ctypes.c_int32),
                ("num_simulations", ctypes.c_int32), ("num_players", ctypes.c_int32),
                ("support_size", ctypes.c_int32), ("hidden_floats", ctypes.c_int32),
                ("device", ctypes.c_int32), ("group_width", ctypes.c_int32),
                ("discount", ctypes.c_double), ("pb_c_base", ctypes.c_double),
                ("pb_c_init", ctypes.c_double), ("root_dirichlet_alpha", ctypes.c_double),
                ("root_exploration_fraction", ctypes.c_double), ("hidden_pool", c_void)]


class MzRootStats(ctypes.Structure):
    _fields_ = [("visits", c_i32_p), ("child_value_sum", c_f64_p), ("child_prior", c_f64_p),
                ("child_reward", c_f64_p), ("child_expanded", c_i32_p), ("root_value_sum", c_f64_p),
                ("root_visits", c_i32_p), ("max_tree_depth", c_i32_p),
                ("root_predicted_value", c_f64_p), ("min_max", c_f64_p), ("depth_sum", c_i64_p),
                ("tie_break_words", c_u32_p)]


class MzProfile(ctypes.Structure):
    _fields_ = [("select_ms", ctypes.c_double), ("expand_backup_ms", ctypes.c_double),
                ("root_ms", ctypes.c_double), ("fused_ms", ctypes.c_double),
                ("select_launches", ctypes.c_int64), ("expand_backup_launches", ctypes.c_int64),
                ("root_launches", ctypes.c_int64), ("fused_launches", ctypes.c_int64),
                ("select_depth_sum", ctypes.c_int64), ("simulations", ctypes.c_int64),
                ("step_ms", ctypes.c_double), ("step_launches", ctypes.c_int64)]


class MzTrainLossArgs(ctypes.Structure):
    """include/mztrain.h mztrain_loss_args: raw device pointers + sizes of one training step's loss."""
    _fields_ = [(name, ctypes.c_void_p) for name in ("value_logits", "reward_logits", "policy_logits", "target_value",
                                                     "target_reward", "target_policy", "gradient_scale", "weight")] + \
               [("batch", ctypes.c_int32), ("steps", ctypes.c_int32), ("support_size", ctypes.c_int32),
                ("actions", ctypes.c_int32), ("value_loss_weight", ctypes.c_float), ("per_alpha", ctypes.c_float)] + \
               [(name, ctypes.c_void_p) for name in ("sample_loss", "head_sums", "priorities", "grad_value", "grad_reward",
                                                     "grad_policy")]


class MzTowerGather(ctypes.Structure):
    """include/mzmcts.h mzmcts_tower_gather."""
    _fields_ = [("pool", ctypes.c_void_p), ("parent", ctypes.c_void_p), ("action", ctypes.c_void_p),
                ("envs", ctypes.c_int64), ("hidden_floats", ctypes.c_int32), ("action_space", ctypes.c_float)]


class MzTrainFcArgs(ctypes.Structure):
    """include/mztrain.h mztrain_fc_args: one training step of a fully-connected network."""
    _fields_ = [(name, ctypes.c_void_p) for name in ("observations", "actions", "target_value", "target_reward",
                                                     "target_policy", "gradient_scale", "weight")] + \
               [("batch", ctypes.c_int32), ("steps", ctypes.c_int32), ("value_loss_weight", ctypes.c_float),
                ("per_alpha", ctypes.c_float)] + \
               [(name, ctypes.c_void_p) for name in ("sample_loss", "head_sums", "priorities")]


class MzTrainOptArgs(ctypes.Structure):
    """include/mztrain.h mztrain_opt_args: one optimizer step on the flat weight / gradient buffers."""
    _fields_ = [("kind", ctypes.c_int32), ("n", ctypes.c_int64)] + \
               [(name, ctypes.c_void_p) for name in ("weights", "grads", "moment1", "moment2", "lr", "steps_done")] + \
               [(name, ctypes.c_double) for name in ("beta1", "beta2", "eps", "weight_decay", "momentum")]


OPT_ADAM, OPT_SGD = 0, 1


class MzTrainFoldSegment(ctypes.Structure):
    """include/mztrain.h mztrain_fold_segment: one parameter tensor in the flat buffers and its slots in the staging buffer."""
    _fields_ = [(name, ctypes.c_int64) for name in ("offset", "count", "slot_base", "slot_stride")] + \
               [("capacity", ctypes.c_int32), ("reserved", ctypes.c_int32)]


class MzTrainFoldArgs(ctypes.Structure):
    """include/mztrain.h mztrain_fold_args: one fold-and-update step."""
    _fields_ = [("opt", MzTrainOptArgs), ("staging", ctypes.c_void_p), ("staging_floats", ctypes.c_int64)]


FOLD_SLOT_ALIGN = 128     # floats: the trainer rounds a segment's slot_stride up to this (512 bytes)
FOLD_CHUNK = 1024         # floats of a full chunk of the launch (csrc/grad_fold.h kChunk)
FOLD_MAX_BLOCKS = 1024


class MzTrainEpilogueForwardArgs(ctypes.Structure):
    """include/mztrain.h mztrain_epilogue_forward_args: relu(batch_norm(x) [+ residual]) in training."""
    _fields_ = [(name, ctypes.c_void_p) for name in ("x", "residual", "gamma", "beta", "running_mean", "running_var", "out",
                                                     "save_mean", "save_invstd")] + \
               [("batch", ctypes.c_int64), ("channels", ctypes.c_int32), ("hw", ctypes.c_int32), ("eps", ctypes.c_double),
                ("momentum", ctypes.c_double)]


class MzTrainEpilogueBackwardArgs(ctypes.Structure):
    """include/mztrain.h mztrain_epilogue_backward_args."""
    _fields_ = [(name, ctypes.c_void_p) for name in ("dy", "x", "out", "gamma", "save_mean", "save_invstd", "dx", "dresidual",
                                                     "dgamma", "dbeta")] + \
               [("batch", ctypes.c_int64), ("channels", ctypes.c_int32), ("hw", ctypes.c_int32)]


EPILOGUE_KEEP_VALUES = 4096     # include/mztrain.h MZTRAIN_EPILOGUE_KEEP_VALUES


class MzTrainConvPackArgs(ctypes.Structure):
    """include/mztrain.h mztrain_conv_pack_args: both packings of a 3 x 3 weight and the ones | zeros pair."""
    _fields_ = [(name, ctypes.c_void_p) for name in ("weight", "packed", "packed_dx", "affine")] + \
               [("cin", ctypes.c_int32), ("cout", ctypes.c_int32), ("dx_planes", ctypes.c_int32)]


class MzTrainConvForwardArgs(ctypes.Structure):
    """include/mztrain.h mztrain_conv_forward_args."""
    _fields_ = [(name, ctypes.c_void_p) for name in ("x", "packed", "affine", "weight", "y")] + \
               [("batch", ctypes.c_int64), ("cin", ctypes.c_int32), ("cout", ctypes.c_int32), ("height", ctypes.c_int32),
                ("width", ctypes.c_int32)]


class MzTrainConvDgradArgs(ctypes.Structure):
    """include/mztrain.h mztrain_conv_dgrad_args."""
    _fields_ = [(name, ctypes.c_void_p) for name in ("dy", "packed_dx", "affine", "weight", "dx")] + \
               [("batch", ctypes.c_int64), ("cin", ctypes.c_int32), ("cout", ctypes.c_int32), ("height", ctypes.c_int32),
                ("width", ctypes.c_int32), ("dx_planes", ctypes.c_int32)]


class MzTrainConvWgradArgs(ctypes.Structure):
    """include/mztrain.h mztrain_conv_wgrad_args."""
    _fields_ = [(name, ctypes.c_void_p) for name in ("x", "dy", "dw")] + \
               [("batch", ctypes.c_int64), ("cin", ctypes.c_int32), ("cout", ctypes.c_int32), ("height", ctypes.c_int32),
                ("width", ctypes.c_int32)]


CONV_SLICE = 64                 # include/mztrain.h MZTRAIN_CONV_SLICE
CONV_AFFINE = 64                # include/mztrain.h MZTRAIN_CONV_AFFINE


class MzHeadDesc(ctypes.Structure):
    """mzmcts_head_desc (include/mzmcts.h): one reward / value / policy head of the residual networks."""
    _fields_ = [("conv_w", c_void), ("conv_b", c_void), ("fc1_w", c_void), ("fc1_b", c_void), ("fc2_w", c_void),
                ("fc2_b", c_void), ("channels", ctypes.c_int32), ("plane", ctypes.c_int32), ("reduced", ctypes.c_int32),
                ("hidden", ctypes.c_int32), ("outputs", ctypes.c_int32)]


HEADS_MAX = 2                   # include/mztrain.h MZTRAIN_HEADS_MAX
HEADS_ELU_ULPS = 4              # include/mztrain.h MZTRAIN_HEADS_ELU_ULPS
HEADS_MAX_BATCH = 65536         # include/mztrain.h MZTRAIN_HEADS_MAX_BATCH


class MzTrainHeadsForwardArgs(ctypes.Structure):
    """include/mztrain.h mztrain_heads_forward_args: one or two heads reading one tensor."""
    _fields_ = [("x", c_void), ("heads", MzHeadDesc * HEADS_MAX), ("logits", c_void * HEADS_MAX), ("flat", c_void * HEADS_MAX),
                ("pre", c_void * HEADS_MAX), ("batch", ctypes.c_int64), ("n_heads", ctypes.c_int32)]


class MzTrainHeadsGrads(ctypes.Structure):
    """include/mztrain.h mztrain_heads_grads: one head's parameter gradients (None: not computed)."""
    _fields_ = [(name, c_void) for name in ("conv_w", "conv_b", "fc1_w", "fc1_b", "fc2_w", "fc2_b")]


class MzTrainHeadsBackwardArgs(ctypes.Structure):
    """include/mztrain.h mztrain_heads_backward_args."""
    _fields_ = [("x", c_void), ("heads", MzHeadDesc * HEADS_MAX)] + \
               [(name, c_void * HEADS_MAX) for name in ("dlogits", "flat", "pre", "dpre", "dflat")] + \
               [("dx", c_void), ("grads", MzTrainHeadsGrads * HEADS_MAX), ("batch", ctypes.c_int64), ("n_heads", ctypes.c_int32)]


class MzTrainRescaleBackwardArgs(ctypes.Structure):
    """include/mztrain.h mztrain_rescale_backward_args: rows of row_len floats."""
    _fields_ = [("x", c_void), ("grad_out", c_void), ("grad_x", c_void), ("rows", ctypes.c_int64), ("row_len", ctypes.c_int32)]


class MzFcDesc(ctypes.Structure):
    _fields_ = [("observation_floats", ctypes.c_int32), ("encoding_size", ctypes.c_int32),
                ("n_hidden", ctypes.c_int32 * 5), ("hidden", (ctypes.c_int32 * 3) * 5)]


# name -> (restype, argtypes); every symbol include/mzmcts.h declares
PROTOTYPES = {
    "mzmcts_abi_version": (ctypes.c_int, []),
    "mzmcts_create": (ctypes.c_int, [ctypes.POINTER(MzConfig), ctypes.POINTER(c_void)]),
    "mzmcts_destroy": (None, [c_void]),
    "mzmcts_last_error": (ctypes.c_char_p, [c_void]),
    "mzmcts_seed": (ctypes.c_int, [c_void, c_u32_p, c_void]),
    "mzmcts_rng_set_state": (ctypes.c_int, [c_void, ctypes.c_int32, c_u32_p, ctypes.c_int32,
                                            ctypes.c_int32, ctypes.c_double, c_void]),
    "mzmcts_rng_get_state": (ctypes.c_int, [c_void, ctypes.c_int32, c_u32_p, c_i32_p, c_i32_p,
                                            c_f64_p, c_void]),
    "mzmcts_begin_search": (ctypes.c_int, [c_void, c_i32_p, c_i32_p, c_i32_p, ctypes.c_int32,
                                           c_f64_p, c_void]),
    "mzmcts_expand_roots": (ctypes.c_int, [c_void, c_void, c_void, c_void, c_void, c_void]),
    "mzmcts_expand_roots_injected": (ctypes.c_int, [c_void, c_void, c_void, c_void]),
    "mzmcts_select": (ctypes.c_int, [c_void, c_void, c_void, c_void]),
    "mzmcts_select_planes": (ctypes.c_int, [c_void, c_void, c_void, ctypes.c_int32, ctypes.c_int32, c_void]),
    "mzmcts_expand_backup": (ctypes.c_int, [c_void, c_void, c_void, c_void, c_void, c_void]),
    "mzmcts_expand_backup_injected": (ctypes.c_int, [c_void, c_void, c_void, c_void, c_void]),
    "mzmcts_hidden_slab": (c_void, [c_void, ctypes.c_int32]),
    "mzmcts_next_slab": (ctypes.c_int32, [c_void]),
    "mzmcts_simulations_done": (ctypes.c_int32, [c_void]),
    "mzmcts_set_simulations_done": (ctypes.c_int, [c_void, ctypes.c_int32]),
    "mzmcts_readout": (ctypes.c_int, [c_void, ctypes.POINTER(MzRootStats), c_void]),
    "mzmcts_readout_begin": (ctypes.c_int, [c_void, c_void]),
    "mzmcts_sample_actions": (ctypes.c_int, [c_void, c_f64_p, c_i32_p, c_i32_p]),
    "mzmcts_search_statistics": (ctypes.c_int, [c_void, c_f64_p, c_f64_p]),
    "mzmcts_last_paths": (ctypes.c_int, [c_void, c_i32_p, c_i32_p, c_i32_p, c_void]),
    "mzmcts_set_debug_ties": (ctypes.c_int, [c_void, ctypes.c_int32]),
    "mzmcts_export_tree": (ctypes.c_int, [c_void, ctypes.c_int32, c_i32_p, c_f64_p, c_f64_p, c_f64_p,
                                          c_i32_p, c_void]),
    "mzmcts_fc_configure": (ctypes.c_int, [c_void, ctypes.POINTER(MzFcDesc), c_void, ctypes.c_int64]),
    "mzmcts_fc_initial_inference": (ctypes.c_int, [c_void, c_void, c_void, c_void, c_void, c_void, c_void]),
    "mzmcts_fc_recurrent_inference": (ctypes.c_int, [c_void, c_void, c_void, c_void, c_void, c_void, c_void, c_void]),
    "mzmcts_search_fused_fc": (ctypes.c_int, [c_void, c_void, ctypes.c_int32, c_void]),
    "mzmcts_fused_lds_bytes": (ctypes.c_int64, [c_void, ctypes.c_int32]),
    "mzmcts_set_fused_options": (ctypes.c_int, [c_void, ctypes.c_int32, ctypes.c_int32]),
    "mzmcts_fused_variant": (ctypes.c_int32, [c_void]),
    "mzmcts_moves_prepare": (ctypes.c_int, [c_void, ctypes.c_int32, c_i32_p, c_i32_p, c_i32_p, ctypes.c_int32, c_f64_p, c_void]),
    "mzmcts_moves_predraw_next": (ctypes.c_int, [c_void, ctypes.c_int32, c_i32_p, c_i32_p, c_i32_p, ctypes.c_int32, c_f64_p]),
    "mzmcts_moves_submit_next": (ctypes.c_int, [c_void, c_void]),
    "mzmcts_moves_discard_next": (ctypes.c_int, [c_void]),
    "mzmcts_moves_prepare_device": (ctypes.c_int, [c_void, ctypes.c_int32, c_void, c_void, c_void, ctypes.c_int32, c_f64_p, c_void]),
    "mzmcts_moves_inputs": (ctypes.c_int, [c_void, c_i32_p, c_i32_p, c_i32_p]),
    "mzmcts_moves_enqueue": (ctypes.c_int, [c_void, c_void, c_void]),
    "mzmcts_moves_begin_lockstep": (ctypes.c_int, [c_void, c_void]),
    "mzmcts_moves_end_lockstep": (ctypes.c_int, [c_void, c_void]),
    "mzmcts_moves_temperature_threshold": (ctypes.c_int, [c_void, ctypes.c_int32, c_i32_p, c_void]),
    "mzmcts_moves_finished": (ctypes.c_int, [c_void, c_void]),
    "mzmcts_moves_sit_out": (ctypes.c_int, [c_void, ctypes.c_int32]),
    "mzmcts_rng_streams": (ctypes.c_int, [c_void, ctypes.POINTER(c_void), ctypes.POINTER(c_void)]),
    "mzmcts_rng_consumed": (ctypes.c_int, [c_void, c_u32_p]),
    "mzmcts_noise_rows": (ctypes.c_int, [c_void, ctypes.POINTER(c_void)]),
    "mzmcts_moves_actions": (c_void, [c_void, ctypes.c_int32]),
    "mzmcts_moves_ring": (ctypes.c_int, [c_void, ctypes.POINTER(c_void), c_i64_p, c_i64_p, c_i32_p]),
    "mzmcts_moves_inputs_ring": (ctypes.c_int, [c_void, ctypes.POINTER(c_void), c_i64_p, c_i64_p]),
    "mzmcts_moves_device_ring": (ctypes.c_int, [c_void, ctypes.POINTER(c_void), c_i64_p, c_i64_p, c_i32_p]),
    "mzmcts_moves_inputs_device_ring": (ctypes.c_int, [c_void, ctypes.POINTER(c_void), c_i64_p, c_i64_p]),
    "mzmcts_moves_collect": (ctypes.c_int, [c_void, c_i32_p, c_i32_p, c_i32_p, c_f64_p, c_f32_p, c_i32_p, c_void]),
    "mzmcts_set_profiling": (ctypes.c_int, [c_void, ctypes.c_int32]),
    "mzmcts_set_select_queue": (ctypes.c_int, [c_void, ctypes.c_int32]),
    "mzmcts_get_profile": (ctypes.c_int, [c_void, ctypes.POINTER(MzProfile), ctypes.c_int32]),
    "mzmcts_device_bytes": (ctypes.c_int64, [c_void]),
    "mzmcts_state_action_planes": (ctypes.c_int, [c_void, c_void, c_void, ctypes.c_int64, ctypes.c_int32, ctypes.c_int32,
                                                  ctypes.c_int32, c_void]),
    "mzmcts_conv_heads": (ctypes.c_int, [c_void, c_void, ctypes.c_int32, c_void, ctypes.c_int64, c_void]),
    "mzmcts_conv_heads_multi": (ctypes.c_int, [c_void, c_void, ctypes.c_int32, c_void, ctypes.c_int64, c_void]),
    "mzmcts_conv_head": (ctypes.c_int, [c_void, c_void, c_void, ctypes.c_int64, c_void]),
    "mzmcts_unit_rescale": (ctypes.c_int, [c_void, c_void, ctypes.c_int64, ctypes.c_int32, c_void]),
    "mzmcts_expand_backup_select": (ctypes.c_int, [c_void] * 8),
    "mzmcts_expand_backup_select_planes": (ctypes.c_int, [c_void] * 7 + [ctypes.c_int32, ctypes.c_int32, c_void]),
    "mzmcts_expand_backup_select_injected": (ctypes.c_int, [c_void] * 7),
    "mzmcts_board_conv_packed_floats": (ctypes.c_int64, [ctypes.c_int32, ctypes.c_int32]),
    "mzmcts_board_conv_pack": (ctypes.c_int, [c_void, c_void, ctypes.c_int32, ctypes.c_int32, c_void]),
    "mzmcts_board_conv_supported": (ctypes.c_int, [ctypes.c_int32] * 4),
    "mzmcts_board_conv3x3": (ctypes.c_int, [c_void] * 6 + [ctypes.c_int64] + [ctypes.c_int32] * 5 + [c_void]),
    "mzmcts_board_tower_blocks": (ctypes.c_int64, [ctypes.c_int64] + [ctypes.c_int32] * 3),
    "mzmcts_board_tower_heads": (ctypes.c_int, [c_void, c_void, ctypes.c_int64] + [ctypes.c_int32] * 4 +
                                 [c_void, ctypes.c_int32, c_void, ctypes.c_int32, c_void]),
    "mzmcts_board_tower": (ctypes.c_int, [c_void, ctypes.c_int64] + [ctypes.c_int32] * 4 + [c_void, ctypes.c_int32, c_void]),
    "mzmcts_board_conv_wide_supported": (ctypes.c_int, [ctypes.c_int32] * 4),
    "mzmcts_board_conv_wide_halfs": (ctypes.c_int64, [ctypes.c_int32, ctypes.c_int32]),
    "mzmcts_board_conv_wide_pack": (ctypes.c_int, [c_void, c_void, ctypes.c_int32, ctypes.c_int32, c_void]),
    "mzmcts_board_conv_wide": (ctypes.c_int, [c_void] * 8 + [ctypes.c_int64] + [ctypes.c_int32] * 5 + [c_void]),
    "mzmcts_board_conv_split_halfs": (ctypes.c_int64, [ctypes.c_int32, ctypes.c_int32]),
    "mzmcts_board_conv_pack_split": (ctypes.c_int, [c_void, c_void, c_void] + [ctypes.c_int32] * 5 + [c_void]),
    "mzmcts_tower_gather_args": (ctypes.c_int, [c_void, c_void, ctypes.c_int32, ctypes.POINTER(MzTowerGather)]),
    "mzmcts_board_tower_gathered": (ctypes.c_int, [ctypes.POINTER(MzTowerGather), ctypes.c_int64] + [ctypes.c_int32] * 5 +
                                    [c_void, ctypes.c_int32, c_void]),
    "mzmcts_board_tower_split": (ctypes.c_int, [c_void, ctypes.c_int64] + [ctypes.c_int32] * 5 + [c_void, ctypes.c_int32, c_void]),
    "mzmcts_downsample_cnn": (ctypes.c_int, [c_void, ctypes.c_int64, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, c_void, c_void,
                                             ctypes.c_int32, ctypes.c_int32, c_void, c_void, ctypes.c_int32, ctypes.c_int32,
                                             ctypes.c_int32, c_void, c_void]),
    "mzmcts_affine_act": (ctypes.c_int, [c_void] * 5 + [ctypes.c_int64, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, c_void]),
    # include/mzenv.h
    "mzenv_advance": (ctypes.c_int, [c_void] * 10),
    "mztrain_unroll_loss": (ctypes.c_int, [ctypes.POINTER(MzTrainLossArgs), c_void]),
    "mztrain_fc_create": (ctypes.c_int, [ctypes.POINTER(MzFcDesc), ctypes.c_int32, ctypes.c_int32, c_void, ctypes.c_int64,
                                         c_void, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(c_void)]),
    "mztrain_fc_destroy": (None, [c_void]),
    "mztrain_fc_workspace_bytes": (ctypes.c_int64, [c_void]),
    "mztrain_fc_step": (ctypes.c_int, [c_void, ctypes.POINTER(MzTrainFcArgs), c_void]),
    "mztrain_fc_logits": (ctypes.c_int, [c_void, ctypes.POINTER(c_void), ctypes.POINTER(c_void), ctypes.POINTER(c_void)]),
    "mztrain_opt_step": (ctypes.c_int, [ctypes.POINTER(MzTrainOptArgs), c_void]),
    "mztrain_opt_reference": (ctypes.c_int, [ctypes.POINTER(MzTrainOptArgs)]),
    "mztrain_opt_scalars": (ctypes.c_int, [ctypes.c_double, ctypes.c_double, ctypes.c_double, ctypes.c_int64,
                                           ctypes.POINTER(ctypes.c_double)]),
    "mztrain_fold_create": (ctypes.c_int, [ctypes.POINTER(MzTrainFoldSegment), ctypes.c_int32, ctypes.c_int64, ctypes.c_int64,
                                           ctypes.c_int32, ctypes.POINTER(c_void)]),
    "mztrain_fold_destroy": (None, [c_void]),
    "mztrain_fold_set_uses": (ctypes.c_int, [c_void, ctypes.POINTER(ctypes.c_int32), ctypes.c_int32]),
    "mztrain_fold_step": (ctypes.c_int, [c_void, ctypes.POINTER(MzTrainFoldArgs), c_void]),
    "mztrain_fold_reference": (ctypes.c_int, [ctypes.POINTER(MzTrainFoldSegment), ctypes.POINTER(ctypes.c_int32),
                                              ctypes.c_int32, ctypes.POINTER(MzTrainFoldArgs)]),
    "mztrain_fold_plan": (ctypes.c_int, [ctypes.POINTER(MzTrainFoldSegment), ctypes.c_int32, ctypes.c_int64, ctypes.c_int64,
                                         ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int64), ctypes.c_int64]),
    "mztrain_epilogue_forward": (ctypes.c_int, [ctypes.POINTER(MzTrainEpilogueForwardArgs), c_void]),
    "mztrain_epilogue_backward": (ctypes.c_int, [ctypes.POINTER(MzTrainEpilogueBackwardArgs), c_void]),
    "mztrain_epilogue_reference_forward": (ctypes.c_int, [ctypes.POINTER(MzTrainEpilogueForwardArgs)]),
    "mztrain_epilogue_reference_backward": (ctypes.c_int, [ctypes.POINTER(MzTrainEpilogueBackwardArgs)]),
    "mztrain_conv_supported": (ctypes.c_int, [ctypes.c_int32] * 5),
    "mztrain_conv_slice": (ctypes.c_int32, []),
    "mztrain_conv_max_batch": (ctypes.c_int64, [ctypes.c_int32] * 4),
    "mztrain_conv_wgrad_plan": (ctypes.c_int, [ctypes.c_int64] + [ctypes.c_int32] * 4 + [ctypes.POINTER(ctypes.c_int64)]),
    "mztrain_conv_pack": (ctypes.c_int, [ctypes.POINTER(MzTrainConvPackArgs), c_void]),
    "mztrain_conv_forward": (ctypes.c_int, [ctypes.POINTER(MzTrainConvForwardArgs), c_void]),
    "mztrain_conv_dgrad": (ctypes.c_int, [ctypes.POINTER(MzTrainConvDgradArgs), c_void]),
    "mztrain_conv_wgrad": (ctypes.c_int, [ctypes.POINTER(MzTrainConvWgradArgs), c_void]),
    "mztrain_conv_reference_pack": (ctypes.c_int, [ctypes.POINTER(MzTrainConvPackArgs)]),
    "mztrain_conv_reference_forward": (ctypes.c_int, [ctypes.POINTER(MzTrainConvForwardArgs)]),
    "mztrain_conv_reference_dgrad": (ctypes.c_int, [ctypes.POINTER(MzTrainConvDgradArgs)]),
    "mztrain_conv_reference_wgrad": (ctypes.c_int, [ctypes.POINTER(MzTrainConvWgradArgs)]),
    "mztrain_heads_supported": (ctypes.c_int, [ctypes.c_int32] * 6),
    "mztrain_heads_forward": (ctypes.c_int, [ctypes.POINTER(MzTrainHeadsForwardArgs), c_void]),
    "mztrain_heads_backward": (ctypes.c_int, [ctypes.POINTER(MzTrainHeadsBackwardArgs), c_void]),
    "mztrain_heads_reference_forward": (ctypes.c_int, [ctypes.POINTER(MzTrainHeadsForwardArgs)]),
    "mztrain_heads_reference_backward": (ctypes.c_int, [ctypes.POINTER(MzTrainHeadsBackwardArgs)]),
    "mztrain_rescale_supported": (ctypes.c_int, [ctypes.c_int64, ctypes.c_int32]),
    "mztrain_rescale_backward": (ctypes.c_int, [ctypes.POINTER(MzTrainRescaleBackwardArgs), c_void]),
    "mztrain_rescale_reference_backward": (ctypes.c_int, [ctypes.POINTER(MzTrainRescaleBackwardArgs)]),
    "mztrain_rescale_backward_plan": (ctypes.c_int, [ctypes.c_int64, ctypes.c_int32, ctypes.POINTER(ctypes.c_int64)]),
    "mzhist_create": (ctypes.c_int, [ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(c_void)]),
    "mzhist_destroy": (None, [c_void]),
    "mzhist_last_error": (ctypes.c_char_p, [c_void]),
    "mzhist_begin": (ctypes.c_int, [c_void, c_f32_p, c_i32_p]),
    "mzhist_file": (ctypes.c_int, [c_void, c_void, c_i32_p]),
    "mzhist_finished": (ctypes.c_int, [c_void] + [ctypes.POINTER(c_void)] * 8 + [c_i32_p]),
    "mzhist_lengths": (c_void, [c_void]),
    "mzhist_searched_moves": (ctypes.c_int64, [c_void]),
    "mzreplay_create": (ctypes.c_int, [c_void, ctypes.POINTER(c_void)]),
    "mzreplay_destroy": (None, [c_void]),
    "mzreplay_last_error": (ctypes.c_char_p, [c_void]),
    "mzreplay_add_games": (ctypes.c_int, [c_void, ctypes.c_int32, c_i32_p, c_i32_p, c_f32_p, c_i32_p, c_f64_p, c_i32_p,
                                          c_f64_p, c_f64_p, c_f32_p, c_f32_p, c_void]),
    "mzreplay_make_batch": (ctypes.c_int, [c_void, ctypes.c_int32, c_i32_p, c_i32_p, c_i32_p, c_void, c_void, c_void,
                                           c_void, c_void, c_void, c_void]),
    "mzreplay_game_observations": (ctypes.c_int, [c_void, ctypes.c_int32, ctypes.c_int32, c_void, c_void]),
    "mzreplay_set_reanalysed": (ctypes.c_int, [c_void, ctypes.c_int32, c_void, ctypes.c_int32, c_void]),
    "mzreplay_device_bytes": (ctypes.c_int64, [c_void]),
    "mzreplay_sampler_enable": (ctypes.c_int, [c_void, ctypes.c_uint32, ctypes.c_int64]),
    "mzreplay_sampler_get_rng": (ctypes.c_int, [c_void, c_u32_p, c_i32_p]),
    "mzreplay_sampler_set_rng": (ctypes.c_int, [c_void, c_u32_p, ctypes.c_int32]),
    "mzreplay_set_priorities": (ctypes.c_int, [c_void, ctypes.c_int32, ctypes.c_int64, c_f32_p, ctypes.c_int32, c_void]),
    "mzreplay_get_priorities": (ctypes.c_int, [c_void, ctypes.c_int32, c_f32_p, c_f32_p, c_i64_p, c_void]),
    "mzreplay_sample_batch": (ctypes.c_int, [c_void, ctypes.c_int32, ctypes.c_int64, ctypes.c_int32, ctypes.c_int64,
                                             ctypes.c_int32, c_void, c_void, c_void, c_void, c_void, c_void]),
    "mzreplay_make_batch_device": (ctypes.c_int, [c_void, ctypes.c_int32, c_void, c_void, c_void, c_void, c_void, c_void,
                                                  c_void, c_void, c_void, c_void]),
    "mzreplay_update_priorities": (ctypes.c_int, [c_void, ctypes.c_int32, c_void, c_void, c_void, c_void]),
    "mzreplay_read_games": (ctypes.c_int, [c_void, ctypes.c_int32, c_i32_p, c_i32_p, c_f32_p, c_i32_p, c_f64_p, c_i32_p,
                                           c_f64_p, c_f64_p, c_void]),
    "mzreplay_filer_create": (ctypes.c_int, [c_void, ctypes.c_int32, ctypes.POINTER(c_void)]),
    "mzreplay_filer_destroy": (None, [c_void]),
    "mzreplay_filer_begin": (ctypes.c_int, [c_void, c_void, c_void, c_void]),
    "mzreplay_filer_set_counters": (ctypes.c_int, [c_void, c_i64_p, c_void]),
    "mzreplay_filer_file": (ctypes.c_int, [c_void, c_void, c_void]),
    "mzreplay_filer_sync": (ctypes.c_int, [c_void, c_i32_p, ctypes.POINTER(c_void), ctypes.POINTER(c_void), c_i64_p, c_i64_p,
                                           c_void]),
    "mzreplay_filer_sync_ids": (ctypes.c_int, [c_void, c_i32_p, ctypes.POINTER(c_void), ctypes.POINTER(c_void),
                                               ctypes.POINTER(c_void), c_i64_p, c_void]),
    "mzreplay_filer_lengths": (ctypes.c_int, [c_void, c_i32_p, c_void]),
    "mzreplay_filer_priorities": (ctypes.c_int, [c_void, ctypes.c_int32, c_i32_p, c_f32_p, c_f32_p, c_void]),
    "mzreplay_outcomes_reference": (ctypes.c_int, [ctypes.c_int32, c_f64_p, ctypes.POINTER(ctypes.c_int8), c_f64_p, c_void]),
    "mzreplay_game_outcomes": (ctypes.c_int, [c_void, ctypes.c_int32, c_i32_p, c_void, c_void]),
    "mzreplay_filer_enable_outcomes": (ctypes.c_int, [c_void, ctypes.c_int32]),
    "mzreplay_filer_sync_outcomes": (ctypes.c_int, [c_void, c_i32_p, ctypes.POINTER(c_void)]),
    "mzreplay_reanalyse_enable": (ctypes.c_int, [c_void, ctypes.c_uint32]),
    "mzreplay_reanalyse_get_rng": (ctypes.c_int, [c_void, c_u32_p, c_i32_p]),
    "mzreplay_reanalyse_set_rng": (ctypes.c_int, [c_void, c_u32_p, ctypes.c_int32]),
    "mzreplay_reanalyse_plan": (ctypes.c_int, [c_void, ctypes.c_int32, ctypes.c_int64, ctypes.c_int32, c_i64_p, c_void, c_void,
                                               c_void, c_void]),
    "mzreplay_reanalyse_observations": (ctypes.c_int, [c_void, ctypes.c_int32, c_void, c_void, ctypes.c_int32, c_void, c_void]),
    "mzreplay_reanalyse_store": (ctypes.c_int, [c_void, ctypes.c_int32, c_void, c_void, c_void, c_void]),
    "mzreplay_read_reanalysed": (ctypes.c_int, [c_void, ctypes.c_int32, c_i32_p, c_f32_p, c_void, c_void]),
    "mzreplay_reanalyse_fc_configure": (ctypes.c_int, [c_void, ctypes.POINTER(MzFcDesc), ctypes.c_int32, c_void, ctypes.c_int64]),
    "mzreplay_reanalyse_fc": (ctypes.c_int, [c_void, ctypes.c_int32, c_void, c_void, c_void]),
    "mzreplay_reanalyse_fc_group_width": (ctypes.c_int32, []),
    "mzenv_create": (ctypes.c_int, [ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, c_u32_p, ctypes.POINTER(c_void)]),
    "mzenv_destroy": (None, [c_void]),
    "mzenv_last_error": (ctypes.c_char_p, [c_void]),
    "mzenv_shape": (ctypes.c_int, [c_void, c_i32_p, c_i32_p, c_i32_p]),
    "mzenv_reset": (ctypes.c_int, [c_void, c_void, c_void]),
    "mzenv_step": (ctypes.c_int, [c_void, c_void, c_void, c_void, c_void]),
    "mzenv_observe": (ctypes.c_int, [c_void, c_void, c_void, c_void, c_void, c_void]),
    "mzenv_set_opponent": (ctypes.c_int, [c_void, ctypes.c_int32, ctypes.c_int32, c_void, c_void]),
    "mzenv_step_opponent": (ctypes.c_int, [c_void] * 7),
    "mzenv_advance_opponent": (ctypes.c_int, [c_void] * 12),
    "mzenv_advance_paired": (ctypes.c_int, [c_void] * 12),
    "mzenv_set_boards": (ctypes.c_int, [c_void, c_void, c_void]),
    "mzenv_get_state": (ctypes.c_int, [c_void, c_void, c_void]),
    "mzenv_set_state": (ctypes.c_int, [c_void, c_void, c_void]),
    "mzenv_set_max_moves": (ctypes.c_int, [c_void, ctypes.c_int32]),
    "mzenv_game_moves": (ctypes.c_int, [c_void, c_void, c_void]),
    # the device frame stack (config.stacked_observations)
    "mzenv_stack_create": (ctypes.c_int, [ctypes.c_int32] * 6 + [ctypes.POINTER(c_void)]),
    "mzenv_stack_destroy": (None, [c_void]),
    "mzenv_stack_last_error": (ctypes.c_char_p, [c_void]),
    "mzenv_stack_floats": (ctypes.c_int64, [c_void]),
    "mzenv_stack_reset": (ctypes.c_int, [c_void] * 5),
    "mzenv_stack_push": (ctypes.c_int, [c_void] * 7),
    "mzmcts_rng_create": (c_void, [ctypes.c_uint32]),
    "mzmcts_rng_destroy": (None, [c_void]),
    "mzmcts_rng_reseed": (None, [c_void, ctypes.c_uint32]),
    "mzmcts_rng_next_u32": (ctypes.c_uint32, [c_void]),
    "mzmcts_rng_random_sample": (ctypes.c_double, [c_void]),
    "mzmcts_rng_choice": (ctypes.c_uint32, [c_void, ctypes.c_uint32]),
    "mzmcts_rng_choice_p_many": (None, [c_void, c_f64_p, ctypes.c_int32, ctypes.c_int32, c_i32_p]),
    "mzmcts_rng_choice_priorities": (ctypes.c_int32, [c_void, c_f32_p, ctypes.c_int32, c_f32_p]),
    "mzmcts_rng_choice_p": (ctypes.c_int32, [c_void, c_f64_p, ctypes.c_int32]),
    "mzmcts_rng_dirichlet": (None, [c_void, ctypes.c_double, ctypes.c_int32, c_f64_p]),
    "mzmcts_set_device_noise": (ctypes.c_int, [c_void, ctypes.c_int32]),
    "mzmcts_get_noise": (ctypes.c_int, [c_void, c_f64_p]),
    "mzmcts_device_libm": (ctypes.c_int, [c_f64_p, c_f64_p, ctypes.c_int64, c_f64_p, c_f64_p]),
    "mzmcts_device_sincos": (ctypes.c_int, [c_f64_p, ctypes.c_int64, c_f64_p, c_f64_p]),
    "mzmcts_device_dirichlet": (ctypes.c_int, [c_u32_p, ctypes.c_int32, ctypes.c_double, ctypes.c_int32, ctypes.c_int32,
                                               c_f64_p, c_u32_p]),
    "mzmcts_set_device_temperatures": (ctypes.c_int, [c_void, ctypes.c_int32]),
    "mzmcts_device_select_action": (ctypes.c_int, [c_u32_p, ctypes.c_int32, c_i32_p, ctypes.c_int32, c_f64_p, ctypes.c_int32,
                                                   c_i32_p, c_u32_p]),
    "mzmcts_device_numerics": (ctypes.c_int, [ctypes.c_int32, ctypes.c_uint64, ctypes.c_uint64, c_u64_p, c_u64_p, c_f64_p]),
    "mzmcts_rng_export": (None, [c_void, c_u32_p, c_i32_p, c_i32_p, c_f64_p]),
    "mzmcts_rng_import": (None, [c_void, c_u32_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_double]),
    "mzmcts_rng_select_action": (ctypes.c_int32, [c_void, c_i32_p, ctypes.c_int32, ctypes.c_double]),
}

_lib = None


class NativeLibraryError(RuntimeError):
    pass


def load():
    """Load libmzmcts.so and bind every prototype.  Raises if the extension has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise NativeLibraryError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950).  The MCTS engine has no Python fallback.")
    # PyTorch-ROCm ships its own libamdhip64 (same SONAME as /opt/rocm's).  It must be the one already
    # mapped when libmzmcts.so resolves its dependency: two HIP runtimes in one process do not see the
    # same devices / streams.  Importing torch first guarantees that.
    import torch  # noqa: F401
    lib = ctypes.CDLL(LIB_PATH)
    for name, (restype, argtypes) in PROTOTYPES.items():
        fn = getattr(lib, name)  # AttributeError here == header / library out of sync
        fn.restype = restype
        fn.argtypes = argtypes
    if lib.mzmcts_abi_version() != ABI_VERSION:
        raise NativeLibraryError("libmzmcts.so ABI version mismatch; rebuild the extension")
    _lib = lib
    return lib


def ptr(arr, typ):
    """ctypes pointer to a C-contiguous numpy array (or None)."""
    if arr is None:
        return None
    assert arr.flags["C_CONTIGUOUS"]
    return arr.ctypes.data_as(typ)


def check(lib, engine, rc):
    """Translate a C-ABI status into the reference's exception types / messages."""
    if rc == 0:
        return
    msg = lib.mzmcts_last_error(engine)
    msg = msg.decode() if msg else f"mzmcts error {rc}"
    if rc in (ERR_EMPTY_LEGAL, ERR_LEGAL_RANGE):
        raise AssertionError(msg)
    if rc == ERR_PLAYERS:
        raise NotImplementedError(msg)
    raise RuntimeError(msg)


def check_train(lib, rc, what, where="", reason=True, refusal=None):
    """Translate the status of a mztrain_* call (include/mztrain.h): RuntimeError "<what> failed (<rc>)<where>: <the
    library's last error>" (`reason=False`: the call leaves no error string, the text ends at <where>).  With `refusal`,
    status -1 -- a shape the library does not cover -- is NotImplementedError "<refusal>: <last error>"."""
    if rc == 0:
        return
    message = (lib.mzmcts_last_error(None) or b"").decode() if reason else ""
    if rc == -1 and refusal is not None:
        raise NotImplementedError(f"{refusal}: {message}")
    raise RuntimeError(f"{what} failed ({rc}){where}" + (f": {message}" if reason else ""))


class MzTowerHead(ctypes.Structure):
    """mzmcts_tower_head (include/mzmcts.h): a head computed inside a tower launch."""
    _fields_ = [("head", MzHeadDesc), ("out", c_void), ("layer", ctypes.c_int32), ("reserved", ctypes.c_int32)]


class MzHistMoves(ctypes.Structure):
    _fields_ = [("n_moves", ctypes.c_int32), ("num_simulations", ctypes.c_int32), ("moves_done", c_void),
                ("actions", c_void), ("actions_stride", ctypes.c_int64), ("visits", c_void),
                ("visits_stride", ctypes.c_int64), ("root_value_sum", c_void), ("root_value_sum_stride", ctypes.c_int64),
                ("legal", c_void), ("num_legal", c_void), ("rewards", c_void), ("done", c_void), ("obs_after", c_void),
                ("obs_next", c_void), ("to_play_after", c_void), ("to_play_next", c_void),
                ("legal_stride", ctypes.c_int64), ("num_legal_stride", ctypes.c_int64), ("played", c_void),
                ("slots", ctypes.c_int32), ("reset_obs", c_void)]


class MzReplayFileMoves(ctypes.Structure):
    """mzreplay_file_moves (include/mzreplay.h): a move batch in device memory, as the device filer reads it."""
    _fields_ = [("n_moves", ctypes.c_int32), ("num_simulations", ctypes.c_int32),
                ("actions", c_void), ("actions_stride", ctypes.c_int64), ("visits", c_void),
                ("visits_stride", ctypes.c_int64), ("root_value_sum", c_void), ("root_value_sum_stride", ctypes.c_int64),
                ("legal", c_void), ("legal_stride", ctypes.c_int64), ("num_legal", c_void),
                ("num_legal_stride", ctypes.c_int64), ("to_play", c_void), ("to_play_stride", ctypes.c_int64),
                ("to_play_last", c_void), ("rewards", c_void), ("done", c_void), ("obs_after", c_void),
                ("obs_next", c_void), ("players", ctypes.c_int32), ("reserved", ctypes.c_int32)]


class MzReplayGameOutcome(ctypes.Structure):
    """mzreplay_game_outcome (include/mzreplay.h): what one finished game reports, 40 bytes."""
    _fields_ = [("total_reward", ctypes.c_double), ("reward_of_player", ctypes.c_double * 2),
                ("value_sum", ctypes.c_double), ("value_count", ctypes.c_int32), ("reserved", ctypes.c_int32)]


# the same 40 bytes as a numpy record: arrays of outcomes cross the C ABI as this dtype
GAME_OUTCOME_DTYPE = np.dtype([("total_reward", np.float64), ("reward_of_player", np.float64, (2,)),
                               ("value_sum", np.float64), ("value_count", np.int32), ("reserved", np.int32)])


def outcomes_reference(rewards, to_play, root_values):
    """mzreplay_outcomes_reference: csrc/game_outcomes.h's rule for one game of n = len(root_values) moves on host arrays
    (rewards [n + 1], to_play [n + 1]); touches no device.  Returns a GAME_OUTCOME_DTYPE record."""
    rewards = np.ascontiguousarray(rewards, dtype=np.float64)
    to_play = np.ascontiguousarray(to_play, dtype=np.int8)
    root_values = np.ascontiguousarray(root_values, dtype=np.float64)
    n = len(root_values)
    if len(rewards) != n + 1 or len(to_play) != n + 1:
        raise ValueError("outcomes_reference: rewards and to_play hold one entry more than root_values")
    out = np.zeros(1, dtype=GAME_OUTCOME_DTYPE)
    lib = load()
    if lib.mzreplay_outcomes_reference(n, ptr(rewards, c_f64_p), ptr(to_play, ctypes.POINTER(ctypes.c_int8)),
                                       ptr(root_values, c_f64_p), out.ctypes.data) != 0:
        raise ValueError(lib.mzreplay_last_error(None).decode())
    return out[0]


class HostRng:
    """numpy legacy RandomState clone on the host (stand-alone stream of the C library)."""

    def __init__(self, seed=0):
        self._lib = load()
        self._h = self._lib.mzmcts_rng_create(int(seed) & 0xFFFFFFFF)

    def __del__(self):
        try:
            self._lib.mzmcts_rng_destroy(self._h)
        except Exception:
            pass

    def seed(self, seed):
        self._lib.mzmcts_rng_reseed(self._h, int(seed) & 0xFFFFFFFF)

    def next_u32(self):
        return self._lib.mzmcts_rng_next_u32(self._h)

    def random_sample(self):
        return self._lib.mzmcts_rng_random_sample(self._h)

    def choice(self, n):
        return self._lib.mzmcts_rng_choice(self._h, n)

    def choice_p(self, p):
        p = np.ascontiguousarray(p, dtype=np.float64)
        return self._lib.mzmcts_rng_choice_p(self._h, ptr(p, c_f64_p), len(p))

    def choice_p_many(self, p, count):
        p = np.ascontiguousarray(p, dtype=np.float64)
        out = np.zeros(count, dtype=np.int32)
        self._lib.mzmcts_rng_choice_p_many(self._h, ptr(p, c_f64_p), len(p), int(count), ptr(out, c_i32_p))
        return out

    def choice_priorities(self, priorities):
        """(index, float32 probability) of choice(n, p=priorities / sum(priorities)) with float32 probabilities."""
        pri = np.ascontiguousarray(priorities, dtype=np.float32)
        prob = ctypes.c_float()
        idx = self._lib.mzmcts_rng_choice_priorities(self._h, ptr(pri, c_f32_p), len(pri), ctypes.byref(prob))
        return idx, np.float32(prob.value)

    def dirichlet(self, alpha, k):
        out = np.zeros(k, dtype=np.float64)
        self._lib.mzmcts_rng_dirichlet(self._h, float(alpha), k, ptr(out, c_f64_p))
        return out

    def select_action(self, visits, temperature):
        v = np.ascontiguousarray(visits, dtype=np.int32)
        return self._lib.mzmcts_rng_select_action(self._h, ptr(v, c_i32_p), len(v), float(temperature))

    def get_state(self):
        key = np.zeros(624, dtype=np.uint32)
        pos, hg, g = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_double()
        self._lib.mzmcts_rng_export(self._h, ptr(key, c_u32_p), ctypes.byref(pos), ctypes.byref(hg),
                                    ctypes.byref(g))
        return ("MT19937", key, pos.value, hg.value, g.value)

    def set_state(self, state):
        key = np.ascontiguousarray(state[1], dtype=np.uint32)
        self._lib.mzmcts_rng_import(self._h, ptr(key, c_u32_p), int(state[2]), int(state[3]),
                                    float(state[4]))


class MzTowerLayer(ctypes.Structure):
    """include/mzmcts.h mzmcts_tower_layer"""
    _fields_ = [("packed", ctypes.c_void_p), ("scale", ctypes.c_void_p), ("shift", ctypes.c_void_p),
                ("const_table", ctypes.c_void_p), ("export_raw", ctypes.c_void_p), ("export_unit", ctypes.c_void_p),
                ("cin", ctypes.c_int32),
                ("relu", ctypes.c_int32), ("skip", ctypes.c_int32), ("reserved", ctypes.c_int32),
                ("gate", ctypes.c_void_p)]


def device_select_action(seeds, visits, temperature, draws=1):
    """mzmcts_device_select_action: stream s = numpy.random.seed(seeds[s]), then `draws` x SelfPlay.select_action on
    visits[s] ([N, n] by child slot) at temperature[s], all on the GPU with the move batches' sampler.
    Returns (slots int32 [N, draws], words uint32 [N])."""
    seeds = np.ascontiguousarray(seeds, dtype=np.uint32)
    visits = np.ascontiguousarray(visits, dtype=np.int32)
    n_streams, n = visits.shape
    temps = np.ascontiguousarray(np.broadcast_to(np.asarray(temperature, dtype=np.float64), (n_streams,)))
    assert seeds.shape == (n_streams,)
    slots = np.zeros((n_streams, int(draws)), dtype=np.int32)
    words = np.zeros(n_streams, dtype=np.uint32)
    rc = load().mzmcts_device_select_action(ptr(seeds, c_u32_p), n_streams, ptr(visits, c_i32_p), n, ptr(temps, c_f64_p),
                                            int(draws), ptr(slots, c_i32_p), ptr(words, c_u32_p))
    if rc != 0:
        raise RuntimeError(f"mzmcts_device_select_action failed ({rc})")
    return slots, words


NUMERICS = {"exp": 1, "reciprocal": 2, "inverse_transform": 3, "quotient": 4, "normalized": 5, "quotient_guarded": 6,
            "plain_range": 7, "log": 8, "pow_half": 9, "pow_one": 10}
NUMERICS_MAX_COUNT = 1 << 28


def device_numerics(which, first, count):
    """mzmcts_device_numerics over the patterns first .. first + count - 1 of check `which` (a NUMERICS key), walked in
    calls of at most NUMERICS_MAX_COUNT.  Returns (mismatches, offending patterns (up to 8 per call), worst distance);
    stops at the first call that does not return MZMCTS_OK."""
    lib, code = load(), NUMERICS[which]
    mismatches, bad, worst = 0, [], 0.0
    n_bad, w = ctypes.c_uint64(), ctypes.c_double()
    patterns = (ctypes.c_uint64 * 8)()
    done = 0
    while done < count:
        step = min(NUMERICS_MAX_COUNT, count - done)
        rc = lib.mzmcts_device_numerics(code, first + done, step, ctypes.byref(n_bad), patterns, ctypes.byref(w))
        if rc != 0:
            raise RuntimeError(f"mzmcts_device_numerics({which}, {first + done}, {step}) failed ({rc})")
        mismatches += n_bad.value
        bad += [int(p) for p in patterns[:min(8, n_bad.value)]]
        worst = max(worst, w.value)
        done += step
    return mismatches, bad, worst


def exact_inverse_temperature(temperature):
    """k when 1 / temperature is an integer k in 1..4 (the temperatures the device sampler handles exactly:
    csrc/np_legacy_rng.h exact_inverse_temperature), else 0."""
    if temperature in (0, float("inf")) or temperature != temperature:
        return 0
    inv = 1.0 / float(temperature)
    k = int(inv)
    return k if inv == k and 1 <= k <= 4 else 0
