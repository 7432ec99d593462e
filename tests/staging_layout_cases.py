"""The search engine's five staging blocks as the code laid them out before csrc/staging_layout.h: the offset chains of
mzmcts_create (per-move upload, per-tree download), ensure_batch_capacity (move-batch control block and output ring) and
ensure_inputs_capacity (inputs ring), restated from those functions.  Each block: [(field, offset, element bytes, elements)]
in the order the chain places them, plus its size ("bytes") or per-move step ("stride").  tests/test_staging_layout_cpu.py
holds the header to it on the CPU, tests/test_gpu_moves.py the offsets the library reports on the GPU."""


def align256(v):
    return (v + 255) // 256 * 256


def align8(v):
    return (v + 7) // 8 * 8


def upload(E, A):
    o_legal = 0
    o_nlegal = o_legal + 4 * E * A
    o_to_play = o_nlegal + 4 * E
    o_skip = o_to_play + 4 * E
    o_noise = align8(o_skip + 4 * E)
    fields = [("legal", o_legal, 4, E * A), ("num_legal", o_nlegal, 4, E), ("to_play", o_to_play, 4, E), ("rng_skip", o_skip, 4, E),
              ("noise", o_noise, 8, E * A)]
    return dict(fields=fields, bytes=o_noise + 8 * E * A, bytes_no_noise=o_noise)


def download(E):
    o_rvs = 0
    o_mm = o_rvs + 8 * E
    o_ds = o_mm + 16 * E                                 # mz::MinMax: two doubles
    o_pred = o_ds + 8 * E
    o_md = o_pred + 4 * E
    o_tw = o_md + 4 * E
    o_nw = o_tw + 4 * E
    o_err = o_nw + 4 * E
    fields = [("root_value_sum", o_rvs, 8, E), ("min_max", o_mm, 16, E), ("depth_sum", o_ds, 8, E), ("root_predicted", o_pred, 4, E),
              ("max_depth", o_md, 4, E), ("tie_words", o_tw, 4, E), ("noise_words", o_nw, 4, E), ("error_flag", o_err, 4, 4)]
    return dict(fields=fields, bytes=o_err + 4 * 4)


def move_control(E, A, M):
    o_skip = align256(8 * M * E * A)
    o_temp = align256(o_skip + 4 * M * E)
    o_limit = align256(o_temp + 8 * E)
    o_expect = align256(o_limit + 4 * E)
    fields = [("noise", 0, 8, M * E * A), ("rng_skip", o_skip, 4, M * E), ("temperature", o_temp, 8, E), ("move_limit", o_limit, 4, E),
              ("expected_ties", o_expect, 4, E)]
    return dict(fields=fields, bytes=align256(o_expect + 4 * E))


def move_output(E, A):
    o_actions = 0
    o_visits = align256(4 * E)
    o_rvs = align256(o_visits + 4 * E * A)
    o_pred = align256(o_rvs + 8 * E)
    o_depth = align256(o_pred + 4 * E)
    o_ties = align256(o_depth + 4 * E)
    o_sample = align256(o_ties + 4 * E)
    o_dsum = align256(o_sample + 4 * E)
    fields = [("actions", o_actions, 4, E), ("visits", o_visits, 4, E * A), ("root_value_sum", o_rvs, 8, E), ("root_predicted", o_pred, 4, E),
              ("max_depth", o_depth, 4, E), ("tie_words", o_ties, 4, E), ("sample_words", o_sample, 4, E), ("depth_sum", o_dsum, 4, E)]
    return dict(fields=fields, stride=align256(o_dsum + 4 * E))


def move_inputs(E, A):
    o2_nlegal = 0
    o2_to_play = align256(4 * E)
    o2_words = align256(o2_to_play + 4 * E)
    o2_legal = align256(o2_words + 4 * E)
    fields = [("num_legal", o2_nlegal, 4, E), ("to_play", o2_to_play, 4, E), ("noise_words", o2_words, 4, E), ("legal", o2_legal, 4, E * A)]
    return dict(fields=fields, stride=align256(o2_legal + 4 * E * A))


def offsets(block):
    return {name: offset for name, offset, _, _ in block["fields"]}


# what mzmcts_moves_ring / mzmcts_moves_device_ring and mzmcts_moves_inputs_ring / _device_ring report (include/mzmcts.h)
def ring_offsets(E, A):
    o = offsets(move_output(E, A))
    return [o[k] for k in ("actions", "visits", "root_value_sum", "root_predicted", "max_depth")], move_output(E, A)["stride"]


def inputs_ring_offsets(E, A):
    o = offsets(move_inputs(E, A))
    return [o[k] for k in ("num_legal", "to_play", "legal")], move_inputs(E, A)["stride"]
