/* mztrain.h -- C ABI of the trainer-side HIP kernels (libmzmcts.so), SURVEY.md section 8(f) row 4.
 *
 * One entry: the loss of Trainer.update_weights (reference trainer.py:176-215 and loss_function, trainer.py:271-291)
 * over ALL unrolled steps of a batch in one launch -- the two-hot value / reward targets (models.scalar_to_support,
 * models.py:665-685), the three cross-entropies per step, their sums over the steps in the reference's order, the
 * per-sample total with the value-loss weight and the PER importance weight, the new PER priorities
 * (|support_to_scalar(value logits) - target value| ** PER_alpha, trainer.py:199-209) and the gradient of the total
 * with respect to every logit (each unrolled step's share divided by its gradient scale, trainer.py:176-198).
 * It replaces the ~25 element-wise launches per unrolled step between the network's forward and backward.  For
 * fully-connected networks the forward and the backward are HIP launches too (mztrain_fc_*, below); residual networks
 * keep both with PyTorch-ROCm but for the convolution epilogue in training (mztrain_epilogue_*, below, on request) and the
 * 3 x 3 convolutions with their two gradients (mztrain_conv_*, below, on request) and the three heads (mztrain_heads_*,
 * below, on request) and the backward of the hidden state's min-max rescale (mztrain_rescale_*, below, on request); the
 * optimizer stays there too unless the caller asks for mztrain_opt_step (below) on the
 * flat buffers of a fully-connected network, or for mztrain_fold_step (below), which folds a residual network's weight
 * gradients and applies the same rule in one launch.  Raw device pointers, fp32, contiguous; no torch types.
 *
 * Domain.  Value and reward logits of loss-bearing positions are finite; a `-inf` entry outside the two target entries
 * does not contribute (the two-hot cross-entropy reads the logits at the two target entries only, where the reference's
 * sum over all F entries would meet 0 * -inf = NaN).  Step 0's reward row is never read and may hold anything, NaN
 * included.  Policy rows follow the reference entry by entry: a positive target on a `-inf` logit gives a +inf loss, a
 * zero target on one gives NaN, and both stay within their sample.
 */
#ifndef MZTRAIN_H
#define MZTRAIN_H
#include <stdint.h>

#include "mzmcts.h"
#ifdef __cplusplus
extern "C" {
#endif

typedef struct mztrain_loss_args {
    const float *value_logits;   /* [K1][B][F]  step-major stack of the unroll's value logits, F = 2 support + 1 */
    const float *reward_logits;  /* [K1][B][F]  (step 0's row is ignored: no reward is predicted for the root)  */
    const float *policy_logits;  /* [K1][B][A] */
    const float *target_value;   /* [B][K1]     scalar targets (ReplayBuffer.make_target)                       */
    const float *target_reward;  /* [B][K1] */
    const float *target_policy;  /* [B][K1][A] */
    const float *gradient_scale; /* [B][K1] */
    const float *weight;         /* [B] PER importance-sampling weights, or NULL (config.PER off)               */
    int32_t batch;               /* B  */
    int32_t steps;               /* K1 = num_unroll_steps + 1 */
    int32_t support_size;
    int32_t actions;             /* A  */
    float value_loss_weight;
    float per_alpha;
    float *sample_loss;   /* out [B]      (value sum * value_loss_weight + reward sum + policy sum) * weight         */
    float *head_sums;     /* out [3][B]   per-sample sums over the steps of the value / reward / policy losses      */
    float *priorities;    /* out [B][K1] */
    float *grad_value;    /* out [K1][B][F]  d(sample_loss[b]) / d(value_logits[k][b][:]), gradient scale applied    */
    float *grad_reward;   /* out [K1][B][F]  (zeros for step 0) */
    float *grad_policy;   /* out [K1][B][A] */
} mztrain_loss_args;

/* Queues the launch on `stream` (hipStream_t); 0 = ok, < 0 = error (MZMCTS_ERR_*).  Refused with MZMCTS_ERR_INVALID before
 * anything touches a device: a null `args`, a null pointer among its members (`weight` alone may be null), and a
 * non-positive batch, steps, support_size or actions (support_size = 0, a one-entry support, is refused too). */
int mztrain_unroll_loss(const mztrain_loss_args *args, void *stream);

/* ---- the training step of a fully-connected network (csrc/fc_train.hip, csrc/fc_backward.h) ----------------------------
 * Four launches queued on the caller's stream, no allocation, no host decision, no synchronisation (capturable):
 *   forward   a lane group of 16 per sample walks its K1 positions with the search's own fc_initial / fc_recurrent,
 *             writes the logits step-major and saves per position what the backward reads
 *   loss      mztrain_unroll_loss on those logits
 *   backward  the same lane group walks k = K1-1 .. 0: the gradient of every layer's pre-activation (csrc/fc_backward.h)
 *   weights   every entry of `grads` = sum over (b, k), b-major, of delta * input: exact float64 products accumulated in
 *             float64 in one fixed order, rounded once; no atomics, the same bits from run to run, every entry written
 * `grads` is the gradient of mean_b(sample_loss[b]) in the layout of `weights` (every Linear's weight then bias in
 * state_dict order, as mzmcts_fc_configure).  Both pointers are retained.  Messages through mzmcts_last_error(NULL). */
typedef struct mztrain_fc mztrain_fc;

typedef struct mztrain_fc_args {
    const float *observations;   /* [B][obs]  the (stacked) observations of the root positions */
    const int64_t *actions;      /* [B][K1]   column k is the action of unroll step k (column 0 is unread); an action
                                              outside [0, A) is an all-zero one-hot */
    const float *target_value;   /* the seven batch pointers and the three outputs of mztrain_loss_args */
    const float *target_reward;
    const float *target_policy;
    const float *gradient_scale;
    const float *weight;         /* or NULL */
    int32_t batch;               /* B  <= max_batch */
    int32_t steps;               /* K1 <= max_steps */
    float value_loss_weight;
    float per_alpha;
    float *sample_loss;          /* out [B] */
    float *head_sums;            /* out [3][B] */
    float *priorities;           /* out [B][K1] */
} mztrain_fc_args;

/* weights / grads: dev f32[n_weights].  MZMCTS_ERR_INVALID before anything touches a device: a null pointer, a
 * non-positive actions, support_size, max_batch or max_steps, build_fc_net's refusals (layer sizes, n_weights), a
 * network whose weights and per-group activations do not fit a workgroup's 160 KB of LDS, and max_batch * max_steps
 * beyond int32 (the kernels count the positions b * K1 + k in int32). */
int mztrain_fc_create(const mzmcts_fc_desc *desc, int32_t actions, int32_t support_size, const float *weights,
                      int64_t n_weights, float *grads, int32_t max_batch, int32_t max_steps, int32_t device,
                      mztrain_fc **out);
void mztrain_fc_destroy(mztrain_fc *handle);
int64_t mztrain_fc_workspace_bytes(const mztrain_fc *handle);   /* device memory the handle owns; -1 for a null handle */
/* MZMCTS_ERR_INVALID before anything touches a device: a null handle, `args` or member (`weight` alone may be null),
 * non-positive batch or steps, batch or steps above the created maxima. */
int mztrain_fc_step(mztrain_fc *handle, const mztrain_fc_args *args, void *stream);
/* The last step's logits inside the workspace: value [K1][B][F], reward [K1][B][F] (step 0's row unspecified), policy
 * [K1][B][A], with the B and K1 of that step. */
int mztrain_fc_logits(const mztrain_fc *handle, const float **value_logits, const float **reward_logits,
                      const float **policy_logits);

/* ---- the optimizer's step on the flat buffers (csrc/fc_optimizer.hip, csrc/fc_optimizer.h) ------------------------------
 * Adam (torch's non-AMSGrad, coupled weight decay) or SGD (dampening 0, no Nesterov) on one flat float32 weight buffer and
 * one flat gradient buffer: the rule of csrc/fc_optimizer.h, every fused multiply-add spelled out, the per-step scalars in
 * float64 with glibc's pow, so that the device and mztrain_opt_reference on the host give the same bits.  No handle: the
 * caller owns every buffer. */
#define MZTRAIN_OPT_ADAM 0
#define MZTRAIN_OPT_SGD 1

typedef struct mztrain_opt_args {
    int32_t kind;            /* MZTRAIN_OPT_ADAM / MZTRAIN_OPT_SGD */
    int64_t n;               /* floats in each flat buffer */
    float *weights;          /* dev f32[n], updated in place */
    const float *grads;      /* dev f32[n] */
    float *moment1;          /* dev f32[n]: Adam exp_avg / SGD momentum buffer (may be NULL for SGD with momentum 0) */
    float *moment2;          /* dev f32[n]: Adam exp_avg_sq (NULL for SGD) */
    const double *lr;        /* dev f64[1]: this step's learning rate, filled by the caller */
    int64_t *steps_done;     /* dev i64[1]: Adam's t - 1; advanced by one per call, on the device */
    double beta1, beta2, eps, weight_decay, momentum;
} mztrain_opt_args;

/* Queues two launches on `stream` (the update, then a one-thread launch that advances steps_done: every element of a step
 * sees the same count), no allocation, no host decision, no synchronisation (capturable).  Writes exactly [0, n) of
 * `weights` and of the moments the kind uses; reads `grads`.  MZMCTS_ERR_INVALID with a message through
 * mzmcts_last_error(NULL) before anything touches a device: null `args`; a null weights, grads, lr or steps_done; a null
 * moment1 or moment2 for Adam, a null moment1 for SGD with momentum != 0; n <= 0; an unknown kind; beta1 or beta2 outside
 * [0, 1) and eps <= 0 (Adam); a negative or non-finite weight_decay or momentum. */
int mztrain_opt_step(const mztrain_opt_args *args, void *stream);
/* The same rule, and the same refusals, with every pointer a HOST array: what the tests hold the kernel to. */
int mztrain_opt_reference(const mztrain_opt_args *args);
/* Adam's per-step scalars {bc1, bc2, step_size, bc2s} of step t >= 1 as the kernel forms them (float64), into out[4]. */
int mztrain_opt_scalars(double lr, double beta1, double beta2, int64_t t, double *out);

/* ---- weight gradients folded and the optimizer applied in one launch (csrc/grad_fold.hip, csrc/grad_fold.h) ---------------
 * For networks whose parameters are used several times in a step (a residual network's dynamics and prediction networks,
 * once per unrolled position): every use writes its weight gradient into a SLOT of one staging buffer, and one launch per
 * step folds each parameter's slots in ascending order -- plain float32 additions, the order in which autograd's
 * AccumulateGrad would have summed them --, writes the sum into the flat gradient buffer and applies the rule of
 * mztrain_opt_step to the parameter.  A segment is one parameter tensor.  A segment with uses == 0 is left alone (weights,
 * moments, gradient); slots at index uses or above are never read; floats of the flat buffers outside every segment (batch
 * norm statistics, padding) are never written, so weight decay does not reach them. */
typedef struct mztrain_fold_segment {
    int64_t offset;          /* first float of the tensor in the flat weight / moment / gradient buffers */
    int64_t count;           /* floats of the tensor */
    int64_t slot_base;       /* first float of slot 0 in the staging buffer */
    int64_t slot_stride;     /* floats between two slots: >= count, a multiple of 4 */
    int32_t capacity;        /* slots the staging buffer holds for the tensor */
    int32_t reserved;
} mztrain_fold_segment;

typedef struct mztrain_fold_args {
    mztrain_opt_args opt;    /* as mztrain_opt_step reads it, n = floats of each flat buffer -- but `grads` is WRITTEN here:
                                the folded gradient of every segment with uses >= 1 */
    const float *staging;    /* dev f32[staging_floats]: the slots */
    int64_t staging_floats;
} mztrain_fold_args;

typedef struct mztrain_fold mztrain_fold;

/* The handle keeps the segment list, the chunk table of the launch and the per-segment uses on `device`.  Refused with
 * MZMCTS_ERR_INVALID and a message through mzmcts_last_error(NULL) before anything touches a device: a null `segments` or
 * `out`; n_segments <= 0; n or staging_floats <= 0; a count <= 0; a segment outside [0, n) or one that overlaps another; a
 * slot_stride below count or not a multiple of 4; a capacity < 1; slots [0, capacity) outside [0, staging_floats). */
int mztrain_fold_create(const mztrain_fold_segment *segments, int32_t n_segments, int64_t n, int64_t staging_floats,
                        int32_t device, mztrain_fold **out);
void mztrain_fold_destroy(mztrain_fold *handle);
/* The slots written per segment from now on.  Synchronous (waits for the device before and after the upload): not for a
 * stream capture.  Refused: a null handle or `uses`, another n_segments than the handle's, a uses[k] outside [0, capacity]. */
int mztrain_fold_set_uses(mztrain_fold *handle, const int32_t *uses, int32_t n_segments);
/* Queues two launches on `stream` (the fold and update, then the one-thread launch of mztrain_opt_step that advances
 * steps_done); no allocation, no host decision beyond the alignment of the base pointers, no synchronisation (capturable).
 * 16 bytes per lane where a segment's offset and slot_base are multiples of 4 and every base pointer is 16-byte aligned,
 * scalar accesses otherwise.  Refused before anything touches a device: a null handle, `args` or staging; the refusals of
 * mztrain_opt_step on `opt`; an opt.n that is not the handle's n; staging_floats below the handle's; uses never set. */
int mztrain_fold_step(mztrain_fold *handle, const mztrain_fold_args *args, void *stream);
/* The same rule, and the refusals of create, set_uses and step, with every pointer a HOST array: what the tests hold the
 * launch to. */
int mztrain_fold_reference(const mztrain_fold_segment *segments, const int32_t *uses, int32_t n_segments,
                           const mztrain_fold_args *args);
/* The launch's plan into out[4] = {chunks, grid, block, floats of a full chunk}, and with `chunks` non-null (room for
 * max_chunks entries) every chunk as {segment, first element within it, count, 1 where it may move 16 bytes per lane}.
 * create's refusals; MZMCTS_ERR_INVALID (and zeros) for a null `out` or max_chunks below the plan's. */
int mztrain_fold_plan(const mztrain_fold_segment *segments, int32_t n_segments, int64_t n, int64_t staging_floats,
                      int64_t *out, int64_t *chunks, int64_t max_chunks);

/* ---- the convolution epilogue of a residual network in training (csrc/bn_epilogue.hip, csrc/bn_epilogue.h) --------------
 * out = relu(batch_norm(x) [+ residual]) with the batch's own statistics, and its backward, one launch each: a workgroup
 * per channel, every sum over a channel in float64 in the one fixed order the header states, no atomics, the same bits from
 * run to run and as the host entries below.  x, residual, out, dy, dx, dresidual are NCHW float32, contiguous, hw = H * W;
 * a channel has M = batch * hw values.  No alignment beyond a float's is assumed. */
typedef struct mztrain_epilogue_forward_args {
    const float *x;          /* [batch][channels][hw] */
    const float *residual;   /* [batch][channels][hw], or NULL */
    const float *gamma;      /* [channels] batch norm's weight */
    const float *beta;       /* [channels] batch norm's bias */
    float *running_mean;     /* [channels] updated in place: (1 - momentum) * running + momentum * mean */
    float *running_var;      /* [channels] updated in place with the unbiased variance (sum of squares / (M - 1)) */
    float *out;              /* out [batch][channels][hw]; must not overlap x */
    float *save_mean;        /* out [channels] what the backward reads */
    float *save_invstd;      /* out [channels] 1 / sqrt(biased variance + eps) */
    int64_t batch;
    int32_t channels;
    int32_t hw;
    double eps;
    double momentum;
} mztrain_epilogue_forward_args;

typedef struct mztrain_epilogue_backward_args {
    const float *dy;          /* [batch][channels][hw] gradient of `out` */
    const float *x;           /* the forward's x */
    const float *out;         /* the forward's out: the ReLU mask is out > 0 */
    const float *gamma;
    const float *save_mean;
    const float *save_invstd;
    float *dx;                /* out [batch][channels][hw] */
    float *dresidual;         /* out [batch][channels][hw] (dy where out > 0, else 0), or NULL */
    float *dgamma;            /* out [channels] */
    float *dbeta;             /* out [channels] */
    int64_t batch;
    int32_t channels;
    int32_t hw;
} mztrain_epilogue_backward_args;

/* Each queues one launch on `stream`, no allocation, no host decision beyond the choice of the kernel's form by M, no
 * synchronisation (capturable).  MZMCTS_ERR_INVALID with a message through mzmcts_last_error(NULL) before anything touches
 * a device: null `args`; a null member (`residual` / `dresidual` alone may be null); channels < 1; batch or hw < 1;
 * M = batch * hw < 2; hw > 2^30 or M > 2^40; forward: a negative eps, a momentum outside [0, 1]. */
int mztrain_epilogue_forward(const mztrain_epilogue_forward_args *args, void *stream);
int mztrain_epilogue_backward(const mztrain_epilogue_backward_args *args, void *stream);
/* The same rule, and the same refusals, with every pointer a HOST array: what the tests hold the kernels to. */
int mztrain_epilogue_reference_forward(const mztrain_epilogue_forward_args *args);
int mztrain_epilogue_reference_backward(const mztrain_epilogue_backward_args *args);
/* M up to which a channel stays in LDS between the kernels' passes (the one switch of form). */
#define MZTRAIN_EPILOGUE_KEEP_VALUES 4096

/* ---- the 3 x 3 convolutions of a residual network in training (csrc/conv_train.hip, csrc/conv_train.h) ------------------
 * The padded, stride-1, bias-free 3 x 3 convolution on the boards of mzmcts_board_conv_supported (3 x 3, 6 x 6, 6 x 7; cout
 * 16 or 64; 1 <= cin <= 80), its data gradient and its weight gradient, exact float32 on v_mfma_f32_16x16x4_f32.  Forward and
 * data gradient run mzmcts_board_conv3x3 on two packings of the weight; the weight gradient is a kernel of its own.  The
 * order of every sum is csrc/conv_train.h's; the device entries and the reference entries give the same bits.
 *   forward   y = conv3x3(x, w), raw.  The launch path is the inference one with a ones / zeros scale / shift pair and no
 *             ReLU: y = acc * 1 + 0, so a sum of -0 comes out as +0, on the device and in the reference entry alike.
 *   dgrad     dx [batch][dx_planes][hw] = the gradient of x's FIRST dx_planes planes: conv3x3(dy, w') with
 *             w'[ci][co][ky][kx] = w[co][ci][2 - ky][2 - kx], ci < dx_planes (cin' = cout, cout' = dx_planes), the same -0 rule.
 *   wgrad     dw[co][ci][ky][kx] = sum over k = b * hw + p, ascending, of dy[b][co][p] * xpad[b][ci][p + (ky - 1, kx - 1)]:
 *             float32 fmaf chains from zero over slices of MZTRAIN_CONV_SLICE indices (the last one padded with 0 * 0
 *             terms), the slice sums added in ascending order in float64, one rounding.  No atomics; every entry of dw is
 *             written by every call; the same bits from run to run, eager and captured.
 * A border tap multiplies a float32 zero (a NaN dy or weight there gives NaN).  All tensors float32, contiguous. */
#define MZTRAIN_CONV_SLICE 64
#define MZTRAIN_CONV_AFFINE 64      /* floats of each half of `affine`: ones, then zeros */

typedef struct mztrain_conv_pack_args {
    const float *weight;     /* [cout][cin][3][3] */
    float *packed;           /* out f32[mzmcts_board_conv_packed_floats(cin, cout)]: the layout of mzmcts_board_conv_pack */
    float *packed_dx;        /* out f32[mzmcts_board_conv_packed_floats(cout, dx_planes)]: that layout for w'; NULL with
                                dx_planes == 0 */
    float *affine;           /* out f32[2 * MZTRAIN_CONV_AFFINE]: the ones | zeros pair the two convolutions read */
    int32_t cin;
    int32_t cout;
    int32_t dx_planes;       /* 0 (no data gradient wanted), 16 or 64, at most cin */
} mztrain_conv_pack_args;

typedef struct mztrain_conv_forward_args {
    const float *x;          /* [batch][cin][hw] */
    const float *packed;     /* what mztrain_conv_pack wrote (the launch reads these two) */
    const float *affine;
    const float *weight;     /* [cout][cin][3][3] (the reference entry reads this one instead) */
    float *y;                /* out [batch][cout][hw]; must not be x */
    int64_t batch;
    int32_t cin;
    int32_t cout;
    int32_t height;
    int32_t width;
} mztrain_conv_forward_args;

typedef struct mztrain_conv_dgrad_args {
    const float *dy;         /* [batch][cout][hw] */
    const float *packed_dx;  /* what mztrain_conv_pack wrote (the launch reads these two) */
    const float *affine;
    const float *weight;     /* [cout][cin][3][3] (the reference entry reads this one instead) */
    float *dx;               /* out [batch][dx_planes][hw]; must not be dy */
    int64_t batch;
    int32_t cin;
    int32_t cout;
    int32_t height;
    int32_t width;
    int32_t dx_planes;       /* 16 or 64, at most cin */
} mztrain_conv_dgrad_args;

typedef struct mztrain_conv_wgrad_args {
    const float *x;          /* [batch][cin][hw] */
    const float *dy;         /* [batch][cout][hw] */
    float *dw;               /* out [cout][cin][3][3] */
    int64_t batch;
    int32_t cin;
    int32_t cout;
    int32_t height;
    int32_t width;
} mztrain_conv_wgrad_args;

/* 1 where the three launches take the shape: the forward shapes of mzmcts_board_conv_supported that mzmcts_board_conv3x3
 * launches (with cout 16 its workgroup's planes fit 160 KB of LDS up to cin 48 on 3 x 3 boards, 32 on 6 x 6, 64 on 6 x 7), and
 * for need_dx_planes > 0 a data gradient of exactly 16 or 64 planes, at most cin, whose convolution cout -> need_dx_planes is
 * such a shape too (need_dx_planes == 0: no data gradient is asked for). */
int mztrain_conv_supported(int32_t cin, int32_t cout, int32_t height, int32_t width, int32_t need_dx_planes);
int32_t mztrain_conv_slice(void);                                  /* MZTRAIN_CONV_SLICE as the library was built */
/* the largest batch the entries take (batch * hw * max(cin, cout) + MZTRAIN_CONV_SLICE within int32); -1: unsupported shape */
int64_t mztrain_conv_max_batch(int32_t cin, int32_t cout, int32_t height, int32_t width);
/* the weight gradient's launch plan into out[5] = {grid, block, LDS bytes, slices per block, rounds}; MZMCTS_ERR_INVALID
 * (and zeros) for an unsupported shape or a batch outside [1, mztrain_conv_max_batch] */
int mztrain_conv_wgrad_plan(int64_t batch, int32_t cin, int32_t cout, int32_t height, int32_t width, int64_t *out);

/* Each queues one launch on `stream`, no allocation, no host decision beyond the choice of the launch's form, no
 * synchronisation (capturable); pack writes both packings and `affine` in its one launch, into buffers the caller keeps
 * (a captured step repacks on replay).  MZMCTS_ERR_INVALID with a message through mzmcts_last_error(NULL) before anything
 * touches a device: null `args`; a null member a launch reads or writes (`weight` may be null for the launches, `packed`,
 * `packed_dx` and `affine` for the reference entries, `packed_dx` for a pack with dx_planes == 0); an unsupported shape;
 * batch < 1 or above mztrain_conv_max_batch; dx_planes not 16 or 64 (pack: or 0), or above cin; y == x or dx == dy; x, y,
 * dy, dx, packed or packed_dx not 16-byte aligned (forward and dgrad launches: they move 16 bytes per lane). */
int mztrain_conv_pack(const mztrain_conv_pack_args *args, void *stream);
int mztrain_conv_forward(const mztrain_conv_forward_args *args, void *stream);
int mztrain_conv_dgrad(const mztrain_conv_dgrad_args *args, void *stream);
int mztrain_conv_wgrad(const mztrain_conv_wgrad_args *args, void *stream);
/* The same rule, and the same refusals but for alignment, with every pointer a HOST array: what the tests hold the
 * kernels to. */
int mztrain_conv_reference_pack(const mztrain_conv_pack_args *args);
int mztrain_conv_reference_forward(const mztrain_conv_forward_args *args);
int mztrain_conv_reference_dgrad(const mztrain_conv_dgrad_args *args);
int mztrain_conv_reference_wgrad(const mztrain_conv_wgrad_args *args);

/* ---- the reward / value / policy heads of a residual network in training (csrc/head_train.hip, csrc/head_train.h) -------
 * One call of models.conv_heads: n_heads (1 or 2) heads in the layout of mzmcts_head_desc -- 1 x 1 convolution with bias,
 * flatten (i = r * plane + p), Linear, ELU with alpha 1, Linear -- read ONE x [batch][channels][plane]; all heads of a call
 * share channels and plane.  The order of every sum is csrc/head_train.h's.
 *   forward   one launch, a workgroup per sample: the logits of every head, and what the backward does not recompute: the
 *             flattened convolution output `flat` and the fc1 pre-activation `pre`, into buffers of the caller's.
 *   backward  two launches.  Per sample: dlogits -> dh -> dpre = dh * elu'(pre) -> dflat -> dx; dx is one chain over all
 *             heads of the call, written once (not accumulated into), and skipped with dx == NULL; dpre and dflat go to
 *             caller-owned buffers that the second launch reads.  Reduction: the six parameter gradients of each head, every
 *             entry 16 float64 partial sums over interleaved samples (for the convolution: samples and positions) folded in
 *             ascending order and rounded once.  A NULL gradient pointer: that gradient is not computed.  No atomics, nothing
 *             that has to be zeroed; every entry of every wanted output is written by every call; the same bits from run to
 *             run, eager and captured.
 * Host and device: bit for bit the same where no fc1 pre-activation is negative; with negative ones ELU goes through expm1f
 * (its derivative through expf), whose bits differ between a host libm and the device's: each ELU output and each derivative
 * agrees within MZTRAIN_HEADS_ELU_ULPS float32 ulps, and what follows them within what that perturbation propagates to
 * (csrc/head_train.h).  No alignment beyond a float's is assumed. */
#define MZTRAIN_HEADS_MAX 2
#define MZTRAIN_HEADS_ELU_ULPS 4
#define MZTRAIN_HEADS_MAX_BATCH 65536

typedef struct mztrain_heads_forward_args {
    const float *x;                              /* [batch][channels][plane] */
    mzmcts_head_desc heads[MZTRAIN_HEADS_MAX];   /* the first n_heads are read */
    float *logits[MZTRAIN_HEADS_MAX];            /* out [batch][outputs] */
    float *flat[MZTRAIN_HEADS_MAX];              /* out [batch][reduced * plane] */
    float *pre[MZTRAIN_HEADS_MAX];               /* out [batch][hidden] */
    int64_t batch;
    int32_t n_heads;
} mztrain_heads_forward_args;

typedef struct mztrain_heads_grads {             /* one head's parameter gradients, in the shapes of the parameters */
    float *conv_w, *conv_b, *fc1_w, *fc1_b, *fc2_w, *fc2_b;    /* out; each may be NULL */
} mztrain_heads_grads;

typedef struct mztrain_heads_backward_args {
    const float *x;                              /* the forward's x */
    mzmcts_head_desc heads[MZTRAIN_HEADS_MAX];
    const float *dlogits[MZTRAIN_HEADS_MAX];     /* [batch][outputs] */
    const float *flat[MZTRAIN_HEADS_MAX];        /* what the forward wrote */
    const float *pre[MZTRAIN_HEADS_MAX];
    float *dpre[MZTRAIN_HEADS_MAX];              /* out [batch][hidden]: the per-sample launch writes, the reduction reads */
    float *dflat[MZTRAIN_HEADS_MAX];             /* out [batch][reduced * plane] */
    float *dx;                                   /* out [batch][channels][plane], or NULL */
    mztrain_heads_grads grads[MZTRAIN_HEADS_MAX];
    int64_t batch;
    int32_t n_heads;
} mztrain_heads_backward_args;

/* 1 where the launches take the shape (per head; all heads of a call must pass): n_heads 1 or 2, channels in [1, 256], plane
 * in [1, 128], reduced in [1, 16], hidden in [1, 128], outputs in [1, 256]; batches up to MZTRAIN_HEADS_MAX_BATCH.  0
 * otherwise, with the reason through mzmcts_last_error(NULL). */
int mztrain_heads_supported(int32_t channels, int32_t plane, int32_t reduced, int32_t hidden, int32_t outputs, int32_t n_heads);
/* Forward queues one launch, backward two, on `stream`; no allocation, no host decision beyond the grid sizes, no
 * synchronisation (capturable).  MZMCTS_ERR_INVALID with a message through mzmcts_last_error(NULL) before anything touches a
 * device: null `args`; a null member of a head in use (`dx` and the members of `grads` alone may be null); heads of
 * different channels or plane; a shape mztrain_heads_supported refuses; batch outside [1, MZTRAIN_HEADS_MAX_BATCH]. */
int mztrain_heads_forward(const mztrain_heads_forward_args *args, void *stream);
int mztrain_heads_backward(const mztrain_heads_backward_args *args, void *stream);
/* The same rule, and the same refusals, with every pointer a HOST array: what the tests hold the kernels to. */
int mztrain_heads_reference_forward(const mztrain_heads_forward_args *args);
int mztrain_heads_reference_backward(const mztrain_heads_backward_args *args);

/* ---- the hidden state's min-max rescale of a residual network in training (csrc/rescale_train.hip, csrc/rescale_train.h) -----
 * The backward of mzmcts_unit_rescale (include/mzmcts.h), which stays the forward: a row is one (sample, channel) plane of
 * row_len = H * W floats, y = (x - min) / s with s = max - min, + 1e-5 where that is below 1e-5.  One launch: lo, hi, s and y
 * are formed again from x by the forward's float32 operations (nothing but x is saved), the two sums over a row -- of g and
 * of g * y -- run in float64 in ascending order, ties at an extreme share its gradient evenly (torch's amin / amax), and
 * every grad_x entry is rounded to float32 once.  No atomics, nothing that has to be zeroed; every entry of grad_x is written
 * by every call; the same bits from run to run, eager and captured, and as the host entry.  A NaN in a row makes that row's
 * grad_x NaN and no other's.  grad_x may be grad_out.  No alignment beyond a float's is assumed. */
typedef struct mztrain_rescale_backward_args {
    const float *x;          /* [rows][row_len] the forward's input */
    const float *grad_out;   /* [rows][row_len] gradient of the forward's output */
    float *grad_x;           /* out [rows][row_len] */
    int64_t rows;            /* batch * channels */
    int32_t row_len;         /* H * W */
} mztrain_rescale_backward_args;

/* 1 where the launch takes the shape: row_len in [1, 128] (the bound of mzmcts_unit_rescale), rows >= 1, rows * row_len below
 * 2^31.  0 otherwise, with the reason through mzmcts_last_error(NULL). */
int mztrain_rescale_supported(int64_t rows, int32_t row_len);
/* Queues one launch on `stream`, no allocation, no host decision beyond the plan below, no synchronisation (capturable).
 * MZMCTS_ERR_INVALID with a message through mzmcts_last_error(NULL) before anything touches a device: null `args`; a null
 * member; a shape mztrain_rescale_supported refuses. */
int mztrain_rescale_backward(const mztrain_rescale_backward_args *args, void *stream);
/* The same rule, and the same refusals, with every pointer a HOST array: what the tests hold the kernel to. */
int mztrain_rescale_reference_backward(const mztrain_rescale_backward_args *args);
/* The launch's plan into out[5] = {grid, block, rows per workgroup, floats between two rows in LDS (odd), LDS bytes};
 * MZMCTS_ERR_INVALID (and zeros) for a null `out` or a shape mztrain_rescale_supported refuses. */
int mztrain_rescale_backward_plan(int64_t rows, int32_t row_len, int64_t *out);

#ifdef __cplusplus
}
#endif
#endif
