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
 * keep both with PyTorch-ROCm but for the convolution epilogue in training (mztrain_epilogue_*, below, on request); the
 * optimizer stays there too unless the caller asks for mztrain_opt_step (below) on the
 * flat buffers of a fully-connected network.  Raw device pointers, fp32, contiguous; no torch types.
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

#ifdef __cplusplus
}
#endif
#endif
