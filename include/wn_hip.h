/* libwn_hip.so -- C-ABI of the MI355X (gfx950) WaveNet training / generation hot path.
 *
 * Drop-in boundary for jirsat/wavenets (reference paths relative to /root/reference).  The
 * reference has no FFI: its boundary is the Keras class surface of src/layers.py
 * (WaveNetLayer) and src/model.py (WaveNet).  The Python mirror of those classes
 * (wavenets_amd/layers.py, wavenets_amd/model.py) binds exactly the entry points declared
 * here through ctypes; each one cites the reference method it replaces.
 *
 * Conventions
 *  - all tensors are device pointers to contiguous fp32 (or int32 where stated) buffers in the
 *    reference's channels-last layout (B, T, C); Conv1D kernels (k, C_in, C_out), Dense
 *    kernels (in, out), biases (C_out)                        [src/layers.py:134]
 *  - parameters / gradients / Adam moments are ONE flat fp32 buffer each, tensors in Keras
 *    creation order (causal; per block: dilated stack, conv1, conv_skip, conv_cond; final
 *    convs; mapping Dense stack) -- wn_plan_tensor_info() enumerates them
 *  - no function allocates or frees caller-visible memory: outputs, saved activations and
 *    scratch live in a caller-provided workspace of wn_plan_workspace_floats() floats
 *  - every launch is asynchronous on the given hipStream_t (passed as void*); no host sync
 *  - return value: 0 = ok, <0 = WN_E_* ; message via wn_last_error_string() (thread-local)
 */
#ifndef WN_HIP_H
#define WN_HIP_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define WN_OK 0
#define WN_E_INVALID (-1)      /* bad argument (the Python layer raises ValueError) */
#define WN_E_UNSUPPORTED (-2)  /* shape / option outside what the kernels cover */
#define WN_E_HIP (-3)          /* HIP runtime error */

/* activation ids (Keras activation strings used by the reference configs, train.py:35,38) */
#define WN_ACT_LINEAR 0
#define WN_ACT_RELU 1
#define WN_ACT_LEAKY_RELU 2
#define WN_ACT_TANH 3
#define WN_ACT_SIGMOID 4
#define WN_ACT_ELU 5

/* output head / sampling_function (src/model.py:65-69) */
#define WN_HEAD_CATEGORICAL 0
#define WN_HEAD_LOGISTIC 1
#define WN_HEAD_GAUSSIAN 2

#define WN_MAX_FINAL 8
#define WN_MAX_MAPPING 8

/* Mirror of the WaveNet constructor keywords, src/model.py:14-34 */
typedef struct wn_config {
  int32_t kernel_size;
  int32_t channels;
  int32_t blocks;
  int32_t layers_per_block;
  int32_t activation;           /* WN_ACT_* for non-gated convs and the head */
  int32_t dilation_bound;
  int32_t num_mixtures;         /* 0 = None */
  int32_t head;                 /* WN_HEAD_* */
  int32_t bits;
  int32_t skip_channels;        /* 0 = None */
  int32_t dilation_channels;    /* 0 = None (-> channels, src/layers.py:49-50) */
  int32_t use_residual;
  int32_t use_skip;
  int32_t n_final;              /* len(final_layers_channels) */
  int32_t final_channels[WN_MAX_FINAL];
  int32_t cond_inputs;          /* 0 = conditioning None; else width of the raw global condition */
  int32_t n_mapping;            /* len(mapping_layers) */
  int32_t mapping_channels[WN_MAX_MAPPING];
  int32_t mapping_activation;
  float l2_reg_factor;
} wn_config;

typedef struct wn_plan wn_plan;

const char* wn_last_error_string(void);

/* ---- plan (WaveNet.__init__ + build, src/model.py:14-211).  The network description inside a plan (shapes, dilation
 * schedule, tensor table, image layouts, workspace layouts) is immutable after wn_plan_create; device copies of its small
 * tables are made once, on first use, under a lock.  The per-caller launch state the calls below set and the entry
 * points read -- dropout counter (wn_plan_set_dropout), armed step-sample pointer (wn_plan_arm_step_sample), phase
 * selection (wn_plan_set_train_phases), side stream / events, measurement hooks (wn_prof_*, wn_stack_prof_*, wn_phase_*),
 * device-side job tables cached per (B, T) -- is NOT in the plan but in an execution state (wn_exec, below): the
 * plan's own by default, or the one the calling thread has bound.  The setters named wn_plan_* act on that state. ---- */
wn_plan* wn_plan_create(const wn_config* cfg);          /* NULL on error */
void wn_plan_destroy(wn_plan* p);

/* Execution state.  A wn_plan is immutable once created (configuration, tensor table, weight-image layouts, workspace
 * layouts) and may be shared by any number of host threads and streams.  What changes while a plan is
 * USED -- the dropout counter, the armed step sample, the phase selection, the weight-gradient job tables and generation
 * block table cached for the last (B, T) (device memory), the side stream and its events, the profiling events -- lives
 * in a wn_exec.  Every plan carries one of its own, used by callers that never bind another: the single-threaded use of
 * the reference (one Python thread drives everything, train.py:203-258) needs nothing below.  A caller that drives ONE
 * plan from several threads / streams creates one wn_exec per thread and binds it there; the binding is thread-local
 * and applies to calls on the plan the state was created for.  A new state copies the dropout setting and phase
 * selection the plan's own state has at that moment.  wn_exec_bind(NULL) unbinds. */
typedef struct wn_exec wn_exec;
wn_exec* wn_exec_create(const wn_plan* p);
void wn_exec_destroy(wn_exec* e);
int wn_exec_bind(wn_exec* e);
int64_t wn_plan_param_count(const wn_plan* p);
int32_t wn_plan_num_tensors(const wn_plan* p);
/* tensor idx in Keras creation order: flat offset, element count, rank, shape[3] */
int wn_plan_tensor_info(const wn_plan* p, int32_t idx, int64_t* offset, int64_t* len,
                        int32_t* ndim, int64_t* shape3, int32_t* is_kernel);
int32_t wn_plan_receptive_field(const wn_plan* p);      /* src/model.py:122 */
int32_t wn_plan_out_channels(const wn_plan* p);
int32_t wn_plan_dilation(const wn_plan* p, int32_t conv_index);   /* src/model.py:79-81 */
/* workspace size in floats for a (B, T) call; training != 0 keeps activations for backward */
int64_t wn_plan_workspace_floats(const wn_plan* p, int32_t B, int32_t T, int32_t training);

/* ---- Dropout(rate) on every block input in training calls (src/layers.py:108-111,195-196; WaveNet
 * keyword `dropout`).  The keep-mask is a counter-based hash of (seed, block, step, element); `step`
 * is used as given by every following training call: the CALLER owns the counter (the Python mirror sets
 * step = call_index * world_size + rank + 1 before each step, so that replicas draw independent masks as
 * under MirroredStrategy, and stores call_index in its checkpoints).  rate 0 disables. */
int wn_plan_set_dropout(wn_plan* p, float rate, uint64_t seed, uint64_t step);
uint32_t wn_dropout_key_for(uint64_t seed, int32_t block, uint64_t step);   /* test hook */

/* ---- measurement hook (bench.py): HIP events on the caller's stream around the residual-block
 * forward launches -- one pair around the whole chain when it is N back-to-back launches of the fused
 * block kernel (a pair per launch would time its own event packets too), else one pair per block;
 * wn_prof_read returns launches and the average per-launch time after a stream sync.
 * Not part of the reference surface. */
int wn_debug_set(int key, int value);     /* kernel-variant switches of the CALLING THREAD (list: csrc/wn_error.cpp);
                                             key 1 = 1 selects the exact-fp32 MFMA kernels */
int wn_debug_value(int key);              /* current value of a switch in the calling thread */
int wn_debug_gen_ts(unsigned long long* out_96); /* switch 24: s_memtime stamps [role 3][block 4][phase 8] of the last
                                             generation chain launch (profiling hook; -1 if none was taken) */
/* one line naming the kernel family every phase of a pass selects for this plan under the calling thread's switches */
int wn_plan_describe(const wn_plan* p, char* buf, int32_t len);
int wn_prof_enable(wn_plan* p, int32_t max_launches);
int wn_prof_read(wn_plan* p, int32_t* launches, float* avg_ms);
/* test / diagnosis hook: float offset and length, inside the caller's TRAINING workspace for (B, T), of an
 * intermediate the last wn_train_fwd_bwd left there (deferred weight-gradient layout, layers_per_block = 1).
 * what: 0 H[idx] | 1 Z[idx] | 2 saved sigmoid[idx] | 3 skip sum | 4 head activation[idx] | 5 logits |
 *       6 dL/d(final[idx] pre-activation) | 7 dL/d(skip sum) | 8 dL/du[idx] | 9 dL/dH[idx] | 10 max-abs slots |
 *       11 activated output of non-gated dilated conv i of block b, idx = b * (layers_per_block - 1) + i (any layout) |
 *       12 the per-row losses (B * T; overwritten by the L2 term's norms when l2_reg_factor > 0) |
 *       13 dL/d(pre-activation output of that conv): GP[b][i], idx and length (rows * D) as for 11 |
 *       14 XD[idx], the dropped copy of block input idx (rows * channels).  It exists only while the calling state's
 *          dropout rate is above 0; with dropout off it is WN_E_INVALID, like every other absent region */
int wn_debug_ws_region(const wn_plan* p, int32_t B, int32_t T, int32_t what, int32_t idx, int64_t* off,
                       int64_t* len);
/* the same for the INFERENCE workspace of (B, T) (wn_forward, wn_eval_loss, wn_score): what = 5 the logits (B * T * C_out;
 * untouched by a wn_score pass that formed the loss in the last conv's epilogue) | 12 the per-row losses (B * T).
 * Any other `what` is WN_E_INVALID. */
int wn_debug_eval_region(const wn_plan* p, int32_t B, int32_t T, int32_t what, int64_t* off, int64_t* len);
/* test / diagnosis hook, host only: which kernels a forward pass over (B, T) takes under the calling thread's switches,
 * for a call without dropout and without ring capture.  loss: 0 none | 1 the training loss epilogue wanted | 2 the
 * evaluation epilogue wanted.  One `name=value` token per decision, separated by blanks:
 *   cond=none|small|rows  conv_cond=none|batched|per_block  inconv=elementwise|rows  zfill=0|1  fold=0|1
 *   prep=none|inline|side  drop=0|1  deep16=0|1  skip=none|folded/planes|folded/rows|sum  first_final=<i>  hc0=<width>
 *   head=<epilogue|planes|rows of every head layer from first_final on, in order, comma separated> */
int wn_debug_fwd_paths(const wn_plan* p, int32_t B, int32_t T, int32_t training, int32_t loss, char* buf, int32_t len);
/* test / diagnosis hook, host only: which kernels block 0 takes in a model pass over (B, T) under the calling thread's
 * switches, without dropout -- the decisions the launches of the block's forward and (training != 0) backward read:
 *   inner=<planes|rows16|rows32 of every non-gated conv, in order, comma separated; none>
 *   gate=s128|two|fused16|fused32|composed
 *   go=xout|sum|skip  gu=fold|pad|image|fp32|zero  gu_pad=0|1  gu_am=<none|gxout|gskip|gfold>,<...>
 *   data=<planes|rows16|rows32 of the backward-data product of conv 1.., comma separated; none>
 *   gx=none|g16x|deep|fp32+absmax|fp32  drop=0|1 */
int wn_debug_block_paths(const wn_plan* p, int32_t B, int32_t T, int32_t training, char* buf, int32_t len);
/* the whole residual-block stack of a forward pass: one event pair per pass from the first block launch to
 * the end of the folded skip contraction = t_stack_fwd of SURVEY.md 8(d); read returns passes and the average */
int wn_stack_prof_enable(wn_plan* p, int32_t max_passes);
int wn_stack_prof_read(wn_plan* p, int32_t* passes, float* avg_ms);
/* the per-pass weight-space preparation of the folded skip path of the same passes (bias sum, V = W_s W_f0, fp16 images;
 * it runs before the first block launch, outside the pair above): average per pass, 0 when the plan does not fold */
int wn_stack_prof_read_foldprep(wn_plan* p, int32_t* passes, float* avg_ms);
/* phase marks of wn_train_fwd_bwd: ms4 = {forward, loss, backward-data chain, weight gradients + rest}
 * of the last call (read after a stream sync) */
int wn_phase_enable(wn_plan* p, int32_t on);
int wn_phase_read(wn_plan* p, float* ms4);

/* ---- WaveNet.call, src/model.py:213-239 ----
 * x (B,T,1); cond (B, cond_inputs) or NULL; out (B,T,C_out): probabilities (categorical) or
 * linear mixture parameters; logits_out optional (B,T,C_out) pre-softmax. */
int wn_forward(wn_plan* p, const float* params, const float* x, const float* cond, int32_t B,
               int32_t T, float* out, float* logits_out, float* workspace, int64_t ws_floats,
               void* stream);

/* WaveNet.call(inputs, training=True): the same forward with the Dropout layers active (src/layers.py:195-196),
 * mask of the step last set by wn_plan_set_dropout; workspace sized for training (wn_plan_workspace_floats(.., 1)) */
int wn_forward_training(wn_plan* p, const float* params, const float* x, const float* cond, int32_t B,
                        int32_t T, float* out, float* logits_out, float* workspace, int64_t ws_floats,
                        void* stream);

/* ---- gradient half of WaveNet.train_step, src/model.py:319-335 ----
 * x_full (B,T+1,1): inputs = x[:, :-1], targets = prepare_target(x[:, 1:]).
 * loss = sum_{b,t} l / global_batch (+ l2 * sum W^2 / n_replicas).  grads receives
 * d(loss)/d(params) for THIS replica's rows (to be SUM-all-reduced by the caller).
 * loss_out: 3 device floats {loss, reg_loss, range_flag}.  pred_out optional (B,T,C_out). */
int wn_train_fwd_bwd(wn_plan* p, const float* params, const float* x_full, const float* cond,
                     int32_t B, int32_t T, int32_t global_batch, int32_t n_replicas, float* grads,
                     float* loss_out, float* pred_out, float* workspace, int64_t ws_floats,
                     void* stream);

/* ---- Vector-Jacobian product of the network: the backward pass from a gradient the CALLER supplies (custom losses) ----
 * Must follow a wn_forward_training(p, params, x, cond, B, T, ..., workspace) on the SAME workspace, in the same thread
 * state (math mode, dropout rate / seed / step), with no other pass on that workspace in between: the saved activations
 * are read from there.
 * g_out (B,T,C_out): gradient w.r.t. what g_kind names: 0 = the output of WaveNet.call (probabilities for the
 * categorical head -- the softmax vector-Jacobian product q (g - <g, q>) is formed from the logits in the workspace --,
 * linear mixture parameters otherwise), 1 = the pre-softmax logits.  Plain fp32: a non-finite g_out gives non-finite
 * gradients.
 * grads: d<g_out, out>/d(params), the whole flat buffer, every tensor written (overwritten, not accumulated).
 * g_x (B,T,1) and g_cond (B,cond_inputs): the gradients at the input waveform and the condition; optional (NULL = not
 * formed).  Nothing of the built-in losses is added: no 1/global_batch, no L2 term.  wn_plan_set_train_phases and an
 * armed step sample do not apply.
 * WN_E_INVALID (checked before the device is touched): a null plan / params / x / g_out / grads / workspace, cond null
 * on a conditioned plan, B < 1 or T < 1, g_kind outside {0, 1}, g_cond on a plan without conditioning, a workspace
 * smaller than wn_plan_workspace_floats(p, B, T, 1). */
int wn_vjp(wn_plan* p, const float* params, const float* x, const float* cond, int32_t B, int32_t T,
           const float* g_out, int32_t g_kind, float* grads, float* g_x, float* g_cond,
           float* workspace, int64_t ws_floats, void* stream);

/* ---- WaveNet.test_step loss, src/model.py:362-381 (forward + loss only); loss_out: 3 device floats as above ---- */
int wn_eval_loss(wn_plan* p, const float* params, const float* x_full, const float* cond,
                 int32_t B, int32_t T, int32_t global_batch, float* loss_out, float* pred_out,
                 float* workspace, int64_t ws_floats, void* stream);

/* ---- per-utterance negative log-likelihoods in one evaluation pass (WaveNet.score) ----
 * Inputs and targets as wn_eval_loss: inputs = x[:, :-1], targets = prepare_target(x[:, 1:]); the inference forward (no
 * dropout) on the INFERENCE workspace, wn_plan_workspace_floats(p, B, T, 0).  l[b,t] is the per-row loss exactly as loss_fn
 * defines it for the head (the clipped cross entropy, or the mixture negative log-likelihood), in nats: no 1 / global_batch,
 * no L2 term.
 *   nll_out    B floats:   sum_t w[b,t] l[b,t]
 *   weight_out B floats:   sum_t w[b,t], exactly T when no weights are armed; NULL = not wanted
 *   rows_out   B*T floats: w[b,t] l[b,t] as the loss kernel stored it; NULL = not wanted
 *   flag_out   1 float:    the range flag, as loss_out[2] of wn_eval_loss (1: repeat the call with the exact-fp32 kernels)
 * Armed row weights (wn_plan_arm_row_weights) apply as they do to wn_eval_loss: rows are stored weighted, w == 0 is a select
 * (a row whose own loss is inf or NaN contributes +0), a row count other than B * T is WN_E_INVALID naming both numbers.
 * Each utterance is summed by one workgroup in double, without atomics, in an order that depends on T alone: nll_out[b] is
 * a function of utterance b's rows only, bit for bit, whatever B is and whatever the other rows hold.
 * A 256-class categorical head whose last conv the streamed kernel takes forms the rows in that conv's epilogue
 * (evaluation form: no logits and no d loss / d logits are written); every other head and shape, and the exact-fp32 mode,
 * run the standalone loss kernels on the logits.
 * WN_E_INVALID (checked before the device is touched): a null plan / params / x_full / nll_out / flag_out / workspace,
 * cond null on a conditioned plan, B < 1 or T < 1, a workspace smaller than the inference size (message: both sizes). */
int wn_score(wn_plan* p, const float* params, const float* x_full, const float* cond, int32_t B, int32_t T,
             float* nll_out, float* weight_out, float* rows_out, float* flag_out,
             float* workspace, int64_t ws_floats, void* stream);

/* ---- optimizer.apply_gradients with Adam(lr, clipnorm), train.py:225-226, model.py:336 ----
 * Keras Adam: alpha = lr*sqrt(1-b2^t)/(1-b1^t); p -= alpha*m/(sqrt(v)+eps); per-tensor
 * tf.clip_by_norm when clipnorm > 0.  step is 1-based.  scratch: >= num_tensors floats. */
int wn_adam_step(wn_plan* p, float* params, const float* grads, float* m, float* v, int64_t step,
                 float lr, float beta1, float beta2, float eps, float clipnorm, float* scratch,
                 void* stream);
/* the same update, skipped on the device when *skip_flag != 0 (the range flag of the step, after the data-parallel
 * SUM: see "forward range guard" below); skip_flag may be NULL */
int wn_adam_step_guarded(wn_plan* p, float* params, const float* grads, float* m, float* v, int64_t step,
                         float lr, float beta1, float beta2, float eps, float clipnorm, float* scratch,
                         const float* skip_flag, void* stream);
/* Adam(use_ema=True): the guarded update plus the exponential moving average of the weights, in the same launch.
 * After the parameter update of step t: t == 1: ema = p (a copy); t > 1: ema = ema + (p - ema) * (1 - ema_momentum),
 * fp32 in that form; then, when ema_overwrite is 1, p = ema (the host decides: t % ema_overwrite_frequency == 0).
 * A skipped step (*skip_flag != 0) leaves ema untouched together with p, m, v.  ema: wn_plan_param_count floats.
 * ema_momentum must be finite and in [0, 1], ema_overwrite 0 or 1 (WN_E_INVALID otherwise, checked before the device is
 * touched). */
int wn_adam_step_ema(wn_plan* p, float* params, const float* grads, float* m, float* v, float* ema, int64_t step,
                     float lr, float beta1, float beta2, float eps, float clipnorm, float ema_momentum,
                     int32_t ema_overwrite, float* scratch, const float* skip_flag, void* stream);

/* ---- per-replica clipnorm ahead of the data-parallel all-reduce (Adam(clip_before_reduce=True)) ----
 * In place on the plan's flat gradient: every tensor t of wn_plan_tensor_info becomes
 * g_t * clipnorm / max(||g_t||, clipnorm), the norm accumulated in double.  A tensor whose norm is <= clipnorm (0
 * included) stays bit-identical.  Nothing past wn_plan_param_count(p) floats is read or written.  scratch: >= num_tensors
 * floats, receives the squared norms.  clipnorm must be finite and > 0 (WN_E_INVALID otherwise, checked before the
 * device is touched).  The following wn_adam_step then takes clipnorm 0. */
int wn_clip_gradients(wn_plan* p, float* grads, float clipnorm, float* scratch, void* stream);

/* ---- Adam with the other Keras keywords: global_clipnorm, clipvalue, weight_decay (AdamW), amsgrad ----
 * One guarded launch, a sibling of the kernels behind the three entry points above, which stay as they are: callers
 * that use none of the keywords keep calling those.  fp32 on the device, in exactly these forms (t = step, 1-based):
 *   clip    clip_mode is ONE of the WN_CLIP_* bits (or 0 = none) and `clip` its value c, finite and > 0:
 *             WN_CLIP_NORM         per tensor, g' = g * (c / fmaxf(||g_t||, c)), as wn_adam_step;
 *             WN_CLIP_GLOBAL_NORM  N2 = sum over the tensors of ||g_t||^2 (each accumulated in double, stored as a float,
 *                                  the floats added in double in tensor order), N = sqrtf((float)N2),
 *                                  g' = g * (c / fmaxf(N, c) + (N - N)): N <= c leaves g bit-identical, a non-finite N
 *                                  makes every g' NaN (it does not pass silently);
 *             WN_CLIP_VALUE        g' = g < -c ? -c : (g > c ? c : g); a NaN stays NaN.
 *   decay   weight_decay wd, finite and >= 0 (0 = off): p0 = p - (p * wd) * lr ahead of the update of the same step, on
 *           tensor i of wn_plan_tensor_info when decay_flags[i] != 0 -- decay_flags: num_tensors int32 in DEVICE memory, or
 *           NULL = every tensor.  It uses lr, not alpha, and never enters g', m or v.
 *   moments m = m + (g' - m) * (1 - beta1), v = v + (g' g' - v) * (1 - beta2)
 *   amsgrad amsgrad == 1: vhat = fmaxf(vhat, v) (wn_plan_param_count floats, state of the caller's, zeros at the start)
 *           and the denominator takes vhat; v keeps its own recursion.  amsgrad == 0: the denominator takes v and vhat is
 *           not looked at (it may be NULL).
 *   update  p = p0 - alpha * m / (sqrtf(v or vhat) + eps), alpha = lr sqrt(1 - beta2^t) / (1 - beta1^t) formed on the host
 *   ema     ema != NULL: as wn_adam_step_ema on that p (t == 1: ema = p; else ema + (p - ema) * (1 - ema_momentum); then
 *           p = ema when ema_overwrite is 1).  ema == NULL: ema_momentum and ema_overwrite must be 0.
 *   guard   *skip_flag != 0 (skip_flag may be NULL) leaves p, m, v, vhat and ema untouched, the decay included.
 * scratch: >= num_tensors floats (the squared norms of the two norm clips).
 * WN_E_INVALID, checked before the device is touched and named in wn_last_error_string: a NULL plan, params, grads, m, v,
 * options or scratch; step < 1; clip_mode with more than one bit or an unknown bit; a clip_mode with a clip that is not
 * finite and > 0; weight_decay negative or not finite; ema_momentum outside [0, 1] or not finite, ema_overwrite not 0 / 1,
 * either one non-zero without ema; amsgrad not 0 / 1, or 1 with a NULL vhat. */
#define WN_CLIP_NONE 0
#define WN_CLIP_NORM 1
#define WN_CLIP_GLOBAL_NORM 2
#define WN_CLIP_VALUE 4
typedef struct wn_adam_options {
  float lr, beta1, beta2, eps;
  int32_t clip_mode;            /* one WN_CLIP_* */
  float clip;                   /* its value; ignored when clip_mode is WN_CLIP_NONE */
  float weight_decay;
  float ema_momentum;
  int32_t ema_overwrite;
  int32_t amsgrad;              /* 0 / 1 */
  const int32_t* decay_flags;   /* device memory, or NULL */
} wn_adam_options;
int wn_adam_step_ext(wn_plan* p, float* params, const float* grads, float* m, float* v, float* vhat, float* ema,
                     int64_t step, const wn_adam_options* options, float* scratch, const float* skip_flag, void* stream);
/* The clips of wn_adam_step_ext alone and in place, for a replica's own gradient ahead of the data-parallel all-reduce
 * (Adam(clip_before_reduce=True)); the following step then takes WN_CLIP_NONE.  clip_mode is exactly one WN_CLIP_* bit,
 * clip finite and > 0 (WN_E_INVALID otherwise, before the device is touched).  WN_CLIP_NORM is wn_clip_gradients.  The
 * global form leaves a gradient inside the bound bit-identical, the value form writes only what it clamps; nothing past
 * wn_plan_param_count floats is read or written.  scratch: >= num_tensors floats. */
int wn_clip_gradients_ext(wn_plan* p, float* grads, int32_t clip_mode, float clip, float* scratch, void* stream);

/* ---- gradient accumulation: Adam(gradient_accumulation_steps=k), Keras's keyword ----
 * The optimizer is called once per micro-step.  Calls 1 .. k-1 of a cycle only store the gradient; call k forms the mean
 * g = (g_k + acc) / k, clips THAT with whichever clip is set (Keras 3 base_optimizer: divide, then _clip_gradients), runs
 * the Adam step above exactly as it is (decay, amsgrad and ema unchanged) and starts a new cycle.  The step number of
 * wn_adam_step* counts updates, not calls.  The accumulator is state of the caller's: one buffer of wn_plan_param_count
 * floats.  This entry point is the arithmetic of one micro-step, over two flat buffers of n floats (it takes no plan):
 *   WN_ACCUM_FIRST   acc = g                   the first micro-step of a cycle OVERWRITES: no memset, acc is not read
 *   WN_ACCUM_ADD     acc = acc + g             every later storing micro-step
 *   WN_ACCUM_FINISH  g = (g + acc) / (float)steps, acc untouched: the mean is left in grads, where the step reads it
 * fp32, one correctly rounded add or IEEE division per element, nothing fused.
 *   guard   *skip_flag != 0 (skip_flag may be NULL) leaves both buffers untouched in every mode: a pass whose range flag is
 *           up does not reach the accumulator (the caller repeats it with the exact-fp32 kernels).
 * float4 accesses when both pointers are 16-byte aligned, scalar ones otherwise; no access outside [0, n) of either buffer.
 * One pass of the largest grid covers WN_ACCUM_ONE_PASS floats; beyond it the grid strides.
 * WN_E_INVALID, checked before the device is touched and named in wn_last_error_string: a NULL acc or grads; n < 0; a mode
 * other than the three; steps < 2 in WN_ACCUM_FINISH (the other modes do not look at steps).  n == 0 is WN_OK, no launch. */
#define WN_ACCUM_FIRST 0
#define WN_ACCUM_ADD 1
#define WN_ACCUM_FINISH 2
#define WN_ACCUM_ONE_PASS 2097152
int wn_grad_accumulate(float* acc, float* grads, int64_t n, int32_t mode, int32_t steps, const float* skip_flag, void* stream);

/* ---- forward range guard of the split-precision mode ----
 * The default kernels evaluate fp32 products from fp16 hi|lo operand splits; an activation beyond the fp16 range
 * (65504) would turn into inf/NaN.  Every forward pass therefore keeps the running max-abs of the tensors that feed
 * such kernels (residual stream, skip sum, head activations) in one workspace float: wn_train_fwd_bwd / wn_eval_loss
 * write loss_out[2] = 1 when it reached wn_range_limit() (else 0; always 0 in exact-fp32 mode); wn_forward callers
 * read the float at workspace[wn_plan_range_slot()].  A tripped pass must be repeated with the exact-fp32 kernels
 * (wn_debug_set(1, 1)): the Python mirror does (WaveNet.train_step / call / test_step). */
int64_t wn_plan_range_slot(const wn_plan* p, int32_t B, int32_t T, int32_t training);
float wn_range_limit(void);

/* ---- WaveNet.generate / _generation, src/model.py:241-307 (intended semantics) ----
 * window (B,RF,1) initial samples; out (B,length,1).  deterministic != 0: argmax / mode
 * sampling; else Philox draws keyed by seed.  queued != 0 uses per-layer ring buffers
 * (result-identical to the sliding window; the reference's README.md:16 TODO).
 * A queued step of 128-channel blocks is ONE launch of one workgroup per (block, 32 utterances) that hand their rows
 * on inside the launch (wn_gen_relay128_kernel); it is taken while blocks x ceil(B / 32) fits the device's CU count,
 * every wait in it is bounded, and a wait that gave up is reported through the word behind wn_generate_guard_slot. */
int wn_generate(wn_plan* p, const float* params, const float* window, const float* cond, int32_t B,
                int32_t length, int32_t deterministic, int32_t queued, uint64_t seed, float* out,
                float* workspace, int64_t ws_floats, void* stream);
/* ---- sampling controls of the stochastic draw (generation and sample_waveform) ----
 * temperature T: finite and > 0 with a finite 1 / T (no denormal), else WN_E_INVALID.
 *   categorical head: the draw is from p_T(j) ~ p(j)^(1/T), i.e. softmax(logits / T), evaluated max-normalised as
 *   (p / p_max)^(1/T) -- the largest term is exactly 1, so no T underflows the total.
 *   mixture heads, row [w | mu | s]: a draw at temperature T is a draw at temperature 1 from [w / T | mu | s + ln T]
 *   (component pick sharpened, component scale times T, clip to [-1, 1] unchanged).
 * top_k: 0 = off; < 0 is WN_E_INVALID; categorical head only (non-zero with a mixture head is WN_E_INVALID).
 *   top_k >= classes is off (the unmodified path, bit for bit).  Otherwise the classes are ranked by (probability
 *   descending, class index ascending), the first top_k kept and renormalised.  With that tie rule top_k = 1 is the
 *   deterministic arg max ("first maximum wins").  The kept set does not depend on T.  Offered for up to 1024 classes
 *   (WN_E_UNSUPPORTED beyond).
 * seed: the Philox key of the draws.
 * top_p (nucleus; the last member, so {T, k, seed} initialisers leave it 0): 0 and 1 = off (the unmodified path, bit for
 *   bit); a value in (0, 1) = on; anything else, NaN included, is WN_E_INVALID.  Categorical head only (on with a mixture
 *   head is WN_E_INVALID), offered for up to 1024 classes (WN_E_UNSUPPORTED beyond).  Order: temperature -> top_k ->
 *   top_p.  With K the set top_k kept (all classes when it is off), q_j = (p_j / p_max)^(1/T) for j in K and 0 elsewhere,
 *   Q = sum q_j, and the classes ranked as for top_k (probability descending, class index ascending), the nucleus is
 *   the shortest prefix of that ranking whose sum of q is >= top_p * Q: a prefix whose sum equals top_p * Q suffices,
 *   it holds at least one class, and of the classes tied at the cut as many as needed are kept, lower class index
 *   first.  The draw is the same inverse-CDF draw from q restricted to the nucleus; the Philox words keep their use.
 *   All of this is fp32 arithmetic on q (sums, comparisons, one division).  The largest q is exactly 1 and Q <= 1024,
 *   so top_p <= 2^-11 keeps exactly the first-ranked class: the arg max of the deterministic draw.
 * A deterministic draw ignores temperature, top_k and top_p (arg max and mode do not depend on them); they are still
 * checked.
 * {1.0f, 0, seed} is the draw of the entry points without controls, bit for bit.  The fields are checked before
 * any other argument is looked at and before anything touches the device. */
typedef struct wn_sampling { float temperature; int32_t top_k; uint64_t seed; float top_p; } wn_sampling;
/* wn_generate with the sampling controls in place of the seed; wn_generate is its {1.0f, 0, seed} case */
int wn_generate_sampled(wn_plan* p, const float* params, const float* window, const float* cond, int32_t B,
                        int32_t length, int32_t deterministic, int32_t queued, const wn_sampling* sampling, float* out,
                        float* workspace, int64_t ws_floats, void* stream);
/* One piece of a sequence: the samples first .. first + length - 1, out (B, length).  wn_generate_sampled is its
 * (window, first = 0) case.  The pieces of a sequence, concatenated, are bit for bit the one call of the total length
 * with the same arguments: the Philox counter, the relay's epoch, the window parity and tau follow the index in the
 * sequence, only the output column is step - first.
 *   window != NULL begins a sequence and requires first == 0: window copy, priming pass (queued), then the steps.
 *   window == NULL goes on at first >= 1, on a workspace in which the samples 0 .. first - 1 were made by earlier calls
 *     with the same p, params, B, queued and seed.  It runs no priming pass and no weight preparation: the weight images
 *     and the condition biases of the priming pass are in the workspace (queued: cond may be NULL; the sliding window
 *     maps the condition in every step and needs it).  Between two calls the caller may copy the floats of
 *     wn_generate_state_range away and back; nothing else in the workspace changes from step to step.
 *   The range guard and the relay's give-up word (wn_generate_guard_slot) are cleared at the start of every call and
 *     speak of that call's steps.  A continuation in exact-fp32 mode (wn_debug_set(1, 1)) reads only what a
 *     split-precision priming pass left as well; the reverse does not hold (an exact-fp32 priming pass prepares no folded
 *     skip images and clears no relay area): a sequence begun in exact-fp32 mode stays there.
 *   On the 64-channel chain the head launch of a step carries the next step's pre work only when that step belongs to
 *     the same call; the first step of a continuation does its own (the launch step 1 takes): the same arithmetic.
 * WN_E_INVALID, before the device is touched: first < 0; window with first != 0; window == NULL with first == 0;
 * first + length > 2^31 - 1 (steps are 32-bit in the launch arguments). */
int wn_generate_chunk(wn_plan* p, const float* params, const float* window, const float* cond, int32_t B,
                      int64_t first, int32_t length, int32_t deterministic, int32_t queued, const wn_sampling* sampling,
                      float* out, float* workspace, int64_t ws_floats, void* stream);
/* ---- sampling controls per utterance ----
 * One generate call, B utterances, each with its own temperature, top_k, top_p, seed and Philox stream.
 * struct wn_sampling_row is the packed record of one utterance: what the check of struct wn_sampling leaves for the
 * kernels (T, 1 / T, the effective top_k: 0 for off or >= classes, the effective top_p: 0 for off or 1), the Philox key
 * `seed`, and `stream`, the row word of the Philox counter: utterance b draws sample t from counter (stream, t) under
 * key seed.  A table is B records, 8 floats each (wn_sampling_rows_floats), indexed by the utterance index of the call.
 *
 * wn_sampling_rows_pack: host only, touches no device.  Checks sampling[0 .. B) by the rules above for `head`
 *   (WN_HEAD_*) and `classes` (the categorical row length) and writes the B records into the caller's host memory `rows`;
 *   *flags gets WN_SAMPLING_ROWS_ON when some row has a control on (T != 1, top_k or top_p on) and WN_SAMPLING_ROWS_TOP_P
 *   when some row has top_p on.  stream: B values below 2^63, or NULL for stream[b] = b.  The first bad row ends it:
 *   WN_E_INVALID / WN_E_UNSUPPORTED exactly where the check of one struct wn_sampling gives them, and the error text names
 *   the row ("row 3: ...").  Null sampling / rows / flags, B < 1 and a stream value >= 2^63 are WN_E_INVALID.
 *
 * wn_generate_rows_chunk: wn_generate_chunk with `rows`, a DEVICE pointer (16-byte aligned) to the table the caller copied
 *   there, and the flags the pack function returned, in place of the struct wn_sampling.  The table lies outside the
 *   generation workspace (workspace size, state range and guard slot are those of wn_generate_chunk) and is only read;
 *   it must stay as it is until the call's work on the stream is done, and a continuation passes the same table.  The
 *   rules for window / first and the guarantee that the pieces of a sequence concatenated are the one call carry over
 *   word for word, and so do the errors, after: rows null, rows misaligned, flags that no pack call returns.
 *   The step's kernels are chosen once per call from the flags, i.e. from the union of the rows: with top_p on in some
 *   row the draw of every row is the sampler launch's.  Every stochastic draw reads the record of its utterance, whichever
 *   workgroup or tile the utterance falls into.
 * The defining property: utterance b of such a call, with stream[b] = b, is bit for bit utterance b of
 *   wn_generate_chunk at the same B, window, cond with {T[b], top_k[b], seed[b], top_p[b]}; a row whose controls are all off
 *   takes the draw without controls.  So a table of equal rows with streams 0 .. B - 1 gives wn_generate_chunk's result.
 *   Rows with equal window, cond, key and stream make equal samples.  (The samples of an utterance depend on nothing
 *   but its own row of window and cond, its record, and the weights -- not on its index, not on B: DESIGN.md section 31
 *   says what was checked.)
 * deterministic != 0 ignores the table's controls, keys and streams (arg max / mode), as it ignores struct wn_sampling.
 * Out of scope: per-row controls in wn_sample_waveform_sampled and in the training step's metric draw; a per-row
 *   deterministic flag (top_k = 1 on a categorical row is the arg max); changing B inside a sequence (a new request into
 *   a row of the running batch is wn_generate_admit, below). */
typedef struct wn_sampling_row { float T, inv_T; int32_t top_k; float top_p; uint64_t seed, stream; } wn_sampling_row;
#define WN_SAMPLING_ROWS_ON 1
#define WN_SAMPLING_ROWS_TOP_P 2
int64_t wn_sampling_rows_floats(int32_t B);
int wn_sampling_rows_pack(const wn_sampling* sampling, const uint64_t* stream, int32_t B, int32_t head, int32_t classes,
                          wn_sampling_row* rows, int32_t* flags);
int wn_generate_rows_chunk(wn_plan* p, const float* params, const float* window, const float* cond, int32_t B,
                           int64_t first, int32_t length, int32_t deterministic, int32_t queued,
                           const wn_sampling_row* rows, int32_t rows_flags, float* out, float* workspace,
                           int64_t ws_floats, void* stream);
/* ---- a new request into a row of a running batch ----
 * wn_generate_rows_begin: begins a sequence whose first sample has index `first` >= 0.  The arguments are those of
 *   wn_generate_rows_chunk; window is required.  Window copy, (queued) the priming pass, then the steps
 *   first + 1 .. first + length - 1.  The priming draw is sample `first`: drawn from counter (stream, first), written to output
 *   column 0; the window's index t stands at time t + first in every ring, and the relay's epoch, the window parity and
 *   tau follow the index in the sequence as they do in wn_generate_chunk.  first == 0 is
 *   wn_generate_rows_chunk(window, 0, ...) bit for bit.  The sequence is continued by wn_generate_rows_chunk(NULL, first', ...).
 *   (wn_generate_chunk / wn_generate_rows_chunk keep their rule: a window there requires first == 0.)  A deterministic
 *   sequence does not depend on `first`; a stochastic one does, through the counter.
 *   WN_E_INVALID, before the device is touched: rows null or misaligned, flags that no pack call returns, first < 0,
 *   window == NULL, first + length > 2^31 - 1.
 *
 * wn_generate_admit: `workspace` is a QUEUED session at B utterances in which the samples 0 .. position - 1 have been
 *   made (position >= 1).  The call replaces the k utterances slots[0 .. k) of it (host array, distinct values in [0, B))
 *   by k new requests: windows (k, RF), cond (k, cond_inputs) or NULL, rows_k (device, k records, 16-byte aligned) with
 *   their flags.  It does two things on `stream`:
 *     1. on `scratch` (wn_generate_admit_scratch_floats(p, k) floats: the queued generation workspace of k rows) the
 *        priming part of wn_generate_rows_begin at B' = k, first = position - 1, length = 1: sample position - 1 of request
 *        j goes to first_out[j] (device, k floats).  The pass prepares the weight images again, into the scratch.
 *     2. one launch (wn_gen_admit_rows_kernel) copies, for every j, everything the steps read per utterance from row j of
 *        the scratch's layout to row slots[j] of the session's: the KS raw-sample slots of xin, every slot of every block's
 *        ring (R floats) and inner rings (D floats), and on a conditioned net the condition bias of every block (2D
 *        floats, from the priming layout of k rows to that of B rows).  Both sequences share the time axis: slot s goes
 *        to slot s.  Nothing else per utterance outlives a step (the per-step rows and partial accumulators are written
 *        before they are read in every step and call; the relay's granules are tagged per step).
 *   After it, wn_generate_rows_chunk(NULL, position, ...) on the session treats the admitted rows like any other; the
 *   caller must have written the new records into its own device table at slots[j], and passes the new union of flags.
 *   The defining property: row slots[j] of the session, from index position - 1 on (first_out[j], then the row of the later
 *   chunks), is bit for bit row 0 of wn_generate_rows_begin at B = 1, first = position - 1 with request j's window,
 *   condition and record; every row not in `slots` is bit for bit what it is without the admission.
 *   Through wn_generate_rows_chunk / wn_generate_rows_begin / wn_generate_admit a draw at position t uses counter
 *   (stream, t): what a request draws there depends on the position it was admitted at.  Their *_origin forms below give
 *   every row a clock of its own, and with it draws that depend on the request alone.
 *   Range guard: the scratch has its own slot, wn_generate_guard_slot(p, k, 1), which speaks of the admission's priming
 *   pass; the session's slot is untouched.  A tripped admission is repeated in exact-fp32 mode (the move overwrites the
 *   same rows), and the session then stays in that mode.
 *   There is no `queued` argument: admission into a sliding-window session is not offered.  Not offered either: changing
 *   B, retiring a row (a free slot runs on until something is admitted into it), sharing the session's weight images.
 *   WN_E_INVALID, before the device is touched, the message naming the argument: a null pointer among p, params,
 *   windows, slots, rows_k, first_out, workspace, scratch; k < 1 or k > B; a slot outside [0, B) or a duplicate (with its
 *   index); position < 1 or > 2^31 - 2; rows_k misaligned; flags that no pack call returns; either workspace too small;
 *   cond == NULL on a conditioned net.
 *
 * wn_generate_admit_describe: test / diagnosis hook, host only.  One line listing the segments the move of (k, B) copies,
 *   separated by " | ", each as
 *     <name> block=<block or -1> slots=<slots> width=<floats per slot and utterance> src=<float offset in the scratch> dst=<... in the session>
 *   (a segment is [slot][rows][width]: k rows at src, B rows at dst), and last "floats_per_utterance=<sum of slots * width>".
 *   WN_E_INVALID as wn_layer_describe: null p or buffer, len < 1, k or B out of range, a buffer too short. */
int wn_generate_rows_begin(wn_plan* p, const float* params, const float* window, const float* cond, int32_t B,
                           int64_t first, int32_t length, int32_t deterministic, int32_t queued,
                           const wn_sampling_row* rows, int32_t rows_flags, float* out, float* workspace,
                           int64_t ws_floats, void* stream);
int64_t wn_generate_admit_scratch_floats(const wn_plan* p, int32_t k);
int wn_generate_admit(wn_plan* p, const float* params, const float* windows, const float* cond, int32_t k,
                      const int32_t* slots, int32_t B, int64_t position, int32_t deterministic,
                      const wn_sampling_row* rows_k, int32_t rows_flags_k, float* first_out, float* workspace,
                      int64_t ws_floats, float* scratch, int64_t scratch_floats, void* stream);
int wn_generate_admit_describe(const wn_plan* p, int32_t k, int32_t B, char* buf, int32_t len);
/* ---- a row's own clock ----
 * The three entry points above with one more argument, `origin`: a DEVICE array of one uint64_t per utterance of the call
 * (B values; origin_k: k values), 8-byte aligned, or NULL.  Utterance b draws sample t from counter
 * (stream[b], t - origin[b]) under key seed[b]; the subtraction is unsigned 64-bit.  Nothing else changes: output columns,
 * rings, tau, the relay's epoch and the window parity follow t, and the network is time invariant.  So a request whose
 * origin is the index of its first sample draws from counters (stream, 0), (stream, 1), ... wherever in the sequence, in
 * whichever row and beside whichever other rows it runs.
 * The defining property: a request admitted at `position` with origin_k[j] = position - 1, whose row then carries that
 *   origin in the session's array, is from first_out[j] on bit for bit row 0 of wn_generate_rows_chunk(window, first = 0, ...)
 *   at B = 1 with the request's window, condition and record -- the request alone, from position 0.  Likewise
 *   wn_generate_rows_begin_origin at `first` with every origin = first is wn_generate_rows_chunk(window, 0, ...).
 * The array is treated like `rows`: it lies outside the workspace and is only read; it must stay as it is until the
 *   call's work on the stream is done, and a continuation passes the same array.  After wn_generate_admit_origin the
 *   caller writes origin_k[j] into its own session array at slots[j], as it does for the records.
 * origin == NULL is the entry point without the argument, bit for bit (the same code runs); an array of zeros gives those
 *   bits too.  deterministic != 0 ignores the array.  queued == 0 (the sliding window) takes it like the table.
 * The library cannot see the values: origin[b] <= the index of every sample utterance b draws in the call is the
 *   caller's duty.  Beyond it the counter word wraps modulo 2^64 (a row then draws from (stream, 2^64 - d)); nothing faults.
 * WN_E_INVALID, before the device is touched and before any other argument is looked at: origin / origin_k not aligned to
 *   8 bytes, the message naming the argument.  Every other error is the one of the entry point without the argument.
 * Out of scope: origins in wn_sample_waveform_sampled and in the training step's draw; a per-row deterministic flag. */
int wn_generate_rows_chunk_origin(wn_plan* p, const float* params, const float* window, const float* cond, int32_t B,
                                  int64_t first, int32_t length, int32_t deterministic, int32_t queued,
                                  const wn_sampling_row* rows, int32_t rows_flags, const uint64_t* origin, float* out,
                                  float* workspace, int64_t ws_floats, void* stream);
int wn_generate_rows_begin_origin(wn_plan* p, const float* params, const float* window, const float* cond, int32_t B,
                                  int64_t first, int32_t length, int32_t deterministic, int32_t queued,
                                  const wn_sampling_row* rows, int32_t rows_flags, const uint64_t* origin, float* out,
                                  float* workspace, int64_t ws_floats, void* stream);
int wn_generate_admit_origin(wn_plan* p, const float* params, const float* windows, const float* cond, int32_t k,
                             const int32_t* slots, int32_t B, int64_t position, int32_t deterministic,
                             const wn_sampling_row* rows_k, int32_t rows_flags_k, const uint64_t* origin_k, float* first_out,
                             float* workspace, int64_t ws_floats, float* scratch, int64_t scratch_floats, void* stream);
/* ---- a new condition for a running queued sequence ----
 * cond (B, cond_inputs).  Runs the conditioning phase again (mapping stack, every block's conv_cond) into the bias table of
 * the workspace, where the priming pass of the sequence wrote it: the table is state the steps read, not a per-step input.
 * The steps of the following chunks use it; nothing else of the sequence changes, and the step kernels are what they were.
 * A locally conditioned model's frame schedule is this call at every frame boundary, between two chunks.
 * Queued sequences only.  The workspace must be the one the calling state primed last, at the same B (an admission's
 * scratch call at another B moves that mark: call this before admitting, or begin again).
 * WN_E_INVALID, before the device is touched, the message naming the cause: a null plan / params / cond / workspace; B < 1;
 * queued == 0; a plan without conditioning; condition frames armed; a workspace too small; a workspace not primed. */
int wn_generate_set_condition(wn_plan* p, const float* params, const float* cond, int32_t B, int32_t queued,
                              float* workspace, int64_t ws_floats, void* stream);
/* ---- frame schedules of queued generation: a schedule per row, advanced on the device ----
 * A request's bias rows are computed once for all of its frames, into a table the request keeps; during the step loop a
 * small copy kernel moves every scheduled row's current frame into the compact table cb[N][B][2D] of the workspace, which
 * is all the step kernels ever read (they are the kernels of the calls without a schedule).
 *
 * wn_generate_frames_floats(plan, rows): the floats of a frame table for `rows` condition rows (requests x frames): the bias
 *   rows [N][rows][2D] and, behind them, the scratch of the conditioning phase at that row count.  0 for a null plan, a plan
 *   without conditioning or rows < 1.
 * wn_generate_frames_build: the conditioning phase (mapping stack, every block's conv_cond, biases, scatter) over the k * F
 *   rows of cond (k, F, cond_inputs), into `table` (device, 16-byte aligned, >= wn_generate_frames_floats(plan, k * F)
 *   floats): row (j, f) of block n is the 2D floats at table + (n * k * F + j * F + f) * 2D, so request j's record is
 *   rows = table + j * F * 2D with block_stride = k * F * 2D.  It runs in the calling thread's math mode (wn_debug_set(1, .)).
 *   The weight images it reads are those a priming pass left in `workspace`, a queued generation workspace of batch size B
 *   in which a sequence has begun with these parameters (any queued call that begins a sequence primes): read only --
 *   nothing in any workspace is written.  That the workspace has been primed is the caller's word: unlike
 *   wn_generate_set_condition this call does not ask for the calling state's last primed workspace, so that a session
 *   can build a request's table while other sequences run on the same state; an unprimed workspace gives rows without
 *   meaning and no fault (ws_floats is checked against the layout of B).  Every row is bit for bit the row
 *   wn_generate_set_condition writes into cb for that condition alone: which kernel a product takes does not depend on the
 *   row count.
 *   WN_E_INVALID, before the device is touched, the message naming the cause and its numbers: a null plan / params / cond /
 *   table / workspace; k < 1 or F < 1; k * F * blocks * 2D beyond 2^31 - 1; a plan without conditioning; condition frames
 *   armed (wn_plan_set_cond_frames); table not aligned to 16 bytes; table_floats too small; B < 1; a workspace too small.
 * struct wn_frame_row: the schedule of one row of the batch.  rows == NULL: the row is off the schedule and its cb rows are
 *   left as they are.  Otherwise block n's row of frame f is the 2D floats at rows + n * block_stride + f * 2D; origin is the
 *   sequence index of the row's sample 0, and the step that emits sample t uses frame (t - origin) / hop (frame 0 where
 *   t < origin).  The table belongs to the caller and must outlive every call made while the record is armed; the session
 *   has no table of its own, no cap on frames and copies nothing at admission.
 * wn_plan_arm_gen_frames(plan, records (host, B of them), B) arms the calling thread's execution state, in the manner of
 *   wn_plan_arm_row_weights; records == NULL or B == 0 disarms.  Host only: the library copies the records, and uploads
 *   them inside the first queued call that needs them (a blocking copy behind a stream synchronise, made only when the
 *   records differ from those it uploaded last).  The device copy is one per execution state, like the cached block
 *   table of the chains, and the upload waits for the CALLING stream alone: sequences that share a state must run on one
 *   stream (or take a wn_exec each), and two sessions that alternate on one state pay the synchronise and the upload at
 *   every change of hands.  While armed, the queued forms of wn_generate_chunk,
 *   wn_generate_rows_chunk[_origin] and wn_generate_rows_begin[_origin]
 *     launch the copy kernel in front of whichever launch reads cb for step t -- the head launch of step t - 1 where that
 *     launch carries the next step's pre work, the chain, relay or first block launch of step t otherwise -- at the call's
 *     first step behind the priming pass, and at every later step t of the call where some scheduled row has
 *     (t - origin) % hop == 0 (computed on the host from the records).  The priming pass of a call that begins a sequence
 *     takes `cond` as ever (a frame schedule hands it frame 0);
 *     return WN_E_INVALID, before anything is launched, when a scheduled row would need a frame >= frames at one of the
 *     call's steps: the message names the row, its frames and its hop;
 *     return WN_E_INVALID when armed with another B than the call's, and for a sliding-window call (queued == 0).
 *   wn_generate_admit[_origin] ignores the armed schedule (its scratch pass at k rows takes cond).
 *   With nothing armed every entry point queues exactly the launches it queues without this entry point.
 *   WN_E_INVALID: a null plan; B < 0; records != NULL on a plan without conditioning or while condition frames are armed; a
 *   scheduled record with frames < 1, hop < 1, or block_stride < frames * 2D; the message names the row. */
typedef struct wn_frame_row {
  const float* rows;
  int64_t block_stride;
  int64_t origin;
  int32_t frames;
  int32_t hop;
} wn_frame_row;
int64_t wn_generate_frames_floats(const wn_plan* p, int64_t rows);
int wn_generate_frames_build(wn_plan* p, const float* params, const float* cond, int32_t k, int32_t F, float* table,
                             int64_t table_floats, const float* workspace, int64_t ws_floats, int32_t B, void* stream);
int wn_plan_arm_gen_frames(wn_plan* p, const wn_frame_row* records, int32_t B);
int64_t wn_generate_workspace_floats(const wn_plan* p, int32_t B, int32_t queued);
/* The one contiguous part of the generation workspace that steps write and a continuation reads, as a float offset and a
 * float count.  queued: from the raw-sample slots to the end of the layout (rings, inner rings, per-step rows, partial
 * accumulators, the relay's granule area, the head rows); sliding window: the two window buffers. */
int wn_generate_state_range(const wn_plan* p, int32_t B, int32_t queued, int64_t* offset, int64_t* floats);
/* float offset, inside the caller's generation workspace, of the call's range-guard slot.  After wn_generate (stream
 * synchronised) the float is >= wn_range_limit() if and only if some split-precision kernel of the call was fed an
 * |activation| at or beyond that limit: the priming pass (residual stream, skip sum, head activations), and in EVERY
 * queued step the residual stream and folded skip sum of the chain kernels, the per-block kernels, the skip contraction
 * and the hidden head activations.  (Below the limit it holds the priming pass's largest magnitude; the per-step kernels
 * only ever raise it past the limit.)  A tripped call is to be repeated with the exact-fp32 kernels (wn_debug_set(1, 1)).
 * The 32-bit word right behind it (slot + 1) is the hand-off watchdog of the multi-workgroup generation step
 * (wn_gen_relay128_kernel): zero after a good call; non-zero bits name a workgroup that gave up waiting for its
 * predecessor's rows -- the samples of such a call are invalid and the caller must treat it as failed. */
int64_t wn_generate_guard_slot(const wn_plan* p, int32_t B, int32_t queued);

/* ---- WaveNetLayer.call, src/layers.py:178-224, standalone block ----
 * weights in Keras layout: dil_kernels = layers_in_block kernels concatenated
 * [(k,Cin_i,Cout_i)...], dil_biases likewise; conv1 (D,R); conv_skip (D,S) or NULL;
 * conv_cond (Cc,2D) or NULL with cond (B,T,Cc).  dilations[depth].
 * saved: caller buffer of wn_layer_saved_floats() floats kept for wn_layer_bwd (or NULL). */
typedef struct wn_layer_desc {
  int32_t kernel_size, channels, dilation_channels, skip_channels /*0 = None*/;
  int32_t depth;                 /* len(dilation_rate) */
  int32_t dilations[16];
  int32_t activation, residual, cond_channels /*0 = no condition*/;
  int32_t in_channels;           /* channels of the input tensor */
} wn_layer_desc;
int64_t wn_layer_saved_floats(const wn_layer_desc* d, int32_t B, int32_t T);
int64_t wn_layer_workspace_floats(const wn_layer_desc* d, int32_t B, int32_t T);
int wn_layer_fwd(const wn_layer_desc* d, const float* params, const float* x, const float* cond,
                 int32_t B, int32_t T, float* x_out, float* skip_out, float* saved,
                 float* workspace, void* stream);
/* Backward of the wn_layer_fwd call that filled `saved` (same d, params, x, cond, B, T):
 * gradients of <g_x_out, x_out> + <g_skip, skip_out>.  g_x_out (B,T,R), g_skip (B,T,S), or (B,T,R) when skip_channels is 0
 * (the skip output is then the 1x1 conv's output before the residual is added).
 *   g_x_out == NULL  x_out does not enter the objective: no residual term in g_x; with skip_channels > 0 conv1 gets no
 *                    gradient and dW_r, db_r are written as zeros (with skip_channels 0 they come from g_skip).
 *   g_skip == NULL   skip_out does not enter the objective: with skip_channels > 0 dW_s, db_s are written as zeros.
 *   both NULL        the gradient at u is zero: every element of g_params, g_x and g_cond is written as zero.
 *   both given, skip_channels 0: the 1x1 conv's output gradient is g_x_out + g_skip (formed in the workspace).
 *   g_x == NULL      the input gradient is not formed: the backward-data product of the stack's first conv is not run (those
 *                    of the convs above it still are: the weight gradients below them need their results).  Nothing else
 *                    changes.
 *   g_cond == NULL   the condition's gradient is not formed; dW_c, db_c and everything else are unchanged.
 * g_params (wn_layer_param_count floats, the layout of params): EVERY element is written by every call, overwritten and
 * not accumulated; the caller need not clear it.  g_x (B,T,in_channels) and g_cond (B,T,Cc) likewise where given.
 * workspace: wn_layer_workspace_floats(d, B, T) floats; nothing in it is carried from the forward call to this one. */
int wn_layer_bwd(const wn_layer_desc* d, const float* params, const float* x, const float* cond,
                 const float* saved, const float* g_x_out, const float* g_skip, int32_t B, int32_t T,
                 float* g_x, float* g_cond, float* g_params, float* workspace, void* stream);
int64_t wn_layer_param_count(const wn_layer_desc* d);
/* test / diagnosis hook, host only: one line naming every weight-gradient product wn_layer_bwd launches over (B, T) when
 * both output gradients are given, in launch order -- conv1, conv_skip, conv_cond, then the stack from its last conv to its
 * first, one product per tap (`dil<i>.tap<j>`) -- separated by " | ", each as
 *   <name> K=<rows of dW> N=<columns of dW> splits=<time ranges per utterance> nsplit=<B * splits> reduce=one-stage|two-stage
 * computed by the functions the launches themselves call (the split heuristic and the reduce's stage decision).
 * WN_E_INVALID: a bad descriptor, B < 1 or T < 1, a null buffer or len < 1, or a buffer too short for the line (the message
 * names the bytes needed; buf then holds the truncated, terminated text). */
int wn_layer_describe(const wn_layer_desc* d, int32_t B, int32_t T, char* buf, int32_t len);

/* ---- elementwise pieces of the boundary ---- */
/* prepare_target = Discretization (tf Bucketize), src/model.py:151-153: bit-exact indices */
int wn_quantize(const float* x, int32_t* idx, int64_t n, int32_t bits, void* stream);
/* index -> left bin edge, src/model.py:411,418 */
int wn_dequantize(const int32_t* idx, float* x, int64_t n, int32_t bits, void* stream);
/* mu-law companding src/utils.py:34-35 and its inverse src/callbacks.py:126-131 */
int wn_mulaw(const float* x, float* y, int64_t n, void* stream);
int wn_inv_mulaw(const float* y, float* x, int64_t n, void* stream);
/* WaveNet.loss_fn(target, pred), src/model.py:505-551: per-(b,t) loss, rows = B*T.
 * categorical: target int32 indices, pred probabilities; mixtures: target fp32 values. */
int wn_loss_fn(int32_t head, const void* target, const float* pred, int64_t rows, int32_t C,
               int32_t num_mixtures, int32_t bits, float* loss_rows, void* stream);
/* Arms the NEXT wn_train_fwd_bwd on this plan to also write sample = sample_waveform(pred) of that step
 * (rows = B*T floats; src/model.py:338, consumed by the compiled metrics :340-346) drawn from the logits inside
 * the step -- the same draw wn_sample_waveform(seed, offset) makes from that step's pred, without the (rows, C)
 * probability tensor.  sample_out = NULL disarms.  WN_E_UNSUPPORTED (nothing armed): categorical head with a
 * deterministic draw or more than 1024 classes; use pred_out + wn_sample_waveform there. */
int wn_plan_arm_step_sample(wn_plan* plan, float* sample_out, int32_t deterministic, uint64_t seed, uint64_t offset);
/* wn_train_fwd_bwd in two calls: phases = 1 runs forward + loss (+ the armed step sample) and returns, phases = 2 runs the
 * backward pass and the weight gradients of THAT forward pass (same arguments, same workspace), 3 = both (default).  A
 * host driver uses the gap to queue its read-back of loss / metrics 4 ms before the step ends. */
int wn_plan_set_train_phases(wn_plan* plan, int32_t phases);
/* tf.keras.metrics.MeanSquaredError(y_true, sample) of one step (train.py:227, src/model.py:338-346) as a device scalar:
 * out[0] = scale * sum_i (a[i] - b[i])^2 in double accumulation; scale = 1 / (n * replicas) makes the SUM over the
 * replicas the metric's mean.  scratch: >= 2048 floats of the caller's. */
int wn_sum_squared_error(const float* a, const float* b, int64_t n, float scale, float* out, float* scratch,
                         void* stream);
/* ---- sample_weight of a training / evaluation step (Keras's train_step contract) ----
 * w: rows = B * T device floats over the target rows, w[b * T + t] belongs to the target x_full[b][t + 1].  Arms the
 * calling thread's execution state; it stays armed until w == NULL disarms it (the caller owns the buffer: disarm before
 * freeing it).  While armed, wn_train_fwd_bwd, wn_eval_loss and wn_score weigh their rows; they return WN_E_INVALID when
 * rows != B * T of the call, checked before the device is touched, the message naming both numbers.  wn_vjp, wn_forward*,
 * wn_loss_fn, generation and the optimizer ignore it.  With wn_plan_set_train_phases the weights are read in phase 1 only.
 *   loss = sum_{b,t} w[b,t] l[b,t] / global_batch (+ the L2 term, unchanged).  The normaliser stays global_batch, as in
 *     tf.nn.compute_average_loss(per_example_loss, sample_weight): no division by sum w.  A caller who wants the mean over
 *     the valid samples scales w.  Data parallelism needs nothing new: every replica weighs its own rows.
 *   gradient: d loss / d logits (or d pred) of a row is that of the unweighted step with gscale = 1 / global_batch replaced
 *     by gscale * w[row], the product taken once per row in fp32; the stored per-row loss (wn_debug_ws_region what 12) is
 *     w[row] * l[row].  w == 1 everywhere therefore gives the bits of the call without weights, which also launches the
 *     kernels it launched before this entry point existed.
 *   w[row] == 0 is a select, not a product: the row's loss is +0 and every entry of its gradient is 0, even where the row's
 *     own loss or gradient is inf or NaN (a mixture likelihood that underflows), and the row contributes nothing to the
 *     published max-abs of the gradient.
 *   Negative and non-finite weights are not checked: a plain product is taken, non-finite in gives non-finite out.
 *   The armed step sample is drawn for every row as without weights; the weights do not enter it.
 * WN_E_INVALID: a null plan; w != NULL with rows < 1. */
int wn_plan_arm_row_weights(wn_plan* plan, const float* w, int64_t rows);
/* ---- local conditioning: a condition frame per `hop` inputs (WaveNet(conditioning='local')) ----
 * The reference maps the condition (B, F, Cin) with 1x1 convolutions and upsamples the result to the input rate by
 * repetition (src/model.py:216-220), so inside a frame conv_cond(condition) is constant: local conditioning is the bias table
 * of global conditioning with one row per (utterance, frame) instead of one per utterance, and the 1x1 mapping stack is the
 * Dense stack over the B * F rows (the flat element order of a (1, cin, w) and a (cin, w) kernel is the same; wn_config and
 * the tensor table do not change).
 * wn_plan_set_cond_frames arms the calling thread's execution state, in the manner of wn_plan_set_dropout: frames = 0 or 1
 * means the calls as they are without it, bit for bit.  With frames = F > 1, in wn_forward, wn_forward_training,
 * wn_train_fwd_bwd, wn_eval_loss, wn_score and wn_vjp:
 *   cond is (B, F, cond_inputs) and g_cond has that shape; with T network inputs hop = T / F, and the mapped condition of
 *   frame f acts on the inputs t in [f * hop, (f + 1) * hop);
 *   wn_plan_workspace_floats answers for the armed F (the conditioning's regions hold B * F rows), and what an execution
 *   state caches per (B, T) is keyed by F as well; wn_debug_ws_region likewise answers for the F armed when it is asked
 *   (the regions carved behind the conditioning's move with F: ask with the frames of the pass armed);
 *   T % F != 0 is WN_E_INVALID (the reference's add would fail), and so is hop % 32 != 0: every kernel that adds the bias
 *   walks 32-row time tiles that start at multiples of 32 inside an utterance and reads ONE bias row per tile, so a frame
 *   must hold whole tiles.  This is a limit of this implementation.  Both messages name T, F (and hop), and both are
 *   raised before the device is touched.
 *   The gradient of the bias table is the per-frame sum of every block's dL/du, one launch for all blocks with a fixed
 *   summation order (wn_cond_frames.hip); from there the conditioning backward is that of global conditioning over B * F rows.
 * The generation entry points take one condition row per utterance and return WN_E_INVALID while F > 1 is armed.
 * WN_E_INVALID: a null plan, frames < 0, frames > 1 on a plan without conditioning. */
int wn_plan_set_cond_frames(wn_plan* plan, int32_t frames);
/* Keras's weighted MeanSquaredError of one step as a device scalar: out[0] = scale * sum_i w[i] (a[i] - b[i])^2 / sum_i w[i],
 * and 0 when sum_i w[i] == 0; numerator and denominator in one pass, double accumulation in two stages as
 * wn_sum_squared_error.  scale = 1 / replicas makes the SUM over the replicas the average of their ratios: the weighted
 * mean of the global batch when the replicas hold equal sum w, an approximation otherwise.  scratch: >= 2048 floats of the
 * caller's.  WN_E_INVALID: a null pointer or n < 1. */
int wn_weighted_squared_error(const float* a, const float* b, const float* w, int64_t n, float scale, float* out,
                              float* scratch, void* stream);
/* WaveNet.sample_waveform(pred, deterministic), src/model.py:393-503: (rows,C) -> (rows) */
int wn_sample_waveform(int32_t head, const float* pred, int64_t rows, int32_t C,
                       int32_t num_mixtures, int32_t bits, int32_t deterministic, uint64_t seed,
                       uint64_t offset, float* out, void* stream);
/* ... with the sampling controls in place of the seed (categorical: pred holds probabilities, C classes) */
int wn_sample_waveform_sampled(int32_t head, const float* pred, int64_t rows, int32_t C,
                               int32_t num_mixtures, int32_t bits, int32_t deterministic, const wn_sampling* sampling,
                               uint64_t offset, float* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* WN_HIP_H */
