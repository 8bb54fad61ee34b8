// The optimizer (gfx950): per-tensor sums of squares, the clips, Keras Adam with all of its keywords in one kernel, and the
// C-ABI entry points over them (train.py:225-226, src/model.py:336).  Shares nothing with the passes but WnTensorDesc and
// the plan's tensor table.
#include <cmath>

#include "wn_plan_internal.h"

// ------------------------------------------------------------------------------------------
// optimizer: per-tensor clipnorm + Keras Adam  (train.py:225-226, src/model.py:336)
__global__ void wn_sumsq_kernel(const float* g, const WnTensorDesc* table, float* norms2) {
  __shared__ double sm[256];
  const WnTensorDesc d = table[blockIdx.x];
  const float* p = g + d.off;
  // four independent chains: a single one ran at one memory round trip per element (63 us for 1.25 M values)
  double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
  int64_t i = threadIdx.x;
  for (; i + 3 * 256 < d.len; i += 4 * 256) {
    const float v0 = p[i], v1 = p[i + 256], v2 = p[i + 512], v3 = p[i + 768];
    a0 += (double)v0 * (double)v0; a1 += (double)v1 * (double)v1;
    a2 += (double)v2 * (double)v2; a3 += (double)v3 * (double)v3;
  }
  for (; i < d.len; i += 256) a0 += (double)p[i] * (double)p[i];
  const double acc = (a0 + a1) + (a2 + a3);
  sm[threadIdx.x] = acc;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (threadIdx.x < o) sm[threadIdx.x] += sm[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) norms2[blockIdx.x] = (float)sm[0];
}
int wn_launch_sumsq(const float* g, const WnTensorDesc* d_table, int n, float* norms2, hipStream_t s) {
  if (n <= 0) return WN_OK;
  hipLaunchKernelGGL(wn_sumsq_kernel, dim3(n), dim3(256), 0, s, g, d_table, norms2);
  WN_HIP_CHECK(hipGetLastError());
  return WN_OK;
}

// Per-replica clipnorm ahead of the data-parallel all-reduce (Adam(clip_before_reduce=True)): in place, tensor t
// becomes g_t * clipnorm / max(||g_t||, clipnorm).  One workgroup of 1024 threads owns one tensor: it reduces the
// squared norm in double (as wn_sumsq_kernel does), then rescales the same <= 256 KiB, which it has just pulled into
// L2 -- no sumsq launch, no norms round trip, no scale launch.  A tensor inside the bound (norm 0 included) has scale
// exactly 1.0f and is not written at all.  The body moves float4; the scalar head and tail keep every access inside
// [off, off + len), whatever the alignment of the tensor: the step's scalars sit right behind the last gradient.
#define WN_CLIP_THREADS 1024
__global__ void __launch_bounds__(WN_CLIP_THREADS)
wn_clip_kernel(float* g, const WnTensorDesc* table, float clipnorm, float* norms2) {
  __shared__ double sm[WN_CLIP_THREADS / 64];
  __shared__ float sm_scale;
  const WnTensorDesc d = table[blockIdx.x];
  float* p = g + d.off;
  const int tid = threadIdx.x;
  int64_t head = (int64_t)((16u - (unsigned)((uintptr_t)p & 15u)) & 15u) >> 2;    // floats up to 16-byte alignment
  if (head > d.len) head = d.len;
  const int64_t nvec = (d.len - head) >> 2;
  const int64_t tail = head + 4 * nvec;
  float4* pv = reinterpret_cast<float4*>(p + head);
  double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
  int64_t i = tid;
  for (; i + WN_CLIP_THREADS < nvec; i += 2 * WN_CLIP_THREADS) {       // two loads in flight per thread
    const float4 x = pv[i], y = pv[i + WN_CLIP_THREADS];
    a0 += (double)x.x * (double)x.x; a1 += (double)x.y * (double)x.y;
    a2 += (double)x.z * (double)x.z; a3 += (double)x.w * (double)x.w;
    a0 += (double)y.x * (double)y.x; a1 += (double)y.y * (double)y.y;
    a2 += (double)y.z * (double)y.z; a3 += (double)y.w * (double)y.w;
  }
  for (; i < nvec; i += WN_CLIP_THREADS) {
    const float4 x = pv[i];
    a0 += (double)x.x * (double)x.x; a1 += (double)x.y * (double)x.y;
    a2 += (double)x.z * (double)x.z; a3 += (double)x.w * (double)x.w;
  }
  if (tid < head) a0 += (double)p[tid] * (double)p[tid];
  if (tail + tid < d.len) a1 += (double)p[tail + tid] * (double)p[tail + tid];
  double acc = (a0 + a1) + (a2 + a3);
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_down(acc, o, 64);
  if ((tid & 63) == 0) sm[tid >> 6] = acc;
  __syncthreads();
  if (tid == 0) {
    double n2 = 0.0;
    for (int w = 0; w < WN_CLIP_THREADS / 64; ++w) n2 += sm[w];
    const float n2f = (float)n2;
    norms2[blockIdx.x] = n2f;
    sm_scale = clipnorm / fmaxf(sqrtf(n2f), clipnorm);     // tf.clip_by_norm, the expression of wn_adam_kernel
  }
  __syncthreads();
  const float scale = sm_scale;
  if (scale == 1.0f) return;       // uniform: inside the bound, the tensor stays bit-identical
  for (i = tid; i < nvec; i += WN_CLIP_THREADS) {
    float4 x = pv[i];
    x.x *= scale; x.y *= scale; x.z *= scale; x.w *= scale;
    pv[i] = x;
  }
  if (tid < head) p[tid] *= scale;
  if (tail + tid < d.len) p[tail + tid] *= scale;
}
int wn_launch_clip(float* g, const WnTensorDesc* d_table, int n, float clipnorm, float* norms2, hipStream_t s) {
  if (n <= 0) return WN_OK;
  hipLaunchKernelGGL(wn_clip_kernel, dim3(n), dim3(WN_CLIP_THREADS), 0, s, g, d_table, clipnorm, norms2);
  WN_HIP_CHECK(hipGetLastError());
  return WN_OK;
}

// The factor of the global-norm clip from the per-tensor sums of wn_sumsq_kernel: every workgroup adds the n floats itself,
// in double and in tensor order (uniform addresses: the same bits everywhere, no launch of its own).  The last term is NaN
// for a non-finite norm and poisons the step as Keras does.
__device__ __forceinline__ float wn_global_clip_scale(const float* norms2, int n, float c) {
  double n2 = 0.0;
  for (int t = 0; t < n; ++t) n2 += (double)norms2[t];
  const float N = sqrtf((float)n2);
  return c / fmaxf(N, c) + (N - N);
}

// Keras Adam, one step, every keyword in one launch: grid (32, n), row t walks tensor t of the table with a grid-stride
// loop; scalar accesses, since tensors start at arbitrary float offsets.  Everything is uniform per launch.  EMA and
// AMSGRAD are template arguments since each adds a stream (a: 2 floats per parameter, vhat: 2 more, 7 without); KEYWORDS
// = a global-norm or value clip or a decay is on: without it those branches are not in the code, which is the step of
// Adam(clipnorm) that everybody runs (measured).
// Per element, in fp32 and in exactly these forms:
//   g'   clip_mode WN_CLIP_NONE:  g
//        WN_CLIP_NORM:            g * (clip / fmaxf(sqrtf(norms2[t]), clip))                         (tf.clip_by_norm)
//        WN_CLIP_GLOBAL_NORM:     g * wn_global_clip_scale(norms2, n, clip)
//        WN_CLIP_VALUE:           g < -clip ? -clip : (g > clip ? clip : g); both comparisons are false for a NaN, which
//                                 therefore stays
//   m    m + (g' - m) * (1 - beta1)
//   v    v + (g' g' - v) * (1 - beta2)
//   vhat AMSGRAD: fmaxf(vhat, v), which feeds the denominator; v keeps its own recursion
//   p0   wd > 0 and (no decay_flags or decay_flags[t] != 0): p - (p * wd) * lr, ahead of the update; it never enters g', m
//        or v.  Otherwise p.
//   p    p0 - alpha * m / (sqrtf(vhat or v) + eps), alpha the bias-corrected rate of the host
//   a    EMA: a + (p - a) * (1 - momentum), the form m and v use; ``first`` (step 1) copies p instead: a multiply by zero
//        would keep a NaN / inf of the initial average.  The average observes, it never feeds back, unless ``overwrite``
//        asks for p = a.
// A raised skip_flag (the range guard tripped: the step is redone in exact fp32) leaves everything alone, decay and average
// included.
template <bool EMA, bool AMSGRAD, bool KEYWORDS>
__global__ void wn_adam_kernel(float* p, const float* g, float* m, float* v, float* vhat, float* a,
                               const WnTensorDesc* table, int n, const float* norms2, int clip_mode, float clip,
                               float lr, float wd, const int32_t* decay_flags, float alpha, float beta1, float beta2,
                               float eps, float momentum, int first, int overwrite, const float* skip_flag) {
  if (skip_flag && *skip_flag != 0.f) return;     // range guard tripped: nothing moves, the decay included (uniform)
  const WnTensorDesc d = table[blockIdx.y];
  float scale = 1.0f;
  if (clip_mode == WN_CLIP_NORM) {
    const float nrm = sqrtf(norms2[blockIdx.y]);
    scale = clip / fmaxf(nrm, clip);     // tf.clip_by_norm
  } else if (KEYWORDS && clip_mode == WN_CLIP_GLOBAL_NORM) {
    scale = wn_global_clip_scale(norms2, n, clip);
  }
  const bool by_value = KEYWORDS && clip_mode == WN_CLIP_VALUE;
  const bool decays = KEYWORDS && wd > 0.f && (!decay_flags || decay_flags[blockIdx.y] != 0);
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < d.len;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t k = d.off + i;
    const float gr = g[k];
    const float gi = by_value ? (gr < -clip ? -clip : (gr > clip ? clip : gr)) : gr * scale;
    const float mi = m[k] + (gi - m[k]) * (1.0f - beta1);
    const float vi = v[k] + (gi * gi - v[k]) * (1.0f - beta2);
    m[k] = mi;
    v[k] = vi;
    float den = vi;
    if (AMSGRAD) {
      den = fmaxf(vhat[k], vi);
      vhat[k] = den;
    }
    const float p0 = decays ? p[k] - (p[k] * wd) * lr : p[k];
    const float pi = p0 - alpha * mi / (sqrtf(den) + eps);
    if (EMA) {
      const float ai = first ? pi : a[k] + (pi - a[k]) * (1.0f - momentum);
      a[k] = ai;
      p[k] = overwrite ? ai : pi;
    } else {
      p[k] = pi;
    }
  }
}
int wn_launch_adam(const WnAdamArgs& x, hipStream_t s) {
  if (x.n <= 0) return WN_OK;
  // [average][amsgrad][a global-norm or value clip or a decay]
  static const decltype(&wn_adam_kernel<false, false, false>) kernels[2][2][2] = {
      {{wn_adam_kernel<false, false, false>, wn_adam_kernel<false, false, true>},
       {wn_adam_kernel<false, true, false>, wn_adam_kernel<false, true, true>}},
      {{wn_adam_kernel<true, false, false>, wn_adam_kernel<true, false, true>},
       {wn_adam_kernel<true, true, false>, wn_adam_kernel<true, true, true>}}};
  const bool keywords = x.clip_mode == WN_CLIP_GLOBAL_NORM || x.clip_mode == WN_CLIP_VALUE || x.wd > 0.f;
  auto k = kernels[x.a != nullptr][x.vhat != nullptr][keywords];
  hipLaunchKernelGGL(k, dim3(32, x.n), dim3(256), 0, s, x.p, x.g, x.m, x.v, x.vhat, x.a, x.table, x.n, x.norms2, x.clip_mode,
                     x.clip, x.lr, x.wd, x.decay_flags, x.alpha, x.beta1, x.beta2, x.eps, x.momentum, x.first, x.overwrite,
                     x.skip_flag);
  WN_HIP_CHECK(hipGetLastError());
  return WN_OK;
}

// The global-norm and value clips ahead of the data-parallel all-reduce (Adam(clip_before_reduce=True)), in place on the
// replica's own gradient.  Scalar accesses over the tensors of the table, as the Adam kernel above: every access lies inside
// [off, off + len) of a tensor, so nothing behind the last gradient (the step's scalars) is read or written.  The global
// form runs behind wn_sumsq_kernel and writes nothing when the gradient is inside the bound (scale exactly 1.0f); the
// value form writes only the elements it clamps.
__global__ void wn_scale_global_kernel(float* g, const WnTensorDesc* table, int n, const float* norms2, float clip) {
  const float scale = wn_global_clip_scale(norms2, n, clip);
  if (scale == 1.0f) return;       // uniform: the whole gradient stays bit-identical
  const WnTensorDesc d = table[blockIdx.y];
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < d.len;
       i += (int64_t)gridDim.x * blockDim.x)
    g[d.off + i] *= scale;
}
__global__ void wn_clip_value_kernel(float* g, const WnTensorDesc* table, float clip) {
  const WnTensorDesc d = table[blockIdx.y];
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < d.len;
       i += (int64_t)gridDim.x * blockDim.x) {
    const float gr = g[d.off + i];
    if (gr < -clip) g[d.off + i] = -clip;
    else if (gr > clip) g[d.off + i] = clip;
  }
}
int wn_launch_scale_global(float* g, const WnTensorDesc* d_table, int n, const float* norms2, float clip, hipStream_t s) {
  if (n <= 0) return WN_OK;
  hipLaunchKernelGGL(wn_scale_global_kernel, dim3(32, n), dim3(256), 0, s, g, d_table, n, norms2, clip);
  WN_HIP_CHECK(hipGetLastError());
  return WN_OK;
}
int wn_launch_clip_value(float* g, const WnTensorDesc* d_table, int n, float clip, hipStream_t s) {
  if (n <= 0) return WN_OK;
  hipLaunchKernelGGL(wn_clip_value_kernel, dim3(32, n), dim3(256), 0, s, g, d_table, clip);
  WN_HIP_CHECK(hipGetLastError());
  return WN_OK;
}

// Gradient accumulation (Adam(gradient_accumulation_steps=k)), beside the Adam launch and not inside it.  One grid-stride
// kernel over two flat buffers of n floats, the mode a template argument; per element, fp32, one correctly rounded operation
// each and nothing fused:
//   WN_ACCUM_FIRST   acc = g                       (an overwrite: whatever acc held is not read)
//   WN_ACCUM_ADD     acc = acc + g
//   WN_ACCUM_FINISH  g = (g + acc) / steps         (acc is not written)
// A raised skip_flag leaves both buffers alone (uniform).  vec: both pointers are 16-byte aligned, the first n / 4 * 4
// elements move as float4 and the second loop takes the n % 4 behind them; otherwise the second loop takes all n.  No access
// leaves [0, n) of either buffer: the step's scalars sit right behind the gradient.
// WN_ACCUM_ONE_PASS (include/wn_hip.h) = WN_ACCUM_MAX_BLOCKS * WN_ACCUM_THREADS * 4 floats is what the largest grid covers
// without a second trip round the loop: the 1.25 M parameters of the benchmarked network take one.
#define WN_ACCUM_THREADS 256
#define WN_ACCUM_MAX_BLOCKS 2048
static_assert((int64_t)WN_ACCUM_MAX_BLOCKS * WN_ACCUM_THREADS * 4 == WN_ACCUM_ONE_PASS, "wn_hip.h states the coverage");
template <int MODE>
__device__ __forceinline__ void wn_accum_one(float& a, float& g, float steps) {
  if (MODE == WN_ACCUM_FIRST) a = g;
  else if (MODE == WN_ACCUM_ADD) a = a + g;
  else g = (g + a) / steps;
}
template <int MODE>
__global__ void __launch_bounds__(WN_ACCUM_THREADS)
wn_grad_accumulate_kernel(float* acc, float* g, int64_t n, float steps, int vec, const float* skip_flag) {
  if (skip_flag && *skip_flag != 0.f) return;     // range guard tripped: the pass does not reach the accumulator
  const int64_t tid = (int64_t)blockIdx.x * WN_ACCUM_THREADS + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * WN_ACCUM_THREADS;
  const int64_t nvec = vec ? n >> 2 : 0;
  float4* av = reinterpret_cast<float4*>(acc);
  float4* gv = reinterpret_cast<float4*>(g);
  for (int64_t i = tid; i < nvec; i += stride) {
    float4 x = gv[i];
    float4 a = MODE == WN_ACCUM_FIRST ? x : av[i];
    wn_accum_one<MODE>(a.x, x.x, steps); wn_accum_one<MODE>(a.y, x.y, steps);
    wn_accum_one<MODE>(a.z, x.z, steps); wn_accum_one<MODE>(a.w, x.w, steps);
    if (MODE == WN_ACCUM_FINISH) gv[i] = x; else av[i] = a;
  }
  for (int64_t i = 4 * nvec + tid; i < n; i += stride) {
    float x = g[i];
    float a = MODE == WN_ACCUM_FIRST ? x : acc[i];
    wn_accum_one<MODE>(a, x, steps);
    if (MODE == WN_ACCUM_FINISH) g[i] = x; else acc[i] = a;
  }
}
int wn_launch_grad_accumulate(float* acc, float* g, int64_t n, int mode, float steps, const float* skip_flag, hipStream_t s) {
  if (n <= 0) return WN_OK;
  const int vec = (((uintptr_t)acc | (uintptr_t)g) & 15u) == 0;
  const int64_t units = vec ? (n >> 2) + (n & 3) : n;       // threads that have an element of either loop
  int64_t blocks = (units + WN_ACCUM_THREADS - 1) / WN_ACCUM_THREADS;
  if (blocks > WN_ACCUM_MAX_BLOCKS) blocks = WN_ACCUM_MAX_BLOCKS;
  auto k = mode == WN_ACCUM_FIRST ? wn_grad_accumulate_kernel<WN_ACCUM_FIRST>
           : mode == WN_ACCUM_ADD ? wn_grad_accumulate_kernel<WN_ACCUM_ADD> : wn_grad_accumulate_kernel<WN_ACCUM_FINISH>;
  hipLaunchKernelGGL(k, dim3((unsigned)blocks), dim3(WN_ACCUM_THREADS), 0, s, acc, g, n, steps, vec, skip_flag);
  WN_HIP_CHECK(hipGetLastError());
  return WN_OK;
}

// ------------------------------------------------------------------------------------------
// C-ABI (include/wn_hip.h): every entry point validates its own arguments under its own name, fills a wn_adam_options and
// calls adam_apply / clip_apply.

// one WN_CLIP_* bit with a finite value > 0 (or, where allowed, no bit at all)
static int check_clip(const char* who, int32_t mode, float clip, bool none_ok) {
  if (mode == WN_CLIP_NONE && none_ok) return WN_OK;
  if (mode != WN_CLIP_NORM && mode != WN_CLIP_GLOBAL_NORM && mode != WN_CLIP_VALUE) {
    wn_set_error("%s: clip_mode must be exactly one of WN_CLIP_NORM, WN_CLIP_GLOBAL_NORM, WN_CLIP_VALUE%s (got %d): only one "
                 "of clipnorm, clipvalue and global_clipnorm can be set", who, none_ok ? " or WN_CLIP_NONE" : "", (int)mode);
    return WN_E_INVALID;
  }
  if (!(clip > 0.f) || !std::isfinite(clip)) {
    wn_set_error("%s: clip must be finite and > 0 (got %g)", who, (double)clip);
    return WN_E_INVALID;
  }
  return WN_OK;
}

static int check_ema(const char* who, float momentum, int32_t overwrite) {
  if (!std::isfinite(momentum) || momentum < 0.f || momentum > 1.f) {
    wn_set_error("%s: ema_momentum must be finite and in [0, 1] (got %g)", who, (double)momentum);
    return WN_E_INVALID;
  }
  if (overwrite != 0 && overwrite != 1) { wn_set_error("%s: ema_overwrite must be 0 or 1 (got %d)", who, (int)overwrite); return WN_E_INVALID; }
  return WN_OK;
}

// The step behind every wn_adam_step*: arguments are valid.  vhat is used under o.amsgrad only, ema when it is non-null.
static int adam_apply(wn_plan* p, float* params, const float* grads, float* m, float* v, float* vhat, float* ema, int64_t step,
                      const wn_adam_options& o, float* scratch, const float* skip_flag, hipStream_t s) {
  int rc = wnp::ensure_device_tables(p);
  if (rc) return rc;
  const int n = (int)p->tdesc.size();
  if (o.clip_mode == WN_CLIP_NORM || o.clip_mode == WN_CLIP_GLOBAL_NORM) {
    rc = wn_launch_sumsq(grads, p->d_tdesc, n, scratch, s);
    if (rc) return rc;
  }
  const double alpha = (double)o.lr * sqrt(1.0 - pow((double)o.beta2, (double)step)) / (1.0 - pow((double)o.beta1, (double)step));
  WnAdamArgs x;
  x.p = params; x.g = grads; x.m = m; x.v = v; x.vhat = o.amsgrad ? vhat : nullptr; x.a = ema;
  x.table = p->d_tdesc; x.n = n; x.norms2 = scratch;
  x.clip_mode = o.clip_mode; x.clip = o.clip; x.lr = o.lr; x.wd = o.weight_decay; x.decay_flags = o.decay_flags;
  x.alpha = (float)alpha; x.beta1 = o.beta1; x.beta2 = o.beta2; x.eps = o.eps;
  x.momentum = o.ema_momentum; x.first = step == 1 ? 1 : 0; x.overwrite = (int)o.ema_overwrite; x.skip_flag = skip_flag;
  return wn_launch_adam(x, s);
}

// the options of the two steps that predate wn_adam_options: clipnorm <= 0 (or NaN) is no clip, and nothing else is on
static wn_adam_options legacy_options(float lr, float beta1, float beta2, float eps, float clipnorm) {
  wn_adam_options o = {};
  o.lr = lr; o.beta1 = beta1; o.beta2 = beta2; o.eps = eps;
  o.clip_mode = clipnorm > 0.f ? WN_CLIP_NORM : WN_CLIP_NONE;
  o.clip = clipnorm;
  return o;
}

extern "C" int wn_adam_step_guarded(wn_plan* p, float* params, const float* grads, float* m, float* v, int64_t step,
                                    float lr, float beta1, float beta2, float eps, float clipnorm, float* scratch,
                                    const float* skip_flag, void* stream) {
  if (!p || !params || !grads || !m || !v || !scratch || step < 1) { wn_set_error("adam_step: bad arguments"); return WN_E_INVALID; }
  return adam_apply(p, params, grads, m, v, nullptr, nullptr, step, legacy_options(lr, beta1, beta2, eps, clipnorm), scratch,
                    skip_flag, (hipStream_t)stream);
}

extern "C" int wn_adam_step(wn_plan* p, float* params, const float* grads, float* m, float* v, int64_t step,
                            float lr, float beta1, float beta2, float eps, float clipnorm, float* scratch,
                            void* stream) {
  return wn_adam_step_guarded(p, params, grads, m, v, step, lr, beta1, beta2, eps, clipnorm, scratch, nullptr, stream);
}

extern "C" int wn_adam_step_ema(wn_plan* p, float* params, const float* grads, float* m, float* v, float* ema, int64_t step,
                                float lr, float beta1, float beta2, float eps, float clipnorm, float ema_momentum,
                                int32_t ema_overwrite, float* scratch, const float* skip_flag, void* stream) {
  if (!p || !params || !grads || !m || !v || !ema || !scratch || step < 1) { wn_set_error("adam_step_ema: bad arguments"); return WN_E_INVALID; }
  if (check_ema("adam_step_ema", ema_momentum, ema_overwrite)) return WN_E_INVALID;
  wn_adam_options o = legacy_options(lr, beta1, beta2, eps, clipnorm);
  o.ema_momentum = ema_momentum;
  o.ema_overwrite = ema_overwrite;
  return adam_apply(p, params, grads, m, v, nullptr, ema, step, o, scratch, skip_flag, (hipStream_t)stream);
}

extern "C" int wn_adam_step_ext(wn_plan* p, float* params, const float* grads, float* m, float* v, float* vhat, float* ema,
                                int64_t step, const wn_adam_options* o, float* scratch, const float* skip_flag,
                                void* stream) {
  const char* null_arg = !p ? "plan" : !params ? "params" : !grads ? "grads" : !m ? "m" : !v ? "v" : !o ? "options"
                         : !scratch ? "scratch" : nullptr;
  if (null_arg) { wn_set_error("adam_step_ext: %s is NULL", null_arg); return WN_E_INVALID; }
  if (step < 1) { wn_set_error("adam_step_ext: step must be >= 1 (got %lld)", (long long)step); return WN_E_INVALID; }
  if (check_clip("adam_step_ext", o->clip_mode, o->clip, true)) return WN_E_INVALID;
  if (!(o->weight_decay >= 0.f) || !std::isfinite(o->weight_decay)) {
    wn_set_error("adam_step_ext: weight_decay must be finite and >= 0 (got %g)", (double)o->weight_decay);
    return WN_E_INVALID;
  }
  if (o->amsgrad != 0 && o->amsgrad != 1) { wn_set_error("adam_step_ext: amsgrad must be 0 or 1 (got %d)", (int)o->amsgrad); return WN_E_INVALID; }
  if (o->amsgrad && !vhat) { wn_set_error("adam_step_ext: amsgrad without vhat (vhat is NULL)"); return WN_E_INVALID; }
  if (check_ema("adam_step_ext", o->ema_momentum, o->ema_overwrite)) return WN_E_INVALID;
  if (!ema && (o->ema_momentum != 0.f || o->ema_overwrite != 0)) {
    wn_set_error("adam_step_ext: ema_momentum / ema_overwrite set without ema (ema is NULL)");
    return WN_E_INVALID;
  }
  return adam_apply(p, params, grads, m, v, vhat, ema, step, *o, scratch, skip_flag, (hipStream_t)stream);
}

// the clip behind both wn_clip_gradients*: mode is one WN_CLIP_* bit, clip finite and > 0
static int clip_apply(wn_plan* p, float* grads, int32_t mode, float clip, float* scratch, hipStream_t s) {
  int rc = wnp::ensure_device_tables(p);
  if (rc) return rc;
  const int n = (int)p->tdesc.size();
  if (mode == WN_CLIP_NORM) return wn_launch_clip(grads, p->d_tdesc, n, clip, scratch, s);
  if (mode == WN_CLIP_VALUE) return wn_launch_clip_value(grads, p->d_tdesc, n, clip, s);
  rc = wn_launch_sumsq(grads, p->d_tdesc, n, scratch, s);
  if (rc) return rc;
  return wn_launch_scale_global(grads, p->d_tdesc, n, scratch, clip, s);
}

extern "C" int wn_clip_gradients(wn_plan* p, float* grads, float clipnorm, float* scratch, void* stream) {
  if (!p || !grads || !scratch) { wn_set_error("clip_gradients: bad arguments"); return WN_E_INVALID; }
  if (!(clipnorm > 0.f) || !std::isfinite(clipnorm)) { wn_set_error("clip_gradients: clipnorm must be finite and > 0 (got %g)", (double)clipnorm); return WN_E_INVALID; }
  return clip_apply(p, grads, WN_CLIP_NORM, clipnorm, scratch, (hipStream_t)stream);
}

extern "C" int wn_clip_gradients_ext(wn_plan* p, float* grads, int32_t clip_mode, float clip, float* scratch, void* stream) {
  const char* null_arg = !p ? "plan" : !grads ? "grads" : !scratch ? "scratch" : nullptr;
  if (null_arg) { wn_set_error("clip_gradients_ext: %s is NULL", null_arg); return WN_E_INVALID; }
  if (check_clip("clip_gradients_ext", clip_mode, clip, false)) return WN_E_INVALID;
  return clip_apply(p, grads, clip_mode, clip, scratch, (hipStream_t)stream);
}

// Takes no plan: two flat buffers and a count.  Everything is checked before the device is touched.
extern "C" int wn_grad_accumulate(float* acc, float* grads, int64_t n, int32_t mode, int32_t steps, const float* skip_flag,
                                  void* stream) {
  const char* null_arg = !acc ? "acc" : !grads ? "grads" : nullptr;
  if (null_arg) { wn_set_error("grad_accumulate: %s is NULL", null_arg); return WN_E_INVALID; }
  if (n < 0) { wn_set_error("grad_accumulate: n must be >= 0 (got %lld)", (long long)n); return WN_E_INVALID; }
  if (mode != WN_ACCUM_FIRST && mode != WN_ACCUM_ADD && mode != WN_ACCUM_FINISH) {
    wn_set_error("grad_accumulate: mode must be WN_ACCUM_FIRST, WN_ACCUM_ADD or WN_ACCUM_FINISH (got %d)", (int)mode);
    return WN_E_INVALID;
  }
  if (mode == WN_ACCUM_FINISH && steps < 2) {
    wn_set_error("grad_accumulate: steps must be >= 2 in WN_ACCUM_FINISH (got %d)", (int)steps);
    return WN_E_INVALID;
  }
  return wn_launch_grad_accumulate(acc, grads, n, mode, (float)steps, skip_flag, (hipStream_t)stream);
}
