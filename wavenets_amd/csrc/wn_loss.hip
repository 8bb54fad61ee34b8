// Softmax, loss and reduction kernels of the WaveNet hot path (gfx950).  The categorical row arithmetic is that of
// wn_catrow.h; losses src/model.py:505-551.
#include <algorithm>

#include "wn_kernels.h"
#include "wn_sample.h"

__global__ __launch_bounds__(256) void wn_softmax_kernel(const float* logits, float* probs,
                                                         int64_t rows, int C) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  WnSoftmaxLoop(logits + row * C, C, lane).each([&](int j, float q) { probs[row * C + j] = q; });
}
int wn_launch_softmax(const float* logits, float* probs, int64_t rows, int C, hipStream_t s) {
  if (rows <= 0) return WN_OK;
  hipLaunchKernelGGL(wn_softmax_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, s, logits,
                     probs, rows, C);
  WN_HIP_CHECK(hipGetLastError());
  return WN_OK;
}

// Keras sparse_categorical_crossentropy(target, softmax(logits)), from_logits=False, and its gradient w.r.t. the logits:
// wn_cat_ce_row (wn_catrow.h) on the softmax row of the logits.
// sample_out (C <= 256 only): also draw sample_waveform(softmax(logits)) of the row (src/model.py:338,407-411)
// from the probabilities already in registers -- the values wn_softmax_kernel would write, the draw
// wn_sample_rand_cat_kernel would make from them.
// C <= 256, the shape of every BASELINE categorical head: persistent waves, one row at a time per wave with the NEXT row's
// logits and target already requested (a one-row-per-wave launch spends most of a row waiting for its loads: 172 us for
// 268 MB); the row lives in registers, and the max-abs of the gradients is published once per wave.
// WEIGHTED (sample_weight): weight[row] goes through wn_cat_ce_row; the next row's weight travels with
// its prefetch.  The two __global__ functions below are the instantiations: the one without weights keeps its arguments.
template <bool WEIGHTED>
__device__ __forceinline__ void wn_cat_loss256_body(const float* logits, const int32_t* target, int64_t rows, int C, float gscale,
                                                    float* loss_rows, float* g_logits, float* absmax_out, float* sample_out,
                                                    float inv_lv, uint64_t seed, uint64_t offset, const float* weight) {
  __shared__ float qs[4][256];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int64_t stride = (int64_t)gridDim.x * 4;
  int64_t row = (int64_t)blockIdx.x * 4 + w;
  float vn[4];
  int tn = 0;
  float wnx = 1.0f;
  auto fetch = [&](int64_t r) {
    wn_cat_load4(logits + r * C, C, lane, vn);
    tn = target[r];
    if constexpr (WEIGHTED) wnx = weight[r];
  };
  if (row < rows) fetch(row);
  float gmax = 0.f;
  for (; row < rows; row += stride) {
    float v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = vn[k];
    const int tgt = tn;
    const float rw = wnx;
    if (row + stride < rows) fetch(row + stride);     // in flight while this row is worked on
    const WnSoftmaxRegs r(v, C, lane);
    if (sample_out) {
      float* qw = qs[w];
      r.each([&](int j, float q) { qw[j] = q; });
      __builtin_amdgcn_wave_barrier();
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      const int drawn = wn_draw_cat_row((const float*)qw, C, lane, row, seed, offset);
      if (lane == 0) sample_out[row] = (float)drawn * inv_lv - 1.0f;
      __builtin_amdgcn_wave_barrier();                // the next row rewrites qw
    }
    wn_cat_ce_row<WEIGHTED>(r, tgt, gscale, loss_rows + row, g_logits, row * C, gmax, rw);
  }
  if (g_logits && absmax_out) {
    gmax = wn_wave_max(gmax);
    if (lane == 0) wn_absmax_publish(absmax_out, gmax);
  }
}
__global__ __launch_bounds__(256) void wn_cat_loss256_kernel(const float* logits, const int32_t* target,
                                                             int64_t rows, int C, float gscale,
                                                             float* loss_rows, float* g_logits, float* absmax_out,
                                                             float* sample_out, float inv_lv, uint64_t seed, uint64_t offset) {
  wn_cat_loss256_body<false>(logits, target, rows, C, gscale, loss_rows, g_logits, absmax_out, sample_out, inv_lv, seed, offset, nullptr);
}
__global__ __launch_bounds__(256) void wn_cat_loss256_weighted_kernel(const float* logits, const int32_t* target,
                                                                      int64_t rows, int C, float gscale,
                                                                      float* loss_rows, float* g_logits, float* absmax_out,
                                                                      float* sample_out, float inv_lv, uint64_t seed, uint64_t offset,
                                                                      const float* weight) {
  wn_cat_loss256_body<true>(logits, target, rows, C, gscale, loss_rows, g_logits, absmax_out, sample_out, inv_lv, seed, offset, weight);
}

// more than 256 classes: one row per wave, the row re-read from memory on every pass
template <bool WEIGHTED>
__device__ __forceinline__ void wn_cat_loss_body(const float* logits, const int32_t* target, int64_t rows, int C, float gscale,
                                                 float* loss_rows, float* g_logits, float* absmax_out, const float* weight) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  float gmax = 0.f;
  float rw = 1.0f;
  if constexpr (WEIGHTED) rw = weight[row];
  wn_cat_ce_row<WEIGHTED>(WnSoftmaxLoop(logits + row * C, C, lane), target[row], gscale, loss_rows + row, g_logits, row * C, gmax, rw);
  if (g_logits && absmax_out) {
    gmax = wn_wave_max(gmax);
    if (lane == 0) wn_absmax_publish(absmax_out, gmax);
  }
}
__global__ __launch_bounds__(256) void wn_cat_loss_kernel(const float* logits, const int32_t* target,
                                                          int64_t rows, int C, float gscale,
                                                          float* loss_rows, float* g_logits, float* absmax_out) {
  wn_cat_loss_body<false>(logits, target, rows, C, gscale, loss_rows, g_logits, absmax_out, nullptr);
}
__global__ __launch_bounds__(256) void wn_cat_loss_weighted_kernel(const float* logits, const int32_t* target,
                                                                   int64_t rows, int C, float gscale,
                                                                   float* loss_rows, float* g_logits, float* absmax_out,
                                                                   const float* weight) {
  wn_cat_loss_body<true>(logits, target, rows, C, gscale, loss_rows, g_logits, absmax_out, weight);
}
int wn_launch_cat_loss(const float* logits, const int32_t* target, int64_t rows, int C,
                       float gscale, float* loss_rows, float* g_logits, float* absmax_out, hipStream_t s,
                       float* sample_out, int bits, uint64_t seed, uint64_t offset, const float* weight) {
  if (rows <= 0) return WN_OK;
  if (sample_out && C > 256) { wn_set_error("cat_loss: the in-kernel sample draw needs <= 256 classes"); return WN_E_UNSUPPORTED; }
  const float inv_lv = sample_out ? 1.0f / (float)(1 << (bits - 1)) : 0.f;
  if (C <= 256) {
    const int64_t wgs = std::min<int64_t>((rows + 3) / 4, 256 * 8);
    if (weight) hipLaunchKernelGGL(wn_cat_loss256_weighted_kernel, dim3((unsigned)wgs), dim3(256), 0, s, logits, target, rows, C,
                                   gscale, loss_rows, g_logits, absmax_out, sample_out, inv_lv, seed, offset, weight);
    else hipLaunchKernelGGL(wn_cat_loss256_kernel, dim3((unsigned)wgs), dim3(256), 0, s, logits, target, rows, C, gscale,
                            loss_rows, g_logits, absmax_out, sample_out, inv_lv, seed, offset);
  } else if (weight) {
    hipLaunchKernelGGL(wn_cat_loss_weighted_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, s, logits,
                       target, rows, C, gscale, loss_rows, g_logits, absmax_out, weight);
  } else {
    hipLaunchKernelGGL(wn_cat_loss_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, s, logits,
                       target, rows, C, gscale, loss_rows, g_logits, absmax_out);
  }
  WN_HIP_CHECK(hipGetLastError());
  return WN_OK;
}

// ------------------------------------------------------------------------------------------
// Seeds of a backward pass that starts from a caller's gradient (wn_vjp): they leave
// d<g, out>/d(logits) where the loss kernels above leave d loss / d logits, with the same max-abs publication (the
// split-precision backward products scale their operand by that slot).
// Softmax vector-Jacobian product: g is the gradient at the probabilities q = softmax(l) that wn_softmax_kernel wrote
// (the row in either storage form holds the same bits),  dot = sum_j g_j q_j  (a lane sums its classes lane, lane + 64, ...
// in that order, then wn_wave_sum),  dl_j = q_j (g_j - dot).  Plain fp32, nothing clipped: a non-finite g gives a
// non-finite row.  Persistent waves, one row at a time per wave, one publication per wave.
template <bool REGS>
__global__ __launch_bounds__(256) void wn_softmax_vjp_kernel(const float* logits, const float* g, int64_t rows, int C,
                                                             float* dl, float* absmax_out) {
  const int lane = threadIdx.x & 63;
  const int64_t stride = (int64_t)gridDim.x * 4;
  float gmax = 0.f;
  for (int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); row < rows; row += stride) {
    const float* gr = g + row * C;
    float* dr = dl + row * C;
    auto vjp = [&](const auto& r) {
      float dot = 0.f;
      r.each([&](int j, float q) { dot += gr[j] * q; });
      dot = wn_wave_sum(dot);
      r.each([&](int j, float q) {
        const float d = q * (gr[j] - dot);
        dr[j] = d;
        gmax = fmaxf(gmax, fabsf(d));
      });
    };
    if (REGS) {
      float v[4];
      wn_cat_load4(logits + row * C, C, lane, v);
      vjp(WnSoftmaxRegs(v, C, lane));
    } else {
      vjp(WnSoftmaxLoop(logits + row * C, C, lane));
    }
  }
  if (absmax_out) {
    gmax = wn_wave_max(gmax);
    if (lane == 0) wn_absmax_publish(absmax_out, gmax);
  }
}
// identity seed (gradient given at the logits, or at the linear parameters of a mixture head): a copy with the publication
__global__ __launch_bounds__(256) void wn_seed_copy_kernel(const float* g, int64_t n, float* dl, float* absmax_out) {
  float gmax = 0.f;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const float v = g[i];
    dl[i] = v;
    gmax = fmaxf(gmax, fabsf(v));
  }
  if (absmax_out) {
    gmax = wn_wave_max(gmax);
    if ((threadIdx.x & 63) == 0) wn_absmax_publish(absmax_out, gmax);
  }
}
int wn_launch_vjp_seed(const float* logits, const float* g, int64_t rows, int C, int through_softmax, float* dl,
                       float* absmax_out, hipStream_t s) {
  if (rows <= 0 || C <= 0) return WN_OK;
  if (!through_softmax) {
    hipLaunchKernelGGL(wn_seed_copy_kernel, dim3(wn_blocks(rows * C, 256, 2048)), dim3(256), 0, s, g, rows * C, dl, absmax_out);
  } else {
    const dim3 grid((unsigned)std::min<int64_t>((rows + 3) / 4, 256 * 8));
    if (C <= 256) hipLaunchKernelGGL(wn_softmax_vjp_kernel<true>, grid, dim3(256), 0, s, logits, g, rows, C, dl, absmax_out);
    else hipLaunchKernelGGL(wn_softmax_vjp_kernel<false>, grid, dim3(256), 0, s, logits, g, rows, C, dl, absmax_out);
  }
  WN_HIP_CHECK(hipGetLastError());
  return WN_OK;
}

__global__ __launch_bounds__(256) void wn_cat_loss_probs_kernel(const float* probs,
                                                                const int32_t* target, int64_t rows,
                                                                int C, float* loss_rows) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const float* q = probs + row * C;
  float S = 0.f;
  for (int j = lane; j < C; j += 64) S += wn_ce_clip(q[j]);
  S = wn_wave_sum(S);
  const float pt = wn_ce_clip(q[wn_ce_target(target[row], C)]);
  if (lane == 0) loss_rows[row] = wn_ce_loss(pt, S);
}
int wn_launch_cat_loss_probs(const float* probs, const int32_t* target, int64_t rows, int C,
                             float* loss_rows, hipStream_t s) {
  if (rows <= 0) return WN_OK;
  hipLaunchKernelGGL(wn_cat_loss_probs_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, s,
                     probs, target, rows, C, loss_rows);
  WN_HIP_CHECK(hipGetLastError());
  return WN_OK;
}

// mixture losses, one thread per (b,t) row; M <= 32.  Evaluated in double: with bits = 16 the
// half-bin (src/model.py:538) is 7.6e-6, so sigmoid(a) - sigmoid(b) cancels ~5 digits and an
// fp32 evaluation (the reference's own included) carries 1e-3..1e-2 relative noise per term.
// The logistic bin mass sigmoid(a) - sigmoid(b) is taken on the negative side: above a sharp component's mean both
// sigmoids round to 1 (from (y - mu) e^-ls ~ 37 on; digits go from ~20 on) and the mass is lost -- inf loss, NaN gradients
// -- where the mirrored row below the mean is exact.  sigmoid(x) = 1 - sigmoid(-x): when a + b > 0 the mass is
// sigmoid(-b) - sigmoid(-a), and sigmoid'(x) = sigmoid(x) sigmoid(-x) is even.  
#define WN_MAXMIX 32
__device__ __forceinline__ double wn_sigmoid_d(double x) { return 1.0 / (1.0 + exp(-x)); }
__device__ __forceinline__ double wn_dsigmoid_d(double x) { return wn_sigmoid_d(x) * wn_sigmoid_d(-x); }
// the bin's edges (hi >= lo, hi + lo <= 0) on the side where the mass is sigmoid(hi) - sigmoid(lo); true: mirrored
__device__ __forceinline__ bool wn_logistic_bin(double a, double b, double& hi, double& lo) {
  const bool up = a + b > 0.0;
  hi = up ? -b : a;
  lo = up ? -a : b;
  return up;
}
// WEIGHTED (sample_weight; the factor of wn_catrow.h): dl = -(double)(gscale * w) / lik, the stored loss
// is w * (float)(-log lik); a row with w == 0 writes its zeros and returns before anything of it is evaluated, so a
// likelihood that underflows there (section 17's open case) reaches neither the loss, the gradient nor the max-abs.
template <bool WEIGHTED>
__device__ __forceinline__ void wn_mix_loss_body(const float* pred, const float* y, int64_t rows, int M, int bits, int kind,
                                                 float gscale, float* loss_rows, float* g_pred, float* absmax_out,
                                                 const float* weight) {
  const int64_t row = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= rows) return;
  float rw = 1.0f;
  if constexpr (WEIGHTED) {
    rw = weight[row];
    if (rw == 0.f) {
      loss_rows[row] = 0.f;
      if (g_pred)
        for (int k = 0; k < 3 * M; ++k) g_pred[row * 3 * M + k] = 0.f;
      return;
    }
    gscale = wn_w_gscale(gscale, rw);
  }
  const float* p = pred + row * 3 * M;
  const double yy = (double)y[row];
  double w[WN_MAXMIX], comp[WN_MAXMIX];
  double wm = -INFINITY;
  for (int k = 0; k < M; ++k) wm = fmax(wm, (double)p[k]);
  double wz = 0.0;
  for (int k = 0; k < M; ++k) { w[k] = exp((double)p[k] - wm); wz += w[k]; }
  const double winv = 1.0 / wz;
  const double halfbit = 0.5 / (double)(1 << bits);                      // src/model.py:538
  const double sqrt2pi = sqrt(2.0 * 3.14159265359);                      // src/model.py:9
  double lik = 0.0;
  for (int k = 0; k < M; ++k) {
    w[k] *= winv;
    const double mu = (double)p[M + k];
    const double ls = fmax((double)p[2 * M + k], -7.0);
    if (kind == 1) {
      const double inv = exp(-ls);
      double hi, lo;
      wn_logistic_bin((yy - mu + halfbit) * inv, (yy - mu - halfbit) * inv, hi, lo);
      comp[k] = wn_sigmoid_d(hi) - wn_sigmoid_d(lo);
    } else {
      const double sc = exp(ls);
      const double xx = fmin((yy - mu) / sc, 1e8);
      comp[k] = exp(-0.5 * xx * xx) / (sc * sqrt2pi);
    }
    lik += w[k] * comp[k];
  }
  loss_rows[row] = WEIGHTED ? rw * (float)(-log(lik)) : (float)(-log(lik));
  if (!g_pred) return;
  float* g = g_pred + row * 3 * M;
  const double dl = -(double)gscale / lik;                               // dL/dlik
  for (int k = 0; k < M; ++k) {
    const double mu = (double)p[M + k];
    const double lsr = (double)p[2 * M + k];
    const double ls = fmax(lsr, -7.0);
    const double lsmask = lsr >= -7.0 ? 1.0 : 0.0;
    g[k] = (float)(dl * (w[k] * comp[k] - w[k] * lik));
    if (kind == 1) {
      const double inv = exp(-ls);
      double hi, lo;
      const bool up = wn_logistic_bin((yy - mu + halfbit) * inv, (yy - mu - halfbit) * inv, hi, lo);
      const double dhi = wn_dsigmoid_d(hi), dlo = wn_dsigmoid_d(lo);
      // mirrored: a = -lo, b = -hi, so sigmoid'(a) - sigmoid'(b) changes sign and a sigmoid'(a) - b sigmoid'(b) does not
      g[M + k] = (float)(dl * (-w[k] * inv * (up ? dlo - dhi : dhi - dlo)));
      g[2 * M + k] = (float)(dl * lsmask * (-w[k] * (hi * dhi - lo * dlo)));
    } else {
      const double sc = exp(ls);
      const double xr = (yy - mu) / sc;
      const double xx = fmin(xr, 1e8);
      const double xmask = xr <= 1e8 ? 1.0 : 0.0;
      const double pdf = comp[k];
      // d pdf/d mu = pdf * xx / sc ; d pdf/d ls = pdf * (xx^2 - 1)
      g[M + k] = (float)(dl * w[k] * pdf * xx / sc * xmask);
      g[2 * M + k] = (float)(dl * lsmask * w[k] * pdf * (xx * xx * xmask - 1.0));
    }
  }
  if (absmax_out) {
    float gmax = 0.f;
    for (int k = 0; k < 3 * M; ++k) gmax = fmaxf(gmax, fabsf(g[k]));
    wn_absmax_publish(absmax_out, gmax);
  }
}
__global__ void wn_mix_loss_kernel(const float* pred, const float* y, int64_t rows, int M, int bits,
                                   int kind, float gscale, float* loss_rows, float* g_pred, float* absmax_out) {
  wn_mix_loss_body<false>(pred, y, rows, M, bits, kind, gscale, loss_rows, g_pred, absmax_out, nullptr);
}
__global__ void wn_mix_loss_weighted_kernel(const float* pred, const float* y, int64_t rows, int M, int bits,
                                            int kind, float gscale, float* loss_rows, float* g_pred, float* absmax_out,
                                            const float* weight) {
  wn_mix_loss_body<true>(pred, y, rows, M, bits, kind, gscale, loss_rows, g_pred, absmax_out, weight);
}
int wn_launch_mix_loss(const float* pred, const float* y, int64_t rows, int M, int bits, int kind,
                       float gscale, float* loss_rows, float* g_pred, float* absmax_out, hipStream_t s, const float* weight) {
  if (rows <= 0) return WN_OK;
  if (M < 1 || M > WN_MAXMIX) { wn_set_error("mix_loss: num_mixtures %d unsupported (max %d)", M, WN_MAXMIX); return WN_E_UNSUPPORTED; }
  if (weight) hipLaunchKernelGGL(wn_mix_loss_weighted_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, s, pred,
                                 y, rows, M, bits, kind, gscale, loss_rows, g_pred, absmax_out, weight);
  else hipLaunchKernelGGL(wn_mix_loss_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, s, pred,
                          y, rows, M, bits, kind, gscale, loss_rows, g_pred, absmax_out);
  WN_HIP_CHECK(hipGetLastError());
  return WN_OK;
}

// ------------------------------------------------------------------------------------------
// deterministic two-stage sum (double accumulation), out[0] = scale * sum(v)
__global__ void wn_sum_stage1(const float* v, int64_t n, double* scratch) {
  __shared__ double sm[256];
  double acc = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x)
    acc += (double)v[i];
  sm[threadIdx.x] = acc;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (threadIdx.x < o) sm[threadIdx.x] += sm[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) scratch[blockIdx.x] = sm[0];
}
__global__ void wn_sum_stage2(const double* scratch, int nb, float scale, float* out) {
  __shared__ double sm[256];
  double acc = 0.0;
  for (int i = threadIdx.x; i < nb; i += blockDim.x) acc += scratch[i];
  sm[threadIdx.x] = acc;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (threadIdx.x < o) sm[threadIdx.x] += sm[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[0] = (float)(sm[0] * (double)scale);
}
// scratch: >= 1024 doubles (8 KiB)
int wn_launch_sum(const float* v, int64_t n, float scale, float* out, float* scratch, hipStream_t s) {
  int nb = wn_blocks(n, 256, 1024);
  hipLaunchKernelGGL(wn_sum_stage1, dim3(nb), dim3(256), 0, s, v, n, reinterpret_cast<double*>(scratch));
  hipLaunchKernelGGL(wn_sum_stage2, dim3(1), dim3(256), 0, s, reinterpret_cast<const double*>(scratch), nb, scale, out);
  WN_HIP_CHECK(hipGetLastError());
  return WN_OK;
}

// Per-utterance sums of a scoring pass (wn_score): workgroup b owns utterance b.  Thread i adds the rows
// t = i, i + 256, ... of its utterance in that order, in double -- the rows as the loss kernels stored them, weighted rows
// already weighted, so the first sum is sum_t w l; the second is sum_t w from the weight buffer when one is armed -- then the
// tree of wn_sum_stage1 over the 256 partial sums, and one store as float.  No atomics, nothing shared between
// workgroups: the order of summation depends on T alone, so nll[b] is a function of utterance b's rows only, bit for bit.
__global__ __launch_bounds__(256) void wn_score_reduce_kernel(const float* rows, const float* weight, int T, float* nll,
                                                              float* wsum) {
  __shared__ double sl[256], sw[256];
  const int64_t base = (int64_t)blockIdx.x * T;
  double l = 0.0, w = 0.0;
  int t = threadIdx.x;
  // eight of a thread's rows requested before the first is added (8 workgroups at the configs[1] batch: one load per
  // trip would leave the kernel waiting for memory 63 times in a row); the adds keep the order t, t + 256, ...
  for (; t + 7 * 256 < T; t += 8 * 256) {
    float r[8], q[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      r[k] = rows[base + t + 256 * k];
      q[k] = weight ? weight[base + t + 256 * k] : 0.f;
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      l += (double)r[k];
      w += (double)q[k];
    }
  }
  for (; t < T; t += 256) {
    l += (double)rows[base + t];
    if (weight) w += (double)weight[base + t];
  }
  sl[threadIdx.x] = l;
  sw[threadIdx.x] = w;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (threadIdx.x < o) { sl[threadIdx.x] += sl[threadIdx.x + o]; sw[threadIdx.x] += sw[threadIdx.x + o]; }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    nll[blockIdx.x] = (float)sl[0];
    if (wsum) wsum[blockIdx.x] = weight ? (float)sw[0] : (float)T;
  }
}
int wn_launch_score_reduce(const float* rows, const float* weight, int B, int T, float* nll, float* wsum, hipStream_t s) {
  if (B <= 0 || T <= 0) return WN_OK;
  hipLaunchKernelGGL(wn_score_reduce_kernel, dim3((unsigned)B), dim3(256), 0, s, rows, weight, T, nll, wsum);
  WN_HIP_CHECK(hipGetLastError());
  return WN_OK;
}

// out[0] = scale * sum((a - b)^2): tf.keras.metrics.MeanSquaredError(y_true, sample) of a step (src/model.py:346,
// train.py:227) with scale = 1 / (n * replicas); same two-stage double accumulation as wn_launch_sum
__global__ void wn_sqdiff_stage1(const float* a, const float* b, int64_t n, double* scratch) {
  __shared__ double sm[256];
  double acc = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    const float d = a[i] - b[i];
    acc += (double)(d * d);
  }
  sm[threadIdx.x] = acc;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (threadIdx.x < o) sm[threadIdx.x] += sm[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) scratch[blockIdx.x] = sm[0];
}
int wn_launch_sqdiff_sum(const float* a, const float* b, int64_t n, float scale, float* out, float* scratch, hipStream_t s) {
  int nb = wn_blocks(n, 256, 1024);
  hipLaunchKernelGGL(wn_sqdiff_stage1, dim3(nb), dim3(256), 0, s, a, b, n, reinterpret_cast<double*>(scratch));
  hipLaunchKernelGGL(wn_sum_stage2, dim3(1), dim3(256), 0, s, reinterpret_cast<const double*>(scratch), nb, scale, out);
  WN_HIP_CHECK(hipGetLastError());
  return WN_OK;
}

// out[0] = scale * sum(w (a - b)^2) / sum(w), 0 when sum(w) == 0: Keras's weighted MeanSquaredError of one step (DESIGN.md
// section 25).  Numerator and denominator in one pass, the same two-stage double accumulation as above: block i leaves its
// two partial sums at scratch[i] and scratch[512 + i] (at most 512 blocks: the 1024 doubles of the other reductions' scratch).
__global__ void wn_wsqdiff_stage1(const float* a, const float* b, const float* w, int64_t n, double* scratch) {
  __shared__ double sn[256], sd[256];
  double num = 0.0, den = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    const float d = a[i] - b[i];
    const double wi = (double)w[i];
    num += wi * (double)(d * d);
    den += wi;
  }
  sn[threadIdx.x] = num;
  sd[threadIdx.x] = den;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (threadIdx.x < o) { sn[threadIdx.x] += sn[threadIdx.x + o]; sd[threadIdx.x] += sd[threadIdx.x + o]; }
    __syncthreads();
  }
  if (threadIdx.x == 0) { scratch[blockIdx.x] = sn[0]; scratch[512 + blockIdx.x] = sd[0]; }
}
__global__ void wn_wsqdiff_stage2(const double* scratch, int nb, float scale, float* out) {
  __shared__ double sn[256], sd[256];
  double num = 0.0, den = 0.0;
  for (int i = threadIdx.x; i < nb; i += blockDim.x) { num += scratch[i]; den += scratch[512 + i]; }
  sn[threadIdx.x] = num;
  sd[threadIdx.x] = den;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (threadIdx.x < o) { sn[threadIdx.x] += sn[threadIdx.x + o]; sd[threadIdx.x] += sd[threadIdx.x + o]; }
    __syncthreads();
  }
  if (threadIdx.x == 0) out[0] = sd[0] == 0.0 ? 0.f : (float)((double)scale * sn[0] / sd[0]);
}
// scratch: >= 1024 doubles (8 KiB)
int wn_launch_wsqdiff_mean(const float* a, const float* b, const float* w, int64_t n, float scale, float* out, float* scratch,
                           hipStream_t s) {
  int nb = wn_blocks(n, 256, 512);
  hipLaunchKernelGGL(wn_wsqdiff_stage1, dim3(nb), dim3(256), 0, s, a, b, w, n, reinterpret_cast<double*>(scratch));
  hipLaunchKernelGGL(wn_wsqdiff_stage2, dim3(1), dim3(256), 0, s, reinterpret_cast<const double*>(scratch), nb, scale, out);
  WN_HIP_CHECK(hipGetLastError());
  return WN_OK;
}
