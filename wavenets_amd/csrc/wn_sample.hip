// Sampling kernels of the WaveNet hot path (gfx950): sample_waveform, src/model.py:393-503.  The row functions are those
// of wn_sample.h, shared with the generation head kernel (wn_gen.hip).
// (queued generation: a launcher given an emit target also puts the sample into the output rows and the network's input
// ring, wn_emit_sample; categorical rows with an emit target are LOGITS rows -- softmax, sampler and emit in one launch)
#include "wn_kernels.h"
#include "wn_sample.h"

__global__ __launch_bounds__(256) void wn_sample_det_cat_kernel(const float* pred, int64_t rows, int C,
                                                                float inv, float* out) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const float* p = pred + row * C;
  float best = -INFINITY;
  int bi = 0x7fffffff;
  for (int j = lane; j < C; j += 64) {
    const float v = p[j];
    if (v > best) { best = v; bi = j; }          // strictly greater keeps the first maximum
  }
  wn_wave_argmax_first(best, bi);
  if (lane == 0) out[row] = (float)bi * inv - 1.0f;
}
// softmax -> arg max -> sample value -> output row and next network input from the logits: wn_cat_det_row gives the
// sample wn_softmax_kernel followed by the kernel above gives
__global__ __launch_bounds__(256) void wn_sample_det_cat_logits_kernel(const float* logits, int64_t rows, int C, float inv_lv,
                                                                       float* out, WnEmit em) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const float v = wn_cat_det_row(logits + row * C, C, lane, inv_lv);
  if (lane == 0) {
    if (out) out[row] = v;
    wn_emit_sample(em, row, v);
  }
}
__global__ void wn_sample_det_mix_kernel(const float* pred, int64_t rows, int M, float* out, WnEmit em) {
  const int64_t row = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= rows) return;
  const float v = wn_mix_det_row(pred + row * 3 * M, M);
  out[row] = v;
  wn_emit_sample(em, row, v);
}
int wn_launch_sample_det(const float* pred, int64_t rows, int C, int M, int bits, float* out, hipStream_t s, WnEmit em) {
  if (rows <= 0) return WN_OK;
  const float inv_lv = 1.0f / (float)(1 << (bits - 1));
  if (M <= 0 && em.out) {
    hipLaunchKernelGGL(wn_sample_det_cat_logits_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, s,
                       pred, rows, C, inv_lv, out, em);
  } else if (M <= 0) {
    hipLaunchKernelGGL(wn_sample_det_cat_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, s,
                       pred, rows, C, inv_lv, out);
  } else {
    hipLaunchKernelGGL(wn_sample_det_mix_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0,
                       s, pred, rows, M, out, em);
  }
  WN_HIP_CHECK(hipGetLastError());
  return WN_OK;
}

// CTL (here and below): the draw under the sampling controls, from the tempered / truncated view of the same row.  The
// host picks <false> when the controls are off: the instruction stream of before the controls existed.
template <bool CTL>
__global__ __launch_bounds__(256) void wn_sample_rand_cat_kernel(const float* pred, int64_t rows, int C,
                                                                 float inv, uint64_t seed, uint64_t offset,
                                                                 float* out, WnSampleCtl ctl) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  int result;
  if constexpr (CTL) result = wn_draw_cat_row(wn_cat_ctl_view(pred + row * C, C, lane, ctl), C, lane, row, seed, offset);
  else result = wn_draw_cat_row(pred + row * C, C, lane, row, seed, offset);
  if (lane == 0) out[row] = (float)result * inv - 1.0f;
}

// The same draw straight from the logits (training step with a compiled sample metric, src/model.py:338; queued
// generation): wn_cat_rand_row keeps the probabilities wn_softmax_kernel would store in LDS instead of a (rows, C) tensor
// in HBM, so the drawn class is the one sample_waveform(softmax(logits)) draws.
#define WN_SAMPLE_FUSED_MAXC 1024
template <bool CTL>
__global__ __launch_bounds__(256) void wn_sample_rand_cat_logits_kernel(const float* logits, int64_t rows, int C,
                                                                        float inv_lv, uint64_t seed, uint64_t offset,
                                                                        float* out, WnEmit em, WnSampleCtl ctl) {
  __shared__ float q[4][WN_SAMPLE_FUSED_MAXC];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int64_t row = (int64_t)blockIdx.x * 4 + w;
  if (row >= rows) return;
  const float v = wn_cat_rand_row<CTL>(logits + row * C, C, lane, q[w], row, seed, offset, inv_lv, ctl);
  if (lane == 0) {
    out[row] = v;
    wn_emit_sample(em, row, v);
  }
}
// Per-row controls: row r draws with tab[r] -- its controls, key and counter row -- in the forms
// wn_draw_cat_row_tab / wn_cat_rand_row_tab / wn_mix_rand_row_tab pick per row; the kernels above stay as they are.
// LOGITS false: from a stored probability row (wn_sample_rand_cat_kernel's twin); true: from the logits, with the emit
// (wn_sample_rand_cat_logits_kernel's twin).  Templates first used at the END of this file (wn_launch_sample_rand_rows):
// instantiations are emitted in the order of first use, so the twins land behind the kernels of before in the code object.
template <bool LOGITS>
__global__ __launch_bounds__(256) void wn_sample_rand_cat_rows_kernel(const float* pred, int64_t rows, int C, float inv,
                                                                      uint64_t offset, float* out, WnEmit em,
                                                                      const WnSampleRow* tab, const uint64_t* origin) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int64_t row = (int64_t)blockIdx.x * 4 + w;
  if (row >= rows) return;
  const WnSampleRow r = wn_sample_row_uniform(tab, row);
  offset = wn_sample_clock_uniform(origin, row, offset);     // the row's own clock
  if constexpr (LOGITS) {
    __shared__ float q[4][WN_SAMPLE_FUSED_MAXC];
    const float v = wn_cat_rand_row_tab(pred + row * C, C, lane, q[w], r, offset, inv);
    if (lane == 0) {
      out[row] = v;
      wn_emit_sample(em, row, v);
    }
  } else {
    const int result = wn_draw_cat_row_tab(pred + row * C, C, lane, r, offset);
    if (lane == 0) out[row] = (float)result * inv - 1.0f;
  }
}
// (defined at the end of the file)
static void wn_launch_sample_rand_rows(const float* pred, int64_t rows, int C, int M, int bits, int kind, uint64_t offset,
                                       float* out, hipStream_t s, WnEmit em, const WnSampleRow* tab, bool logits,
                                       const uint64_t* origin);
int wn_sample_from_logits_supported(int C) { return C <= WN_SAMPLE_FUSED_MAXC ? 1 : 0; }
int wn_sample_top_k_max_classes() { return WN_SAMPLE_FUSED_MAXC; }
int wn_launch_sample_rand_cat_logits(const float* logits, int64_t rows, int C, int bits, uint64_t seed, uint64_t offset,
                                     float* out, hipStream_t s, WnSampleCtl ctl, WnEmit em, const WnSampleRow* tab,
                                     const uint64_t* origin) {
  if (rows <= 0) return WN_OK;
  if (C > WN_SAMPLE_FUSED_MAXC) { wn_set_error("sample from logits: %d classes > %d", C, WN_SAMPLE_FUSED_MAXC); return WN_E_UNSUPPORTED; }
  if (tab) {
    wn_launch_sample_rand_rows(logits, rows, C, 0, bits, 0, offset, out, s, em, tab, true, origin);
    WN_HIP_CHECK(hipGetLastError());
    return WN_OK;
  }
  const auto kernel = ctl.on() ? wn_sample_rand_cat_logits_kernel<true> : wn_sample_rand_cat_logits_kernel<false>;
  hipLaunchKernelGGL(kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, s, logits, rows, C,
                     1.0f / (float)(1 << (bits - 1)), seed, offset, out, em, ctl);
  WN_HIP_CHECK(hipGetLastError());
  return WN_OK;
}
template <bool CTL>
__global__ void wn_sample_rand_mix_kernel(const float* pred, int64_t rows, int M, int kind, uint64_t seed,
                                          uint64_t offset, float* out, WnEmit em, WnSampleCtl ctl) {
  const int64_t row = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= rows) return;
  const float vc = wn_mix_rand_row<CTL>(pred + row * 3 * M, M, kind, row, seed, offset, ctl);
  out[row] = vc;
  wn_emit_sample(em, row, vc);
}
template <bool EMIT>
__global__ void wn_sample_rand_mix_rows_kernel(const float* pred, int64_t rows, int M, int kind, uint64_t offset, float* out,
                                              WnEmit em, const WnSampleRow* tab, const uint64_t* origin) {
  const int64_t row = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= rows) return;
  const float vc = wn_mix_rand_row_tab(pred + row * 3 * M, M, kind, tab, row, offset, origin);
  out[row] = vc;
  if constexpr (EMIT) wn_emit_sample(em, row, vc);
}
int wn_launch_sample_rand(const float* pred, int64_t rows, int C, int M, int bits, int kind, uint64_t seed, uint64_t offset,
                          float* out, hipStream_t s, WnSampleCtl ctl, WnEmit em, const WnSampleRow* tab, const uint64_t* origin) {
  if (rows <= 0) return WN_OK;
  if (M > 0 && (ctl.top_k > 0 || ctl.top_p > 0.f)) {
    wn_set_error("sample_rand: top_k and top_p apply to the categorical head only");
    return WN_E_INVALID;
  }
  if (M <= 0 && (ctl.top_k > 0 || ctl.top_p > 0.f) && C > WN_SAMPLE_FUSED_MAXC) {
    wn_set_error("sample_rand: top_k / top_p over %d classes > %d", C, WN_SAMPLE_FUSED_MAXC);
    return WN_E_UNSUPPORTED;
  }
  if (M <= 0 && em.out) return wn_launch_sample_rand_cat_logits(pred, rows, C, bits, seed, offset, out, s, ctl, em, tab, origin);
  if (tab) {
    wn_launch_sample_rand_rows(pred, rows, C, M, bits, kind, offset, out, s, em, tab, false, origin);
  } else if (M <= 0) {
    const auto kernel = ctl.on() ? wn_sample_rand_cat_kernel<true> : wn_sample_rand_cat_kernel<false>;
    hipLaunchKernelGGL(kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, s,
                       pred, rows, C, 1.0f / (float)(1 << (bits - 1)), seed, offset, out, ctl);
  } else {
    const auto kernel = ctl.on() ? wn_sample_rand_mix_kernel<true> : wn_sample_rand_mix_kernel<false>;
    hipLaunchKernelGGL(kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0,
                       s, pred, rows, M, kind, seed, offset, out, em, ctl);
  }
  WN_HIP_CHECK(hipGetLastError());
  return WN_OK;
}

static void wn_launch_sample_rand_rows(const float* pred, int64_t rows, int C, int M, int bits, int kind, uint64_t offset,
                                       float* out, hipStream_t s, WnEmit em, const WnSampleRow* tab, bool logits,
                                       const uint64_t* origin) {
  const float inv = 1.0f / (float)(1 << (bits - 1));
  if (M <= 0) {
    const auto kernel = logits ? wn_sample_rand_cat_rows_kernel<true> : wn_sample_rand_cat_rows_kernel<false>;
    hipLaunchKernelGGL(kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, s, pred, rows, C, inv, offset, out, em, tab, origin);
  } else {
    const auto kernel = em.out ? wn_sample_rand_mix_rows_kernel<true> : wn_sample_rand_mix_rows_kernel<false>;
    hipLaunchKernelGGL(kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, s, pred, rows, M, kind, offset, out, em, tab, origin);
  }
}
