// The categorical row, written once: softmax of one row per wave in its two storage forms, Keras clipped sparse cross
// entropy and its gradient, the first-maximum arg max, and the emit of a generated sample.  Every kernel that promises
// "the same bits as ..." for a categorical row (loss kernels, softmax, samplers, generation head, the fused loss epilogue of
// wn_gemm16s.hip) evaluates the expressions below -- the build uses -ffp-contract=on, so an expression rounds the same way
// wherever it is inlined.  
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>
#include "wn_kernels.h"

// ------------------------------------------------------------------------------------------
// wave-per-row reductions
// Over the 64 lanes on the DPP cross-lane operands of the VALU (no LDS round trips: __shfl_xor is a ds_bpermute
// with its own address and wait, six in a row per reduction): quad butterflies, then the two mirror permutations leave
// every lane with the sum / max of its row of 16; the four row results are read as scalars.  Every lane returns the result.
// (All 64 lanes must be active, as with the shuffles.)
#define WN_DPP_F(v, ctrl) __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, v), __builtin_bit_cast(int, v), ctrl, 0xf, 0xf, false))
__device__ __forceinline__ float wn_wave_max(float v) {
  v = fmaxf(v, WN_DPP_F(v, 0xB1));                  // quad_perm [1, 0, 3, 2]
  v = fmaxf(v, WN_DPP_F(v, 0x4E));                  // quad_perm [2, 3, 0, 1]
  v = fmaxf(v, WN_DPP_F(v, 0x141));                 // row_half_mirror
  v = fmaxf(v, WN_DPP_F(v, 0x140));                 // row_mirror
  const int b = __builtin_bit_cast(int, v);
  const float r0 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(b, 0)), r1 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(b, 16));
  const float r2 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(b, 32)), r3 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(b, 48));
  return fmaxf(fmaxf(r0, r1), fmaxf(r2, r3));
}
__device__ __forceinline__ float wn_wave_sum(float v) {
  v += WN_DPP_F(v, 0xB1);
  v += WN_DPP_F(v, 0x4E);
  v += WN_DPP_F(v, 0x141);
  v += WN_DPP_F(v, 0x140);
  const int b = __builtin_bit_cast(int, v);
  const float r0 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(b, 0)), r1 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(b, 16));
  const float r2 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(b, 32)), r3 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(b, 48));
  return (r0 + r1) + (r2 + r3);
}
// arg max over the lanes' (best, bi) candidates, the FIRST maximum winning: among equal values the smaller class index
// (a lane's own candidate must already be its first maximum: take v only when v > best).  Every lane gets the result.
__device__ __forceinline__ void wn_wave_argmax_first(float& best, int& bi) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(best, o);
    const int oi = __shfl_xor(bi, o);
    if (ov > best || (ov == best && oi < bi)) { best = ov; bi = oi; }
  }
}

// ------------------------------------------------------------------------------------------
// Row softmax, one wave per row: m = max_j l_j, z = sum_j expf(l_j - m), q_j = expf(l_j - m) * (1 / z).  A lane owns the
// classes lane, lane + 64, ... and sums them in that order; m and z come from wn_wave_max / wn_wave_sum.  Two storage
// forms give the same bits behind one interface: m, inv, each(f) visiting f(j, q_j) in the lane's order, prob(t) = q_t
// for a wave-uniform class t.
// What differs on purpose: prob(t) of the register form comes from the lane that holds exp(l_t - m) (a __shfl), that of
// the loop form from a second read of l[t]; both evaluate expf(l_t - m) * inv.

// C <= 256: four register slots per lane, slot k = class lane + 64 k.  Built from logits that are already loaded (-inf
// in the slots beyond C: wn_cat_load4), so that a persistent kernel can have the next row in flight.
__device__ __forceinline__ void wn_cat_load4(const float* l, int C, int lane, float (&v)[4]) {
#pragma unroll
  for (int k = 0; k < 4; ++k) v[k] = lane + 64 * k < C ? l[lane + 64 * k] : -INFINITY;
}
struct WnSoftmaxRegs {
  float e[4];                                        // exp(l - m); 0 in the slots beyond C
  float m, inv;
  int C, lane;
  __device__ __forceinline__ WnSoftmaxRegs(const float (&v)[4], int C_, int lane_) : C(C_), lane(lane_) {
    m = -INFINITY;
#pragma unroll
    for (int k = 0; k < 4; ++k) m = fmaxf(m, v[k]);
    m = wn_wave_max(m);
    float z = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      e[k] = lane + 64 * k < C ? expf(v[k] - m) : 0.f;
      if (lane + 64 * k < C) z += e[k];
    }
    z = wn_wave_sum(z);
    inv = 1.0f / z;
  }
  template <typename F>
  __device__ __forceinline__ void each(F f) const {
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (lane + 64 * k < C) f(lane + 64 * k, e[k] * inv);
  }
  __device__ __forceinline__ float prob(int t) const {
    const int tk = t >> 6;                            // wave-uniform: the lane t & 63 holds e[tk] = exp(l[t] - m)
    float et = e[0];
#pragma unroll
    for (int k = 1; k < 4; ++k) et = tk == k ? e[k] : et;
    return __shfl(et, t & 63) * inv;
  }
};
// any C: the row is read again from memory on every pass
struct WnSoftmaxLoop {
  const float* l;
  float m, inv;
  int C, lane;
  __device__ __forceinline__ WnSoftmaxLoop(const float* l_, int C_, int lane_) : l(l_), C(C_), lane(lane_) {
    m = -INFINITY;
    for (int j = lane; j < C; j += 64) m = fmaxf(m, l[j]);
    m = wn_wave_max(m);
    float z = 0.f;
    for (int j = lane; j < C; j += 64) z += expf(l[j] - m);
    z = wn_wave_sum(z);
    inv = 1.0f / z;
  }
  template <typename F>
  __device__ __forceinline__ void each(F f) const {
    for (int j = lane; j < C; j += 64) f(j, expf(l[j] - m) * inv);
  }
  __device__ __forceinline__ float prob(int t) const { return expf(l[t] - m) * inv; }
};

// ------------------------------------------------------------------------------------------
// Keras sparse_categorical_crossentropy(target, q), from_logits=False (src/model.py:505-551):
//   p = clip(q, eps, 1 - eps); loss = -(log p_t - log S), S = sum_j p_j
// and its gradient w.r.t. the logits behind q = softmax (the clip passes gradient where eps <= q <= 1 - eps):
//   A = sum_j q_j [eps <= q_j <= 1 - eps];  dot = A / S - c_t q_t / p_t  (= sum_j g_j q_j)
//   dL/dl_j = gscale q_j (c_j / S - [j = t] c_t / p_t - dot)
// The per-element pieces are scalar functions, so that a kernel with another register layout (the MFMA accumulators of
// the fused epilogue in wn_gemm16s.hip) sums S and A its own way and still rounds every term as the row kernels do.
// That epilogue keeps, on purpose, its own exponentials (exp2 on the scaled argument), its two-lanes-per-row exchange
// and its tile-wise draw; only clip, indicator, row terms and the per-class gradient come from here.
__device__ __forceinline__ float wn_ce_clip(float q) { return fminf(fmaxf(q, WN_KERAS_EPS), 1.0f - WN_KERAS_EPS); }
__device__ __forceinline__ bool wn_ce_inside(float q) { return q >= WN_KERAS_EPS && q <= 1.0f - WN_KERAS_EPS; }
__device__ __forceinline__ int wn_ce_target(int tgt, int C) { return tgt < 0 ? 0 : (tgt >= C ? C - 1 : tgt); }
__device__ __forceinline__ float wn_ce_loss(float pt, float S) { return -(logf(pt) - logf(S)); }
// the terms of a row that every class shares, from S, A and the target's probability
struct WnCeRow {
  float pt, ct, invS, ct_pt, dot;
  __device__ __forceinline__ WnCeRow(float S, float A, float qt) {
    pt = wn_ce_clip(qt);
    ct = wn_ce_inside(qt) ? 1.f : 0.f;
    invS = 1.0f / S;
    ct_pt = ct / pt;                   // (a quotient is rounded where it stands: taking it once changes no bit)
    dot = A * invS - ct * qt / pt;     // sum_j g_j q_j
  }
  __device__ __forceinline__ float grad(float q, bool is_target, float gscale) const {
    const float c = wn_ce_inside(q) ? 1.f : 0.f;
    float g = c * invS;
    if (is_target) g -= ct_pt;
    return gscale * q * (g - dot);
  }
};
// sample_weight of a row (every loss kernel, the mixture one included, takes the factor from here):
// the gradient is that of the unweighted row with gscale * w in gscale's place, the product taken once per row; the stored
// loss is w * l.  w == 0 is a select, not a product: loss +0 and gradient 0 whatever the row holds (inf, NaN), and so nothing
// of the row reaches the max-abs.  Any other w, negative and non-finite included, is a plain product.  w == 1 changes no bit.
__device__ __forceinline__ float wn_w_gscale(float gscale, float w) { return gscale * w; }
__device__ __forceinline__ float wn_w_loss(float w, float l) { return w == 0.f ? 0.f : w * l; }
__device__ __forceinline__ float wn_w_grad(float w, float g) { return w == 0.f ? 0.f : g; }
// Loss and (g != null) gradient of one row held as a softmax row (either form): lane 0 stores the loss, every lane
// stores the gradients of its classes to g[g_off + 0..C) and folds their magnitudes into gmax.
// WEIGHTED: the row's sample_weight w (wave-uniform) enters as above; false is the row without weights, w unused.
template <bool WEIGHTED = false, typename Row>
__device__ __forceinline__ void wn_cat_ce_row(const Row& r, int tgt, float gscale, float* loss, float* g, int64_t g_off,
                                              float& gmax, float w = 1.0f) {
  if constexpr (WEIGHTED) gscale = wn_w_gscale(gscale, w);
  float S = 0.f, A = 0.f;
  r.each([&](int, float q) {
    S += wn_ce_clip(q);
    if (wn_ce_inside(q)) A += q;
  });
  S = wn_wave_sum(S);
  A = wn_wave_sum(A);
  tgt = wn_ce_target(tgt, r.C);
  const float qt = r.prob(tgt);
  const float pt = wn_ce_clip(qt);
  if (r.lane == 0) *loss = WEIGHTED ? wn_w_loss(w, wn_ce_loss(pt, S)) : wn_ce_loss(pt, S);
  if (g) {
    const WnCeRow ce(S, A, qt);
    r.each([&](int j, float q) {
      float gl = ce.grad(q, j == tgt, gscale);
      if constexpr (WEIGHTED) gl = wn_w_grad(w, gl);
      g[g_off + j] = gl;
      gmax = fmaxf(gmax, fabsf(gl));
    });
  }
}

// ------------------------------------------------------------------------------------------
// queued generation: the sample also goes to its place in the output rows and into the network's input ring -- the
// emit step of a generation step rides in the sampler's launch
__device__ __forceinline__ void wn_emit_sample(const WnEmit& e, int64_t row, float v) {
  if (!e.out) return;
  e.out[row * e.length + e.step] = v;
  if (e.xin_slot) e.xin_slot[row] = v;
}
