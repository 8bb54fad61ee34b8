// Row samplers shared by the sampling kernels (wn_sample.hip) and the generation head kernel (wn_gen.hip): one wave per row.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>
#include "wn_kernels.h"
#include "wn_catrow.h"

// ------------------------------------------------------------------------------------------
// wave-per-row helpers (wn_wave_max / wn_wave_sum: wn_catrow.h)
// inclusive prefix sum over the lanes: shifts by 1, 2, 4, 8 inside the rows of 16 (lanes without a source add zero), then
// the last lane of rows 0 / 2 into rows 1 / 3 and lane 31 into the upper half
#define WN_DPP_Z(v, ctrl, rmask) __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), ctrl, rmask, 0xf, false))
__device__ __forceinline__ float wn_wave_scan_incl(float v) {
  v += WN_DPP_Z(v, 0x111, 0xf);                     // row_shr:1
  v += WN_DPP_Z(v, 0x112, 0xf);                     // row_shr:2
  v += WN_DPP_Z(v, 0x114, 0xf);                     // row_shr:4
  v += WN_DPP_Z(v, 0x118, 0xf);                     // row_shr:8
  v += WN_DPP_Z(v, 0x142, 0xa);                     // row_bcast:15 into rows 1, 3
  v += WN_DPP_Z(v, 0x143, 0xc);                     // row_bcast:31 into rows 2, 3
  return v;
}

// Philox4x32-10 (Salmon et al. 2011), counter = (row, offset), key = seed
__device__ __forceinline__ void wn_philox(uint64_t ctr_lo, uint64_t ctr_hi, uint64_t key, uint32_t out[4]) {
  uint32_t c0 = (uint32_t)ctr_lo, c1 = (uint32_t)(ctr_lo >> 32), c2 = (uint32_t)ctr_hi, c3 = (uint32_t)(ctr_hi >> 32);
  uint32_t k0 = (uint32_t)key, k1 = (uint32_t)(key >> 32);
#pragma unroll
  for (int i = 0; i < 10; ++i) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c1 = (uint32_t)p1; c3 = (uint32_t)p0; c0 = n0; c2 = n2;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}
__device__ __forceinline__ float wn_u01(uint32_t r) {   // (0,1), 24-bit
  return ((float)(r >> 8) + 0.5f) * (1.0f / 16777216.0f);
}

// inverse-CDF categorical draw from the (unnormalised) probabilities p[0..C) of one row per wave
// (p may live in global memory or in LDS); every lane returns the drawn class
template <typename P>
__device__ __forceinline__ int wn_draw_cat_row(P p, int C, int lane, int64_t row, uint64_t seed, uint64_t offset) {
  const int per = (C + 63) / 64;               // contiguous chunk per lane
  const int j0 = lane * per;
  float loc = 0.f;
  for (int j = j0; j < min(C, j0 + per); ++j) loc += fmaxf(p[j], 0.f);
  const float incl = wn_wave_scan_incl(loc);   // inclusive scan over lanes
  const float total = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, incl), 63));
  uint32_t r[4];
  wn_philox((uint64_t)row, offset, seed, r);
  const float target = wn_u01(r[0]) * total;
  const unsigned long long hit = __ballot(incl > target);
  const int sel_lane = hit ? __builtin_ctzll(hit) : 63;
  int result = C - 1;
  if (lane == sel_lane) {
    float run = incl - loc;
    result = min(C, j0 + per) - 1;
    for (int j = j0; j < min(C, j0 + per); ++j) {
      run += fmaxf(p[j], 0.f);
      if (run > target) { result = j; break; }
    }
  }
  return __shfl(result, sel_lane);
}


// ------------------------------------------------------------------------------------------
// Sampling controls: temperature T and top-k.  on() false = the draw without controls, which every
// call site reaches by the code it ran before the controls existed (wave-uniform branch or a second instantiation).
// (struct WnSampleCtl: wn_kernels.h)

// The tempered / truncated law of a categorical row, as a view of the normalised probability row p[0..C) the wave holds
// (global memory or LDS): element j reads as  keep(j) ? (p[j] / p_max)^(1/T) : 0.  The largest term is exactly 1, so no T
// underflows the total.  wn_draw_cat_row takes the view in place of the row; the sliding window (stored softmax row), the
// queued samplers (softmax row in LDS) and sample_waveform build it with wn_cat_ctl_view from the same values, so they
// pick the same class for the same uniform number.
// keep(j): rank by (probability descending, class index ascending), first top_k.  Probabilities are non-negative, so
// their bit patterns order as unsigned integers: key > thr, or key == thr and j <= idx_cut.
template <typename P>
struct WnCatCtlView {
  P p;
  float pmax, inv_T;
  uint32_t thr;
  int idx_cut;
  __device__ __forceinline__ static uint32_t key(float v) { return v > 0.f ? __builtin_bit_cast(uint32_t, v) : 0u; }
  __device__ __forceinline__ float operator[](int j) const {
    const float v = p[j];
    const uint32_t k = key(v);
    if (!(k > thr || (k == thr && j <= idx_cut))) return 0.f;
    return term(v);
  }
  // the term of a kept class whose probability is v
  __device__ __forceinline__ float term(float v) const {
    const float r = fmaxf(v, 0.f) / pmax;
    return inv_T == 1.0f ? r : expf(inv_T * logf(r));      // r = 1 -> exactly 1; r = 0 -> 0
  }
};
// Builds the view: one wave per row, all 64 lanes active, every lane gets the same view.  The k-th largest key by
// bisection on the key (at most 31 rounds of count(key >= mid), a ballot + popcount per register slot for C <= 256, a
// strided loop over the row beyond), then the ties at the threshold by class index with ballot prefix counts.
// TOPP false: built without the top-p search (ctl.top_p must be off) -- the head kernel of queued generation, whose
// register allocation the search would disturb on every step, the default one included.
template <bool TOPP = true, typename P>
__device__ __forceinline__ WnCatCtlView<P> wn_cat_ctl_view(P p, int C, int lane, WnSampleCtl ctl) {
  using V = WnCatCtlView<P>;
  V w{p, 1.0f, ctl.inv_T, 0u, 0x7fffffff};
  const bool regs = C <= 256;
  uint32_t kr[4] = {0u, 0u, 0u, 0u};
  float m = 0.f;
  if (regs) {
#pragma unroll
    for (int s = 0; s < 4; ++s)
      if (lane + 64 * s < C) { const float v = p[lane + 64 * s]; kr[s] = V::key(v); m = fmaxf(m, v); }
  } else {
    for (int j = lane; j < C; j += 64) m = fmaxf(m, p[j]);
  }
  m = wn_wave_max(m);
  w.pmax = m > 0.f ? m : 1.0f;                       // an all-zero row stays all zero (the draw then returns class C - 1)
  const bool topk = ctl.top_k > 0 && ctl.top_k < C, topp = TOPP && ctl.top_p > 0.f && ctl.top_p < 1.0f;
  if (!topk && !topp) return w;
  // count of classes whose key is >= t (t > 0 excludes the empty register slots, key 0) / == t, wave-uniform
  auto count_ge = [&](uint32_t t) {
    int c = 0;
    if (regs) {
#pragma unroll
      for (int s = 0; s < 4; ++s) c += __popcll(__ballot(kr[s] >= t));
    } else {
      for (int j0 = 0; j0 < C; j0 += 64) c += __popcll(__ballot(j0 + lane < C && V::key(p[min(j0 + lane, C - 1)]) >= t));
    }
    return c;
  };
  int need = 0;
  // slot s = classes 64 s .. 64 s + 63 in lane order; returns true once the need-th tie is found
  auto take = [&](int s, bool tie) {
    const unsigned long long mask = __ballot(tie);
    const int cnt = __popcll(mask);
    if (need > cnt) { need -= cnt; return false; }
    const unsigned long long hit = __ballot(tie && __popcll(mask & ((2ull << lane) - 1ull)) == need);
    w.idx_cut = 64 * s + __builtin_ctzll(hit);
    return true;
  };
  // idx_cut: of the classes up to index cap whose key is t, the need-th by class index
  auto cut_ties = [&](uint32_t t, int cap) {
    if (regs) {
      bool done = false;
#pragma unroll
      for (int s = 0; s < 4; ++s)
        if (!done) done = take(s, lane + 64 * s < C && kr[s] == t && lane + 64 * s <= cap);
    } else {
      for (int s = 0; 64 * s < C; ++s)
        if (take(s, 64 * s + lane < C && V::key(p[min(64 * s + lane, C - 1)]) == t && 64 * s + lane <= cap)) break;
    }
  };
  if (topk) {
    // largest thr with count(key >= thr) >= top_k: lo always satisfies it (count(key >= 0) = C > top_k), hi never does
    uint32_t lo = 0u, hi = V::key(m) + 1u;
    while (hi - lo > 1u) {
      const uint32_t mid = lo + ((hi - lo) >> 1);
      if (count_ge(mid) >= ctl.top_k) lo = mid; else hi = mid;
    }
    need = ctl.top_k - count_ge(lo + 1u);                 // of the ties at thr, the first `need` by class index
    cut_ties(lo, 0x7fffffff);
    w.thr = lo;
  }
  if constexpr (!TOPP) return w;
  if (!topp) return w;
  // top-p on the set K that top-k kept (wk; all classes when top-k is off): with q_j = wk[j] and Q = sum q, the shortest
  // prefix of the same ranking whose sum q reaches top_p Q.  mass(t) = sum of q over key >= t, every lane's terms in the
  // order lane, lane + 64, ... and then wn_wave_sum, whatever t: each addition is monotone in its operands, so mass is
  // monotone in t also as rounded, and where the partial sums are exactly representable the decisions are exact.
  const V wk = w;
  float qr[4] = {0.f, 0.f, 0.f, 0.f};
  if (regs) {
#pragma unroll
    for (int s = 0; s < 4; ++s)
      if (lane + 64 * s < C) qr[s] = wk[lane + 64 * s];
  }
  auto mass_ge = [&](uint32_t t) {
    float a = 0.f;
    if (regs) {
#pragma unroll
      for (int s = 0; s < 4; ++s) a += kr[s] >= t ? qr[s] : 0.f;
    } else {
      for (int j = lane; j < C; j += 64) a += V::key(p[j]) >= t ? wk[j] : 0.f;
    }
    return wn_wave_sum(a);
  };
  const float Q = mass_ge(wk.thr);
  if (!(Q > 0.f)) return w;                               // all-zero row
  const float target = ctl.top_p * Q;
  // largest thr with mass(key >= thr) >= target: lo = K's own threshold always satisfies it (target <= Q), hi never does
  // (nothing lies above the largest key and target > 0).  At most 31 rounds, a wave sum each.
  uint32_t lo = wk.thr, hi = V::key(m) + 1u;
  while (hi - lo > 1u) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (mass_ge(mid) >= target) lo = mid; else hi = mid;
  }
  // mass(lo + 1) < target <= mass(lo): classes of K tie at lo, each with the term q_thr > 0; the smallest n with
  // above + n q_thr >= target of them are kept, by class index
  const float above = mass_ge(lo + 1u), q_thr = wk.term(__builtin_bit_cast(float, lo));
  int n = (int)fminf(ceilf((target - above) / q_thr), 1024.f);
  while (n > 1 && above + (float)(n - 1) * q_thr >= target) --n;
  while (n < 1 || (n < C && above + (float)n * q_thr < target)) ++n;
  // (n beyond the number of ties -- the rounding of mass(lo) against above + n q_thr -- keeps them all)
  need = n;
  w.thr = lo;
  w.idx_cut = lo == wk.thr ? wk.idx_cut : 0x7fffffff;     // at K's own threshold only K's ties count
  cut_ties(lo, w.idx_cut);
  return w;
}


// Categorical head, deterministic (src/model.py:393-421 with deterministic sampling): softmax -> arg max -> sample value.
// The probabilities are those wn_softmax_kernel stores and the arg max is that of wn_sample_det_cat_kernel (the same row
// and the same butterfly of wn_catrow.h), so the result is the same sample.  Every lane returns it.
__device__ __forceinline__ float wn_cat_det_row(const float* l, int C, int lane, float inv_lv) {
  float best = -INFINITY;
  int bi = 0x7fffffff;
  WnSoftmaxLoop(l, C, lane).each([&](int j, float v) {
    if (v > best) { best = v; bi = j; }            // strictly greater keeps the first maximum
  });
  wn_wave_argmax_first(best, bi);
  return (float)bi * inv_lv - 1.0f;
}

// Categorical head, stochastic draw straight from the logits: the probabilities are those wn_softmax_kernel stores, kept
// in the LDS row q[0..C) instead of a (rows, C) tensor in HBM, so the drawn class is the one
// sample_waveform(softmax(logits)) draws.  Every lane returns the sample value.
// CTL: the draw under the sampling controls, from the view of the same LDS row (TOPP: wn_cat_ctl_view).
template <bool CTL = false, bool TOPP = CTL>
__device__ __forceinline__ float wn_cat_rand_row(const float* l, int C, int lane, float* q, int64_t row, uint64_t seed,
                                                 uint64_t offset, float inv_lv, WnSampleCtl ctl = WN_SAMPLE_CTL_OFF) {
  auto keep = [&](int j, float v) { q[j] = v; };
  if (C <= 256) {                                    // one read of the row, one exp per class
    float v[4];
    wn_cat_load4(l, C, lane, v);
    WnSoftmaxRegs(v, C, lane).each(keep);
  } else {
    WnSoftmaxLoop(l, C, lane).each(keep);
  }
  __builtin_amdgcn_wave_barrier();
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  int result;
  if constexpr (CTL) result = wn_draw_cat_row(wn_cat_ctl_view<TOPP>((const float*)q, C, lane, ctl), C, lane, row, seed, offset);
  else result = wn_draw_cat_row((const float*)q, C, lane, row, seed, offset);
  return (float)result * inv_lv - 1.0f;
}

// Mixture heads (logistic / gaussian), one row per thread: src/model.py:423-503.  p = [M logit weights | M means | M log scales].
__device__ __forceinline__ float wn_mix_det_row(const float* p, int M) {
  int bi = 0;
  float best = p[0];
  for (int k = 1; k < M; ++k) if (p[k] > best) { best = p[k]; bi = k; }
  return fminf(fmaxf(p[M + bi], -1.0f), 1.0f);
}
// CTL: at temperature T the row reads [w / T | mu | s + ln T] -- component pick sharpened, component scale times T; the
// Philox words keep their use and the clip is unchanged.
template <bool CTL = false>
__device__ __forceinline__ float wn_mix_rand_row(const float* p, int M, int kind, int64_t row, uint64_t seed, uint64_t offset,
                                                 WnSampleCtl ctl = WN_SAMPLE_CTL_OFF) {
  uint32_t r[4];
  wn_philox((uint64_t)row, offset, seed, r);
  auto w = [&](int k) { if constexpr (CTL) return p[k] * ctl.inv_T; else return p[k]; };
  float wm = -INFINITY;
  for (int k = 0; k < M; ++k) wm = fmaxf(wm, w(k));
  float wz = 0.f;
  for (int k = 0; k < M; ++k) wz += expf(w(k) - wm);
  const float target = wn_u01(r[0]) * wz;
  int sel = M - 1;
  float run = 0.f;
  for (int k = 0; k < M; ++k) { run += expf(w(k) - wm); if (run > target) { sel = k; break; } }
  const float mu = p[M + sel];
  float sc = expf(p[2 * M + sel]);
  if constexpr (CTL) sc *= ctl.T;                  // e^(s + ln T)
  float v;
  if (kind == 1) {                       // logistic: mu + s (ln z - ln(1-z))     src/model.py:463-483
    const float zz = wn_u01(r[1]);
    v = mu + sc * (logf(zz) - logf(1.0f - zz));
  } else {                               // gaussian: mu + s n                   src/model.py:423-443
    const float u1 = wn_u01(r[1]), u2 = wn_u01(r[2]);
    v = mu + sc * sqrtf(-2.0f * logf(u1)) * cosf(6.283185307179586f * u2);
  }
  return fminf(fmaxf(v, -1.0f), 1.0f);
}


// ------------------------------------------------------------------------------------------
// Per-row controls (struct WnSampleRow, wn_kernels.h): row r of a *_rows kernel draws with tab[r] --
// its controls, its Philox key, its counter row.  The categorical helpers make, per row, exactly the call the scalar
// kernels make for a whole launch (<false> for a row whose controls are off, <true> otherwise); the mixture helper runs
// <true> for every row, which at T = 1 has the bits of <false>.  So row r has the bits of the scalar launch with tab[r]'s
// controls.

// The record of a wave's row in scalar registers: every lane loads the same 32 bytes (an ordinary vector load), the first
// lane's copy is broadcast, and the branches on it below are wave-uniform for the compiler as well.
__device__ __forceinline__ WnSampleRow wn_sample_row_uniform(const WnSampleRow* tab, int64_t row) {
  const uint4* src = reinterpret_cast<const uint4*>(tab + row);
  const uint4 a = src[0], b = src[1];
  auto u = [](uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); };
  WnSampleRow r;
  r.T = __builtin_bit_cast(float, u(a.x)); r.inv_T = __builtin_bit_cast(float, u(a.y));
  r.top_k = (int32_t)u(a.z); r.top_p = __builtin_bit_cast(float, u(a.w));
  r.seed = (uint64_t)u(b.x) | ((uint64_t)u(b.y) << 32);
  r.stream = (uint64_t)u(b.z) | ((uint64_t)u(b.w) << 32);
  return r;
}
// The row's own clock: beside a table a *_rows kernel may take `origin`, one uint64_t per row of the
// call, and row r then draws with the counter word offset - origin[r] (unsigned 64-bit: beyond offset the word wraps
// modulo 2^64).  Null = every origin 0 = the counter word of before.  Wave-uniform form for the categorical kernels, read
// as the record is read above; the mixture kernels load theirs per thread, beside tab[row].
__device__ __forceinline__ uint64_t wn_sample_clock_uniform(const uint64_t* origin, int64_t row, uint64_t offset) {
  if (!origin) return offset;
  const uint2 o = *reinterpret_cast<const uint2*>(origin + row);
  auto u = [](uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); };
  return offset - ((uint64_t)u(o.x) | ((uint64_t)u(o.y) << 32));
}
// categorical draw from a stored probability row (wn_sample_rand_cat_kernel's two forms)
__device__ __forceinline__ int wn_draw_cat_row_tab(const float* p, int C, int lane, const WnSampleRow& r, uint64_t offset) {
  if (r.ctl().on()) return wn_draw_cat_row(wn_cat_ctl_view(p, C, lane, r.ctl()), C, lane, (int64_t)r.stream, r.seed, offset);
  return wn_draw_cat_row(p, C, lane, (int64_t)r.stream, r.seed, offset);
}
// categorical draw from the logits (wn_cat_rand_row's forms; TOPP false: the head kernel, no row has top_p on)
template <bool TOPP = true>
__device__ __forceinline__ float wn_cat_rand_row_tab(const float* l, int C, int lane, float* q, const WnSampleRow& r,
                                                     uint64_t offset, float inv_lv) {
  if (r.ctl().on()) return wn_cat_rand_row<true, TOPP>(l, C, lane, q, (int64_t)r.stream, r.seed, offset, inv_lv, r.ctl());
  return wn_cat_rand_row(l, C, lane, q, (int64_t)r.stream, r.seed, offset, inv_lv);
}
// mixture draw, one row per thread: lanes differ in their records, in data only -- every lane runs the <true> form.  For a
// row at T = 1 that form has the bits of the <false> form: its only extra operations are w * inv_T and e^s * T, and a
// product with 1.0f is exact for every finite and infinite fp32 value, denormals included (fp32 denormals are not flushed
// on gfx950; the product and the subtraction behind it are separate source expressions, so -ffp-contract=on fuses
// nothing, and a fused (w * 1 - wm) would round like (w - wm) anyway).  One instruction stream for all lanes: a mixed
// batch costs what the uniform one costs (a per-lane branch between the two forms ran both, measured +2 us a step).
__device__ __forceinline__ float wn_mix_rand_row_tab(const float* p, int M, int kind, const WnSampleRow* tab, int64_t row,
                                                     uint64_t offset, const uint64_t* origin = nullptr) {
  const WnSampleRow r = tab[row];
  if (origin) offset -= origin[row];                 // (a kernel argument: uniform)
  return wn_mix_rand_row<true>(p, M, kind, (int64_t)r.stream, r.seed, offset, r.ctl());
}
