// Split-precision MFMA arithmetic (gfx950), written once for every fast kernel.  An fp32 operand becomes fp16 hi = fp16(v)
// plus lo = fp16(v - hi), optionally scaled by an exact power of two of its running max-abs, and a product is three
// v_mfma_f32_32x32x16_f16 into an fp32 accumulator, always in the order a_lo*b_hi, a_hi*b_lo, a_hi*b_hi.  This sets the
// accuracy contract of both math modes, and the generation kernels reproduce the training-forward kernels bit for bit
// only because both go through these definitions.  For the generation kernels (wn_gen.hip, wn_gen128.hip) also the quads
// of a D-layout accumulator and the products over hi|lo operands in LDS (mac_lds).  Also here: the 16-byte global loads,
// LDS-DMA by inline assembly and the store of a 32 x 32 accumulator tile as whole row segments from a scalar base
// (store_tile), or of a row of such tiles as buffer stores on a descriptor that ends behind the last valid row
// (wn_store_tile: block forward and backward pair kernels).
#pragma once
#include <hip/hip_fp16.h>

#include "wn_kernels.h"

namespace wn_split16 {

typedef _Float16 h8 __attribute__((ext_vector_type(8)));
typedef _Float16 h4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ f32x16 mfma16(h8 a, h8 b, f32x16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0);
}

// acc += a b: the three products of the split operands in the fixed order lo*hi, hi*lo, hi*hi.  The operands are taken by
// reference so that each is read where its product issues (by value, every read moves in front of the first product).
__device__ __forceinline__ void mfma3(const h8& a_hi, const h8& a_lo, const h8& b_hi, const h8& b_lo, f32x16& acc) {
  acc = mfma16(a_lo, b_hi, acc);
  acc = mfma16(a_hi, b_lo, acc);
  acc = mfma16(a_hi, b_hi, acc);
}

// hi = fp16(v), lo = fp16(v - hi) of 8 values (an array or two quads) or 4.  Round-to-nearest keeps the split error at
// 2^-22 |v| and unbiased (a packed round-toward-zero split is faster, but its truncation error is visible after Adam's
// normalisation on near-zero gradient entries).
__device__ __forceinline__ void split8(const float (&v)[8], h8& hi, h8& lo) {
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const _Float16 h = (_Float16)v[e];
    hi[e] = h;
    lo[e] = (_Float16)(v[e] - (float)h);
  }
}
__device__ __forceinline__ void split8(const f32x4& q0, const f32x4& q1, h8& hi, h8& lo) {
  const float v[8] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w};
  split8(v, hi, lo);
}
__device__ __forceinline__ void split4(const f32x4& q, h4& hi, h4& lo) {
  const float v[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const _Float16 h = (_Float16)v[e];
    hi[e] = h;
    lo[e] = (_Float16)(v[e] - (float)h);
  }
}

// the same with the operand scaled by s (an exact power of two): hi = fp16(v s), lo = fp16(v s - hi) with the product
// unrounded.  The fma is explicit: one operation fewer in loops that are VALU-bound on this split, and independent of the
// contraction mode.
__device__ __forceinline__ void split8s(const float (&v)[8], float s, h8& hi, h8& lo) {
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const _Float16 h = (_Float16)(v[e] * s);
    hi[e] = h;
    lo[e] = (_Float16)__builtin_fmaf(v[e], s, -(float)h);
  }
}
__device__ __forceinline__ void split8s(const f32x4& q0, const f32x4& q1, float s, h8& hi, h8& lo) {
  const float v[8] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w};
  split8s(v, s, hi, lo);
}
__device__ __forceinline__ void split4s(const f32x4& q, float s, h4& hi, h4& lo) {
  const float v[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const _Float16 h = (_Float16)(v[e] * s);
    hi[e] = h;
    lo[e] = (_Float16)__builtin_fmaf(v[e], s, -(float)h);
  }
}

// operand scale of a tensor with max-abs m: sc = 2^-e, inv = 2^e with m = f 2^e (0.5 <= f < 1), e clamped to +-100;
// sc = inv = 1 for m = 0 or not finite
__device__ __forceinline__ void pow2_scale(float m, float& sc, float& inv) {
  float s = 1.0f, i = 1.0f;
  if (m > 0.f && m < 3.0e38f) {
    int e;
    (void)frexpf(m, &e);
    e = max(-100, min(100, e));
    s = ldexpf(1.0f, -e);
    i = ldexpf(1.0f, e);
  }
  sc = s;
  inv = i;
}

// global-address-space 16-byte load.  Pointers that went through a per-segment select lose their address space and hipcc
// emits flat_load: flat loads also count on lgkmcnt, so every LDS fragment wait would drain the prefetched loads, and the
// compiler waits vmcnt(0) while one is pending.
__device__ __forceinline__ f32x4 ldg4(const float* p) { return *(const __attribute__((address_space(1))) f32x4*)(p); }
__device__ __forceinline__ f32x4 ldg4(const __attribute__((address_space(1))) char* p) {
  return *(const __attribute__((address_space(1))) f32x4*)p;
}
// ... of eight halves: one hi or lo weight fragment of a lane (generation kernels)
__device__ __forceinline__ h8 ldg_h8(const void* p) { return *(const __attribute__((address_space(1))) h8*)(p); }

// Quad rq (0..3) of a D-layout accumulator tile: a lane's values 4 rq .. 4 rq + 3 are four consecutive channels
// (8 rq + 4 h .. of the tile's 32), so a quad is what one 16-byte access of a bias, a row or an operand piece holds.
__device__ __forceinline__ f32x4 get_quad(const f32x16& v, int rq) {
  return f32x4{v[4 * rq + 0], v[4 * rq + 1], v[4 * rq + 2], v[4 * rq + 3]};
}
__device__ __forceinline__ void set_quad(f32x16& v, int rq, const f32x4& q) {
  v[4 * rq + 0] = q.x; v[4 * rq + 1] = q.y; v[4 * rq + 2] = q.z; v[4 * rq + 3] = q.w;
}
__device__ __forceinline__ void add_quad(f32x16& v, int rq, const f32x4& q) {
  v[4 * rq + 0] += q.x; v[4 * rq + 1] += q.y; v[4 * rq + 2] += q.z; v[4 * rq + 3] += q.w;
}

// acc += W^T b over k-steps K0 .. K0 + NK - 1: fragments w[k][hi, lo] in registers, hi|lo B operands in LDS (2 KB a k-step;
// bl = this lane's hi operand of k-step 0, the lo operand 64 further), the three products of a k-step in the order of the
// training kernels.  The operands of k-step k + 1 are requested BEFORE the products of k-step k are issued: written the
// plain way the compiler reads, waits, multiplies, reads, ... and every k-step pays an LDS round trip (measured on the
// conv1 waves of wn_gen_chain3_kernel: 1220 -> 550 cycles for the 12 products).
template <int K0, int NK, int NW>
__device__ __forceinline__ void mac_lds(f32x16& acc, const h8 (&w)[NW][2], const h8* bl) {
  static_assert(K0 + NK <= NW, "k-steps beyond the fragments");
  h8 bh[2], blo[2];
  bh[0] = bl[(K0 * 2 + 0) * 64];
  blo[0] = bl[(K0 * 2 + 1) * 64];
  wn_static_for<NK>([&](auto kc) {
    constexpr int ks = decltype(kc)::value;
    if constexpr (ks + 1 < NK) {
      bh[(ks + 1) & 1] = bl[((K0 + ks + 1) * 2 + 0) * 64];
      blo[(ks + 1) & 1] = bl[((K0 + ks + 1) * 2 + 1) * 64];
      __builtin_amdgcn_sched_barrier(0);            // keep the two reads above the products below
    }
    mfma3(w[K0 + ks][0], w[K0 + ks][1], bh[ks & 1], blo[ks & 1], acc);
  });
}

// LDS-DMA of 16 bytes per lane: global address = scalar base + 32-bit lane offset, LDS address = M0 + lane * 16.
// Inline assembly on purpose: through the builtin hipcc forms every address as a 64-bit VGPR pair, hoists the pairs out of
// the loop, spills them and reloads each with s_waitcnt vmcnt(0) in front of its request.  The
// compiler does not count these requests in its own vmcnt bookkeeping: its waits only become more conservative.
__device__ __forceinline__ void dma16(const void* sbase, unsigned voff, unsigned lds_addr) {
  asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1"
               :: "v"(voff), "s"(sbase), "s"(lds_addr) : "memory");   // (m0 is reserved: the compiler never keeps a value in it)
}
__device__ __forceinline__ unsigned lds_addr_of(const void* p) {
  return (unsigned)(uintptr_t)(const __attribute__((address_space(3))) unsigned char*)p;
}

// one 32 x 32 D-layout accumulator tile -> wave-private LDS stage (32 rows of PITCH floats) -> 128-byte row segments in
// HBM.  dst = wave-uniform address of the tile's first row (+ column offset), voff = this lane's byte offset inside a
// group of eight rows.  The base goes through an empty asm so that it stays ONE scalar (otherwise hipcc re-associates
// (tensor + lane offset) + row, hoists that 64-bit VGPR pair per output tensor out of the tile loop, spills it and reloads
// it with s_waitcnt vmcnt(0) in the middle of the stores); the asm drops the address space, which is restored, or the
// stores become flat_store.  FULL: all 32 rows exist (no per-row predicate).  ADD: add[i] is added to row group i before
// the store.  NOSTORE: timing ablation, a store only of a value that never occurs.
template <int PITCH, bool FULL, bool NOSTORE = false, bool ADD = false>
__device__ __forceinline__ void store_tile(const f32x16& v, float* stage, float* dst, unsigned voff, unsigned ld_bytes,
                                           int rows_valid, int lane, const f32x4* add = nullptr) {
  const int tl = lane & 31, h = lane >> 5;
#pragma unroll
  for (int rq = 0; rq < 4; ++rq) {
    f32x4 o;
    o.x = v[4 * rq + 0]; o.y = v[4 * rq + 1]; o.z = v[4 * rq + 2]; o.w = v[4 * rq + 3];
    *reinterpret_cast<f32x4*>(stage + tl * PITCH + 8 * rq + 4 * h) = o;
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  const float* rd = stage + (lane >> 3) * PITCH + (lane & 7) * 4;
  char* base0 = reinterpret_cast<char*>(dst);
  asm volatile("" : "+s"(base0));
  __attribute__((address_space(1))) char* base = (__attribute__((address_space(1))) char*)base0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    f32x4 o = *reinterpret_cast<const f32x4*>(rd + i * 8 * PITCH);
    if constexpr (ADD) { o.x += add[i].x; o.y += add[i].y; o.z += add[i].z; o.w += add[i].w; }
    if (NOSTORE ? (o.x == 1.2345e-30f) : (FULL || i * 8 + (lane >> 3) < rows_valid))
      *(__attribute__((address_space(1))) f32x4*)(base + (uint64_t)((unsigned)(i * 8) * ld_bytes) + voff) = o;
  }
  asm volatile("" ::: "memory");
}

// tile (32 rows x C floats) held as D-layout registers -> LDS stage -> coalesced rows in HBM.
// The rows leave as buffer stores on a descriptor that ends behind the tile's last valid row (dst and rows_valid are
// wave-uniform): the hardware drops the rows of a ragged tile, and no store sits in a branch.  As `if (row < rows_valid)`
// around a global store every store had an exec-skip branch of its own, and hipcc's wait counts behind them are those of
// the path that stored nothing: requests made before a tile's stores could not be told from the stores (vmcnt(15) where
// 38 were allowed).
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
template <int C32, int PITCH>
__device__ __forceinline__ void wn_store_tile(const f32x16 (&v)[C32], float* stage, float* dst, int ld, int rows_valid, int lane) {
  const int tl = lane & 31, h = lane >> 5;
#pragma unroll
  for (int j = 0; j < C32; ++j)
#pragma unroll
    for (int rq = 0; rq < 4; ++rq) {
      f32x4 o;
      o.x = v[j][4 * rq + 0]; o.y = v[j][4 * rq + 1]; o.z = v[j][4 * rq + 2]; o.w = v[j][4 * rq + 3];
      *reinterpret_cast<f32x4*>(stage + tl * PITCH + 32 * j + 8 * rq + 4 * h) = o;
    }
  // LDS instructions of one wave execute in order, so the reads below see every lane's writes;
  // the asm statements only stop the compiler from moving LDS accesses across the two phases
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  constexpr int LPR = C32 * 8;                 // lanes (16-byte pieces) per row
  constexpr int RPI = 64 / LPR;                // rows per store instruction
  const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(dst, 0, rows_valid * ld * 4, 0x00020000);
#pragma unroll
  for (int i = 0; i < 32 / RPI; ++i) {
    const int row = i * RPI + lane / LPR;
    const int col = (lane % LPR) * 4;
    const f32x4 o = *reinterpret_cast<const f32x4*>(stage + row * PITCH + col);
    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, o), rs, (row * ld + col) * 4, 0, 0);
  }
  asm volatile("" ::: "memory");
}

}  // namespace wn_split16
