// Backward-data chain, two products per launch (gfx950, split-precision MFMA):
//   g_x(b+1)[t] = W_0(b+1) g_u(b+1)[t + d] + W_1(b+1) g_u(b+1)[t] + g_x(b+2)[t]        (dilated conv of block b+1, reversed;
//                                                                                        + the residual path)
//   g_u(b)[t]   = gate'( W_r(b) g_x(b+1)[t] + V(b) dL/da[t] )                            (1x1 conv + folded skip path of block b)
// (src/layers.py:199-223 reversed; V(b) = W_s(b) W_f0, see wn_skip_fold in wn_elem.hip).  g_x(b+1) is the output gradient
// of block b at the SAME rows, so the tile a wave has just produced stays in its registers -- a 32x32 accumulator tile is,
// unchanged, the B operand of the next contraction over its channel index (wn_layer16.hip uses the same fact for z) --
// instead of going to HBM and back between two launches.  One launch per block boundary instead of two: every launch of
// the chain pays ~17 us of ramp (weight images -> LDS, first HBM latency) and drain on top of its bytes.
//
// Structure = the resident rows GEMM of wn_gemm16.hip twice: persistent workgroups of 8 waves, one 32-row tile per wave
// at a time, both weight images resident in LDS (A[64][256] of the reversed conv: 64 KiB; [W_r | V]: 48 KiB), a rolling
// register ring of 4 k-steps of activations that runs through both products and across tile boundaries (24 "memory"
// k-steps per tile: 8 of g_u[t + d], 8 of g_u[t], 8 of dL/da[t]; the 4 k-steps over g_x come from registers), epilogue
// operands requested ahead, outputs through a wave-private LDS stage of 32 columns (the images leave 36 KiB for stages) as
// 128-byte row segments.  Operand scaling: the first product uses the running max-abs of g_u(b+1) like the unfused
// kernel (bit-identical g_x); the second one cannot know the max-abs of the tensor it is producing, so every tile is
// scaled by the exact power of two of max(its own max |g_x|, running max-abs of dL/da).
//
// Waits: every load and store is compiler-visible and the code is shaped so that hipcc's own vmcnt counts come out right
// (no hand-written s_waitcnt vmcnt).  The tile body is instantiated once per position in a wave's
// walk (only tile, first of several, later with a successor, last): the ring refills that belong to the next tile are
// unconditional where there is one and absent where there is none, and no copy joins a state it is not entered with.
// Rows leave as buffer stores on a descriptor that ends behind the tile's last valid row, so no store sits in a branch.
// The tile index and all that follows from it (utterance, first row, valid rows, tensor bases) are scalar.
#include "wn_split16.h"

using namespace wn_split16;

namespace {

constexpr int BP_NK1 = 16;                       // k-steps of the reversed conv (KS * 2D / 16)
constexpr int BP_NKR = 4;                        // k-steps over g_x (R / 16), operands from registers
constexpr int BP_NKF = 8;                        // k-steps over dL/da (F0 / 16)
constexpr int BP_NKM = BP_NK1 + BP_NKF;          // memory k-steps per tile
constexpr int BP_W1 = BP_NK1 * 2 * 2048, BP_W2 = (BP_NKR + BP_NKF) * 2 * 2048;
constexpr int BP_PITCH = 36;
constexpr int BP_STAGE = 32 * BP_PITCH * 4;      // 4608
constexpr int BP_LDS = BP_W1 + BP_W2 + 8 * BP_STAGE;   // 151552
constexpr int BP_PF = 4;

// one 32 x 32 tile (D layout) -> LDS stage -> 128-byte row segments, through wn_store_tile (wn_split16.h): buffer stores on
// a descriptor that starts at dst and is rows_valid * ld * 4 bytes long (dst and rows_valid are wave-uniform).  dst is the
// tile's first row PLUS the sub-tile's column offset (32 j floats of a 64-float g_x row, 64 part + 32 j of a 128-float g_u
// row), so with c = that offset in bytes and L = ld * 4 (256 or 512) the segment of row r covers descriptor offsets
// [r L, r L + 128).  Valid rows: r <= rows_valid - 1, so r L + 128 <= rows_valid L - (L - 128) < rows_valid L: inside, whole
// (128 <= L).  Rows r >= rows_valid start at r L >= rows_valid L: outside, dropped by the hardware.  In tensor bytes the
// descriptor ends at c + rows_valid L, i.e. c bytes into the first row behind the tile -- but the only offsets a lane
// forms are r L + 16 q (q < 8), and none of those with r >= rows_valid is inside.
__device__ __forceinline__ void bp_store32(const f32x16& v, float* stage, float* dst, int ld, int rows_valid, int lane) {
  const f32x16 t[1] = {v};
  wn_store_tile<1, BP_PITCH>(t, stage, dst, ld, rows_valid, lane);
}

}  // namespace

__global__ __launch_bounds__(512, 2) void wn_bwd_pair_kernel(WnBwdPairArgs a) {
  __shared__ __attribute__((aligned(16))) unsigned char smem[BP_LDS];
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // uniform: what follows from the tile index stays in scalar registers
  const int tl = lane & 31, h = lane >> 5;
  float* stage = reinterpret_cast<float*>(smem + BP_W1 + BP_W2 + wave * BP_STAGE);
  {
    // both images in ONE round trip (wn_images_to_lds: every load in flight before the first LDS store)
    wn_images_to_lds<512, BP_W1 / 16, BP_W2 / 16>(a.wx16, smem, BP_W1 / 16, a.wu16, smem + BP_W1, BP_W2 / 16, tid);
  }
  __syncthreads();
  const h8* w1 = reinterpret_cast<const h8*>(smem) + lane;
  const h8* w2 = reinterpret_cast<const h8*>(smem + BP_W1) + lane;

  float sc1, inv1;
  pow2_scale(a.am_gu_in ? *a.am_gu_in : 0.f, sc1, inv1);
  const float gfmax = a.am_gf ? *a.am_gf : 0.f;

  const int tiles_per_b = (a.T + 31) >> 5;
  const int64_t ntiles = (int64_t)a.B * tiles_per_b;
  // Where a tile is: all of it wave-uniform (scalar registers).  Per lane there are only t0 + tl and the row clamps.
  struct TileCtx {
    int b, t0, rows_valid;
    int64_t row0;
  };
  auto make_ctx = [&](int64_t tile) {
    TileCtx c;
    c.b = (int)(tile / tiles_per_b);
    c.t0 = (int)(tile % tiles_per_b) * 32;
    c.rows_valid = min(32, a.T - c.t0);                            // 1 .. 32: every tile of a walk starts inside its utterance
    c.row0 = (int64_t)c.b * a.T + c.t0;
    return c;
  };
  // memory k-step m of a tile: 0..7 g_u(b+1)[t + d], 8..15 g_u(b+1)[t], 16..23 dL/da[t]  (straight-line, unconditional:
  // masked rows read a clamped row and are zeroed where they are consumed)
  auto load_x = [&](const TileCtx& c, int m, f32x4& q0, f32x4& q1, bool& okout) {
    const int seg = m >> 3;                                        // compile-time at every call
    const int kk = m & 7;
    const int t = c.t0 + tl;
    const int ts = t + (seg == 0 ? a.dil : 0);
    const bool ok = t < a.T && ts < a.T;
    const float* base = seg == 2 ? a.gf : a.gu_in;
    const float* src = base + ((int64_t)c.b * a.T + (ok ? ts : 0)) * 128 + 4 * h + 16 * kk;
    q0 = ldg4(src);
    q1 = ldg4(src + 8);
    okout = ok;
  };

  float wmax_x = 0.f, wmax_u = 0.f;
  const WnTileWalk walk = wn_tile_walk(ntiles, 8, wave);          // each XCD a contiguous eighth of the tiles (wn_common.h)
  TileCtx cur, nxt;
  f32x4 xr[BP_PF][2];
  bool okr[BP_PF];

  // One tile.  Whether it has a successor in the wave's walk (`nextc`) and whether its own first four k-steps are still to
  // be requested (`firstc`) are COMPILE-TIME properties: the body is instantiated once per position in the walk (below),
  // as in wn_layer_fwd_f16_kernel.  The ring refills of memory k-steps 20..23 belong to the next tile: with a successor
  // they are unconditional requests, without one there are none.  As one loop with `else if (has_next)` around them they
  // were four exec-skip branches and hipcc's wait counts those of the path that requested nothing (vmcnt(6) .. vmcnt(0) in
  // front of the tile's last products, i.e. a wait for the next tile's loads just issued); and the loop header joined the
  // prologue's state with the back edge's, so that a later tile's first product waited for the previous tile's stores.
  auto do_tile = [&](int64_t tile, auto nextc, auto firstc) __attribute__((always_inline)) {
    constexpr bool has_next = decltype(nextc)::value;
    constexpr bool first = decltype(firstc)::value;
    // The copies start alike: a marker that differs from copy to copy keeps hipcc from hoisting their common head in front
    // of the branch that chooses between them (see wn_layer16.hip).
    asm volatile("; pair tile body %0" ::"n"(2 * (int)has_next + (int)first) : "memory");
    if constexpr (first) {
      cur = make_ctx(tile);
#pragma unroll
      for (int k = 0; k < BP_PF; ++k) load_x(cur, k, xr[k][0], xr[k][1], okr[k]);
    }
    if constexpr (has_next) nxt = make_ctx(tile + walk.stride);
    const int rows_valid = cur.rows_valid;
    const int64_t row0 = cur.row0;
    const bool tin = cur.t0 + tl < a.T;
    const int64_t row = row0 + (tin ? tl : 0);                      // rows past the end read the tile's first row (unused)

    // ---- residual operand of the first product, requested before its contraction ----
    f32x4 addc[2][4];
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int rq = 0; rq < 4; ++rq) addc[j][rq] = ldg4(a.gx_res + row * 64 + 32 * j + 8 * rq + 4 * h);
    // pin them in front of the first operand split (in the loop copy hipcc started the split above them, with a wait for
    // the ring's first quad in front of these requests)
    __builtin_amdgcn_sched_barrier(0);

    // ---- g_x(b+1) = reversed dilated conv of g_u(b+1) ----
    f32x16 acc[2];
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;
    wn_static_for<BP_NK1>([&](auto mc) {
      constexpr int m = decltype(mc)::value;
      constexpr int k = m % BP_PF;
      h8 bh, bl;
      split8s(xr[k][0], xr[k][1], okr[k] ? sc1 : 0.f, bh, bl);
      __builtin_amdgcn_sched_barrier(0);
      load_x(cur, m + BP_PF, xr[k][0], xr[k][1], okr[k]);           // m + 4 <= 19 < 24: always this tile
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const h8 ah = w1[((m * 2 + j) * 2 + 0) * 64];
        const h8 al = w1[((m * 2 + j) * 2 + 1) * 64];
        mfma3(ah, al, bh, bl, acc[j]);
      }
      __builtin_amdgcn_sched_barrier(0);
    });
    // epilogue 1: + g_x(b+2) (residual path); rows past the utterance are exact zeros (they feed the next product)
    f32x16 gx[2];
    float tmax = 0.f;
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int rq = 0; rq < 4; ++rq) {
        const float cv[4] = {addc[j][rq].x, addc[j][rq].y, addc[j][rq].z, addc[j][rq].w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float v = tin ? acc[j][4 * rq + e] * inv1 + cv[e] : 0.f;
          gx[j][4 * rq + e] = v;
          tmax = fmaxf(tmax, fabsf(v));
        }
      }
    // ---- gate-derivative operands of block b, requested before the second contraction ----
    f32x4 sg[2][4], zz[2][4];
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int rq = 0; rq < 4; ++rq) {
        sg[j][rq] = ldg4(a.ag + row * 64 + 32 * j + 8 * rq + 4 * h);
        zz[j][rq] = ldg4(a.z + row * a.ldz + 32 * j + 8 * rq + 4 * h);
      }
    bp_store32(gx[0], stage, a.gx_out + row0 * 64, 64, rows_valid, lane);
    bp_store32(gx[1], stage, a.gx_out + row0 * 64 + 32, 64, rows_valid, lane);
    wmax_x = fmaxf(wmax_x, tmax);
    // per-tile power-of-two scale of the second product's B operands
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) tmax = fmaxf(tmax, __shfl_xor(tmax, o));
    float sc2, inv2;
    pow2_scale(fmaxf(tmax, gfmax), sc2, inv2);

    // ---- g_z = W_r g_x (registers: a D tile IS the B operand over its channel index) + V dL/da (memory) ----
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;
    wn_static_for<BP_NKR>([&](auto sc) {
      constexpr int ks = decltype(sc)::value;
      constexpr int jz = ks / 2, r0 = 8 * (ks % 2);
      f32x4 q0, q1;
      q0.x = gx[jz][r0 + 0]; q0.y = gx[jz][r0 + 1]; q0.z = gx[jz][r0 + 2]; q0.w = gx[jz][r0 + 3];
      q1.x = gx[jz][r0 + 4]; q1.y = gx[jz][r0 + 5]; q1.z = gx[jz][r0 + 6]; q1.w = gx[jz][r0 + 7];
      h8 bh, bl;
      split8s(q0, q1, sc2, bh, bl);
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const h8 ah = w2[((ks * 2 + j) * 2 + 0) * 64];
        const h8 al = w2[((ks * 2 + j) * 2 + 1) * 64];
        mfma3(ah, al, bh, bl, acc[j]);
      }
    });
    wn_static_for<BP_NKF>([&](auto mc) {
      constexpr int m = BP_NK1 + decltype(mc)::value;
      constexpr int k = m % BP_PF;
      h8 bh, bl;
      split8s(xr[k][0], xr[k][1], okr[k] ? sc2 : 0.f, bh, bl);
      __builtin_amdgcn_sched_barrier(0);
      constexpr int mn = m + BP_PF;
      if constexpr (mn < BP_NKM) load_x(cur, mn, xr[k][0], xr[k][1], okr[k]);
      else if constexpr (has_next) load_x(nxt, mn - BP_NKM, xr[k][0], xr[k][1], okr[k]);   // the next tile's k-steps 0..3
      constexpr int ks2 = BP_NKR + (m - BP_NK1);
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const h8 ah = w2[((ks2 * 2 + j) * 2 + 0) * 64];
        const h8 al = w2[((ks2 * 2 + j) * 2 + 1) * 64];
        mfma3(ah, al, bh, bl, acc[j]);
      }
      __builtin_amdgcn_sched_barrier(0);
    });
    // epilogue 2: gate derivative (filter half -> columns 0..63, gate half -> columns 64..127 of g_u)
#pragma unroll
    for (int part = 0; part < 2; ++part)
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        f32x16 o;
#pragma unroll
        for (int rq = 0; rq < 4; ++rq) {
          const float gv[4] = {sg[j][rq].x, sg[j][rq].y, sg[j][rq].z, sg[j][rq].w};
          const float zv[4] = {zz[j][rq].x, zz[j][rq].y, zz[j][rq].z, zz[j][rq].w};
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const float dz = acc[j][4 * rq + e] * inv2;
            const float v = tin ? (part == 0 ? wn_gate_bwd_f(dz, gv[e], zv[e]) : wn_gate_bwd_g(dz, gv[e], zv[e])) : 0.f;
            o[4 * rq + e] = v;
            wmax_u = fmaxf(wmax_u, fabsf(v));
          }
        }
        bp_store32(o, stage, a.gu_out + row0 * 128 + 64 * part + 32 * j, 128, rows_valid, lane);
      }
    if constexpr (has_next) cur = nxt;
  };
  using Next = std::true_type;
  using Last = std::false_type;
  using First = std::true_type;
  using Later = std::false_type;                          // enters with k-steps 0..3 requested and the last 16 g_u stores in flight
  if (walk.first < walk.end) {
    int64_t tile = walk.first;
    if (tile + walk.stride < walk.end) {
      do_tile(tile, Next{}, First{});
      for (tile += walk.stride; tile + walk.stride < walk.end; tile += walk.stride) do_tile(tile, Next{}, Later{});
      do_tile(tile, Last{}, Later{});
    } else {
      do_tile(tile, Last{}, First{});                     // the wave's only tile (every launch of up to 2048 tiles)
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    wmax_x = fmaxf(wmax_x, __shfl_xor(wmax_x, o));
    wmax_u = fmaxf(wmax_u, __shfl_xor(wmax_u, o));
  }
  if (lane == 0) {
    if (a.am_gx) wn_absmax_publish(a.am_gx, wmax_x);
    if (a.am_gu) wn_absmax_publish(a.am_gu, wmax_u);
  }
}

int wn_bwd_pair_supported(int R, int D, int KS, int F0) { return (R == 64 && D == 64 && KS == 2 && F0 == 128) ? 1 : 0; }

int wn_launch_bwd_pair(const WnBwdPairArgs& a, hipStream_t s) {
  const int64_t tiles = (int64_t)a.B * ((a.T + 31) / 32);
  if (tiles <= 0) return WN_OK;
  int64_t gx = (tiles + 7) / 8;
  if (gx > 256) gx = 256;
  hipLaunchKernelGGL(wn_bwd_pair_kernel, dim3((unsigned)gx), dim3(512), 0, s, a);
  WN_HIP_CHECK(hipGetLastError());
  return WN_OK;
}
