// One queued-generation time step through every residual block for R = D = 128 (gfx950): rows = utterances (<= 32 per
// tile).  Reference: WaveNetLayer.generate, src/layers.py:226-290 -- the step of WaveNetLayer.call on one time sample.
//
// The training-forward kernel of these blocks (wn_layer16s.hip) STREAMS its 320 KiB of weight images through LDS two
// 16 KiB chunks ahead.  With 32 time steps per wave that hides the stream; with one row per utterance it is ten dependent
// L2 round trips per block (25-30 us a block, 0.96 ms a step for 30 blocks = 1.0 k samples/s per utterance).  Here one
// workgroup of 8 waves takes a block; wave w owns output row tile w of the gated conv (32 of the 256 channels of u)
// and requests ALL 16 k-steps of its weight fragments, hi and lo, straight into registers before anything else (128
// VGPRs, one round trip for the whole conv), waves 0..3 also their 8 k-steps of the 1x1.  The operand rows (two taps x
// 128 channels of at most 32 utterances) are staged once in LDS in B-fragment order.
//
// Bit for bit the arithmetic of wn_layer_fwd_s128_kernel (the sliding window's kernel) per output element: accumulators
// start at the bias (+ conditioning bias), k-steps ascending with lo*hi, hi*lo, hi*hi each, the same gate functions, the
// 1x1 the same way from the z tiles, x_out = o + residual in fp32.  tests: queued == sliding window.
//
// Two kernels walk the blocks: wn_gen_chain128_kernel inside one workgroup, wn_gen_relay128_kernel as one workgroup per
// block.  Every piece of the step that both state -- the fragment requests, the operand pieces with the input conv, the
// accumulator from the bias, the skip epilogue -- is one function below; the products over LDS operands are mac_lds of
// wn_split16.h.  (A generate call that neither takes runs the sliding window's kernel per block: block_fwd_path.)
#include "wn_split16.h"

using namespace wn_split16;

namespace {

constexpr int R = 128, D = 128;
constexpr int NK1 = 16, NK2 = 8;                      // k-steps of the gated conv (two taps) | of the 1x1 and the skip contraction
// LDS: the conv's B operands, [16 k-steps][2][64 lanes] x 16 B (chain: fp32 quads q = 0, 1; relay: fp16 hi, lo) ...
constexpr int XOP_BYTES = NK1 * 2048;
constexpr int NPIECES = XOP_BYTES / 16, TAP_PIECES = NPIECES / 2;   // 16-byte operand pieces of both taps | of one
// ... chain: | gate tiles [4][16][64] floats | z tiles [4][16][64] floats
constexpr int TILE_FLOATS = 16 * 64;
// ... relay: | the newest tap in fp32 (the residual) [1024 pieces] | z operands, fp16 hi | lo, [8 k-steps][hi, lo][64]
constexpr int XRES_BYTES = TAP_PIECES * 16, ZOP_BYTES = NK2 * 2048;

// every hi|lo fragment of a wave, requested at once: k-step c at base + c * kstep_bytes, lo 1 KiB behind hi
template <int NK>
__device__ __forceinline__ void fetch_frags(h8 (&w)[NK][2], const char* base, int kstep_bytes) {
#pragma unroll
  for (int c = 0; c < NK; ++c) {
    w[c][0] = ldg_h8(base + c * kstep_bytes);
    w[c][1] = ldg_h8(base + c * kstep_bytes + 1024);
  }
}
// waves 0..3: the 1x1's fragments of row tile `wave`; 4..7 (skip contraction in the chain): block b's of column tile wave - 4
__device__ __forceinline__ void fetch_frags_r(h8 (&wr)[NK2][2], const WnGen128Args& a, const WnGenBlock& g, int b, int wave, int lane) {
  const char* base = wave < 4 ? reinterpret_cast<const char*>(a.ws + g.w16r_off) + (int64_t)wave * 2048 + lane * 16
                              : reinterpret_cast<const char*>(a.ws + a.skip_w16_off) + (int64_t)b * (NK2 * 8192) +
                                    (int64_t)(wave - 4) * 2048 + lane * 16;
  fetch_frags(wr, base, 8192);
}

// operand piece e of an utterance tile, in B-fragment order: (c, q, l) = channels ch0 .. ch0 + 3 of utterance `row`, tap c / 8
struct Piece { int c, q, l, row, ch0; };
__device__ __forceinline__ Piece piece_of(int e, int tile) {
  Piece p;
  p.c = e >> 7; p.q = (e >> 6) & 1; p.l = e & 63;
  p.row = tile * 32 + (p.l & 31);
  p.ch0 = 16 * (p.c & 7) + 8 * p.q + 4 * (p.l >> 5);
  return p;
}
// block 0's newest tap = the input causal conv of this step (src/model.py:84-88,228), computed here with the arithmetic of
// wn_inconv_fwd_kernel (fma chain over the taps from zero, then + bias) and written to the block's ring slot
__device__ __forceinline__ f32x4 piece_inconv(const WnGen128Args& a, const WnGenBlock& g0, const Piece& p) {
  float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
  for (int tap = 0; tap < 2; ++tap) {
    const float xv = a.xin[(int64_t)((a.tau - (1 - tap)) % 2) * a.B + (p.row < a.B ? p.row : 0)];
    const f32x4 wv = ldg4(a.causal_w + (int64_t)tap * R + p.ch0);
    a0 = fmaf(wv.x, xv, a0); a1 = fmaf(wv.y, xv, a1); a2 = fmaf(wv.z, xv, a2); a3 = fmaf(wv.w, xv, a3);
  }
  const f32x4 bv = ldg4(a.causal_b + p.ch0);
  const f32x4 v = f32x4{a0 + bv.x, a1 + bv.y, a2 + bv.z, a3 + bv.w};
  if (p.row < a.B) *reinterpret_cast<f32x4*>(a.ws + g0.ring_off + (int64_t)(a.tau % g0.nslots) * a.B * R + (int64_t)p.row * R + p.ch0) = v;
  return v;
}
// the piece's value: from the tap's ring rows (block 0's newest tap: the input conv, when the launch carries it), zero
// beyond the last utterance
__device__ __forceinline__ f32x4 piece_value(const WnGen128Args& a, const WnGenBlock& g, const float* xold, const float* xnew, const Piece& p) {
  const float* src = (p.c < 8 ? xold : xnew) + (int64_t)(p.row < a.B ? p.row : 0) * R + p.ch0;
  f32x4 v;
  if (p.c >= 8 && a.xin) v = piece_inconv(a, g, p);
  else v = ldg4(src);
  if (p.row >= a.B) v = f32x4{0.f, 0.f, 0.f, 0.f};
  return v;
}

// accumulator of a row tile of the gated conv: the bias, + the utterance's conditioning-bias row (wn_layer_fwd_s128_kernel
// adds the conditioning bias of the tile's utterance: rows of a tile are one utterance there, one utterance per column
// here).  ch(rq) = first of the four channels of accumulator quad rq.
template <typename Ch>
__device__ __forceinline__ void acc_from_bias(f32x16& u, const float* bias, bool has_cb, const float* cb_row, Ch ch) {
#pragma unroll
  for (int rq = 0; rq < 4; ++rq) set_quad(u, rq, ldg4(bias + ch(rq)));
  if (has_cb) {
#pragma unroll
    for (int rq = 0; rq < 4; ++rq) add_quad(u, rq, ldg4(cb_row + ch(rq)));
  }
}

// acc += W^T z over the 8 k-steps of the 1x1 or of the skip contraction, B operand = the fp32 z tiles as they stand
// (k-step ks = rows 8 (ks & 1) .. + 7 of tile ks / 2), split in front of its products
__device__ __forceinline__ void mac_ztiles(f32x16& acc, const h8 (&w)[NK2][2], const float* zs, int lane) {
#pragma unroll
  for (int ks = 0; ks < NK2; ++ks) {
    const float* z = zs + ((ks >> 1) * 16 + 8 * (ks & 1)) * 64 + lane;
    const f32x4 q0 = {z[0 * 64], z[1 * 64], z[2 * 64], z[3 * 64]};
    const f32x4 q1 = {z[4 * 64], z[5 * 64], z[6 * 64], z[7 * 64]};
    h8 bh, bl;
    split8(q0, q1, bh, bl);
    mfma3(w[ks][0], w[ks][1], bh, bl, acc);
  }
}

// where the rows of block b go besides the next block's operands: the next block's ring slot of this time step, the head's
// input row behind the last block (use_skip False), or nowhere
__device__ __forceinline__ float* rows_dst(const WnGen128Args& a, int b) {
  if (b + 1 < a.nblocks) {
    const WnGenBlock gn = a.blocks[b + 1];
    return a.ws + gn.ring_off + (int64_t)(a.tau % gn.nslots) * a.B * R;
  }
  return a.hrow_off >= 0 ? a.ws + a.hrow_off : nullptr;
}

// column tile j of the folded skip contraction, finished: + bias, activation, range guard, store -- the epilogue of
// wn_gemm_planes16s_kernel, which runs this contraction for the sliding window
__device__ __forceinline__ void skip_epilogue(const WnGen128Args& a, const f32x16& sacc, int j, int h, int row, bool rok, float& wmax) {
#pragma unroll
  for (int rq = 0; rq < 4; ++rq) {
    const int n0 = 32 * j + 8 * rq + 4 * h;
    const f32x4 bv = ldg4(a.ws + a.skip_bias_off + n0);
    f32x4 v;
    v.x = wn_act(sacc[4 * rq + 0] + bv.x, a.skip_act); v.y = wn_act(sacc[4 * rq + 1] + bv.y, a.skip_act);
    v.z = wn_act(sacc[4 * rq + 2] + bv.z, a.skip_act); v.w = wn_act(sacc[4 * rq + 3] + bv.w, a.skip_act);
    if (rok) {
      wmax = wn_absmax_acc(wmax, v.x, v.y, v.z, v.w);
      *reinterpret_cast<f32x4*>(a.ws + a.skiprow_off + (int64_t)row * 128 + n0) = v;
    }
  }
}

}  // namespace

// All residual blocks of one queued-generation step in ONE launch (R = D = 128, kernel size 2, depth 1): the loop over
// blocks inside the workgroup.  The gate pairs tiles j and j + 4 through LDS, the 1x1 reads the z tiles back as they
// stand.  Block b's output rows stay in LDS as the newest tap of block b + 1 (a D-layout tile IS the next conv's B-operand
// piece of the same lane) and as its residual; only the older tap comes from the block's ring.  Per block: one round trip
// for the weight fragments, 48 + 24 products, three barriers.
__global__ __launch_bounds__(512, 2) void wn_gen_chain128_kernel(WnGen128Args a) {
  __shared__ __attribute__((aligned(16))) unsigned char smem[XOP_BYTES + 2 * 4 * TILE_FLOATS * 4];
  f32x4* xs = reinterpret_cast<f32x4*>(smem);
  float* gs = reinterpret_cast<float*>(smem + XOP_BYTES);
  float* zs = gs + 4 * TILE_FLOATS;
  const int tid0 = threadIdx.x, lane = tid0 & 63, wave = __builtin_amdgcn_readfirstlane(tid0 >> 6);
  const int tl = lane & 31, h = lane >> 5;
  const int row = blockIdx.x * 32 + tl;
  const bool rok = row < a.B;
  float wmax = 0.f;
  // folded skip contraction (a.skip_tiles == 4: 128 columns): waves 4..7 own one column tile each and carry its accumulator
  // through all blocks -- k ascending over (block, k-step) from zero, as wn_gemm_planes16s_kernel runs it
  const bool skip_on = a.skip_w16_off >= 0;
  f32x16 sacc;
#pragma unroll
  for (int r = 0; r < 16; ++r) sacc[r] = 0.f;
  for (int b = 0; b < a.nblocks; ++b) {
    // (the thread index goes through an empty asm once per block: what is derived from it is then a few vector operations
    // per block, not per-lane addresses hoisted out of the block loop, spilled and reloaded with s_waitcnt vmcnt(0) in
    // front of the staging and bias loads)
    int tid = tid0;
    asm volatile("" : "+v"(tid));
    const int lane = tid & 63, tl = lane & 31, h = lane >> 5;
    const int row = blockIdx.x * 32 + tl;
    const bool rok = row < a.B;
    const WnGenBlock g = a.blocks[b];
    h8 wd[NK1][2];
    fetch_frags(wd, reinterpret_cast<const char*>(a.ws + g.w16d_off) + (int64_t)wave * 2048 + lane * 16, 16384);
    h8 wr[NK2][2];                                     // waves 0..3: the 1x1's fragments; 4..7: the skip contraction's
    f32x4 bv4[4];
    if (wave < 4 || skip_on) fetch_frags_r(wr, a, g, b, wave, lane);
    // operand rows: the older tap from the ring (block 0: the newest tap too, written by the input conv's launch)
    const float* ring = a.ws + g.ring_off;
    const float* xold = ring + (int64_t)((a.tau - g.dilation) % g.nslots) * a.B * R;
    const float* xnew = ring + (int64_t)(a.tau % g.nslots) * a.B * R;
    const int npieces = b == 0 ? NPIECES : TAP_PIECES;
    for (int e = tid; e < npieces; e += 512) xs[e] = piece_value(a, g, xold, xnew, piece_of(e, blockIdx.x));
    f32x16 u;
    acc_from_bias(u, a.params + g.bias_d_off, g.cb_off >= 0, a.ws + g.cb_off + (int64_t)(rok ? row : 0) * 2 * D,
                  [&](int rq) { return 32 * wave + 8 * rq + 4 * h; });
    __syncthreads();
#pragma unroll
    for (int c = 0; c < NK1; ++c) {
      const f32x4 q0 = xs[(c * 2 + 0) * 64 + lane], q1 = xs[(c * 2 + 1) * 64 + lane];
      h8 bh, bl;
      split8(q0, q1, bh, bl);
      mfma3(wd[c][0], wd[c][1], bh, bl, u);
    }
    // ---- gate: tiles 4..7 hold the gate channels of tiles 0..3 ----
    if (wave >= 4) {
#pragma unroll
      for (int r = 0; r < 16; ++r) gs[((wave - 4) * 16 + r) * 64 + lane] = wn_sigmoid_fast(u[r]);
    }
    __syncthreads();
    if (wave < 4) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float sg = gs[(wave * 16 + r) * 64 + lane];
        u[r] = wn_tanh_fast(u[r]) * sg;
        zs[(wave * 16 + r) * 64 + lane] = u[r];
      }
      if (rok) {
        float* zp = a.ws + a.zrow_off + ((int64_t)b * a.B + row) * D + 32 * wave + 4 * h;
#pragma unroll
        for (int rq = 0; rq < 4; ++rq) *reinterpret_cast<f32x4*>(zp + 8 * rq) = get_quad(u, rq);
      }
      // (the 1x1's bias, requested here, when the conv's weight registers are free: in flight across the barrier)
#pragma unroll
      for (int rq = 0; rq < 4; ++rq) bv4[rq] = ldg4(a.params + g.bias_r_off + 32 * wave + 8 * rq + 4 * h);
    }
    __syncthreads();
    if (wave < 4) {
      f32x16 o;
#pragma unroll
      for (int rq = 0; rq < 4; ++rq) set_quad(o, rq, bv4[rq]);
      mac_ztiles(o, wr, zs, lane);
      // residual = this lane's own pieces of the newest tap in LDS; x_out goes back into the same pieces (the next block's
      // newest tap) and to the next block's ring slot
      float* dst = rows_dst(a, b);
#pragma unroll
      for (int rq = 0; rq < 4; ++rq) {
        f32x4 ov = get_quad(o, rq);
        const int piece = ((8 + 2 * wave + (rq >> 1)) * 2 + (rq & 1)) * 64 + lane;
        if (rok) wmax = wn_absmax_acc(wmax, ov.x, ov.y, ov.z, ov.w);
        if (a.residual) {
          const f32x4 rv = xs[piece];
          if (rok) wmax = wn_absmax_acc(wmax, rv.x, rv.y, rv.z, rv.w);
          ov.x += rv.x; ov.y += rv.y; ov.z += rv.z; ov.w += rv.w;
        }
        xs[piece] = rok ? ov : f32x4{0.f, 0.f, 0.f, 0.f};
        if (dst && rok) *reinterpret_cast<f32x4*>(dst + (int64_t)row * R + 32 * wave + 8 * rq + 4 * h) = ov;
      }
    }
    else if (skip_on) mac_ztiles(sacc, wr, zs, lane);
    // (the next iteration's barrier after staging orders these LDS writes before the conv reads them; zs is rewritten
    // two barriers later)
  }
  if (skip_on && wave >= 4) skip_epilogue(a, sacc, wave - 4, h, row, rok, wmax);
  if (a.guard && (wave < 4 || skip_on)) {
    wmax = wn_wave_absmax_bits(wmax);
    if (lane == 0) wn_absmax_publish_any(a.guard, wmax);
  }
}

// ------------------------------------------------------------------------------------------------------------------
// The same step as a RELAY over workgroups: one workgroup per (block, utterance tile), all of them resident at once.
//
// wn_gen_chain128_kernel walks the blocks inside ONE workgroup, and every block starts with a cold round trip for its
// 384 KiB of weight fragments through one CU (13 us a block: 0.39 ms a step, 2.5 k samples/s per utterance).  Here
// workgroup b requests the fragments of ITS block the moment the launch starts -- all blocks at once, every CU its own
// fetch path -- stages the older tap (written by an earlier launch) and runs that tap's half of the gated conv (k-steps
// 0..7 come first in the summation order anyway) while the chain is still upstream.  Then it waits for its block input,
// which workgroup b - 1 hands over through memory, finishes the block and hands its output on.  The skip accumulator
// travels the same way between the waves 4..7 of consecutive workgroups (its summation order is block order), off the
// critical path.  Per element the arithmetic is wn_gen_chain128_kernel's, operation for operation.
//
// Hand-off (guide: Guideline 16, form R2 "the data is the flag"): every handed-over fp32 value travels as one naturally
// aligned 8-byte granule {value, epoch} written by ONE relaxed agent-scope (sc1, write-through) atomic store and read by
// relaxed agent-scope atomic loads (sc1: past the reader's L1), re-read until every tag of the wave equals the launch's
// epoch.  No flags, no fences.  Epoch = the step index inside the wn_generate call (>= 1); wn_generate zeroes the granule
// area once per call.  A workgroup only ever waits for the workgroup before it, which has a smaller index and is
// therefore dispatched no later: the chain drains whatever the residency.  Every wait is bounded: a reader that gives up
// records the block in a.tmo and carries on with what it has (wn_generate reports the call as failed afterwards), so
// the launch ends in any case.
typedef __attribute__((address_space(1))) unsigned long long wn_gu64;
#define WN_RLX_AGENT __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT
#define WN_RELAY_SPINS (1u << 21)

namespace {

__device__ __forceinline__ void granule_store(unsigned long long* g, unsigned epoch, float v) {
  __hip_atomic_store((wn_gu64*)g, ((unsigned long long)epoch << 32) | (unsigned long long)__float_as_uint(v), WN_RLX_AGENT);
}
__device__ __forceinline__ unsigned long long granule_load(const unsigned long long* g) {
  return __hip_atomic_load((wn_gu64*)g, WN_RLX_AGENT);
}
// Two granules side by side in one 16-byte access ({value, epoch, value, epoch}): each 8-byte half is a granule of its own
// (a 16-byte sc1 access has never been seen to tear an aligned 8-byte half on gfx950; the halves are checked separately).
// Buffer instructions with aux = 16 (sc1): half the requests of 8-byte atomics -- a request costs the issuing wave ~100
// clocks and the sender's stores sit on the chain's critical path.
__device__ __forceinline__ void granule2_store(__amdgpu_buffer_rsrc_t rs, unsigned off, unsigned epoch, float v0, float v1) {
  const u32x4 q = {__float_as_uint(v0), epoch, __float_as_uint(v1), epoch};
  __builtin_amdgcn_raw_buffer_store_b128(q, rs, (int)off, 0, 16);
}
__device__ __forceinline__ u32x4 granule2_load(__amdgpu_buffer_rsrc_t rs, unsigned off) {
  return __builtin_amdgcn_raw_buffer_load_b128(rs, (int)off, 0, 16);
}
__device__ __forceinline__ void relay_give_up(unsigned* tmo, int code, int lane) {
  if (lane == 0) __hip_atomic_store((__attribute__((address_space(1))) unsigned*)tmo, (unsigned)code, WN_RLX_AGENT);
}

}  // namespace

__global__ __launch_bounds__(512, 2) void wn_gen_relay128_kernel(WnGen128Args a) {
  // LDS: B operands of the conv, ALREADY split into fp16 hi | lo, [16 k-steps][hi, lo][64 lanes] x 16 B -- the split is done
  // once by the thread that stages a piece, not by each of the eight waves in front of every product (the operand
  // conversions sat between the LDS read and the products of every k-step of the critical path) | the newest tap in fp32
  // (the residual) [1024 pieces] | z operands, split the same way, [8 k-steps][hi, lo][64]
  __shared__ __attribute__((aligned(16))) unsigned char smem[XOP_BYTES + XRES_BYTES + ZOP_BYTES];
  __shared__ unsigned x_sent;                          // waves 0..3 that have issued their hand-over stores
  h8* const xh = reinterpret_cast<h8*>(smem);
  f32x4* const xr = reinterpret_cast<f32x4*>(smem + XOP_BYTES);
  h8* const zh = reinterpret_cast<h8*>(smem + XOP_BYTES + XRES_BYTES);
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int tl = lane & 31, h = lane >> 5;
  // quad q (0, 1) of k-step ks of lane l: the split8 on one half of the operand
  auto put_quad = [&](h8* base, int ks, int q, int l, const f32x4& v) {
    h4 hi, lo;
    split4(v, hi, lo);
    h4* b4 = reinterpret_cast<h4*>(base);
    b4[((ks * 2 + 0) * 64 + l) * 2 + q] = hi;
    b4[((ks * 2 + 1) * 64 + l) * 2 + q] = lo;
  };
  const int b = (int)blockIdx.x / a.ntiles, tile = (int)blockIdx.x % a.ntiles;   // block-major: predecessors first
  const int row = tile * 32 + tl;
  const bool rok = row < a.B;
  const unsigned epoch = a.epoch;
  const bool skip_on = a.skip_w16_off >= 0;
  const bool last = b + 1 == a.nblocks;
  float wmax = 0.f;
  // knob 24: s_memtime stamps of tile 0, [block][8]: 0 entry, 1 older tap staged, 2 older tap's products done, 3 input arrived (every wave's pieces in LDS),
  // 4 z ready, 5 output handed on (wave 0); 6 skip accumulator arrived, 7 handed on (wave 4)
#define RL_TS(w, k) do { if (a.ts && tile == 0 && tid == 64 * (w)) a.ts[b * 8 + (k)] = __builtin_amdgcn_s_memtime(); } while (0)
  RL_TS(0, 0);
  // waves 0..3 carry the rows (the chain's critical path) through the 1x1 and share their SIMDs' matrix pipes with the skip
  // waves 4..7, whose accumulator has a block's worth of slack: issue priority to waves 0..3 (as in wn_gen_chain3_kernel)
  if (wave < 4) __builtin_amdgcn_s_setprio(3);
  if (tid == 0) x_sent = 0;                            // (visible after the first barrier; first read far behind it)
  const WnGenBlock g = a.blocks[b];
  // granule areas of this workgroup's INPUT (written by block b - 1) and OUTPUT (read by block b + 1)
  unsigned long long* const gbase = reinterpret_cast<unsigned long long*>(a.ws + a.relay_off);
  auto xg_of = [&](int blk) { return gbase + ((int64_t)blk * a.ntiles + tile) * 8192; };            // [1024 pieces][4]
  auto sg_of = [&](int blk) { return gbase + ((int64_t)(a.nblocks + blk) * a.ntiles + tile) * 8192 ; };   // [4][64][16] (+ pad)

  // ---- every weight fragment of this wave, requested at once ----
  h8 wd[NK1][2];
  {
    // Wave w owns a MIXED row tile of the gated conv: rows 0..15 = filter channels 16 w .. 16 w + 15, rows 16..31 = the gate
    // channels of the same 16 (the two 16-row halves of image tiles w / 2 and 4 + w / 2), as in wn_gen_chain3_kernel.  A
    // lane's 16 accumulators are then 8 filter values and THEIR 8 gate values: the gate runs in registers, nothing is
    // exchanged through LDS, and every wave ends up with one k-step of z.  Only the lanes' fetch addresses differ from
    // a plain tile: every output element is the same dot product over the same operands in the same order.
    const int src_tile = tl < 16 ? (wave >> 1) : 4 + (wave >> 1);
    const int src_lane = 32 * h + 16 * (wave & 1) + (tl & 15);
    fetch_frags(wd, reinterpret_cast<const char*>(a.ws + g.w16d_off) + (int64_t)src_tile * 2048 + src_lane * 16, 16384);
  }
  h8 wr[NK2][2];                                       // waves 0..3: the 1x1's fragments; 4..7: the skip contraction's
  if (wave < 4 || skip_on) fetch_frags_r(wr, a, g, b, wave, lane);
  // ---- operand rows of the older tap (block 0: of both taps) -> LDS in B-fragment order ----
  const float* ring = a.ws + g.ring_off;
  const float* xold = ring + (int64_t)((a.tau - g.dilation) % g.nslots) * a.B * R;
  const float* xnew = ring + (int64_t)(a.tau % g.nslots) * a.B * R;
  const int npieces = b == 0 ? NPIECES : TAP_PIECES;
  for (int e = tid; e < npieces; e += 512) {
    const Piece p = piece_of(e, tile);
    const f32x4 v = piece_value(a, g, xold, xnew, p);
    put_quad(xh, p.c, p.q, p.l, v);
    if (p.c >= 8) xr[e - TAP_PIECES] = v;
  }
  // accumulator quad rq of the mixed tile: channels 16 w + 8 rq + 4 h .. (rq = 0, 1: filter), D + 16 w + 8 (rq - 2) + 4 h .. (gate)
  auto uch = [&](int rq) { return (rq < 2 ? 0 : D - 16) + 16 * wave + 8 * rq + 4 * h; };
  f32x16 u;
  acc_from_bias(u, a.params + g.bias_d_off, g.cb_off >= 0, a.ws + g.cb_off + (int64_t)(rok ? row : 0) * 2 * D, uch);
  // (far down the chain: one lane watches the hand-off INTO the block before this one, so that the whole workgroup
  // only starts polling when its own input is one block away -- 29 workgroups x 512 lanes re-reading their granules for
  // the whole step would load the fabric the chain's own hand-offs travel on)
  if (b >= 2 && tid == 0) {
    const unsigned long long* w = xg_of(b - 1);
    for (unsigned spins = 0; (unsigned)(granule_load(w) >> 32) != epoch; ) {
      if (++spins > WN_RELAY_SPINS) { relay_give_up(a.tmo, b, 0); break; }
      __builtin_amdgcn_s_sleep(8);
    }
  }
  __syncthreads();
  RL_TS(0, 1);
  // ---- gated conv, older tap: k-steps 0..7 ----
  mac_lds<0, NK1 / 2>(u, wd, xh + lane);
  RL_TS(0, 2);
  // ---- the block input of this step, from block b - 1: pieces 1024..2047 (2 per thread, 4 granules each) ----
  if (b > 0) {
    const unsigned long long* xg = xg_of(b);
    f32x4 v[2];
    bool lv[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int e = tid + 512 * i;
      lv[i] = tile * 32 + (e & 31) < a.B;
      v[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    const __amdgpu_buffer_rsrc_t xrs = __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned long long*>(xg), 0, 65536, 0x00020000);
    for (unsigned spins = 0;;) {
      bool ok = true;
      u32x4 q[2][2];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        if (lv[i]) {
          q[i][0] = granule2_load(xrs, (unsigned)(tid + 512 * i) * 32u);
          q[i][1] = granule2_load(xrs, (unsigned)(tid + 512 * i) * 32u + 16u);
        }
      }
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        if (lv[i]) {
          ok = ok && q[i][0].y == epoch && q[i][0].w == epoch && q[i][1].y == epoch && q[i][1].w == epoch;
          v[i] = f32x4{__uint_as_float(q[i][0].x), __uint_as_float(q[i][0].z), __uint_as_float(q[i][1].x), __uint_as_float(q[i][1].z)};
        }
      }
      if (__all(ok)) break;                            // wave-uniform
      if (++spins > WN_RELAY_SPINS) { relay_give_up(a.tmo, 1000 + b, lane); break; }
      __builtin_amdgcn_s_sleep(1);
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int e = tid + 512 * i;                       // piece 1024 + e: k-step 8 + (e >> 7), quad (e >> 6) & 1, lane e & 63
      put_quad(xh, 8 + (e >> 7), (e >> 6) & 1, e & 63, v[i]);
      xr[e] = v[i];
    }
    __syncthreads();
    RL_TS(0, 3);
  }
  // ---- gated conv, newest tap: k-steps 8..15 ----
  mac_lds<NK1 / 2, NK1 / 2>(u, wd, xh + lane);
  // The skip accumulator of block b - 1 was handed over BEFORE that block's rows (its products run while the 1x1 of the
  // rows is still busy), so it has landed by now: waves 4..7 request it here, under the gate's transcendentals, and check the
  // tags once z is in LDS.  Kept out of the phase in which waves 0..3 issue their hand-over stores: those are the chain's
  // critical path, they share the CU's one memory queue with every other request of the workgroup, and a wave that
  // polls 8 x 16 B per lane there was measured to stretch "z ready -> rows handed on" from 1.8 to 2.9 us.
  const bool skip_recv = skip_on && wave >= 4 && b > 0 && rok;
  const int sj = wave - 4;
  u32x4 sq[8];
  if (skip_recv) {
    const __amdgpu_buffer_rsrc_t srs = __builtin_amdgcn_make_buffer_rsrc(sg_of(b), 0, 65536, 0x00020000);
#pragma unroll
    for (int r = 0; r < 8; ++r) sq[r] = granule2_load(srs, (unsigned)(sj * 64 + lane) * 128u + 16u * r);
  }
  // the gate, in registers: accumulators 0..7 are filter channels, 8..15 their gate channels; z = k-step `wave` of the
  // 1x1 and the skip contraction, split into fp16 hi | lo on the way into LDS
  f32x4 zq[2];
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    zq[q].x = wn_tanh_fast(u[4 * q + 0]) * wn_sigmoid_fast(u[8 + 4 * q + 0]);
    zq[q].y = wn_tanh_fast(u[4 * q + 1]) * wn_sigmoid_fast(u[8 + 4 * q + 1]);
    zq[q].z = wn_tanh_fast(u[4 * q + 2]) * wn_sigmoid_fast(u[8 + 4 * q + 2]);
    zq[q].w = wn_tanh_fast(u[4 * q + 3]) * wn_sigmoid_fast(u[8 + 4 * q + 3]);
    put_quad(zh, wave, q, lane, zq[q]);
  }
  f32x4 bv4[4];
  if (wave < 4) {
#pragma unroll
    for (int rq = 0; rq < 4; ++rq) bv4[rq] = ldg4(a.params + g.bias_r_off + 32 * wave + 8 * rq + 4 * h);
  }
  __syncthreads();
  RL_TS(0, 4);
  auto store_zrow = [&]() {                              // gated activations of this block (later launches only)
    if (rok) {
      float* zp = a.ws + a.zrow_off + ((int64_t)b * a.B + row) * D + 16 * wave + 4 * h;
      *reinterpret_cast<f32x4*>(zp) = zq[0];
      *reinterpret_cast<f32x4*>(zp + 8) = zq[1];
    }
  };
  if (wave < 4) {
    f32x16 o;
#pragma unroll
    for (int rq = 0; rq < 4; ++rq) set_quad(o, rq, bv4[rq]);
    mac_lds<0, NK2>(o, wr, zh + lane);
    // residual = this lane's own pieces of the newest tap; the sum goes to block b + 1 as granules FIRST (its workgroup
    // is waiting for them), then to that block's ring slot of this time step (read by later launches only)
    unsigned long long* xgn = last ? nullptr : xg_of(b + 1);
    float* dst = rows_dst(a, b);
    const __amdgpu_buffer_rsrc_t xnrs = __builtin_amdgcn_make_buffer_rsrc(xgn ? xgn : gbase, 0, 65536, 0x00020000);
    f32x4 ov[4];
#pragma unroll
    for (int rq = 0; rq < 4; ++rq) {
      ov[rq] = get_quad(o, rq);
      const int piece = ((8 + 2 * wave + (rq >> 1)) * 2 + (rq & 1)) * 64 + lane;
      if (rok) wmax = wn_absmax_acc(wmax, ov[rq].x, ov[rq].y, ov[rq].z, ov[rq].w);
      if (a.residual) {
        const f32x4 rv = xr[piece - TAP_PIECES];
        if (rok) wmax = wn_absmax_acc(wmax, rv.x, rv.y, rv.z, rv.w);
        ov[rq].x += rv.x; ov[rq].y += rv.y; ov[rq].z += rv.z; ov[rq].w += rv.w;
      }
      if (xgn && rok && b != a.mute_block) {
        granule2_store(xnrs, (unsigned)(piece - TAP_PIECES) * 32u, epoch, ov[rq].x, ov[rq].y);
        granule2_store(xnrs, (unsigned)(piece - TAP_PIECES) * 32u + 16u, epoch, ov[rq].z, ov[rq].w);
      }
    }
    if (lane == 0) __hip_atomic_fetch_add(&x_sent, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    RL_TS(0, 5);
    if (dst && rok) {
#pragma unroll
      for (int rq = 0; rq < 4; ++rq) *reinterpret_cast<f32x4*>(dst + (int64_t)row * R + 32 * wave + 8 * rq + 4 * h) = ov[rq];
    }
    store_zrow();
  }
  if (wave >= 4 && skip_on) {
    // ---- folded skip contraction: the accumulator of column tile wave - 4 arrives from block b - 1 (same lane, same
    //      register), takes this block's 24 products, and travels on (or, after the last block, through the epilogue of
    //      wn_gemm_planes16s_kernel) ----
    const int j = wave - 4;
    f32x16 sacc;
#pragma unroll
    for (int r = 0; r < 16; ++r) sacc[r] = 0.f;
    if (skip_recv) {
      const __amdgpu_buffer_rsrc_t srs = __builtin_amdgcn_make_buffer_rsrc(sg_of(b), 0, 65536, 0x00020000);
      const unsigned soff = (unsigned)(j * 64 + lane) * 128u;
      for (unsigned spins = 0;;) {
        bool ok = true;
#pragma unroll
        for (int r = 0; r < 8; ++r) {
          ok = ok && sq[r].y == epoch && sq[r].w == epoch;
          sacc[2 * r] = __uint_as_float(sq[r].x);
          sacc[2 * r + 1] = __uint_as_float(sq[r].z);
        }
        if (ok) break;                                  // (per lane: the lanes of a wave leave the loop one by one)
        if (++spins > WN_RELAY_SPINS) { relay_give_up(a.tmo, 2000 + b, 0); break; }
        __builtin_amdgcn_s_sleep(1);
#pragma unroll
        for (int r = 0; r < 8; ++r) sq[r] = granule2_load(srs, soff + 16u * r);
      }
    }
    RL_TS(4, 6);
    mac_lds<0, NK2>(sacc, wr, zh + lane);
    if (!last) {
      // (behind the rows' hand-over stores, see above; bounded like every wait of this kernel)
      for (unsigned spins = 0; __hip_atomic_load(&x_sent, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) < 4u && spins < WN_RELAY_SPINS; ++spins)
        __builtin_amdgcn_s_sleep(1);
      if (rok) {
        const __amdgpu_buffer_rsrc_t srs = __builtin_amdgcn_make_buffer_rsrc(sg_of(b + 1), 0, 65536, 0x00020000);
#pragma unroll
        for (int r = 0; r < 8; ++r) granule2_store(srs, (unsigned)(j * 64 + lane) * 128u + 16u * r, epoch, sacc[2 * r], sacc[2 * r + 1]);
      }
      RL_TS(4, 7);
    } else {
      skip_epilogue(a, sacc, j, h, row, rok, wmax);
    }
  }
  if (wave >= 4) store_zrow();                          // (last: nothing of waves 4..7 may sit in the memory queue before the rows' hand-over)
  if (a.guard && (wave < 4 || (skip_on && last))) {
    wmax = wn_wave_absmax_bits(wmax);
    if (lane == 0) wn_absmax_publish_any(a.guard, wmax);
  }
}

// floats of workspace the relay's granule areas take: [x | skip accumulator][block][tile][8192 granules]
int64_t wn_gen_relay128_floats(int B, int nblocks) { return (int64_t)2 * nblocks * ((B + 31) / 32) * 8192 * 2; }

// knob 24: phase stamps of the relay (profiling hook, read by wn_debug_relay_ts)
static unsigned long long* g_relay_ts = nullptr;
extern "C" int wn_debug_relay_ts(unsigned long long* out, int nblocks) {
  if (!g_relay_ts || nblocks > 128) return -1;
  return (int)hipMemcpy(out, g_relay_ts, (size_t)nblocks * 8 * 8, hipMemcpyDeviceToHost);
}

int wn_launch_gen_relay128(const WnGen128Args& a0, hipStream_t s) {
  WnGen128Args a = a0;
  a.ts = nullptr;
  a.mute_block = wn_debug_get(3) - 1;                  // knob 3 = b + 1: block b withholds its rows (watchdog test)
  if (wn_debug_get(24) && a.nblocks <= 128) {
    if (!g_relay_ts) { (void)hipMalloc((void**)&g_relay_ts, 128 * 8 * 8); (void)hipMemset(g_relay_ts, 0, 128 * 8 * 8); }
    a.ts = g_relay_ts;
  }
  if (a.B <= 0 || a.nblocks <= 0) return WN_OK;
  if (a.ntiles != (a.B + 31) / 32 || a.epoch == 0 || !a.tmo || a.relay_off < 0) { wn_set_error("gen_relay128: bad arguments"); return WN_E_INVALID; }
  hipLaunchKernelGGL(wn_gen_relay128_kernel, dim3((unsigned)(a.ntiles * a.nblocks)), dim3(512), 0, s, a);
  WN_HIP_CHECK(hipGetLastError());
  return WN_OK;
}

int wn_launch_gen_chain128(const WnGen128Args& a, hipStream_t s) {
  if (a.B <= 0 || a.nblocks <= 0) return WN_OK;
  hipLaunchKernelGGL(wn_gen_chain128_kernel, dim3((unsigned)((a.B + 31) / 32)), dim3(512), 0, s, a);
  WN_HIP_CHECK(hipGetLastError());
  return WN_OK;
}

int wn_gen_chain128_supported(int R, int D, int KS) { return R == 128 && D == 128 && KS == 2; }
