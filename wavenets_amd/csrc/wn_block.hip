// One residual block, forward and backward, on explicit pointers (WaveNetLayer.call, src/layers.py:178-224): shared by
// the model orchestration and by the standalone WaveNetLayer entry points at the end of this file.
#include "wn_plan_internal.h"

namespace wnp {

// the time split of one K x N weight-gradient product as wgrad() launches it (wn_layer_describe reads the same)
struct WgradSplit { int per_b, nsplit; };
static WgradSplit wgrad_split(int B, int T, int K, int N) {
  WgradSplit w;
  w.per_b = wn_wgrad_choose_splits(B, T, K, N);
  w.nsplit = B * w.per_b;
  return w;
}

// dW (+ optional db, + optional per-utterance column sums) through slabs
int wgrad(const float* x, int ldx, int K, int shift, const float* g, int ldg, int N, int B, int T,
          float* dW, float* db, float* per_batch, float* slab, hipStream_t s) {
  WnWgradArgs a;
  memset(&a, 0, sizeof(a));
  a.x = x; a.ldx = ldx; a.K = K; a.shift = shift; a.g = g; a.ldg = ldg; a.N = N; a.B = B; a.T = T;
  const WgradSplit w = wgrad_split(B, T, K, N);
  a.splits_per_b = w.per_b;
  const int nsplit = w.nsplit;
  a.slab = slab;
  a.slab_bias = (db || per_batch) ? slab + (int64_t)nsplit * K * N : nullptr;
  int rc = wn_launch_wgrad(a, s);
  if (rc) return rc;
  // per-utterance sums first: the reduces below fold the slabs in place
  if (per_batch) {
    rc = wn_launch_batch_reduce(a.slab_bias, B, a.splits_per_b, N, per_batch, s);
    if (rc) return rc;
  }
  if (dW) {
    WnReduceArgs r;
    memset(&r, 0, sizeof(r));
    r.slab = slab; r.nsplit = nsplit; r.K = K; r.N = N; r.out = dW; r.seg_len = K; r.seg_stride = 0;
    r.accumulate = 0; r.replicate = 1; r.rep_stride = 0;
    rc = wn_launch_reduce(r, s);
    if (rc) return rc;
  }
  if (db) {
    WnReduceArgs r;
    memset(&r, 0, sizeof(r));
    r.slab = a.slab_bias; r.nsplit = nsplit; r.K = 1; r.N = N; r.out = db; r.seg_len = 1; r.seg_stride = 0;
    r.accumulate = 0; r.replicate = 1; r.rep_stride = 0;
    rc = wn_launch_reduce(r, s);
    if (rc) return rc;
  }
  return rc;
}

// Which kernels block_forward(k, f) takes under knob 1 (launches nothing).  Every term stands as it stood in front of its
// launch.
BlockFwdPath block_fwd_path(const BlockPtrs& k, const BlockBufs& f) {
  BlockFwdPath p;
  const int64_t rows = (int64_t)k.B * k.T;
  int hc = k.Cin;
  if (f.pre_done && k.depth > 1) hc = k.D;
  for (int i = 0; i + 1 < k.depth && !f.pre_done; ++i) {
    const bool i16 = k.F16i[i] != nullptr;            // (training passes of deep stacks: split-precision, see deep16_ptrs)
    // 32 / 64 channels: the streamed kernel's second form with the taps as shifted planes (the rows GEMM for other widths)
    p.inner[i] = (i16 && k.JTi[i] == 2 && k.KS <= 4 && Planes::takes(true, k.D, hc, k.KS, hc, k.D, rows, {hc})) ? BLK_CONV_PLANES
                 : i16 ? BLK_CONV_ROWS16 : BLK_CONV_ROWS32;
    p.ninner = i + 1;
    hc = k.D;
  }
  // blocks too wide for LDS-resident weights (R = D = 128): one kernel that streams the fp16 hi|lo images through an LDS
  // ring and keeps u and z on chip (wn_layer16s.hip)
  if (k.F16n && k.F16r && k.depth == 1 && k.Cc == 0 && hc == k.R && k.Cin == k.R && f.ldz % 4 == 0 && wn_debug_get(1) != 1 &&
      wn_layer_fwd_s128_supported(k.R, k.D, k.KS) && (int64_t)rows * k.R * 4 < ((int64_t)1 << 32)) {
    // (also one block of a queued-generation step that no chain of wn_gen128.hip takes: T == 1 with the taps in f.xt[])
    p.gate = BLK_GATE_S128;
  } else if (k.F16g && k.F16r && k.Cc == 0 && !k.cb && !f.O && hc == k.R && f.ldz % 4 == 0 && wn_debug_get(1) != 1) {
    // wider blocks (or other kernel sizes) as [gated conv + gate] -> [1x1 + residual], two split-precision contractions,
    // ahead of the exact-fp32 one-kernel forward
    p.gate = BLK_GATE_TWO;
  } else if (k.fused && k.Cc == 0 && hc == k.R) {
    // knob 1 = 1 forces the exact-fp32 MFMA kernel
    p.gate = (k.F16d && k.F16r && wn_debug_get(1) != 1) ? BLK_GATE_FUSED16 : BLK_GATE_FUSED32;
  } else {
    p.gate = BLK_GATE_COMPOSED;
  }
  return p;
}

namespace {

// non-gated conv i of the stack: h [rows][hc] -> P[i] [rows][D]
int fwd_inner(const BlockPtrs& k, const BlockBufs& f, BlkConv path, int i, const float* h, int hc, hipStream_t s) {
  if (path == BLK_CONV_PLANES)
    return Planes(k.B, k.T, k.D).operand(h, hc, hc).taps(k.KS, k.dil[i]).w16(k.F16i[i]).bias(k.bd[i]).act(k.act).run(f.P[i], k.D, s);
  const bool i16 = path == BLK_CONV_ROWS16;
  Gemm g(k.B, k.T, k.D, i16 ? k.JTi[i] : ceil32(k.D));
  for (int t = 0; t < k.KS; ++t) g.seg(h, hc, hc, (k.KS - 1 - t) * k.dil[i], i16 ? nullptr : k.Fd[i] + t * k.Fd_stride[i]);
  if (i16) g.w16(k.F16i[i]);
  return g.bias(k.bd[i]).act(k.act).run(f.P[i], k.D, s);
}

// the one-kernel forms: everything of WnLayerFwdArgs but the two weight images and the third tap's rows
WnLayerFwdArgs layer_fwd_args(const BlockPtrs& k, const BlockBufs& f, const float* h) {
  const int li = k.depth - 1;
  WnLayerFwdArgs a;
  memset(&a, 0, sizeof(a));
  a.x = h;
  a.bias_d = k.bd[li]; a.bias_r = k.br; a.cb = k.cb; a.cb_frames = k.cb_frames; a.cb_hop = k.cb_hop;
  a.x_out = f.x_out; a.o_out = f.O; a.z_out = f.Z; a.ldz = f.ldz; a.ag_out = f.AG;
  a.res = f.res ? f.res : ((k.depth > 1) ? f.x : nullptr);   // (null: the residual is the conv input itself)
  a.xt[0] = f.xt[0]; a.xt[1] = f.xt[1];
  a.B = k.B; a.T = k.T; a.R = k.R; a.D = k.D; a.KS = k.KS; a.dilation = k.dil[li]; a.residual = k.residual;
  a.absmax_out = f.fwd_absmax;
  return a;
}

// streamed weights (depth 1, kernel size 2): wn_layer16s.hip
int fwd_streamed(const BlockPtrs& k, const BlockBufs& f, const float* h, hipStream_t s) {
  WnLayerFwdArgs a = layer_fwd_args(k, f, h);
  a.frag_d = k.F16n; a.frag_r = k.F16r;
  return wn_launch_layer_fwd_s128(a, s);
}

// LDS-resident weights: fp16 hi|lo images, or the exact-fp32 MFMA kernel on the fp32 fragments
int fwd_fused(const BlockPtrs& k, const BlockBufs& f, BlkGate gate, const float* h, hipStream_t s) {
  const bool use16 = gate == BLK_GATE_FUSED16;
  WnLayerFwdArgs a = layer_fwd_args(k, f, h);
  a.frag_d = use16 ? k.F16d : k.Fd[k.depth - 1]; a.frag_r = use16 ? k.F16r : k.Fr;
  a.xt[2] = f.xt[2];
  return use16 ? wn_launch_layer_fwd_f16(a, s) : wn_launch_layer_fwd(a, s);
}

// [gated conv + gate] -> [1x1 + residual] on the split-precision rows kernel
int fwd_two(const BlockPtrs& k, const BlockBufs& f, const float* h, int hc, hipStream_t s) {
  const int li = k.depth - 1;
  Gemm g(k.B, k.T, 2 * k.D, ceil32(2 * k.D));
  for (int t = 0; t < k.KS; ++t) {
    if (f.xt[t]) g.seg(f.xt[t], hc, hc, 0, nullptr);
    else g.seg(h, hc, hc, (k.KS - 1 - t) * k.dil[li], nullptr);
  }
  const int rc = g.bias(k.bd[li]).w16(k.F16g).gate_fwd(f.AG, k.D).run(f.Z, f.ldz, s);
  if (rc) return rc;
  Gemm r(k.B, k.T, k.R, ceil32(k.R));
  r.seg(f.Z, f.ldz, k.D, 0, k.Fr).bias(k.br).w16(k.F16r);
  if (k.residual) r.addc(f.res ? f.res : f.x, k.Cin);
  if (f.fwd_absmax) r.absmax_fwd(f.fwd_absmax);
  return r.run(f.x_out, k.R, s);
}

// u -> gate -> 1x1 in exact fp32
int fwd_composed(const BlockPtrs& k, const BlockBufs& f, const float* h, int hc, hipStream_t s) {
  const int64_t rows = (int64_t)k.B * k.T;
  const int li = k.depth - 1;
  int rc;
  {
    Gemm g(k.B, k.T, 2 * k.D, ceil32(2 * k.D));
    for (int t = 0; t < k.KS; ++t) {
      if (f.xt[t]) g.seg(f.xt[t], hc, hc, 0, k.Fd[li] + t * k.Fd_stride[li]);
      else g.seg(h, hc, hc, (k.KS - 1 - t) * k.dil[li], k.Fd[li] + t * k.Fd_stride[li]);
    }
    if (k.Cc > 0) g.seg(k.cond, k.Cc, k.Cc, 0, k.Fc);
    g.bias(k.bd[li]);
    if (k.cb) g.rowbias(k.cb, 2 * k.D, k.cb_frames, k.cb_hop);
    rc = g.run(f.U, 2 * k.D, s);
    if (rc) return rc;
  }
  rc = wn_launch_gate(f.U, rows, k.D, f.AG, f.Z, f.ldz, s);
  if (rc) return rc;
  {
    Gemm g(k.B, k.T, k.R, ceil32(k.R));
    g.seg(f.Z, f.ldz, k.D, 0, k.Fr).bias(k.br);
    if (f.O) {
      rc = g.run(f.O, k.R, s);
      if (rc) return rc;
      if (k.residual) return wn_launch_add(f.O, f.res ? f.res : f.x, f.x_out, rows * k.R, s);
      return hipMemcpyAsync(f.x_out, f.O, rows * k.R * sizeof(float), hipMemcpyDeviceToDevice, s) == hipSuccess ? WN_OK : WN_E_HIP;
    }
    if (k.residual) g.addc(f.res ? f.res : f.x, k.Cin);
    return g.run(f.x_out, k.R, s);
  }
}

}  // namespace

int block_forward(const BlockPtrs& k, const BlockBufs& f, hipStream_t s) {
  const BlockFwdPath p = block_fwd_path(k, f);
  const float* h = f.x;
  int hc = k.Cin;
  if (f.pre_done && k.depth > 1) { h = nullptr; hc = k.D; }
  for (int i = 0; i < p.ninner; ++i) {
    const int rc = fwd_inner(k, f, p.inner[i], i, h, hc, s);
    if (rc) return rc;
    h = f.P[i]; hc = k.D;
  }
  switch (p.gate) {
    case BLK_GATE_S128: return fwd_streamed(k, f, h, s);
    case BLK_GATE_TWO: return fwd_two(k, f, h, hc, s);
    case BLK_GATE_FUSED16: case BLK_GATE_FUSED32: return fwd_fused(k, f, p.gate, h, s);
    case BLK_GATE_COMPOSED: break;
  }
  return fwd_composed(k, f, h, hc, s);
}

namespace {

// gradient w.r.t. the conv1 output o
const float* go_ptr(BlkGo go, const BlockGrads& g) { return go == BLK_GO_XOUT ? g.g_xout : go == BLK_GO_SUM ? g.g_o_tmp : g.g_skip; }

const float* am_ptr(BlkAm a, const BlockGrads& g) {
  return a == BLK_AM_GXOUT ? g.am_gxout : a == BLK_AM_GSKIP ? g.am_gskip : a == BLK_AM_GFOLD ? g.am_gfold : nullptr;
}

}  // namespace

// Which kernels block_backward(k, f, g) takes (launches nothing).  Every term stands as it stood in front of its launch;
// knob 1 is not among them: an image chosen here goes to Gemm::run, which has that test.
BlockBwdPath block_bwd_path(const BlockPtrs& k, const BlockBufs&, const BlockGrads& g) {   // (no term reads the buffers today)
  BlockBwdPath p;
  const int64_t rows = (int64_t)k.B * k.T;
  const int li = k.depth - 1;
  if (k.S == 0 && g.g_skip) p.go = g.g_xout ? BLK_GO_SUM : BLK_GO_SKIP;
  const float* g_o = go_ptr(p.go, g);
  // g_u = gate'( W_r g_o + W_s g_skip ): the max-abs slots of its (up to) two operands
  const BlkAm s0 = (g_o == g.g_xout) ? BLK_AM_GXOUT : (g_o == g.g_skip ? BLK_AM_GSKIP : BLK_AM_GXOUT);
  const BlkAm s1 = (k.S > 0 || g_o == g.g_o_tmp) ? BLK_AM_GSKIP : BLK_AM_NONE;
  // (deep stacks in training: the [W_r | W_s] image may be padded to two row tiles; it is only set when it will be used)
  const bool full_u = (k.S > 0) ? (g_o && g.g_skip) : (g_o != nullptr);
  p.gu_pad = k.JTu > 0 && k.G16u && full_u && k.Cc == 0 && g.am_gu && am_ptr(s0, g) != nullptr;
  const bool use_fold = g.g_fold && g_o && k.G16uf && g.am_gu && g.am_gxout && g.am_gfold && k.Cc == 0;
  if (use_fold) {
    p.gu = BLK_GU_FOLD; p.gu_am[0] = BLK_AM_GXOUT; p.gu_am[1] = BLK_AM_GFOLD;
  } else if (!g_o && !(k.S > 0 && g.g_skip)) {
    p.gu = BLK_GU_ZERO;
  } else {
    // the [W_r | W_s] image matches the segment list only when both (or, for S == 0, the single) operands exist
    const bool full = (k.S > 0) ? (g_o && g.g_skip) : true;
    if (k.G16u && full && k.Cc == 0 && (k.JTu == 0 || p.gu_pad) && g.am_gu && am_ptr(s0, g)) {
      p.gu = p.gu_pad ? BLK_GU_PAD : BLK_GU_IMAGE; p.gu_am[0] = s0; p.gu_am[1] = s1;
    } else {
      p.gu = BLK_GU_FP32;     // (no image for this shape)
    }
  }
  // dilated stack, last (gated) conv first
  int gc = 2 * k.D;
  for (int i = li; i >= 0; --i) {
    const int hc = (i > 0) ? k.D : k.Cin;
    if (!((i > 0) || g.g_x)) break;
    // deep stacks in training: split-precision product, operand scaled by the running max-abs of gcur, the result's
    // max-abs published for the next product and for the weight-gradient jobs
    const float* am_cur = (i == li) ? g.am_gu : g.am_gp[i];
    const float* am_dst = (i > 0) ? g.am_gp[i - 1] : g.am_gx;
    const bool b16 = k.depth > 1 && k.G16i[i] && am_cur && am_dst;
    if (i > 0) {
      // inner convs (their output gradient gets act' folded in): the streamed kernel's second form, backward-data
      // instantiation with the taps as negatively shifted planes (the rows GEMM for other widths)
      p.data[i] = (b16 && k.JTb[i] == 2 && k.KS <= 4 && Planes::takes(true, hc, gc, k.KS, gc, hc, rows, {gc})) ? BLK_CONV_PLANES
                  : b16 ? BLK_CONV_ROWS16 : BLK_CONV_ROWS32;
      gc = k.D;
      continue;
    }
    p.drop = g.drop_rate > 0.f;
    // (under dropout the dropout kernel publishes g_x's max-abs: the products publish none and G16x does not ask for the slot)
    if (p.drop) p.gx = (k.G16x && k.depth == 1 && g.am_gu) ? BLK_GX_G16X : b16 ? BLK_GX_DEEP : BLK_GX_FP32;
    else p.gx = (k.G16x && k.depth == 1 && g.am_gu && g.am_gx) ? BLK_GX_G16X : b16 ? BLK_GX_DEEP : g.am_gx ? BLK_GX_FP32_ABSMAX : BLK_GX_FP32;
  }
  return p;
}

namespace {

// g_u = gate'( W_r g_o + W_s g_skip )
int bwd_gu(const BlockPtrs& k, const BlockBufs& f, const BlockGrads& g, const BlockBwdPath& p, const float* g_o, hipStream_t s) {
  if (p.gu == BLK_GU_ZERO) return wn_launch_fill(g.g_u, 0.f, (int64_t)k.B * k.T * 2 * k.D, s);
  const bool fold = p.gu == BLK_GU_FOLD;
  Gemm gm(k.B, k.T, k.D, p.gu_pad ? k.JTu : ceil32(k.D));
  if (g_o) gm.seg(g_o, k.R, k.R, 0, (fold || p.gu_pad) ? nullptr : k.Br_);
  if (fold) gm.seg(g.g_fold, g.fold_F0, g.fold_F0, 0, nullptr);
  else if (k.S > 0 && g.g_skip) gm.seg(g.g_skip, k.S, k.S, 0, p.gu_pad ? nullptr : k.Bs);
  // (exact fp32: the kernel still owes g_u's scale to the g_x product and the jobs)
  if (p.gu == BLK_GU_FP32) { if (g.am_gu) gm.absmax(nullptr, nullptr, g.am_gu); }
  else gm.w16(fold ? k.G16uf : k.G16u).absmax(am_ptr(p.gu_am[0], g), am_ptr(p.gu_am[1], g), g.am_gu);
  return gm.gate_bwd(f.AG, k.D, f.Z, f.ldz).run(g.g_u, 2 * k.D, s);
}

// conv1 / conv_skip weight gradients, and the time-varying condition's (standalone layer)
int bwd_block_wgrads(const BlockPtrs& k, const BlockBufs& f, const BlockGrads& g, const float* g_o, hipStream_t s) {
  int rc = WN_OK;
  if (g.defer) {
    // batched later; only the per-utterance column sums of g_u are needed now (conditioning)
    if (g.dcb) {
      rc = wn_launch_colsum_per_batch(g.g_u, k.B, k.T, 2 * k.D, g.dcb, g.slab, s);
      if (rc) return rc;
    }
  } else if (g_o) {
    rc = wgrad(f.Z, f.ldz, k.D, 0, g_o, k.R, k.R, k.B, k.T, g.dWr, g.dbr, nullptr, g.slab, s);
  } else {
    rc = wn_launch_fill(g.dWr, 0.f, (int64_t)k.D * k.R, s);
    if (!rc) rc = wn_launch_fill(g.dbr, 0.f, k.R, s);
  }
  if (rc) return rc;
  if (!g.defer && k.S > 0 && g.dWs) {
    if (g.g_skip) {
      rc = wgrad(f.Z, f.ldz, k.D, 0, g.g_skip, k.S, k.S, k.B, k.T, g.dWs, g.dbs, nullptr, g.slab, s);
    } else {
      rc = wn_launch_fill(g.dWs, 0.f, (int64_t)k.D * k.S, s);
      if (!rc) rc = wn_launch_fill(g.dbs, 0.f, k.S, s);
    }
    if (rc) return rc;
  }
  // time-varying condition (standalone layer)
  if (k.Cc > 0) {
    rc = wgrad(k.cond, k.Cc, k.Cc, 0, g.g_u, 2 * k.D, 2 * k.D, k.B, k.T, g.dWc, g.dbc, nullptr, g.slab, s);
    if (rc) return rc;
    if (g.g_cond) {
      rc = Gemm(k.B, k.T, k.Cc, ceil32(k.Cc)).seg(g.g_u, 2 * k.D, 2 * k.D, 0, k.Bc).run(g.g_cond, k.Cc, s);
      if (rc) return rc;
    }
  }
  return WN_OK;
}

// backward data of conv i >= 1: gcur [rows][gc] -> dst, the gradient at conv i - 1's pre-activation output (act' folded in)
int bwd_inner(const BlockPtrs& k, const BlockBufs& f, const BlockGrads& g, BlkConv path, int i, const float* gcur, int gc,
              float* dst, hipStream_t s) {
  // deep stacks in training: split-precision product, operand scaled by the running max-abs of gcur, the result's
  // max-abs published for the next product and for the weight-gradient jobs
  const float* am_cur = (i == k.depth - 1) ? g.am_gu : g.am_gp[i];
  float* am_dst = g.am_gp[i - 1];
  if (path == BLK_CONV_PLANES)
    return Planes(k.B, k.T, k.D).operand(gcur, gc, gc).taps(k.KS, -k.dil[i]).w16(k.G16i[i]).act(k.act)
        .bwd(am_cur, am_dst, f.P[i - 1], k.D).run(dst, k.D, s);
  const bool b16 = path == BLK_CONV_ROWS16;
  Gemm gm(k.B, k.T, k.D, b16 ? k.JTb[i] : ceil32(k.D));
  for (int t = 0; t < k.KS; ++t)
    gm.seg(gcur, gc, gc, -(k.KS - 1 - t) * k.dil[i], b16 ? nullptr : k.Bd[i] + t * k.Bd_stride[i]);
  if (b16) gm.w16(k.G16i[i]).absmax(am_cur, nullptr, am_dst);
  return gm.dact(f.P[i - 1], k.D, k.act).run(dst, k.D, s);
}

// backward data of conv 0: gcur [rows][gc] -> g_x (+ the residual path); under dropout the conv-path gradient first, then
// the keep-mask, then the (unmasked) residual path, and the dropout kernel publishes g_x's max-abs
int bwd_gx(const BlockPtrs& k, const BlockGrads& g, const BlockBwdPath& p, const float* gcur, int gc, hipStream_t s) {
  const int hc = k.Cin;
  const bool b16 = p.gx == BLK_GX_DEEP;
  const float* am_cur = (k.depth == 1) ? g.am_gu : g.am_gp[0];
  float* am_out = p.drop ? nullptr : g.am_gx;
  Gemm gm(k.B, k.T, hc, b16 ? k.JTb[0] : ceil32(hc));
  for (int t = 0; t < k.KS; ++t)
    gm.seg(gcur, gc, gc, -(k.KS - 1 - t) * k.dil[0], b16 ? nullptr : k.Bd[0] + t * k.Bd_stride[0]);
  if (!p.drop && k.residual && g.g_xout) gm.addc(g.g_xout, k.R);
  switch (p.gx) {
    case BLK_GX_G16X: gm.w16(k.G16x).absmax(g.am_gu, nullptr, am_out); break;
    case BLK_GX_DEEP: gm.w16(k.G16i[0]).absmax(am_cur, nullptr, am_out); break;
    case BLK_GX_FP32_ABSMAX: gm.absmax(nullptr, nullptr, g.am_gx); break;   // (the next block's g_u product reads it)
    case BLK_GX_FP32: case BLK_GX_NONE: break;
  }
  if (!p.drop) return gm.run(g.g_x, hc, s);
  const int rc = gm.run(g.g_xd, hc, s);
  if (rc) return rc;
  return wn_launch_dropout(g.g_xd, (k.residual && g.g_xout) ? g.g_xout : nullptr, g.g_x, (int64_t)k.B * k.T * hc, g.drop_rate,
                           g.drop_key, g.am_gx, s);
}

}  // namespace

int block_backward(const BlockPtrs& k, const BlockBufs& f, const BlockGrads& g, hipStream_t s) {
  const BlockBwdPath p = block_bwd_path(k, f, g);
  const int64_t rows = (int64_t)k.B * k.T;
  const int li = k.depth - 1;
  int rc;
  const float* g_o = go_ptr(p.go, g);
  if (p.go == BLK_GO_SUM && (rc = wn_launch_add(g.g_xout, g.g_skip, g.g_o_tmp, rows * k.R, s))) return rc;
  if ((rc = bwd_gu(k, f, g, p, g_o, s))) return rc;
  if ((rc = bwd_block_wgrads(k, f, g, g_o, s))) return rc;
  // dilated stack, last (gated) conv first
  const float* gcur = g.g_u;       // gradient w.r.t. the pre-activation output of conv i
  int gc = 2 * k.D;
  for (int i = li; i >= 0; --i) {
    const float* hin = (i > 0) ? f.P[i - 1] : f.x;
    const int hc = (i > 0) ? k.D : k.Cin;
    for (int t = 0; t < k.KS && !g.defer; ++t) {
      const bool last_tap = (t == k.KS - 1);
      rc = wgrad(hin, hc, hc, (k.KS - 1 - t) * k.dil[i], gcur, gc, gc, k.B, k.T,
                 g.dWd[i] + (int64_t)t * hc * gc, last_tap ? g.dbd[i] : nullptr,
                 (last_tap && i == li) ? g.dcb : nullptr, g.slab, s);
      if (rc) return rc;
    }
    if (i == 0) return p.gx == BLK_GX_NONE ? WN_OK : bwd_gx(k, g, p, gcur, gc, s);
    // where the gradient at conv i - 1's output goes: kept for the deferred weight gradients, or a half of g_p
    float* dst = g.g_pi[i - 1] ? g.g_pi[i - 1] : g.g_p + (int64_t)((i & 1) ? 0 : rows * k.D);
    if ((rc = bwd_inner(k, f, g, p.data[i], i, gcur, gc, dst, s))) return rc;
    gcur = dst; gc = k.D;
  }
  return WN_OK;
}

}  // namespace wnp

using namespace wnp;

// ==========================================================================================
// standalone residual block: WaveNetLayer.call, src/layers.py:178-224
// ==========================================================================================
namespace {

struct LayerLayout {
  // parameter offsets (floats) inside the layer's flat parameter buffer (Keras order)
  int64_t Wd[16], bd[16], Wr, br, Ws, bs, Wc, bc, nparams;
  int cin[16], cout[16];
  // workspace
  int64_t Fd[16], Bd[16], Fd_stride[16], Bd_stride[16], Fr, Br, Bs, Fs, Fc, Bc;
  int64_t bias_u, U, O, g_u, g_o, g_p, slab, ws_total;
  int64_t F16d, F16r;   // fp16 split images (or -1)
  // saved
  int64_t sP[16], sAG, sZ, saved_total;
};

int layer_layout(const wn_layer_desc* d, int B, int T, LayerLayout& L) {
  if (!d || d->depth < 1 || d->depth > 16 || d->kernel_size < 2 || d->kernel_size > 3 || d->channels < 1) {
    wn_set_error("layer: bad descriptor"); return WN_E_INVALID;
  }
  const int KS = d->kernel_size, R = d->channels, D = d->dilation_channels > 0 ? d->dilation_channels : R;
  const int S = d->skip_channels, Cc = d->cond_channels;
  const int64_t rows = (int64_t)B * T;
  int64_t o = 0;
  int cin = d->in_channels > 0 ? d->in_channels : R;
  for (int i = 0; i < d->depth; ++i) {
    const int cout = (i == d->depth - 1) ? 2 * D : D;
    L.cin[i] = cin; L.cout[i] = cout;
    L.Wd[i] = o; o += (int64_t)KS * cin * cout;
    L.bd[i] = o; o += cout;
    cin = cout;
  }
  L.Wr = o; o += (int64_t)D * R; L.br = o; o += R;
  L.Ws = L.bs = L.Wc = L.bc = -1;
  if (S > 0) { L.Ws = o; o += (int64_t)D * S; L.bs = o; o += S; }
  if (Cc > 0) { L.Wc = o; o += (int64_t)Cc * 2 * D; L.bc = o; o += 2 * D; }
  L.nparams = o;
  Carver cv;
  for (int i = 0; i < d->depth; ++i) {
    L.Fd_stride[i] = (int64_t)wn_frag_floats(L.cout[i], L.cin[i]);
    L.Bd_stride[i] = (int64_t)wn_frag_floats(L.cin[i], L.cout[i]);
    L.Fd[i] = cv.take(KS * L.Fd_stride[i]);
    L.Bd[i] = cv.take(KS * L.Bd_stride[i]);
  }
  L.Fr = cv.take((int64_t)wn_frag_floats(R, D));
  L.Br = cv.take((int64_t)wn_frag_floats(D, R));
  L.Fs = cv.take(S > 0 ? (int64_t)wn_frag_floats(S, D) : 0);
  L.Bs = cv.take(S > 0 ? (int64_t)wn_frag_floats(D, S) : 0);
  L.Fc = cv.take(Cc > 0 ? (int64_t)wn_frag_floats(2 * D, Cc) : 0);
  L.Bc = cv.take(Cc > 0 ? (int64_t)wn_frag_floats(Cc, 2 * D) : 0);
  L.F16d = L.F16r = -1;
  if (d->depth == 1 && Cc == 0 && cin == 2 * D && (d->in_channels > 0 ? d->in_channels : R) == R &&
      ((wn_layer_fwd_supported(R, D, KS) && wn_layer_fwd_f16_supported(R, D, KS)) || wn_layer_fwd_s128_supported(R, D, KS))) {
    L.F16d = cv.take((int64_t)wn_frag16_floats(2 * D, KS * R));
    L.F16r = cv.take((int64_t)wn_frag16_floats(R, D));
  }
  L.bias_u = cv.take(2 * D);
  L.U = cv.take(rows * 2 * D);
  L.O = cv.take(rows * R);
  L.g_u = L.U;                     // backward reuses the u scratch
  L.g_o = L.O;
  L.g_p = cv.take(d->depth > 1 ? 2 * rows * D : 0);
  int64_t need = 0;
  if (B > 0 && T > 0) {
    for (int i = 0; i < d->depth; ++i) need = std::max(need, slab_need(B, T, L.cin[i], L.cout[i]));
    need = std::max(need, slab_need(B, T, D, R));
    if (S > 0) need = std::max(need, slab_need(B, T, D, S));
    if (Cc > 0) need = std::max(need, slab_need(B, T, Cc, 2 * D));
  }
  L.slab = cv.take(need);
  L.ws_total = cv.pos;
  Carver sv;
  for (int i = 0; i + 1 < d->depth; ++i) L.sP[i] = sv.take(rows * D);
  L.sAG = sv.take(rows * D);
  L.sZ = sv.take(rows * D);
  L.saved_total = sv.pos;
  return WN_OK;
}

int layer_prep(const wn_layer_desc* d, const LayerLayout& L, const float* params, float* ws, hipStream_t s) {
  const int KS = d->kernel_size, R = d->channels, D = d->dilation_channels > 0 ? d->dilation_channels : R;
  const int S = d->skip_channels, Cc = d->cond_channels;
  auto one = [&](int64_t src, int64_t dst, int I, int KK, int ld, int tr) {
    WnPrepDesc pd;
    memset(&pd, 0, sizeof(pd));
    pd.src_off = src; pd.dst_off = dst; pd.I = I; pd.KK = KK; pd.ld = ld; pd.transpose = tr;
    pd.JT = (I + 31) / 32;
    return wn_launch_prep_one(pd, params, ws, s);
  };
  int rc;
  for (int i = 0; i < d->depth; ++i)
    for (int t = 0; t < KS; ++t) {
      const int64_t src = L.Wd[i] + (int64_t)t * L.cin[i] * L.cout[i];
      if ((rc = one(src, L.Fd[i] + t * L.Fd_stride[i], L.cout[i], L.cin[i], L.cout[i], 1))) return rc;
      if ((rc = one(src, L.Bd[i] + t * L.Bd_stride[i], L.cin[i], L.cout[i], L.cout[i], 0))) return rc;
    }
  if ((rc = one(L.Wr, L.Fr, R, D, R, 1))) return rc;
  if ((rc = one(L.Wr, L.Br, D, R, R, 0))) return rc;
  if (L.F16d >= 0) {
    for (int t = 0; t < KS; ++t) {
      WnPrepDesc pd;
      memset(&pd, 0, sizeof(pd));
      pd.src_off = L.Wd[0] + (int64_t)t * R * 2 * D; pd.dst_off = L.F16d; pd.I = 2 * D; pd.KK = R; pd.ld = 2 * D;
      pd.transpose = 1; pd.q_off = t * (R / 16); pd.JT = (2 * D + 31) / 32; pd.kind = 1;
      if ((rc = wn_launch_prep_one(pd, params, ws, s))) return rc;
    }
    WnPrepDesc pd;
    memset(&pd, 0, sizeof(pd));
    pd.src_off = L.Wr; pd.dst_off = L.F16r; pd.I = R; pd.KK = D; pd.ld = R; pd.transpose = 1; pd.JT = (R + 31) / 32; pd.kind = 1;
    if ((rc = wn_launch_prep_one(pd, params, ws, s))) return rc;
  }
  if (S > 0) {
    if ((rc = one(L.Ws, L.Fs, S, D, S, 1))) return rc;
    if ((rc = one(L.Ws, L.Bs, D, S, S, 0))) return rc;
  }
  if (Cc > 0) {
    if ((rc = one(L.Wc, L.Fc, 2 * D, Cc, 2 * D, 1))) return rc;
    if ((rc = one(L.Wc, L.Bc, Cc, 2 * D, 2 * D, 0))) return rc;
    // u's bias = last dilated conv bias + conv_cond bias (src/layers.py:82-88,116-120,203-204)
    WnVecSumArgs v;
    v.base = params; v.off0 = L.bd[d->depth - 1]; v.stride = L.bc - L.bd[d->depth - 1]; v.count = 2; v.len = 2 * D;
    v.out = ws + L.bias_u;
    if ((rc = wn_launch_vecsum(v, s))) return rc;
  }
  return WN_OK;
}

void layer_ptrs(const wn_layer_desc* d, const LayerLayout& L, const float* params, const float* ws,
                const float* cond, int B, int T, BlockPtrs& k) {
  memset(&k, 0, sizeof(k));
  const int R = d->channels, D = d->dilation_channels > 0 ? d->dilation_channels : R;
  k.B = B; k.T = T; k.KS = d->kernel_size; k.R = R; k.D = D; k.S = d->skip_channels;
  k.Cin = d->in_channels > 0 ? d->in_channels : R; k.depth = d->depth; k.act = d->activation; k.residual = d->residual;
  for (int i = 0; i < d->depth; ++i) {
    k.dil[i] = d->dilations[i];
    k.Wd[i] = params + L.Wd[i]; k.bd[i] = params + L.bd[i];
    k.Fd[i] = ws + L.Fd[i]; k.Bd[i] = ws + L.Bd[i]; k.Fd_stride[i] = L.Fd_stride[i]; k.Bd_stride[i] = L.Bd_stride[i];
  }
  k.br = params + L.br; k.Fr = ws + L.Fr; k.Br_ = ws + L.Br;
  if (d->skip_channels > 0) { k.bs = params + L.bs; k.Fs = ws + L.Fs; k.Bs = ws + L.Bs; }
  k.Cc = d->cond_channels; k.cond = cond; k.cb = nullptr;
  if (k.Cc > 0) { k.Fc = ws + L.Fc; k.Bc = ws + L.Bc; k.bc = params + L.bc; k.bd[d->depth - 1] = ws + L.bias_u; }
  k.fused = wn_layer_fwd_supported(R, D, d->kernel_size) != 0;
  if (L.F16d >= 0) {
    // (the natural-order image serves the LDS-resident kernel or, for 128 channels, the streamed one)
    if (wn_layer_fwd_f16_supported(R, D, d->kernel_size)) k.F16d = ws + L.F16d; else k.F16n = ws + L.F16d;
    k.F16r = ws + L.F16r;
  }
}

// the layer's input and its saved buffer (stack activations, sigmoid, z): what wn_layer_fwd writes and wn_layer_bwd reads
BlockBufs layer_bufs(const wn_layer_desc* d, const LayerLayout& L, const float* x, float* saved) {
  BlockBufs f;
  memset(&f, 0, sizeof(f));
  f.x = x;
  for (int i = 0; i + 1 < d->depth; ++i) f.P[i] = saved + L.sP[i];
  f.AG = saved + L.sAG;
  f.Z = saved + L.sZ; f.ldz = d->dilation_channels > 0 ? d->dilation_channels : d->channels;
  return f;
}

}  // namespace

extern "C" int64_t wn_layer_param_count(const wn_layer_desc* d) {
  LayerLayout L;
  if (layer_layout(d, 0, 0, L)) return -1;
  return L.nparams;
}
extern "C" int64_t wn_layer_saved_floats(const wn_layer_desc* d, int32_t B, int32_t T) {
  LayerLayout L;
  if (layer_layout(d, B, T, L)) return -1;
  return L.saved_total;
}
extern "C" int64_t wn_layer_workspace_floats(const wn_layer_desc* d, int32_t B, int32_t T) {
  LayerLayout L;
  if (layer_layout(d, B, T, L)) return -1;
  return L.ws_total;
}

// The weight-gradient products of wn_layer_bwd over (B, T) and how each is split over time and reduced: the products in
// the order block_backward launches them, K and N as it passes them to wgrad(), the split from wgrad_split() and the
// reduce form from wn_reduce_two_stage() -- the functions the launches themselves read (host only).
extern "C" int wn_layer_describe(const wn_layer_desc* d, int32_t B, int32_t T, char* buf, int32_t len) {
  if (!buf || len < 1) { wn_set_error("layer_describe: no buffer"); return WN_E_INVALID; }
  buf[0] = 0;
  if (B < 1 || T < 1) { wn_set_error("layer_describe: B and T must be at least 1"); return WN_E_INVALID; }
  LayerLayout L;
  int rc = layer_layout(d, B, T, L);
  if (rc) return rc;
  const int R = d->channels, D = d->dilation_channels > 0 ? d->dilation_channels : R;
  std::string out;
  auto add = [&](const std::string& name, int K, int N) {
    const WgradSplit w = wgrad_split(B, T, K, N);
    char item[160];
    snprintf(item, sizeof(item), "%s%s K=%d N=%d splits=%d nsplit=%d reduce=%s", out.empty() ? "" : " | ", name.c_str(), K, N,
             w.per_b, w.nsplit, wn_reduce_two_stage(w.nsplit) ? "two-stage" : "one-stage");
    out += item;
  };
  add("conv1", D, R);
  if (d->skip_channels > 0) add("conv_skip", D, d->skip_channels);
  if (d->cond_channels > 0) add("conv_cond", d->cond_channels, 2 * D);
  for (int i = d->depth - 1; i >= 0; --i)
    for (int t = 0; t < d->kernel_size; ++t) add("dil" + std::to_string(i) + ".tap" + std::to_string(t), L.cin[i], L.cout[i]);
  snprintf(buf, (size_t)len, "%s", out.c_str());
  if ((int64_t)out.size() + 1 > (int64_t)len) {
    wn_set_error("layer_describe: the line needs %d bytes, the buffer has %d", (int)out.size() + 1, (int)len);
    return WN_E_INVALID;
  }
  return WN_OK;
}

extern "C" int wn_layer_fwd(const wn_layer_desc* d, const float* params, const float* x, const float* cond,
                            int32_t B, int32_t T, float* x_out, float* skip_out, float* saved,
                            float* workspace, void* stream) {
  LayerLayout L;
  int rc = layer_layout(d, B, T, L);
  if (rc) return rc;
  if (!params || !x || !x_out || !workspace) { wn_set_error("layer_fwd: null pointer"); return WN_E_INVALID; }
  if (d->cond_channels > 0 && !cond) { wn_set_error("layer_fwd: condition tensor missing"); return WN_E_INVALID; }
  if (d->residual && (d->in_channels > 0 ? d->in_channels : d->channels) != d->channels) {
    wn_set_error("Residual connection must have the same shape as input"); return WN_E_INVALID;   // src/layers.py:161-162
  }
  hipStream_t s = (hipStream_t)stream;
  if ((rc = layer_prep(d, L, params, workspace, s))) return rc;
  BlockPtrs k;
  layer_ptrs(d, L, params, workspace, cond, B, T, k);
  const int D = k.D;
  if (!saved) { wn_set_error("layer_fwd: saved buffer is required (holds z and the stack activations)"); return WN_E_INVALID; }
  BlockBufs f = layer_bufs(d, L, x, saved);
  f.U = workspace + L.U;
  const bool skip_is_o = (d->skip_channels == 0);
  f.O = (skip_is_o && skip_out) ? skip_out : nullptr;
  f.x_out = x_out;
  if ((rc = block_forward(k, f, s))) return rc;
  if (!skip_is_o && skip_out) {
    rc = Gemm(B, T, d->skip_channels, ceil32(d->skip_channels)).seg(f.Z, D, D, 0, k.Fs).bias(k.bs).run(skip_out, d->skip_channels, s);
  }
  return rc;
}

extern "C" int wn_layer_bwd(const wn_layer_desc* d, const float* params, const float* x, const float* cond,
                            const float* saved, const float* g_x_out, const float* g_skip, int32_t B, int32_t T,
                            float* g_x, float* g_cond, float* g_params, float* workspace, void* stream) {
  LayerLayout L;
  int rc = layer_layout(d, B, T, L);
  if (rc) return rc;
  if (!params || !x || !saved || !g_params || !workspace) { wn_set_error("layer_bwd: null pointer"); return WN_E_INVALID; }
  hipStream_t s = (hipStream_t)stream;
  if ((rc = layer_prep(d, L, params, workspace, s))) return rc;
  BlockPtrs k;
  layer_ptrs(d, L, params, workspace, cond, B, T, k);
  const BlockBufs f = layer_bufs(d, L, x, const_cast<float*>(saved));
  BlockGrads g;
  memset(&g, 0, sizeof(g));
  g.g_xout = g_x_out; g.g_skip = g_skip; g.g_o_tmp = workspace + L.g_o; g.g_u = workspace + L.g_u;
  g.g_p = workspace + L.g_p; g.g_x = g_x; g.g_cond = g_cond;
  for (int i = 0; i < d->depth; ++i) { g.dWd[i] = g_params + L.Wd[i]; g.dbd[i] = g_params + L.bd[i]; }
  g.dWr = g_params + L.Wr; g.dbr = g_params + L.br;
  if (d->skip_channels > 0) { g.dWs = g_params + L.Ws; g.dbs = g_params + L.bs; }
  if (d->cond_channels > 0) { g.dWc = g_params + L.Wc; g.dbc = g_params + L.bc; }
  g.slab = workspace + L.slab;
  return block_backward(k, f, g, s);
}
