// The model's forward pass and loss: WaveNet.call src/model.py:213-239, loss_fn :505-551, test_step's loss :362-381.
#include "wn_plan_internal.h"

namespace {

__global__ void wn_ring_capture_kernel(const float* src, int B, int T, int C, int nslots, float* ring, int64_t t0) {
  // ring[((t + t0) % nslots)][b][c] = src[b][t][c] for the last nslots time steps (t0: the time of src's index 0)
  const int64_t n = (int64_t)nslots * B * C;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int c = (int)(i % C);
    const int b = (int)((i / C) % B);
    const int k = (int)(i / ((int64_t)C * B));
    const int t = T - nslots + k;
    if (t >= 0) ring[((int64_t)((t + t0) % nslots) * B + b) * C + c] = src[((int64_t)b * T + t) * C + c];
  }
}

__global__ void wn_shift_split_kernel(const float* x_full, int B, int T, float* inputs, float* y_true) {
  const int64_t n = (int64_t)B * T;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t b = i / T, t = i % T;
    inputs[i] = x_full[b * (T + 1) + t];        // x[:, :-1]   src/model.py:321
    y_true[i] = x_full[b * (T + 1) + t + 1];    // x[:, 1:]    src/model.py:319
  }
}

}  // namespace

namespace wnp {

BlockPtrs block_ptrs(const wn_plan* p, int b, const float* params, const float* fragbase, int B, int T) {
  BlockPtrs k;
  memset(&k, 0, sizeof(k));
  const BlockInfo& bi = p->blocks[b];
  k.B = B; k.T = T; k.KS = p->KS; k.R = p->R; k.D = p->D; k.S = p->S; k.Cin = p->R; k.depth = p->LPB;
  k.act = p->c.activation; k.residual = p->c.use_residual;
  for (int i = 0; i < p->LPB; ++i) {
    const ConvInfo& c = bi.dil[i];
    k.dil[i] = c.dil;
    k.Wd[i] = params + p->tensors[c.kernel_t].off;
    k.bd[i] = params + p->tensors[c.bias_t].off;
    k.Fd[i] = fragbase + c.fragF; k.Fd_stride[i] = c.fragF_stride;
    k.Bd[i] = fragbase + c.fragB; k.Bd_stride[i] = c.fragB_stride;
  }
  k.br = params + p->tensors[bi.conv1.bias_t].off;
  k.Fr = fragbase + bi.conv1.fragF; k.Br_ = fragbase + bi.conv1.fragB;
  if (bi.has_skip) { k.bs = params + p->tensors[bi.conv_skip.bias_t].off; k.Bs = fragbase + bi.conv_skip.fragB; }
  k.Cc = 0; k.cond = nullptr; k.cb = nullptr;
  k.fused = p->fused_ok;
  if (p->fused16_ok && p->LPB == 1) { k.F16d = fragbase + bi.dil.back().frag16; k.F16r = fragbase + bi.conv1.frag16; }
  if (bi.f16gate >= 0) { k.F16g = fragbase + bi.f16gate; k.F16r = fragbase + bi.conv1.frag16; }
  if (bi.f16nat >= 0) k.F16n = fragbase + bi.f16nat;
  if (bi.g16u >= 0 && p->LPB == 1) k.G16u = fragbase + bi.g16u;
  if (bi.g16uf >= 0) k.G16uf = fragbase + bi.g16uf;
  if (p->LPB == 1 && bi.dil[0].frag16B >= 0) k.G16x = fragbase + bi.dil[0].frag16B;
  return k;
}

void deep16_ptrs(const wn_plan* p, int b, const float* fragbase, BlockPtrs& k) {
  if (!deep16(p)) return;
  const BlockInfo& bi = p->blocks[b];
  k.F16d = fragbase + bi.dil.back().frag16; k.F16r = fragbase + bi.conv1.frag16;
  for (int i = 0; i < p->LPB; ++i) {
    const ConvInfo& c = bi.dil[i];
    if (bi.d16F[i] >= 0) { k.F16i[i] = fragbase + bi.d16F[i]; k.JTi[i] = std::max(2, ceil32(c.cout)); }
    if (bi.d16B[i] >= 0) { k.G16i[i] = fragbase + bi.d16B[i]; k.JTb[i] = std::max(2, ceil32(c.cin)); }
  }
  if (bi.g16u >= 0) { k.G16u = fragbase + bi.g16u; k.JTu = std::max(2, ceil32(p->D)); }
}

BlockBufs block_bufs(const wn_plan* p, const WsLayout& L, float* ws, int b, int64_t rows, bool training, bool drop) {
  BlockBufs f;
  memset(&f, 0, sizeof(f));
  float* hin = ws + L.H[training ? b : (b & 1)];
  f.x = hin;
  // x = dropout(x) feeds the dilated stack; the residual keeps the original (src/layers.py:192-196)
  if (drop) { f.x = ws + L.XD[b]; f.res = hin; }
  for (int i = 0; i + 1 < p->LPB; ++i) f.P[i] = ws + L.P[b][i];
  f.AG = training ? ws + L.AG[b] : nullptr;
  f.Z = ws + L.Z + (int64_t)b * rows * p->Dp; f.ldz = p->Dp;      // block-major [N][rows][Dp]
  return f;
}

int ring_capture(const float* src, int B, int T, int C, int nslots, float* ring, int64_t t0, hipStream_t s) {
  const int64_t n = (int64_t)nslots * B * C;
  hipLaunchKernelGGL(wn_ring_capture_kernel, dim3((unsigned)std::min<int64_t>((n + 255) / 256, 4096)), dim3(256), 0, s,
                     src, B, T, C, nslots, ring, t0);
  WN_HIP_CHECK(hipGetLastError());
  return WN_OK;
}

// ------------------------------------------------------------------------------------------
// One forward pass: the calling thread's execution state, the caller's buffers, the workspace layout and the kernel paths
// of the call (fwd_paths, wn_plan.hip); its phases are the member functions, in launch order.
// ------------------------------------------------------------------------------------------
struct FwdCall {
  wn_exec& e;
  wn_plan* p; const float* params; const float* x; const float* cond; int B, T; bool training, prep;
  float* ws; const WsLayout& L; hipStream_t s; const GenRings* rings; LossFuse* lf;
  int64_t rows; float* fragbase;
  int F, hop, Bc;                    // condition frames per utterance (1: global), inputs per frame, condition rows B * F
  // Forward range guard.  The split-precision kernels cast fp32 activations to fp16 hi|lo unscaled: beyond 65504 the
  // hi part is inf.  Every kernel that produces an input of such a kernel -- the residual stream H[b], the skip sum,
  // the head activations (z is bounded by 1) -- publishes its running max-abs here; the callers turn it into a flag
  // (WN_RANGE_LIMIT) and redo the pass with the exact-fp32 kernels when it tripped.
  float* fam;
  FwdPaths fp;
  bool stack_prof = false;           // an event pair around the stack is open (blocks() -> skip())
  const float* hin = nullptr;        // the head's input rows (skip() -> head())

  FwdCall(wn_plan* p_, const float* params_, const float* x_, bool prep_, const float* cond_, int B_, int T_, bool training_,
          float* ws_, const WsLayout& L_, hipStream_t s_, const GenRings* rings_, LossFuse* lf_)
      : e(wnp::ex(p_)), p(p_), params(params_), x(x_), cond(cond_), B(B_), T(T_), training(training_), prep(prep_), ws(ws_),
        L(L_), s(s_), rings(rings_), lf(lf_), rows((int64_t)B_ * T_), fragbase(ws_ + L_.frag), F(L_.frames), hop(T_ / L_.frames),
        Bc(B_ * L_.frames), fam(ws_ + L_.fwd_absmax),
        fp(fwd_paths(p_, e, B_, T_, training_, prep_, rings_ != nullptr, !lf_ ? FWD_LOSS_NONE : lf_->eval ? FWD_LOSS_EVAL : FWD_LOSS_TRAIN)) {}

  const float* par(int tensor) const { return params + p->tensors[tensor].off; }

  // The timing hooks bench.py reads: (start, stop) event pairs out of the calling state's pools, recorded on `sp` at the
  // points they always were.  A stop takes the pair.
  static bool pair_free(const std::vector<hipEvent_t>& ev, int used) { return used + 2 <= (int)ev.size(); }
  static void mark(const std::vector<hipEvent_t>& ev, int& used, bool stop, hipStream_t sp) {
    (void)hipEventRecord(ev[used + (stop ? 1 : 0)], sp);
    if (stop) used += 2;
  }

  int weight_images() {
    return prep ? wn_launch_prep_table(p->d_prep, (int)p->prep.size(), params, fragbase, s) : WN_OK;
  }

  // The weight-space preparation of the skip path (bias sum, V = W_s W_f0, its fp16 images: ~45 us of small launches) is
  // only needed by the folded contraction at the END of the block chain.  With the side stream allowed (knob 9 = 0) it is
  // forked off right where the stack begins (the stack's start event in blocks()) and runs beside the first blocks; the
  // contraction waits for it.  Otherwise it runs on the caller's stream, ahead of the conditioning.
  int fold_prep(hipStream_t sp) {
    const bool fp_prof = fp.fold && pair_free(e.foldprep_ev, e.foldprep_used);
    if (fp_prof) mark(e.foldprep_ev, e.foldprep_used, false, sp);
    // bias of the folded skip sum = sum over blocks of conv_skip (or conv1) biases
    if (p->c.use_skip) {
      const ConvInfo& c0 = p->blocks[0].has_skip ? p->blocks[0].conv_skip : p->blocks[0].conv1;
      WnVecSumArgs v;
      v.base = params; v.off0 = p->tensors[c0.bias_t].off;
      v.stride = p->N > 1 ? (p->tensors[(p->blocks[1].has_skip ? p->blocks[1].conv_skip : p->blocks[1].conv1).bias_t].off - v.off0) : 0;
      v.count = p->N; v.len = p->Sh; v.out = ws + L.bias_sum;
      const int r = wn_launch_vecsum(v, sp);
      if (r) return r;
    }
    // (inference and the generation priming pass fold too: the queued sampler carries the folded contraction in its chain
    // kernel and must reproduce the sliding window bit for bit)
    if (fp.fold) {
      const BlockInfo& b0 = p->blocks[0];
      const int64_t wst = p->N > 1 ? p->tensors[p->blocks[1].conv_skip.kernel_t].off - p->tensors[b0.conv_skip.kernel_t].off : 0;
      int r = wn_launch_skip_fold(params, p->tensors[b0.conv_skip.kernel_t].off, wst, p->tensors[p->finals[0].kernel_t].off,
                                  p->tensors[p->finals[0].bias_t].off, ws + L.bias_sum, p->N, p->D, p->S, p->fold_F0, ws + L.vfold,
                                  ws + L.bfold, ws + L.wsall, sp);
      if (r) return r;
      r = wn_launch_prep_table(p->d_prep2, (int)p->prep2.size(), ws, fragbase, sp, 64);  // sources relative to the workspace
      if (r) return r;
    }
    if (fp_prof) mark(e.foldprep_ev, e.foldprep_used, true, sp);
    return WN_OK;
  }

  // ... on the side stream, behind whatever wrote the parameters
  int fold_prep_fork() {
    if (!e.side) {
      WN_HIP_CHECK(hipStreamCreateWithFlags(&e.side, hipStreamNonBlocking));
      WN_HIP_CHECK(hipEventCreateWithFlags(&e.ev_fork, hipEventDisableTiming));
      WN_HIP_CHECK(hipEventCreateWithFlags(&e.ev_join, hipEventDisableTiming));
    }
    if (!e.ev_ffork) {
      WN_HIP_CHECK(hipEventCreateWithFlags(&e.ev_ffork, hipEventDisableTiming));
      WN_HIP_CHECK(hipEventCreateWithFlags(&e.ev_fjoin, hipEventDisableTiming));
    }
    WN_HIP_CHECK(hipEventRecord(e.ev_ffork, s));
    WN_HIP_CHECK(hipStreamWaitEvent(e.side, e.ev_ffork, 0));
    const int rc = fold_prep(e.side);
    if (rc) return rc;
    WN_HIP_CHECK(hipEventRecord(e.ev_fjoin, e.side));
    return WN_OK;
  }

  // conditioning: mapping Dense stack + per-block time-invariant bias  (src/model.py:221-225,
  // src/layers.py:203-204: conv_cond(repeat(m)) == per-utterance bias).  With F frames armed (local conditioning,
  // src/model.py:216-220: the mapped condition is upsampled by repetition) the same phase runs over Bc = B * F rows: the
  // 1x1 mapping convs over (B, F, Cin) are the Dense stack over its rows, and the bias table has a row per (utterance, frame).
  // Which kernel each product takes does not depend on Bc: the small-product kernel tiles its rows by 32, the rows GEMM
  // walks them as one "utterance" of Bc time steps.
  int condition() {
    if (fp.cond == FWD_COND_NONE) return WN_OK;
    if (!cond) { wn_set_error("Conditioning must be provided."); return WN_E_INVALID; }
    const bool small = fp.cond == FWD_COND_SMALL;
    const float* m = cond;
    int mc = p->c.cond_inputs, rc;
    for (size_t j = 0; j < p->mapping.size(); ++j) {
      const ConvInfo& c = p->mapping[j];
      if (small)              // Dense: M[j] = act(m W + b), W = kernel (cin, cout)
        rc = wn_launch_sgemm_small_batched(m, mc, 1, 0, par(c.kernel_t), c.cout, 1, 0, ws + L.M[j], c.cout, 0,
                                           Bc, c.cout, mc, 1, par(c.bias_t), p->c.mapping_activation, s);
      else
        rc = Gemm(1, Bc, c.cout, ceil32(c.cout)).seg(m, mc, mc, 0, fragbase + c.fragF)
                 .bias(par(c.bias_t)).act(p->c.mapping_activation).run(ws + L.M[j], c.cout, s);
      if (rc) return rc;
      m = ws + L.M[j]; mc = c.cout;
    }
    const int D2 = 2 * p->D;
    if (!fp.cond_batched) {
      for (int b = 0; b < p->N; ++b) {
        const ConvInfo& c = p->blocks[b].conv_cond;
        rc = Gemm(1, Bc, D2, ceil32(D2)).seg(m, p->Cc, p->Cc, 0, fragbase + c.fragF)
                 .bias(par(c.bias_t)).run(ws + L.cb + (int64_t)b * Bc * D2, D2, s);
        if (rc) return rc;
      }
      return WN_OK;
    }
    // all blocks in one contraction, then [B][N*2D] -> [N][B][2D] with the biases added
    const ConvInfo& c0 = p->blocks[0].conv_cond;
    const int64_t bst = p->N > 1 ? p->tensors[p->blocks[1].conv_cond.bias_t].off - p->tensors[c0.bias_t].off : 0;
    if (small) {              // block z: cbt[:, z * 2D ..] = m W_c(z), W_c = kernel (1, Cc, 2D)
      const int64_t wst = p->N > 1 ? p->tensors[p->blocks[1].conv_cond.kernel_t].off - p->tensors[c0.kernel_t].off : 0;
      rc = wn_launch_sgemm_small_batched(m, p->Cc, 1, 0, par(c0.kernel_t), D2, 1, wst, ws + L.cbt, p->N * D2, D2,
                                         Bc, D2, p->Cc, p->N, nullptr, 0, s);
    } else {
      rc = Gemm(1, Bc, p->N * D2, ceil32(p->N * D2)).seg(m, p->Cc, p->Cc, 0, fragbase + p->frag_condF).run(ws + L.cbt, p->N * D2, s);
    }
    if (rc) return rc;
    return wn_launch_cond_scatter(ws + L.cbt, params, p->tensors[c0.bias_t].off, bst, Bc, p->N, D2, ws + L.cb, s);
  }

  // input causal conv, src/model.py:84-88,228 : KS taps with C_in = 1 (behind the cleared range-guard slot)
  int input_conv() {
    WN_HIP_CHECK(hipMemsetAsync(fam, 0, sizeof(float), s));
    int rc;
    if (fp.inconv_elem) {
      rc = wn_launch_inconv_fwd(x, par(p->causal.kernel_t), par(p->causal.bias_t), B, T, p->R, p->KS, ws + L.H[0], fam, s);
    } else {
      Gemm g(B, T, p->R, ceil32(p->R));
      for (int t = 0; t < p->KS; ++t)
        g.seg(x, 1, 1, (p->KS - 1 - t), fragbase + p->causal.fragF + t * p->causal.fragF_stride);
      rc = g.bias(par(p->causal.bias_t)).run(ws + L.H[0], p->R, s);
    }
    if (rc) return rc;
    if (rings) {
      rc = ring_capture(x, B, T, 1, p->KS, rings->xin, rings->t0, s);
      if (!rc) rc = ring_capture(ws + L.H[0], B, T, p->R, rings->nslots[0], rings->h[0], rings->t0, s);
    }
    return rc;
  }

  // residual blocks, src/model.py:230-234
  int blocks() {
    int rc;
    if (fp.zfill) {
      rc = wn_launch_fill(ws + L.Z, 0.f, rows * p->N * p->Dp, s);
      if (rc) return rc;
    }
    // profiling: is the chain N back-to-back launches of the fused block kernel?
    const bool prof_chain = e.prof_on && !rings && p->LPB == 1 && p->c.cond_inputs == 0 && p->R == p->D && !fp.drop && p->fused_ok;
    stack_prof = !rings && pair_free(e.stack_ev, e.stack_used);
    if (stack_prof) mark(e.stack_ev, e.stack_used, false, s);
    // the stack's start event (above) is the fork point: whatever the preparation costs the chain shows inside the pair
    if (fp.prep == FWD_PREP_SIDE) {
      rc = fold_prep_fork();
      if (rc) return rc;
    }
    for (int b = 0; b < p->N; ++b) {
      BlockPtrs k = block_ptrs(p, b, params, fragbase, B, T);
      if (fp.deep16) deep16_ptrs(p, b, fragbase, k);
      if (fp.cond != FWD_COND_NONE) {
        k.cb = ws + L.cb + (int64_t)b * Bc * 2 * p->D;
        k.cb_frames = F; k.cb_hop = hop;                 // (F == 1: the row is the utterance)
      }
      BlockBufs f = block_bufs(p, L, ws, b, rows, training, fp.drop);
      if (fp.drop) {
        rc = wn_launch_dropout(f.res, nullptr, ws + L.XD[b], rows * p->R, e.drop_rate,
                               wn_dropout_key(e.drop_seed, b, e.drop_step), nullptr, s);
        if (rc) return rc;
      }
      f.U = ws + L.U;
      f.x_out = ws + L.H[training ? b + 1 : ((b + 1) & 1)];
      f.fwd_absmax = fam;
      // one event pair per block launch, or one around the whole chain
      const bool prof = e.prof_on && pair_free(e.prof_ev, e.prof_used);
      if (prof && (!prof_chain || b == 0)) mark(e.prof_ev, e.prof_used, false, s);
      rc = block_forward(k, f, s);
      if (rc) return rc;
      if (prof && (!prof_chain || b == p->N - 1)) {
        e.prof_cnt[e.prof_used / 2] = prof_chain ? p->N : 1;
        mark(e.prof_ev, e.prof_used, true, s);
      }
      if (rings && b + 1 < p->N) {
        rc = ring_capture(f.x_out, B, T, p->R, rings->nslots[b + 1], rings->h[b + 1], rings->t0, s);
        if (rc) return rc;
      }
      if (rings)
        for (int i = 0; i + 1 < p->LPB; ++i) {
          rc = ring_capture(f.P[i], B, T, p->D, rings->nslots_p[b][i], rings->hp[b][i], rings->t0, s);
          if (rc) return rc;
        }
    }
    if (fp.prep == FWD_PREP_SIDE) WN_HIP_CHECK(hipStreamWaitEvent(s, e.ev_fjoin, 0));   // the fold's images and biases are ready
    return WN_OK;
  }

  // skip sum folded into one contraction over all blocks' gated activations (src/model.py:235-236
  // with src/layers.py:216-219), or the last block output when use_skip is False
  int skip() {
    int rc = WN_OK;
    switch (fp.skip) {
      // a = act(sum_b V(b)^T z_b + b'): the skip sum and the head's first conv in ONE contraction with F0 output columns
      case FWD_SKIP_FOLD_PLANES:   // streamed kernel, second form (wn_gemm16s.hip)
        rc = Planes(B, T, fp.hc0).operand(ws + L.Z, p->Dp, p->D, p->N, rows * p->Dp).w16(fragbase + p->frag16_foldF)
                 .bias(ws + L.bfold).act(p->c.activation).absmax_fwd(fam).run(ws + L.HA[0], fp.hc0, s);
        hin = ws + L.HA[0];
        break;
      case FWD_SKIP_FOLD_ROWS:     // other shapes: wn_gemm_rows16_kernel, the same products in the same order
        rc = Gemm(B, T, fp.hc0, ceil32(fp.hc0)).seg_planes(ws + L.Z, p->Dp, rows * p->Dp, p->N * p->Dp, nullptr)
                 .w16(fragbase + p->frag16_foldF).bias(ws + L.bfold).act(p->c.activation).absmax_fwd(fam)
                 .run(ws + L.HA[0], fp.hc0, s);
        hin = ws + L.HA[0];
        break;
      case FWD_SKIP_SUM:
        rc = Gemm(B, T, p->Sh, ceil32(p->Sh)).seg_planes(ws + L.Z, p->Dp, rows * p->Dp, p->N * p->Dp, fragbase + p->frag_skipF)
                 .w16(p->frag16_skipF >= 0 ? fragbase + p->frag16_skipF : nullptr)
                 .bias(ws + L.bias_sum).absmax_fwd(fam).run(ws + L.skipsum, p->Sh, s);
        hin = ws + L.skipsum;
        break;
      case FWD_SKIP_NONE:
        hin = ws + L.H[training ? p->N : (p->N & 1)];
        break;
    }
    if (rc) return rc;
    if (stack_prof) mark(e.stack_ev, e.stack_used, true, s);
    return WN_OK;
  }

  // head, src/model.py:105-119,237-238: conv -> activation, last conv linear (softmax applied later)
  int head() {
    int hc = fp.hc0;
    for (int i = fp.first_final; i < fp.nhead; ++i) {
      const ConvInfo& c = p->finals[i];
      const bool last = (i + 1 == fp.nhead);
      float* dst = last ? ws + L.logits : ws + L.HA[i];
      int rc;
      switch (fp.head[i]) {
        // training pass of a 256-class categorical head: the loss is this conv's epilogue (no logits tensor); a scoring
        // pass (lf->eval) takes the evaluation form of it: the loss rows and nothing else
        case FWD_HEAD_EPILOGUE:
          rc = Planes(B, T, c.cout).operand(hin, hc, hc).w16(fragbase + c.frag16).bias(par(c.bias_t)).act(WN_ACT_LINEAR)
                   .loss(*lf).run(lf->g_logits, c.cout, s);
          if (rc) return rc;
          lf->done = true;
          return WN_OK;
        // 128 / 256 output columns: the streamed kernel's second form (wn_gemm16s.hip; the operand is one "plane"); same
        // products in the same order as the rows GEMM below
        case FWD_HEAD_PLANES:
          rc = Planes(B, T, c.cout).operand(hin, hc, hc).w16(fragbase + c.frag16).bias(par(c.bias_t))
                   .act(last ? WN_ACT_LINEAR : p->c.activation).absmax_fwd(last ? nullptr : fam).run(dst, c.cout, s);
          break;
        default:
          rc = Gemm(B, T, c.cout, ceil32(c.cout)).seg(hin, hc, hc, 0, fragbase + c.fragF)
                   .w16(c.frag16 >= 0 ? fragbase + c.frag16 : nullptr)
                   .bias(par(c.bias_t)).act(last ? WN_ACT_LINEAR : p->c.activation)
                   .absmax_fwd(last ? nullptr : fam).run(dst, c.cout, s);
          break;
      }
      if (rc) return rc;
      hin = dst; hc = c.cout;
    }
    return WN_OK;
  }
};

int forward_core(wn_plan* p, const float* params, const float* x, bool prep, const float* cond, int B,
                 int T, bool training, float* ws, const WsLayout& L, hipStream_t s, const GenRings* rings, LossFuse* lf) {
  int rc = ensure_device_tables(p);
  if (rc) return rc;
  FwdCall c(p, params, x, prep, cond, B, T, training, ws, L, s, rings, lf);
  if ((rc = c.weight_images())) return rc;
  if (c.fp.prep == FWD_PREP_INLINE && (rc = c.fold_prep(s))) return rc;
  if ((rc = c.condition())) return rc;
  if ((rc = c.input_conv())) return rc;
  if ((rc = c.blocks())) return rc;      // (FWD_PREP_SIDE: fold_prep() forked off at their start, joined at their end)
  if ((rc = c.skip())) return rc;
  return c.head();
}

int emit_outputs(const wn_plan* p, const float* ws, const WsLayout& L, int64_t rows, float* logits_out, float* out, hipStream_t s) {
  const size_t bytes = rows * p->Cout * sizeof(float);
  if (logits_out) WN_HIP_CHECK(hipMemcpyAsync(logits_out, ws + L.logits, bytes, hipMemcpyDeviceToDevice, s));
  if (!out) return WN_OK;
  if (p->c.head == WN_HEAD_CATEGORICAL) return wn_launch_softmax(ws + L.logits, out, rows, p->Cout, s);
  WN_HIP_CHECK(hipMemcpyAsync(out, ws + L.logits, bytes, hipMemcpyDeviceToDevice, s));
  return WN_OK;
}

int shift_split(const float* x_full, int B, int T, float* inputs, float* y_true, hipStream_t s) {
  const int64_t rows = (int64_t)B * T;
  hipLaunchKernelGGL(wn_shift_split_kernel, dim3((unsigned)std::min<int64_t>((rows + 255) / 256, 4096)), dim3(256), 0, s,
                     x_full, B, T, inputs, y_true);
  WN_HIP_CHECK(hipGetLastError());
  return WN_OK;
}

// the split-precision head of a 256-class categorical model whose last conv the streamed 256-column kernel takes
bool loss_fusable(const wn_plan* p, int64_t rows) {
  if (p->c.head != WN_HEAD_CATEGORICAL || p->Cout != 256 || wn_debug_get(1) == 1 || p->finals.empty()) return false;
  const ConvInfo& c = p->finals.back();
  return c.frag16 >= 0 && c.cout == 256 && rows > 0;
}

int loss_stage(wn_plan* p, int B, int T, int global_batch, bool want_grad, float* ws, const WsLayout& L,
               float* loss_out, float* absmax_out, hipStream_t s, bool fused_done, const float* row_weight) {
  const int64_t rows = (int64_t)B * T;
  const float gscale = 1.0f / (float)global_batch;     // compute_average_loss, src/model.py:328-329
  int rc;
  // (the head's last conv already left the row losses and d loss / d logits: see LossFuse; weighted rows are stored
  // weighted by every loss kernel, so the sum below is the same launch with and without weights)
  if (fused_done) return wn_launch_sum(ws + L.loss_rows, rows, gscale, loss_out, ws + L.sum_scratch, s);
  // deferred weight gradients read d loss / d logits from GF.back(): written there directly (no 131 MB copy)
  float* g_logits = want_grad ? ws + L.GF.back() : nullptr;
  rc = loss_rows_stage(p, rows, gscale, g_logits, want_grad, ws, L, absmax_out, s, row_weight);
  if (rc) return rc;
  return wn_launch_sum(ws + L.loss_rows, rows, gscale, loss_out, ws + L.sum_scratch, s);
}

int loss_rows_stage(wn_plan* p, int64_t rows, float gscale, float* g_logits, bool want_grad, float* ws, const WsLayout& L,
                    float* absmax_out, hipStream_t s, const float* row_weight) {
  int rc;
  if (p->c.head == WN_HEAD_CATEGORICAL) {
    rc = wn_launch_quantize(ws + L.yt, reinterpret_cast<int32_t*>(ws + L.target), rows, p->c.bits, s);
    if (rc) return rc;
    // an armed step sample (wn_plan_arm_step_sample) rides in the loss kernel when the row fits its registers
    float* so = nullptr;
    if (want_grad && wnp::ex(p).step_sample && !wnp::ex(p).step_sample_det && p->Cout <= 256) { so = wnp::ex(p).step_sample; wnp::ex(p).step_sample = nullptr; }
    rc = wn_launch_cat_loss(ws + L.logits, reinterpret_cast<const int32_t*>(ws + L.target), rows, p->Cout,
                            gscale, ws + L.loss_rows, g_logits, absmax_out, s, so, p->c.bits, wnp::ex(p).step_sample_seed,
                            wnp::ex(p).step_sample_off, row_weight);
  } else {
    rc = wn_launch_mix_loss(ws + L.logits, ws + L.yt, rows, p->c.num_mixtures, p->c.bits,
                            p->c.head == WN_HEAD_LOGISTIC ? 1 : 2, gscale, ws + L.loss_rows, g_logits, absmax_out, s, row_weight);
  }
  return rc;
}

int condition_only(wn_plan* p, const float* params, const float* cond, int B, int T, float* ws, const WsLayout& L, hipStream_t s) {
  // (prep = false: the weight images of the priming pass are in the workspace)
  FwdCall c(p, params, nullptr, false, cond, B, T, false, ws, L, s, nullptr, nullptr);
  return c.condition();
}

int condition_rows(wn_plan* p, const float* params, const float* cond, int rows, const float* fragbase, float* buf,
                   const WsLayout& L, hipStream_t s) {
  // (B = rows utterances of one time step, one frame each: Bc = rows; condition() only reads the images)
  FwdCall c(p, params, nullptr, false, cond, rows, 1, false, buf, L, s, nullptr, nullptr);
  c.fragbase = const_cast<float*>(fragbase);
  return c.condition();
}

int cond_frames_check(const char* who, const wn_plan* p, int T) {
  const int F = ex(p).cond_frames;
  if (F <= 1 || p->c.cond_inputs <= 0) return 1;
  if (T % F != 0) {
    wn_set_error("%s: T = %d inputs do not divide into F = %d condition frames (hop = T / F)", who, T, F);
    return WN_E_INVALID;
  }
  const int hop = T / F;
  if (hop % 32 != 0) {
    wn_set_error("%s: T = %d, F = %d gives hop = %d, which is not a multiple of 32 (F > 1 needs whole 32-row tiles per frame)",
                 who, T, F, hop);
    return WN_E_INVALID;
  }
  return F;
}

int row_weights_check(const char* who, const wn_exec& e, int B, int T) {
  if (!e.row_weights || e.row_weights_n == (int64_t)B * T) return WN_OK;
  wn_set_error("%s: the armed row weights cover %lld rows, the call has B * T = %lld", who, (long long)e.row_weights_n,
               (long long)((int64_t)B * T));
  return WN_E_INVALID;
}

}  // namespace wnp

using namespace wnp;

// wn_forward / wn_forward_training: one body; `who` is the prefix of its error texts
static int forward_entry(const char* who, bool training, wn_plan* p, const float* params, const float* x, const float* cond,
                         int32_t B, int32_t T, float* out, float* logits_out, float* workspace, int64_t ws_floats, void* stream) {
  if (!p || !params || !x || !workspace || B < 1 || T < 1) { wn_set_error("%s: bad arguments", who); return WN_E_INVALID; }
  if (cond_frames_check(who, p, T) < 0) return WN_E_INVALID;
  hipStream_t s = (hipStream_t)stream;
  const WsLayout L = make_layout(p, B, T, training);
  if (ws_floats < L.total) { wn_set_error("%s: workspace too small (%lld < %lld floats)", who, (long long)ws_floats, (long long)L.total); return WN_E_INVALID; }
  const int rc = forward_core(p, params, x, true, cond, B, T, training, workspace, L, s);
  if (rc) return rc;
  return emit_outputs(p, workspace, L, (int64_t)B * T, logits_out, out, s);
}

extern "C" int wn_forward(wn_plan* p, const float* params, const float* x, const float* cond, int32_t B,
                          int32_t T, float* out, float* logits_out, float* workspace, int64_t ws_floats,
                          void* stream) {
  return forward_entry("forward", false, p, params, x, cond, B, T, out, logits_out, workspace, ws_floats, stream);
}

// WaveNet.call(inputs, training=True), src/model.py:213-239 with src/layers.py:195-196: the forward pass with the
// Dropout layers active (the mask of the step set by wn_plan_set_dropout).  Needs the TRAINING workspace size.
extern "C" int wn_forward_training(wn_plan* p, const float* params, const float* x, const float* cond, int32_t B,
                                   int32_t T, float* out, float* logits_out, float* workspace, int64_t ws_floats,
                                   void* stream) {
  return forward_entry("forward_training", true, p, params, x, cond, B, T, out, logits_out, workspace, ws_floats, stream);
}

extern "C" int wn_eval_loss(wn_plan* p, const float* params, const float* x_full, const float* cond,
                            int32_t B, int32_t T, int32_t global_batch, float* loss_out, float* pred_out,
                            float* workspace, int64_t ws_floats, void* stream) {
  if (!p || !params || !x_full || !workspace || !loss_out || B < 1 || T < 1) { wn_set_error("eval_loss: bad arguments"); return WN_E_INVALID; }
  if (row_weights_check("eval_loss", wnp::ex(p), B, T)) return WN_E_INVALID;
  if (cond_frames_check("eval_loss", p, T) < 0) return WN_E_INVALID;
  hipStream_t s = (hipStream_t)stream;
  const WsLayout L = make_layout(p, B, T, false);
  if (ws_floats < L.total) { wn_set_error("eval_loss: workspace too small"); return WN_E_INVALID; }
  const int64_t rows = (int64_t)B * T;
  // inputs live in the (otherwise unused here) probs region
  float* inputs = workspace + L.probs;
  { const int rcs = shift_split(x_full, B, T, inputs, workspace + L.yt, s); if (rcs) return rcs; }
  int rc = forward_core(p, params, inputs, true, cond, B, T, false, workspace, L, s);
  if (rc) return rc;
  rc = loss_stage(p, B, T, global_batch > 0 ? global_batch : B, false, workspace, L, loss_out, nullptr, s, false,
                  wnp::ex(p).row_weights);
  if (rc) return rc;
  rc = wn_launch_guard_flag(workspace + L.fwd_absmax, WN_RANGE_LIMIT, wn_debug_get(1) != 1, loss_out + 2, s);
  if (rc) return rc;
  return emit_outputs(p, workspace, L, rows, nullptr, pred_out, s);
}

// WaveNet.score: the evaluation pass of wn_eval_loss up to the row losses, then one workgroup per utterance.  A 256-class
// head the streamed kernel takes forms the rows in the last conv's epilogue (evaluation form: LossFuse.eval); everything
// else runs the standalone loss kernel on the logits, without a gradient, as wn_eval_loss does.
extern "C" int wn_score(wn_plan* p, const float* params, const float* x_full, const float* cond, int32_t B, int32_t T,
                        float* nll_out, float* weight_out, float* rows_out, float* flag_out,
                        float* workspace, int64_t ws_floats, void* stream) {
  if (!p) { wn_set_error("score: null plan"); return WN_E_INVALID; }
  if (!params || !x_full || !nll_out || !flag_out || !workspace) {
    wn_set_error("score: null %s", !params ? "params" : !x_full ? "x_full" : !nll_out ? "nll_out" : !flag_out ? "flag_out" : "workspace");
    return WN_E_INVALID;
  }
  if (p->c.cond_inputs > 0 && !cond) { wn_set_error("score: the plan is conditioned (%d inputs) and cond is null", p->c.cond_inputs); return WN_E_INVALID; }
  if (B < 1 || T < 1) { wn_set_error("score: B = %d, T = %d: both must be at least 1", (int)B, (int)T); return WN_E_INVALID; }
  if (row_weights_check("score", wnp::ex(p), B, T)) return WN_E_INVALID;
  if (cond_frames_check("score", p, T) < 0) return WN_E_INVALID;
  hipStream_t s = (hipStream_t)stream;
  const WsLayout L = make_layout(p, B, T, false);
  if (ws_floats < L.total) {
    wn_set_error("score: workspace too small (%lld < %lld floats)", (long long)ws_floats, (long long)L.total);
    return WN_E_INVALID;
  }
  const int64_t rows = (int64_t)B * T;
  const float* rw = wnp::ex(p).row_weights;
  float* inputs = workspace + L.probs;                   // (as wn_eval_loss: the probs region is free in this pass)
  int rc = shift_split(x_full, B, T, inputs, workspace + L.yt, s);
  if (rc) return rc;
  LossFuse lf;
  memset(&lf, 0, sizeof(lf));
  const bool fuse = loss_fusable(p, rows);
  if (fuse) {
    rc = wn_launch_quantize(workspace + L.yt, reinterpret_cast<int32_t*>(workspace + L.target), rows, p->c.bits, s);
    if (rc) return rc;
    lf.target = reinterpret_cast<const int32_t*>(workspace + L.target);
    lf.loss_rows = workspace + L.loss_rows;
    lf.row_weight = rw;
    lf.eval = true;
  }
  rc = forward_core(p, params, inputs, true, cond, B, T, false, workspace, L, s, nullptr, fuse ? &lf : nullptr);
  if (rc) return rc;
  if (!lf.done) {
    rc = loss_rows_stage(p, rows, 1.0f, nullptr, false, workspace, L, nullptr, s, rw);
    if (rc) return rc;
  }
  rc = wn_launch_score_reduce(workspace + L.loss_rows, rw, B, T, nll_out, weight_out, s);
  if (rc) return rc;
  if (rows_out) WN_HIP_CHECK(hipMemcpyAsync(rows_out, workspace + L.loss_rows, rows * sizeof(float), hipMemcpyDeviceToDevice, s));
  return wn_launch_guard_flag(workspace + L.fwd_absmax, WN_RANGE_LIMIT, wn_debug_get(1) != 1, flag_out, s);
}
