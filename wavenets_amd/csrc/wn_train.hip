// The gradient half of WaveNet.train_step (src/model.py:319-336): backward-data chain and deferred weight gradients (the
// optimizer step: wn_optim.hip).
#include "wn_plan_internal.h"

namespace {
using namespace wnp;

// ---- batched weight-gradient job table for one (B, T) layout ----
void add_jobs(std::vector<WnWgJob>& jobs, int64_t x_off, int ldx, int K, int shift, int64_t g_off, int ldg, int N,
              int64_t out_off, int64_t bias_off, int64_t gmax_off) {
  const int tk = wn_wgrad_tile_k(), tn = wn_wgrad_tile_n();
  for (int k0 = 0; k0 < K; k0 += tk)
    for (int n0 = 0; n0 < N; n0 += tn) {
      WnWgJob j;
      memset(&j, 0, sizeof(j));
      j.x_off = x_off; j.g_off = g_off; j.out_off = out_off; j.bias_off = (k0 == 0) ? bias_off : -1;
      j.gmax_off = gmax_off;
      j.ldx = ldx; j.ldg = ldg; j.K = K; j.N = N; j.shift = shift; j.k0 = k0; j.n0 = n0;
      jobs.push_back(j);
    }
}

// the cached schedule of e: rebuilt when (B, T, bsplits, condition frames, paths) is not the key it was built for (the
// tables hold workspace offsets, and the regions behind the conditioning's move with its row count)
int ensure_schedule(const wn_plan* p, wn_exec& e, const WsLayout& L, int B, int T, const TrainPaths& tp) {
  WgSchedule& g = e.wg;
  if (g.valid && g.B == B && g.T == T && g.bsplits == L.bsplits && g.frames == L.frames && g.paths == tp) return WN_OK;
  const bool layerk = tp.layerk(), pairk = tp.pairk(), fold = tp.fold;
  std::vector<WnWgLayer> wgl, wgli;
  std::vector<WnWgPair> pairs[3];
  std::vector<WnWgPair> hpairs[6];
  std::vector<WnWgJob> jobs;
  std::vector<WnTensorDesc> cov;
  auto cover = [&](int t) { WnTensorDesc d; d.off = p->tensors[t].off; d.len = p->tensors[t].len; cov.push_back(d); };
  const AbsmaxSlots slot{(int)p->finals.size(), p->N, p->LPB};
  const int64_t am_skip = L.absmax + slot.gskip();
  auto am_GU = [&](int b) { return L.absmax + slot.gu(b); };
  auto am_GH = [&](int b) { return L.absmax + slot.gh(b); };
  auto am_GP = [&](int b, int i) { return tp.deep16 ? L.absmax + slot.gp(b, i) : (int64_t)-1; };
  // input causal conv: x = inputs (B,T,1), g = d loss / d H[0]
  if (!tp.in_split)
    for (int t = 0; t < p->KS; ++t)
      add_jobs(jobs, L.probs, 1, 1, p->KS - 1 - t, L.GH[0], p->R, p->R,
               p->tensors[p->causal.kernel_t].off + (int64_t)t * p->R,
               t == p->KS - 1 ? p->tensors[p->causal.bias_t].off : -1, am_GH(0));
  cover(p->causal.kernel_t); cover(p->causal.bias_t);
  for (int b = 0; b < p->N; ++b) {
    const BlockInfo& bi = p->blocks[b];
    const ConvInfo& c = bi.dil.back();
    const int64_t zoff = L.Z + (int64_t)b * B * T * p->Dp;      // block-major Z
    if (layerk) {
      const int64_t xin0 = tp.drop ? L.XD[b] : L.H[b];
      for (int i = 0; i + 1 < p->LPB; ++i) {                     // inner convs of a deeper stack
        const ConvInfo& ci = bi.dil[i];
        WnWgLayer w;
        memset(&w, 0, sizeof(w));
        w.x_off = i == 0 ? xin0 : L.P[b][i - 1];
        w.du_off = L.GP[b][i];
        w.dwd_off = p->tensors[ci.kernel_t].off; w.dbd_off = p->tensors[ci.bias_t].off;
        w.dwr_off = w.dbr_off = -1; w.z_off = w.go_off = 0;
        w.gmax_u_off = am_GP(b, i); w.gmax_h_off = -1;
        w.dilation = ci.dil; w.ldz = p->Dp;
        wgli.push_back(w);
        cover(ci.kernel_t); cover(ci.bias_t);
      }
      WnWgLayer w;
      w.x_off = p->LPB > 1 ? L.P[b][p->LPB - 2] : xin0;
      w.du_off = L.GU[b]; w.z_off = zoff; w.ldz = p->Dp;
      w.go_off = p->S == 0 ? L.GO[b] : L.GH[b + 1];
      w.dwd_off = p->tensors[c.kernel_t].off; w.dbd_off = p->tensors[c.bias_t].off;
      w.dwr_off = p->tensors[bi.conv1.kernel_t].off; w.dbr_off = p->tensors[bi.conv1.bias_t].off;
      w.gmax_u_off = am_GU(b); w.gmax_h_off = p->S == 0 ? am_skip : am_GH(b + 1);
      w.dilation = c.dil;
      wgl.push_back(w);
    } else if (pairk) {
      const int64_t xoff = tp.drop ? L.XD[b] : L.H[b];
      {
        // both taps in one job: x[t - d] | x[t] against ONE read of du
        WnWgPair w;
        memset(&w, 0, sizeof(w));
        w.x_off = xoff; w.g_off = L.GU[b]; w.shift = c.dil;
        w.w_off = p->tensors[c.kernel_t].off;
        w.b_off = p->tensors[c.bias_t].off;
        w.gmax_off = am_GU(b);
        pairs[1].push_back(w);
      }
      WnWgPair w;
      memset(&w, 0, sizeof(w));
      w.x_off = zoff; w.g_off = p->S == 0 ? L.GO[b] : L.GH[b + 1]; w.shift = 0;
      w.w_off = p->tensors[bi.conv1.kernel_t].off; w.b_off = p->tensors[bi.conv1.bias_t].off;
      w.gmax_off = p->S == 0 ? am_skip : am_GH(b + 1);
      w.g2_off = w.w2_off = w.b2_off = w.gmax2_off = -1;
      if (tp.mfused) {
        // the folded skip path's M(b) = z_b^T dL/da rides in the same job (one read of z_b): second slab = mslab
        w.g2_off = L.GF[0]; w.w2_off = (int64_t)b * p->D * p->fold_F0;
        w.b2_off = b == 0 ? (int64_t)p->N * p->D * p->fold_F0 : -1;       // colsum(dL/da) once
        w.gmax2_off = L.absmax + slot.gf(0);
      }
      pairs[2].push_back(w);
    } else {
    // the dilated stack: conv i reads H[b] (or its dropped copy) / the activated output of conv i - 1; its output gradient
    // is GP[b][i], or GU[b] for the last, gated conv (2D wide).  (Inner gradients have no max-abs slot: stacks deeper
    // than 1 run this table in exact fp32, see the launch.)
    for (int i = 0; i < p->LPB; ++i) {
      const ConvInfo& ci = bi.dil[i];
      const bool lastc = i == p->LPB - 1;
      const int64_t xo = i == 0 ? (tp.drop ? L.XD[b] : L.H[b]) : L.P[b][i - 1];
      const int kc = i == 0 ? p->R : p->D, nc = lastc ? 2 * p->D : p->D;
      for (int t = 0; t < p->KS; ++t)
        add_jobs(jobs, xo, kc, kc, (p->KS - 1 - t) * ci.dil, lastc ? L.GU[b] : L.GP[b][i], nc, nc,
                 p->tensors[ci.kernel_t].off + (int64_t)t * kc * nc,
                 t == p->KS - 1 ? p->tensors[ci.bias_t].off : -1, lastc ? am_GU(b) : am_GP(b, i));
      if (!lastc) { cover(ci.kernel_t); cover(ci.bias_t); }
    }
    // S == 0: g_o = g_xout + g_skip (or a copy of g_skip): bounded by twice the larger max-abs -> no slot
    add_jobs(jobs, zoff, p->Dp, p->D, 0, p->S == 0 ? L.GO[b] : L.GH[b + 1], p->R, p->R,
             p->tensors[bi.conv1.kernel_t].off, p->tensors[bi.conv1.bias_t].off, p->S == 0 ? am_skip : am_GH(b + 1));
    }
    cover(bi.dil.back().kernel_t); cover(bi.dil.back().bias_t);
    cover(bi.conv1.kernel_t); cover(bi.conv1.bias_t);
    if (bi.has_skip && p->c.use_skip && !fold) {     // (folded: dW_s, db_s come out of M, see the weight-gradient phase)
      if (!tp.skipk)
        add_jobs(jobs, zoff, p->Dp, p->D, 0, L.g_skipsum, p->S, p->S,
                 p->tensors[bi.conv_skip.kernel_t].off, p->tensors[bi.conv_skip.bias_t].off, am_skip);
      cover(bi.conv_skip.kernel_t); cover(bi.conv_skip.bias_t);
    }
  }
  if (tp.mtr != 0) {
    // 64-channel blocks: dW_r, db_r of the job's blocks ride along (one read of z for both; the layer table then runs
    // without its 1x1 part)
    const bool zonce = tp.mtr == 7;
    const int per = zonce ? 2 : 256 / p->D;                   // blocks per job
    for (int b0 = 0; b0 < p->N; b0 += per) {
      WnWgPair w;
      memset(&w, 0, sizeof(w));
      w.x_off = L.Z + (int64_t)b0 * B * T * p->Dp;            // block-major Z: segment stride = one block's plane
      w.seg_stride = (int64_t)B * T * p->Dp;
      w.nseg = std::min(per, p->N - b0);
      w.g_off = L.GF[0]; w.shift = 0;
      w.w_off = (int64_t)b0 * p->D * p->fold_F0;
      w.b_off = b0 == 0 ? (int64_t)p->N * p->D * p->fold_F0 : -1;       // colsum(dL/da) once
      w.gmax_off = L.absmax + slot.gf(0);
      w.w2_off = w.b2_off = w.gmax2_off = -1;
      for (int sg = 0; zonce && sg < 2; ++sg) {               // (a segment that does not exist repeats the first: never written)
        const int b = b0 + (sg < w.nseg ? sg : 0);
        const BlockInfo& bi = p->blocks[b];
        w.seg[sg].g_off = L.GH[b + 1]; w.seg[sg].gmax_off = am_GH(b + 1);
        w.seg[sg].w_off = p->tensors[bi.conv1.kernel_t].off; w.seg[sg].b_off = p->tensors[bi.conv1.bias_t].off;
      }
      pairs[0].push_back(w);
    }
  }
  const int head_first = (int)jobs.size(), cov_head = (int)cov.size();
  for (size_t i = fold ? 1 : 0; i < p->finals.size(); ++i) {      // (folded: the first conv's gradients come from M too)
    const ConvInfo& c = p->finals[i];
    const int64_t xin = (i == 0) ? (p->c.use_skip ? L.skipsum : L.H[p->N]) : L.HA[i - 1];
    if (tp.headpairs() && wn_wgrad_pair_kind(c.cin, c.cout) != 0) {
      WnWgPair w;
      memset(&w, 0, sizeof(w));
      w.x_off = xin; w.g_off = L.GF[i]; w.shift = 0;
      w.w_off = p->tensors[c.kernel_t].off; w.b_off = p->tensors[c.bias_t].off;
      w.gmax_off = L.absmax + slot.gf((int)i);
      const int kind = wn_wgrad_pair_kind(c.cin, c.cout);
      hpairs[kind].push_back(w);
      if (kind == 5) {                     // second 128-column half
        w.g_off += 128; w.w_off += 128; w.b_off += 128;
        hpairs[kind].push_back(w);
      }
    } else {
      add_jobs(jobs, xin, c.cin, c.cin, 0, L.GF[i], c.cout, c.cout, p->tensors[c.kernel_t].off,
               p->tensors[c.bias_t].off, L.absmax + slot.gf((int)i));
    }
    cover(c.kernel_t); cover(c.bias_t);
  }
  // ---- the launches over these tables, in issue order: first the low-occupancy leftovers (input conv, generic jobs, the
  // head) that may run beside the rest on a side stream, then the per-block kernels and the skip path ----
  std::vector<WnWgPair> all;     // one pair table: the blocks' jobs by kind, then the head's
  int pfirst[3], hfirst[6] = {0, 0, 0, 0, 0, 0};
  for (int kd = 0; kd <= 2; ++kd) { pfirst[kd] = (int)all.size(); all.insert(all.end(), pairs[kd].begin(), pairs[kd].end()); }
  for (int kd = 1; kd <= 5; ++kd) { hfirst[kd] = (int)all.size(); all.insert(all.end(), hpairs[kd].begin(), hpairs[kd].end()); }
  std::vector<WgSpan> spans;
  auto span = [&](WgSpan::Op op, WgSpan::Slab slab, int kind, int first, size_t count) {
    if (count > 0) spans.push_back(WgSpan{op, slab, kind, first, (int)count});
  };
  const int njobs = (int)jobs.size();
  const bool head_own = tp.head_split && (head_first < njobs || tp.headpairs());
  span(WgSpan::INCONV, WgSpan::BATCH, 0, 0, tp.in_split);      // the input conv's dW / db from the dedicated reduction kernel
  span(WgSpan::JOBS, WgSpan::BATCH, tp.wg == WG_GENERIC_FP32, 0, head_own ? head_first : njobs);
  if (head_own) span(WgSpan::JOBS, WgSpan::HEAD, 0, head_first, njobs - head_first);
  for (int kd = 1; kd <= 5; ++kd) {
    // staged kinds 1 (128 x 256), 3 (256 x 128), 5 (256 x 256 halves) have transposed-read forms (3, 4, 5)
    const int trk = kd == 1 ? 3 : (kd == 3 ? 4 : (kd == 5 ? 5 : (kd == 2 ? 2 : 0)));
    // (with 64-channel blocks the staged head jobs are faster beside the side stream's neighbours)
    if (trk != 0 && tp.pairk()) span(WgSpan::TR, WgSpan::HEAD, trk, hfirst[kd], hpairs[kd].size());
    else span(WgSpan::PAIRS, WgSpan::HEAD, kd, hfirst[kd], hpairs[kd].size());
  }
  const int n_side = (int)spans.size();
  // transposed-read kernels: both taps of dW_d in one job; dW_r (+ M)
  span(WgSpan::TR, WgSpan::BATCH, 1, pfirst[1], pairs[1].size());
  span(WgSpan::TR, WgSpan::BATCH, tp.mfused ? 6 : 2, pfirst[2], pairs[2].size());
  span(WgSpan::LAYERS, WgSpan::BATCH, tp.mtr == 7 ? 2 : 0, 0, wgl.size());
  span(WgSpan::LAYERS, WgSpan::BATCH, 1, 0, wgli.size());
  // folded skip path: M = Z^T dL/da (N*D x F0) and colsum(dL/da) into their own slab; else dW_s, db_s of every block
  if (tp.mtr != 0) span(WgSpan::TR, WgSpan::MFOLD, tp.mtr, pfirst[0], pairs[0].size());
  else if (tp.fold) span(WgSpan::SKIP, WgSpan::MFOLD, 0, 0, !tp.mfused);
  else span(WgSpan::SKIP, WgSpan::BATCH, 0, 0, tp.skipk);
  g.valid = false;
  int rc = g.jobs.upload(jobs, 1);
  if (!rc) rc = g.cov.upload(cov);
  if (!rc) rc = g.layers.upload(wgl);
  if (!rc) rc = g.inner.upload(wgli);
  if (!rc) rc = g.pairs.upload(all);
  if (rc) return rc;
  g.h_cov.swap(cov); g.spans.swap(spans);
  g.n_side = n_side; g.overlap = layerk || pairk; g.cov_head = head_own ? cov_head : (int)g.h_cov.size();
  g.B = B; g.T = T; g.bsplits = L.bsplits; g.frames = L.frames; g.paths = tp;
  g.valid = true;
  return WN_OK;
}

// ------------------------------------------------------------------------------------------
// One call of wn_train_fwd_bwd: the caller's buffers, the workspace layout of (B, T) and the running max-abs slots of the
// gradient tensors; the phases of the step are its member functions, in launch order.
// ------------------------------------------------------------------------------------------
struct TrainCall {
  wn_exec& e;                        // the calling thread's execution state for p
  wn_plan* p; const float* params; const float* x_full; const float* cond;
  int B, T, global_batch, n_replicas;
  float* grads; float* loss_out; float* pred_out; float* ws; hipStream_t s;
  WsLayout L;
  int64_t rows;
  float* inputs;
  const float* fragbase; float* slab;
  float* am; AbsmaxSlots slot;       // running max-abs scalars of the gradient tensors (operand scaling of the split-precision GEMMs)
  int nf; float* am_gskip;
  const float* mlast = nullptr;      // the mapped condition (input of every conv_cond)
  TrainPaths tp;                     // backward half: the kernel families of this call
  bool cond_batched = false;
  int F = 1, Bc = 0;                 // condition frames per utterance (local conditioning; 1: global) and condition rows B * F
  float* g_x = nullptr; float* g_cond = nullptr;   // wn_vjp: gradients at the input waveform / the condition (null: not formed)
  int64_t pm = 0;                    // folded skip path: row pitch of the slab of M = Z^T dL/da with the column sums behind it
  float* am_GF(int i) const { return am + slot.gf(i); }
  float* am_GU(int b) const { return am + slot.gu(b); }
  float* am_GH(int b) const { return am + slot.gh(b); }
  float* am_GP(int b, int i) const { return am + slot.gp(b, i); }
  // flat-buffer offset of a tensor of block 0 and its distance to block 1's (evenly spaced blocks)
  struct Strided { int64_t off, stride; };
  Strided strided(int t0, int t1) const { return {p->tensors[t0].off, p->N > 1 ? p->tensors[t1].off - p->tensors[t0].off : 0}; }
  Strided skip_w{0, 0}, skip_b{0, 0};   // conv_skip kernels / biases

  // what every entry point sets the same way: buffers, the training layout of (B, T), the max-abs slots (host only)
  void bind(wn_plan* p_, const float* params_, const float* cond_, int B_, int T_, float* grads_, float* workspace, hipStream_t s_) {
    p = p_; params = params_; x_full = nullptr; cond = cond_; B = B_; T = T_; global_batch = B_; n_replicas = 1;
    grads = grads_; loss_out = nullptr; pred_out = nullptr; ws = workspace; s = s_;
    L = make_layout(p, B, T, true);
    F = L.frames; Bc = B * F;
    rows = (int64_t)B * T;
    inputs = workspace + L.probs;
    am = workspace + L.absmax;
    nf = (int)p->finals.size();
    slot = AbsmaxSlots{nf, p->N, p->LPB};
    am_gskip = am + slot.gskip();
  }

  // ---- forward + loss (+ the armed step sample, the L2 loss term, the range flag): src/model.py:319-334 ----
  int forward_and_loss() {
    int rc;
    { const int rcs = shift_split(x_full, B, T, inputs, ws + L.yt, s); if (rcs) return rcs; }
    if (e.phase_on) (void)hipEventRecord(e.phase_ev[0], s);
    // (zeroed before the forward pass: a fused loss epilogue publishes the max-abs of d loss / d logits from there)
    WN_HIP_CHECK(hipMemsetAsync(am, 0, L.n_absmax * sizeof(float), s));
    // 256-class categorical head: the loss rides in the head's last conv (LossFuse) unless the caller wants the probabilities
    LossFuse lf;
    memset(&lf, 0, sizeof(lf));
    const bool fuse = !pred_out && loss_fusable(p, rows);
    if (fuse) {
      rc = wn_launch_quantize(ws + L.yt, reinterpret_cast<int32_t*>(ws + L.target), rows, p->c.bits, s);
      if (rc) return rc;
      lf.target = reinterpret_cast<const int32_t*>(ws + L.target);
      lf.gscale = 1.0f / (float)global_batch;          // compute_average_loss, src/model.py:328-329
      lf.loss_rows = ws + L.loss_rows; lf.g_logits = ws + L.GF.back(); lf.absmax_out = am_GF(nf - 1);
      if (e.step_sample && !e.step_sample_det) {     // the armed sample_waveform(pred) draw of the step (src/model.py:338)
        lf.sample_out = e.step_sample; lf.inv_lv = 1.0f / (float)(1 << (p->c.bits - 1));
        lf.seed = e.step_sample_seed; lf.offset = e.step_sample_off;
      }
      lf.row_weight = e.row_weights;                   // armed sample_weight: the weighted instantiation of the epilogue
    }
    rc = forward_core(p, params, inputs, true, cond, B, T, true, ws, L, s, nullptr, fuse ? &lf : nullptr);
    if (rc) return rc;
    if (lf.done && lf.sample_out) e.step_sample = nullptr;     // drawn
    if (e.phase_on) (void)hipEventRecord(e.phase_ev[1], s);
    rc = loss_stage(p, B, T, global_batch, true, ws, L, loss_out, am_GF(nf - 1), s, lf.done, e.row_weights);
    if (rc) return rc;
    rc = emit_outputs(p, ws, L, rows, nullptr, pred_out, s);
    if (rc) return rc;
    if (e.step_sample) {
      // sample_waveform(pred) of this step (src/model.py:338) drawn from the logits while they are still hot:
      // no (rows, C) probability tensor is written or re-read
      float* so = e.step_sample;
      e.step_sample = nullptr;
      if (p->c.head == WN_HEAD_CATEGORICAL) {
        if (e.step_sample_det) {
          wn_set_error("step sample: deterministic categorical draws go through wn_sample_waveform");
          return WN_E_UNSUPPORTED;
        }
        rc = wn_launch_sample_rand_cat_logits(ws + L.logits, rows, p->Cout, p->c.bits, e.step_sample_seed, e.step_sample_off, so, s);
      } else {
        // mixture heads: the model output IS the logits tensor
        if (e.step_sample_det) rc = wn_launch_sample_det(ws + L.logits, rows, p->Cout, p->c.num_mixtures, p->c.bits, so, s);
        else rc = wn_launch_sample_rand(ws + L.logits, rows, p->Cout, p->c.num_mixtures, p->c.bits, p->c.head, e.step_sample_seed, e.step_sample_off, so, s);
      }
      if (rc) return rc;
    }
    // the step's other two scalars are complete here too: the L2 regulariser's loss term (src/model.py:331-334) and the
    // range flag of the forward pass
    if (p->c.l2_reg_factor > 0.f) {
      float* norms = ws + L.loss_rows;   // free by now
      rc = wn_launch_sumsq(params, p->d_kdesc, (int)p->kdesc.size(), norms, s);
      if (rc) return rc;
      rc = wn_launch_sum(norms, (int64_t)p->kdesc.size(), p->c.l2_reg_factor / (float)n_replicas, loss_out + 1, ws + L.sum_scratch, s);
      if (rc) return rc;
    } else {
      rc = wn_launch_fill(loss_out + 1, 0.f, 1, s);
      if (rc) return rc;
    }
    // (with dropout the split kernels read H * mask / (1 - rate) while only H is published: compare against limit * (1 - rate))
    rc = wn_launch_guard_flag(ws + L.fwd_absmax, WN_RANGE_LIMIT * (e.drop_rate > 0.f ? 1.f - e.drop_rate : 1.f),
                              wn_debug_get(1) != 1, loss_out + 2, s);
    if (rc) return rc;
    if (e.phase_on) (void)hipEventRecord(e.phase_ev[2], s);
    return WN_OK;
  }

  // conv_cond of ONE block on the time-invariant mapped condition: dW_c = m^T dcb, db_c = sum_b dcb, g_m += dcb W_c^T
  // (dcb: the Bc sums of this block's g_u, [Bc][ld])
  int cond_block_bwd(const BlockInfo& bi, const float* dcb, int ld) {
    const ConvInfo& c = bi.conv_cond;
    int r = wgrad(mlast, p->Cc, p->Cc, 0, dcb, ld, 2 * p->D, 1, Bc, grads + p->tensors[c.kernel_t].off,
                  grads + p->tensors[c.bias_t].off, nullptr, slab, s);
    if (r) return r;
    return Gemm(1, Bc, p->Cc, ceil32(p->Cc)).seg(dcb, ld, 2 * p->D, 0, fragbase + c.fragB)
        .addc(ws + L.g_m0, p->Cc).run(ws + L.g_m0, p->Cc, s);
  }

  // local conditioning: the per-frame sums of every block's g_u, [Bc][N * 2D] into cbt (wn_cond_frames.hip).  The blocks'
  // own per-utterance sums and the slab gather are the F == 1 paths.
  int frame_sums() {
    const int64_t stride = p->N > 1 ? L.GU[1] - L.GU[0] : 0;
    for (int b = 1; b < p->N; ++b)
      if (L.GU[b] != L.GU[0] + (int64_t)b * stride) { wn_set_error("cond_frame_sum: g_u regions are not evenly spaced"); return WN_E_UNSUPPORTED; }
    return wn_launch_cond_frame_sum(ws + L.GU[0], stride, B, T, F, p->N, 2 * p->D, ws + L.cbt, s);
  }

  // ---- head, last conv first: d loss / d logits (written by the loss stage into GF.back()) down to the skip sum ----
  int head_backward() {
    int rc;
    float* head_out = p->c.use_skip ? ws + L.g_skipsum : ws + L.GH[p->N];
    for (int i = (int)p->finals.size() - 1; i >= (tp.fold ? 1 : 0); --i) {
      const ConvInfo& c = p->finals[i];
      float* dst = (i == 0) ? head_out : ws + L.GF[i - 1];
      // 128 / 256 input channels: the streamed kernel's second form in its backward-data instantiation
      if (c.frag16B >= 0 && wn_debug_get(1) != 1 && Planes::takes(false, c.cin, c.cout, 1, c.cout, c.cin, rows, {c.cout})) {
        rc = Planes(B, T, c.cin).operand(ws + L.GF[i], c.cout, c.cout).w16(fragbase + c.frag16B).act(p->c.activation)
                 .bwd(am_GF(i), i > 0 ? am_GF(i - 1) : (p->c.use_skip ? am_gskip : am_GH(p->N)),
                      i > 0 ? ws + L.HA[i - 1] : nullptr, i > 0 ? c.cin : 0)
                 .run(dst, c.cin, s);
        if (rc) return rc;
        continue;
      }
      Gemm gm(B, T, c.cin, ceil32(c.cin));
      gm.seg(ws + L.GF[i], c.cout, c.cout, 0, fragbase + c.fragB);
      if (i > 0) gm.dact(ws + L.HA[i - 1], c.cin, p->c.activation);
      // (a layer without an image -- 32 or 48 input columns, the 30 outputs of a mixture head -- runs the exact-fp32 kernel,
      // which still owes its result's scale to the layer below and to the weight-gradient jobs)
      if (c.frag16B >= 0) gm.w16(fragbase + c.frag16B);
      gm.absmax(am_GF(i), nullptr, i > 0 ? am_GF(i - 1) : (p->c.use_skip ? am_gskip : am_GH(p->N)));
      rc = gm.run(dst, c.cin, s);
      if (rc) return rc;
    }
    return WN_OK;
  }

  // folded skip path: the gradient of the skip sum is never formed; the blocks contract dL/da = GF[0] with V(b)
  const float* g_skipsum() const { return (p->c.use_skip && !tp.fold) ? ws + L.g_skipsum : nullptr; }

  // what block_backward of block b reads and writes: gradients in the workspace, their max-abs slots (host only)
  BlockGrads block_grads(int b) const {
    const BlockInfo& bi = p->blocks[b];
    const float* g_skip = g_skipsum();
    BlockGrads bg;
    memset(&bg, 0, sizeof(bg));
    bg.defer = true;
    for (int i = 0; i + 1 < p->LPB; ++i) bg.g_pi[i] = ws + L.GP[b][i];
    if (tp.deep16)
      for (int i = 0; i + 1 < p->LPB; ++i) bg.am_gp[i] = am_GP(b, i);
    if (tp.drop) {
      bg.drop_rate = e.drop_rate; bg.drop_key = wn_dropout_key(e.drop_seed, b, e.drop_step); bg.g_xd = ws + L.gxd;
    }
    // the last block's output gradient is identically zero when the head reads the skip sum
    // (with the skip head nothing flows into the last block's output: GH[N] was zero-filled above.  It is
    //  still passed as a gradient -- unless S == 0, where g_o is assembled from g_skip alone -- so that
    //  the last block runs the same split-precision kernels as the others instead of the fp32 fallback
    //  for the one-segment product)
    bg.g_xout = (p->c.use_skip && b == p->N - 1 && p->S == 0) ? nullptr : ws + L.GH[b + 1];
    bg.g_skip = g_skip;
    bg.g_o_tmp = p->S == 0 ? ws + L.GO[b] : nullptr;
    bg.g_u = ws + L.GU[b];
    bg.g_x = tp.bwd_pairs() ? nullptr : ws + L.GH[b];     // (pairs: the next launch forms g_x of this block)
    bg.dcb = (bi.has_cond && !cond_batched && F == 1) ? ws + L.dcb : nullptr;
    bg.slab = slab;
    bg.am_gxout = bg.g_xout ? am_GH(b + 1) : nullptr;
    bg.am_gskip = g_skip ? am_gskip : nullptr;
    bg.am_gu = am_GU(b); bg.am_gx = am_GH(b);
    if (tp.fold) { bg.g_fold = ws + L.GF[0]; bg.fold_F0 = p->fold_F0; bg.am_gfold = am_GF(0); }
    return bg;
  }

  // ---- residual blocks, last to first: data gradients only, every g_u / g_x is kept for the deferred weight gradients ----
  int chain_backward() {
    int rc;
    const float* g_skip = g_skipsum();
    if (p->c.use_skip) {
      rc = wn_launch_fill(ws + L.GH[p->N], 0.f, rows * p->R, s);   // nothing flows into the last block output
      if (rc) return rc;
    }
    // Two products per launch (wn_bwd_pair.hip): g_x(b+1) and, from it in registers, g_u(b).  The chain is then
    //   g_u(N-1) | { g_x(b+1), g_u(b) } for b = N-2 .. 0 | g_x(0)   = N + 1 launches instead of 2 N.
    const bool pairk = tp.bwd_pairs();
    for (int b = p->N - 1; b >= 0; --b) {
      BlockPtrs k = block_ptrs(p, b, params, fragbase, B, T);
      deep16_ptrs(p, b, fragbase, k);
      const BlockInfo& bi = p->blocks[b];
      const BlockBufs f = block_bufs(p, L, ws, b, rows, true, tp.drop);   // where the forward pass saved them
      if (pairk && b < p->N - 1) {
        const BlockPtrs k1 = block_ptrs(p, b + 1, params, fragbase, B, T);
        WnBwdPairArgs a;
        memset(&a, 0, sizeof(a));
        a.gu_in = ws + L.GU[b + 1]; a.gx_res = ws + L.GH[b + 2]; a.gf = ws + L.GF[0];
        a.ag = f.AG; a.z = f.Z; a.ldz = f.ldz;
        a.gx_out = ws + L.GH[b + 1]; a.gu_out = ws + L.GU[b];
        a.wx16 = k1.G16x; a.wu16 = k.G16uf;
        a.am_gu_in = am_GU(b + 1); a.am_gf = am_GF(0); a.am_gx = am_GH(b + 1); a.am_gu = am_GU(b);
        a.B = B; a.T = T; a.dil = k1.dil[0];
        if (!a.wx16 || !a.wu16) { wn_set_error("bwd_pair: weight images missing"); return WN_E_UNSUPPORTED; }
        rc = tp.bwd == BWD_S128 ? wn_launch_bwd_s128(a, s) : wn_launch_bwd_pair(a, s);
        if (rc) return rc;
        if (b == 0) {
          // g_x(0): the gradient at the first block's input (only the input conv's weight gradients need it)
          Gemm gm(B, T, p->R, ceil32(p->R));
          for (int t = 0; t < p->KS; ++t)
            gm.seg(ws + L.GU[0], 2 * p->D, 2 * p->D, -(p->KS - 1 - t) * k.dil[0], k.Bd[0] + t * k.Bd_stride[0]);
          if (p->c.use_residual) gm.addc(ws + L.GH[1], p->R);
          gm.w16(k.G16x).absmax(am_GU(0), nullptr, am_GH(0));
          rc = gm.run(ws + L.GH[0], p->R, s);
          if (rc) return rc;
        }
        continue;
      }
      const BlockGrads bg = block_grads(b);
      rc = block_backward(k, f, bg, s);
      if (rc) return rc;
      if (p->S == 0 && bg.g_xout == nullptr && g_skip) {
        // g_o == g_skip for this block: the job table reads GO[b]
        WN_HIP_CHECK(hipMemcpyAsync(ws + L.GO[b], g_skip, rows * p->R * sizeof(float), hipMemcpyDeviceToDevice, s));
      }
      if (bi.has_cond && !cond_batched && F == 1) {
        rc = cond_block_bwd(bi, ws + L.dcb, 2 * p->D);
        if (rc) return rc;
      }
    }
    if (F > 1 && p->c.cond_inputs > 0 && !cond_batched) {
      // frames: every block's sums in one launch behind the chain, then the per-block products on their columns of cbt
      if ((rc = frame_sums())) return rc;
      for (int b = p->N - 1; b >= 0; --b)
        if (p->blocks[b].has_cond && (rc = cond_block_bwd(p->blocks[b], ws + L.cbt + (int64_t)b * 2 * p->D, p->N * 2 * p->D))) return rc;
    }
    return WN_OK;
  }

  // folded skip path: M = Z^T dL/da -> dW_s, db_s of every block and dW_f0, db_f0 (three small weight-space products)
  int fold_weight_gradients() {
    // M = Z^T dL/da and colsum(dL/da) are in their slab (the schedule's last span): reduced, then the three small products
    const int F0 = p->fold_F0;
    int rc = wn_launch_reduce_table(ws + L.mslab, B * L.bsplits, pm, ws + L.mtot, p->d_cov_fold, 1, s, &p->h_cov_fold);
    if (rc) return rc;
    // Y = [M; colsum] W_f0^T -> dW_s of every block and db_s;  dW_f0 = [W_s(all); sum b_s]^T [M; colsum];  db_f0 = colsum
    const ConvInfo& c0 = p->finals[0];
    const int nd1 = p->N * p->D + 1;
    const float* wf0 = params + p->tensors[c0.kernel_t].off;          // (1, S, F0): W_f0[s][n]
    rc = wn_launch_sgemm_small(ws + L.mtot, F0, 1, wf0, 1, F0, ws + L.ytmp, p->S, nd1, p->S, F0, s);          // B[k = n][j = s]
    if (rc) return rc;
    // (a long-K product with a small output: the rows-contraction kernel splits K over workgroups)
    // split K in chunks of 128 on the small-product kernel, partial results in the (idle) slab, summed in chunk order
    // (wn_wgrad_kernel when the slab is too small for them)
    const int nzk = (nd1 + 127) / 128;
    if ((int64_t)nzk * p->S * F0 <= L.slab_floats) {
      rc = wn_launch_sgemm_small_batched(ws + L.wsall, 1, p->S, (int64_t)128 * p->S, ws + L.mtot, F0, 1, (int64_t)128 * F0, slab, F0,
                                         (int64_t)p->S * F0, p->S, F0, nd1, nzk, nullptr, 0, s, 128);
      if (rc) return rc;
      WnVecSumArgs v;
      v.base = slab; v.off0 = 0; v.stride = (int64_t)p->S * F0; v.count = nzk; v.len = p->S * F0;
      v.out = grads + p->tensors[c0.kernel_t].off;
      rc = wn_launch_vecsum(v, s);
    } else
    rc = wgrad(ws + L.wsall, p->S, p->S, 0, ws + L.mtot, F0, F0, 1, nd1, grads + p->tensors[c0.kernel_t].off, nullptr, nullptr,
               slab, s);
    if (rc) return rc;
    return wn_launch_skip_scatter(ws + L.ytmp, ws + L.mtot + (int64_t)p->N * p->D * F0, skip_w.off, skip_w.stride, skip_b.off,
                                  skip_b.stride, p->tensors[c0.bias_t].off, p->N, p->D, p->S, F0, grads, s);
  }

  // global conditioning of all blocks as one layer: per-utterance sums of d u out of the weight-gradient slab, g_m, dW_c, db_c
  int cond_weight_gradients() {
    int rc;
    const int D2 = 2 * p->D;
    const BlockInfo& b0 = p->blocks[0]; const BlockInfo& b1 = p->blocks[p->N > 1 ? 1 : 0];
    const Strided db = strided(b0.dil.back().bias_t, b1.dil.back().bias_t);
    const Strided cw = strided(b0.conv_cond.kernel_t, b1.conv_cond.kernel_t), cbi = strided(b0.conv_cond.bias_t, b1.conv_cond.bias_t);
    rc = F > 1 ? frame_sums()
               : wn_launch_cond_gather(ws + L.bslab, p->nparams, L.bsplits, db.off, db.stride, B, p->N, D2, ws + L.cbt, s);
    if (rc) return rc;
    if (cond_small(p) && (int64_t)p->N * Bc * p->Cc <= L.slab_floats) {
      // g_m = sum_z dcb_z W_c(z)^T: one product per block into the (idle) slab, then their sum
      rc = wn_launch_sgemm_small_batched(ws + L.cbt, p->N * D2, 1, D2, params + cw.off, 1, D2, cw.stride,
                                         slab, p->Cc, (int64_t)Bc * p->Cc, Bc, p->Cc, D2, p->N, nullptr, 0, s);
      if (rc) return rc;
      WnVecSumArgs v;
      v.base = slab; v.off0 = 0; v.stride = (int64_t)Bc * p->Cc; v.count = p->N; v.len = Bc * p->Cc; v.out = ws + L.g_m0;
      rc = wn_launch_vecsum(v, s);
    } else
    rc = Gemm(1, Bc, p->Cc, ceil32(p->Cc)).seg(ws + L.cbt, p->N * D2, p->N * D2, 0, fragbase + p->frag_condB).run(ws + L.g_m0, p->Cc, s);
    if (rc) return rc;
    // dW_c, db_c: one thread per element walks the condition rows (wn_cond_wgrad_kernel) -- written for a handful of
    // utterances.  With frames the rows are B * F: the generic weight-gradient product per block, as cond_block_bwd takes it
    if (F > 1) {
      for (int b = 0; b < p->N; ++b) {
        const ConvInfo& c = p->blocks[b].conv_cond;
        rc = wgrad(mlast, p->Cc, p->Cc, 0, ws + L.cbt + (int64_t)b * D2, p->N * D2, D2, 1, Bc, grads + p->tensors[c.kernel_t].off,
                   grads + p->tensors[c.bias_t].off, nullptr, slab, s);
        if (rc) return rc;
      }
      return WN_OK;
    }
    return wn_launch_cond_wgrad(mlast, ws + L.cbt, B, p->Cc, p->N, D2, grads, cw.off, cw.stride, cbi.off, cbi.stride, s);
  }

  // one launch of the schedule
  int launch(const WgSpan& sp, hipStream_t st) {
    const WgSchedule& g = e.wg;
    float* out = ws + L.bslab; int64_t pitch = p->nparams; int splits = L.bsplits;
    if (sp.slab == WgSpan::HEAD) { out = ws + L.hslab - L.head_base; pitch = L.head_span; splits = L.hsplits; }
    if (sp.slab == WgSpan::MFOLD) { out = ws + L.mslab; pitch = pm; }
    switch (sp.op) {
      case WgSpan::INCONV:
        return wn_launch_inconv_wgrad(inputs, ws + L.GH[0], B, T, p->R, p->KS, L.isplits, ws + L.islab, (int64_t)(p->KS + 1) * p->R,
                                      0, (int64_t)p->KS * p->R, st);
      case WgSpan::JOBS: return wn_launch_wgrad_batched(g.jobs.d + sp.first, sp.count, ws, out, pitch, B, T, splits, st, sp.kind != 0);
      case WgSpan::PAIRS: return wn_launch_wgrad_pairs(sp.kind, g.pairs.d + sp.first, sp.count, ws, out, pitch, B, T, splits, st);
      case WgSpan::TR:        // (kind 6: M into its own slab beside dW_r; kind 7: dW_r into the batched slab beside M)
        return wn_launch_wgrad_tr(sp.kind, g.pairs.d + sp.first, sp.count, ws, out, pitch, B, T, splits, st,
                                  sp.kind == 6 ? ws + L.mslab : (sp.kind == 7 ? ws + L.bslab : nullptr),
                                  sp.kind == 6 ? pm : (sp.kind == 7 ? p->nparams : 0));
      case WgSpan::LAYERS: return wn_launch_wgrad_layers(sp.kind == 1 ? g.inner.d : g.layers.d, sp.count, p->R, ws, out, pitch, B, T, splits, st, sp.kind);
      case WgSpan::SKIP:
        if (sp.slab == WgSpan::MFOLD)
          return wn_launch_wgrad_skip(ws + L.Z, p->Dp, ws + L.GF[0], p->fold_F0, rows, p->N * p->D, p->fold_F0, p->D, B * splits, out, pitch,
                                      0, (int64_t)p->D * p->fold_F0, (int64_t)p->N * p->D * p->fold_F0, 0, 1, am_GF(0), st);
        return wn_launch_wgrad_skip(ws + L.Z, p->Dp, ws + L.g_skipsum, p->S, rows, p->N * p->D, p->S, p->D, B * splits, out, pitch,
                                    skip_w.off, skip_w.stride, skip_b.off, skip_b.stride, p->N, am_gskip, st);
    }
    return WN_E_INVALID;
  }

  // ---- every weight gradient of the step: the schedule's low-occupancy leftovers (input conv, head) on a side stream
  //      beside the per-block kernels on the caller's, then the slab reductions into the flat gradient ----
  int weight_gradients() {
    int rc;
    const WgSchedule& g = e.wg;
    if (e.phase_on) (void)hipEventRecord(e.phase_ev[3], s);      // backward-data chain done
    // the side spans run on disjoint slab regions and are joined before the reduce.
    // knob 9 = 1 keeps everything on the caller's stream (A/B of the overlap).
    const bool fork = g.overlap && wn_debug_get(9) != 1;
    if (fork && !e.side) {
      WN_HIP_CHECK(hipStreamCreateWithFlags(&e.side, hipStreamNonBlocking));
      WN_HIP_CHECK(hipEventCreateWithFlags(&e.ev_fork, hipEventDisableTiming));
      WN_HIP_CHECK(hipEventCreateWithFlags(&e.ev_join, hipEventDisableTiming));
    }
    // Whatever happens after the fork, the caller's stream must not run ahead of the side stream's kernels (they
    // read and write the workspace and the gradient slab): an early error return joins through this guard.
    struct SideJoin {
      wn_exec& e; hipStream_t s; bool armed;
      ~SideJoin() {
        if (!armed) return;
        if (hipEventRecord(e.ev_join, e.side) != hipSuccess || hipStreamWaitEvent(s, e.ev_join, 0) != hipSuccess)
          (void)hipStreamSynchronize(e.side);
      }
    } side_join{e, s, false};
    if (fork) {
      WN_HIP_CHECK(hipEventRecord(e.ev_fork, s));
      WN_HIP_CHECK(hipStreamWaitEvent(e.side, e.ev_fork, 0));
      side_join.armed = true;
    }
    size_t i = 0;
    for (; i < (size_t)g.n_side; ++i)
      if ((rc = launch(g.spans[i], fork ? e.side : s))) return rc;
    if (fork) WN_HIP_CHECK(hipEventRecord(e.ev_join, e.side));
    for (; i < g.spans.size(); ++i)
      if ((rc = launch(g.spans[i], s))) return rc;
    if (tp.fold && (rc = fold_weight_gradients())) return rc;
    if (fork) { WN_HIP_CHECK(hipStreamWaitEvent(s, e.ev_join, 0)); side_join.armed = false; }
    if (cond_batched && (rc = cond_weight_gradients())) return rc;
    // coverage entries 0, 1 are the input conv's kernel and bias: from their compact slab when the dedicated kernel ran;
    // the head's entries come last: from the head's slab when it has one
    const int cov0 = tp.in_split ? 2 : 0, ncov = (int)g.h_cov.size(), cov1 = g.cov_head;
    rc = wn_launch_reduce_table(ws + L.bslab, B * L.bsplits, p->nparams, grads, g.cov.d + cov0, cov1 - cov0, s, g.h_cov.data() + cov0);
    if (rc) return rc;
    if (tp.in_split && (rc = wn_launch_reduce_table(ws + L.islab, B * L.isplits, (int64_t)(p->KS + 1) * p->R, grads, g.cov.d, 2, s, g.h_cov.data())))
      return rc;
    if (cov1 < ncov && (rc = wn_launch_reduce_table(ws + L.hslab - L.head_base, B * L.hsplits, L.head_span, grads, g.cov.d + cov1, ncov - cov1,
                                                    s, g.h_cov.data() + cov1)))
      return rc;
    if (!p->c.use_skip && p->S > 0) {
      for (const BlockInfo& bi : p->blocks) {     // unused skip convs: zero gradients
        rc = wn_launch_fill(grads + p->tensors[bi.conv_skip.kernel_t].off, 0.f, p->tensors[bi.conv_skip.kernel_t].len, s);
        if (!rc) rc = wn_launch_fill(grads + p->tensors[bi.conv_skip.bias_t].off, 0.f, p->tensors[bi.conv_skip.bias_t].len, s);
        if (rc) return rc;
      }
    }
    return WN_OK;
  }

  int mapping_backward() {
    int rc;
    // ---- mapping Dense stack backward ----
    if (p->c.cond_inputs > 0) {
      const float* gm_cur = ws + L.g_m0;      // gradient w.r.t. post-activation output of the last Dense
      float* gm_other = ws + L.g_m1;
      if (g_cond && p->mapping.empty())       // the blocks read the condition itself
        WN_HIP_CHECK(hipMemcpyAsync(g_cond, gm_cur, (int64_t)Bc * p->Cc * sizeof(float), hipMemcpyDeviceToDevice, s));
      for (int j = (int)p->mapping.size() - 1; j >= 0; --j) {
        const ConvInfo& c = p->mapping[j];
        const float* yin = (j == 0) ? cond : ws + L.M[j - 1];
        // pre-activation gradient g_pre = g * act'(M[j])  (tiny: B x width)
        rc = wn_launch_dact_mul(gm_cur, ws + L.M[j], gm_other, (int64_t)Bc * c.cout, p->c.mapping_activation, s);
        if (rc) return rc;
        if (j == 0 && g_cond) {   // wn_vjp: the gradient at the condition, g_pre W_0^T (B x cond_inputs)
          rc = wn_launch_sgemm_small_batched(gm_other, c.cout, 1, 0, params + p->tensors[c.kernel_t].off, 1, c.cout, 0, g_cond, c.cin, 0,
                                             Bc, c.cin, c.cout, 1, nullptr, 0, s);
          if (rc) return rc;
        }
        // (the small form's bias sum is one thread per column walking the rows: for the handful of rows of global conditioning)
        if (cond_small(p) && F == 1) {
          // dW = yin^T g_pre (cin x cout, contraction over the B utterances), db = column sums of g_pre
          rc = wn_launch_sgemm_small_batched(yin, 1, c.cin, 0, gm_other, c.cout, 1, 0, grads + p->tensors[c.kernel_t].off, c.cout, 0,
                                             c.cin, c.cout, B, 1, nullptr, 0, s);
          if (rc) return rc;
          WnVecSumArgs v;
          v.base = gm_other; v.off0 = 0; v.stride = c.cout; v.count = B; v.len = c.cout; v.out = grads + p->tensors[c.bias_t].off;
          rc = wn_launch_vecsum(v, s);
          if (rc) return rc;
          if (j > 0) {          // g_in = g_pre W^T
            float* dst = const_cast<float*>(gm_cur);
            rc = wn_launch_sgemm_small_batched(gm_other, c.cout, 1, 0, params + p->tensors[c.kernel_t].off, 1, c.cout, 0, dst, c.cin, 0,
                                               B, c.cin, c.cout, 1, nullptr, 0, s);
            if (rc) return rc;
          }
          continue;
        }
        rc = wgrad(yin, c.cin, c.cin, 0, gm_other, c.cout, c.cout, 1, Bc, grads + p->tensors[c.kernel_t].off,
                   grads + p->tensors[c.bias_t].off, nullptr, slab, s);
        if (rc) return rc;
        if (j > 0) {
          float* dst = const_cast<float*>(gm_cur);
          rc = Gemm(1, Bc, c.cin, ceil32(c.cin)).seg(gm_other, c.cout, c.cout, 0, fragbase + c.fragB).run(dst, c.cin, s);
          if (rc) return rc;
        }
      }
    }
    return WN_OK;
  }

  // ---- the backward pass from d / d logits in GF.back() (max-abs in am_GF(nf - 1)): of a loss of the step, or a caller's ----
  int backward_from_logits() {
    int rc;
    fragbase = ws + L.frag;
    slab = ws + L.slab;
    if (p->c.cond_inputs > 0) {
      mlast = p->mapping.empty() ? cond : ws + L.M.back();
      rc = wn_launch_fill(ws + L.g_m0, 0.f, (int64_t)Bc * p->Cc, s);
      if (rc) return rc;
    }
    // conditioning of all blocks as one layer: the per-utterance sums of d u come out of the weight-gradient
    // slab afterwards instead of 2 column-sum launches + 3 tiny products per block
    cond_batched = p->frag_condB >= 0;
    tp = train_paths(p, e, L, rows);               // (fold: the forward pass of this call made the same decision)
    pm = (int64_t)p->N * p->D * p->fold_F0 + p->fold_F0;
    if (p->blocks[0].has_skip) {
      const BlockInfo& b0 = p->blocks[0]; const BlockInfo& b1 = p->blocks[p->N > 1 ? 1 : 0];
      skip_w = strided(b0.conv_skip.kernel_t, b1.conv_skip.kernel_t); skip_b = strided(b0.conv_skip.bias_t, b1.conv_skip.bias_t);
    }
    rc = ensure_schedule(p, e, L, B, T, tp);
    if (rc) return rc;
    if ((rc = head_backward())) return rc;
    if ((rc = chain_backward())) return rc;
    if ((rc = weight_gradients())) return rc;
    if ((rc = mapping_backward())) return rc;
    // the input conv's data gradient: GH[0] is formed by every chain (only wn_vjp asks for it)
    if (g_x)
      return wn_launch_inconv_bwd_data(ws + L.GH[0], params + p->tensors[p->causal.kernel_t].off, B, T, p->R, p->KS, g_x, s);
    return WN_OK;
  }

  int backward() {
    int rc = backward_from_logits();
    if (rc) return rc;
    // ---- L2 regulariser, src/model.py:331-334: its gradient (the loss term is formed with the loss, above) ----
    if (p->c.l2_reg_factor > 0.f) {
      rc = wn_launch_axpy_table(grads, params, p->d_kdesc, (int)p->kdesc.size(), 2.0f * p->c.l2_reg_factor / (float)n_replicas, s);
      if (rc) return rc;
    }
    if (e.phase_on) {
      (void)hipEventRecord(e.phase_ev[4], s);
    }

    return WN_OK;
  }
};

}  // namespace

extern "C" int wn_plan_set_train_phases(wn_plan* p, int32_t phases) {
  if (!p || phases < 1 || phases > 3) { wn_set_error("set_train_phases: 1 (forward + loss), 2 (backward), 3 (both)"); return WN_E_INVALID; }
  wnp::ex(p).train_phases = phases;
  return WN_OK;
}

extern "C" int wn_train_fwd_bwd(wn_plan* p, const float* params, const float* x_full, const float* cond,
                                int32_t B, int32_t T, int32_t global_batch, int32_t n_replicas, float* grads,
                                float* loss_out, float* pred_out, float* workspace, int64_t ws_floats,
                                void* stream) {
  if (!p || !params || !x_full || !workspace || !loss_out || !grads || B < 1 || T < 1) { wn_set_error("train_fwd_bwd: bad arguments"); return WN_E_INVALID; }
  if (wnp::row_weights_check("train_fwd_bwd", wnp::ex(p), B, T)) return WN_E_INVALID;
  if (wnp::cond_frames_check("train_fwd_bwd", p, T) < 0) return WN_E_INVALID;
  TrainCall c{wnp::ex(p)};
  c.bind(p, params, cond, B, T, grads, workspace, (hipStream_t)stream);
  c.x_full = x_full;
  c.global_batch = global_batch > 0 ? global_batch : B;
  c.n_replicas = n_replicas > 0 ? n_replicas : 1;
  c.loss_out = loss_out; c.pred_out = pred_out;
  if (ws_floats < c.L.total) { wn_set_error("train_fwd_bwd: workspace too small (%lld < %lld floats)", (long long)ws_floats, (long long)c.L.total); return WN_E_INVALID; }
  // A caller may run the step as two calls (wn_plan_set_train_phases 1, then 2) and queue work of its own in between --
  // the Python mirror reads the loss and the metrics back from there, 4 ms before the step ends.  Everything the second
  // half needs lives in the workspace.
  const int phases = c.e.train_phases;
  int rc = WN_OK;
  if (phases & 1) rc = c.forward_and_loss();
  if (!rc && (phases & 2)) rc = c.backward();
  return rc;
}

// Backward pass from a caller's gradient at the network output (include/wn_hip.h): the saved activations of the
// wn_forward_training call before it are in the workspace; the seed kernel stands where the loss stage stands in a step.
extern "C" int wn_vjp(wn_plan* p, const float* params, const float* x, const float* cond, int32_t B, int32_t T,
                      const float* g_out, int32_t g_kind, float* grads, float* g_x, float* g_cond,
                      float* workspace, int64_t ws_floats, void* stream) {
  if (!p || !params || !x || !g_out || !grads || !workspace) { wn_set_error("vjp: bad arguments (null plan, params, x, g_out, grads or workspace)"); return WN_E_INVALID; }
  if (B < 1 || T < 1) { wn_set_error("vjp: B and T must be >= 1 (got %d, %d)", (int)B, (int)T); return WN_E_INVALID; }
  if (g_kind != 0 && g_kind != 1) { wn_set_error("vjp: g_kind must be 0 (network output) or 1 (logits) (got %d)", (int)g_kind); return WN_E_INVALID; }
  if (p->c.cond_inputs > 0 && !cond) { wn_set_error("vjp: the plan is conditioned and cond is null"); return WN_E_INVALID; }
  if (p->c.cond_inputs <= 0 && g_cond) { wn_set_error("vjp: g_cond on a plan without conditioning"); return WN_E_INVALID; }
  if (B >= 1 && T >= 1 && wnp::cond_frames_check("vjp", p, T) < 0) return WN_E_INVALID;
  TrainCall c{wnp::ex(p)};
  c.bind(p, params, cond, B, T, grads, workspace, (hipStream_t)stream);
  c.g_x = g_x; c.g_cond = g_cond;
  if (ws_floats < c.L.total) { wn_set_error("vjp: workspace too small (%lld < %lld floats)", (long long)ws_floats, (long long)c.L.total); return WN_E_INVALID; }
  hipStream_t s = c.s;
  // the weight-gradient schedule reads the input waveform from the workspace (a training step's shift_split leaves it there)
  WN_HIP_CHECK(hipMemcpyAsync(c.inputs, x, c.rows * sizeof(float), hipMemcpyDeviceToDevice, s));
  // (the forward pass without a fused loss writes none of these slots)
  WN_HIP_CHECK(hipMemsetAsync(c.am, 0, c.L.n_absmax * sizeof(float), s));
  const int rc = wn_launch_vjp_seed(workspace + c.L.logits, g_out, c.rows, p->Cout,
                                    g_kind == 0 && p->c.head == WN_HEAD_CATEGORICAL, workspace + c.L.GF.back(), c.am_GF(c.nf - 1), s);
  if (rc) return rc;
  return c.backward_from_logits();
}

// block_fwd_path / block_bwd_path of block 0 as a model pass over B x T rows binds it, under the calling thread's knobs,
// without dropout: one `name=value` token per decision, the convs of the stack in order (host only: the pointers are
// offsets from a placeholder and never dereferenced)
extern "C" int wn_debug_block_paths(const wn_plan* p, int32_t B, int32_t T, int32_t training, char* buf, int32_t len) {
  if (!p || !buf || len < 1 || B < 1 || T < 1) return WN_E_INVALID;
  static float placeholder[4];
  float* const base = placeholder;
  wn_exec none;                       // (a state of its own: no dropout)
  TrainCall c{none};
  c.bind(const_cast<wn_plan*>(p), base, base, B, T, base, base, nullptr);
  c.fragbase = base + c.L.frag; c.slab = base + c.L.slab;
  c.cond_batched = p->frag_condB >= 0;
  c.tp = train_paths(p, none, c.L, c.rows);
  static const char* const conv[] = {"planes", "rows16", "rows32"};
  static const char* const gate[] = {"s128", "two", "fused16", "fused32", "composed"};
  static const char* const go[] = {"xout", "sum", "skip"};
  static const char* const gu[] = {"fold", "pad", "image", "fp32", "zero"};
  static const char* const am[] = {"none", "gxout", "gskip", "gfold"};
  static const char* const gx[] = {"none", "g16x", "deep", "fp32+absmax", "fp32"};
  auto list = [&](const BlkConv* v, int first, int end) {
    std::string t;
    for (int i = first; i < end; ++i) t += std::string(t.empty() ? "" : ",") + conv[v[i]];
    return t.empty() ? std::string("none") : t;
  };
  // forward: FwdCall::blocks()
  const FwdPaths fp = fwd_paths(p, none, B, T, training != 0, true, false, FWD_LOSS_NONE);
  const WsLayout Lf = training ? c.L : make_layout(p, B, T, false);
  BlockPtrs k = block_ptrs(p, 0, base, base + Lf.frag, B, T);
  if (fp.deep16) deep16_ptrs(p, 0, base + Lf.frag, k);
  if (fp.cond != FWD_COND_NONE) k.cb = base + Lf.cb;
  const BlockFwdPath f = block_fwd_path(k, block_bufs(p, Lf, base, 0, c.rows, training != 0, false));
  std::string out = "inner=" + list(f.inner, 0, f.ninner) + " gate=" + gate[f.gate];
  if (training) {
    // backward: TrainCall::chain_backward()
    BlockPtrs kb = block_ptrs(p, 0, base, c.fragbase, B, T);
    deep16_ptrs(p, 0, c.fragbase, kb);
    const BlockBwdPath b = block_bwd_path(kb, block_bufs(p, c.L, base, 0, c.rows, true, false), c.block_grads(0));
    out += std::string(" go=") + go[b.go] + " gu=" + gu[b.gu] + " gu_pad=" + (b.gu_pad ? "1" : "0") + " gu_am=" + am[b.gu_am[0]] + "," +
           am[b.gu_am[1]] + " data=" + list(b.data, 1, p->LPB) + " gx=" + gx[b.gx] + " drop=" + (b.drop ? "1" : "0");
  }
  snprintf(buf, (size_t)len, "%s", out.c_str());
  return WN_OK;
}
