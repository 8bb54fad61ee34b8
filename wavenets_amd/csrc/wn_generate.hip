// ==========================================================================================
// generation: WaveNet.generate / _generation, src/model.py:241-307 (intended semantics:
// SURVEY.md section 9 item 8 -- the reference's bad kwarg / rank bugs are not reproduced)
// ==========================================================================================
#include "wn_plan_internal.h"

using namespace wnp;

namespace {

__global__ void wn_gen_shift_kernel(const float* win, const float* sample, int B, int RF, float* win_next,
                                    float* out, int length, int step) {
  const int64_t n = (int64_t)B * RF;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int b = (int)(i / RF), t = (int)(i % RF);
    win_next[i] = (t == RF - 1) ? sample[b] : win[i + 1];
    if (t == RF - 1) out[(int64_t)b * length + step] = sample[b];
  }
}

__global__ void wn_gather_last_kernel(const float* logits, int B, int RF, int C, float* last) {
  const int64_t n = (int64_t)B * C;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int b = (int)(i / C), c = (int)(i % C);
    last[i] = logits[((int64_t)b * RF + (RF - 1)) * C + c];
  }
}

}  // namespace

namespace {

struct GenLayout {
  int64_t prime;                       // priming forward workspace (make_layout(B, RF, inference))
  int64_t win0, win1, last, lastp, samp;
  int64_t guard;                       // range guard of the call: running max-abs of every input of a split-precision kernel
                                       // (+ 1: the relay's give-up word, see wn_gen_relay128_kernel)
  int64_t relay;                       // granule areas of the 128-channel relay, or < 0
  int64_t xin;                         // [KS][B]
  std::vector<int64_t> ring;           // per block [nslots][B][R]: inputs of the first dilated conv
  std::vector<int> nslots;
  std::vector<std::vector<int64_t>> ringp;   // layers_per_block > 1: inputs of dilated conv i + 1, [nslots][B][D]
  std::vector<std::vector<int>> nslots_p;
  int64_t Zrow, skiprow, hrow0, hrow1, dummy;   // per-step rows
  int64_t u0;                          // fused step: partial accumulators of all blocks
  std::vector<int64_t> HArow;
  int64_t total;
};

GenLayout gen_layout(const wn_plan* p, int B, bool queued) {
  GenLayout G;
  Carver cv;
  const int RF = wn_plan_receptive_field(p);
  G.prime = cv.take(make_layout(p, B, RF, false).total);
  G.win0 = cv.take((int64_t)B * RF);
  G.win1 = cv.take((int64_t)B * RF);
  G.last = cv.take((int64_t)B * p->Cout);
  G.lastp = cv.take((int64_t)B * p->Cout);
  G.samp = cv.take(B);
  G.guard = cv.take(2);
  G.relay = -1;
  G.xin = G.Zrow = G.skiprow = G.hrow0 = G.hrow1 = G.dummy = G.u0 = 0;
  if (queued) {
    G.xin = cv.take((int64_t)p->KS * B);
    for (int b = 0; b < p->N; ++b) {
      const int ns = (p->KS - 1) * p->blocks[b].dil.front().dil + 1;
      G.nslots.push_back(ns);
      G.ring.push_back(cv.take((int64_t)ns * B * p->R));
      G.ringp.emplace_back();
      G.nslots_p.emplace_back();
      for (int i = 1; i < p->LPB; ++i) {
        const int nsi = (p->KS - 1) * p->blocks[b].dil[i].dil + 1;
        G.nslots_p.back().push_back(nsi);
        G.ringp.back().push_back(cv.take((int64_t)nsi * B * p->D));
      }
    }
    G.Zrow = cv.take((int64_t)B * p->N * p->Dp);
    G.skiprow = cv.take((int64_t)B * p->Hin);
    G.hrow0 = cv.take((int64_t)B * p->R);
    G.hrow1 = cv.take((int64_t)B * 2 * p->D);
    G.dummy = cv.take((int64_t)B * p->R);
    G.u0 = cv.take(wn_gen_u0_floats(B, p->N, p->D));
    if (p->LPB == 1 && wn_gen_chain128_supported(p->R, p->D, p->KS)) G.relay = cv.take(wn_gen_relay128_floats(B, p->N));
    for (size_t i = 0; i + 1 < p->finals.size(); ++i) G.HArow.push_back(cv.take((int64_t)B * p->finals[i].cout));
  }
  G.total = cv.pos;
  return G;
}

__global__ void wn_gen_emit_kernel(const float* samp, int B, float* out, int length, int step, float* xin_slot) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  out[(int64_t)b * length + step] = samp[b];
  if (xin_slot) xin_slot[b] = samp[b];
}

// sample from the logits rows [B][Cout] (src/model.py:253-255 + sample_waveform)
int sample_rows(wn_plan* p, const float* logits_rows, int B, bool deterministic, uint64_t seed, uint64_t step,
                float* probs_tmp, float* samp, hipStream_t s, WnSampleCtl ctl, const WnSampleRow* tab = nullptr,
                const uint64_t* origin = nullptr) {
  const float* pred = logits_rows;
  int rc;
  if (p->c.head == WN_HEAD_CATEGORICAL) {
    rc = wn_launch_softmax(logits_rows, probs_tmp, B, p->Cout, s);     // the model output is probabilities
    if (rc) return rc;
    pred = probs_tmp;
  }
  if (deterministic) return wn_launch_sample_det(pred, B, p->Cout, p->c.num_mixtures, p->c.bits, samp, s);
  return wn_launch_sample_rand(pred, B, p->Cout, p->c.num_mixtures, p->c.bits, p->c.head, seed, step, samp, s, ctl, WN_EMIT_NONE, tab, origin);
}

// the compute units of the current device (-1: unknown)
int device_cu_count() {
  static const int n = [] {
    int dev = 0, v = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) v = -1;
    return v;
  }();
  return n;
}

// the cached block table of e: rebuilt when (B, chain128) is not the key it was built for
int ensure_gen_table(const wn_plan* p, wn_exec& e, const GenLayout& G, const WsLayout& L, int B, bool chain128) {
  GenTable& t = e.gen;
  if (t.valid && t.B == B && t.chain128 == chain128) return WN_OK;
  std::vector<WnGenBlock> tab(p->N);
  for (int b = 0; b < p->N; ++b) {
    const BlockInfo& bi = p->blocks[b];
    WnGenBlock& g = tab[b];
    g.ring_off = G.ring[b];
    g.w16d_off = G.prime + L.frag + (chain128 ? bi.f16nat : bi.dil.back().frag16);
    g.w16r_off = G.prime + L.frag + bi.conv1.frag16;
    g.bias_d_off = p->tensors[bi.dil.back().bias_t].off;
    g.bias_r_off = p->tensors[bi.conv1.bias_t].off;
    g.cb_off = p->c.cond_inputs > 0 ? G.prime + L.cb + (int64_t)b * B * 2 * p->D : -1;
    g.nslots = G.nslots[b];
    g.dilation = bi.dil.back().dil;
  }
  t.valid = false;
  const int rc = t.blocks.upload(tab);
  if (rc) return rc;
  for (int b = 0; b < 3; ++b) t.blk0[b] = tab[std::min(b, p->N - 1)];
  // conv1 biases at a uniform stride (every block has the same tensors): the chain kernel fetches them without the table
  t.bias_stride = p->N > 1 ? tab[1].bias_r_off - tab[0].bias_r_off : 1;
  for (int b = 1; b < p->N; ++b)
    if (tab[b].bias_r_off != tab[0].bias_r_off + (int64_t)b * t.bias_stride) t.bias_stride = 0;
  t.B = B; t.chain128 = chain128;
  t.valid = true;
  return WN_OK;
}

// ---- frame schedules ----
// the frame table of `rows` condition rows as offsets into the caller's buffer: the bias rows first (what the records point
// into), the conditioning phase's scratch at that row count behind them
WsLayout frame_table_layout(const wn_plan* p, int64_t rows) {
  WsLayout L{};
  Carver cv;
  L.frames = 1;
  L.cb = cv.take((int64_t)p->N * rows * 2 * p->D);
  for (const ConvInfo& c : p->mapping) L.M.push_back(cv.take(rows * c.cout));
  L.cbt = cv.take(rows * p->N * 2 * p->D);
  L.total = cv.pos;
  return L;
}

// the armed schedules against a call of B rows over the steps [first, first + length): WN_E_INVALID with the numbers
int frames_call_check(const GenFrames& fr, int B, int64_t first, int length, bool queued) {
  if (!queued) {
    wn_set_error("generate: frame schedules are armed (wn_plan_arm_gen_frames); the sliding window takes none (queued = 0)");
    return WN_E_INVALID;
  }
  if ((int64_t)fr.host.size() != B) {
    wn_set_error("generate: frame schedules are armed for B = %d rows, the call has B = %d", (int)fr.host.size(), B);
    return WN_E_INVALID;
  }
  if (length < 1) return WN_OK;
  const int64_t last = first + length - 1;
  for (int b = 0; b < B; ++b) {
    const wn_frame_row& r = fr.host[b];
    if (!r.rows || last < r.origin) continue;
    const int64_t f = (last - r.origin) / r.hop;
    if (f >= r.frames) {
      wn_set_error("generate: row %d runs past its condition frames: sample %lld is in frame %lld, the row has frames = %d of hop = %d "
                   "from origin %lld (its last sample is %lld)", b, (long long)last, (long long)f, (int)r.frames, (int)r.hop,
                   (long long)r.origin, (long long)(r.origin + (int64_t)r.frames * r.hop - 1));
      return WN_E_INVALID;
    }
  }
  return WN_OK;
}

// the device copy of the armed records: uploaded when it holds other records than the armed ones.  A blocking copy, behind
// everything the stream still has queued (an earlier call's copy kernels read the table)
int ensure_frame_table(GenFrames& fr, hipStream_t s) {
  const size_t n = fr.host.size();
  if (fr.dev.d && fr.on_dev.size() == n && memcmp(fr.on_dev.data(), fr.host.data(), n * sizeof(wn_frame_row)) == 0) return WN_OK;
  WN_HIP_CHECK(hipStreamSynchronize(s));
  if (fr.dev.d && fr.on_dev.size() == n) {
    fr.on_dev.clear();
    WN_HIP_CHECK(hipMemcpy(fr.dev.d, fr.host.data(), n * sizeof(wn_frame_row), hipMemcpyHostToDevice));
  } else {
    fr.on_dev.clear();
    const int rc = fr.dev.upload(fr.host);
    if (rc) return rc;
  }
  fr.on_dev = fr.host;
  return WN_OK;
}

// marks[t - first] != 0: the copy kernel runs for step t -- the call's first queued step step0, and every later step at
// which some scheduled row begins a frame
std::vector<uint8_t> frame_marks(const GenFrames& fr, int first, int step0, int end) {
  std::vector<uint8_t> m((size_t)(end - first), 0);
  m[(size_t)(step0 - first)] = 1;
  for (const wn_frame_row& r : fr.host) {
    if (!r.rows) continue;
    int64_t t = (int64_t)step0 + 1;
    if (t <= r.origin) t = r.origin;
    else t += (r.hop - (t - r.origin) % r.hop) % r.hop;
    for (; t < end; t += r.hop) m[(size_t)(t - first)] = 1;
  }
  return m;
}

// ------------------------------------------------------------------------------------------
// One call of wn_generate_chunk: the caller's buffers, the generation layout of B, the priming layout, the rings and
// the kernel paths of the call; its phases are the member functions, in launch order.  A call makes the samples
// first .. first + length - 1 of a sequence; every `step` below is the index in the sequence, and everything between two
// steps lives in the workspace (xin, the rings, the relay's granule area; the weight images and cb of the priming pass),
// so a call with first > 0 goes on where the call before it stopped.  A call that `primes` begins a sequence from a
// window: its first step is the priming pass.  That is the call with first == 0 of every entry point, and the call of
// wn_generate_rows_begin at any first: the window's index t then stands at time t + first, and the counter, the output
// column, the window parity and tau of the first sample are those of step `first`.
// ------------------------------------------------------------------------------------------
struct GenCall {
  wn_exec& e;                        // the calling thread's execution state for p
  wn_plan* p; const float* params; const float* cond; int B, length; bool deterministic;
  int first, end, step0;             // the call's steps are [first, end); step0: the first one that is not the priming pass
  bool primes;                       // step `first` is the priming pass over the caller's window
  uint64_t seed; WnSampleCtl ctl;    // the sampling controls
  // per-row controls (wn_generate_rows_chunk): the caller's device table, one record per utterance, or null.  With a
  // table every stochastic draw of the call -- sliding window, priming step, sampler launch, head tail -- reads its row's
  // record; ctl is the union of the rows (what gen_paths and the launchers' checks look at) and seed is unused.
  const WnSampleRow* rows = nullptr;
  // the rows' clocks (the *_origin entry points): the caller's device array, one origin per utterance,
  // or null.  Travels with the table to every draw that reads it: row b draws sample t from counter (stream, t - origin[b]).
  const uint64_t* origin = nullptr;
  float* out; float* ws; hipStream_t s;
  int RF;
  GenLayout G;
  WsLayout L;                        // of the priming forward over the window
  GenRings R;
  GenPaths gp;                       // queued: the kernel paths of this call
  float* pws; const float* fragbase;
  float* win[2]; float* last; float* lastp; float* samp; float* Zrow;
  // Range guard (wn_generate_guard_slot): the split-precision kernels cast activations to fp16 hi | lo unscaled, so every
  // kernel that produces one -- priming pass, per-step blocks, the fused chain kernel -- publishes its running max-abs
  // here; the caller reads the float after the call and repeats it with the exact-fp32 kernels when it reached
  // wn_range_limit().  One slot per call: cleared by begin(), only ever raised afterwards.
  float* gguard;
  const float* hin = nullptr;        // the head's input rows of the step (skip() -> head())
  // arguments that do not change from step to step (build_*)
  WnGenStepArgs ga; WnGen128Args ca; WnGenHeadArgs ha;

  void bind(wn_plan* p_, const float* params_, const float* cond_, int B_, int first_, int length_, bool primes_, bool det,
            uint64_t seed_, const WnSampleCtl& ctl_, float* out_, float* workspace, hipStream_t s_, GenLayout&& G_) {
    p = p_; params = params_; cond = cond_; B = B_; length = length_; deterministic = det; seed = seed_; ctl = ctl_;
    first = first_; end = first_ + length_; primes = primes_; step0 = primes_ ? first_ + 1 : first_;
    out = out_; ws = workspace; s = s_;
    RF = wn_plan_receptive_field(p);
    G = std::move(G_);
    L = make_layout(p, B, RF, false);
    pws = ws + G.prime; fragbase = pws + L.frag;
    win[0] = ws + G.win0; win[1] = ws + G.win1;
    last = ws + G.last; lastp = ws + G.lastp; samp = ws + G.samp; Zrow = ws + G.Zrow;
    gguard = ws + G.guard;
    R.xin = ws + G.xin;
    R.t0 = primes ? first : 0;         // the window's index t is the sample at time t + first
    for (size_t b = 0; b < G.ring.size(); ++b) {
      R.h.push_back(ws + G.ring[b]);
      R.nslots.push_back(G.nslots[b]);
      R.hp.emplace_back();
      for (int64_t off : G.ringp[b]) R.hp.back().push_back(ws + off);
      R.nslots_p.push_back(G.nslots_p[b]);
    }
  }

  int64_t tau(int step) const { return (int64_t)RF + step - 1; }   // time of the newest known sample at `step`
  // where sample `step` goes: output column `step - first`, and the slot of the raw sample ring it enters the network
  // from (it is x[RF + step], the input at time tau(step) + 1)
  WnEmit emit(int step) const { return WnEmit{out, length, step - first, R.xin + (int64_t)((tau(step) + 1) % p->KS) * B}; }

  // the window into the workspace (a continuation has none), the guard (and the relay's give-up word behind it) cleared
  int begin(const float* window) {
    // (the window buffers alternate with the step's parity: the sequence's first step reads win[first & 1])
    if (window) WN_HIP_CHECK(hipMemcpyAsync(win[first & 1], window, (int64_t)B * RF * sizeof(float), hipMemcpyDeviceToDevice, s));
    WN_HIP_CHECK(hipMemsetAsync(gguard, 0, 2 * sizeof(float), s));
    return WN_OK;
  }

  // forward over the window `w` (rings captured when given), guard, the logits of its last time step -> `last`
  int window_forward(const float* w, bool prep, const GenRings* rings) {
    int rc = forward_core(p, params, w, prep, cond, B, RF, false, pws, L, s, rings);
    if (rc) return rc;
    rc = wn_launch_guard_accumulate(pws + L.fwd_absmax, gguard, s);
    if (rc) return rc;
    hipLaunchKernelGGL(wn_gather_last_kernel, dim3((B * p->Cout + 255) / 256), dim3(256), 0, s, pws + L.logits, B, RF, p->Cout, last);
    return WN_OK;
  }

  // ---- naive sliding window: one full forward over the window per sample (src/model.py:296-305) ----
  int sliding_window() {
    for (int step = first; step < end; ++step) {
      int rc = window_forward(win[step & 1], primes && step == first, nullptr);
      if (rc) return rc;
      rc = sample_rows(p, last, B, deterministic, seed, (uint64_t)step, lastp, samp, s, ctl, rows, origin);
      if (rc) return rc;
      hipLaunchKernelGGL(wn_gen_shift_kernel, dim3((B * RF + 255) / 256), dim3(256), 0, s, win[step & 1], samp, B, RF,
                         win[(step + 1) & 1], out, length, step - first);
      WN_HIP_CHECK(hipGetLastError());
    }
    return WN_OK;
  }

  // ---- queued: prime the per-block rings with one forward over the window, then one time step per
  //      sample with rows = utterances; every kernel and every per-row operation order is the one
  //      the sliding window uses, so the results are identical ----
  int prime() {
    int rc = window_forward(win[first & 1], true, &R);
    if (rc) return rc;
    rc = sample_rows(p, last, B, deterministic, seed, (uint64_t)first, lastp, samp, s, ctl, rows, origin);
    if (rc) return rc;
    // sample `first` is x[RF + first]; it becomes the network input at time tau = RF + first (output column 0)
    hipLaunchKernelGGL(wn_gen_emit_kernel, dim3((B + 255) / 256), dim3(256), 0, s, samp, B, out, length, 0, emit(first).xin_slot);
    if (gp.chain == GEN_RELAY128)   // every granule tag starts below the first epoch
      WN_HIP_CHECK(hipMemsetAsync(ws + G.relay, 0, (size_t)wn_gen_relay128_floats(B, p->N) * sizeof(float), s));
    return WN_OK;
  }

  // the launch arguments of the steps, everything but tau / epoch / the tail's counter and emit target
  void build_args() {
    if (gp.chain == GEN_CHAIN64) build_chain64();
    if (gp.chain128()) build_chain128();
    if (gp.head != GEN_HEAD_LAYERS) build_head();
  }

  void build_chain64() {
    memset(&ga, 0, sizeof(ga));
    ga.params = params; ga.ws = ws; ga.blocks = e.gen.blocks.d; ga.xin = R.xin;
    ga.causal_w = params + p->tensors[p->causal.kernel_t].off;
    ga.causal_b = params + p->tensors[p->causal.bias_t].off;
    ga.u0_off = G.u0;
    for (int b = 0; b < 3; ++b) ga.blk0[b] = e.gen.blk0[b];
    ga.bias_r_off0 = e.gen.blk0[0].bias_r_off; ga.bias_r_stride = e.gen.bias_stride;
    if (gp.skip == GEN_SKIP_IN_CHAIN) {
      ga.skip_w16_off = G.prime + L.frag + gp.skip_img;
      ga.skip_bias_off = G.prime + (gp.fold ? L.bfold : L.bias_sum);
      ga.skiprow_off = G.skiprow; ga.skip_ld = gp.skipw; ga.skip_tiles = gp.skipw / 32;
      ga.skip_act = gp.fold ? p->c.activation : WN_ACT_LINEAR;
    }
    // the chain kernel raises the guard slot in EVERY step, but only from lanes whose own running max-abs reached the
    // limit (wn_guard_publish_over: no wave reduction, no read of the slot)
    ga.guard = gguard;
    ga.zrow_off = G.Zrow; ga.hrow_off = p->c.use_skip ? -1 : G.hrow0;
    ga.B = B; ga.nblocks = p->N; ga.residual = p->c.use_residual;
  }

  void build_chain128() {
    memset(&ca, 0, sizeof(ca));
    ca.params = params; ca.ws = ws; ca.blocks = e.gen.blocks.d; ca.zrow_off = G.Zrow;
    ca.hrow_off = p->c.use_skip ? -1 : G.hrow0; ca.B = B; ca.nblocks = p->N; ca.residual = p->c.use_residual;
    ca.guard = gguard;
    if (gp.inconv_in_chain) {
      ca.xin = R.xin; ca.causal_w = params + p->tensors[p->causal.kernel_t].off; ca.causal_b = params + p->tensors[p->causal.bias_t].off;
    }
    ca.skip_w16_off = -1;
    if (gp.skip == GEN_SKIP_IN_CHAIN) {
      ca.skip_w16_off = G.prime + L.frag + gp.skip_img; ca.skip_bias_off = G.prime + L.bfold; ca.skiprow_off = G.skiprow;
      ca.skip_act = p->c.activation;
    }
    if (gp.chain == GEN_RELAY128) {
      ca.ntiles = (B + 31) / 32; ca.relay_off = G.relay;
      ca.tmo = reinterpret_cast<unsigned*>(gguard + 1);
    }
  }

  // both one-launch heads: the split-precision layers from first_final on; GEN_HEAD_MIX keeps the last layer for the
  // exact-fp32 rows behind them and always samples, GEN_HEAD_FUSED samples where the call has head_tail
  void build_head() {
    const bool mix = gp.head == GEN_HEAD_MIX;
    const size_t nf = p->finals.size(), first = (size_t)gp.first_final, end = mix ? nf - 1 : nf;
    memset(&ha, 0, sizeof(ha));
    ha.params = params; ha.ws = ws; ha.in_off = gp.skip == GEN_SKIP_NONE ? G.hrow0 : G.skiprow; ha.in_ld = gp.hc0; ha.out_off = G.last;
    ha.nlayers = (int)(end - first); ha.B = B;
    ha.guard = gguard;
    for (size_t i = first; i < end; ++i) {
      const ConvInfo& c = p->finals[i];
      const size_t l = i - first;
      ha.w16_off[l] = G.prime + L.frag + c.frag16; ha.bias_off[l] = p->tensors[c.bias_t].off;
      ha.K[l] = c.cin; ha.N[l] = c.cout;
      ha.act[l] = (i + 1 == nf) ? WN_ACT_LINEAR : p->c.activation;
    }
    if (mix) {
      const ConvInfo& cl = p->finals.back();
      ha.f32_w_off = G.prime + L.frag + cl.fragF; ha.f32_bias_off = p->tensors[cl.bias_t].off;
      ha.f32_K = cl.cin; ha.f32_N = cl.cout;
      ha.tail = deterministic ? 3 : 4; ha.mix_M = p->c.num_mixtures; ha.mix_kind = p->c.head;
    } else if (gp.head_tail) {
      ha.tail = deterministic ? 1 : 2;
      ha.inv_lv = 1.0f / (float)(1 << (p->c.bits - 1));
    }
    if (ha.tail) { ha.seed = seed; ha.ctl = ctl; ha.samp = samp; }
  }

  // frame schedules: the scheduled rows' frames of step `step` into cb, in front of the launch that reads cb for that step
  int frame_copy(int step) {
    return wn_launch_gen_frame_copy(e.frames.dev.d, e.frames.vec, B, p->N, 2 * p->D, (int64_t)step, pws + L.cb, s);
  }

  // the input conv and every block of the step: x[tau] -> the rings' slots tau, the gated activations Zrow
  int blocks(int step) {
    const int64_t tau = this->tau(step);
    if (gp.chain == GEN_CHAIN64) {
      ga.tau = tau;
      // (the pre work of the call's first step rode in no head launch: that step does its own)
      return wn_launch_gen_blocks(ga, p->R, p->KS, (gp.pre_in_head && step > step0) ? 2 : 3, s);
    }
    int rc;
    // input causal conv on [x[tau-(KS-1)], ..., x[tau]]  ->  block 0's ring slot tau  (128-channel chain: inside its launch)
    if (!gp.inconv_in_chain) {
      Gemm g(B, 1, p->R, ceil32(p->R));
      for (int t = 0; t < p->KS; ++t)
        g.seg(R.xin + (int64_t)((tau - (p->KS - 1 - t)) % p->KS) * B, 1, 1, 0,
              fragbase + p->causal.fragF + t * p->causal.fragF_stride);
      rc = g.bias(params + p->tensors[p->causal.bias_t].off).run(R.h[0] + (int64_t)(tau % R.nslots[0]) * B * p->R, p->R, s);
      if (rc) return rc;
    }
    if (gp.chain128()) {
      ca.tau = tau;
      if (gp.chain == GEN_CHAIN128) return wn_launch_gen_chain128(ca, s);
      ca.epoch = (uint32_t)step;
      return wn_launch_gen_relay128(ca, s);
    }
    for (int b = 0; b < p->N; ++b) {
      BlockPtrs k = block_ptrs(p, b, params, fragbase, B, 1);
      if (p->c.cond_inputs > 0) k.cb = pws + L.cb + (int64_t)b * B * 2 * p->D;
      const int d = p->blocks[b].dil.back().dil;
      BlockBufs f;
      memset(&f, 0, sizeof(f));
      // layers_per_block > 1 (the reference's stated blocker, README.md:16): every dilated conv of the
      // stack has a ring of ITS inputs; the non-gated convs run here, one output row each, and feed the
      // next ring's slot tau
      const float* in_ring = R.h[b];
      int in_ns = R.nslots[b], in_c = p->R;
      for (int i = 0; i + 1 < p->LPB; ++i) {
        const int di = p->blocks[b].dil[i].dil;
        Gemm g(B, 1, p->D, ceil32(p->D));
        for (int t = 0; t < p->KS; ++t)
          g.seg(in_ring + (int64_t)((tau - (int64_t)(p->KS - 1 - t) * di) % in_ns) * B * in_c, in_c, in_c, 0,
                k.Fd[i] + t * k.Fd_stride[i]);
        float* dst = R.hp[b][i] + (int64_t)(tau % R.nslots_p[b][i]) * B * p->D;
        rc = g.bias(k.bd[i]).act(k.act).run(dst, p->D, s);
        if (rc) return rc;
        in_ring = R.hp[b][i]; in_ns = R.nslots_p[b][i]; in_c = p->D;
      }
      for (int t = 0; t < p->KS; ++t)
        f.xt[t] = in_ring + (int64_t)((tau - (int64_t)(p->KS - 1 - t) * d) % in_ns) * B * in_c;
      f.x = f.xt[p->KS - 1];
      if (p->LPB > 1) {
        f.pre_done = true;
        f.res = R.h[b] + (int64_t)(tau % R.nslots[b]) * B * p->R;     // the block input at time tau
      }
      f.U = ws + G.hrow1;
      f.AG = nullptr;
      f.Z = Zrow + (int64_t)b * B * p->Dp; f.ldz = p->Dp;
      f.O = nullptr;
      f.x_out = (b + 1 < p->N) ? R.h[b + 1] + (int64_t)(tau % R.nslots[b + 1]) * B * p->R
                               : (p->c.use_skip ? ws + G.dummy : ws + G.hrow0);
      f.fwd_absmax = gguard;
      rc = block_forward(k, f, s);
      if (rc) return rc;
    }
    return WN_OK;
  }

  // the skip contraction over Zrow (unless the chain launch carried it): the head's input rows
  int skip(int) {
    hin = ws + (gp.skip == GEN_SKIP_NONE ? G.hrow0 : G.skiprow);
    if (gp.skip != GEN_SKIP_LAUNCH) return WN_OK;
    // utterances are the ROWS of these contractions (no time shift, no per-utterance bias here)
    return Gemm(1, B, gp.skipw, ceil32(gp.skipw)).seg_planes(Zrow, p->Dp, (int64_t)B * p->Dp, p->N * p->Dp, gp.fold ? nullptr : fragbase + p->frag_skipF)
        .w16(gp.skip_img >= 0 ? fragbase + gp.skip_img : nullptr)
        .bias(pws + (gp.fold ? L.bfold : L.bias_sum)).act(gp.fold ? p->c.activation : WN_ACT_LINEAR)
        .absmax_fwd(gguard).run(ws + G.skiprow, gp.skipw, s);
  }

  // the head layers -> the logits rows `last` (one-launch heads: with their sampling tail, and GEN_HEAD_FUSED with the pre
  // work of the next step)
  int head(int step) {
    if (gp.head != GEN_HEAD_LAYERS) {
      if (ha.tail) { ha.offset = (uint64_t)step; ha.em = emit(step); }
      if (gp.pre_in_head && step + 1 < end) {
        ga.tau = tau(step) + 1;
        return wn_launch_gen_head_pre(ha, ga, p->R, p->KS, s, rows, origin);
      }
      return wn_launch_gen_head(ha, s, rows, origin);
    }
    const float* in = hin;
    int hc = gp.hc0;
    for (size_t i = (size_t)gp.first_final; i < p->finals.size(); ++i) {
      const ConvInfo& c = p->finals[i];
      const bool lastl = (i + 1 == p->finals.size());
      float* dst = lastl ? last : ws + G.HArow[i];
      const int rc = Gemm(1, B, c.cout, ceil32(c.cout)).seg(in, hc, hc, 0, fragbase + c.fragF)
                         .w16(c.frag16 >= 0 ? fragbase + c.frag16 : nullptr)
                         .bias(params + p->tensors[c.bias_t].off).act(lastl ? WN_ACT_LINEAR : p->c.activation)
                         .absmax_fwd(lastl ? nullptr : gguard).run(dst, c.cout, s);
      if (rc) return rc;
      in = dst; hc = c.cout;
    }
    return WN_OK;
  }

  // sampler and emit in one launch (categorical: straight from the logits -- softmax + arg max, or the softmax of
  // wn_softmax_kernel in LDS and the class sample_waveform(softmax(logits)) draws), unless the head launch did both
  int sample(int step) {
    const bool cat = p->c.head == WN_HEAD_CATEGORICAL;
    switch (gp.sampler) {
      case GEN_SAMPLE_IN_HEAD: return WN_OK;
      case GEN_SAMPLE_DET:
        return wn_launch_sample_det(last, B, p->Cout, p->c.num_mixtures, p->c.bits, cat ? nullptr : samp, s, emit(step));
      case GEN_SAMPLE_RAND:
        return wn_launch_sample_rand(last, B, p->Cout, p->c.num_mixtures, p->c.bits, p->c.head, seed, (uint64_t)step, samp, s, ctl, emit(step), rows, origin);
      case GEN_SAMPLE_ROWS: break;
    }
    const int rc = sample_rows(p, last, B, false, seed, (uint64_t)step, lastp, samp, s, ctl, rows, origin);
    if (rc) return rc;
    hipLaunchKernelGGL(wn_gen_emit_kernel, dim3((B + 255) / 256), dim3(256), 0, s, samp, B, out, length, step - first, emit(step).xin_slot);
    WN_HIP_CHECK(hipGetLastError());
    return WN_OK;
  }
};

}  // namespace

// The sampling arguments of the *_sampled entry points, checked before anything touches the device or any other argument
// is looked at (head: WN_HEAD_*, classes: the categorical row length).  On success *ctl holds the controls the kernels
// take: top_k >= classes is off, top_p = 1 is off.
int wn_sampling_check(const char* who, const wn_sampling* sp, int head, int classes, WnSampleCtl* ctl) {
  if (!sp) { wn_set_error("%s: sampling is null", who); return WN_E_INVALID; }
  const float T = sp->temperature;
  if (!(T > 0.f) || !std::isfinite(T) || !std::isfinite(1.0f / T)) {
    wn_set_error("%s: temperature must be finite and > 0 with a finite reciprocal (got %g)", who, (double)T);
    return WN_E_INVALID;
  }
  if (sp->top_k < 0) { wn_set_error("%s: top_k must be >= 0 (got %d)", who, (int)sp->top_k); return WN_E_INVALID; }
  if (sp->top_k > 0 && head != WN_HEAD_CATEGORICAL) {
    wn_set_error("%s: top_k applies to the categorical head only (got top_k = %d with a mixture head)", who, (int)sp->top_k);
    return WN_E_INVALID;
  }
  const float tp = sp->top_p;
  if (!(tp >= 0.f && tp <= 1.0f)) {                       // NaN fails both comparisons
    wn_set_error("%s: top_p must lie in (0, 1], or be 0 for off (got %g)", who, (double)tp);
    return WN_E_INVALID;
  }
  const bool topp = tp > 0.f && tp < 1.0f;
  if (topp && head != WN_HEAD_CATEGORICAL) {
    wn_set_error("%s: top_p applies to the categorical head only (got top_p = %g with a mixture head)", who, (double)tp);
    return WN_E_INVALID;
  }
  ctl->T = T; ctl->inv_T = 1.0f / T;
  ctl->top_k = (sp->top_k >= classes) ? 0 : sp->top_k;
  ctl->top_p = topp ? tp : 0.f;
  if (ctl->top_k > 0 && classes > wn_sample_top_k_max_classes()) {
    wn_set_error("%s: top_k is offered for up to %d classes (got %d)", who, wn_sample_top_k_max_classes(), classes);
    return WN_E_UNSUPPORTED;
  }
  if (topp && classes > wn_sample_top_k_max_classes()) {
    wn_set_error("%s: top_p is offered for up to %d classes (got %d)", who, wn_sample_top_k_max_classes(), classes);
    return WN_E_UNSUPPORTED;
  }
  return WN_OK;
}

extern "C" int64_t wn_generate_guard_slot(const wn_plan* p, int32_t B, int32_t queued) {
  if (!p || B < 1) return -1;
  return gen_layout(p, B, queued != 0).guard;
}
extern "C" int64_t wn_generate_workspace_floats(const wn_plan* p, int32_t B, int32_t queued) {
  if (!p || B < 1) return 0;
  return gen_layout(p, B, queued != 0).total;
}

extern "C" int wn_generate(wn_plan* p, const float* params, const float* window, const float* cond, int32_t B,
                           int32_t length, int32_t deterministic, int32_t queued, uint64_t seed, float* out,
                           float* workspace, int64_t ws_floats, void* stream) {
  const wn_sampling sp = {1.0f, 0, seed};
  return wn_generate_sampled(p, params, window, cond, B, length, deterministic, queued, &sp, out, workspace, ws_floats, stream);
}

// wn_generate_sampled (window given, first = 0) and wn_generate_chunk
// ... and wn_generate_rows_chunk: rows (device) in place of sampling, with the union of its rows from rows_flags
// ... and wn_generate_rows_begin (GEN_ENTRY_BEGIN): a window at any first >= 0
// ... and their *_origin forms: origin (device, with rows only), the clock origin of every utterance, or null
enum GenEntry { GEN_ENTRY_ONE, GEN_ENTRY_CHUNK, GEN_ENTRY_BEGIN };
static int generate_call(GenEntry entry, wn_plan* p, const float* params, const float* window, const float* cond, int32_t B,
                         int64_t first, int32_t length, int32_t deterministic, int32_t queued, const wn_sampling* sampling,
                         float* out, float* workspace, int64_t ws_floats, void* stream,
                         const WnSampleRow* rows = nullptr, int32_t rows_flags = 0, const uint64_t* origin = nullptr,
                         bool scheduled = true) {
  const bool chunk = entry != GEN_ENTRY_ONE, begins = entry == GEN_ENTRY_BEGIN;
  WnSampleCtl ctl = WN_SAMPLE_CTL_OFF;
  if (rows) {
    // the union of the rows as a WnSampleCtl: on() when some row is on, top_p > 0 when some row has top_p on (the values
    // stand for "on" only: the kernels read the rows)
    if (rows_flags & WN_SAMPLING_ROWS_ON) { ctl.T = 2.0f; ctl.inv_T = 0.5f; }
    if (rows_flags & WN_SAMPLING_ROWS_TOP_P) ctl.top_p = 0.5f;
  } else {
    const int rc = wn_sampling_check("generate", sampling, p ? p->c.head : WN_HEAD_CATEGORICAL, p ? p->Cout : 0x7fffffff, &ctl);
    if (rc) return rc;
  }
  if (chunk) {
    if (first < 0) { wn_set_error("generate: first must be >= 0 (got %lld)", (long long)first); return WN_E_INVALID; }
    if (begins && !window) { wn_set_error("generate: window is null (wn_generate_rows_begin begins a sequence from a window)"); return WN_E_INVALID; }
    if (!begins && window && first != 0) {
      wn_set_error("generate: window begins a sequence and requires first == 0 (got first = %lld)", (long long)first);
      return WN_E_INVALID;
    }
    if (!window && first == 0) { wn_set_error("generate: window is null with first == 0 (a sequence begins from a window)"); return WN_E_INVALID; }
    // (steps are 32-bit in the launch arguments: the output column, the time tau = RF + step - 1 of the chains)
    if (length > 0 && first + length > 0x7fffffffLL) {
      wn_set_error("generate: first + length must not exceed 2147483647 (got first = %lld, length = %d)", (long long)first, (int)length);
      return WN_E_INVALID;
    }
  }
  if (!p || !params || (!window && first == 0) || !out || !workspace || B < 1 || length < 0) { wn_set_error("generate: bad arguments"); return WN_E_INVALID; }
  // (a step is one time row and takes one condition row per utterance: frames belong to the training-form calls)
  if (wnp::ex(p).cond_frames > 1) {
    wn_set_error("generate: %d condition frames are armed (wn_plan_set_cond_frames); generation takes one condition row per utterance", wnp::ex(p).cond_frames);
    return WN_E_INVALID;
  }
  // the armed frame schedules (wn_plan_arm_gen_frames; scheduled = false: an admission's scratch pass takes cond)
  GenFrames* fr = (scheduled && wnp::ex(p).frames.armed) ? &wnp::ex(p).frames : nullptr;
  if (fr) {
    const int rc = frames_call_check(*fr, B, first, length, queued != 0);
    if (rc) return rc;
  }
  GenLayout G = gen_layout(p, B, queued != 0);
  if (ws_floats < G.total) { wn_set_error("generate: workspace too small"); return WN_E_INVALID; }
  if (length == 0) return WN_OK;
  if (fr) {                                  // (a blocking copy when the records changed: nothing of this call is queued yet)
    const int rc = ensure_frame_table(*fr, (hipStream_t)stream);
    if (rc) return rc;
  }
  GenCall c{wnp::ex(p)};
  c.bind(p, params, cond, B, (int)first, length, window != nullptr, deterministic != 0, rows ? 0 : sampling->seed, ctl, out, workspace,
         (hipStream_t)stream, std::move(G));
  c.rows = rows;
  c.origin = c.deterministic ? nullptr : origin;
  int rc = c.begin(window);
  if (rc) return rc;
  if (!queued) return c.sliding_window();
  c.gp = gen_paths(p, B, c.end, device_cu_count(), c.G.relay >= 0, c.deterministic, ctl);
  if (c.primes) {
    rc = c.prime();
    if (rc) return rc;
    c.e.primed_ws = workspace; c.e.primed_B = B;       // (what wn_generate_set_condition may write into)
  }
  // (a call that is its priming pass alone launches no step: the admission's scratch call at B' = k leaves the session's
  // table, cached by B, where it is)
  if (c.step0 >= c.end) return WN_OK;
  // (in every call that reads it: a call at another B may have rebuilt the table in between)
  if (c.gp.table()) {
    rc = ensure_gen_table(p, c.e, c.G, c.L, B, c.gp.chain128());
    if (rc) return rc;
  }
  c.build_args();
  // frame schedules: the copy kernel in front of the launch that reads cb for a marked step -- the head launch of the step
  // before where it carries the pre work (never for step0, which does its own), the chain / relay / block launch otherwise
  const std::vector<uint8_t> marks = fr ? frame_marks(*fr, c.first, c.step0, c.end) : std::vector<uint8_t>();
  const bool in_head = fr && c.gp.pre_in_head;
  for (int step = c.step0; step < c.end; ++step) {
    if (fr && marks[step - c.first] && (!in_head || step == c.step0) && (rc = c.frame_copy(step)) != WN_OK) return rc;
    if ((rc = c.blocks(step)) != WN_OK) return rc;
    if ((rc = c.skip(step)) != WN_OK) return rc;
    if (in_head && step + 1 < c.end && marks[step + 1 - c.first] && (rc = c.frame_copy(step + 1)) != WN_OK) return rc;
    if ((rc = c.head(step)) != WN_OK) return rc;
    if ((rc = c.sample(step)) != WN_OK) return rc;
  }
  return WN_OK;
}

// A new condition for a running queued sequence: the conditioning phase again, into the bias table of the primed workspace.
// The steps read cb from there (it is state, not a per-step input), so the next step of the next chunk uses it; a chunk's
// first step does its own pre work (wn_generate_chunk), which is where the 64-channel chain adds cb.
extern "C" int wn_generate_set_condition(wn_plan* p, const float* params, const float* cond, int32_t B, int32_t queued,
                                         float* workspace, int64_t ws_floats, void* stream) {
  if (!p || !params || !cond || !workspace) {
    wn_set_error("generate_set_condition: null %s", !p ? "plan" : !params ? "params" : !cond ? "cond" : "workspace");
    return WN_E_INVALID;
  }
  if (B < 1) { wn_set_error("generate_set_condition: B must be >= 1 (got %d)", (int)B); return WN_E_INVALID; }
  if (!queued) { wn_set_error("generate_set_condition: queued sequences only (the sliding window maps the condition in every step)"); return WN_E_INVALID; }
  if (p->c.cond_inputs <= 0) { wn_set_error("generate_set_condition: the plan has no conditioning"); return WN_E_INVALID; }
  if (wnp::ex(p).cond_frames > 1) { wn_set_error("generate_set_condition: %d condition frames are armed; a step takes one row per utterance", wnp::ex(p).cond_frames); return WN_E_INVALID; }
  const GenLayout G = gen_layout(p, B, true);
  if (ws_floats < G.total) { wn_set_error("generate_set_condition: workspace too small (%lld < %lld floats)", (long long)ws_floats, (long long)G.total); return WN_E_INVALID; }
  const wn_exec& e = wnp::ex(p);
  if (e.primed_ws != workspace || e.primed_B != B) {
    wn_set_error("generate_set_condition: the workspace has not been primed at B = %d by this state (begin the sequence first)", (int)B);
    return WN_E_INVALID;
  }
  const int RF = wn_plan_receptive_field(p);
  const WsLayout L = make_layout(p, B, RF, false);
  return condition_only(p, params, cond, B, RF, workspace + G.prime, L, (hipStream_t)stream);
}

// ---- frame schedules: a request's table, and the records of the batch (include/wn_hip.h) ----
extern "C" int64_t wn_generate_frames_floats(const wn_plan* p, int64_t rows) {
  if (!p || p->c.cond_inputs <= 0 || rows < 1) return 0;
  return frame_table_layout(p, rows).total;
}

// The conditioning phase of wn_generate_set_condition over k * F rows, into the caller's table.  The weight images are the
// ones the priming pass left in the primed workspace (FwdCall::condition reads them and nothing else of it).
extern "C" int wn_generate_frames_build(wn_plan* p, const float* params, const float* cond, int32_t k, int32_t F, float* table,
                                        int64_t table_floats, const float* workspace, int64_t ws_floats, int32_t B, void* stream) {
  if (!p || !params || !cond || !table || !workspace) {
    wn_set_error("generate_frames_build: null %s", !p ? "plan" : !params ? "params" : !cond ? "cond" : !table ? "table" : "workspace");
    return WN_E_INVALID;
  }
  if (k < 1 || F < 1) { wn_set_error("generate_frames_build: k and F must be >= 1 (got k = %d, F = %d)", (int)k, (int)F); return WN_E_INVALID; }
  if (p->c.cond_inputs <= 0) { wn_set_error("generate_frames_build: the plan has no conditioning"); return WN_E_INVALID; }
  const int64_t rows = (int64_t)k * F;
  // (the products and the scatter index their rows with 32-bit arithmetic)
  if (rows * p->N * 2 * p->D > 0x7fffffffLL) {
    wn_set_error("generate_frames_build: k * F * blocks * 2D must not exceed 2147483647 (got k = %d, F = %d: %lld rows of %d blocks, 2D = %d)",
                 (int)k, (int)F, (long long)rows, p->N, 2 * p->D);
    return WN_E_INVALID;
  }
  if (wnp::ex(p).cond_frames > 1) {
    wn_set_error("generate_frames_build: %d condition frames are armed (wn_plan_set_cond_frames); disarm them first", wnp::ex(p).cond_frames);
    return WN_E_INVALID;
  }
  if ((uintptr_t)table % 16 != 0) { wn_set_error("generate_frames_build: table must be aligned to 16 bytes"); return WN_E_INVALID; }
  const WsLayout T = frame_table_layout(p, rows);
  if (table_floats < T.total) {
    wn_set_error("generate_frames_build: table too small (%lld floats, wn_generate_frames_floats(p, %lld) is %lld)", (long long)table_floats,
                 (long long)rows, (long long)T.total);
    return WN_E_INVALID;
  }
  if (B < 1) { wn_set_error("generate_frames_build: B must be >= 1 (got %d)", (int)B); return WN_E_INVALID; }
  const GenLayout G = gen_layout(p, B, true);
  if (ws_floats < G.total) {
    wn_set_error("generate_frames_build: workspace too small (%lld < %lld floats)", (long long)ws_floats, (long long)G.total);
    return WN_E_INVALID;
  }
  // (no look at the primed mark of the calling state: other sequences of the same state may have begun since, and the images
  // of this workspace are as good as they were -- that it has been primed is the caller's word)
  const WsLayout L = make_layout(p, B, wn_plan_receptive_field(p), false);
  return condition_rows(p, params, cond, (int)rows, workspace + G.prime + L.frag, table, T, (hipStream_t)stream);
}

extern "C" int wn_plan_arm_gen_frames(wn_plan* p, const wn_frame_row* records, int32_t B) {
  if (!p) { wn_set_error("arm_gen_frames: null plan"); return WN_E_INVALID; }
  if (B < 0) { wn_set_error("arm_gen_frames: B must be >= 0 (got %d)", (int)B); return WN_E_INVALID; }
  GenFrames& fr = wnp::ex(p).frames;
  if (!records || B == 0) {            // disarm (the device copy stays: the next arming of the same records uploads nothing)
    fr.armed = false; fr.host.clear();
    return WN_OK;
  }
  if (p->c.cond_inputs <= 0) { wn_set_error("arm_gen_frames: %d frame schedules on a plan without conditioning", (int)B); return WN_E_INVALID; }
  if (wnp::ex(p).cond_frames > 1) {
    wn_set_error("arm_gen_frames: %d condition frames are armed (wn_plan_set_cond_frames); a generation step takes one row per utterance",
                 wnp::ex(p).cond_frames);
    return WN_E_INVALID;
  }
  const int64_t D2 = 2 * p->D;
  bool vec = true;
  for (int32_t b = 0; b < B; ++b) {
    const wn_frame_row& r = records[b];
    if (!r.rows) continue;
    if (r.frames < 1 || r.hop < 1) {
      wn_set_error("arm_gen_frames: row %d: frames and hop must be >= 1 (got frames = %d, hop = %d)", (int)b, (int)r.frames, (int)r.hop);
      return WN_E_INVALID;
    }
    if (r.block_stride < (int64_t)r.frames * D2) {
      wn_set_error("arm_gen_frames: row %d: block_stride = %lld is below frames * 2D = %d * %d", (int)b, (long long)r.block_stride, (int)r.frames, (int)D2);
      return WN_E_INVALID;
    }
    if ((uintptr_t)r.rows % 4 != 0) { wn_set_error("arm_gen_frames: row %d: rows must be aligned to 4 bytes", (int)b); return WN_E_INVALID; }
    vec = vec && (uintptr_t)r.rows % 16 == 0 && r.block_stride % 4 == 0;
  }
  fr.host.assign(records, records + B);
  fr.vec = vec;
  fr.armed = true;
  return WN_OK;
}

extern "C" int wn_generate_sampled(wn_plan* p, const float* params, const float* window, const float* cond, int32_t B,
                                   int32_t length, int32_t deterministic, int32_t queued, const wn_sampling* sampling,
                                   float* out, float* workspace, int64_t ws_floats, void* stream) {
  return generate_call(GEN_ENTRY_ONE, p, params, window, cond, B, 0, length, deterministic, queued, sampling, out, workspace, ws_floats, stream);
}

extern "C" int wn_generate_chunk(wn_plan* p, const float* params, const float* window, const float* cond, int32_t B,
                                 int64_t first, int32_t length, int32_t deterministic, int32_t queued,
                                 const wn_sampling* sampling, float* out, float* workspace, int64_t ws_floats, void* stream) {
  return generate_call(GEN_ENTRY_CHUNK, p, params, window, cond, B, first, length, deterministic, queued, sampling, out, workspace, ws_floats, stream);
}

extern "C" int wn_generate_state_range(const wn_plan* p, int32_t B, int32_t queued, int64_t* offset, int64_t* floats) {
  if (!p || B < 1 || !offset || !floats) { wn_set_error("generate_state_range: bad arguments"); return WN_E_INVALID; }
  const GenLayout G = gen_layout(p, B, queued != 0);
  // queued: xin, the rings, the inner rings, the per-step rows, u0, the relay's granule area and the head rows -- everything
  // behind the guard; sliding window: the two window buffers
  *offset = queued ? G.xin : G.win0;
  *floats = queued ? G.total - G.xin : G.win1 + (int64_t)B * wn_plan_receptive_field(p) - G.win0;
  return WN_OK;
}

// ---- per-row sampling controls (include/wn_hip.h, struct wn_sampling_row) ----
static_assert(sizeof(wn_sampling_row) == sizeof(WnSampleRow) && offsetof(wn_sampling_row, seed) == offsetof(WnSampleRow, seed) &&
              offsetof(wn_sampling_row, stream) == offsetof(WnSampleRow, stream) && offsetof(wn_sampling_row, top_p) == offsetof(WnSampleRow, top_p),
              "wn_sampling_row is WnSampleRow");

extern "C" int64_t wn_sampling_rows_floats(int32_t B) {
  return B < 1 ? 0 : (int64_t)B * (int64_t)(sizeof(wn_sampling_row) / sizeof(float));
}

extern "C" int wn_sampling_rows_pack(const wn_sampling* sampling, const uint64_t* stream, int32_t B, int32_t head, int32_t classes,
                                     wn_sampling_row* rows, int32_t* flags) {
  if (!sampling || !rows || !flags || B < 1) {
    wn_set_error("sampling_rows_pack: bad arguments (sampling, rows and flags must not be null, B >= 1; got B = %d)", (int)B);
    return WN_E_INVALID;
  }
  int32_t f = 0;
  for (int32_t b = 0; b < B; ++b) {
    char who[48];
    snprintf(who, sizeof(who), "sampling_rows_pack: row %d", (int)b);
    WnSampleCtl ctl = WN_SAMPLE_CTL_OFF;
    const int rc = wn_sampling_check(who, sampling + b, head, classes, &ctl);
    if (rc) return rc;
    const uint64_t st = stream ? stream[b] : (uint64_t)b;
    if (st >> 63) {
      wn_set_error("sampling_rows_pack: row %d: stream must be below 2^63 (got %llu)", (int)b, (unsigned long long)st);
      return WN_E_INVALID;
    }
    rows[b] = wn_sampling_row{ctl.T, ctl.inv_T, ctl.top_k, ctl.top_p, sampling[b].seed, st};
    if (ctl.on()) f |= WN_SAMPLING_ROWS_ON;
    if (ctl.top_p > 0.f) f |= WN_SAMPLING_ROWS_TOP_P;
  }
  *flags = f;
  return WN_OK;
}

// a caller's device table and its flags, before anything else is looked at (rows_name / flags_name: the argument names in the text)
static int rows_table_check(const char* who, const char* rows_name, const char* flags_name, const wn_sampling_row* rows, int32_t rows_flags) {
  if (!rows) { wn_set_error("%s: %s is null (the device table of wn_sampling_rows_pack)", who, rows_name); return WN_E_INVALID; }
  if ((uintptr_t)rows % 16 != 0) { wn_set_error("%s: %s must be aligned to 16 bytes", who, rows_name); return WN_E_INVALID; }
  if (rows_flags & ~(WN_SAMPLING_ROWS_ON | WN_SAMPLING_ROWS_TOP_P) || ((rows_flags & WN_SAMPLING_ROWS_TOP_P) && !(rows_flags & WN_SAMPLING_ROWS_ON))) {
    wn_set_error("%s: %s must be the flags wn_sampling_rows_pack returned (got %d)", who, flags_name, (int)rows_flags);
    return WN_E_INVALID;
  }
  return WN_OK;
}

// the clock origins of a *_origin entry point, before anything else is looked at: null is "none"
static int origin_check(const char* who, const char* name, const uint64_t* origin) {
  if ((uintptr_t)origin % 8 != 0) { wn_set_error("%s: %s must be aligned to 8 bytes", who, name); return WN_E_INVALID; }
  return WN_OK;
}

extern "C" int wn_generate_rows_chunk_origin(wn_plan* p, const float* params, const float* window, const float* cond, int32_t B,
                                             int64_t first, int32_t length, int32_t deterministic, int32_t queued,
                                             const wn_sampling_row* rows, int32_t rows_flags, const uint64_t* origin, float* out,
                                             float* workspace, int64_t ws_floats, void* stream) {
  int rc = origin_check("generate", "origin", origin);
  if (rc) return rc;
  rc = rows_table_check("generate", "rows", "rows_flags", rows, rows_flags);
  if (rc) return rc;
  return generate_call(GEN_ENTRY_CHUNK, p, params, window, cond, B, first, length, deterministic, queued, nullptr, out, workspace, ws_floats,
                       stream, reinterpret_cast<const WnSampleRow*>(rows), rows_flags, origin);
}
extern "C" int wn_generate_rows_chunk(wn_plan* p, const float* params, const float* window, const float* cond, int32_t B,
                                      int64_t first, int32_t length, int32_t deterministic, int32_t queued,
                                      const wn_sampling_row* rows, int32_t rows_flags, float* out, float* workspace,
                                      int64_t ws_floats, void* stream) {
  return wn_generate_rows_chunk_origin(p, params, window, cond, B, first, length, deterministic, queued, rows, rows_flags, nullptr, out,
                                       workspace, ws_floats, stream);
}

// ---- a sequence that begins at a position other than 0, and admission into a running batch ----
extern "C" int wn_generate_rows_begin_origin(wn_plan* p, const float* params, const float* window, const float* cond, int32_t B,
                                             int64_t first, int32_t length, int32_t deterministic, int32_t queued,
                                             const wn_sampling_row* rows, int32_t rows_flags, const uint64_t* origin, float* out,
                                             float* workspace, int64_t ws_floats, void* stream) {
  int rc = origin_check("generate", "origin", origin);
  if (rc) return rc;
  rc = rows_table_check("generate", "rows", "rows_flags", rows, rows_flags);
  if (rc) return rc;
  return generate_call(GEN_ENTRY_BEGIN, p, params, window, cond, B, first, length, deterministic, queued, nullptr, out, workspace, ws_floats,
                       stream, reinterpret_cast<const WnSampleRow*>(rows), rows_flags, origin);
}
extern "C" int wn_generate_rows_begin(wn_plan* p, const float* params, const float* window, const float* cond, int32_t B,
                                      int64_t first, int32_t length, int32_t deterministic, int32_t queued,
                                      const wn_sampling_row* rows, int32_t rows_flags, float* out, float* workspace,
                                      int64_t ws_floats, void* stream) {
  return wn_generate_rows_begin_origin(p, params, window, cond, B, first, length, deterministic, queued, rows, rows_flags, nullptr, out,
                                       workspace, ws_floats, stream);
}

namespace {

// One run of consecutive ring slots that the admission moves, as wn_gen_admit_rows_kernel reads it: slot s of utterance j
// is `width` floats at src + (s * k + j) * width in the scratch workspace and goes to dst + (s * B + slots[j]) * width in the
// session's.  Both sequences share the time axis, so slot s goes to slot s.
struct AdmitSeg {
  char name[24];
  int block;                         // the block it belongs to, or -1 (xin)
  WnAdmitSeg d;
};

// everything the steps read per utterance (GenLayout, the step kernels; DESIGN.md section 32 says why this is all of it):
// Gk / Lk: the scratch's layouts (k rows), G / L: the session's (B rows)
std::vector<AdmitSeg> admit_segments(const wn_plan* p, const GenLayout& Gk, const WsLayout& Lk, int k, const GenLayout& G,
                                     const WsLayout& L, int B) {
  std::vector<AdmitSeg> v;
  auto add = [&](const char* fmt, int block, int i, int64_t src, int64_t dst, int nslots, int width) {
    AdmitSeg a;
    snprintf(a.name, sizeof(a.name), fmt, block, i);
    a.block = block;
    a.d = WnAdmitSeg{src, dst, nslots, width};
    v.push_back(a);
  };
  add("xin", -1, 0, Gk.xin, G.xin, p->KS, 1);
  for (int b = 0; b < p->N; ++b) {
    add("ring[%d]", b, 0, Gk.ring[b], G.ring[b], G.nslots[b], p->R);
    for (size_t i = 0; i < G.ringp[b].size(); ++i) add("ringp[%d][%d]", b, (int)i, Gk.ringp[b][i], G.ringp[b][i], G.nslots_p[b][i], p->D);
  }
  if (p->c.cond_inputs > 0)          // [block][rows][2D] of the priming layout: one "slot" per block
    for (int b = 0; b < p->N; ++b)
      add("cb[%d]", b, 0, Gk.prime + Lk.cb + (int64_t)b * k * 2 * p->D, G.prime + L.cb + (int64_t)b * B * 2 * p->D, 1, 2 * p->D);
  return v;
}

// One launch per admission: blockIdx.y = segment, blockIdx.z strides over the admitted utterances, the threads of the x
// dimension stride over the segment's nslots * width floats of one utterance (consecutive threads, consecutive floats of a row).
__global__ void wn_gen_admit_rows_kernel(const WnAdmitSeg* __restrict__ segs, const int32_t* __restrict__ slots, int k, int B,
                                         const float* __restrict__ scratch, float* __restrict__ ws) {
  const WnAdmitSeg sg = segs[blockIdx.y];
  const int64_t n = (int64_t)sg.nslots * sg.width;
  for (int j = blockIdx.z; j < k; j += gridDim.z) {
    const int row = slots[j];
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
      const int64_t s = i / sg.width, c = i % sg.width;
      ws[sg.dst + (s * B + row) * sg.width + c] = scratch[sg.src + (s * k + j) * sg.width + c];
    }
  }
}

// the cached device copies of e: rebuilt when (k, B, slots) is not the key they were built for
int ensure_admit_table(wn_exec& e, const std::vector<AdmitSeg>& segs, int k, int B, const int32_t* slots) {
  AdmitTable& t = e.admit;
  if (t.valid && t.k == k && t.B == B && std::equal(t.slots.begin(), t.slots.end(), slots)) return WN_OK;
  t.valid = false;
  if (t.k != k || t.B != B || !t.segs.d) {
    std::vector<WnAdmitSeg> d;
    for (const AdmitSeg& a : segs) d.push_back(a.d);
    const int rc = t.segs.upload(d);
    if (rc) return rc;
  }
  t.slots.assign(slots, slots + k);
  const int rc = t.slots_d.upload(t.slots);
  if (rc) return rc;
  t.k = k; t.B = B;
  t.valid = true;
  return WN_OK;
}

// the arguments of wn_generate_admit that speak of k, B and the slots: WN_E_INVALID with the argument named
int admit_slots_check(const char* who, int32_t k, const int32_t* slots, int32_t B) {
  if (B < 1) { wn_set_error("%s: B must be >= 1 (got %d)", who, (int)B); return WN_E_INVALID; }
  if (k < 1 || k > B) { wn_set_error("%s: k must lie in [1, B] (got k = %d, B = %d)", who, (int)k, (int)B); return WN_E_INVALID; }
  if (!slots) return WN_OK;
  std::vector<char> seen((size_t)B, 0);
  for (int32_t j = 0; j < k; ++j) {
    if (slots[j] < 0 || slots[j] >= B) {
      wn_set_error("%s: slots[%d] = %d lies outside [0, B = %d)", who, (int)j, (int)slots[j], (int)B);
      return WN_E_INVALID;
    }
    if (seen[slots[j]]) { wn_set_error("%s: slots[%d] = %d is a duplicate (the slots must be distinct)", who, (int)j, (int)slots[j]); return WN_E_INVALID; }
    seen[slots[j]] = 1;
  }
  return WN_OK;
}

}  // namespace

extern "C" int64_t wn_generate_admit_scratch_floats(const wn_plan* p, int32_t k) {
  return wn_generate_workspace_floats(p, k, 1);
}

extern "C" int wn_generate_admit_describe(const wn_plan* p, int32_t k, int32_t B, char* buf, int32_t len) {
  if (!buf || len < 1) { wn_set_error("generate_admit_describe: no buffer"); return WN_E_INVALID; }
  buf[0] = 0;
  if (!p) { wn_set_error("generate_admit_describe: p is null"); return WN_E_INVALID; }
  int rc = admit_slots_check("generate_admit_describe", k, nullptr, B);
  if (rc) return rc;
  const int RF = wn_plan_receptive_field(p);
  const std::vector<AdmitSeg> segs = admit_segments(p, gen_layout(p, k, true), make_layout(p, k, RF, false), k, gen_layout(p, B, true),
                                                    make_layout(p, B, RF, false), B);
  int64_t per = 0;
  std::string out;
  for (const AdmitSeg& a : segs) {
    char item[200];
    snprintf(item, sizeof(item), "%s%s block=%d slots=%d width=%d src=%lld dst=%lld", out.empty() ? "" : " | ", a.name, a.block, a.d.nslots,
             a.d.width, (long long)a.d.src, (long long)a.d.dst);
    out += item;
    per += (int64_t)a.d.nslots * a.d.width;
  }
  out += " | floats_per_utterance=" + std::to_string(per);
  snprintf(buf, (size_t)len, "%s", out.c_str());
  if ((int64_t)out.size() + 1 > (int64_t)len) {
    wn_set_error("generate_admit_describe: the line needs %d bytes, the buffer has %d", (int)out.size() + 1, (int)len);
    return WN_E_INVALID;
  }
  return WN_OK;
}

extern "C" int wn_generate_admit(wn_plan* p, const float* params, const float* windows, const float* cond, int32_t k,
                                 const int32_t* slots, int32_t B, int64_t position, int32_t deterministic,
                                 const wn_sampling_row* rows_k, int32_t rows_flags_k, float* first_out, float* workspace,
                                 int64_t ws_floats, float* scratch, int64_t scratch_floats, void* stream) {
  return wn_generate_admit_origin(p, params, windows, cond, k, slots, B, position, deterministic, rows_k, rows_flags_k, nullptr, first_out,
                                  workspace, ws_floats, scratch, scratch_floats, stream);
}

// origin_k: the clocks of the k requests in the scratch priming pass (their priming draw is sample position - 1), or null
extern "C" int wn_generate_admit_origin(wn_plan* p, const float* params, const float* windows, const float* cond, int32_t k,
                                        const int32_t* slots, int32_t B, int64_t position, int32_t deterministic,
                                        const wn_sampling_row* rows_k, int32_t rows_flags_k, const uint64_t* origin_k,
                                        float* first_out, float* workspace, int64_t ws_floats, float* scratch,
                                        int64_t scratch_floats, void* stream) {
  int rc = origin_check("generate_admit", "origin_k", origin_k);
  if (rc) return rc;
  const struct { const void* ptr; const char* name; } ptrs[] = {{p, "p"}, {params, "params"}, {windows, "windows"}, {slots, "slots"},
                                                                {rows_k, "rows_k"}, {first_out, "first_out"}, {workspace, "workspace"},
                                                                {scratch, "scratch"}};
  for (const auto& a : ptrs)
    if (!a.ptr) { wn_set_error("generate_admit: %s is null", a.name); return WN_E_INVALID; }
  rc = admit_slots_check("generate_admit", k, slots, B);
  if (rc) return rc;
  if (wnp::ex(p).cond_frames > 1) {
    wn_set_error("generate_admit: %d condition frames are armed (wn_plan_set_cond_frames); generation takes one condition row per utterance", wnp::ex(p).cond_frames);
    return WN_E_INVALID;
  }
  // (the admission's priming draw is sample position - 1, and the session goes on at `position`: both are 32-bit steps)
  if (position < 1 || position > 0x7fffffffLL - 1) {
    wn_set_error("generate_admit: position must lie in [1, 2147483646] (got %lld)", (long long)position);
    return WN_E_INVALID;
  }
  rc = rows_table_check("generate_admit", "rows_k", "rows_flags_k", rows_k, rows_flags_k);
  if (rc) return rc;
  const int RF = wn_plan_receptive_field(p);
  const GenLayout Gk = gen_layout(p, k, true), G = gen_layout(p, B, true);
  if (ws_floats < G.total) {
    wn_set_error("generate_admit: workspace too small (%lld floats, the queued session of B = %d needs %lld)", (long long)ws_floats, (int)B, (long long)G.total);
    return WN_E_INVALID;
  }
  if (scratch_floats < Gk.total) {
    wn_set_error("generate_admit: scratch too small (%lld floats, wn_generate_admit_scratch_floats(p, %d) is %lld)", (long long)scratch_floats, (int)k, (long long)Gk.total);
    return WN_E_INVALID;
  }
  if (p->c.cond_inputs > 0 && !cond) { wn_set_error("generate_admit: cond is null on a conditioned net"); return WN_E_INVALID; }
  // the tables first (a rebuild is a blocking copy: nothing of this call is queued yet), then the requests primed alone
  // in the scratch at the session's time, then their state rows into the session's rows
  const std::vector<AdmitSeg> segs = admit_segments(p, Gk, make_layout(p, k, RF, false), k, G, make_layout(p, B, RF, false), B);
  if (segs.size() > 65535) { wn_set_error("generate_admit: %d state segments (the launch takes up to 65535)", (int)segs.size()); return WN_E_UNSUPPORTED; }
  wn_exec& e = wnp::ex(p);
  rc = ensure_admit_table(e, segs, k, B, slots);
  if (rc) return rc;
  rc = generate_call(GEN_ENTRY_BEGIN, p, params, windows, cond, k, position - 1, 1, deterministic, 1, nullptr, first_out, scratch,
                     scratch_floats, stream, reinterpret_cast<const WnSampleRow*>(rows_k), rows_flags_k, origin_k, false);
  if (rc) return rc;
  e.primed_ws = workspace; e.primed_B = B;             // (the scratch's priming pass moved the mark: back to the session)
  int64_t widest = 1;
  for (const AdmitSeg& a : segs) widest = std::max(widest, (int64_t)a.d.nslots * a.d.width);
  const dim3 grid((unsigned)std::min<int64_t>((widest + 255) / 256, 256), (unsigned)segs.size(), (unsigned)std::min(k, 65535));
  hipLaunchKernelGGL(wn_gen_admit_rows_kernel, grid, dim3(256), 0, (hipStream_t)stream, e.admit.segs.d, e.admit.slots_d.d, k, B, scratch, workspace);
  WN_HIP_CHECK(hipGetLastError());
  return WN_OK;
}
