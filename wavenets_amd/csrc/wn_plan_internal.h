// Internal interface of the plan / orchestration translation units behind the C-ABI of include/wn_hip.h
// (wn_plan.hip: plan + workspace layout; wn_block.hip: one residual block; wn_forward.hip: the model's forward pass and
// loss; wn_train.hip: backward pass, weight gradients; wn_optim.hip: optimizer; wn_generate.hip: generation;
// wn_cabi_ops.hip: the elementwise entry points).  Host-side only.
#pragma once
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <mutex>
#include <vector>

#include "../../include/wn_hip.h"
#include "wn_kernels.h"

namespace wnp {

inline int64_t align64(int64_t v) { return (v + 63) & ~(int64_t)63; }
inline int ceil32(int v) { return (v + 31) / 32; }
inline int ceil8(int v) { return (v + 7) / 8 * 8; }

struct TensorInfo {
  int64_t off, len;
  int ndim;
  int64_t shape[3];
  int is_kernel;
};

// one convolution / dense: raw parameter offsets plus its two weight images
struct ConvInfo {
  int kernel_t = -1, bias_t = -1;   // tensor indices
  int taps = 1, cin = 0, cout = 0, dil = 1;
  int64_t fragF = -1;   // taps images of A[cout][cin]  (forward:  A[n][k] = W[tap][k][n])
  int64_t fragB = -1;   // taps images of A[cin][cout]  (backward: A[k][n] = W[tap][k][n])
  int64_t fragF_stride = 0, fragB_stride = 0;
  int64_t frag16 = -1;  // fp16 hi/lo split forward image (all taps concatenated along k), or -1
  int64_t frag16B = -1; // fp16 split backward-data image A[cin][taps*cout], or -1
};

struct BlockInfo {
  std::vector<ConvInfo> dil;
  ConvInfo conv1, conv_skip, conv_cond;
  bool has_skip = false, has_cond = false;
  int64_t g16u = -1;    // fp16 split image [W_r | W_s] (backward: d z) or -1
  int64_t f16gate = -1; // fp16 split image of the gated conv with row tiles ordered [f f g g] per 64 channels, or -1
  int64_t f16nat = -1;  // fp16 split image of the gated conv in natural row-tile order for the streamed one-kernel forward (R = D = 128), or -1
  int64_t g16uf = -1;   // fp16 split image [W_r | V(b)], V(b) = W_s(b) W_f0 (skip path folded into the first head conv), or -1
  // stacks deeper than 1 (training passes): forward images of the non-gated convs, backward-data images of every conv of
  // the stack; 32-channel outputs are padded to two row tiles (see wn_gemm_rows16_ok)
  int64_t d16F[16], d16B[16];
  BlockInfo() { for (int i = 0; i < 16; ++i) d16F[i] = d16B[i] = -1; }
};

// The running max-abs scalars of the gradient tensors (operand scaling of the split-precision products), as indices from
// WsLayout::absmax: GF[i] | g_skipsum | GU[b] | GH[b] (N + 1 of them) | GP[b][i] (inner convs of deeper stacks)
struct AbsmaxSlots {
  int nf, N, LPB;
  int gf(int i) const { return i; }
  int gskip() const { return nf; }
  int gu(int b) const { return nf + 1 + b; }
  int gh(int b) const { return nf + 1 + N + b; }
  int gp(int b, int i) const { return nf + 1 + N + (N + 1) + b * (LPB - 1) + i; }
  int count() const { return gp(N, 0); }
};

// Which kernel family each part of the gradient half of a training step takes: decided once (train_paths, wn_plan.hip),
// read by the schedule builder, the launch phases and wn_plan_describe.
// block weight gradients: wn_wgrad_layer_kernel | ... with its INNER form for the inner convs of deeper stacks | two
// wn_wgrad_tr_kernel jobs per block | generic job table | ... forced to exact fp32 (deeper stacks without split images)
enum WgFamily { WG_LAYER, WG_LAYER_INNER, WG_TR_PAIRS, WG_GENERIC, WG_GENERIC_FP32 };
enum BwdFamily { BWD_BLOCKS, BWD_PAIR, BWD_S128 };   // per-block backward | wn_bwd_pair_kernel | wn_bwd_s128_kernel
struct TrainPaths {
  // from the plan and knob 1
  WgFamily wg = WG_GENERIC;
  BwdFamily bwd = BWD_BLOCKS;
  int mtr = 0;             // M = Z^T dL/da of the folded skip path as wn_wgrad_tr jobs over several blocks' z (kind 7 / 8), or 0
                           // (kind 7: the jobs carry the blocks' dW_r, db_r too and the layer kernel runs without its 1x1 part)
  bool mfused = false;     // ... or riding in the dW_r jobs of WG_TR_PAIRS
  // the skip convs' own weight-gradient kernel | skip path folded into the head's first conv | deeper stacks train in split
  // precision (inner gradients carry max-abs slots) | some head layer has a staged pair kind
  bool skipk = false, fold = false, deep16 = false, head_pairs = false;
  // from the call: dropout on, the head / the input conv on a time split of their own, the pair chain's 32-bit row limit
  bool drop = false, head_split = false, in_split = false, rows32 = true;
  bool layerk() const { return wg == WG_LAYER || wg == WG_LAYER_INNER; }
  bool pairk() const { return wg == WG_TR_PAIRS; }
  bool headpairs() const { return head_pairs && head_split; }
  bool bwd_pairs() const { return bwd != BWD_BLOCKS && !drop && (bwd != BWD_S128 || rows32); }
  bool operator==(const TrainPaths& o) const {
    return wg == o.wg && bwd == o.bwd && mtr == o.mtr && mfused == o.mfused && skipk == o.skipk && fold == o.fold &&
           deep16 == o.deep16 && head_pairs == o.head_pairs && drop == o.drop && head_split == o.head_split &&
           in_split == o.in_split && rows32 == o.rows32;
  }
};

// Which kernels a queued generate call takes: decided once per call (gen_paths, wn_plan.hip), read by the phases of
// GenCall (wn_generate.hip).
// blocks of a step: one launch each | wn_gen_chain kernels (32 / 64 channels, input conv included) | 128 channels in one
// workgroup per utterance tile (wn_gen_chain128_kernel) | ... as a relay over one workgroup per block (wn_gen_relay128_kernel)
enum GenChain { GEN_BLOCKS, GEN_CHAIN64, GEN_CHAIN128, GEN_RELAY128 };
enum GenSkip { GEN_SKIP_NONE, GEN_SKIP_IN_CHAIN, GEN_SKIP_LAUNCH };   // no skip connections | in the chain launch | a contraction of its own
// one contraction per layer | every layer in one launch (wn_gen_head_kernel) | ... with the exact-fp32 last layer and the
// mixture sampler behind the split-precision layers
enum GenHead { GEN_HEAD_LAYERS, GEN_HEAD_FUSED, GEN_HEAD_MIX };
// the head launch samples and emits | arg max + emit | Philox draw + emit | softmax, sampler and emit as three launches
enum GenSampler { GEN_SAMPLE_IN_HEAD, GEN_SAMPLE_DET, GEN_SAMPLE_RAND, GEN_SAMPLE_ROWS };
struct GenPaths {
  GenChain chain = GEN_BLOCKS;
  bool inconv_in_chain = false;   // the input causal conv rides in the chain launch
  // the skip contraction: folded with the head's first conv (half the columns, as in forward_core) or the reference's skip
  // sum; its width, its split-precision image (or < 0), the first head layer behind it and that layer's input width
  GenSkip skip = GEN_SKIP_NONE;
  bool fold = false;
  int skipw = 0, first_final = 0, hc0 = 0;
  int64_t skip_img = -1;
  GenHead head = GEN_HEAD_LAYERS;
  bool pre_in_head = false;       // the pre kernel's work of step tau + 1 rides in the head launch of step tau
  bool head_tail = false;         // categorical heads: the sampling tail and the emit ride in the head launch too
  GenSampler sampler = GEN_SAMPLE_DET;
  bool chain128() const { return chain == GEN_CHAIN128 || chain == GEN_RELAY128; }
  bool table() const { return chain != GEN_BLOCKS; }   // the chain reads the device block table (GenTable)
  bool operator==(const GenPaths& o) const {
    return chain == o.chain && inconv_in_chain == o.inconv_in_chain && skip == o.skip && fold == o.fold && skipw == o.skipw &&
           first_final == o.first_final && hc0 == o.hc0 && skip_img == o.skip_img && head == o.head &&
           pre_in_head == o.pre_in_head && head_tail == o.head_tail && sampler == o.sampler;
  }
};

// Which kernels one forward pass takes: decided once per call (fwd_paths, wn_plan.hip), read by the phases of FwdCall
// (wn_forward.hip) and written out by wn_debug_fwd_paths.
enum FwdCond { FWD_COND_NONE, FWD_COND_SMALL, FWD_COND_ROWS };   // unconditioned | wn_sgemm_small32_kernel | rows GEMMs
enum FwdPrep { FWD_PREP_NONE, FWD_PREP_INLINE, FWD_PREP_SIDE };  // the skip path's weight-space preparation: none | caller's stream | side stream
// the skip stage: the last block output feeds the head | folded with the head's first conv on the planes kernel | ... on the
// rows GEMM | the reference's skip sum
enum FwdSkip { FWD_SKIP_NONE, FWD_SKIP_FOLD_PLANES, FWD_SKIP_FOLD_ROWS, FWD_SKIP_SUM };
enum FwdHead : uint8_t { FWD_HEAD_ROWS, FWD_HEAD_PLANES, FWD_HEAD_EPILOGUE };   // rows GEMM | planes kernel | ... with the loss as its epilogue
enum FwdLoss { FWD_LOSS_NONE, FWD_LOSS_TRAIN, FWD_LOSS_EVAL };   // what the caller wants of the loss epilogue (LossFuse)
struct FwdPaths {
  FwdCond cond = FWD_COND_NONE;
  bool cond_batched = false;      // all blocks' conv_cond as one contraction + scatter (else one rows GEMM per block)
  bool inconv_elem = false;       // the input conv on the elementwise kernel (else a rows GEMM over KS one-channel taps)
  bool zfill = false;             // Z has padding columns (Dp != D): zero-filled before the blocks
  bool fold = false;
  FwdPrep prep = FWD_PREP_NONE;
  bool drop = false;              // dropped copies of the block inputs
  bool deep16 = false;            // the deep-stack split-precision images are bound (training, no rings)
  FwdSkip skip = FWD_SKIP_NONE;
  int first_final = 0, hc0 = 0;   // the first head layer behind the skip stage and its input width
  int nhead = 0;                  // = finals.size(); head[i] for i >= first_final
  FwdHead head[WN_MAX_FINAL + 1] = {};
  bool operator==(const FwdPaths& o) const {
    return cond == o.cond && cond_batched == o.cond_batched && inconv_elem == o.inconv_elem && zfill == o.zfill && fold == o.fold &&
           prep == o.prep && drop == o.drop && deep16 == o.deep16 && skip == o.skip && first_final == o.first_final &&
           hc0 == o.hc0 && nhead == o.nhead && std::equal(head, head + WN_MAX_FINAL + 1, o.head);
  }
};

// Which kernels one residual block takes: decided once per call of block_forward / block_backward (block_fwd_path,
// block_bwd_path, wn_block.hip), read by their launch functions and written out by wn_debug_block_paths.
// a conv of the dilated stack, forward or backward data: the streamed kernel's second form with the taps as shifted planes |
// rows GEMM on a split-precision image | rows GEMM in exact fp32
enum BlkConv : uint8_t { BLK_CONV_PLANES, BLK_CONV_ROWS16, BLK_CONV_ROWS32 };
// the gated conv + 1x1: streamed one-kernel forward (wn_layer16s.hip) | two split-precision contractions | LDS-resident
// one-kernel forward on fp16 images | ... in exact fp32 | rows GEMM -> gate kernel -> rows GEMM
enum BlkGate : uint8_t { BLK_GATE_S128, BLK_GATE_TWO, BLK_GATE_FUSED16, BLK_GATE_FUSED32, BLK_GATE_COMPOSED };
struct BlockFwdPath {
  int ninner = 0;                 // non-gated convs this call runs (none when the queued generation step ran them: pre_done)
  BlkConv inner[16] = {};
  BlkGate gate = BLK_GATE_COMPOSED;
  bool operator==(const BlockFwdPath& o) const {
    return ninner == o.ninner && std::equal(inner, inner + 16, o.inner) && gate == o.gate;
  }
};
// g_o, the gradient at the 1x1 conv's output: g_xout | g_xout + g_skip into g_o_tmp (S == 0, both given) | g_skip (S == 0)
enum BlkGo : uint8_t { BLK_GO_XOUT, BLK_GO_SUM, BLK_GO_SKIP };
// the g_u product: [W_r | V(b)] image over (g_o, dL/da) | [W_r | W_s] image padded to two row tiles | [W_r | W_s] image |
// exact fp32 | no operand: zero fill
enum BlkGu : uint8_t { BLK_GU_FOLD, BLK_GU_PAD, BLK_GU_IMAGE, BLK_GU_FP32, BLK_GU_ZERO };
enum BlkAm : uint8_t { BLK_AM_NONE, BLK_AM_GXOUT, BLK_AM_GSKIP, BLK_AM_GFOLD };   // an input max-abs slot of BlockGrads
// the g_x product (conv 0's backward data): not formed | G16x | the deep stack's image | exact fp32 publishing g_x's max-abs | exact fp32
enum BlkGx : uint8_t { BLK_GX_NONE, BLK_GX_G16X, BLK_GX_DEEP, BLK_GX_FP32_ABSMAX, BLK_GX_FP32 };
struct BlockBwdPath {
  BlkGo go = BLK_GO_XOUT;
  BlkGu gu = BLK_GU_ZERO;
  bool gu_pad = false;            // the g_u contraction walks JTu row tiles of an image without fp32 fragments
  BlkAm gu_am[2] = {};            // the two input max-abs slots of an image form of the g_u product
  BlkConv data[16] = {};          // backward data of conv i, depth > i >= 1 (its result gets act' folded in)
  BlkGx gx = BLK_GX_NONE;
  bool drop = false;              // g_x's conv path into g_xd, then the keep-mask and the residual path (wn_launch_dropout)
  bool operator==(const BlockBwdPath& o) const {
    return go == o.go && gu == o.gu && gu_pad == o.gu_pad && gu_am[0] == o.gu_am[0] && gu_am[1] == o.gu_am[1] &&
           std::equal(data, data + 16, o.data) && gx == o.gx && drop == o.drop;
  }
};

// owning device copy of a host table
template <class T> struct DevTable {
  T* d = nullptr;
  void release() { if (d) (void)hipFree(d); d = nullptr; }
  int upload(const std::vector<T>& v, size_t min_count = 0) {
    release();
    const size_t n = std::max(v.size(), min_count);
    if (n == 0) return WN_OK;
    WN_HIP_CHECK(hipMalloc((void**)&d, n * sizeof(T)));
    if (!v.empty()) WN_HIP_CHECK(hipMemcpy(d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
    return WN_OK;
  }
};

// one launch of the weight-gradient phase, everything about it resolved when the schedule is built
struct WgSpan {
  enum Op : uint8_t { INCONV, JOBS, PAIRS, TR, LAYERS, SKIP } op;
  enum Slab : uint8_t { BATCH, HEAD, MFOLD } slab;   // batched slab | the head's compact slab and time split | the slab of M
  int kind;            // PAIRS / TR: the kernel's kind; JOBS: 1 = exact fp32; LAYERS: 1 = the inner table, INNER form; 2 = without the 1x1 part
  int first, count;    // entries of the op's table
};

// The weight-gradient schedule of one workspace layout: device tables and the launches over them.  Valid for its key
// (B, T, bsplits, paths) only; `valid` is false from before the first upload of a rebuild until the last one succeeds.
struct WgSchedule {
  bool valid = false;
  int B = 0, T = 0, bsplits = 0;
  int frames = 0;                    // condition frames the layout was carved for (the job tables hold workspace offsets)
  TrainPaths paths;
  DevTable<WnWgJob> jobs;
  DevTable<WnWgLayer> layers, inner;
  DevTable<WnWgPair> pairs;
  DevTable<WnTensorDesc> cov;
  std::vector<WnTensorDesc> h_cov;   // host copy of the coverage table (the flattened reduce sizes its grid from it)
  std::vector<WgSpan> spans;         // in issue order: the first n_side on the side stream when the step forks
  int n_side = 0;
  bool overlap = false;              // the side-stream spans may run beside the others
  int cov_head = 0;                  // coverage table: from here on the entries are reduced from the head's own slab
  void release() { valid = false; jobs.release(); layers.release(); inner.release(); pairs.release(); cov.release(); }
};

// The per-block offsets the generation chains read, for one batch size (ensure_gen_table, wn_generate.hip).  Valid for its
// key (B, chain128) only; `valid` is false from before the upload of a rebuild until it has succeeded.
struct GenTable {
  bool valid = false;
  int B = 0;
  bool chain128 = false;      // the table carries the 128-channel chain's images (BlockInfo::f16nat)
  DevTable<WnGenBlock> blocks;
  WnGenBlock blk0[3]{};       // entries 0..2 by value (the chain's first fetches do not wait for the table)
  int64_t bias_stride = 0;    // conv1 biases at a uniform stride (the chain fetches them without the table), or 0
  void release() { valid = false; blocks.release(); }
};

// one segment of an admission's move (wn_gen_admit_rows_kernel, wn_generate.hip): nslots x width floats per utterance,
// [slot][rows][width] at float offset src of the scratch workspace (k rows) and dst of the session's (B rows)
struct WnAdmitSeg { int64_t src, dst; int32_t nslots, width; };

// the device copies wn_generate_admit reads: the segment list of (k, B) and the slot list of the last admission
struct AdmitTable {
  bool valid = false;
  int k = 0, B = 0;
  std::vector<int32_t> slots;
  DevTable<WnAdmitSeg> segs;
  DevTable<int32_t> slots_d;
  void release() { valid = false; segs.release(); slots_d.release(); }
};

// The frame schedules armed by wn_plan_arm_gen_frames: the caller's records as armed (host), and the
// device copy the copy kernel reads.  Arming touches no device (a plan can be armed without one): the queued call that finds
// `dev` holding other records than `host` uploads them before it queues anything (ensure_frame_table, wn_generate.hip).
struct GenFrames {
  bool armed = false;
  bool vec = false;                    // every scheduled record: rows 16-byte aligned, block_stride % 4 == 0
  std::vector<wn_frame_row> host;      // B records
  std::vector<wn_frame_row> on_dev;    // what `dev` holds
  DevTable<wn_frame_row> dev;
  void release() { armed = false; host.clear(); on_dev.clear(); dev.release(); }
};

}  // namespace wnp

// The mutable side of a plan: per-caller state of the orchestration ("a wn_plan is immutable and shareable
// across streams").  One per stream of execution: dropout counter, the armed step sample, phase selection, the cached
// weight-gradient schedule of the last (B, T) it trained and the generation block table of the last batch size it
// generated (device memory they own, freed by exec_release), its side stream and events, its profiling events.  A
// caller that drives one plan from several host threads / streams creates
// one wn_exec per thread (wn_exec_create) and binds it there (wn_exec_bind: thread-local); unbound callers share the
// plan's own.
struct wn_exec {
  const struct wn_plan* plan = nullptr;
  float drop_rate = 0.f;        // Dropout rate applied to every block input in training (src/layers.py:108-111)
  uint64_t drop_seed = 0, drop_step = 0;
  // armed by wn_plan_arm_step_sample: the next training step also draws sample_waveform(pred)
  float* step_sample = nullptr; int step_sample_det = 0; uint64_t step_sample_seed = 0, step_sample_off = 0;
  // armed by wn_plan_arm_row_weights: sample_weight of the (B, T) target rows for wn_train_fwd_bwd / wn_eval_loss / wn_score; it stays
  // armed until the caller disarms it
  const float* row_weights = nullptr; int64_t row_weights_n = 0;
  // armed by wn_plan_set_cond_frames: the condition of the training-form entry points holds this many frames per utterance
  // (local conditioning); 0 / 1 = one row per utterance (global conditioning)
  int cond_frames = 0;
  // the queued generation workspace this state primed last and its batch size (wn_generate_set_condition writes into it)
  const float* primed_ws = nullptr; int primed_B = 0;
  wnp::WgSchedule wg;           // the cached weight-gradient schedule of the last (B, T) layout it trained
  wnp::GenTable gen;            // the cached block table of the generation chains, for the last batch size it generated
  wnp::AdmitTable admit;        // the cached segment and slot tables of the last admission (wn_generate_admit)
  wnp::GenFrames frames;        // the frame schedules armed by wn_plan_arm_gen_frames and their device copy
  // side stream: the side spans of the weight-gradient schedule run beside the per-block / skip kernels
  hipStream_t side = nullptr;
  hipEvent_t ev_fork = nullptr, ev_join = nullptr;
  hipEvent_t ev_ffork = nullptr, ev_fjoin = nullptr;   // forward pass: the fold's weight preparation beside the block chain
  int train_phases = 3;   // wn_plan_set_train_phases: bit 0 forward + loss (+ step sample), bit 1 backward + weight gradients
  // optional HIP-event timing of the fused block-forward launches (bench.py roofline leg)
  std::vector<hipEvent_t> prof_ev;   // pairs (start, stop)
  std::vector<int> prof_cnt;         // launches between the events of pair i
  hipEvent_t phase_ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};   // wn_phase_enable: train-step phase marks
  bool phase_on = false;
  int prof_used = 0;
  bool prof_on = false;
  // wn_stack_prof_enable: event pairs around the whole residual-block stack forward (first block launch -> end of
  // the folded skip contraction): SURVEY.md 8(d)'s t_stack_fwd
  std::vector<hipEvent_t> stack_ev;
  std::vector<hipEvent_t> foldprep_ev;   // pairs around the per-pass weight-space preparation of the folded skip path
  int foldprep_used = 0;
  int stack_used = 0;
};

struct wn_plan {
  wn_config c;
  int KS, R, D, S, N, LPB, Cout, Sh, Hin, Cc, Dp;
  std::vector<int> dilations;
  std::vector<wnp::TensorInfo> tensors;
  int64_t nparams = 0;
  wnp::ConvInfo causal;
  std::vector<wnp::BlockInfo> blocks;
  std::vector<wnp::ConvInfo> finals, mapping;
  int64_t frag_skipF = -1;     // A[Sh][N*Dp] image of the folded skip sum
  // all blocks' conv_cond as one layer (when every block has one and 2D % 32 == 0): forward image
  // A[N*2D][Cc], backward image A[Cc][N*2D]; -1 = per-block path
  int64_t frag_condF = -1, frag_condB = -1;
  int64_t frag16_skipF = -1;   // the same as an fp16 split image, or -1
  int64_t frag_floats = 0;
  // skip path folded into the head's first convolution (training passes; see wn_skip_fold_kernel): F0 = its width,
  // forward image A[F0][N*D] of V^T.  prep2 = pieces whose SOURCE is the workspace (the V matrix), not the parameters
  int fold_F0 = 0;
  int64_t frag16_foldF = -1;
  std::vector<WnPrepDesc> prep2;
  WnPrepDesc* d_prep2 = nullptr;
  WnTensorDesc* d_cov_fold = nullptr;
  WnTensorDesc h_cov_fold = {0, 0};     // host copies of the coverage tables (the flattened reduce sizes its grid from them)
  std::vector<WnPrepDesc> prep;
  std::vector<WnTensorDesc> tdesc, kdesc;
  // device copies (lazy)
  WnPrepDesc* d_prep = nullptr;
  WnTensorDesc* d_tdesc = nullptr;
  WnTensorDesc* d_kdesc = nullptr;
  bool fused_ok = false, fused16_ok = false;
  bool deep16_ok = false;      // layers_per_block > 1: split-precision images of the whole stack exist
  // device copies of the immutable tables above are made on first use (a plan can be created without a GPU): guarded
  // by tables_once, never changed afterwards
  std::mutex tables_mu;
  bool tables_ready = false;
  // Everything that CHANGES while a plan is used lives in a wn_exec (below).  `own` is the execution state of callers that
  // never bind one of their own (wn_exec_bind): created with the plan, destroyed with it.
  struct wn_exec* own = nullptr;
};

namespace wnp {
// the execution state of the calling thread for this plan: the bound one if it belongs to the plan, else the plan's own
wn_exec& ex(const wn_plan* p);
void exec_release(wn_exec* e);


struct Carver {
  int64_t pos = 0;
  int64_t take(int64_t n) { int64_t o = pos; pos = align64(pos + (n > 0 ? n : 0)); return o; }
};

struct WsLayout {
  int64_t frag, bias_sum;
  std::vector<int64_t> H;               // N+1 block inputs/outputs (training) or 2 (inference)
  std::vector<std::vector<int64_t>> P;  // per block: outputs of the non-gated convs (depth > 1)
  int64_t Z;                            // [rows][N*Dp]
  std::vector<int64_t> AG;              // per block [rows][D] saved sigmoid (training)
  std::vector<std::vector<int64_t>> GP; // per block, per non-gated conv: [rows][D] gradient of its pre-activation output
  int64_t U;                            // [rows][2D] scratch of the composed path / g_u
  int64_t O;                            // [rows][R] pre-residual output scratch
  int64_t skipsum;                      // [rows][Hin]
  std::vector<int64_t> HA;              // head activations
  int64_t logits, probs;
  int64_t target, loss_rows, yt;
  int64_t g_skipsum;                    // [rows][Hin]
  int64_t slab, slab_floats;
  std::vector<int64_t> GU, GH, GO, GF;  // deferred-wgrad mode: per-block g_u, g_h (N+1), g_o; per-final g
  int64_t bslab; int bsplits;           // batched slab [B*bsplits][nparams]
  // the head's weight gradients get their own, finer time split: a compact slab [B*hsplits][head_span] over the
  // contiguous parameter range of the final layers (head_base = its first float); 0 splits = share bslab
  int64_t hslab; int hsplits; int64_t head_base, head_span;
  // the input conv's (KS + 1) * R sums have a compact slab of their own too: [B * isplits][(KS + 1) * R] (its kernel
  // and bias are the first two tensors of the flat buffer), so that the 33 MB stream is spread over ~512 workgroups
  int64_t islab; int isplits;
  // folded skip path: V [N*D][F0], b' [F0] (fixed offsets right behind the images), [W_s(all blocks); sum b_s]
  // ([N*D + 1][S]), the slab [B*bsplits][N*D*F0 + F0] of M = Z^T dL/da with the column sums behind it, its reduced
  // form [M; colsum] and Y = [M; colsum] W_f0^T ([N*D + 1][S])
  int64_t vfold, bfold, wsall, mslab, mtot, ytmp;
  std::vector<int64_t> XD;              // dropout: dropped copy of every block input (training)
  int64_t gxd;                          // dropout: scratch for d loss / d (dropped input)
  int64_t absmax; int n_absmax;         // running max-abs scalars of the gradient tensors (AbsmaxSlots)
  int64_t fwd_absmax;                   // forward range guard: running max-abs of H[b], skip sum, head activations
  int64_t sum_scratch;
  // conditioning.  Bc = B * frames condition rows: one per utterance (global), one per (utterance, frame) when frames are
  // armed (local, wn_plan_set_cond_frames)
  int frames;                           // >= 1
  std::vector<int64_t> M;               // mapping activations [Bc][w]
  int64_t cb;                           // [N][Bc][2D]
  int64_t dcb, g_m0, g_m1;
  int64_t cbt;                          // [Bc][N*2D]: all blocks' conditioning biases / their gradients
  int64_t total;
};

inline bool al16(const void* p) { return (((uintptr_t)p) & 15) == 0; }

struct Gemm {
  WnGemmArgs a;
  const float* w16_ = nullptr;
  const float* am0_ = nullptr;
  const float* am1_ = nullptr;
  float* amo_ = nullptr;
  // split-precision image of ALL segments (concatenated along k); optional max-abs scalars
  Gemm& w16(const float* img) { w16_ = img; return *this; }
  Gemm& absmax(const float* in0, const float* in1, float* out) { am0_ = in0; am1_ = in1; amo_ = out; return *this; }
  // forward range-guard slot: unlike a gradient's scale slot it must also record inf / NaN
  Gemm& absmax_fwd(float* out) { amo_ = out; a.absmax_any = out ? 1 : 0; return *this; }
  Gemm(int B, int T, int N, int JTtot) {
    memset(&a, 0, sizeof(a));
    a.B = B; a.T = T; a.N = N; a.JTtot = JTtot; a.act = WN_ACT_LINEAR; a.epi = WN_EPI_PLAIN;
  }
  Gemm& seg(const float* x, int ldx, int K, int shift, const float* frag) {
    WnSeg& s = a.seg[a.nseg++];
    s.x = x; s.ldx = ldx; s.K = K; s.shift = shift; s.frag = frag;
    s.vec = (ldx % 4 == 0 && K % 4 == 0 && al16(x)) ? 1 : 0;
    s.plane_k = 0; s.plane_stride = 0;
    return *this;
  }
  // block-major operand [K / plane_k][rows][plane_k] (the gated activations Z of all blocks)
  Gemm& seg_planes(const float* x, int plane_k, int64_t plane_stride, int K, const float* frag) {
    seg(x, plane_k, K, 0, frag);
    WnSeg& s = a.seg[a.nseg - 1];
    s.plane_k = plane_k; s.plane_stride = plane_stride;
    s.vec = (plane_k % 4 == 0 && plane_stride % 4 == 0 && al16(x)) ? 1 : 0;
    return *this;
  }
  Gemm& bias(const float* b) { a.bias = b; return *this; }
  // frames > 1: one row of b per (utterance, frame of hop rows), hop % 32 == 0 (local conditioning)
  Gemm& rowbias(const float* b, int ld, int frames = 0, int hop = 0) {
    a.rowbias = b; a.ld_rowbias = ld; a.rb_frames = frames; a.rb_hop = hop;
    return *this;
  }
  Gemm& addc(const float* c, int ld) { a.addc = c; a.ld_addc = ld; return *this; }
  Gemm& act(int act) { a.act = act; return *this; }
  Gemm& dact(const float* ysaved, int ld, int act) { a.epi = WN_EPI_DACT; a.aux = ysaved; a.ld_aux = ld; a.act = act; return *this; }
  Gemm& gate_bwd(const float* g, int ldg, const float* z, int ldz) {
    a.epi = WN_EPI_GATE_BWD; a.aux = g; a.ld_aux = ldg; a.aux2 = z; a.ld_aux2 = ldz;
    return *this;
  }
  Gemm& gate_fwd(float* sig, int ld) { a.epi = WN_EPI_GATE_FWD; a.y2 = sig; a.ld_y2 = ld; return *this; }
  int run(float* y, int ldy, hipStream_t s) {
    a.y = y; a.ldy = ldy;
    bool v = (a.N % 4 == 0) && (ldy % 4 == 0) && al16(y);
    if (a.bias) v = v && al16(a.bias);
    if (a.addc) v = v && (a.ld_addc % 4 == 0) && al16(a.addc);
    if (a.aux) v = v && (a.ld_aux % 4 == 0) && al16(a.aux);
    if (a.aux2) v = v && (a.ld_aux2 % 4 == 0) && al16(a.aux2);
    if (a.y2) v = v && (a.ld_y2 % 4 == 0) && al16(a.y2);
    a.vec_out = v ? 1 : 0;
    // The split-precision rows kernels read one row bias per utterance.  No call hands them a row per frame today (block_forward
    // takes its two-contraction form only without a conditioning bias); one that did would otherwise drop to the exact-fp32
    // kernel without a word
    if (w16_ && a.rowbias && a.rb_frames > 1 && wn_debug_get(1) != 1) {
      wn_set_error("a row bias per frame on the split-precision rows contraction is not built (local conditioning)");
      return WN_E_UNSUPPORTED;
    }
    // knob 1 = 1 forces the exact-fp32 MFMA kernels
    if (w16_ && wn_debug_get(1) != 1 && wn_gemm_rows16_ok(a)) return wn_launch_gemm_rows16(a, w16_, am0_, am1_, amo_, s);
    if (a.epi == WN_EPI_GATE_FWD) { wn_set_error("gate-forward contraction needs the split-precision kernel (alignment / shape)"); return WN_E_UNSUPPORTED; }
    for (int i = 0; i < a.nseg; ++i)
      if (!a.seg[i].frag) { wn_set_error("contraction without an fp32 weight image needs the split-precision kernel"); return WN_E_UNSUPPORTED; }
    const int rc = wn_launch_gemm_rows(a, s);
    // A gradient inside a split-precision chain (32 output columns without a padded image, an operand width the images do
    // not take): the next product and the weight-gradient jobs scale it by its max-abs slot, which the exact-fp32 kernel
    // does not keep -- taken from the result.  (The gate-derivative epilogue writes both halves of u: 2 N columns.)
    if (rc || !amo_ || a.absmax_any || wn_debug_get(1) == 1) return rc;
    return wn_launch_absmax(y, (int64_t)a.B * a.T, a.epi == WN_EPI_GATE_BWD ? 2 * a.N : a.N, ldy, amo_, s);
  }
};

// Training passes of a 256-class categorical head: the loss runs as the epilogue of the head's last conv
// (wn_gemm_planes16s_kernel<1, 8, -3>): where that launch puts its results.  forward_core sets `done` when it took the
// fused path (the logits are then never written); loss_stage only sums the row losses.
struct LossFuse {
  const int32_t* target; float gscale; float* loss_rows; float* g_logits; float* absmax_out;
  float* sample_out; float inv_lv; uint64_t seed, offset;
  const float* row_weight;     // [rows] sample_weight of the rows, or null (the unweighted instantiation)
  bool done;
  // wn_score: the evaluation form of the epilogue (<1, 8, -5> / <1, 8, -6>): the loss rows and nothing else -- g_logits,
  // absmax_out, gscale and the draw are not used
  bool eval;
};

// The streamed kernel's second form (wn_gemm_planes16s_kernel): one builder for its arguments, one test for "does it take
// this contraction".
struct Planes {
  WnGemmPlanesArgs a;
  // The shape rule (with `taps`: of the shifted-planes form) and the kernel's 32-bit byte offsets: rows * w * 4 < 2^32 for
  // every row width w the calling site lists (the sites do not list the same ones: DESIGN.md section 27)
  static bool takes(bool taps, int N, int plane_k, int nplanes, int ld, int ldy, int64_t rows, std::initializer_list<int> widths) {
    if (!(taps ? wn_gemm_taps16s_supported(N, plane_k, nplanes, ld, ldy) : wn_gemm_planes16s_supported(N, plane_k, nplanes, ld, ldy)))
      return false;
    for (int w : widths)
      if (!((int64_t)rows * w * 4 < ((int64_t)1 << 32))) return false;
    return true;
  }
  Planes(int B, int T, int N) {
    memset(&a, 0, sizeof(a));
    a.B = B; a.T = T; a.N = N;
  }
  // plane q, row r: z + q * plane_stride + r * ld, plane_k columns of it
  Planes& operand(const float* z, int ld, int plane_k, int nplanes = 1, int64_t plane_stride = 0) {
    a.z = z; a.ld = ld; a.plane_k = plane_k; a.nplanes = nplanes; a.plane_stride = plane_stride;
    return *this;
  }
  // the n taps of a dilated conv as shifted planes of the one operand: tap t reads row time - (n - 1 - t) * step (backward
  // data: step = -dilation)
  Planes& taps(int n, int step) {
    a.nplanes = n; a.nshift = n;
    for (int t = 0; t < n; ++t) a.shift[t] = (n - 1 - t) * step;
    return *this;
  }
  Planes& w16(const float* img) { a.w16 = img; return *this; }
  Planes& bias(const float* b) { a.bias = b; return *this; }
  Planes& act(int act) { a.act = act; return *this; }
  Planes& absmax_fwd(float* out) { a.absmax_out = out; return *this; }     // forward range-guard slot
  // backward-data form: operand scaled by *am_in, the result's max-abs into am_out, * act'(aux) when aux is given
  Planes& bwd(const float* am_in, float* am_out, const float* aux = nullptr, int ld_aux = 0) {
    a.bwd = 1; a.absmax_in = am_in; a.absmax_out = am_out; a.aux = aux; a.ld_aux = ld_aux;
    return *this;
  }
  // the categorical loss as the epilogue (training or evaluation form); run() then takes lf.g_logits as y
  Planes& loss(const LossFuse& lf) {
    a.absmax_out = lf.absmax_out;
    a.cat_loss = lf.eval ? 2 : 1; a.target = lf.target; a.gscale = lf.gscale; a.loss_rows = lf.loss_rows;
    a.sample_out = lf.sample_out; a.inv_lv = lf.inv_lv; a.seed = lf.seed; a.offset = lf.offset;
    a.row_weight = lf.row_weight;
    return *this;
  }
  int run(float* y, int ldy, hipStream_t s) {
    a.y = y; a.ldy = ldy;
    return wn_launch_gemm_planes16s(a, s);
  }
};

struct BlockPtrs {
  // geometry
  int B, T, KS, R, D, S, Cin, depth, act, residual;
  int dil[16];
  // raw parameters
  const float* Wd[16]; const float* bd[16];
  const float* br; const float* bs; const float* bc;
  // images
  const float* Fd[16]; const float* Bd[16]; int64_t Fd_stride[16], Bd_stride[16];
  const float* Fr; const float* Br_;
  const float* Fs; const float* Bs;
  const float* Fc; const float* Bc;
  int Cc;                   // time-varying condition channels (standalone layer) or 0
  const float* cond;        // [rows][Cc]
  const float* cb;          // [B][2D] per-utterance conditioning bias (model) or null
  int cb_frames, cb_hop;    // cb_frames > 1: cb is [B * cb_frames][2D], row b * cb_frames + t / cb_hop (cb_hop % 32 == 0)
  bool fused;
  const float* F16d; const float* F16r;   // fp16 split images of the gated conv / conv1, or null
  const float* G16u; const float* G16x;   // fp16 split images of the backward-data products, or null
  const float* G16uf;                     // [W_r | V(b)]: skip path folded into the first head conv (training), or null
  const float* F16g;                      // gated conv, row tiles [f f g g] per 64 channels (composed split-precision forward), or null
  const float* F16n;                      // gated conv, natural row-tile order, for the streamed one-kernel forward (R = D = 128), or null
  // depth > 1, training passes (set by deep16_ptrs): split-precision images of the non-gated convs (forward) and of every
  // conv's backward-data product; JTi / JTb = row tiles of those images (32-wide outputs are padded to 2)
  const float* F16i[16]; const float* G16i[16];
  int JTi[16], JTb[16], JTu;
};

struct BlockBufs {
  const float* x;           // [rows][Cin]
  float* P[16];             // outputs of non-gated convs [rows][D]
  float* U;                 // [rows][2D] scratch
  float* AG;                // [rows][D] saved sigmoid or null
  float* Z; int ldz;        // gated activations
  float* O;                 // [rows][R] pre-residual output or null
  float* x_out;             // [rows][R]
  const float* xt[3];       // queued generation: per-tap input rows (no time shift), or null
  const float* res;         // residual source when it is not x (dropout: x is the dropped copy), or null
  bool pre_done;            // queued generation: the non-gated convs already ran, xt[] are the gated conv's taps
  float* fwd_absmax;        // forward range guard slot (running max-abs of x_out), or null
};

struct BlockGrads {
  const float* g_xout;      // [rows][R] or null (treated as zero)
  const float* g_skip;      // [rows][Sh] or null; Sh = S, or R when S == 0 (skip = pre-residual o)
  float* g_o_tmp;           // [rows][R] scratch (needed when S == 0 and both grads exist)
  float* g_u;               // [rows][2D] scratch
  float* g_p;               // [2][rows][D] scratch (depth > 1), halves used alternately
  float* g_pi[16];          // deferred weight gradients: where the gradient of conv i's pre-activation output is KEPT, or null
  float* g_x;               // [rows][Cin] out (may be null when not needed)
  float* g_cond;            // [rows][Cc] out or null
  float* dWd[16]; float* dbd[16];
  float* dWr; float* dbr; float* dWs; float* dbs; float* dWc; float* dbc;
  float* dcb;               // [B][2D] per-utterance sums of g_u (model conditioning) or null
  float* slab;
  bool defer;               // weight gradients are computed later by the batched job table
  const float* am_gxout; const float* am_gskip;   // running max-abs of g_xout / g_skip (or null)
  float* am_gu; float* am_gx;                      // where to publish max-abs of g_u / g_x (or null)
  float* am_gp[16];                                // ... of the kept inner gradients g_pi[i] (deep stacks in training), or null
  const float* g_fold; int fold_F0; const float* am_gfold;   // folded skip path: dL/da of the first head conv [rows][F0] replaces g_skip
  float drop_rate; uint32_t drop_key; float* g_xd;  // dropout on the block input: mask the conv-path gradient
};

// queued generation state: per block a ring of its most recent input rows, [slot][B][R]
struct GenRings {
  float* xin;                  // [KS][B] raw samples
  std::vector<float*> h;       // per block: [nslots_b][B][R] inputs of the block's first dilated conv
  std::vector<int> nslots;
  // layers_per_block > 1: hp[b][i] = [nslots_p[b][i]][B][D] inputs of dilated conv i + 1 (= outputs of conv i)
  std::vector<std::vector<float*>> hp;
  std::vector<std::vector<int>> nslots_p;
  // the time of the captured window's index 0: index t of the priming pass goes to slot (t + t0) % nslots (0 unless the
  // sequence begins at a position other than 0, wn_generate_rows_begin)
  int64_t t0 = 0;
};

inline bool m16(int v) { return v > 0 && v % 16 == 0; }
inline bool m32(int v) { return v >= 64 && v % 32 == 0; }

// ---- wn_plan.hip ----
int ensure_device_tables(wn_plan* p);
WsLayout make_layout(const wn_plan* p, int B, int T, bool training);
bool deep16(const wn_plan* p);
bool cond_small(const wn_plan* p);
bool fold_ok(const wn_plan* p);
bool head_pairs_ok(const wn_plan* p);
TrainPaths train_paths(const wn_plan* p);   // the plan-level part; the per-call part as of a call without dropout or splits
TrainPaths train_paths(const wn_plan* p, const wn_exec& e, const WsLayout& L, int64_t rows);
// (cu_count: the device's compute units; relay_area: the generation workspace carries the relay's granule areas)
GenPaths gen_paths(const wn_plan* p, int B, int length, int cu_count, bool relay_area, bool deterministic, const WnSampleCtl& ctl);
// (e: the calling state, for its dropout rate; rings: the generation priming pass captures the rings)
FwdPaths fwd_paths(const wn_plan* p, const wn_exec& e, int B, int T, bool training, bool prep, bool rings, FwdLoss loss);
int64_t slab_need(int B, int T, int K, int N);
// ---- wn_block.hip ----
int wgrad(const float* x, int ldx, int K, int shift, const float* g, int ldg, int N, int B, int T,
          float* dW, float* db, float* per_batch, float* slab, hipStream_t s);
BlockFwdPath block_fwd_path(const BlockPtrs& k, const BlockBufs& f);
BlockBwdPath block_bwd_path(const BlockPtrs& k, const BlockBufs& f, const BlockGrads& g);
int block_forward(const BlockPtrs& k, const BlockBufs& f, hipStream_t s);
int block_backward(const BlockPtrs& k, const BlockBufs& f, const BlockGrads& g, hipStream_t s);
// ---- wn_forward.hip ----
bool loss_fusable(const wn_plan* p, int64_t rows);
BlockPtrs block_ptrs(const wn_plan* p, int b, const float* params, const float* fragbase, int B, int T);
void deep16_ptrs(const wn_plan* p, int b, const float* fragbase, BlockPtrs& k);
// the buffers of block b in the workspace of layout L: its input (drop: the dropped copy, the original as the residual
// source), the stack's activations, the saved sigmoid (training layouts) and its plane of Z -- what the forward pass writes
// and the backward pass reads
BlockBufs block_bufs(const wn_plan* p, const WsLayout& L, float* ws, int b, int64_t rows, bool training, bool drop);
int forward_core(wn_plan* p, const float* params, const float* x, bool prep, const float* cond, int B,
                 int T, bool training, float* ws, const WsLayout& L, hipStream_t s, const GenRings* rings = nullptr,
                 LossFuse* lf = nullptr);
// the conditioning phase of a forward pass alone: mapping stack and the blocks' bias table cb into the workspace of layout L
// (wn_generate_set_condition: a new condition into the table a queued generation step reads)
int condition_only(wn_plan* p, const float* params, const float* cond, int B, int T, float* ws, const WsLayout& L, hipStream_t s);
// ... over `rows` condition rows into a buffer of the caller's (wn_generate_frames_build): M, cb and cbt of L are offsets into
// `buf` (L.frames = 1), the weight images are read at `fragbase`, which belongs to a primed workspace and is not written
int condition_rows(wn_plan* p, const float* params, const float* cond, int rows, const float* fragbase, float* buf,
                   const WsLayout& L, hipStream_t s);
// what a pass hands back from the logits in the workspace: a copy of them, and the model output (their softmax for a
// categorical head, the logits themselves for a mixture head); either may be null
int emit_outputs(const wn_plan* p, const float* ws, const WsLayout& L, int64_t rows, float* logits_out, float* out, hipStream_t s);
// inputs = x[:, :-1], y_true = x[:, 1:]  (src/model.py:319-321)
int shift_split(const float* x_full, int B, int T, float* inputs, float* y_true, hipStream_t s);
int loss_stage(wn_plan* p, int B, int T, int global_batch, bool want_grad, float* ws, const WsLayout& L,
               float* loss_out, float* absmax_out, hipStream_t s, bool fused_done = false, const float* row_weight = nullptr);
// the standalone loss kernel of the head on the logits in the workspace: the row losses (and d loss / d logits when
// g_logits is given).  loss_stage is this plus the sum of the rows; wn_score takes the rows as they are
int loss_rows_stage(wn_plan* p, int64_t rows, float gscale, float* g_logits, bool want_grad, float* ws, const WsLayout& L,
                    float* absmax_out, hipStream_t s, const float* row_weight);
// the armed row weights against the rows of a call: WN_E_INVALID with both numbers, before the device is touched
int row_weights_check(const char* who, const wn_exec& e, int B, int T);
// the armed condition frames against a call over T inputs: the frames per utterance (>= 1), or WN_E_INVALID (negative) with
// T, the frames and the hop in the message when T % frames != 0 or the hop is no multiple of 32; before the device is touched
int cond_frames_check(const char* who, const wn_plan* p, int T);

}  // namespace wnp

// ---- wn_generate.hip ----
// the sampling arguments of wn_generate_sampled / wn_sample_waveform_sampled -> the controls the kernels take
int wn_sampling_check(const char* who, const wn_sampling* sp, int head, int classes, WnSampleCtl* ctl);
