// Local conditioning, backward: the per-frame sums of every block's g_u.
//
// The condition of frame f of utterance b enters block n as the bias row cb[n][b * F + f][0 .. 2D) of the rows
// t in [f * hop, (f + 1) * hop), so its gradient is the sum of g_u(n) over those rows:
//     dcb[(b, f)][n][:] = sum_{t in frame f} g_u(n)[b, t, :]
// written in the layout the conditioning backward already reads, (Bc, N * 2D) with Bc = B * F (WsLayout::cbt).  From there
// the products are the ones of global conditioning with Bc rows in place of B.
//
// One workgroup per (condition row, block); all blocks in one launch (block n's g_u at gu + n * gu_stride: the training
// workspace carves them at one stride).  The 2D columns lie on lanes as float4 (2D / 4 lanes
// hold one row, a wave of 64 lanes holds RPW = 256 / 2D rows at a time), the rows of the frame are dealt to the waves in
// turn, and every lane adds its rows in ascending time.  The partial sums meet in LDS and one thread per column adds them in
// a fixed order (wave 0's row groups first, then wave 1's, ...): no atomics, the same bits on every run.
// g_u is stored in its own units on every chain (the split-precision chains scale their OPERAND copies by the max-abs
// slots, the stored tensor is unscaled), so the sums need no factor.
#include "wn_kernels.h"

namespace {

constexpr int CF_WAVES = 4;

template <int Q>     // Q = 2D / 4 float4 columns: a power of two <= 64
__global__ __launch_bounds__(64 * CF_WAVES) void wn_cond_frame_sum_kernel(const float* gu, int64_t gu_stride, int N, int F,
                                                                          int T, int hop, float* dcb) {
  constexpr int RPW = 64 / Q;                        // rows a wave reads per step
  constexpr int GROUPS = CF_WAVES * RPW;             // partial sums per column
  __shared__ f32x4 part[GROUPS][Q];
  const int row = blockIdx.x;                        // condition row b * F + f
  const int n = blockIdx.y;
  const int b = row / F, f = row % F;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int q = lane % Q, r = lane / Q;              // column quad, row inside the wave's step
  const float* g = gu + (int64_t)n * gu_stride + ((int64_t)b * T + (int64_t)f * hop) * (4 * Q) + 4 * q;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  for (int t = wave * RPW + r; t < hop; t += GROUPS) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(g + (int64_t)t * (4 * Q));
    acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
  }
  part[wave * RPW + r][q] = acc;
  __syncthreads();
  if (threadIdx.x < Q) {
    f32x4 s = part[0][threadIdx.x];
    for (int i = 1; i < GROUPS; ++i) {
      const f32x4 v = part[i][threadIdx.x];
      s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
    }
    *reinterpret_cast<f32x4*>(dcb + ((int64_t)row * N + n) * (4 * Q) + 4 * threadIdx.x) = s;
  }
}

// any width: one thread per column, rows in ascending time (widths the float4 form does not take)
__global__ __launch_bounds__(256) void wn_cond_frame_sum_any_kernel(const float* gu, int64_t gu_stride, int N, int F, int T,
                                                                    int hop, int D2, float* dcb) {
  const int row = blockIdx.x, n = blockIdx.y;
  const int b = row / F, f = row % F;
  const float* g = gu + (int64_t)n * gu_stride + ((int64_t)b * T + (int64_t)f * hop) * D2;
  for (int c = threadIdx.x; c < D2; c += blockDim.x) {
    float acc = 0.f;
    for (int t = 0; t < hop; ++t) acc += g[(int64_t)t * D2 + c];
    dcb[((int64_t)row * N + n) * D2 + c] = acc;
  }
}

}  // namespace

int wn_launch_cond_frame_sum(const float* gu, int64_t gu_stride, int B, int T, int F, int N, int D2, float* dcb,
                             hipStream_t s) {
  if (B < 1 || F < 1 || N < 1 || D2 < 1 || T % F != 0) { wn_set_error("cond_frame_sum: bad geometry"); return WN_E_INVALID; }
  const int hop = T / F;
  const dim3 grid((unsigned)(B * F), (unsigned)N);
  const bool al = (((uintptr_t)gu) & 15) == 0 && gu_stride % 4 == 0 && (((uintptr_t)dcb) & 15) == 0;
  switch (al ? D2 : 0) {
    case 64: hipLaunchKernelGGL((wn_cond_frame_sum_kernel<16>), grid, dim3(64 * CF_WAVES), 0, s, gu, gu_stride, N, F, T, hop, dcb); break;
    case 128: hipLaunchKernelGGL((wn_cond_frame_sum_kernel<32>), grid, dim3(64 * CF_WAVES), 0, s, gu, gu_stride, N, F, T, hop, dcb); break;
    case 256: hipLaunchKernelGGL((wn_cond_frame_sum_kernel<64>), grid, dim3(64 * CF_WAVES), 0, s, gu, gu_stride, N, F, T, hop, dcb); break;
    default: hipLaunchKernelGGL(wn_cond_frame_sum_any_kernel, grid, dim3(256), 0, s, gu, gu_stride, N, F, T, hop, D2, dcb); break;
  }
  WN_HIP_CHECK(hipGetLastError());
  return WN_OK;
}
