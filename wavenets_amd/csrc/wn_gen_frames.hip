// Frame schedules of queued generation: the current frame of every scheduled row into the compact
// bias table the step kernels read.
//
// A request's bias rows for all of its frames are built once (wn_generate_frames_build) into a table of its own,
// [N][rows][2D].  The step kernels keep reading cb[N][B][2D] of the session's workspace; at the steps where some row's frame
// changes the host puts this launch in front of the launch that reads cb for the step:
//     cb[n][b][:] = rows_b[n * block_stride_b + f_b * 2D ..],   f_b = clamp((t - origin_b) / hop_b, 0, frames_b - 1)
// for every block n and every row b whose record has rows != null.  A row whose frame did not change is written with the
// bits it holds, so the kernel does not know which rows crossed a boundary.
//
// One workgroup of one wave per (row, block); all blocks in one launch.  The record is indexed by blockIdx alone, so its
// read and the frame arithmetic are wave-uniform.  The 2D floats of a row go as float4 where every pointer of the launch is
// 16-byte aligned, one float per lane otherwise.  Plain loads and stores.
#include "wn_kernels.h"

namespace {

template <bool VEC>
__global__ __launch_bounds__(64) void wn_gen_frame_copy_kernel(const wn_frame_row* __restrict__ recs, int B, int D2, int64_t t,
                                                               float* __restrict__ cb) {
  const int b = blockIdx.x, n = blockIdx.y;
  const wn_frame_row r = recs[b];
  if (!r.rows) return;                                  // off the schedule: its cb rows stay as they are
  int64_t f = (t - r.origin) / r.hop;
  f = f < 0 ? 0 : (f >= r.frames ? (int64_t)r.frames - 1 : f);
  const float* src = r.rows + (int64_t)n * r.block_stride + f * D2;
  float* dst = cb + ((int64_t)n * B + b) * D2;
  if (VEC) {
    for (int i = threadIdx.x; i < D2 / 4; i += 64) reinterpret_cast<f32x4*>(dst)[i] = reinterpret_cast<const f32x4*>(src)[i];
  } else {
    for (int i = threadIdx.x; i < D2; i += 64) dst[i] = src[i];
  }
}

}  // namespace

int wn_launch_gen_frame_copy(const wn_frame_row* recs, bool recs_vec, int B, int N, int D2, int64_t t, float* cb, hipStream_t s) {
  if (!recs || !cb || B < 1 || N < 1 || D2 < 1 || N > 65535) {
    wn_set_error("gen_frame_copy: bad geometry (B = %d rows, %d blocks, %d floats a row)", B, N, D2);
    return WN_E_INVALID;
  }
  const dim3 grid((unsigned)B, (unsigned)N);
  const bool vec = recs_vec && D2 % 4 == 0 && (((uintptr_t)cb) & 15) == 0;
  if (vec) hipLaunchKernelGGL(wn_gen_frame_copy_kernel<true>, grid, dim3(64), 0, s, recs, B, D2, t, cb);
  else hipLaunchKernelGGL(wn_gen_frame_copy_kernel<false>, grid, dim3(64), 0, s, recs, B, D2, t, cb);
  WN_HIP_CHECK(hipGetLastError());
  return WN_OK;
}
