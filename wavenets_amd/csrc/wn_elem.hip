// Elementwise and small dense kernels of the WaveNet hot path (gfx950); losses: wn_loss.hip, samplers: wn_sample.hip,
// optimizer: wn_optim.hip.  References: quantiser src/model.py:151-153; mu-law src/utils.py:34-35; inverse
// src/callbacks.py:126-131.
#include <algorithm>

#include "wn_kernels.h"
#include "wn_sample.h"

// ------------------------------------------------------------------------------------------
__global__ void wn_add_kernel(const float* a, const float* b, float* out, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x)
    out[i] = a[i] + b[i];
}
int wn_launch_add(const float* a, const float* b, float* out, int64_t n, hipStream_t s) {
  if (n <= 0) return WN_OK;
  hipLaunchKernelGGL(wn_add_kernel, dim3(wn_blocks(n)), dim3(256), 0, s, a, b, out, n);
  WN_HIP_CHECK(hipGetLastError());
  return WN_OK;
}

__global__ void wn_fill_kernel(float* p, float v, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x)
    p[i] = v;
}
int wn_launch_fill(float* p, float v, int64_t n, hipStream_t s) {
  if (n <= 0) return WN_OK;
  hipLaunchKernelGGL(wn_fill_kernel, dim3(wn_blocks(n)), dim3(256), 0, s, p, v, n);
  WN_HIP_CHECK(hipGetLastError());
  return WN_OK;
}

// out[b][c] = sum_t g[b][t][c]: stage 1 sums WN_CS_CHUNKS time chunks per utterance in parallel
// (one block per (utterance, chunk, 64 channels)), stage 2 folds the chunks in a fixed order.
#define WN_CS_CHUNKS 128
__global__ void wn_colsum_stage1(const float* g, int T, int C, float* part) {
  __shared__ float sm[256];
  const int b = blockIdx.x, chunk = blockIdx.y;
  const int c = blockIdx.z * 64 + (threadIdx.x & 63);
  const int p = threadIdx.x >> 6;
  const int len = (T + WN_CS_CHUNKS - 1) / WN_CS_CHUNKS;
  const int t0 = chunk * len, t1 = min(T, t0 + len);
  float acc = 0.f;
  if (c < C)
    for (int t = t0 + p; t < t1; t += 4) acc += g[((int64_t)b * T + t) * C + c];
  sm[threadIdx.x] = acc;
  __syncthreads();
  if (p == 0 && c < C)
    part[((int64_t)b * WN_CS_CHUNKS + chunk) * C + c] = sm[threadIdx.x] + sm[threadIdx.x + 64] + sm[threadIdx.x + 128] + sm[threadIdx.x + 192];
}
__global__ void wn_colsum_stage2(const float* part, int C, float* out, int64_t total) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int64_t b = i / C;
  const int c = (int)(i % C);
  double acc = 0.0;
  for (int k = 0; k < WN_CS_CHUNKS; ++k) acc += (double)part[(b * WN_CS_CHUNKS + k) * C + c];
  out[i] = (float)acc;
}
// scratch: B * WN_CS_CHUNKS * C floats
int64_t wn_colsum_scratch_floats(int B, int C) { return (int64_t)B * WN_CS_CHUNKS * C; }
int wn_launch_colsum_per_batch(const float* g, int B, int T, int C, float* out, float* scratch, hipStream_t s) {
  hipLaunchKernelGGL(wn_colsum_stage1, dim3(B, WN_CS_CHUNKS, (C + 63) / 64), dim3(256), 0, s, g, T, C, scratch);
  const int64_t total = (int64_t)B * C;
  hipLaunchKernelGGL(wn_colsum_stage2, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, scratch, C, out, total);
  WN_HIP_CHECK(hipGetLastError());
  return WN_OK;
}

// ------------------------------------------------------------------------------------------
// quantiser: index = #{ j in 1..2^bits-1 : edge_j <= x },  edge_j = -1 + j * 2^(1-bits) (exact in
// fp32).  Candidate from arithmetic, then corrected against the exact edges so that the result is
// the upper-bound search of tf Bucketize bit for bit.
__device__ __forceinline__ int wn_quantize_one(float x, int bits) {
  const int nmax = (1 << bits) - 1;
  const double step = ldexp(1.0, 1 - bits);
  double f = floor(((double)x + 1.0) / step);
  int idx = f < 0.0 ? 0 : (f > (double)nmax ? nmax : (int)f);
  while (idx > 0 && (float)(-1.0 + idx * step) > x) --idx;
  while (idx < nmax && (float)(-1.0 + (idx + 1) * step) <= x) ++idx;
  return idx;
}
__global__ void wn_quantize_kernel(const float* x, int32_t* idx, int64_t n, int bits) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x)
    idx[i] = wn_quantize_one(x[i], bits);
}
int wn_launch_quantize(const float* x, int32_t* idx, int64_t n, int bits, hipStream_t s) {
  if (n <= 0) return WN_OK;
  if (bits < 1 || bits > 16) { wn_set_error("quantize: bits %d unsupported", bits); return WN_E_UNSUPPORTED; }
  hipLaunchKernelGGL(wn_quantize_kernel, dim3(wn_blocks(n)), dim3(256), 0, s, x, idx, n, bits);
  WN_HIP_CHECK(hipGetLastError());
  return WN_OK;
}

__global__ void wn_dequantize_kernel(const int32_t* idx, float* x, int64_t n, float inv) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x)
    x[i] = (float)idx[i] * inv - 1.0f;       // i / 2^(bits-1) - 1  (src/model.py:411,418)
}
int wn_launch_dequantize(const int32_t* idx, float* x, int64_t n, int bits, hipStream_t s) {
  if (n <= 0) return WN_OK;
  hipLaunchKernelGGL(wn_dequantize_kernel, dim3(wn_blocks(n)), dim3(256), 0, s, idx, x, n,
                     1.0f / (float)(1 << (bits - 1)));
  WN_HIP_CHECK(hipGetLastError());
  return WN_OK;
}

__global__ void wn_mulaw_kernel(const float* x, float* y, int64_t n) {
  const float inv = 1.0f / logf(256.0f);
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    const float v = x[i];
    const float sgn = v > 0.f ? 1.f : (v < 0.f ? -1.f : 0.f);
    y[i] = sgn * (logf(1.0f + 255.0f * fabsf(v)) * inv);
  }
}
int wn_launch_mulaw(const float* x, float* y, int64_t n, hipStream_t s) {
  if (n <= 0) return WN_OK;
  hipLaunchKernelGGL(wn_mulaw_kernel, dim3(wn_blocks(n)), dim3(256), 0, s, x, y, n);
  WN_HIP_CHECK(hipGetLastError());
  return WN_OK;
}

__global__ void wn_inv_mulaw_kernel(const float* y, float* x, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    const float v = y[i];
    const float sgn = v > 0.f ? 1.f : (v < 0.f ? -1.f : 0.f);
    x[i] = sgn * (powf(256.0f, fabsf(v)) - 1.0f) / 255.0f;
  }
}
int wn_launch_inv_mulaw(const float* y, float* x, int64_t n, hipStream_t s) {
  if (n <= 0) return WN_OK;
  hipLaunchKernelGGL(wn_inv_mulaw_kernel, dim3(wn_blocks(n)), dim3(256), 0, s, y, x, n);
  WN_HIP_CHECK(hipGetLastError());
  return WN_OK;
}

// ------------------------------------------------------------------------------------------
// gate of the composed (unfused) block path: u (rows, 2D) -> a = tanh(u[:, :D]), g = sigmoid(u[:, D:]),
// z = a * g   (src/layers.py:208-210)
__global__ void wn_gate_kernel(const float* u, int64_t rows, int D, float* ag, float* z, int ldz) {
  const int64_t total = rows * D;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = i / D;
    const int c = (int)(i % D);
    const float a = wn_tanh_fast(u[r * 2 * D + c]);
    const float g = wn_sigmoid_fast(u[r * 2 * D + D + c]);
    if (ag) ag[r * D + c] = g;          // saved sigmoid only (tanh = z / sigmoid in backward)
    if (z) z[r * ldz + c] = a * g;
  }
}
int wn_launch_gate(const float* u, int64_t rows, int D, float* ag, float* z, int ldz, hipStream_t s) {
  if (rows <= 0) return WN_OK;
  hipLaunchKernelGGL(wn_gate_kernel, dim3(wn_blocks(rows * D)), dim3(256), 0, s, u, rows, D, ag, z, ldz);
  WN_HIP_CHECK(hipGetLastError());
  return WN_OK;
}

// out[b][n] = sum_sp slab[b][sp][n]
__global__ void wn_batch_reduce_kernel(const float* slab, int splits, int N, float* out, int64_t total) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int64_t b = i / N;
  const int n = (int)(i % N);
  float acc = 0.f;
  for (int s = 0; s < splits; ++s) acc += slab[(b * splits + s) * N + n];
  out[i] = acc;
}
int wn_launch_batch_reduce(const float* slab, int B, int splits, int N, float* out, hipStream_t s) {
  const int64_t total = (int64_t)B * N;
  if (total <= 0) return WN_OK;
  hipLaunchKernelGGL(wn_batch_reduce_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s,
                     slab, splits, N, out, total);
  WN_HIP_CHECK(hipGetLastError());
  return WN_OK;
}

// y[off + i] += coef * x[off + i] over the tensors of a table (L2 regulariser gradient)
__global__ void wn_axpy_table_kernel(float* y, const float* x, const WnTensorDesc* table, float coef) {
  const WnTensorDesc d = table[blockIdx.y];
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < d.len;
       i += (int64_t)gridDim.x * blockDim.x)
    y[d.off + i] += coef * x[d.off + i];
}
int wn_launch_axpy_table(float* y, const float* x, const WnTensorDesc* d_table, int n, float coef,
                         hipStream_t s) {
  if (n <= 0) return WN_OK;
  hipLaunchKernelGGL(wn_axpy_table_kernel, dim3(16, n), dim3(256), 0, s, y, x, d_table, coef);
  WN_HIP_CHECK(hipGetLastError());
  return WN_OK;
}

// out = g * act'(y)   (y = saved activation output)
__global__ void wn_dact_mul_kernel(const float* g, const float* y, float* out, int64_t n, int act) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x)
    out[i] = g[i] * wn_dact_from_y(y[i], act);
}
int wn_launch_dact_mul(const float* g, const float* y, float* out, int64_t n, int act, hipStream_t s) {
  if (n <= 0) return WN_OK;
  hipLaunchKernelGGL(wn_dact_mul_kernel, dim3(wn_blocks(n)), dim3(256), 0, s, g, y, out, n, act);
  WN_HIP_CHECK(hipGetLastError());
  return WN_OK;
}

// ------------------------------------------------------------------------------------------
// Dropout on the block input (src/layers.py:108-111,195-196): keep-mask from a counter-based integer
// hash of (seed, block, step, element index) -- reproducible, stateless, identical in forward and
// backward (TF's own random stream is not reproducible; the CPU oracle restates this hash).
//   forward : xd = keep ? x / (1 - rate) : 0
//   backward: g_x = (keep ? g_xd / (1 - rate) : 0) + g_res      (g_res = residual path, may be null)
__device__ __forceinline__ uint32_t wn_hash32(uint32_t x) {
  x ^= x >> 16; x *= 0x7feb352dU; x ^= x >> 15; x *= 0x846ca68bU; x ^= x >> 16;
  return x;
}
__device__ __forceinline__ bool wn_drop_keep(int64_t idx, uint32_t key, float rate) {
  const uint32_t lo = (uint32_t)idx, hi = (uint32_t)((uint64_t)idx >> 32);
  const uint32_t hsh = wn_hash32(lo ^ wn_hash32(hi + key));
  return (float)(hsh >> 8) * (1.0f / 16777216.0f) >= rate;
}
__global__ void wn_dropout_kernel(const float* x, const float* g_res, float* out, int64_t n, float rate, float scale,
                                  uint32_t key, float* absmax_out) {
  float m = 0.f;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    float v = wn_drop_keep(i, key, rate) ? x[i] * scale : 0.f;
    if (g_res) v += g_res[i];
    out[i] = v;
    m = fmaxf(m, fabsf(v));
  }
  if (absmax_out) {
    m = wn_wave_max(m);
    if ((threadIdx.x & 63) == 0) wn_absmax_publish(absmax_out, m);
  }
}
uint32_t wn_dropout_key(uint64_t seed, int block, uint64_t step) {
  uint32_t k = (uint32_t)seed * 0x9E3779B9U + (uint32_t)(seed >> 32);
  k ^= (uint32_t)block * 0x85EBCA6BU + 0x1234567U;
  k ^= (uint32_t)step * 0xC2B2AE35U + (uint32_t)(step >> 32) * 0x27D4EB2FU;
  return k;
}
int wn_launch_dropout(const float* x, const float* g_res, float* out, int64_t n, float rate, uint32_t key,
                      float* absmax_out, hipStream_t s) {
  if (n <= 0) return WN_OK;
  hipLaunchKernelGGL(wn_dropout_kernel, dim3(wn_blocks(n)), dim3(256), 0, s, x, g_res, out, n, rate, 1.0f / (1.0f - rate),
                     key, absmax_out);
  WN_HIP_CHECK(hipGetLastError());
  return WN_OK;
}

// Running max-abs of a gradient tensor the exact-fp32 rows GEMM wrote (that kernel keeps none): what the split-precision
// products and weight-gradient jobs behind it scale their operand by.
__global__ void wn_absmax_kernel(const float* y, int64_t rows, int cols, int ld, float* slot) {
  const int64_t n = rows * cols;
  float m = 0.f;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    m = fmaxf(m, fabsf(y[(i / cols) * ld + i % cols]));
  m = wn_wave_max(m);
  if ((threadIdx.x & 63) == 0) wn_absmax_publish(slot, m);
}
int wn_launch_absmax(const float* y, int64_t rows, int cols, int ld, float* slot, hipStream_t s) {
  if (rows <= 0 || cols <= 0 || !slot) return WN_OK;
  hipLaunchKernelGGL(wn_absmax_kernel, dim3(wn_blocks(rows * cols)), dim3(256), 0, s, y, rows, cols, ld, slot);
  WN_HIP_CHECK(hipGetLastError());
  return WN_OK;
}

// ---------------------------------------------------------------------------------------------
// Global conditioning of ALL residual blocks at once (src/layers.py:116-120,203-204 with the
// time-invariant condition of src/model.py:221-225: conv_cond(repeat(m)) is a per-utterance bias).
// The N per-block 1x1 convs are one contraction tmp[B][N*2D] = m . [W_c^1 | ... | W_c^N]; these three
// kernels move between that layout and the per-block tensors.
// ---------------------------------------------------------------------------------------------
// cb[b][u][n] = tmp[u][b*2D + n] + b_c^b[n]
__global__ void wn_cond_scatter_kernel(const float* tmp, const float* params, int64_t b_off0, int64_t b_stride, int B,
                                       int N, int D2, float* cb) {
  const int64_t total = (int64_t)N * B * D2;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int n = (int)(i % D2);
    const int u = (int)((i / D2) % B);
    const int b = (int)(i / ((int64_t)D2 * B));
    cb[i] = tmp[((int64_t)u * N + b) * D2 + n] + params[b_off0 + (int64_t)b * b_stride + n];
  }
}
// dcb[u][b*2D + n] = sum over the time splits of utterance u of the db_d partial sums that the weight
// gradient kernels left in their slab rows (they ARE the per-utterance column sums of d u)
__global__ void wn_cond_gather_kernel(const float* slab, int64_t P, int spb, int64_t bd_off0, int64_t bd_stride, int B,
                                      int N, int D2, float* dcb) {
  const int64_t total = (int64_t)B * N * D2;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int n = (int)(i % D2);
    const int b = (int)((i / D2) % N);
    const int u = (int)(i / ((int64_t)D2 * N));
    float acc = 0.f;
    for (int sp = 0; sp < spb; ++sp) acc += slab[(int64_t)(u * spb + sp) * P + bd_off0 + (int64_t)b * bd_stride + n];
    dcb[i] = acc;
  }
}
// dW_c^b[c][n] = sum_u m[u][c] dcb[u][b*2D + n];  db_c^b[n] = sum_u dcb[u][b*2D + n]
__global__ void wn_cond_wgrad_kernel(const float* m, const float* dcb, int B, int Cc, int N, int D2, float* grads,
                                     int64_t w_off0, int64_t w_stride, int64_t b_off0, int64_t b_stride) {
  const int64_t total = (int64_t)N * (Cc + 1) * D2;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int n = (int)(i % D2);
    const int c = (int)((i / D2) % (Cc + 1));              // row Cc = the bias
    const int b = (int)(i / ((int64_t)D2 * (Cc + 1)));
    float acc = 0.f;
    for (int u = 0; u < B; ++u) {
      const float g = dcb[((int64_t)u * N + b) * D2 + n];
      acc += c < Cc ? m[(int64_t)u * Cc + c] * g : g;
    }
    if (c < Cc) grads[w_off0 + (int64_t)b * w_stride + (int64_t)c * D2 + n] = acc;
    else grads[b_off0 + (int64_t)b * b_stride + n] = acc;
  }
}
int wn_launch_cond_scatter(const float* tmp, const float* params, int64_t b_off0, int64_t b_stride, int B, int N, int D2,
                           float* cb, hipStream_t s) {
  const int64_t total = (int64_t)N * B * D2;
  hipLaunchKernelGGL(wn_cond_scatter_kernel, dim3((unsigned)std::min<int64_t>((total + 255) / 256, 1024)), dim3(256), 0, s, tmp,
                     params, b_off0, b_stride, B, N, D2, cb);
  WN_HIP_CHECK(hipGetLastError());
  return WN_OK;
}
int wn_launch_cond_gather(const float* slab, int64_t P, int spb, int64_t bd_off0, int64_t bd_stride, int B, int N, int D2,
                          float* dcb, hipStream_t s) {
  const int64_t total = (int64_t)B * N * D2;
  hipLaunchKernelGGL(wn_cond_gather_kernel, dim3((unsigned)std::min<int64_t>((total + 255) / 256, 1024)), dim3(256), 0, s, slab, P,
                     spb, bd_off0, bd_stride, B, N, D2, dcb);
  WN_HIP_CHECK(hipGetLastError());
  return WN_OK;
}
int wn_launch_cond_wgrad(const float* m, const float* dcb, int B, int Cc, int N, int D2, float* grads, int64_t w_off0,
                         int64_t w_stride, int64_t b_off0, int64_t b_stride, hipStream_t s) {
  const int64_t total = (int64_t)N * (Cc + 1) * D2;
  hipLaunchKernelGGL(wn_cond_wgrad_kernel, dim3((unsigned)std::min<int64_t>((total + 255) / 256, 1024)), dim3(256), 0, s, m, dcb, B,
                     Cc, N, D2, grads, w_off0, w_stride, b_off0, b_stride);
  WN_HIP_CHECK(hipGetLastError());
  return WN_OK;
}

// Input causal conv (C_in = 1, src/model.py:84-88,228): y[b][t][c] = b[c] + sum_tap w[tap][c] x[b][t-(KS-1-tap)].
// Arithmetic = the k-ordered fma chain from zero, then + bias: what the fp32 MFMA product it replaces
// computed and what the generation chain kernel (wn_gen.hip) reproduces, so all three agree bit for bit.
__global__ __launch_bounds__(256) void wn_inconv_fwd_kernel(const float* x, const float* w, const float* bias, int B, int T,
                                                            int R, int KS, float* y, float* absmax_out) {
  const int q = R / 4;                                   // float4 groups per row
  const int64_t total = (int64_t)B * T * q;
  float wmax = 0.f;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int c = (int)(i % q) * 4;
    const int64_t row = i / q;
    const int t = (int)(row % T);
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
    for (int tap = 0; tap < KS; ++tap) {
      const int ts = t - (KS - 1 - tap);
      const float xv = ts >= 0 ? x[row - (KS - 1 - tap)] : 0.f;
      const f32x4 wv = *reinterpret_cast<const f32x4*>(w + (int64_t)tap * R + c);
      a0 = fmaf(wv.x, xv, a0); a1 = fmaf(wv.y, xv, a1); a2 = fmaf(wv.z, xv, a2); a3 = fmaf(wv.w, xv, a3);
    }
    const f32x4 bv = *reinterpret_cast<const f32x4*>(bias + c);
    const f32x4 o = f32x4{a0 + bv.x, a1 + bv.y, a2 + bv.z, a3 + bv.w};
    *reinterpret_cast<f32x4*>(y + row * R + c) = o;
    wmax = fmaxf(wmax, fmaxf(fmaxf(fabsf(o.x), fabsf(o.y)), fmaxf(fabsf(o.z), fabsf(o.w))));
  }
  if (absmax_out) {                                      // forward range guard: running max-abs of the first block input
    // one atomic per WORKGROUP at most: thousands of waves finishing together on one address cost ~15 ns each
    __shared__ float wm[4];
    if (!(wmax < 3.0e38f)) wmax = 3.0e38f;               // inf / NaN count as "beyond any limit"
    wmax = wn_wave_max(wmax);
    if ((threadIdx.x & 63) == 0) wm[threadIdx.x >> 6] = wmax;
    __syncthreads();
    if (threadIdx.x == 0) wn_absmax_publish_any(absmax_out, fmaxf(fmaxf(wm[0], wm[1]), fmaxf(wm[2], wm[3])));
  }
}
int wn_launch_inconv_fwd(const float* x, const float* w, const float* bias, int B, int T, int R, int KS, float* y,
                         float* absmax_out, hipStream_t s) {
  const int64_t total = (int64_t)B * T * (R / 4);
  if (total <= 0) return WN_OK;
  hipLaunchKernelGGL(wn_inconv_fwd_kernel, dim3((unsigned)std::min<int64_t>((total + 255) / 256, 1024)), dim3(256), 0, s, x, w, bias,
                     B, T, R, KS, y, absmax_out);
  WN_HIP_CHECK(hipGetLastError());
  return WN_OK;
}

// The same conv's gradient at its input (wn_vjp): gx[b][t] = sum_tap sum_c w[tap][c] g[b][t + (KS-1-tap)][c], g = d / d y; a tap
// whose row lies at or beyond T belongs to no frame of the utterance and is dropped (utterances never mix).  One wave per
// (b, t), persistent; a lane sums its channels lane, lane + 64, ... tap by tap, then wn_wave_sum.  Any R, any KS.
__global__ __launch_bounds__(256) void wn_inconv_bwd_data_kernel(const float* g, const float* w, int B, int T, int R, int KS,
                                                                 float* gx) {
  const int lane = threadIdx.x & 63;
  const int64_t rows = (int64_t)B * T, stride = (int64_t)gridDim.x * 4;
  for (int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); row < rows; row += stride) {
    const int t = (int)(row % T);
    float acc = 0.f;
    for (int tap = 0; tap < KS; ++tap) {
      const int d = KS - 1 - tap;
      if (t + d >= T) continue;                          // (wave-uniform)
      const float* gr = g + (row + d) * R;
      const float* wr = w + (int64_t)tap * R;
      for (int c = lane; c < R; c += 64) acc = fmaf(wr[c], gr[c], acc);
    }
    acc = wn_wave_sum(acc);
    if (lane == 0) gx[row] = acc;
  }
}
int wn_launch_inconv_bwd_data(const float* g, const float* w, int B, int T, int R, int KS, float* gx, hipStream_t s) {
  const int64_t rows = (int64_t)B * T;
  if (rows <= 0) return WN_OK;
  hipLaunchKernelGGL(wn_inconv_bwd_data_kernel, dim3((unsigned)std::min<int64_t>((rows + 3) / 4, 2048)), dim3(256), 0, s, g, w, B, T,
                     R, KS, gx);
  WN_HIP_CHECK(hipGetLastError());
  return WN_OK;
}

// ------------------------------------------------------------------------------------------
// Skip path folded into the head's first convolution (training passes).
//   reference: skip_b = W_s(b)^T z_b + b_s(b)  (src/layers.py:216-217), x = sum_b skip_b  (src/model.py:235-236),
//              a = W_f0^T x + b_f0              (first head conv, src/model.py:105-111: conv, THEN activation)
// Both maps are linear with nothing in between, so  a = sum_b V(b)^T z_b + b',  V(b) = W_s(b) W_f0  (D x F0),
// b' = b_f0 + W_f0^T sum_b b_s(b).  With F0 < S every consumer of the S-wide tensors shrinks: the folded forward
// contraction has F0 instead of S output columns, each block's backward reads dL/da (rows x F0) instead of the
// gradient of the skip sum (rows x S), and the weight gradients of all conv_skip AND of the first head conv come from
// ONE rows-contraction  M = Z^T (dL/da)  (N*D x F0):
//   dW_s(b) = M(b) W_f0^T,  db_s(b) = W_f0 colsum(dL/da),  dW_f0 = sum_b W_s(b)^T M(b) + (sum_b b_s) colsum^T,  db_f0 = colsum.
// V and b' are formed below in plain fp32; the small backward products run on the exact-fp32 rows / weight-gradient
// GEMMs (wn_plan.hip) over [M; colsum] and [W_s(all blocks); sum b_s].  The reassociation moves results by ~1e-6
// relative, far inside the 1e-4 parity bar (checked against the oracle, which keeps the reference's order).
// Small dense fp32 product for the folded skip path's weight-space matrices and the conditioning path (a few thousand rows
// at most, operands L2-resident):  C[i][j] = sum_k A[i * sai + k * sak] * B[k * sbk + j * sbj],  i < M, j < N, k < K, C
// row-major with pitch ldc; the generic operand strides cover the plain, the B-transposed and the A-transposed product.
// 32 x 32 tile per workgroup and K in chunks of 128 whose loads are ALL in flight before the first product (one global
// round trip per chunk).  Plain fma chains, k ascending.
// blockIdx.z = batch index: operand / result bases advance by za / zb / zc floats (the conditioning convs of all blocks as
// one launch); bias (+ activation) = the Dense epilogue of the conditioning's mapping stack (src/model.py:121-135).
__global__ __launch_bounds__(256) void wn_sgemm_small32_kernel(const float* A, int64_t sai, int64_t sak, const float* B, int64_t sbk,
                                                               int64_t sbj, float* C, int ldc, int M, int N, int K,
                                                               int64_t za, int64_t zb, int64_t zc, const float* bias, int act,
                                                               int zk) {
  constexpr int KC = 128;
  __shared__ float As[KC][32 + 1], Bs[KC][32 + 1];
  A += (int64_t)blockIdx.z * za; B += (int64_t)blockIdx.z * zb; C += (int64_t)blockIdx.z * zc;
  // zk > 0: split K -- product z covers k in [z zk, min(K, (z + 1) zk)) of ONE long contraction (za / zb advance the
  // operands by zk rows of k); the partial results are summed by the caller
  if (zk > 0) K = max(0, min(K - (int)blockIdx.z * zk, zk));
  const int i0 = blockIdx.y * 32, j0 = blockIdx.x * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;          // outputs (ty + 8 a, tx), a < 4
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  for (int k0 = 0; k0 < K; k0 += KC) {
    float ra[16], rb[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const int e = threadIdx.x + 256 * q;                           // 32 x 128 elements of each operand
      // the faster-varying index follows the operand's unit stride (coalesced either way round)
      const int ka = sak == 1 ? e % KC : e / 32, ia = sak == 1 ? e / KC : e % 32;
      ra[q] = (i0 + ia < M && k0 + ka < K) ? A[(int64_t)(i0 + ia) * sai + (int64_t)(k0 + ka) * sak] : 0.f;
      const int kb = sbk == 1 ? e % KC : e / 32, jb = sbk == 1 ? e / KC : e % 32;
      rb[q] = (j0 + jb < N && k0 + kb < K) ? B[(int64_t)(k0 + kb) * sbk + (int64_t)(j0 + jb) * sbj] : 0.f;
    }
    if (k0 > 0) __syncthreads();                                     // the previous chunk has been read
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const int e = threadIdx.x + 256 * q;
      const int ka = sak == 1 ? e % KC : e / 32, ia = sak == 1 ? e / KC : e % 32;
      As[ka][ia] = ra[q];
      const int kb = sbk == 1 ? e % KC : e / 32, jb = sbk == 1 ? e / KC : e % 32;
      Bs[kb][jb] = rb[q];
    }
    __syncthreads();
    // (k past the end of K is stored as zero: fma(0, 0, acc) leaves acc as it is; fixed trip count so that the LDS reads
    // of eight k are in flight together)
#pragma unroll 8
    for (int k = 0; k < KC; ++k) {
      const float bv = Bs[k][tx];
#pragma unroll
      for (int a = 0; a < 4; ++a) acc[a] = fmaf(As[k][ty + 8 * a], bv, acc[a]);
    }
  }
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    const int i = i0 + ty + 8 * a, j = j0 + tx;
    if (i < M && j < N) {
      float v = acc[a];
      if (bias) v = wn_act(v + bias[j], act);
      C[(int64_t)i * ldc + j] = v;
    }
  }
}
int wn_launch_sgemm_small(const float* A, int64_t sai, int64_t sak, const float* B, int64_t sbk, int64_t sbj, float* C, int ldc,
                          int M, int N, int K, hipStream_t s) {
  if (M <= 0 || N <= 0) return WN_OK;
  hipLaunchKernelGGL(wn_sgemm_small32_kernel, dim3((N + 31) / 32, (M + 31) / 32), dim3(256), 0, s, A, sai, sak, B, sbk, sbj, C,
                     ldc, M, N, K, (int64_t)0, (int64_t)0, (int64_t)0, (const float*)nullptr, 0, 0);
  WN_HIP_CHECK(hipGetLastError());
  return WN_OK;
}

// nz products in one launch (bases za / zb / zc floats apart), optional Dense epilogue C = act(A B + bias)
int wn_launch_sgemm_small_batched(const float* A, int64_t sai, int64_t sak, int64_t za, const float* B, int64_t sbk, int64_t sbj,
                                  int64_t zb, float* C, int ldc, int64_t zc, int M, int N, int K, int nz, const float* bias,
                                  int act, hipStream_t s, int zk) {
  if (M <= 0 || N <= 0 || nz <= 0) return WN_OK;
  if (nz > 65535) { wn_set_error("sgemm_small_batched: too many products"); return WN_E_UNSUPPORTED; }
  hipLaunchKernelGGL(wn_sgemm_small32_kernel, dim3((N + 31) / 32, (M + 31) / 32, nz), dim3(256), 0, s, A, sai, sak, B, sbk, sbj, C,
                     ldc, M, N, K, za, zb, zc, bias, act, zk);
  WN_HIP_CHECK(hipGetLastError());
  return WN_OK;
}

// gathers every block's W_s into one contiguous [N*D + 1][S] matrix with sum_b b_s as its last row (the blocks' kernels
// are not adjacent in the flat parameter buffer): the A operand of V = W_s(all) W_f0 and of dW_f0 in backward
__global__ void wn_skip_gather_kernel(const float* params, int64_t ws_off0, int64_t ws_stride, const float* bsum, int N, int D,
                                      int S, float* wsall) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < (int64_t)(N * D + 1) * S; i += (int64_t)gridDim.x * blockDim.x) {
    const int k = (int)(i / S), sidx = (int)(i % S);
    wsall[i] = k < N * D ? params[ws_off0 + (int64_t)(k / D) * ws_stride + (int64_t)(k % D) * S + sidx] : bsum[sidx];
  }
}
// b' = b_f0 + (last row of V, = W_f0^T sum_b b_s)
__global__ void wn_vec_add_kernel(const float* a, const float* b, int n, float* out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = a[i] + b[i];
}
int wn_launch_skip_fold(const float* params, int64_t ws_off0, int64_t ws_stride, int64_t wf0_off, int64_t bf0_off,
                        const float* bsum, int N, int D, int S, int F0, float* V, float* bfold, float* wsall, hipStream_t s) {
  const int64_t total = (int64_t)(N * D + 1) * S;
  hipLaunchKernelGGL(wn_skip_gather_kernel, dim3((unsigned)std::min<int64_t>((total + 255) / 256, 2048)), dim3(256), 0, s, params,
                     ws_off0, ws_stride, bsum, N, D, S, wsall);
  WN_HIP_CHECK(hipGetLastError());
  // V ([N*D + 1][F0], the extra row = W_f0^T sum b_s) = wsall W_f0;  W_f0 = kernel (1, S, F0): B[k = s][j = n]
  int rc = wn_launch_sgemm_small(wsall, S, 1, params + wf0_off, F0, 1, V, F0, N * D + 1, F0, S, s);
  if (rc) return rc;
  hipLaunchKernelGGL(wn_vec_add_kernel, dim3((F0 + 255) / 256), dim3(256), 0, s, V + (int64_t)N * D * F0, params + bf0_off, F0, bfold);
  WN_HIP_CHECK(hipGetLastError());
  return WN_OK;
}

// Y = [M; colsum] W_f0^T ([N*D + 1][S], from the rows GEMM): rows b*D.. are dW_s(b), the last row is db_s (the same
// for every block); db_f0 = colsum.  One copy kernel scatters them to the tensors' places in the flat gradient.
__global__ void wn_skip_scatter_kernel(const float* Y, const float* colsum, int64_t ws_off0, int64_t ws_stride, int64_t bs_off0,
                                       int64_t bs_stride, int64_t bf0_off, int N, int D, int S, int F0, float* grads) {
  const int64_t n_ws = (int64_t)N * D * S, n_bs = (int64_t)N * S;
  const int64_t total = n_ws + n_bs + F0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    if (i < n_ws) {
      const int k = (int)(i / S), sidx = (int)(i % S);
      grads[ws_off0 + (int64_t)(k / D) * ws_stride + (int64_t)(k % D) * S + sidx] = Y[i];
    } else if (i < n_ws + n_bs) {
      const int64_t j = i - n_ws;
      grads[bs_off0 + (j / S) * bs_stride + (j % S)] = Y[n_ws + (j % S)];
    } else {
      grads[bf0_off + (i - n_ws - n_bs)] = colsum[i - n_ws - n_bs];
    }
  }
}
int wn_launch_skip_scatter(const float* Y, const float* colsum, int64_t ws_off0, int64_t ws_stride, int64_t bs_off0,
                           int64_t bs_stride, int64_t bf0_off, int N, int D, int S, int F0, float* grads, hipStream_t s) {
  const int64_t total = (int64_t)N * D * S + (int64_t)N * S + F0;
  hipLaunchKernelGGL(wn_skip_scatter_kernel, dim3((unsigned)std::min<int64_t>((total + 255) / 256, 4096)), dim3(256), 0, s, Y, colsum,
                     ws_off0, ws_stride, bs_off0, bs_stride, bf0_off, N, D, S, F0, grads);
  WN_HIP_CHECK(hipGetLastError());
  return WN_OK;
}

__global__ void wn_guard_flag_kernel(const float* absmax, float limit, int enabled, float* out) {
  const float m = absmax ? *absmax : 0.f;
  out[0] = (enabled && !(m < limit)) ? 1.0f : 0.0f;
}
__global__ void wn_guard_accumulate_kernel(const float* src, float* dst) {
  const unsigned a = __float_as_uint(src[0]) & 0x7fffffffu, b = __float_as_uint(dst[0]) & 0x7fffffffu;
  dst[0] = __uint_as_float(a > b ? a : b);
}
int wn_launch_guard_accumulate(const float* src, float* dst, hipStream_t s) {
  hipLaunchKernelGGL(wn_guard_accumulate_kernel, dim3(1), dim3(1), 0, s, src, dst);
  WN_HIP_CHECK(hipGetLastError());
  return WN_OK;
}
int wn_launch_guard_flag(const float* absmax, float limit, int enabled, float* out, hipStream_t s) {
  hipLaunchKernelGGL(wn_guard_flag_kernel, dim3(1), dim3(1), 0, s, absmax, limit, enabled, out);
  WN_HIP_CHECK(hipGetLastError());
  return WN_OK;
}

// Weight gradients of the input causal conv (src/model.py:84-88: C_in = 1, KS taps):
//   dW[tap][c] = sum_{b,t} x[b][t - (KS-1-tap)] * g[b][t][c],   db[c] = sum_{b,t} g[b][t][c]
// i.e. KS + 1 weighted column sums of the gradient at the first block input.  On the generic job table the K = 1
// product ran as a handful of single-wave jobs (0.76 ms at configs[1] for 33 MB of operands); here one workgroup
// per (utterance, time range) streams its rows of g once with 16-byte loads -- lanes = 4-channel groups x row
// lanes -- and leaves its partial sums in the split's slab row (flat-gradient layout), like every other weight
// gradient.  Plain fp32 arithmetic.
template <int KS>
__global__ __launch_bounds__(256) void wn_inconv_wgrad_kernel(const float* x, const float* g, int T, int R, int spb,
                                                              float* slab, int64_t P, int64_t w_off, int64_t b_off) {
  __shared__ float red[256 * (KS + 1) * 4];
  const int split = blockIdx.x, ub = split / spb, sp = split % spb;
  int len = (T + spb - 1) / spb;
  const int r0 = sp * len, r1 = min(T, r0 + len);
  const int ng = R / 4, nrl = 256 / ng;                 // 4-channel groups, row lanes
  const int cg = threadIdx.x % ng, rl = threadIdx.x / ng;
  float acc[KS + 1][4];
#pragma unroll
  for (int i = 0; i <= KS; ++i)
#pragma unroll
    for (int e = 0; e < 4; ++e) acc[i][e] = 0.f;
  const float* xb = x + (int64_t)ub * T;
  const float* gb = g + (int64_t)ub * T * R + 4 * cg;
  for (int t = r0 + rl; t < r1; t += nrl) {
    const f32x4 gv = *reinterpret_cast<const f32x4*>(gb + (int64_t)t * R);
    const float ge[4] = {gv.x, gv.y, gv.z, gv.w};
#pragma unroll
    for (int tap = 0; tap < KS; ++tap) {
      const int ts = t - (KS - 1 - tap);
      const float xv = ts >= 0 ? xb[ts] : 0.f;
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[tap][e] = fmaf(xv, ge[e], acc[tap][e]);
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) acc[KS][e] += ge[e];
  }
#pragma unroll
  for (int i = 0; i <= KS; ++i)
#pragma unroll
    for (int e = 0; e < 4; ++e) red[(i * 4 + e) * 256 + rl * ng + cg] = acc[i][e];
  __syncthreads();
  // (KS + 1) * R outputs, each the sum over the row lanes
  float* row = slab + (int64_t)split * P;
  for (int o = threadIdx.x; o < (KS + 1) * R; o += 256) {
    const int i = o / R, c = o % R;
    float sum = 0.f;
    for (int l = 0; l < nrl; ++l) sum += red[(i * 4 + (c & 3)) * 256 + l * ng + (c >> 2)];
    if (i < KS) row[w_off + (int64_t)i * R + c] = sum;
    else row[b_off + c] = sum;
  }
}

int wn_inconv_wgrad_supported(int R, int KS) { return (R % 4 == 0 && R >= 4 && R <= 1024 && 256 % (R / 4) == 0 && (KS == 2 || KS == 3)) ? 1 : 0; }

int wn_launch_inconv_wgrad(const float* x, const float* g, int B, int T, int R, int KS, int splits_per_b, float* slab,
                           int64_t P, int64_t w_off, int64_t b_off, hipStream_t s) {
  if (!wn_inconv_wgrad_supported(R, KS)) { wn_set_error("inconv_wgrad: unsupported shape R=%d KS=%d", R, KS); return WN_E_UNSUPPORTED; }
  const dim3 grid((unsigned)(B * splits_per_b));
  if (KS == 2) hipLaunchKernelGGL(wn_inconv_wgrad_kernel<2>, grid, dim3(256), 0, s, x, g, T, R, splits_per_b, slab, P, w_off, b_off);
  else hipLaunchKernelGGL(wn_inconv_wgrad_kernel<3>, grid, dim3(256), 0, s, x, g, T, R, splits_per_b, slab, P, w_off, b_off);
  WN_HIP_CHECK(hipGetLastError());
  return WN_OK;
}
