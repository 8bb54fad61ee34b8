// Forms of the per-replica clip (wn_clip_gradients) timed on the tensor table of BASELINE configs[1]
// (188 tensors, 1 251 264 floats, the largest 65 536):
//   one launch   wn_clip_kernel as shipped: one workgroup per tensor reduces and rescales its own tensor
//   two launches wn_sumsq_kernel (one workgroup per tensor), then a rescale spread over 32 workgroups per tensor
// Every tensor gets norm 5 before every call, so each call rescales everything (the case of a real step: 186 of 188).
// The kernels come from wn_optim.hip, whose entry points need the plan: link against the built library.
//   hipcc -O3 -std=c++17 --offload-arch=gfx950 -ffp-contract=on tools/clip_probe.hip -o tools/clip_probe \
//         -Lwavenets_amd -lwn_hip -Wl,-rpath,$PWD/wavenets_amd
#include "../wavenets_amd/csrc/wn_optim.hip"
#include <cstdio>
#include <vector>

__global__ void probe_scale_kernel(float* g, const WnTensorDesc* table, const float* norms2, float clipnorm) {
  const WnTensorDesc d = table[blockIdx.y];
  const float scale = clipnorm / fmaxf(sqrtf(norms2[blockIdx.y]), clipnorm);
  if (scale == 1.0f) return;
  float* p = g + d.off;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < d.len; i += (int64_t)gridDim.x * blockDim.x)
    p[i] *= scale;
}

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)

int main() {
  std::vector<WnTensorDesc> t;
  int64_t off = 0;
  auto add = [&](int64_t len) { t.push_back({off, len}); off += len; };
  // the exact size multiset of configs[1]: 60 x 16384, 30 x 4096, 32 x 128, 32 x 256, 31 x 64, 2 x 32768, 1 x 65536
  add(128); add(64);
  for (int b = 0; b < 30; ++b) { add(16384); add(128); add(4096); add(64); add(16384); add(256); }
  add(32768); add(128); add(32768); add(256); add(65536); add(256);
  const int n = (int)t.size();
  const int64_t total = off;
  printf("%d tensors, %lld floats\n", n, (long long)total);
  std::vector<float> h(total);
  for (const auto& d : t) {
    const float v = 5.0f / sqrtf((float)d.len);
    for (int64_t i = 0; i < d.len; ++i) h[d.off + i] = (i & 1) ? v : -v;
  }
  float *g, *src, *norms;
  WnTensorDesc* dt;
  CK(hipMalloc(&g, total * 4)); CK(hipMalloc(&src, total * 4)); CK(hipMalloc(&norms, n * 4));
  CK(hipMalloc(&dt, n * sizeof(WnTensorDesc)));
  CK(hipMemcpy(src, h.data(), total * 4, hipMemcpyHostToDevice));
  CK(hipMemcpy(dt, t.data(), n * sizeof(WnTensorDesc), hipMemcpyHostToDevice));
  hipStream_t s;
  CK(hipStreamCreate(&s));
  hipEvent_t e0, e1;
  CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
  const int reps = 200;
  for (int round = 0; round < 3; ++round) {
    for (int form = 0; form < 3; ++form) {        // 0: the refill copy alone (subtracted), 1: one launch, 2: two launches
      float ms = 0.f;
      for (int it = -20; it < reps; ++it) {
        if (it == 0) CK(hipEventRecord(e0, s));
        CK(hipMemcpyAsync(g, src, total * 4, hipMemcpyDeviceToDevice, s));
        if (form == 1) {
          if (wn_launch_clip(g, dt, n, 1.0f, norms, s)) return 1;
        } else if (form == 2) {
          if (wn_launch_sumsq(g, dt, n, norms, s)) return 1;
          hipLaunchKernelGGL(probe_scale_kernel, dim3(32, n), dim3(256), 0, s, g, dt, norms, 1.0f);
        }
      }
      CK(hipEventRecord(e1, s));
      CK(hipStreamSynchronize(s));
      CK(hipEventElapsedTime(&ms, e0, e1));
      printf("round %d  %s: %.2f us per call\n", round, form == 0 ? "refill copy alone  " : form == 1 ? "copy + one launch  " : "copy + two launches", ms * 1e3 / reps);
    }
  }
  std::vector<float> out(total), nn(n);
  CK(hipMemcpy(out.data(), g, total * 4, hipMemcpyDeviceToHost));
  CK(hipMemcpy(nn.data(), norms, n * 4, hipMemcpyDeviceToHost));
  double worst = 0.0;
  for (const auto& d : t) {
    double s2 = 0.0;
    for (int64_t i = 0; i < d.len; ++i) s2 += (double)out[d.off + i] * out[d.off + i];
    worst = fmax(worst, fabs(sqrt(s2) - 1.0));
  }
  printf("norms after the last call: max |norm - 1| = %.2e; norms2[0] = %.4f (25 expected)\n", worst, nn[0]);
  return 0;
}
