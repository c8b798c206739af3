// probe_tanh.hip -- does a one-transcendental tanh beat the exp2 + rcp form the fused kernels use?
//   A  fast_tanh of csrc/mfma_prims.h: 1 - 2 / (1 + exp2(2 log2(e) x))          v_exp_f32 + v_rcp_f32 + 3 packed-able ops
//   B  odd rational x P(x^2) / Q(x^2), degrees 13 / 6, clamped at |x| = 7.905         v_rcp_f32 + 2 clamps + 1 + 6 + 3 + 2 FMA / mul
//      (the coefficients of the well-known single-precision rational fit; what fp32-level accuracy costs)
//   C  the same rational at degrees 9 / 4 -- fewer FMAs, accuracy NOT at fp32 level: shown for the cycle count only
// One wave per SIMD (the fused kernels' occupancy), 16 independent registers per lane, packed math where the compiler finds it;
// cycles by s_memtime around 4096 repetitions.  Error: max |f(x) - tanh(x)| in double over 2^20 points of [-9, 9].
//   hipcc --offload-arch=gfx950 -O3 -o tools/probe_tanh tools/probe_tanh.hip && tools/probe_tanh
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <vector>

__device__ __forceinline__ float tanh_a(float x) {
  const float d = 1.0f + __builtin_amdgcn_exp2f(x * 2.885390081777927f);
  return fmaf(__builtin_amdgcn_rcpf(d), -2.0f, 1.0f);
}
__device__ __forceinline__ float tanh_b(float x) {
  x = fminf(fmaxf(x, -7.90531110763549805f), 7.90531110763549805f);
  const float x2 = x * x;
  float p = fmaf(x2, -2.76076847742355e-16f, 2.00018790482477e-13f);
  p = fmaf(x2, p, -8.60467152213735e-11f);
  p = fmaf(x2, p, 5.12229709037114e-08f);
  p = fmaf(x2, p, 1.48572235717979e-05f);
  p = fmaf(x2, p, 6.37261928875436e-04f);
  p = fmaf(x2, p, 4.89352455891786e-03f);
  p = x * p;
  float q = fmaf(x2, 1.19825839466702e-06f, 1.18534705686654e-04f);
  q = fmaf(x2, q, 2.26843463243900e-03f);
  q = fmaf(x2, q, 4.89352518554385e-03f);
  return p * __builtin_amdgcn_rcpf(q);
}
__device__ __forceinline__ float tanh_c(float x) {      // Pade [9/8]-like, truncated: cycle count only
  x = fminf(fmaxf(x, -4.97f), 4.97f);
  const float x2 = x * x;
  float p = fmaf(x2, 1.0f, 378.0f);
  p = fmaf(x2, p, 17325.0f);
  p = fmaf(x2, p, 135135.0f);
  p = x * p;
  float q = fmaf(x2, 28.0f, 3150.0f);
  q = fmaf(x2, q, 62370.0f);
  q = fmaf(x2, q, 135135.0f);
  return p * __builtin_amdgcn_rcpf(q);
}

template <int WHICH>
__global__ __launch_bounds__(256, 1) void k_time(float* io, long long* cyc, int reps) {
  float v[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) v[r] = io[(threadIdx.x * 16 + r) % 4096] * 0.5f;
  const long long t0 = __builtin_amdgcn_s_memtime();
  for (int i = 0; i < reps; ++i) {
#pragma unroll
    for (int r = 0; r < 16; ++r) v[r] = (WHICH == 0 ? tanh_a(v[r]) : WHICH == 1 ? tanh_b(v[r]) : tanh_c(v[r])) + 0.25f;
  }
  const long long t1 = __builtin_amdgcn_s_memtime();
  float s = 0.f;
#pragma unroll
  for (int r = 0; r < 16; ++r) s += v[r];
  io[4096 + threadIdx.x] = s;
  if (threadIdx.x == 0) cyc[WHICH] = t1 - t0;
}

template <int WHICH>
__global__ void k_err(const float* x, float* y, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) y[i] = WHICH == 0 ? tanh_a(x[i]) : WHICH == 1 ? tanh_b(x[i]) : tanh_c(x[i]);
}

int main() {
  const int n = 1 << 20, reps = 4096;
  std::vector<float> hx(n), hy(n);
  for (int i = 0; i < n; ++i) hx[i] = -9.0f + 18.0f * (float)i / (float)(n - 1);
  float *dx, *dy, *io;
  long long* cyc;
  hipMalloc(&dx, n * 4); hipMalloc(&dy, n * 4); hipMalloc(&io, 8192 * 4); hipMalloc(&cyc, 64);
  hipMemcpy(dx, hx.data(), n * 4, hipMemcpyHostToDevice);
  hipMemcpy(io, hx.data(), 4096 * 4, hipMemcpyHostToDevice);
  const char* name[3] = {"A exp2 + rcp (product)", "B rational 13/6 + rcp", "C rational 7/6 + rcp (not fp32-accurate)"};
  for (int w = 0; w < 3; ++w) {
    if (w == 0) { k_time<0><<<1, 256>>>(io, cyc, reps); k_err<0><<<n / 256, 256>>>(dx, dy, n); }
    if (w == 1) { k_time<1><<<1, 256>>>(io, cyc, reps); k_err<1><<<n / 256, 256>>>(dx, dy, n); }
    if (w == 2) { k_time<2><<<1, 256>>>(io, cyc, reps); k_err<2><<<n / 256, 256>>>(dx, dy, n); }
    hipDeviceSynchronize();
    long long c[3];
    hipMemcpy(c, cyc, 24, hipMemcpyDeviceToHost);
    hipMemcpy(hy.data(), dy, n * 4, hipMemcpyDeviceToHost);
    double worst = 0.0;
    for (int i = 0; i < n; ++i) { const double e = std::fabs((double)hy[i] - std::tanh((double)hx[i])); if (e > worst) worst = e; }
    printf("%-44s %7.2f cycles per value and lane-row (one wave per SIMD; %lld cycles / %d x 16)   max abs error %.3e\n", name[w],
           (double)c[w] / (reps * 16.0), c[w], reps, worst);
  }
  return 0;
}
