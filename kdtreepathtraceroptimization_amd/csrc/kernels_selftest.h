// kernels_selftest.h -- the kdpt_selftest_* entry points' kernels (device math, RNG, glm, Fresnel, the bounce).
//
// A section of kdpt_runtime.hip's translation unit, not a stand-alone header: kdpt_runtime.hip includes it
// after kernels_rays.h, and the kernels keep that order in the code object.  Device code and launch-argument
// structs only: no HIP host call lives here (tests/test_stream_discipline.py checks that; the guards read host_*.h).
#pragma once

namespace {

__global__ void k_selftest_math(const float* x, int n, float* so, float* co) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) { so[i] = kdpt_sinf(x[i]); co[i] = kdpt_cosf(x[i]); }
}
// glibc acosf / sin / cos restatements (kdpt_math.h): fn 0 acosf(x), 1 sin((double)x), 2 cos((double)x)
__device__ inline uint64_t libm_bits(int fn, float x) {
  if (fn == 0) return f2u(kdpt_acosf(x));
  return d2u(fn == 1 ? kdpt_sin((double)x) : kdpt_cos((double)x));
}
__device__ inline uint64_t splitmix64(uint64_t z) {
  z += 0x9e3779b97f4a7c15ull;
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}
__global__ void k_selftest_libm(int fn, const float* x, int n, double* out) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint64_t b = libm_bits(fn, x[i]);
  out[i] = fn == 0 ? (double)u2f((uint32_t)b) : u2d(b);
}
__global__ void k_selftest_libm_digest(int fn, uint32_t first, uint64_t count, unsigned long long* acc) {
  uint64_t sum = 0;
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k < count; k += stride) {
    const uint32_t xb = (uint32_t)(first + k);
    sum += splitmix64(libm_bits(fn, u2f(xb)) ^ splitmix64(xb));
  }
  atomicAdd(acc, (unsigned long long)sum);
}
__global__ void k_selftest_rng(const int* iid, int n, int k, float* u) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  Rng r = seeded_rng(iid[3 * i], iid[3 * i + 1], iid[3 * i + 2]);
  float v = 0;
  for (int j = 0; j <= k; j++) v = u01(r);
  u[i] = v;
}
__global__ void k_selftest_rng_draws(int mode, const uint32_t* in, int n, int k, float* out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  Rng r = mode == 0 ? seeded_rng((int)in[3 * i], (int)in[3 * i + 1], (int)in[3 * i + 2])
        : mode == 1 ? rng_seed(utilhash(in[i])) : rng_seed(in[i]);
  for (int j = 0; j < k; j++) out[(size_t)i * k + j] = u01(r);
}
__global__ void k_selftest_glm(int fn, const float* in, int n, float* out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  glm_kat(fn, in + (size_t)glm_kat_inputs(fn) * i, out + (size_t)glm_kat_outputs(fn) * i);
}
// scatterRay / shade on one record per lane (kdpt_bounce_kat.h)
__global__ void k_selftest_scatter(const float* in, int n, float* out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  scatter_kat(in + (size_t)SCATTER_KAT_IN * i, out + (size_t)SCATTER_KAT_OUT * i);
}
__global__ void k_selftest_shade(const float* in, int n, float* out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  shade_kat(in + (size_t)SHADE_KAT_IN * i, out + (size_t)SHADE_KAT_OUT * i);
}
__global__ void k_selftest_fresnel(const float* c, int n, float R0, float* f) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  // getFresnelVal with dot(N,-I) == c[i]: F = R0 + (1-R0) * pow(1 - c, 5)
  double F = (double)R0 + (double)(1.0f - R0) * pow5((double)(1.0f - c[i]));
  f[i] = (float)F;
}

}  // namespace
