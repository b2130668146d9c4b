// host_selftest.h -- the kdpt_selftest_* entry points: device math, RNG, glm, Fresnel, the bounce, the active list.
//
// A host section of kdpt_runtime.hip's translation unit, not a stand-alone header: kdpt_runtime.hip includes it
// after host_moments.h.  Host code only: no kernel is defined here (the kernels_*.h sections hold them), and
// tests/test_stream_discipline.py and tests/test_resource_ownership.py read every host section.
#pragma once


extern "C" {

int kdpt_selftest_math(const float* x, int n, float* so, float* co) {
  DeviceBuf<float> dx, ds, dc;
  HIP_TRY(dx.alloc(n));
  HIP_TRY(ds.alloc(n));
  HIP_TRY(dc.alloc(n));
  HIP_TRY(hipMemcpy(dx.get(), x, sizeof(float) * n, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(k_selftest_math, dim3((n + 255) / 256), dim3(256), 0, 0, dx.get(), n, ds.get(), dc.get());
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpy(so, ds.get(), sizeof(float) * n, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(co, dc.get(), sizeof(float) * n, hipMemcpyDeviceToHost));
  return KDPT_OK;
}

int kdpt_selftest_libm(int fn, const float* x, int n, double* out) {
  if (fn < 0 || fn > 2 || n < 0 || (n && (!x || !out))) return fail(KDPT_ERR_ARG, "kdpt_selftest_libm: bad arguments");
  if (n == 0) return KDPT_OK;
  DeviceBuf<float> dx;
  DeviceBuf<double> dout;
  HIP_TRY(dx.alloc(n));
  HIP_TRY(dout.alloc(n));
  HIP_TRY(hipMemcpy(dx.get(), x, sizeof(float) * n, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(k_selftest_libm, dim3((n + 255) / 256), dim3(256), 0, 0, fn, dx.get(), n, dout.get());
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpy(out, dout.get(), sizeof(double) * n, hipMemcpyDeviceToHost));
  return KDPT_OK;
}

int kdpt_selftest_libm_digest(int fn, uint32_t first, unsigned long long count, unsigned long long* digest) {
  if (fn < 0 || fn > 2 || !digest || count > (1ull << 32) || first + count > (1ull << 32))
    return fail(KDPT_ERR_ARG, "kdpt_selftest_libm_digest: bad arguments");
  DeviceBuf<unsigned long long> dacc;
  HIP_TRY(dacc.alloc(1));
  HIP_TRY(hipMemset(dacc.get(), 0, sizeof(unsigned long long)));
  hipLaunchKernelGGL(k_selftest_libm_digest, dim3(4096), dim3(256), 0, 0, fn, first, (uint64_t)count, dacc.get());
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpy(digest, dacc.get(), sizeof(unsigned long long), hipMemcpyDeviceToHost));
  return KDPT_OK;
}

int kdpt_selftest_rng(const int* iid, int n, int k, float* u) {
  DeviceBuf<int> di;
  DeviceBuf<float> du;
  HIP_TRY(di.alloc(3 * (size_t)n));
  HIP_TRY(du.alloc(n));
  HIP_TRY(hipMemcpy(di.get(), iid, sizeof(int) * 3 * n, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(k_selftest_rng, dim3((n + 255) / 256), dim3(256), 0, 0, di.get(), n, k, du.get());
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpy(u, du.get(), sizeof(float) * n, hipMemcpyDeviceToHost));
  return KDPT_OK;
}

int kdpt_selftest_rng_draws(int mode, const uint32_t* in, int n, int k, float* out) {
  if (mode < 0 || mode > 2 || n < 0 || k < 0 || (n && k && (!in || !out)))
    return fail(KDPT_ERR_ARG, "bad rng selftest arguments");
  if (!n || !k) return KDPT_OK;
  const size_t nin = (size_t)n * (mode == 0 ? 3 : 1), nout = (size_t)n * k;
  DeviceBuf<uint32_t> di;
  DeviceBuf<float> dout;
  HIP_TRY(di.alloc(nin));
  HIP_TRY(dout.alloc(nout));
  HIP_TRY(hipMemcpy(di.get(), in, sizeof(uint32_t) * nin, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(k_selftest_rng_draws, dim3((n + 255) / 256), dim3(256), 0, 0, mode, di.get(), n, k, dout.get());
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpy(out, dout.get(), sizeof(float) * nout, hipMemcpyDeviceToHost));
  return KDPT_OK;
}

int kdpt_selftest_glm(int fn, const float* in, int n, float* out) {
  const int ni = glm_kat_inputs(fn), no = glm_kat_outputs(fn);
  if (!ni || n < 0 || (n && (!in || !out))) return fail(KDPT_ERR_ARG, "bad glm selftest arguments");
  if (!n) return KDPT_OK;
  DeviceBuf<float> din, dout;
  HIP_TRY(din.alloc(ni * (size_t)n));
  HIP_TRY(dout.alloc(no * (size_t)n));
  HIP_TRY(hipMemcpy(din.get(), in, sizeof(float) * ni * (size_t)n, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(dout.get(), out, sizeof(float) * no * (size_t)n, hipMemcpyHostToDevice));  // sentinels
  hipLaunchKernelGGL(k_selftest_glm, dim3((n + 255) / 256), dim3(256), 0, 0, fn, din.get(), n, dout.get());
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpy(out, dout.get(), sizeof(float) * no * (size_t)n, hipMemcpyDeviceToHost));
  return KDPT_OK;
}

namespace {
// one record of `ni` words in, `no` words out per lane
int kdpt_selftest_records(void (*kernel)(const float*, int, float*), const char* what, int ni, int no, const float* in,
                     int n, float* out) {
  if (n < 0 || (n && (!in || !out))) return fail(KDPT_ERR_ARG, what);
  if (!n) return KDPT_OK;
  DeviceBuf<float> din, dout;
  HIP_TRY(din.alloc(ni * (size_t)n));
  HIP_TRY(dout.alloc(no * (size_t)n));
  HIP_TRY(hipMemcpy(din.get(), in, sizeof(float) * ni * (size_t)n, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(kernel, dim3((n + 255) / 256), dim3(256), 0, 0, din.get(), n, dout.get());
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpy(out, dout.get(), sizeof(float) * no * (size_t)n, hipMemcpyDeviceToHost));
  return KDPT_OK;
}
}  // namespace

int kdpt_selftest_scatter(const float* in, int n, float* out) {
  return kdpt_selftest_records(k_selftest_scatter, "bad scatter selftest arguments", SCATTER_KAT_IN, SCATTER_KAT_OUT, in,
                          n, out);
}

int kdpt_selftest_shade(const float* in, int n, float* out) {
  return kdpt_selftest_records(k_selftest_shade, "bad shade selftest arguments", SHADE_KAT_IN, SHADE_KAT_OUT, in, n, out);
}

int kdpt_selftest_fresnel(const float* cs, int n, float ior, float* f) {
  DeviceBuf<float> dc, df;
  HIP_TRY(dc.alloc(n));
  HIP_TRY(df.alloc(n));
  HIP_TRY(hipMemcpy(dc.get(), cs, sizeof(float) * n, hipMemcpyHostToDevice));
  float rr = (1.0f - ior) / (1.0f + ior);
  hipLaunchKernelGGL(k_selftest_fresnel, dim3((n + 255) / 256), dim3(256), 0, 0, dc.get(), n, rr * rr, df.get());
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpy(f, df.get(), sizeof(float) * n, hipMemcpyDeviceToHost));
  return KDPT_OK;
}

}  // extern "C"

int kdpt_selftest_active_list(const float* noise, int npix, float threshold, int* pixels, int* n) {
  if (npix < 0 || !n || (npix && (!noise || !pixels)) || std::isnan(threshold))
    return fail(KDPT_ERR_ARG, "kdpt_selftest_active_list: bad arguments");
  *n = 0;
  if (!npix) return KDPT_OK;
  const size_t nblk = (size_t)adapt_blocks(npix);
  DeviceBuf<float> values;
  DeviceBuf<unsigned long long> masks;
  DeviceBuf<int> blocks, list;
  HIP_TRY(values.alloc((size_t)npix));
  HIP_TRY(masks.alloc(nblk * (ADAPT_BLOCK / 64)));
  HIP_TRY(blocks.alloc(2 * nblk + 1));
  HIP_TRY(list.alloc((size_t)npix));
  HIP_TRY(hipMemcpy(values.get(), noise, sizeof(float) * (size_t)npix, hipMemcpyHostToDevice));
  launch_active_list(nullptr, nullptr, nullptr, values.get(), npix, 0, 1.0f, threshold, masks.get(), blocks.get(),
                     list.get(), 0);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpy(n, blocks.get() + 2 * nblk, sizeof(int), hipMemcpyDeviceToHost));
  if (*n < 0 || *n > npix) return fail(KDPT_ERR_HIP, "kdpt_selftest_active_list: count out of range");
  if (*n) HIP_TRY(hipMemcpy(pixels, list.get(), sizeof(int) * (size_t)*n, hipMemcpyDeviceToHost));
  return KDPT_OK;
}
