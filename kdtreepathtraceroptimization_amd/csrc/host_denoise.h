// host_denoise.h -- the variance-guided edge-avoiding filter (kdpt_default_denoise_params, kdpt_denoise_buffers,
// kdpt_denoise, kdpt_denoise_stats).
//
// A host section of kdpt_runtime.hip's translation unit, not a stand-alone header: kdpt_runtime.hip includes it
// after host_moments.h.  Host code only: no kernel is defined here (the kernels_*.h sections hold them), and
// tests/test_stream_discipline.py and tests/test_resource_ownership.py read every host section.
#pragma once

// Denoising (include/kdpt.h "Denoising"; kernels: k_denoise_rays, k_cast_prep, k_trace, k_cast_resolve,
// k_denoise_pack[_render], k_denoise_pass, k_denoise_unpack).  kdpt_denoise is a composition of what the context
// already computes -- the per-pixel mean and the variance of that mean from the image and the second moments, the
// first-hit records of the camera's pinhole rays from the ray query's kernels -- and the filter kdpt_denoise_buffers
// runs on caller data; all of it on the context's stream, in buffers of its own (Denoiser).
namespace {

// Steps up to this one take k_denoise_pass's LDS-tiled route, larger ones gather from memory.  Measured per pass at
// 800 x 800: tiled 0.054 / 0.078 ms against 0.094 / 0.095 gathered at steps 1 / 2; from step 4
// on the strided staging loses, 0.124 / 0.185 / 0.181 ms tiled against 0.093 / 0.092 / 0.089 gathered.
constexpr int DN_TILED_MAX_STEP = 2;

int check_denoise_params(const kdpt_denoise_params* p, const std::string& who) {
  if (p->passes < 0 || p->passes > 8) return fail(KDPT_ERR_ARG, who + ": params.passes must be in 0 .. 8");
  if (p->normal_power_log2 < 0 || p->normal_power_log2 > 10)
    return fail(KDPT_ERR_ARG, who + ": params.normal_power_log2 must be in 0 .. 10");
  if (!(std::isfinite(p->sigma_l) && p->sigma_l > 0.0f))
    return fail(KDPT_ERR_ARG, who + ": params.sigma_l must be finite and > 0");
  if (!(std::isfinite(p->sigma_z) && p->sigma_z > 0.0f))
    return fail(KDPT_ERR_ARG, who + ": params.sigma_z must be finite and > 0");
  if (!(std::isfinite(p->eps_l) && p->eps_l > 0.0f))
    return fail(KDPT_ERR_ARG, who + ": params.eps_l must be finite and > 0");
  return KDPT_OK;
}

// The passes on stream st: pass 0 reads `in` (which no pass writes unless it is cv[0]), pass k > 0 cv[k & 1]; pass
// k writes cv[~k & 1]; *last: the buffer the result is in.
int launch_denoise_passes(const kdpt_denoise_params& p, int W, int H, const float4* g0, const float4* g1,
                          const float4* in, float4* const cv[2], hipStream_t st, const float4** last) {
  for (int k = 0; k < p.passes; k++) {
    const int s = 1 << k;
    DenoisePass a{g0, g1, k == 0 ? in : cv[k & 1], cv[(k & 1) ^ 1], W, H, s, std::min(s, W), std::min(s, H),
                  p.normal_power_log2, p.sigma_l, p.sigma_z, p.eps_l};
    if (s <= DN_TILED_MAX_STEP) {  // a 32 x 8 tile of each lattice of pixels congruent mod s
      const int lw = (W + s - 1) / s, lh = (H + s - 1) / s;
      const dim3 grid(((lw + DN_TILE_W - 1) / DN_TILE_W) * a.nrx, ((lh + DN_TILE_H - 1) / DN_TILE_H) * a.nry);
      hipLaunchKernelGGL(k_denoise_pass<true>, grid, dim3(DN_TILE_W * DN_TILE_H), 0, st, a);
    } else {
      const dim3 grid((W + DN_TILE_W - 1) / DN_TILE_W, (H + DN_TILE_H - 1) / DN_TILE_H);
      hipLaunchKernelGGL(k_denoise_pass<false>, grid, dim3(DN_TILE_W * DN_TILE_H), 0, st, a);
    }
    HIP_TRY(hipGetLastError());
  }
  *last = p.passes == 0 ? in : cv[p.passes & 1];
  return KDPT_OK;
}
int launch_denoise_passes(const kdpt_denoise_params& p, int W, int H, const float4* g0, const float4* g1,
                          float4* const cv[2], hipStream_t st, const float4** last) {
  return launch_denoise_passes(p, W, H, g0, g1, cv[0], cv, st, last);
}

// The context's denoising buffers, made on first use (nothing is queued on them: every call that uses them ends
// with a synchronisation).
int denoise_buffers(kdpt_ctx* c) {
  Denoiser::Buffers& b = c->den.b;
  if (b.npix == c->npix) return KDPT_OK;
  b = {};
  const size_t m = (size_t)c->npix;
  if (b.g0.alloc(m) != hipSuccess || b.g1.alloc(m) != hipSuccess || b.cv[0].alloc(m) != hipSuccess ||
      b.cv[1].alloc(m) != hipSuccess || b.rays.alloc(6 * m) != hipSuccess || b.hits_out.alloc(m) != hipSuccess ||
      b.cray.alloc(2 * m) != hipSuccess || b.cand.alloc(m) != hipSuccess || b.hits.alloc(m) != hipSuccess ||
      b.cnt.alloc(2) != hipSuccess || b.tt.alloc(3) != hipSuccess || b.out_stage.alloc(4 * m) != hipSuccess) {
    (void)hipGetLastError();
    b = {};
    return fail(KDPT_ERR_HIP, "kdpt_denoise: cannot allocate the buffers of " + std::to_string(m) + " pixels");
  }
  for (Event& e : c->den.ev)
    if (!e) HIP_TRY(e.create());
  b.npix = c->npix;
  return KDPT_OK;
}

// The guides on the context's stream: the camera's pinhole rays through kdpt_cast_rays' kernels, one chunk of W*H
// rays, flags = 0; the hit records land in den.b.hits_out.
int launch_denoise_guides(kdpt_ctx* c) {
  const hipStream_t st = c->stream;
  const Denoiser::Buffers& b = c->den.b;
  const int npix = c->npix;
  const size_t m = (size_t)npix;
  const dim3 lin((npix + 255) / 256);
  HIP_TRY(hipMemsetAsync(b.cnt.get(), 0, sizeof(int) * 2, st));
  HIP_TRY(hipMemsetAsync(b.tt.get(), 0, sizeof(unsigned long long) * 3, st));
  hipLaunchKernelGGL(k_denoise_rays, lin, dim3(256), 0, st, c->cam, b.rays.get(), b.rays.get() + 3 * m);
  HIP_TRY(hipGetLastError());
  CastArgs a;
  a.S = c->S;
  a.o = b.rays.get();
  a.d = b.rays.get() + 3 * m;
  a.n = npix;
  a.normalize = 0;
  a.cray = b.cray.get();
  a.hits = b.hits.get();
  a.cand = b.cand.get();
  a.cnt = b.cnt.get();
  a.tt = b.tt.get();
  a.out = b.hits_out.get();
  const TraceArgs t{c->S, a.cand, a.cray, a.cnt + 1, a.hits, nullptr, 0, a.cnt, 0, c->counters, a.tt};
  hipLaunchKernelGGL(k_cast_prep, dim3((npix + GEN_BLOCK - 1) / GEN_BLOCK), dim3(GEN_BLOCK), 0, st, a);
  HIP_TRY(hipGetLastError());
  launch_trace(c, t, false, c->trace_grid, st);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(hybrid_shading(c) ? k_cast_resolve<true> : k_cast_resolve<false>, lin, dim3(256), 0, st, a);
  HIP_TRY(hipGetLastError());
  return KDPT_OK;
}

}  // namespace

void kdpt_default_denoise_params(kdpt_denoise_params* p) {
  if (!p) return;
  p->passes = 5;
  p->normal_power_log2 = 7;
  p->sigma_l = 4.0f;
  p->sigma_z = 0.02f;
  p->eps_l = 1e-8f;
  p->pad_ = 0.0f;
}

int kdpt_denoise_buffers(int device, int w, int h, const float* color, const float* variance, const float* normal,
                         const float* point, const float* depth, const int* id, const kdpt_denoise_params* p,
                         float* out_color, float* out_variance) {
  const std::string who = "kdpt_denoise_buffers";
  if (w < 1) return fail(KDPT_ERR_ARG, who + ": w must be >= 1");
  if (h < 1) return fail(KDPT_ERR_ARG, who + ": h must be >= 1");
  if ((long long)w * h > (1ll << 26)) return fail(KDPT_ERR_ARG, who + ": w * h must be <= 2^26");
  if (!color) return fail(KDPT_ERR_ARG, who + ": null color");
  if (!variance) return fail(KDPT_ERR_ARG, who + ": null variance");
  if (!normal) return fail(KDPT_ERR_ARG, who + ": null normal");
  if (!point) return fail(KDPT_ERR_ARG, who + ": null point");
  if (!depth) return fail(KDPT_ERR_ARG, who + ": null depth");
  if (!id) return fail(KDPT_ERR_ARG, who + ": null id");
  if (!p) return fail(KDPT_ERR_ARG, who + ": null params");
  if (!out_color) return fail(KDPT_ERR_ARG, who + ": null out_color");
  if (device < 0) return fail(KDPT_ERR_ARG, who + ": device must be >= 0");
  int rc = check_denoise_params(p, who);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(device));
  const int npix = w * h;
  const size_t m = (size_t)npix;
  Stream st;  // (declared before the buffers: destroyed after them)
  HIP_TRY(st.create());
  DeviceBuf<float> in, out;  // colour, normal, point (3 m each), variance, depth (m each); colour, variance
  DeviceBuf<int> ids;
  DeviceBuf<float4> g0, g1, cv0, cv1;
  HIP_TRY(in.alloc(11 * m));
  HIP_TRY(out.alloc(4 * m));
  HIP_TRY(ids.alloc(m));
  HIP_TRY(g0.alloc(m));
  HIP_TRY(g1.alloc(m));
  HIP_TRY(cv0.alloc(m));
  HIP_TRY(cv1.alloc(m));
  float* const d = in.get();
  const DenoiseArrays arr{d, d + 9 * m, d + 3 * m, d + 6 * m, d + 10 * m, ids.get()};
  HIP_TRY(hipMemcpyAsync(d, color, sizeof(float) * 3 * m, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(d + 3 * m, normal, sizeof(float) * 3 * m, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(d + 6 * m, point, sizeof(float) * 3 * m, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(d + 9 * m, variance, sizeof(float) * m, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(d + 10 * m, depth, sizeof(float) * m, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(ids.get(), id, sizeof(int) * m, hipMemcpyHostToDevice, st));
  const dim3 lin((npix + 255) / 256);
  hipLaunchKernelGGL(k_denoise_pack, lin, dim3(256), 0, st, arr, npix, g0.get(), g1.get(), cv0.get());
  HIP_TRY(hipGetLastError());
  float4* const cv[2] = {cv0.get(), cv1.get()};
  const float4* last = nullptr;
  if ((rc = launch_denoise_passes(*p, w, h, g0.get(), g1.get(), cv, st, &last))) return rc;
  hipLaunchKernelGGL(k_denoise_unpack, lin, dim3(256), 0, st, last, npix, out.get(),
                     out_variance ? out.get() + 3 * m : nullptr);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(out_color, out.get(), sizeof(float) * 3 * m, hipMemcpyDeviceToHost, st));
  if (out_variance)
    HIP_TRY(hipMemcpyAsync(out_variance, out.get() + 3 * m, sizeof(float) * m, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  return KDPT_OK;
}

int kdpt_denoise(kdpt_ctx* c, const kdpt_denoise_params* p, float* out_color, float* out_variance) {
  const std::string who = "kdpt_denoise";
  if (!c) return fail(KDPT_ERR_ARG, who + ": null ctx");
  if (!p) return fail(KDPT_ERR_ARG, who + ": null params");
  if (!out_color) return fail(KDPT_ERR_ARG, who + ": null out_color");
  int rc = check_denoise_params(p, who);
  if (rc) return rc;
  if (!c->mom.on) return fail(KDPT_ERR_UNSUPPORTED, who + ": moments are off (kdpt_set_moments)");
  if (c->mom.samples < 2)
    return fail(KDPT_ERR_ARG, who + ": " + std::to_string(c->mom.samples) +
                                  " iteration(s) accumulated, a variance needs at least 2");
  if (c->brute || c->viz)
    return fail(KDPT_ERR_UNSUPPORTED, who + ": the context runs the brute-force or box-view intersect kernel "
                                            "(enable_kd = 0 / viz_kd = 1); the guides need kdpt_cast_rays' KD "
                                            "traversal");
  if ((rc = kdpt_synchronize(c))) return rc;  // everything queued on the context first, the pipelined adds included
  if ((rc = join_accum(c)) || (rc = denoise_buffers(c))) return rc;
  const hipStream_t st = c->stream;
  const Denoiser::Buffers& b = c->den.b;
  const int npix = c->npix;
  const size_t m = (size_t)npix;
  const dim3 lin((npix + 255) / 256);
  // ---- the guides: the pinhole rays through kdpt_cast_rays' kernels, one chunk of W*H rays, flags = 0 ----
  HIP_TRY(hipEventRecord(c->den.ev[0], st));
  if ((rc = launch_denoise_guides(c))) return rc;
  HIP_TRY(hipEventRecord(c->den.ev[1], st));
  // ---- the filter ----
  hipLaunchKernelGGL(k_denoise_pack_render, lin, dim3(256), 0, st, (const float*)c->image,
                     (const float*)c->mom.sumsq.get(), (const uint32_t*)c->mom.adapt.extra.get(), c->mom.samples,
                     (const kdpt_ray_hit*)b.hits_out.get(), npix, b.g0.get(), b.g1.get(), b.cv[0].get());
  HIP_TRY(hipGetLastError());
  float4* const cv[2] = {b.cv[0].get(), b.cv[1].get()};
  const float4* last = nullptr;
  if ((rc = launch_denoise_passes(*p, c->W, c->H, b.g0.get(), b.g1.get(), cv, st, &last))) return rc;
  const bool col_dev = on_context_device(c, out_color), var_dev = out_variance && on_context_device(c, out_variance);
  float* const d_col = col_dev ? out_color : b.out_stage.get();
  float* const d_var = !out_variance ? nullptr : (var_dev ? out_variance : b.out_stage.get() + 3 * m);
  hipLaunchKernelGGL(k_denoise_unpack, lin, dim3(256), 0, st, last, npix, d_col, d_var);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(c->den.ev[2], st));
  if ((rc = stage_out(col_dev, out_color, (const float*)d_col, 3 * m, st))) return rc;
  if (out_variance && (rc = stage_out(var_dev, out_variance, (const float*)d_var, m, st))) return rc;
  HIP_TRY(hipStreamSynchronize(st));
  float g_ms = 0, f_ms = 0;
  HIP_TRY(hipEventElapsedTime(&g_ms, c->den.ev[0], c->den.ev[1]));
  HIP_TRY(hipEventElapsedTime(&f_ms, c->den.ev[1], c->den.ev[2]));
  c->den.guide_ms = g_ms;
  c->den.filter_ms = f_ms;
  return check_fault(&c->solo, c->stream);
}

int kdpt_denoise_stats(kdpt_ctx* c, double* guide_ms, double* filter_ms) {
  if (!c) return fail(KDPT_ERR_ARG, "kdpt_denoise_stats: null ctx");
  if (guide_ms) *guide_ms = c->den.guide_ms;
  if (filter_ms) *filter_ms = c->den.filter_ms;
  return KDPT_OK;
}
