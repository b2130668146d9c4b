// host_temporal.h -- temporal accumulation for the denoiser (kdpt_default_temporal_params, kdpt_temporal_buffers,
// kdpt_denoise_temporal, kdpt_temporal_reset, kdpt_temporal_stats).
//
// A host section of kdpt_runtime.hip's translation unit, not a stand-alone header: kdpt_runtime.hip includes it
// after host_denoise.h, whose guide pass, packing and filter passes it composes.  Host code only: no kernel is
// defined here (kernels_temporal.h holds them), and tests/test_stream_discipline.py and
// tests/test_resource_ownership.py read every host section.
#pragma once

// Temporal accumulation (include/kdpt.h "Temporal accumulation"; kernels: k_temporal, k_temporal_pack_history and
// kdpt_denoise's).  kdpt_denoise_temporal is kdpt_denoise with one stage between packing and the filter: the frame's
// colour and variance are blended with the previous call's, found by projecting each pixel's hit point through the
// previous camera.  The history is two sets of records in the context (Temporal): the frame is built in the set
// that is not the history, and becomes the history by a swap of the two roles.
namespace {

int check_temporal_params(const kdpt_temporal_params* p, const std::string& who) {
  if (!(std::isfinite(p->alpha) && p->alpha > 0.0f && p->alpha <= 1.0f))
    return fail(KDPT_ERR_ARG, who + ": params.alpha must be in (0, 1]");
  if (!(std::isfinite(p->sigma_z) && p->sigma_z > 0.0f))
    return fail(KDPT_ERR_ARG, who + ": params.sigma_z must be finite and > 0");
  if (!(std::isfinite(p->normal_min) && p->normal_min >= -1.0f && p->normal_min <= 1.0f))
    return fail(KDPT_ERR_ARG, who + ": params.normal_min must be in [-1, 1]");
  if (p->max_history < 1 || p->max_history > 4096)
    return fail(KDPT_ERR_ARG, who + ": params.max_history must be in 1 .. 4096");
  return KDPT_OK;
}

// k_temporal on stream st.  hist null: no history.
struct TemporalFrame {
  const float4 *g0, *g1, *cv;
  const float* len;
};
int launch_temporal(const kdpt_temporal_params& p, int W, int H, const TemporalFrame& cur, const TemporalFrame* hist,
                    const kdpt_camera& hcam, float4* out_cv, float* out_len, unsigned int* counts, hipStream_t st) {
  TemporalArgs a{};
  a.g0 = cur.g0;
  a.g1 = cur.g1;
  a.cv = cur.cv;
  if (hist) {
    a.h0 = hist->g0;
    a.h1 = hist->g1;
    a.hcv = hist->cv;
    a.hlen = hist->len;
    a.cam = hcam;
  }
  a.out_cv = out_cv;
  a.out_len = out_len;
  a.counts = counts;
  a.W = W;
  a.H = H;
  a.alpha = p.alpha;
  a.sigma_z = p.sigma_z;
  a.normal_min = p.normal_min;
  a.max_history = (float)p.max_history;
  const long long npix = (long long)W * H;
  hipLaunchKernelGGL(k_temporal, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, st, a);
  HIP_TRY(hipGetLastError());
  return KDPT_OK;
}

// The context's two sets, made on first use (nothing is queued on them: every call that uses them ends with a
// synchronisation).  A remake drops the history.
int temporal_sets(kdpt_ctx* c) {
  Temporal::Sets& s = c->tmp.s;
  if (s.npix == c->npix) return KDPT_OK;
  s = {};
  const size_t m = (size_t)c->npix;
  bool ok = s.counts.alloc(2) == hipSuccess;
  for (Temporal::Set& t : s.set)
    ok = ok && t.g0.alloc(m) == hipSuccess && t.g1.alloc(m) == hipSuccess && t.cv.alloc(m) == hipSuccess &&
         t.len.alloc(m) == hipSuccess;
  if (!ok) {
    (void)hipGetLastError();
    s = {};
    return fail(KDPT_ERR_HIP, "kdpt_denoise_temporal: cannot allocate the history of " + std::to_string(m) + " pixels");
  }
  for (Event& e : c->tmp.ev)
    if (!e) HIP_TRY(e.create());
  s.npix = c->npix;
  return KDPT_OK;
}

}  // namespace

void kdpt_default_temporal_params(kdpt_temporal_params* p) {
  if (!p) return;
  p->alpha = 0.2f;
  p->sigma_z = 0.02f;
  p->normal_min = 0.9f;
  p->max_history = 32;
  p->pad_[0] = p->pad_[1] = 0.0f;
}

int kdpt_temporal_buffers(int device, int w, int h, const float* color, const float* variance, const float* normal,
                          const float* point, const float* depth, const int* id, const float* h_color,
                          const float* h_variance, const float* h_normal, const float* h_point, const float* h_depth,
                          const int* h_id, const float* h_length, const kdpt_camera* h_camera,
                          const kdpt_temporal_params* p, float* out_color, float* out_variance, float* out_length) {
  const std::string who = "kdpt_temporal_buffers";
  if (w < 1) return fail(KDPT_ERR_ARG, who + ": w must be >= 1");
  if (h < 1) return fail(KDPT_ERR_ARG, who + ": h must be >= 1");
  if ((long long)w * h > (1ll << 26)) return fail(KDPT_ERR_ARG, who + ": w * h must be <= 2^26");
  if (!color) return fail(KDPT_ERR_ARG, who + ": null color");
  if (!variance) return fail(KDPT_ERR_ARG, who + ": null variance");
  if (!normal) return fail(KDPT_ERR_ARG, who + ": null normal");
  if (!point) return fail(KDPT_ERR_ARG, who + ": null point");
  if (!depth) return fail(KDPT_ERR_ARG, who + ": null depth");
  if (!id) return fail(KDPT_ERR_ARG, who + ": null id");
  const void* const hist[8] = {h_color, h_variance, h_normal, h_point, h_depth, h_id, h_length, h_camera};
  static const char* const hist_name[8] = {"h_color", "h_variance", "h_normal", "h_point",
                                           "h_depth", "h_id",       "h_length", "h_camera"};
  int given = 0;
  for (const void* q : hist) given += q != nullptr;
  if (given != 0 && given != 8)
    for (int i = 0; i < 8; i++)
      if (!hist[i])
        return fail(KDPT_ERR_ARG, who + ": partial history: null " + hist_name[i] + " beside a non-null history "
                                        "argument (give all eight, or none)");
  if (!p) return fail(KDPT_ERR_ARG, who + ": null params");
  if (!out_color) return fail(KDPT_ERR_ARG, who + ": null out_color");
  if (!out_variance) return fail(KDPT_ERR_ARG, who + ": null out_variance");
  if (!out_length) return fail(KDPT_ERR_ARG, who + ": null out_length");
  if (device < 0) return fail(KDPT_ERR_ARG, who + ": device must be >= 0");
  int rc = check_temporal_params(p, who);
  if (rc) return rc;
  if (given && (h_camera->resolution[0] != w || h_camera->resolution[1] != h))
    return fail(KDPT_ERR_ARG, who + ": h_camera.resolution is " + std::to_string(h_camera->resolution[0]) + " x " +
                                  std::to_string(h_camera->resolution[1]) + ", the buffers are " +
                                  std::to_string(w) + " x " + std::to_string(h));
  HIP_TRY(hipSetDevice(device));
  const int npix = w * h;
  const size_t m = (size_t)npix;
  Stream st;  // (declared before the buffers: destroyed after them)
  HIP_TRY(st.create());
  // per frame: colour, normal, point (3 m each), variance, depth (m each), then for the history its lengths (m)
  DeviceBuf<float> in, hin, out;
  DeviceBuf<int> ids, hids;
  DeviceBuf<float4> g0, g1, cv, h0, h1, hcv, ocv;
  HIP_TRY(in.alloc(11 * m));
  HIP_TRY(ids.alloc(m));
  HIP_TRY(out.alloc(5 * m));  // colour, variance, length
  HIP_TRY(g0.alloc(m));
  HIP_TRY(g1.alloc(m));
  HIP_TRY(cv.alloc(m));
  HIP_TRY(ocv.alloc(m));
  const dim3 lin((npix + 255) / 256);
  const auto upload = [&](float* d, int* di, const float* c3, const float* v1, const float* n3, const float* p3,
                          const float* d1, const int* i1) -> int {
    HIP_TRY(hipMemcpyAsync(d, c3, sizeof(float) * 3 * m, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d + 3 * m, n3, sizeof(float) * 3 * m, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d + 6 * m, p3, sizeof(float) * 3 * m, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d + 9 * m, v1, sizeof(float) * m, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d + 10 * m, d1, sizeof(float) * m, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(di, i1, sizeof(int) * m, hipMemcpyHostToDevice, st));
    return KDPT_OK;
  };
  float* const d = in.get();
  if ((rc = upload(d, ids.get(), color, variance, normal, point, depth, id))) return rc;
  const DenoiseArrays arr{d, d + 9 * m, d + 3 * m, d + 6 * m, d + 10 * m, ids.get()};
  hipLaunchKernelGGL(k_denoise_pack, lin, dim3(256), 0, st, arr, npix, g0.get(), g1.get(), cv.get());
  HIP_TRY(hipGetLastError());
  const TemporalFrame cur{g0.get(), g1.get(), cv.get(), nullptr};
  TemporalFrame hf{};
  if (given) {
    HIP_TRY(hin.alloc(12 * m));
    HIP_TRY(hids.alloc(m));
    HIP_TRY(h0.alloc(m));
    HIP_TRY(h1.alloc(m));
    HIP_TRY(hcv.alloc(m));
    float* const e = hin.get();
    if ((rc = upload(e, hids.get(), h_color, h_variance, h_normal, h_point, h_depth, h_id))) return rc;
    HIP_TRY(hipMemcpyAsync(e + 11 * m, h_length, sizeof(float) * m, hipMemcpyHostToDevice, st));
    const DenoiseArrays harr{e, e + 9 * m, e + 3 * m, e + 6 * m, e + 10 * m, hids.get()};
    hipLaunchKernelGGL(k_temporal_pack_history, lin, dim3(256), 0, st, harr, npix, h0.get(), h1.get(), hcv.get());
    HIP_TRY(hipGetLastError());
    hf = TemporalFrame{h0.get(), h1.get(), hcv.get(), e + 11 * m};
  }
  if ((rc = launch_temporal(*p, w, h, cur, given ? &hf : nullptr, given ? *h_camera : kdpt_camera{}, ocv.get(),
                            out.get() + 4 * m, nullptr, st)))
    return rc;
  hipLaunchKernelGGL(k_denoise_unpack, lin, dim3(256), 0, st, (const float4*)ocv.get(), npix, out.get(),
                     out.get() + 3 * m);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(out_color, out.get(), sizeof(float) * 3 * m, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(out_variance, out.get() + 3 * m, sizeof(float) * m, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(out_length, out.get() + 4 * m, sizeof(float) * m, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  return KDPT_OK;
}

int kdpt_denoise_temporal(kdpt_ctx* c, const kdpt_temporal_params* tp, const kdpt_denoise_params* dp,
                          float* out_color, float* out_variance) {
  const std::string who = "kdpt_denoise_temporal";
  if (!c) return fail(KDPT_ERR_ARG, who + ": null ctx");
  if (!tp) return fail(KDPT_ERR_ARG, who + ": null temporal params");
  if (!dp) return fail(KDPT_ERR_ARG, who + ": null params");
  if (!out_color) return fail(KDPT_ERR_ARG, who + ": null out_color");
  int rc = check_temporal_params(tp, who);
  if (rc || (rc = check_denoise_params(dp, who))) return rc;
  if (!c->mom.on) return fail(KDPT_ERR_UNSUPPORTED, who + ": moments are off (kdpt_set_moments)");
  if (c->mom.samples < 2)
    return fail(KDPT_ERR_ARG, who + ": " + std::to_string(c->mom.samples) +
                                  " iteration(s) accumulated, a variance needs at least 2");
  if (c->brute || c->viz)
    return fail(KDPT_ERR_UNSUPPORTED, who + ": the context runs the brute-force or box-view intersect kernel "
                                            "(enable_kd = 0 / viz_kd = 1); the guides need kdpt_cast_rays' KD "
                                            "traversal");
  if ((rc = kdpt_synchronize(c))) return rc;  // everything queued on the context first, the pipelined adds included
  if ((rc = join_accum(c)) || (rc = denoise_buffers(c)) || (rc = temporal_sets(c))) return rc;
  const hipStream_t st = c->stream;
  const Denoiser::Buffers& b = c->den.b;
  Temporal& T = c->tmp;
  Temporal::Sets& s = T.s;
  const Temporal::Set& hist = s.set[s.cur];
  const Temporal::Set& next = s.set[s.cur ^ 1];
  const int npix = c->npix;
  const size_t m = (size_t)npix;
  const dim3 lin((npix + 255) / 256);
  // ---- the guides, kdpt_denoise's ----
  HIP_TRY(hipEventRecord(T.ev[0], st));
  if ((rc = launch_denoise_guides(c))) return rc;
  HIP_TRY(hipEventRecord(T.ev[1], st));
  // ---- the temporal stage: the frame's records into `next` (C and V through the denoiser's cv[0]), blended ----
  HIP_TRY(hipMemsetAsync(s.counts.get(), 0, sizeof(unsigned int) * 2, st));
  hipLaunchKernelGGL(k_denoise_pack_render, lin, dim3(256), 0, st, (const float*)c->image,
                     (const float*)c->mom.sumsq.get(), (const uint32_t*)c->mom.adapt.extra.get(), c->mom.samples,
                     (const kdpt_ray_hit*)b.hits_out.get(), npix, next.g0.get(), next.g1.get(), b.cv[0].get());
  HIP_TRY(hipGetLastError());
  const TemporalFrame cur{next.g0.get(), next.g1.get(), b.cv[0].get(), nullptr};
  const TemporalFrame hf{hist.g0.get(), hist.g1.get(), hist.cv.get(), hist.len.get()};
  if ((rc = launch_temporal(*tp, c->W, c->H, cur, s.have ? &hf : nullptr, s.cam, next.cv.get(), next.len.get(),
                            s.counts.get(), st)))
    return rc;
  HIP_TRY(hipEventRecord(T.ev[2], st));
  // ---- the filter: pass 0 reads C', V' where they stay as the history; the passes write the denoiser's cv ----
  float4* const cv[2] = {b.cv[0].get(), b.cv[1].get()};
  const float4* last = nullptr;
  if ((rc = launch_denoise_passes(*dp, c->W, c->H, next.g0.get(), next.g1.get(), next.cv.get(), cv, st, &last)))
    return rc;
  const bool col_dev = on_context_device(c, out_color), var_dev = out_variance && on_context_device(c, out_variance);
  float* const d_col = col_dev ? out_color : b.out_stage.get();
  float* const d_var = !out_variance ? nullptr : (var_dev ? out_variance : b.out_stage.get() + 3 * m);
  hipLaunchKernelGGL(k_denoise_unpack, lin, dim3(256), 0, st, last, npix, d_col, d_var);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(T.ev[3], st));
  if ((rc = stage_out(col_dev, out_color, (const float*)d_col, 3 * m, st))) return rc;
  if (out_variance && (rc = stage_out(var_dev, out_variance, (const float*)d_var, m, st))) return rc;
  unsigned int counts[2] = {0, 0};
  HIP_TRY(hipMemcpyAsync(counts, s.counts.get(), sizeof(counts), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  // the frame is complete: it becomes the history, with the camera it was made under
  s.cur ^= 1;
  s.have = true;
  s.cam = c->cam;
  float ms[3] = {0, 0, 0};
  for (int i = 0; i < 3; i++) HIP_TRY(hipEventElapsedTime(&ms[i], T.ev[i], T.ev[i + 1]));
  T.guide_ms = ms[0];
  T.temporal_ms = ms[1];
  T.filter_ms = ms[2];
  T.valid = counts[0];
  T.with_history = counts[1];
  return check_fault(&c->solo, c->stream);
}

int kdpt_temporal_reset(kdpt_ctx* c) {
  if (!c) return fail(KDPT_ERR_ARG, "kdpt_temporal_reset: null ctx");
  c->tmp.s = {};  // (nothing is queued on the sets: every call that uses them ends with a synchronisation)
  return KDPT_OK;
}

int kdpt_temporal_stats(kdpt_ctx* c, double* guide_ms, double* temporal_ms, double* filter_ms, long long* valid,
                        long long* with_history) {
  if (!c) return fail(KDPT_ERR_ARG, "kdpt_temporal_stats: null ctx");
  if (guide_ms) *guide_ms = c->tmp.guide_ms;
  if (temporal_ms) *temporal_ms = c->tmp.temporal_ms;
  if (filter_ms) *filter_ms = c->tmp.filter_ms;
  if (valid) *valid = c->tmp.valid;
  if (with_history) *with_history = c->tmp.with_history;
  return KDPT_OK;
}
