// host_moments.h -- per-pixel second moments (kdpt_set_moments, kdpt_noise_*) and adaptive sampling
// (kdpt_active_pixels, kdpt_trace_adaptive, kdpt_read_sample_counts, kdpt_save_counted).
//
// A host section of kdpt_runtime.hip's translation unit, not a stand-alone header: kdpt_runtime.hip includes it
// after host_queries.h.  Host code only: no kernel is defined here (the kernels_*.h sections hold them), and
// tests/test_stream_discipline.py and tests/test_resource_ownership.py read every host section.
#pragma once

// Per-pixel second moments (include/kdpt.h "Second moments"): kdpt_set_moments, kdpt_read_moments,
// kdpt_noise_map and kdpt_noise_estimate.  While they are on, every add of partial images into the image goes
// through k_accumulate_moments (launch_accumulate), which adds the squares into mom_sumsq in the same pass; the
// shading, intersect and gather kernels never know.
namespace {

// k_noise_partials' workgroups: NOISE_BLOCK * NOISE_PER_LANE pixels each.
int noise_blocks(const kdpt_ctx* c) {
  const int per = NOISE_BLOCK * NOISE_PER_LANE;
  return (int)(((long long)c->npix + per - 1) / per);
}

// What kdpt_noise_map and kdpt_noise_estimate refuse, in the same order.
int check_noise_args(const kdpt_ctx* c, float floor, const std::string& who) {
  if (!c) return fail(KDPT_ERR_ARG, who + ": null ctx");
  if (!(std::isfinite(floor) && floor > 0.0f)) return fail(KDPT_ERR_ARG, who + ": floor must be finite and > 0");
  if (!c->mom.on) return fail(KDPT_ERR_UNSUPPORTED, who + ": moments are off (kdpt_set_moments)");
  if (c->mom.samples < 2)
    return fail(KDPT_ERR_ARG, who + ": " + std::to_string(c->mom.samples) +
                                  " iteration(s) accumulated, a variance needs at least 2");
  return KDPT_OK;
}

}  // namespace

int kdpt_set_moments(kdpt_ctx* c, int enable) {
  if (!c) return fail(KDPT_ERR_ARG, "kdpt_set_moments: null ctx");
  const bool on = enable != 0;
  if (on == c->mom.on) return KDPT_OK;
  if (on && (c->stats.iterations != 0 || c->accumulated))
    return fail(KDPT_ERR_UNSUPPORTED,
                "kdpt_set_moments: iterations have been accumulated into the image since the last kdpt_reset; "
                "call kdpt_reset first, so that the image and the moments describe the same samples");
  int rc = kdpt_synchronize(c);  // everything queued on the context first (the solo state changes its target)
  if (rc) return rc;
  if (!on) {  // the buffers go, and the solo state gathers straight into the image again (solo_targets)
    c->mom = {};
    return KDPT_OK;
  }
  const size_t n3 = 3 * (size_t)c->npix;
  hipError_t e;
  if ((e = c->mom.sumsq.alloc(n3)) != hipSuccess || (e = c->mom.partial.alloc(n3)) != hipSuccess ||
      (e = c->mom.noise_stage.alloc((size_t)c->npix)) != hipSuccess ||
      (e = c->mom.noise_parts.alloc((size_t)noise_blocks(c) + 1)) != hipSuccess ||
      (e = hipMemsetAsync(c->mom.sumsq.get(), 0, sizeof(float) * n3, c->stream)) != hipSuccess ||
      (e = hipStreamSynchronize(c->stream)) != hipSuccess) {
    c->mom = {};
    return hip_fail("kdpt_set_moments", e);
  }
  c->mom.samples = 0;
  c->mom.on = true;
  return KDPT_OK;
}

int kdpt_read_moments(kdpt_ctx* c, float* sumsq, long long* samples) {
  if (!c) return fail(KDPT_ERR_ARG, "kdpt_read_moments: null ctx");
  if (!c->mom.on) return fail(KDPT_ERR_UNSUPPORTED, "kdpt_read_moments: moments are off (kdpt_set_moments)");
  HIP_TRY(hipSetDevice(c->device));
  int rc = join_accum(c);
  if (rc) return rc;
  if (sumsq)
    HIP_TRY(hipMemcpyAsync(sumsq, c->mom.sumsq.get(), sizeof(float) * 3 * (size_t)c->npix, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  if (samples) *samples = c->mom.samples;
  return KDPT_OK;
}

int kdpt_noise_map(kdpt_ctx* c, float floor, float* noise) {
  int rc = check_noise_args(c, floor, "kdpt_noise_map");
  if (rc) return rc;
  if (!noise) return fail(KDPT_ERR_ARG, "kdpt_noise_map: null noise");
  HIP_TRY(hipSetDevice(c->device));
  if ((rc = join_accum(c))) return rc;
  const bool dev = on_context_device(c, noise);
  float* const d = dev ? noise : c->mom.noise_stage.get();
  if (const uint32_t* extra = c->mom.adapt.extra.get())  // per-pixel sample counts since an adaptive call
    hipLaunchKernelGGL(k_noise_map_counted, dim3((c->npix + 255) / 256), dim3(256), 0, c->stream, c->image,
                       c->mom.sumsq.get(), extra, c->npix, c->mom.samples, floor, d);
  else
    hipLaunchKernelGGL(k_noise_map, dim3((c->npix + 255) / 256), dim3(256), 0, c->stream, c->image,
                       c->mom.sumsq.get(), c->npix, c->mom.samples, floor, d);
  HIP_TRY(hipGetLastError());
  if ((rc = stage_out(dev, noise, d, (size_t)c->npix, c->stream))) return rc;
  HIP_TRY(hipStreamSynchronize(c->stream));
  return KDPT_OK;
}

int kdpt_noise_estimate(kdpt_ctx* c, float floor, float threshold, kdpt_noise* out) {
  int rc = check_noise_args(c, floor, "kdpt_noise_estimate");
  if (rc) return rc;
  if (std::isnan(threshold)) return fail(KDPT_ERR_ARG, "kdpt_noise_estimate: threshold is NaN");
  if (!out) return fail(KDPT_ERR_ARG, "kdpt_noise_estimate: null out");
  HIP_TRY(hipSetDevice(c->device));
  if ((rc = join_accum(c))) return rc;
  const int nb = noise_blocks(c);
  NoisePartial* const parts = c->mom.noise_parts.get();
  if (const uint32_t* extra = c->mom.adapt.extra.get())
    hipLaunchKernelGGL(k_noise_partials_counted, dim3(nb), dim3(NOISE_BLOCK), 0, c->stream, c->image,
                       c->mom.sumsq.get(), extra, c->npix, c->mom.samples, floor, threshold, parts);
  else
    hipLaunchKernelGGL(k_noise_partials, dim3(nb), dim3(NOISE_BLOCK), 0, c->stream, c->image, c->mom.sumsq.get(),
                       c->npix, c->mom.samples, floor, threshold, parts);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(k_noise_final, dim3(1), dim3(NOISE_BLOCK), 0, c->stream, parts, nb, parts + nb);
  HIP_TRY(hipGetLastError());
  NoisePartial r{};
  HIP_TRY(hipMemcpyAsync(&r, parts + nb, sizeof r, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  const long long finite = (long long)c->npix - r.nonfinite;
  memset(out, 0, sizeof *out);
  out->samples = c->mom.samples;
  out->pixels = c->npix;
  out->above = r.above;
  out->nonfinite = r.nonfinite;
  out->mean = finite > 0 ? r.sum / (double)finite : 0.0;
  out->max = r.max;
  return KDPT_OK;
}

// ---------------------------------------------------------------------------
// Adaptive sampling (include/kdpt.h "Adaptive sampling"): kdpt_active_pixels, kdpt_trace_adaptive,
// kdpt_read_sample_counts, kdpt_save_counted and kdpt_selftest_active_list.  The list is built on the context's
// stream (k_adapt_flags, k_adapt_scan, k_adapt_list); the iterations over it take kdpt_trace_iterations' pipelined
// route with an active set (enqueue_iterations): k_adapt_geoms_b / k_adapt_rays_b for the camera stage,
// launch_batch's kernels as they are, k_accumulate_adapt for the add.
// ---------------------------------------------------------------------------
namespace {

int adapt_blocks(int npix) { return (npix + ADAPT_BLOCK - 1) / ADAPT_BLOCK; }

// What kdpt_active_pixels and kdpt_trace_adaptive refuse beyond their own arguments, before any device work.
int check_adaptive_args(const kdpt_ctx* c, float floor, float threshold, const std::string& who) {
  if (!(std::isfinite(floor) && floor > 0.0f)) return fail(KDPT_ERR_ARG, who + ": floor must be finite and > 0");
  if (std::isnan(threshold)) return fail(KDPT_ERR_ARG, who + ": threshold is NaN");
  if (!c) return fail(KDPT_ERR_ARG, who + ": null ctx");
  if (!c->mom.on) return fail(KDPT_ERR_UNSUPPORTED, who + ": moments are off (kdpt_set_moments)");
  if (c->frames.comm || c->frames.nranks > 1)
    return fail(KDPT_ERR_UNSUPPORTED, who + ": the context is in a communicator (kdpt_comm_init): its frames reach "
                                            "the image through a reduce that carries no per-pixel counts");
  if (c->mom.samples < 2)
    return fail(KDPT_ERR_ARG, who + ": " + std::to_string(c->mom.samples) +
                                  " iteration(s) accumulated, a variance needs at least 2");
  return KDPT_OK;
}

// The adaptive state, made on first use: extra starts at zero (filled on the context's stream and waited for).
int adaptive_state(kdpt_ctx* c) {
  Adaptive& a = c->mom.adapt;
  if (a.extra) return KDPT_OK;
  const size_t npix = (size_t)c->npix, nblk = (size_t)adapt_blocks(c->npix);
  Adaptive fresh;
  hipError_t e;
  if ((e = fresh.extra.alloc(npix)) != hipSuccess || (e = fresh.list.alloc(npix)) != hipSuccess ||
      (e = fresh.masks.alloc(nblk * (ADAPT_BLOCK / 64))) != hipSuccess ||
      (e = fresh.blocks.alloc(2 * nblk + 1)) != hipSuccess || (e = fresh.totals.alloc(4)) != hipSuccess ||
      (e = fresh.ev[0].create()) != hipSuccess || (e = fresh.ev[1].create()) != hipSuccess ||
      (e = hipMemsetAsync(fresh.extra.get(), 0, sizeof(uint32_t) * npix, c->stream)) != hipSuccess ||
      (e = hipStreamSynchronize(c->stream)) != hipSuccess)
    return hip_fail("adaptive sampling: device buffers", e);
  a = std::move(fresh);
  return KDPT_OK;
}

// The three list launches on stream st; values: the self test's per-pixel values (null: the context's noise).
void launch_active_list(const float* image, const float* sumsq, const uint32_t* extra, const float* values, int npix,
                        long long samples, float floor, float threshold, unsigned long long* masks, int* blocks,
                        int* list, hipStream_t st) {
  const int nblk = adapt_blocks(npix);
  int* const counts = blocks, * const offs = blocks + nblk, * const total = blocks + 2 * nblk;
  if (values)
    hipLaunchKernelGGL(k_adapt_flags<true>, dim3(nblk), dim3(ADAPT_BLOCK), 0, st, image, sumsq, extra, values, npix,
                       samples, floor, threshold, masks, counts);
  else
    hipLaunchKernelGGL(k_adapt_flags<false>, dim3(nblk), dim3(ADAPT_BLOCK), 0, st, image, sumsq, extra, values, npix,
                       samples, floor, threshold, masks, counts);
  hipLaunchKernelGGL(k_adapt_scan, dim3(1), dim3(ADAPT_BLOCK), 0, st, counts, nblk, offs, total);
  hipLaunchKernelGGL(k_adapt_list, dim3(nblk), dim3(ADAPT_BLOCK), 0, st, masks, offs, list);
}

// The context's active list from its current sums, and |A| read back: the call's one host read before its end.
// (The caller has synchronised the context.)
int build_active_list(kdpt_ctx* c, float floor, float threshold, int* active) {
  int rc = adaptive_state(c);
  if (rc) return rc;
  Adaptive& a = c->mom.adapt;
  launch_active_list(c->image, c->mom.sumsq.get(), a.extra.get(), nullptr, c->npix, c->mom.samples, floor, threshold,
                     a.masks.get(), a.blocks.get(), a.list.get(), c->stream);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(active, a.blocks.get() + 2 * adapt_blocks(c->npix), sizeof(int), hipMemcpyDeviceToHost,
                         c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return KDPT_OK;
}

}  // namespace

int kdpt_active_pixels(kdpt_ctx* c, float floor, float threshold, int* pixels, long long* n) {
  if (!n) return fail(KDPT_ERR_ARG, "kdpt_active_pixels: null n");
  int rc = check_adaptive_args(c, floor, threshold, "kdpt_active_pixels");
  if (rc) return rc;
  HIP_TRY(hipSetDevice(c->device));
  int active = 0;
  if ((rc = kdpt_synchronize(c)) || (rc = build_active_list(c, floor, threshold, &active))) return rc;
  *n = active;
  if (!pixels || !active) return KDPT_OK;
  if ((rc = stage_out(on_context_device(c, pixels), pixels, (const int*)c->mom.adapt.list.get(), (size_t)active,
                      c->stream)))
    return rc;
  HIP_TRY(hipStreamSynchronize(c->stream));
  return KDPT_OK;
}

int kdpt_trace_adaptive(kdpt_ctx* c, int first_iter, int count, int pipeline, int batch, float floor,
                        float threshold, kdpt_adaptive* out) {
  const std::string who = "kdpt_trace_adaptive";
  if (first_iter < 1) return fail(KDPT_ERR_ARG, who + ": first_iter must be >= 1");
  if (count < 0) return fail(KDPT_ERR_ARG, who + ": count must be >= 0");
  if (!out) return fail(KDPT_ERR_ARG, who + ": null out");
  int rc = check_adaptive_args(c, floor, threshold, who);
  if (rc) return rc;
  if (c->shade_oob) return refuse_shading();
  HIP_TRY(hipSetDevice(c->device));
  // everything queued on the context first, the pipelined adds included: the list is built from the state before
  // the call
  int active = 0;
  if ((rc = kdpt_synchronize(c)) || (rc = build_active_list(c, floor, threshold, &active))) return rc;
  memset(out, 0, sizeof *out);
  out->pixels = c->npix;
  out->active = active;
  if (!active || !count) return KDPT_OK;
  Adaptive& a = c->mom.adapt;
  const hipStream_t st = c->stream;
  HIP_TRY(hipEventRecord(a.ev[0], st));
  HIP_TRY(hipMemsetAsync(a.totals.get(), 0, sizeof(unsigned long long) * 4, st));
  const ActiveSet act{a.list.get(), active, a.extra.get()};
  if ((rc = enqueue_iterations(c, {first_iter, count, 1, pipeline, batch, c->image, nullptr, &act, a.totals.get()})))
    return rc;
  if ((rc = join_accum(c))) return rc;  // the context's stream after the last add
  HIP_TRY(hipEventRecord(a.ev[1], st));
  unsigned long long totals[4] = {0, 0, 0, 0};
  HIP_TRY(hipMemcpyAsync(totals, a.totals.get(), sizeof totals, hipMemcpyDeviceToHost, st));
  if ((rc = kdpt_synchronize(c))) return rc;  // (the groups' fault words too)
  float ms = 0;
  HIP_TRY(hipEventElapsedTime(&ms, a.ev[0], a.ev[1]));
  out->pixel_samples = (long long)active * count;
  out->segments = (long long)totals[0];
  out->traced = (long long)totals[3];
  out->device_ms = ms;
  return KDPT_OK;
}

int kdpt_read_sample_counts(kdpt_ctx* c, int* counts) {
  if (!c) return fail(KDPT_ERR_ARG, "kdpt_read_sample_counts: null ctx");
  if (!counts) return fail(KDPT_ERR_ARG, "kdpt_read_sample_counts: null counts");
  if (!c->mom.on) return fail(KDPT_ERR_UNSUPPORTED, "kdpt_read_sample_counts: moments are off (kdpt_set_moments)");
  HIP_TRY(hipSetDevice(c->device));
  int rc = join_accum(c);
  if (rc) return rc;
  const size_t npix = (size_t)c->npix;
  if (c->mom.adapt.extra)
    HIP_TRY(hipMemcpyAsync(counts, c->mom.adapt.extra.get(), sizeof(int) * npix, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  for (size_t p = 0; p < npix; p++) counts[p] = (int)c->mom.samples + (c->mom.adapt.extra ? counts[p] : 0);
  return KDPT_OK;
}

int kdpt_save_counted(kdpt_ctx* c, uint8_t* rgb, float* lin) {
  if (!c) return fail(KDPT_ERR_ARG, "kdpt_save_counted: null ctx");
  if (!rgb && !lin) return fail(KDPT_ERR_ARG, "kdpt_save_counted: null rgb and lin");
  if (!c->mom.on) return fail(KDPT_ERR_UNSUPPORTED, "kdpt_save_counted: moments are off (kdpt_set_moments)");
  return save_image_pass(c, 0.0f, rgb, lin, true);
}
