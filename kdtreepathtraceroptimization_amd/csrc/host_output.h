// host_output.h -- reading results out: the image (kdpt_read_image, kdpt_write_pbo, kdpt_save_*), kdpt_get_stats,
// the route reports, and the debug entry points (kdpt_debug_paths, kdpt_count_iteration, the profiles).
//
// A host section of kdpt_runtime.hip's translation unit, not a stand-alone header: kdpt_runtime.hip includes it
// after host_pipeline.h.  Host code only: no kernel is defined here (the kernels_*.h sections hold them), and
// tests/test_stream_discipline.py and tests/test_resource_ownership.py read every host section.
#pragma once

namespace {

// The solo state's next iteration into a scratch image and a scratch segment total (zeroed on the context's
// stream), so that the accumulation image and stats.total_segments stay as they are; the intersect totals are the
// context's.  The scratch buffer goes with the object (hipFree waits for whatever an early return left running).
struct ScratchTargets {
  DeviceBuf<unsigned long long> scratch;  // the total, then the image (the total's 64-bit atomics need its alignment)
  Targets to{};
  int make(kdpt_ctx* c) {
    const size_t words = 1 + (3 * (size_t)c->npix + 1) / 2;
    HIP_TRY(scratch.alloc(words));
    HIP_TRY(hipMemsetAsync(scratch.get(), 0, sizeof(unsigned long long) * words, c->stream));
    to = solo_targets(c);
    to.image = reinterpret_cast<float*>(scratch.get() + 1);
    to.total_segments = scratch.get();
    return KDPT_OK;
  }
};

}  // namespace

#ifdef KDPT_TAIL_PROF
extern "C" int kdpt_debug_tail_prof(unsigned long long* out) {  // sums, then zeroes, the counters
  const unsigned long long zero[4] = {0, 0, 0, 0};
  hipError_t e;
  if ((e = hipDeviceSynchronize()) != hipSuccess ||
      (e = hipMemcpyFromSymbol(out, HIP_SYMBOL(g_tail_prof), sizeof(zero))) != hipSuccess ||
      (e = hipMemcpyToSymbol(HIP_SYMBOL(g_tail_prof), zero, sizeof(zero))) != hipSuccess)
    return fail(-1, std::string("kdpt_debug_tail_prof: ") + hipGetErrorString(e));
  return 0;
}
#endif
#ifdef KDPT_SHADE_PROF
extern "C" int kdpt_debug_shade_prof(unsigned long long* out) {  // sums, then zeroes, the counters
  const unsigned long long zero[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  hipError_t e;
  if ((e = hipDeviceSynchronize()) != hipSuccess ||
      (e = hipMemcpyFromSymbol(out, HIP_SYMBOL(g_shade_prof), sizeof(zero))) != hipSuccess ||
      (e = hipMemcpyToSymbol(HIP_SYMBOL(g_shade_prof), zero, sizeof(zero))) != hipSuccess)
    return fail(-1, std::string("kdpt_debug_shade_prof: ") + hipGetErrorString(e));
  return 0;
}
#endif
extern "C" {

int kdpt_read_image(kdpt_ctx* c, float* rgb) {
  if (!c || !rgb) return fail(KDPT_ERR_ARG, "null arg");
  HIP_TRY(hipSetDevice(c->device));
  int rc = join_accum(c);
  if (rc) return rc;
  HIP_TRY(hipMemcpyAsync(rgb, c->image, sizeof(float) * 3 * (size_t)c->npix, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return KDPT_OK;
}

int kdpt_trace_config(kdpt_ctx* c, int* tree_mode, int* block, int* grid, long long* lds_bytes) {
  if (!c) return fail(KDPT_ERR_ARG, "null ctx");
  const int m = c->tree_mode;
  if (tree_mode) *tree_mode = m;
  if (block) *block = trace_kernel(false, false, m).block;
  if (grid) *grid = c->full_trace_grid;
  if (lds_bytes) *lds_bytes = (long long)c->tree_lds;
  return KDPT_OK;
}

int kdpt_shade_staged(kdpt_ctx* c, int* staged) {
  if (!c || !staged) return fail(KDPT_ERR_ARG, "null arg");
  *staged = shade_staged(c) ? 1 : 0;
  return KDPT_OK;
}

int kdpt_cull_margin(kdpt_ctx* c, float* margin, double* rigorous, int* exact) {
  if (!c) return fail(KDPT_ERR_ARG, "null ctx");
  if (c->brute && c->cull_scene) {
    // the chunk cull: every chunk at its own rigorous coefficient (the smallest is reported; +inf: no chunk culls)
    if (margin) *margin = c->bf.chunk_k_min;
    if (rigorous) *rigorous = c->cull.rigorous;
    if (exact) *exact = 1;
    return KDPT_OK;
  }
  if (margin) *margin = c->S.cl_margin;
  if (rigorous) *rigorous = c->cull.rigorous;
  // the box-only levels use cl_margin; the slab level's margin is rigorous by construction whenever that is;
  // the masked one-level cull is exact whatever the margin (its masks hold every triangle that can pass)
  if (exact) *exact = ((double)c->S.cl_margin >= c->cull.rigorous || c->S.cl_mask) ? 1 : 0;
  return KDPT_OK;
}

int kdpt_write_pbo(kdpt_ctx* c, int iter, uint8_t* rgba) {
  if (!c || !rgba || iter == 0) return fail(KDPT_ERR_ARG, "bad arg");
  HIP_TRY(hipSetDevice(c->device));
  int rc = join_accum(c);
  if (rc) return rc;
  // The reference's pbo is the GL-mapped device buffer (src/main.cpp runCuda); a headless caller passes host
  // memory.  Memory of this context's device is written by the kernel directly; anything else (host memory,
  // another device's buffer) through the context's staging buffer and a copy.
  const bool on_device = on_context_device(c, rgba);
  uchar4* d = reinterpret_cast<uchar4*>(rgba);
  if (!on_device) {
    if (!c->pbo_staging) HIP_TRY(c->pbo_staging.alloc((size_t)c->npix));
    d = c->pbo_staging.get();
  }
  hipLaunchKernelGGL(k_pbo, dim3((c->npix + 255) / 256), dim3(256), 0, c->stream, c->image, c->npix, iter, d);
  HIP_TRY(hipGetLastError());
  if (!on_device)
    HIP_TRY(hipMemcpyAsync(rgba, d, sizeof(uchar4) * (size_t)c->npix, hipMemcpyDefault, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return KDPT_OK;
}

// The saveImage pixel pass on the device; rgb (host, 3*W*H) and/or lin (host, 3*W*H floats).  counted
// (kdpt_save_counted): each pixel divided by its own sample count (k_save_counted) instead of `samples`.
static int save_image_pass(kdpt_ctx* c, float samples, uint8_t* rgb, float* lin, bool counted = false) {
  HIP_TRY(hipSetDevice(c->device));
  for (auto& grp : c->pipe.groups) HIP_TRY(hipStreamSynchronize(grp.stream));
  if (c->frames.reduce_stream) HIP_TRY(hipStreamSynchronize(c->frames.reduce_stream));
  const size_t n3 = 3 * (size_t)c->npix;
  DeviceBuf<uint8_t> d_rgb;
  DeviceBuf<float> d_lin;  // (null without `lin`)
  HIP_TRY(d_rgb.alloc(n3));
  if (lin) HIP_TRY(d_lin.alloc(n3));
  if (counted)
    hipLaunchKernelGGL(k_save_counted, dim3((c->npix + 255) / 256), dim3(256), 0, c->stream, c->image,
                       c->mom.adapt.extra.get(), c->W, c->H, c->mom.samples, d_rgb.get(), d_lin.get());
  else
    hipLaunchKernelGGL(k_save_image, dim3((c->npix + 255) / 256), dim3(256), 0, c->stream, c->image, c->W, c->H,
                       samples, d_rgb.get(), d_lin.get());
  HIP_TRY(hipGetLastError());
  if (rgb) HIP_TRY(hipMemcpyAsync(rgb, d_rgb.get(), n3, hipMemcpyDeviceToHost, c->stream));
  if (lin) HIP_TRY(hipMemcpyAsync(lin, d_lin.get(), n3 * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return KDPT_OK;
}

int kdpt_save_rgb8(kdpt_ctx* c, float samples, uint8_t* rgb) {
  if (!c || !rgb) return fail(KDPT_ERR_ARG, "null arg");
  return save_image_pass(c, samples, rgb, nullptr);
}

int kdpt_save_png(kdpt_ctx* c, const char* path, float samples) {
  if (!c || !path) return fail(KDPT_ERR_ARG, "null arg");
  std::vector<uint8_t> rgb(3 * (size_t)c->npix);
  int rc = save_image_pass(c, samples, rgb.data(), nullptr);
  if (rc) return rc;
  return kdpt_write_png(path, rgb.data(), c->W, c->H);  // (its failure names the path and the reason)
}

int kdpt_save_hdr(kdpt_ctx* c, const char* path, float samples) {
  if (!c || !path) return fail(KDPT_ERR_ARG, "null arg");
  std::vector<float> lin(3 * (size_t)c->npix);
  int rc = save_image_pass(c, samples, nullptr, lin.data());
  if (rc) return rc;
  return kdpt_write_hdr(path, lin.data(), c->W, c->H);
}

int kdpt_cull_masks(kdpt_ctx* c, int* mask_n, int* num_clusters, unsigned long long* masks) {
  if (!c || !mask_n || !num_clusters) return fail(KDPT_ERR_ARG, "null arg");
  HIP_TRY(hipSetDevice(c->device));
  *mask_n = c->masks.dev ? c->masks.n : 0;
  *num_clusters = c->S.num_clusters;
  if (!c->masks.dev) return KDPT_OK;
  const size_t cells = 6 * (size_t)c->masks.n * c->masks.n * (size_t)c->S.num_clusters;
  HIP_TRY(hipStreamSynchronize(c->stream));
  if (masks)
    HIP_TRY(hipMemcpyAsync(masks, c->masks.dev.get(), cells * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return KDPT_OK;
}

int kdpt_get_stats(kdpt_ctx* c, kdpt_stats* st) {
  if (!c || !st) return fail(KDPT_ERR_ARG, "null arg");
  HIP_TRY(hipSetDevice(c->device));
  unsigned long long tot = 0, tt[3] = {0, 0, 0};
  HIP_TRY(hipMemcpyAsync(&tot, c->total_segments, sizeof tot, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipMemcpyAsync(tt, c->trace_total, sizeof tt, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  c->stats.intersect_device_ms_total = (double)tt[0] / c->wall_khz;
  c->stats.intersect_device_launches_total = (long long)tt[1];
  c->stats.total_trace_rays = (long long)tt[2];
  c->stats.total_segments = (long long)tot;
  c->stats.intersect_ms_total = c->intersect_ms_total;
  c->stats.intersect_launches_total = c->intersect_launches_total;
  c->stats.create_ms = c->create_ms;
  c->stats.mask_build_ms = c->masks.build_ms;
  *st = c->stats;
  return KDPT_OK;
}

int kdpt_image_device_ptr(kdpt_ctx* c, void** p) {
  if (!c || !p) return fail(KDPT_ERR_ARG, "null arg");
  *p = c->image;
  return KDPT_OK;
}

int kdpt_debug_paths(kdpt_ctx* c, int iter, int stop_depth, kdpt_path_segment* out, int* npaths) {
  if (!c || !out || stop_depth < 0 || stop_depth >= c->cap) return fail(KDPT_ERR_ARG, "bad arg");
  HIP_TRY(hipSetDevice(c->device));
  IterState& it = c->solo;
  ScratchTargets scratch;
  int rc = scratch.make(c);
  if (rc || (rc = launch_iteration(c, iter, scratch.to, stop_depth))) return rc;
  DeviceBuf<kdpt_path_segment> d;
  HIP_TRY(d.alloc((size_t)c->npix));
  const int depth_slot = stop_depth + 1;
  hipLaunchKernelGGL(k_unpack, dim3((c->npix + 255) / 256), dim3(256), 0, c->stream, it.buf[it.cur], it.counts,
                     depth_slot, d.get());
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(it.h_counts.get(), it.counts, sizeof(int) * (c->cap + 2), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  if ((rc = check_fault(&it, c->stream))) return rc;
  const int n = it.h_counts.get()[depth_slot];
  *npaths = n;
  HIP_TRY(hipMemcpy(out, d.get(), sizeof(kdpt_path_segment) * (size_t)n, hipMemcpyDeviceToHost));
  return KDPT_OK;
}

// Roofline counters: one extra (untimed) iteration with per-path AABB/triangle/hit counts.
int kdpt_count_iteration(kdpt_ctx* c, int iter, unsigned long long* aabb_tri_hit) {
  if (!c || !aabb_tri_hit) return fail(KDPT_ERR_ARG, "null arg");
  HIP_TRY(hipSetDevice(c->device));
  IterState& it = c->solo;
  ScratchTargets scratch;
  int rc = scratch.make(c);
  if (rc) return rc;
  HIP_TRY(hipMemsetAsync(c->counters, 0, sizeof(Counters), c->stream));
  rc = launch_iteration(c, iter, scratch.to, -1, true);
  Counters h{};
  if (!rc) {
    HIP_TRY(hipMemcpyAsync(&h, c->counters, sizeof h, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(it.h_counts.get(), it.counts, sizeof(int) * (c->cap + 3), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    segments_from_counts(c);  // stats.segments / seg_per_bounce now describe the counting iteration
    rc = check_fault(&it, c->stream);
  }
  aabb_tri_hit[0] = h.aabb;
  aabb_tri_hit[1] = h.tri;
  aabb_tri_hit[2] = h.hit;
  c->last_profile = h;
  return rc;
}

int kdpt_count_split(kdpt_ctx* c, unsigned long long* aabb_prep_cand) {
  if (!c || !aabb_prep_cand) return fail(KDPT_ERR_ARG, "null arg");
  aabb_prep_cand[0] = c->last_profile.aabb_prep;
  aabb_prep_cand[1] = c->last_profile.cand;
  return KDPT_OK;
}

int kdpt_wave_profile(kdpt_ctx* c, unsigned long long* out, int n) {
  if (!c || !out) return fail(KDPT_ERR_ARG, "null arg");
  unsigned long long v[PROF_SLOTS + 5];
  for (int k = 0; k < PROF_SLOTS + 2; k++) v[k] = c->last_profile.wave[k];
  v[PROF_SLOTS + 2] = c->last_profile.aabb;
  v[PROF_SLOTS + 3] = c->last_profile.tri;
  v[PROF_SLOTS + 4] = c->last_profile.hit;
  int k = 0;
  for (; k < n && k < PROF_SLOTS + 5; k++) out[k] = v[k];
  for (int b = 0; b < 64 && k < n; b++, k++) out[k] = c->last_profile.life[b];
  for (int b = 0; b < 64 && k < n; b++, k++) out[k] = c->last_profile.steps[b];
  for (int b = 0; b < 8 && k < n; b++, k++) out[k] = c->last_profile.chord_steps[b];
  for (int b = 0; b < 8 && k < n; b++, k++) out[k] = c->last_profile.chord_n[b];
  return PROF_SLOTS + 5 + 64 + 64 + 16;
}

}  // extern "C"
