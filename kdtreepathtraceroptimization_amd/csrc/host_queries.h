// host_queries.h -- ray queries (kdpt_cast_rays) and caller-defined views (kdpt_set_camera, kdpt_camera_rays,
// kdpt_trace_rays[_moments]).
//
// A host section of kdpt_runtime.hip's translation unit, not a stand-alone header: kdpt_runtime.hip includes it
// after host_frames.h.  Host code only: no kernel is defined here (the kernels_*.h sections hold them), and
// tests/test_stream_discipline.py and tests/test_resource_ownership.py read every host section.
#pragma once

// Ray queries (include/kdpt.h "Ray queries"; kernels: k_cast_prep, k_trace, k_cast_resolve)
namespace {

// The query's buffers for chunks of c->cast.chunk rays (nothing is queued on the context: the caller has
// synchronised, so the old ones can go).
int cast_buffers(kdpt_ctx* c) {
  CastQuery::Buffers& b = c->cast.b;
  if (b.alloc == c->cast.chunk) return KDPT_OK;
  b = {};
  const size_t m = (size_t)c->cast.chunk;
  if (b.in.alloc(6 * m) != hipSuccess || b.out.alloc(m) != hipSuccess || b.cray.alloc(2 * m) != hipSuccess ||
      b.cand.alloc(m) != hipSuccess || b.hits.alloc(m) != hipSuccess || b.cnt.alloc(2) != hipSuccess ||
      b.tt.alloc(3) != hipSuccess) {
    (void)hipGetLastError();
    b = {};
    return fail(KDPT_ERR_HIP, "kdpt_cast_rays: cannot allocate the buffers of a " + std::to_string(m) +
                                  "-ray chunk (knob cast_chunk)");
  }
  for (Event& e : c->cast.ev)
    if (!e) HIP_TRY(e.create());
  b.alloc = c->cast.chunk;
  return KDPT_OK;
}

}  // namespace

int kdpt_cast_rays(kdpt_ctx* c, const float* origins, const float* directions, long long n, int flags,
                   kdpt_ray_hit* out) {
  if (n < 0) return fail(KDPT_ERR_ARG, "kdpt_cast_rays: n must be >= 0");
  if (flags & ~KDPT_CAST_NORMALIZE) return fail(KDPT_ERR_ARG, "kdpt_cast_rays: unknown bit in flags");
  if (!c) return fail(KDPT_ERR_ARG, "kdpt_cast_rays: null ctx");
  if (n > 0 && !origins) return fail(KDPT_ERR_ARG, "kdpt_cast_rays: null origins");
  if (n > 0 && !directions) return fail(KDPT_ERR_ARG, "kdpt_cast_rays: null directions");
  if (n > 0 && !out) return fail(KDPT_ERR_ARG, "kdpt_cast_rays: null out");
  if (c->brute || c->viz)
    return fail(KDPT_ERR_UNSUPPORTED, "kdpt_cast_rays: the context runs the brute-force or box-view intersect kernel "
                                      "(enable_kd = 0 / viz_kd = 1); ray queries need the KD traversal");
  if (n == 0) return KDPT_OK;
  int rc = kdpt_synchronize(c);  // everything queued on the context first
  if (rc) return rc;
  if ((rc = cast_buffers(c))) return rc;
  const hipStream_t st = c->stream;
  const bool o_dev = on_context_device(c, origins), d_dev = on_context_device(c, directions),
             out_dev = on_context_device(c, out);
  const CastQuery::Buffers& cb = c->cast.b;
  const int chunk = cb.alloc;
  HIP_TRY(hipMemsetAsync(cb.cnt.get(), 0, sizeof(int) * 2, st));
  HIP_TRY(hipMemsetAsync(cb.tt.get(), 0, sizeof(unsigned long long) * 3, st));
  HIP_TRY(hipEventRecord(c->cast.ev[0], st));
  CastArgs a;
  a.S = c->S;
  a.normalize = (flags & KDPT_CAST_NORMALIZE) ? 1 : 0;
  a.cray = cb.cray.get();
  a.hits = cb.hits.get();
  a.cand = cb.cand.get();
  a.cnt = cb.cnt.get();
  a.tt = cb.tt.get();
  // (one "iteration" at bounce 0: the query's own queue, its length in cast_cnt[1], the chunk counter in [0])
  const TraceArgs t{c->S, a.cand, a.cray, a.cnt + 1, a.hits, nullptr, 0, a.cnt, 0, c->counters, a.tt};
  void (*const resolve)(CastArgs) = hybrid_shading(c) ? k_cast_resolve<true> : k_cast_resolve<false>;
  for (long long off = 0; off < n; off += chunk) {
    const int m = (int)std::min<long long>(chunk, n - off);
    a.n = m;
    a.o = origins + 3 * off;
    a.d = directions + 3 * off;
    if ((rc = stage_in(o_dev, &a.o, 3 * (size_t)m, cb.in.get(), st)) ||
        (rc = stage_in(d_dev, &a.d, 3 * (size_t)m, cb.in.get() + 3 * (size_t)chunk, st)))
      return rc;
    a.out = out_dev ? out + off : cb.out.get();
    hipLaunchKernelGGL(k_cast_prep, dim3((m + GEN_BLOCK - 1) / GEN_BLOCK), dim3(GEN_BLOCK), 0, st, a);
    HIP_TRY(hipGetLastError());
    launch_trace(c, t, false, c->trace_grid, st);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(resolve, dim3((m + 255) / 256), dim3(256), 0, st, a);
    HIP_TRY(hipGetLastError());
    if ((rc = stage_out(out_dev, out + off, a.out, (size_t)m, st))) return rc;
  }
  HIP_TRY(hipEventRecord(c->cast.ev[1], st));
  unsigned long long traced = 0;
  HIP_TRY(hipMemcpyAsync(&traced, a.tt + 2, sizeof traced, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  float ms = 0;
  HIP_TRY(hipEventElapsedTime(&ms, c->cast.ev[0], c->cast.ev[1]));
  c->cast.ms = ms;
  c->cast.rays += n;
  c->cast.traced += (long long)traced;
  return check_fault(&c->solo, c->stream);
}

int kdpt_cast_stats(kdpt_ctx* c, long long* rays, long long* traced, double* device_ms) {
  if (!c) return fail(KDPT_ERR_ARG, "kdpt_cast_stats: null ctx");
  if (rays) *rays = c->cast.rays;
  if (traced) *traced = c->cast.traced;
  if (device_ms) *device_ms = c->cast.ms;
  return KDPT_OK;
}

// ---------------------------------------------------------------------------
// Caller-defined views (include/kdpt.h "Caller-defined views"): kdpt_set_camera, kdpt_camera_rays and
// kdpt_trace_rays.  The two queries run in the context's query state (kdpt_ctx::query), on its stream, after
// everything already queued; kernels: k_gen_rays_b, or k_user_rays_b / k_user_geoms_b and then launch_batch's.
// ---------------------------------------------------------------------------
namespace {

// The query's iteration state and buffers, made on first use (the caller has synchronised the context).
int query_state(kdpt_ctx* c) {
  RayQuery& q = c->query;
  if (!q.state) {  // (a failed alloc_iter drops the half-made state: the next call starts again)
    std::unique_ptr<IterState> it(new IterState());
    if (int rc = alloc_iter(c, it.get(), c->stream, false)) return rc;
    q.state = std::move(it);
  }
  const size_t npix = (size_t)c->npix;
  if (!q.image) HIP_TRY(q.image.alloc(3 * npix));
  if (!q.stage) HIP_TRY(q.stage.alloc(6 * npix));
  if (!q.totals) HIP_TRY(q.totals.alloc(4));
  return KDPT_OK;
}

}  // namespace

int kdpt_set_camera(kdpt_ctx* c, const kdpt_camera* cam) {
  if (!c) return fail(KDPT_ERR_ARG, "kdpt_set_camera: null ctx");
  if (!cam) return fail(KDPT_ERR_ARG, "kdpt_set_camera: null camera");
  // prepare_scene's checks of a scene's camera are on its resolution, which here must be the context's
  if (cam->resolution[0] != c->W || cam->resolution[1] != c->H)
    return fail(KDPT_ERR_ARG, "kdpt_set_camera: resolution " + std::to_string(cam->resolution[0]) + "x" +
                                  std::to_string(cam->resolution[1]) + " is not the context's " +
                                  std::to_string(c->W) + "x" + std::to_string(c->H));
  const float* const vecs[] = {cam->position, cam->lookAt, cam->view, cam->up, cam->right};
  bool finite = std::isfinite(cam->fov[0]) && std::isfinite(cam->fov[1]) && std::isfinite(cam->pixelLength[0]) &&
                std::isfinite(cam->pixelLength[1]);
  for (const float* v : vecs) finite = finite && std::isfinite(v[0]) && std::isfinite(v[1]) && std::isfinite(v[2]);
  if (!finite) return fail(KDPT_ERR_ARG, "kdpt_set_camera: a camera value is not finite");
  c->cam = *cam;  // launches take the camera by value: what is already queued keeps the one it was queued with
  return KDPT_OK;
}

int kdpt_camera_rays(kdpt_ctx* c, int iter, float* origins, float* directions) {
  if (!c) return fail(KDPT_ERR_ARG, "kdpt_camera_rays: null ctx");
  if (iter < 1) return fail(KDPT_ERR_ARG, "kdpt_camera_rays: iter must be >= 1");
  if (!origins) return fail(KDPT_ERR_ARG, "kdpt_camera_rays: null origins");
  if (!directions) return fail(KDPT_ERR_ARG, "kdpt_camera_rays: null directions");
  int rc = kdpt_synchronize(c);  // everything queued on the context first
  if (rc || (rc = query_state(c))) return rc;
  const hipStream_t st = c->stream;
  IterState& q = *c->query.state;
  q.cur = 0;
  GenBatch gb = gen_batch(c);
  gb.it[0] = q.gen_iter(c->opt.cacherays ? 1 : iter, nullptr);
  hipLaunchKernelGGL(k_gen_rays_b, dim3((c->npix + 255) / 256, 1), dim3(256), 0, st, gb);
  HIP_TRY(hipGetLastError());
  // xyz of p0 / p1 (float4 records) into packed triples: a strided copy each, straight into device memory of the
  // caller's, through the staging buffer into host memory
  const size_t npix = (size_t)c->npix, row = 3 * sizeof(float);
  float* const outs[2] = {origins, directions};
  const float4* const srcs[2] = {q.buf[0].p0, q.buf[0].p1};
  for (int k = 0; k < 2; k++) {
    const bool dev = on_context_device(c, outs[k]);
    float* const packed = dev ? outs[k] : c->query.stage.get() + 3 * npix * k;
    HIP_TRY(hipMemcpy2DAsync(packed, row, srcs[k], sizeof(float4), row, npix, hipMemcpyDeviceToDevice, st));
    if ((rc = stage_out(dev, outs[k], packed, 3 * npix, st))) return rc;
  }
  HIP_TRY(hipStreamSynchronize(st));
  return KDPT_OK;
}

namespace {

// kdpt_trace_rays (moments = false: the query's state gathers straight into its radiance buffer) and
// kdpt_trace_rays_moments (each iteration gathers into the query's partial buffer, zeroed by a fill on the stream,
// which k_accumulate_moments then adds into the radiance and sumsq buffers over the 3 n floats).  `who` names the
// entry point in the messages.
int trace_rays_query(kdpt_ctx* c, const float* origins, const float* directions, long long n, int first_iter,
                     int count, int flags, float* radiance, float* sumsq, bool moments, const std::string& who) {
  if (n < 0) return fail(KDPT_ERR_ARG, who + ": n must be >= 0");
  if (count < 0) return fail(KDPT_ERR_ARG, who + ": count must be >= 0");
  if (first_iter < 1) return fail(KDPT_ERR_ARG, who + ": first_iter must be >= 1");
  if (flags & ~KDPT_CAST_NORMALIZE) return fail(KDPT_ERR_ARG, who + ": unknown bit in flags");
  if (!c) return fail(KDPT_ERR_ARG, who + ": null ctx");
  if (n > (long long)c->npix)
    return fail(KDPT_ERR_ARG, who + ": n = " + std::to_string(n) + " exceeds the context's W * H = " +
                                  std::to_string(c->npix) + " paths (create a context of a larger resolution)");
  const bool work = n > 0 && count > 0;
  if (work && !origins) return fail(KDPT_ERR_ARG, who + ": null origins");
  if (work && !directions) return fail(KDPT_ERR_ARG, who + ": null directions");
  if (work && !radiance) return fail(KDPT_ERR_ARG, who + ": null radiance");
  if (work && moments && !sumsq) return fail(KDPT_ERR_ARG, who + ": null sumsq");
  if (!work) return KDPT_OK;
  if (c->shade_oob) return refuse_shading();
  int rc = kdpt_synchronize(c);  // everything queued on the context first
  if (rc || (rc = query_state(c))) return rc;
  const hipStream_t st = c->stream;
  RayQuery& Q = c->query;
  IterState* q = Q.state.get();
  const size_t m = (size_t)n, npix = (size_t)c->npix;
  if (moments) {
    if (!Q.partial) HIP_TRY(Q.partial.alloc(3 * npix));
    if (!Q.sumsq) HIP_TRY(Q.sumsq.alloc(3 * npix));
  }
  float* const image = Q.image.get();
  const float* const partial = Q.partial.get();
  int iter = first_iter;  // (the batch's one iteration number: the loop below moves it)
  // the call's gathers add into the radiance buffer or the partial one; its totals are the query's own
  BatchCall call{&q, &iter, 1, st, c->trace_grid,
                 Targets{moments ? Q.partial.get() : image, false, Q.totals.get(), Q.totals.get() + 1}};
  UserRays& rays = call.src.rays;
  call.src.kind = RaySource::USER_RAYS;
  rays = {origins, directions, (int)n, (flags & KDPT_CAST_NORMALIZE) ? 1 : 0};
  if ((rc = stage_in(on_context_device(c, origins), &rays.o, 3 * m, Q.stage.get(), st)) ||
      (rc = stage_in(on_context_device(c, directions), &rays.d, 3 * m, Q.stage.get() + 3 * npix, st)))
    return rc;
  HIP_TRY(hipEventRecord(q->ev0, st));
  // pixel i of the query's image is ray i: the gathers add into it in iteration order, from zero
  HIP_TRY(hipMemsetAsync(image, 0, sizeof(float) * 3 * m, st));
  HIP_TRY(hipMemsetAsync(Q.totals.get(), 0, sizeof(unsigned long long) * 4, st));
  if (moments) HIP_TRY(hipMemsetAsync(Q.sumsq.get(), 0, sizeof(float) * 3 * m, st));
  for (int k = 0; k < count; k++) {
    iter = first_iter + k;
    if (moments) HIP_TRY(hipMemsetAsync(Q.partial.get(), 0, sizeof(float) * 3 * m, st));
    if ((rc = launch_batch(c, call))) return rc;
    if (moments) {
      const int m3 = 3 * (int)n;
      hipLaunchKernelGGL(k_accumulate_moments, dim3((m3 + 255) / 256), dim3(256), 0, st, image, Q.sumsq.get(),
                         fill_parts<MomentParts>(&partial, 1), m3);
      HIP_TRY(hipGetLastError());
    }
  }
  if ((rc = stage_out(on_context_device(c, radiance), radiance, image, 3 * m, st))) return rc;
  if (moments && (rc = stage_out(on_context_device(c, sumsq), sumsq, Q.sumsq.get(), 3 * m, st)))
    return rc;
  HIP_TRY(hipEventRecord(q->ev1, st));
  unsigned long long totals[4] = {0, 0, 0, 0};
  HIP_TRY(hipMemcpyAsync(totals, Q.totals.get(), sizeof totals, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  float ms = 0;
  HIP_TRY(hipEventElapsedTime(&ms, q->ev0, q->ev1));
  c->query.ms = ms;
  c->query.segments = (long long)totals[0];
  c->query.traced = (long long)totals[3];
  return check_fault(q, st);
}

}  // namespace

int kdpt_trace_rays(kdpt_ctx* c, const float* origins, const float* directions, long long n, int first_iter,
                    int count, int flags, float* radiance) {
  return trace_rays_query(c, origins, directions, n, first_iter, count, flags, radiance, nullptr, false,
                          "kdpt_trace_rays");
}

int kdpt_trace_rays_moments(kdpt_ctx* c, const float* origins, const float* directions, long long n, int first_iter,
                            int count, int flags, float* radiance, float* sumsq) {
  return trace_rays_query(c, origins, directions, n, first_iter, count, flags, radiance, sumsq, true,
                          "kdpt_trace_rays_moments");
}

int kdpt_trace_rays_stats(kdpt_ctx* c, long long* segments, long long* traced, double* device_ms) {
  if (!c) return fail(KDPT_ERR_ARG, "kdpt_trace_rays_stats: null ctx");
  if (segments) *segments = c->query.segments;
  if (traced) *traced = c->query.traced;
  if (device_ms) *device_ms = c->query.ms;
  return KDPT_OK;
}
