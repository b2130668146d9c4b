// host_group.h -- the persistent in-process group of contexts (kdpt_group_*): spp-sharded frames, with or without
// second moments, and adaptive rounds across the ranks; kdpt_render_sharded is create, render, synchronize, destroy
// on top of it.
//
// A host section of kdpt_runtime.hip's translation unit, not a stand-alone header: kdpt_runtime.hip includes it
// after host_moments.h (it uses host_frames.h's frame helpers and host_moments.h's list builder).  Host code only:
// no kernel is defined here (the kernels_*.h sections hold them), and tests/test_stream_discipline.py and
// tests/test_resource_ownership.py read every host section.
#pragma once

// One context per rank, all in this process (include/kdpt.h "A persistent group").  Rank r queues its share of a
// frame on its own batch streams into its frame buffer (enqueue_frame); the ranks' reduce streams carry the
// exchange: RCCL's ncclReduce, or peer copies to rank 0's device, where one kernel adds the parts in rank order.
// With KDPT_GROUP_MOMENTS a frame buffer holds S then Q (frame_floats), one reduce moves both, and
// k_frame_moments finishes the frame on rank 0; an adaptive round reuses frame buffer 0 of every rank as its slot
// buffer (s then q, 3 |A| floats each) and k_adapt_slots finishes it.
//
// Ownership: the members go in reverse order of declaration -- the contexts first (kdpt_destroy drains a context's
// streams and releases its communicator), then the other ranks' list copies and totals, the copy reduce's staged
// parts, and last the events recorded across devices, each released on its device.
struct kdpt_group {
  struct XEvent {
    int dev;
    Event ev;
  };
  std::vector<XEvent> ev_idle, ev_live;  // cross-device events: live until kdpt_group_synchronize, then reused
  std::vector<DeviceBuf<float>> staged;  // copy reduce: the other ranks' parts on rank 0's device
  std::vector<DeviceBuf<int>> lists;     // an adaptive round's list on rank i's device (i > 0; made on first use)
  std::vector<DeviceBuf<unsigned long long>> totals;  // ... and the rank's round totals (Adaptive::totals' layout)
  std::vector<std::unique_ptr<kdpt_ctx, int (*)(kdpt_ctx*)>> cs;
  int reduce = KDPT_REDUCE_RCCL;
  bool moments = false;

  kdpt_group() = default;
  kdpt_group(const kdpt_group&) = delete;
  kdpt_group& operator=(const kdpt_group&) = delete;
  ~kdpt_group() {
    std::vector<int> devs;
    for (auto& c : cs) devs.push_back(c->device);
    while (!cs.empty()) cs.pop_back();
    for (size_t i = 0; i < devs.size(); i++) {
      if (hipSetDevice(devs[i]) != hipSuccess) continue;
      if (i < totals.size()) totals[i].reset();
      if (i < lists.size()) lists[i].reset();
    }
    if (!devs.empty() && hipSetDevice(devs[0]) == hipSuccess) staged.clear();
    for (auto* v : {&ev_live, &ev_idle})
      for (XEvent& x : *v)
        if (hipSetDevice(x.dev) == hipSuccess) x.ev.reset();
  }
};

namespace {

// An event of device `dev` recorded on st, kept by the group: an idle one of that device, or a new one.
int group_event(kdpt_group* g, int dev, hipStream_t st, hipEvent_t* e) {
  HIP_TRY(hipSetDevice(dev));
  kdpt_group::XEvent x{dev, Event()};
  auto it = std::find_if(g->ev_idle.begin(), g->ev_idle.end(), [dev](const kdpt_group::XEvent& v) { return v.dev == dev; });
  if (it != g->ev_idle.end()) {
    x = std::move(*it);
    g->ev_idle.erase(it);
  } else {
    HIP_TRY(x.ev.create_untimed());
  }
  *e = x.ev;
  g->ev_live.push_back(std::move(x));
  HIP_TRY(hipEventRecord(*e, st));
  return KDPT_OK;
}

// The exchange step of a frame or an adaptive round.  Every rank's reduce stream already waits for the rank's share
// in its frame buffer k (nfloats of it count).  RCCL: one grouped ncclReduce into rank 0's `sum`, the one part.
// Copy reduce: rank 0's reduce stream waits for every rank's share and copies the others' over (peer copies: xGMI
// between GPUs; also between two contexts of one device), the parts in rank order; the other ranks' reduce streams
// then wait for the copies, after which their buffer may be reused.
int gather_parts(kdpt_group* g, int k, size_t nfloats, FrameParts* parts) {
  const int ndev = (int)g->cs.size();
  kdpt_ctx* const c0 = g->cs[0].get();
  *parts = FrameParts{};
  if (g->reduce == KDPT_REDUCE_RCCL) {
    const Rccl* R = rccl();
    if (!R) return fail(KDPT_ERR_UNSUPPORTED, "librccl.so.1 not found");
    R->groupStart();
    ncclResult_t e = ncclSuccess;
    for (int i = 0; i < ndev && e == ncclSuccess; i++)
      e = R->reduce(g->cs[i]->frames.buf[k].get(), i == 0 ? c0->frames.sum.get() : nullptr, nfloats, ncclFloat32,
                    ncclSum, 0, (ncclComm_t)g->cs[i]->frames.comm, g->cs[i]->frames.reduce_stream);
    const ncclResult_t e2 = R->groupEnd();
    if (e != ncclSuccess || e2 != ncclSuccess)
      return fail(KDPT_ERR_HIP, std::string("rccl: ") + R->errorString(e != ncclSuccess ? e : e2));
    parts->n = 1;
    parts->p[0] = c0->frames.sum.get();
    return KDPT_OK;
  }
  int rc;
  parts->n = ndev;
  parts->p[0] = c0->frames.buf[k].get();
  for (int i = 1; i < ndev; i++) {
    kdpt_ctx* const ci = g->cs[i].get();
    hipEvent_t share_done;  // (recorded on the rank's reduce stream, which already waits for the share)
    if ((rc = group_event(g, ci->device, ci->frames.reduce_stream, &share_done))) return rc;
    HIP_TRY(hipSetDevice(c0->device));
    HIP_TRY(hipStreamWaitEvent(c0->frames.reduce_stream, share_done, 0));
    HIP_TRY(hipMemcpyPeerAsync(g->staged[i].get(), c0->device, ci->frames.buf[k].get(), ci->device,
                               sizeof(float) * nfloats, c0->frames.reduce_stream));
    parts->p[i] = g->staged[i].get();
  }
  if (ndev > 1) {
    hipEvent_t done;
    if ((rc = group_event(g, c0->device, c0->frames.reduce_stream, &done))) return rc;
    for (int i = 1; i < ndev; i++) {
      HIP_TRY(hipSetDevice(g->cs[i]->device));
      HIP_TRY(hipStreamWaitEvent(g->cs[i]->frames.reduce_stream, done, 0));
    }
  }
  HIP_TRY(hipSetDevice(c0->device));
  return KDPT_OK;
}

// After rank 0's finish of buffer k is queued: every rank's buffer k is consumed once its reduce stream gets here,
// and what reads rank 0's image next follows the finish (join_accum, through img_last).
int release_buffers(kdpt_group* g, int k) {
  for (auto& c : g->cs) {
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipEventRecord(c->frames.ev[k], c->frames.reduce_stream));
  }
  kdpt_ctx* const c0 = g->cs[0].get();
  c0->pipe.img_last = c0->frames.ev[k];
  HIP_TRY(hipSetDevice(c0->device));
  return KDPT_OK;
}

// What kdpt_group_active_pixels and kdpt_group_trace_adaptive refuse beyond their own arguments, before any device
// work: check_adaptive_args' list for a group (whose ranks are in a communicator by construction).
int check_group_adaptive(const kdpt_group* g, float floor, float threshold, const std::string& who) {
  if (!(std::isfinite(floor) && floor > 0.0f)) return fail(KDPT_ERR_ARG, who + ": floor must be finite and > 0");
  if (std::isnan(threshold)) return fail(KDPT_ERR_ARG, who + ": threshold is NaN");
  if (!g) return fail(KDPT_ERR_ARG, who + ": null group");
  if (!g->moments)
    return fail(KDPT_ERR_UNSUPPORTED, who + ": the group was created without KDPT_GROUP_MOMENTS");
  const long long samples = g->cs[0]->mom.samples;
  if (samples < 2)
    return fail(KDPT_ERR_ARG, who + ": " + std::to_string(samples) + " iteration(s) accumulated, a variance needs at least 2");
  return KDPT_OK;
}

}  // namespace

int kdpt_group_create(const kdpt_scene* scene, const kdpt_options* opt, int ndev, const int* devices, int reduce,
                      int flags, kdpt_group** out) {
  const std::string who = "kdpt_group_create";
  if (!out) return fail(KDPT_ERR_ARG, who + ": null out");
  *out = nullptr;
  if (!scene) return fail(KDPT_ERR_ARG, who + ": null scene");
  if (ndev < 1 || ndev > 8) return fail(KDPT_ERR_ARG, who + ": ndev must be 1 .. 8, not " + std::to_string(ndev));
  if (!devices) return fail(KDPT_ERR_ARG, who + ": null devices");
  if (reduce != KDPT_REDUCE_RCCL && reduce != KDPT_REDUCE_COPY)
    return fail(KDPT_ERR_ARG, who + ": reduce must be KDPT_REDUCE_RCCL or KDPT_REDUCE_COPY");
  if (flags & ~KDPT_GROUP_MOMENTS) return fail(KDPT_ERR_ARG, who + ": unknown flag bit");
  kdpt_options o;
  if (opt) o = *opt;
  else kdpt_default_options(&o);
  o.external_image = nullptr;
  std::unique_ptr<kdpt_group> g(new kdpt_group());  // (a failure below releases what has been made)
  g->reduce = reduce;
  g->moments = (flags & KDPT_GROUP_MOMENTS) != 0;
  g->staged.resize(ndev);
  g->lists.resize(ndev);
  g->totals.resize(ndev);
  int rc;
  // (the first kdpt_create reports every scene refusal, before any device work)
  for (int i = 0; i < ndev; i++) {
    kdpt_ctx* ci = nullptr;
    if ((rc = kdpt_create(scene, &o, devices[i], &ci))) return rc;
    g->cs.emplace_back(ci, kdpt_destroy);
    ci->frames.nranks = ndev;
    ci->frames.rank = i;
  }
  if (reduce == KDPT_REDUCE_RCCL) {
    const Rccl* R = rccl();
    if (!R) return fail(KDPT_ERR_UNSUPPORTED, "librccl.so.1 not found");
    std::vector<ncclComm_t> comms(ndev);
    const ncclResult_t e = R->commInitAll(comms.data(), ndev, devices);
    if (e != ncclSuccess) return fail(KDPT_ERR_HIP, std::string("rccl: ") + R->errorString(e));
    for (int i = 0; i < ndev; i++) {
      g->cs[i]->frames.comm = comms[i];
      g->cs[i]->frames.owns_comm = true;
    }
  }
  kdpt_ctx* const c0 = g->cs[0].get();
  HIP_TRY(hipSetDevice(c0->device));
  if (reduce == KDPT_REDUCE_COPY)
    for (int i = 1; i < ndev; i++)
      if (const hipError_t e = g->staged[i].alloc(frame_floats(c0, g->moments))) return hip_fail("hipMalloc", e);
  // rank 0 keeps sumsq, the sample counter and (from the first adaptive call on) extra
  if (g->moments && (rc = kdpt_set_moments(c0, 1))) return rc;
  *out = g.release();
  return KDPT_OK;
}

int kdpt_group_destroy(kdpt_group* g) {
  delete g;
  return KDPT_OK;
}

int kdpt_group_context(kdpt_group* g, int rank, kdpt_ctx** ctx) {
  if (!g) return fail(KDPT_ERR_ARG, "kdpt_group_context: null group");
  if (!ctx) return fail(KDPT_ERR_ARG, "kdpt_group_context: null ctx");
  if (rank < 0 || rank >= (int)g->cs.size())
    return fail(KDPT_ERR_ARG, "kdpt_group_context: rank " + std::to_string(rank) + " of " + std::to_string(g->cs.size()));
  *ctx = g->cs[rank].get();
  return KDPT_OK;
}

// Every rank is drained whatever the others report (a fault on one must not leave another's work queued); the first
// failure is the call's.  Rank 0's kdpt_synchronize releases the pinned `out`.
int kdpt_group_synchronize(kdpt_group* g) {
  if (!g) return fail(KDPT_ERR_ARG, "kdpt_group_synchronize: null group");
  int first = KDPT_OK;
  std::string msg;
  for (auto& c : g->cs) {
    const int rc = kdpt_synchronize(c.get());
    if (rc && !first) {
      first = rc;
      msg = kdpt_last_error();
    }
  }
  // (every stream that waited for or recorded them is drained)
  for (auto& x : g->ev_live) g->ev_idle.push_back(std::move(x));
  g->ev_live.clear();
  return first ? fail(first, msg) : KDPT_OK;
}

int kdpt_group_render_frames(kdpt_group* g, int first_frame, int frames, int spp, int pipeline, int batch, float* out) {
  if (!g) return fail(KDPT_ERR_ARG, "kdpt_group_render_frames: null group");
  if (first_frame < 0 || frames < 0 || spp < 1)
    return fail(KDPT_ERR_ARG, "kdpt_group_render_frames: first_frame and frames must be >= 0, spp >= 1");
  kdpt_ctx* const c0 = g->cs[0].get();
  const int n3 = 3 * c0->npix;
  int rc;
  HIP_TRY(hipSetDevice(c0->device));
  // a pageable host `out` pinned until kdpt_group_synchronize (rank 0's kdpt_synchronize)
  pin_host_out(c0, out, sizeof(float) * (size_t)n3 * (size_t)frames);
  for (int k = 0; k < frames; k++) {
    const int f = first_frame + k, kb = f & 1;
    // each rank queues its share on its batch streams; its reduce stream waits for the share (as in
    // kdpt_render_frames), so frame f + 1's adds never queue behind frame f's reduce
    for (auto& c : g->cs) {
      HIP_TRY(hipSetDevice(c->device));
      if ((rc = enqueue_frame(c.get(), f, spp, pipeline, batch, g->moments))) return rc;
      if ((rc = reduce_spin(c.get(), c->frames.reduce_stream))) return rc;
    }
    HIP_TRY(hipSetDevice(c0->device));
    FrameParts parts;
    if ((rc = gather_parts(g, kb, frame_floats(c0, g->moments), &parts))) return rc;
    const hipStream_t rs = c0->frames.reduce_stream;
    const bool copy = g->reduce == KDPT_REDUCE_COPY;
    if (g->moments) {
      // the frame sum, the image and sumsq in one pass; S_f alone goes out
      float* const frame = copy ? c0->frames.sum.get() : nullptr;
      hipLaunchKernelGGL(k_frame_moments, dim3((n3 + 255) / 256), dim3(256), 0, rs, c0->image, c0->mom.sumsq.get(),
                         frame, parts, n3);
      HIP_TRY(hipGetLastError());
      c0->accumulated = true;
      c0->mom.samples += spp;
      if (out)
        HIP_TRY(hipMemcpyAsync(out + (size_t)k * n3, c0->frames.sum.get(), sizeof(float) * n3, hipMemcpyDefault, rs));
    } else {
      if (copy) {
        hipLaunchKernelGGL(k_sum_frames, dim3((n3 + 255) / 256), dim3(256), 0, rs, c0->frames.sum.get(), parts, n3);
        HIP_TRY(hipGetLastError());
      }
      if ((rc = finish_frame(c0, c0->frames.sum.get(), out, k, rs))) return rc;
    }
    if ((rc = release_buffers(g, kb))) return rc;
  }
  return KDPT_OK;
}

int kdpt_render_sharded(const kdpt_scene* scene, const kdpt_options* opt, int ndev, const int* devices,
                        int first_frame, int frames, int spp, int pipeline, int batch, int reduce, float* out) {
  if (!scene || ndev < 1 || ndev > 8 || !devices || first_frame < 0 || frames < 0 || spp < 1 ||
      (reduce != KDPT_REDUCE_RCCL && reduce != KDPT_REDUCE_COPY))
    return fail(KDPT_ERR_ARG, "bad arguments");
  kdpt_group* made = nullptr;
  int rc = kdpt_group_create(scene, opt, ndev, devices, reduce, 0, &made);
  if (rc) return rc;
  std::unique_ptr<kdpt_group> g(made);  // (destroyed at every return)
  if ((rc = kdpt_group_render_frames(made, first_frame, frames, spp, pipeline, batch, out))) return rc;
  return kdpt_group_synchronize(made);
}

int kdpt_group_set_camera(kdpt_group* g, const kdpt_camera* camera) {
  if (!g) return fail(KDPT_ERR_ARG, "kdpt_group_set_camera: null group");
  // rank 0's checks are every rank's (one resolution): a refusal leaves all of them as they were
  for (auto& c : g->cs)
    if (int rc = kdpt_set_camera(c.get(), camera)) return rc;
  return KDPT_OK;
}

int kdpt_group_set_options(kdpt_group* g, const kdpt_options* opt) {
  if (!g) return fail(KDPT_ERR_ARG, "kdpt_group_set_options: null group");
  if (!opt) return fail(KDPT_ERR_ARG, "kdpt_group_set_options: null options");
  kdpt_options o = *opt;
  o.external_image = nullptr;  // (ignored, as at kdpt_group_create)
  // queued work keeps the options it was queued with; after this no rank's kdpt_set_options has anything to wait
  // for, and rank 0's checks are every rank's (one set of options): a refusal leaves all of them as they were
  int rc = kdpt_group_synchronize(g);
  if (rc) return rc;
  for (auto& c : g->cs)
    if ((rc = kdpt_set_options(c.get(), &o))) return rc;
  return KDPT_OK;
}

int kdpt_group_reset(kdpt_group* g) {
  if (!g) return fail(KDPT_ERR_ARG, "kdpt_group_reset: null group");
  int rc = kdpt_group_synchronize(g);
  if (rc) return rc;
  for (auto& c : g->cs)
    if ((rc = kdpt_reset(c.get()))) return rc;
  return KDPT_OK;
}

int kdpt_group_active_pixels(kdpt_group* g, float floor, float threshold, int* pixels, long long* n) {
  if (!n) return fail(KDPT_ERR_ARG, "kdpt_group_active_pixels: null n");
  int rc = check_group_adaptive(g, floor, threshold, "kdpt_group_active_pixels");
  if (rc) return rc;
  kdpt_ctx* const c0 = g->cs[0].get();
  int active = 0;
  if ((rc = kdpt_group_synchronize(g))) return rc;
  HIP_TRY(hipSetDevice(c0->device));
  if ((rc = build_active_list(c0, floor, threshold, &active))) return rc;
  *n = active;
  if (!pixels || !active) return KDPT_OK;
  if ((rc = stage_out(on_context_device(c0, pixels), pixels, (const int*)c0->mom.adapt.list.get(), (size_t)active,
                      c0->stream)))
    return rc;
  HIP_TRY(hipStreamSynchronize(c0->stream));
  return KDPT_OK;
}

int kdpt_group_trace_adaptive(kdpt_group* g, int first_iter, int count, int pipeline, int batch, float floor,
                              float threshold, kdpt_adaptive* out) {
  const std::string who = "kdpt_group_trace_adaptive";
  if (first_iter < 1) return fail(KDPT_ERR_ARG, who + ": first_iter must be >= 1");
  if (count < 0) return fail(KDPT_ERR_ARG, who + ": count must be >= 0");
  if (!out) return fail(KDPT_ERR_ARG, who + ": null out");
  int rc = check_group_adaptive(g, floor, threshold, who);
  if (rc) return rc;
  const int ndev = (int)g->cs.size();
  kdpt_ctx* const c0 = g->cs[0].get();
  if (c0->shade_oob) return refuse_shading();
  // everything queued on the group first: the list is built on rank 0 from the state before the call
  int active = 0;
  if ((rc = kdpt_group_synchronize(g))) return rc;
  HIP_TRY(hipSetDevice(c0->device));
  if ((rc = build_active_list(c0, floor, threshold, &active))) return rc;
  memset(out, 0, sizeof *out);
  out->pixels = c0->npix;
  out->active = active;
  if (!active || !count) return KDPT_OK;
  Adaptive& a = c0->mom.adapt;
  HIP_TRY(hipEventRecord(a.ev[0], c0->stream));
  // the list to every other rank's device (rank 0's stream is drained: the list is complete), on the rank's reduce
  // stream, which the rank's own stream then follows -- and with it the round's launches (enqueue_iterations' entry)
  const int* list[8];
  unsigned long long* totals[8];
  list[0] = a.list.get();
  totals[0] = a.totals.get();
  for (int i = 1; i < ndev; i++) {
    kdpt_ctx* const ci = g->cs[i].get();
    HIP_TRY(hipSetDevice(ci->device));
    if ((rc = frame_buffers(ci, g->moments))) return rc;
    if (!g->lists[i]) HIP_TRY(g->lists[i].alloc((size_t)ci->npix));
    if (!g->totals[i]) HIP_TRY(g->totals[i].alloc(4));
    list[i] = g->lists[i].get();
    totals[i] = g->totals[i].get();
    HIP_TRY(hipMemcpyPeerAsync(g->lists[i].get(), ci->device, a.list.get(), c0->device, sizeof(int) * (size_t)active,
                               ci->frames.reduce_stream));
    hipEvent_t copied;
    if ((rc = group_event(g, ci->device, ci->frames.reduce_stream, &copied))) return rc;
    HIP_TRY(hipStreamWaitEvent(ci->stream, copied, 0));
  }
  // iteration first_iter + k goes to rank k mod N; rank r accumulates its iterations in order into its slot buffer
  // (frame buffer 0: s, then q), zeroed first; a rank without an iteration contributes zeros
  const size_t slot_floats = 6 * (size_t)active;
  for (int i = 0; i < ndev; i++) {
    kdpt_ctx* const ci = g->cs[i].get();
    HIP_TRY(hipSetDevice(ci->device));
    if ((rc = frame_buffers(ci, g->moments))) return rc;
    float* const sb = ci->frames.buf[0].get();
    const int n = i < count ? (count - i + ndev - 1) / ndev : 0;
    if (n > 0) {
      HIP_TRY(hipMemsetAsync(totals[i], 0, sizeof(unsigned long long) * 4, ci->stream));
      const ActiveSet act{list[i], active, nullptr};
      IterationsCall call{first_iter + i, n, ndev, pipeline, batch, sb, ci->frames.ev[0], &act, totals[i]};
      call.sumsq = sb + 3 * (size_t)active;
      call.zero_floats = slot_floats;
      if ((rc = enqueue_iterations(ci, call))) return rc;
      HIP_TRY(hipStreamWaitEvent(ci->frames.reduce_stream, ci->pipe.acc_last, 0));
    } else {
      HIP_TRY(hipMemsetAsync(sb, 0, sizeof(float) * slot_floats, ci->frames.reduce_stream));
    }
  }
  // the slot buffers are reduced as frames are, and rank 0 adds the round through the list in one pass
  HIP_TRY(hipSetDevice(c0->device));
  FrameParts parts;
  if ((rc = gather_parts(g, 0, slot_floats, &parts))) return rc;
  hipLaunchKernelGGL(k_adapt_slots, dim3((active + 255) / 256), dim3(256), 0, c0->frames.reduce_stream, c0->image,
                     c0->mom.sumsq.get(), a.extra.get(), a.list.get(), active, parts, (uint32_t)count);
  HIP_TRY(hipGetLastError());
  c0->accumulated = true;
  if ((rc = release_buffers(g, 0))) return rc;
  if ((rc = join_accum(c0))) return rc;  // rank 0's stream after the round's add
  HIP_TRY(hipEventRecord(a.ev[1], c0->stream));
  // every rank's totals, after its last add
  unsigned long long got[8][4] = {};
  for (int i = 0; i < ndev && i < count; i++) {
    kdpt_ctx* const ci = g->cs[i].get();
    HIP_TRY(hipSetDevice(ci->device));
    if ((rc = join_accum(ci))) return rc;
    HIP_TRY(hipMemcpyAsync(got[i], totals[i], sizeof got[i], hipMemcpyDeviceToHost, ci->stream));
  }
  if ((rc = kdpt_group_synchronize(g))) return rc;  // (the groups' fault words too)
  float ms = 0;
  HIP_TRY(hipSetDevice(c0->device));
  HIP_TRY(hipEventElapsedTime(&ms, a.ev[0], a.ev[1]));
  out->pixel_samples = (long long)active * count;
  for (int i = 0; i < ndev; i++) {
    out->segments += (long long)got[i][0];
    out->traced += (long long)got[i][3];
  }
  out->device_ms = ms;
  return KDPT_OK;
}
