// host_pipeline.h -- one-at-a-time and pipelined iterations: kdpt_trace_iteration[_async], enqueue_iterations
// (kdpt_trace_iterations, a frame's share, an adaptive round), the add of partial images (launch_accumulate),
// kdpt_synchronize and kdpt_reset.
//
// A host section of kdpt_runtime.hip's translation unit, not a stand-alone header: kdpt_runtime.hip includes it
// after host_launch.h.  Host code only: no kernel is defined here (the kernels_*.h sections hold them), and
// tests/test_stream_discipline.py and tests/test_resource_ownership.py read every host section.
#pragma once

namespace {

// The pixels an adaptive round traces (its batches' source) and the add through them: `extra` counts the samples.
// extra null (a rank of kdpt_group_trace_adaptive): the add goes to a slot buffer, not through the list -- slot j's
// three floats at 3 j of the call's target and of its sumsq, for the group's reduce to carry to rank 0.
struct ActiveSet {
  const int* list;
  int n;
  uint32_t* extra;
};

// (PartialImages or MomentParts: the first nb of `partials`)
template <typename Parts>
Parts fill_parts(const float* const* partials, int nb) {
  Parts parts{};
  parts.nb = nb;
  for (int b = 0; b < nb; b++) parts.p[b] = partials[b];
  return parts;
}

// The add of nb partial images (iteration order) into `target` on stream st: k_accumulate_batch, or, with `sumsq`
// (the context keeps second moments and the target is its image), k_accumulate_moments, which adds the squares
// into it in the same pass.  With an active set the partial images hold list slots, not pixels:
// k_accumulate_adapt adds them through the list and counts the samples into `extra`; an active set without `extra`
// adds the 3 n slot floats in place (k_accumulate_moments over the slots).
int launch_accumulate(kdpt_ctx* c, float* target, float* sumsq, const float* const* partials, int nb, hipStream_t st,
                      const ActiveSet* act = nullptr) {
  const int n3 = 3 * (act ? act->n : c->npix);
  if (act && act->extra) {
    hipLaunchKernelGGL(k_accumulate_adapt, dim3((act->n + 255) / 256), dim3(256), 0, st, target, sumsq, act->extra,
                       act->list, act->n, fill_parts<AdaptParts>(partials, nb));
  } else if (sumsq) {
    hipLaunchKernelGGL(k_accumulate_moments, dim3((n3 + 255) / 256), dim3(256), 0, st, target, sumsq,
                       fill_parts<MomentParts>(partials, nb), n3);
  } else {
    hipLaunchKernelGGL(k_accumulate_batch, dim3((n3 + 255) / 256), dim3(256), 0, st, target,
                       fill_parts<PartialImages>(partials, nb), n3);
  }
  HIP_TRY(hipGetLastError());
  return KDPT_OK;
}

// Read back the intersect-kernel events of finished iterations (testing_mode).
int drain_intersect_events(kdpt_ctx* c) {
  for (auto& evs : c->pipe.pending_ev) {
    for (size_t k = 0; k + 1 < evs.size(); k += 2) {
      float ms = 0;
      HIP_TRY(hipEventSynchronize(evs[k + 1]));
      if (hipEventElapsedTime(&ms, evs[k], evs[k + 1]) == hipSuccess) {
        c->intersect_ms_total += ms;
        c->intersect_launches_total++;
      }
    }
    for (Event& e : evs) c->pipe.free_ev.push_back(std::move(e));
  }
  c->pipe.pending_ev.clear();
  return KDPT_OK;
}

// stats.segments / seg_per_bounce / bounces of the iteration whose counts are in the solo state's h_counts
int segments_from_counts(kdpt_ctx* c) {
  const int* h_counts = c->solo.h_counts.get();
  long long seg = 0;
  int bounces = 0;
  for (int d = 0; d < 32; d++) c->stats.seg_per_bounce[d] = 0;
  for (int d = 0; d < c->cap; d++) {
    const int nd = h_counts[d];
    if (d > 0 && h_counts[d] <= 0) break;  // the reference stops once num_paths <= 0
    seg += nd;
    if (d < 32) c->stats.seg_per_bounce[d] = nd;
    bounces = d + 1;
    if (c->opt.compaction && h_counts[d + 1] <= 0) break;
  }
  c->stats.segments = seg;
  c->stats.bounces = bounces;
  return bounces;
}

// kdpt_trace_iteration[_async]: one whole iteration of the solo state added to the image.  With moments off the
// state gathers straight into the image; with moments on into the context's partial image (mom_partial, which the
// camera kernel clears as it clears the pipeline states'), added to the image and to the second moments on the
// same stream at nb = 1.
int accumulate_iteration(kdpt_ctx* c, int iter) {
  int rc = launch_iteration(c, iter, solo_targets(c));
  if (rc) return rc;
  c->accumulated = true;
  if (!c->mom.on) return KDPT_OK;
  const float* partial = c->mom.partial.get();
  if ((rc = launch_accumulate(c, c->image, c->mom.sumsq.get(), &partial, 1, c->stream))) return rc;
  c->mom.samples++;
  return KDPT_OK;
}

// Iterations first_iter + k * stride (k < count) in batches of `batch`, `pipeline` batches in flight, their
// partial images added into `target` (the context's image, or a frame buffer of kdpt_render_frames) in
// iteration order; with `sumsq` (beside a target that is not the image: a frame buffer that carries second moments,
// a group's slot buffer) their squares into it in the same pass, as the image's moments get them.  Each batch's add runs on the batch's own stream, after the previous batch's add (the one
// cross-stream wait of the pipeline, normally satisfied by the time it is reached): no stream ever waits for a
// whole batch, so none holds an in-order hardware queue that batch streams share (HIP multiplexes a process's
// streams onto GPU_MAX_HW_QUEUES queues, 4 by default).  zero_after: the target is first zeroed, after that
// event (a frame buffer after its previous reduce), zero_floats of it (0: 3 W H; a target with its sumsq behind it in
// one allocation says how many).  Returns once everything is queued.
// act (kdpt_trace_adaptive): every batch starts from the active list instead of the camera's W*H rays and is added
// through it; the list was built on the context's stream, so each group's first launch of the call follows `entry`.
// The segment and intersect totals go to the round's own (`totals`, Adaptive::totals' layout), and kdpt_stats and
// the moments' counter do not move.
struct IterationsCall {
  int first_iter, count, stride, pipeline, batch;
  float* target;
  hipEvent_t zero_after = nullptr;
  const ActiveSet* act = nullptr;
  unsigned long long* totals = nullptr;  // with act
  float* sumsq = nullptr;                // the second target, beside a target that is not the image
  size_t zero_floats = 0;
};
int enqueue_iterations(kdpt_ctx* c, const IterationsCall& call) {
  if (c->shade_oob) return refuse_shading();
  const ActiveSet* const act = call.act;
  const bool into_image = call.target == c->image;
  const int depth = std::min(16, std::max(1, call.pipeline));
  const int B = std::min(MAXB, std::max(1, call.batch));
  // the first add follows everything already queued on the context's own stream (reset, ...); a wait of an
  // earlier call that is still queued keeps the record it was queued after
  const hipEvent_t entry = c->pipe.entry_ev;
  HIP_TRY(hipEventRecord(entry, c->stream));
  // `depth` groups of B iteration states; a group runs one batch at a time on its stream
  if ((int)c->pipe.groups.size() < depth || c->pipe.batch != B) {
    if (!c->pipe.groups.empty()) {
      int rc = kdpt_synchronize(c);
      if (rc) return rc;
      c->pipe.drop_groups();
    }
    c->pipe.batch = B;
    c->pipe.next = 0;
    // One stream per group, created one after another in group order: HIP maps streams onto its hardware
    // queues (GPU_MAX_HW_QUEUES) in creation order, reusing the least-used queue once all exist, so a stream per
    // iteration state (8 x 4) had put pairs of groups -- two batches' chains -- on one in-order queue.
    while ((int)c->pipe.groups.size() < depth) {
      int rc = make_group(c, B);
      if (rc) {
        c->pipe.drop_groups();
        return rc;
      }
    }
  }
  const int ngroups = (int)c->pipe.groups.size();
  // With several batches in flight each intersect launch gets a share of the chip (2/depth of the
  // persistent grid, all of it for depth <= 2, a quarter from depth 8 on): a launch's length is set by its
  // heaviest rays, so concurrent launches on disjoint CU subsets overlap those tails instead of queueing
  // behind them.  (Sweep with every batch on its own hardware queue: a quarter is best at depths 8-12.)
  const int trace_grid =
      c->grid_env ? c->trace_grid : std::max(1, c->trace_grid * 2 / std::min(8, std::max(2, depth)));
  if (!act) c->stats.intersect_grid_share = (float)trace_grid / (float)std::max(1, c->full_trace_grid);
  // every batch gathers into its states' own partial images; its totals are the context's or the round's
  Targets out = context_targets(c, nullptr, false);
  RaySource src{};
  if (act) {
    out.total_segments = call.totals;
    out.trace_total = call.totals + 1;
    src = {RaySource::PIXEL_LIST, act->list, act->n};
  }
  unsigned waited = 0;  // the groups whose stream has waited for `entry` in this call (an active set's)
  // diagnostic ("profile_batches" knob): the counting intersect kernel (kdpt_wave_profile after sync)
  if (c->profile_batches) HIP_TRY(hipMemsetAsync(c->counters, 0, sizeof(Counters), c->stream));
  bool first = true;
  for (int kb = 0; kb < call.count; kb += B) {
    const int nb = std::min(B, call.count - kb);
    // groups in turn, continuing across calls: kdpt_render_frames queues one call per frame, and a frame
    // shorter than the pipeline must not restart at group 0 (it would wait on that group's previous batch)
    const int g = c->pipe.next % ngroups;
    c->pipe.next = (g + 1) % ngroups;
    IterGroup& grp = c->pipe.groups[g];
    hipStream_t st = grp.stream;
    // (the group's previous batch's partial images were added on this stream, before this batch's camera rays
    // clear them)
    int iters[MAXB];
    IterState* its[MAXB];
    for (int b = 0; b < nb; b++) {
      iters[b] = call.first_iter + (kb + b) * call.stride;
      its[b] = grp.its[b].get();
    }
    std::vector<Event>* bev = nullptr;
    if (c->opt.testing_mode && !act) {
      std::vector<Event> evs;
      for (int e = 0; e < 2 * c->cap; e++) {
        Event ev;
        if (!c->pipe.free_ev.empty()) { ev = std::move(c->pipe.free_ev.back()); c->pipe.free_ev.pop_back(); }
        else HIP_TRY(ev.create());
        evs.push_back(std::move(ev));
      }
      c->pipe.pending_ev.push_back(std::move(evs));
      bev = &c->pipe.pending_ev.back();
    }
    if (act) {
      if (!(waited >> g & 1u)) HIP_TRY(hipStreamWaitEvent(st, entry, 0));
      waited |= 1u << g;
    }
    BatchCall bc{its, iters, nb, st, trace_grid, out, src};
    bc.count = c->profile_batches;
    bc.bev = bev;
    int rc = launch_batch(c, bc);
    if (rc) return rc;
    // the add: after the previous add (the chain), and for the call's first batch after the context's stream,
    // the frames' image adds (when the target is the image) and the target's zeroing
    if (c->pipe.acc_last) HIP_TRY(hipStreamWaitEvent(st, c->pipe.acc_last, 0));
    if (first) {
      HIP_TRY(hipStreamWaitEvent(st, entry, 0));
      if (c->pipe.img_last && into_image) HIP_TRY(hipStreamWaitEvent(st, c->pipe.img_last, 0));
      if (call.zero_after) {
        HIP_TRY(hipStreamWaitEvent(st, call.zero_after, 0));
        const size_t nz = call.zero_floats ? call.zero_floats : 3 * (size_t)c->npix;
        HIP_TRY(hipMemsetAsync(call.target, 0, sizeof(float) * nz, st));
      }
      first = false;
    }
    const float* partials[MAXB];
    for (int b = 0; b < nb; b++) partials[b] = its[b]->partial;  // in iteration order
    float* const sumsq = !into_image ? call.sumsq : c->mom.on ? c->mom.sumsq.get() : nullptr;
    if ((rc = launch_accumulate(c, call.target, sumsq, partials, nb, st, act))) return rc;
    HIP_TRY(hipEventRecord(grp.acc_ev, st));
    c->pipe.acc_last = grp.acc_ev;
    if (into_image) {
      c->accumulated = true;
      if (c->mom.on && !act) c->mom.samples += nb;
    }
  }
  if (!act) c->stats.iterations += call.count;
  return KDPT_OK;
}

}  // namespace

extern "C" {

int kdpt_reset(kdpt_ctx* c) {
  if (!c) return fail(KDPT_ERR_ARG, "null ctx");
  HIP_TRY(hipSetDevice(c->device));
  for (auto& grp : c->pipe.groups) HIP_TRY(hipStreamSynchronize(grp.stream));
  if (c->frames.reduce_stream) HIP_TRY(hipStreamSynchronize(c->frames.reduce_stream));
  drain_intersect_events(c);
  c->intersect_ms_total = 0;
  c->intersect_launches_total = 0;
  HIP_TRY(hipMemsetAsync(c->image, 0, sizeof(float) * 3 * (size_t)c->npix, c->stream));
  HIP_TRY(hipMemsetAsync(c->total_segments, 0, sizeof(unsigned long long), c->stream));
  HIP_TRY(hipMemsetAsync(c->trace_total, 0, 3 * sizeof(unsigned long long), c->stream));
  if (c->mom.on) HIP_TRY(hipMemsetAsync(c->mom.sumsq.get(), 0, sizeof(float) * 3 * (size_t)c->npix, c->stream));
  if (c->mom.adapt.extra)
    HIP_TRY(hipMemsetAsync(c->mom.adapt.extra.get(), 0, sizeof(uint32_t) * (size_t)c->npix, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  c->mom.samples = 0;
  c->accumulated = false;
  memset(&c->stats, 0, sizeof c->stats);
  c->stats.intersect_grid_share = 1.0f;
  c->cast.rays = c->cast.traced = 0;
  c->cast.ms = 0;
  return KDPT_OK;
}

int kdpt_trace_iteration_async(kdpt_ctx* c, int frame, int iter) {
  (void)frame;  // unused by the reference too
  if (!c) return fail(KDPT_ERR_ARG, "null ctx");
  return accumulate_iteration(c, iter);
}

int kdpt_synchronize(kdpt_ctx* c) {
  if (!c) return fail(KDPT_ERR_ARG, "null ctx");
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipStreamSynchronize(c->stream));
  for (auto& grp : c->pipe.groups) {
    HIP_TRY(hipStreamSynchronize(grp.stream));
    for (auto& it : grp.its) {
      int rc = check_fault(it.get(), grp.stream);
      if (rc) return rc;
    }
  }
  if (c->frames.reduce_stream) HIP_TRY(hipStreamSynchronize(c->frames.reduce_stream));
  c->frames.host_reg.clear();
  int rc = drain_intersect_events(c);
  if (rc) return rc;
  if (c->profile_batches) HIP_TRY(hipMemcpy(&c->last_profile, c->counters, sizeof(Counters), hipMemcpyDeviceToHost));
  return check_fault(&c->solo, c->stream);
}

int kdpt_trace_iteration(kdpt_ctx* c, int frame, int iter) {
  (void)frame;
  if (!c) return fail(KDPT_ERR_ARG, "null ctx");
  HIP_TRY(hipSetDevice(c->device));
  IterState& it = c->solo;
  HIP_TRY(hipEventRecord(it.ev0, c->stream));
  int rc = accumulate_iteration(c, iter);
  if (rc) return rc;
  HIP_TRY(hipEventRecord(it.ev1, c->stream));
  HIP_TRY(hipMemcpyAsync(it.h_counts.get(), it.counts, sizeof(int) * (c->cap + 3), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  if (it.h_counts.get()[c->cap + 2]) return fault_error(&it, c->stream, it.h_counts.get()[c->cap + 2]);
  float ms = 0;
  HIP_TRY(hipEventElapsedTime(&ms, it.ev0, it.ev1));
  c->stats.ms_last_iteration = ms;
  c->stats.iterations++;
  const int bounces = segments_from_counts(c);
  if (c->opt.testing_mode) {
    float tot = 0;
    for (int d = 0; d < bounces; d++) {
      float b = 0;
      if (hipEventElapsedTime(&b, it.bounce_ev[2 * d], it.bounce_ev[2 * d + 1]) == hipSuccess) tot += b;
    }
    c->stats.ms_intersect = tot;
    c->intersect_ms_total += tot;
    c->intersect_launches_total += bounces;
  }
  return KDPT_OK;
}

int kdpt_trace_iterations(kdpt_ctx* c, int frame, int first_iter, int count, int stride, int pipeline, int batch) {
  (void)frame;
  if (!c || count < 0 || first_iter < 1 || stride < 1) return fail(KDPT_ERR_ARG, "bad arguments");
  HIP_TRY(hipSetDevice(c->device));
  return enqueue_iterations(c, {first_iter, count, stride, pipeline, batch, c->image});
}

}  // extern "C"
