// host_context.h -- the context and its parts (an iteration's working set, the pipeline's groups, each
// feature's own state), alloc_iter / make_group, and the helpers every feature shares: streams, arena
// allocation, join_accum, caller-memory staging (on_context_device, stage_in, stage_out) and the fault word.
//
// A host section of kdpt_runtime.hip's translation unit, not a stand-alone header: kdpt_runtime.hip includes it
// after the kernel sections.  Host code only: no kernel is defined here (the kernels_*.h sections hold them), and
// tests/test_stream_discipline.py and tests/test_resource_ownership.py read every host section.
#pragma once

namespace {

double g_reduce_spin_us = 0;  // kdpt_set_tuning(NULL, "reduce_spin_us", v): the default of new contexts
double g_cluster_chord = -1;   // kdpt_set_tuning(NULL, "cluster_chord", v): big-leaf grouping of new contexts
bool g_cu_mask_streams = true;  // kdpt_set_tuning(NULL, "cu_mask_streams", v): ... and their stream kind

}  // namespace

// A group's ray queue (TraceArgs): the candidate list, its rays and the hit records of all the group's iterations,
// B x npix entries each, and one candidate counter per bounce.  The group's first state owns the memory, and the
// counters are that state's (inside its `counts` allocation, zeroed by its camera-ray launch like the group's work
// counters): every batch of the group, a partial one too, starts at the first state.
struct RayQueue {
  int2* hits0 = nullptr;   // [B npix] hit code + objMaterialIdx from the intersect kernel; iteration b's at b npix
  float4* cray = nullptr;  // [2 B npix] the candidates' rays in queue order (k_geoms / shading -> k_trace)
  int* cand = nullptr;     // [B npix] hits0 entries of the rays that meet the KD root box (k_geoms / shading -> k_trace)
  int* ccount = nullptr;   // [cap] candidates per bounce
  int* ccount0 = nullptr;  // [2] bounce-0 candidate counters of k_gen_geoms_b (alternating uses)
  int gen_parity = 0;      // which of them the next use counts into
  int* cc0_cur = nullptr;  // this use's (bounce 0 reads it instead of ccount[0])
  int* cc0_next = nullptr; // the next use's (this use's launch zeroes it)
  // A batch's camera stage takes this use's bounce-0 counter and hands the other one over for zeroing.
  void begin_use() {
    cc0_cur = ccount0 + gen_parity;
    gen_parity ^= 1;
    cc0_next = ccount0 + gen_parity;
  }
  // The candidate counter of bounce `depth`: k_gen_geoms_b counted bounce 0 into cc0_cur.
  int* count_at(int depth, bool gen_geoms) const { return (depth == 0 && gen_geoms) ? cc0_cur : ccount + depth; }
};

// One iteration's working set (alloc_iter).  The context has one for the one-at-a-time entry points
// (a group of one) and B per pipeline group; everything an iteration shares with the others (scene, options,
// knobs, counters) stays in the context.  A state does not move or copy (its arena does not): `q` of every state
// of a group points into the first state's own_queue, so states live in place (in the context, or behind a
// unique_ptr).
struct IterState {
  Arena allocs;  // the device memory below
  PathBuf buf[2]{};
  int cur = 0;
  int* counts = nullptr;  // [cap + 2] live paths per bounce, [1] fault word, then [cap] work counters, ...
  int* fault = nullptr;
  int* work = nullptr;
  int* tickets = nullptr;   // [cap] k_shade_fused's tile tickets
  RayQueue own_queue;       // the group's queue, in its first state
  RayQueue* q = nullptr;    // the group's queue (the first state's own_queue)
  int qbase = 0;            // this state's place in the group x npix: queue entry = qbase + path
  int2* hits = nullptr;     // [npix] this iteration's hit records: q->hits0 + qbase
  int2* prep = nullptr;     // [npix] next bounce's geoms record + walk flag (k_shade -> k_scatter)
  int* tile_counts = nullptr;
  int* tile_off = nullptr;
  unsigned long long* lb = nullptr;       // [cap][ntiles] k_shade_fused's look-back records
  unsigned long long* trace_t = nullptr;  // per-bounce intersect launch record
  PinnedBuf<int> h_counts;
  Event ev0, ev1;
  std::vector<Event> bounce_ev;
  // a pipeline state's own partial image (alloc_iter; null in every other state).  Where an iteration's light and
  // totals go is the call's to say (Targets), not the state's.
  float* partial = nullptr;

  // The state's part of each launch's arguments (launch_batch's stages).  zero_image: the image the camera stage
  // zeroes for this iteration (null: none).
  GenIter gen_iter(int iter, float* zero_image) const { return {iter, buf[0], counts, work, trace_t, lb, zero_image}; }
  // (after the queue's begin_use of this batch)
  GenGeomsIter gen_geoms_iter() const { return {q->cc0_cur, q->cc0_next, q->cray, hits, q->cand, qbase}; }
  GeomsIter geoms_iter() const { return {buf[cur], counts, q->cray, hits, q->cand, q->ccount, qbase}; }
  // (compaction goes into the other path buffer)
  FuseArgs fuse_args() const { return {buf[cur ^ 1], tickets, lb, counts, q->ccount, q->cray, hits, q->cand, qbase}; }
  ScatterPrep scatter_prep(bool on, int depth) const {
    return {on ? 1 : 0, prep, q->cray, hits, q->cand, q->ccount + depth + 1, qbase};
  }
};

// A pipeline group: `batch` iterations at a time in lockstep on the group's own stream; acc_ev: its last
// batch's add into the target done.
// Ownership (DESIGN.md "Ownership"): members are released in reverse order of declaration, here and in kdpt_ctx,
// so an owner's stream is declared first and goes after the buffers and events used on it; a group's states go
// last first, because state 0 owns the slabs the others view.
struct IterGroup {
  Stream stream;
  Event acc_ev;
  std::vector<std::unique_ptr<IterState>> its;
  IterGroup() = default;
  IterGroup(IterGroup&&) = default;
  ~IterGroup() {
    while (!its.empty()) its.pop_back();
  }
};

// The exact one-level cull's direction masks (kdpt_clusters.h build_dir_masks), built when the scene's rigorous
// margin is above the cap; S.cl_mask points at them unless a knob chose another cull.  A rebuild swaps `dev`.
struct MaskTables {
  DeviceBuf<unsigned long long> dev;
  DeviceBuf<float4> tn;  // the clusters' per-entry normal records (DevScene::cl_tn)
  int n = 0;
  std::unique_ptr<ClusterSet> cs;  // the clusters the masks were built from ("cull_mask_n" rebuilds)
  double build_ms = 0;             // kdpt_stats
};

// enable_kd = 0: the brute-force intersect kernel's view of the OBJ triangles in file order (the context's arena)
struct BruteScene {
  const BruteShape* shapes = nullptr;
  int num_shapes = 0;
  const float4* chunk_lo = nullptr;  // boxes of 64 file-order triangles
  const float4* chunk_hi = nullptr;
  float chunk_k_min = 0.0f;    // the smallest of the chunks' own cull coefficients (chunk_lo[j].w)
};

// Pipelined iterations (kdpt_trace_iterations): groups of `batch` iteration states, each state with a partial
// image of its own; the partial images are added into `image` in iteration order, each batch's add on its
// group's stream after the previous batch's add (acc_ev / acc_last: the chain).
struct Pipeline {
  Event entry_ev;  // enqueue_iterations: what the context's own stream held when the call began
  std::vector<IterGroup> groups;
  int batch = 1;
  int next = 0;                   // the group the next batch goes to
  hipEvent_t acc_last = nullptr;  // the most recent add (a group's acc_ev): the next add follows it
  hipEvent_t img_last = nullptr;  // the most recent frame reduce + image add (one of ShardedFrames::ev)
  // intersect-kernel timing (testing_mode) of every iteration, read back at synchronisation: a pool
  std::vector<std::vector<Event>> pending_ev;  // per launched iteration: 2 events per bounce
  std::vector<Event> free_ev;
  // Drop the groups (their streams drained here), last first.
  void drop_groups() {
    for (; !groups.empty(); groups.pop_back())
      if (groups.back().stream) (void)hipStreamSynchronize(groups.back().stream.get());
    acc_last = nullptr;
  }
};

// spp-sharded frames (kdpt_comm_init / kdpt_render_frames / kdpt_render_sharded): this context's rank, the
// RCCL communicator (null: one rank, or the in-process copy reduce of kdpt_render_sharded), two frame
// buffers (frame f accumulates into buf[f & 1] while f - 1 is reduced) and rank 0's reduced frame
struct ShardedFrames {
  int nranks = 1, rank = 0;
  void* comm = nullptr;  // ncclComm_t (release_comm)
  bool owns_comm = false;
  bool external_reduce = false;  // kdpt_comm_init without an id: each rank hands its frame shares out
  Stream reduce_stream;          // the frames' reduces and image adds, beside the accumulation stream
  DeviceBuf<float> buf[2], sum;
  Event ev[2];                   // buf[k] consumed by its reduce
  double reduce_spin_us = 0;     // "reduce_spin_us" knob: a device spin before every frame's reduce (a slow peer)
  HostRegistrations host_reg;    // pageable host `out` ranges pinned for kdpt_render_frames (until synchronize)
};

// Ray queries (kdpt_cast_rays): buffers of one chunk, made on first use and remade when "cast_chunk" changes --
// the input and output staging buffers (host arrays go through them), the query's own candidate queue, hit
// records and counters (CastArgs); nothing here is shared with the render path.  `b = {}` drops the buffers.
struct CastQuery {
  int chunk = 1 << 20;  // "cast_chunk" knob: rays per chunk
  struct Buffers {
    int alloc = 0;                    // the chunk size the buffers were made for (0: none)
    DeviceBuf<float> in;              // [6 chunk] origins, then directions
    DeviceBuf<kdpt_ray_hit> out;      // [chunk]
    DeviceBuf<float4> cray;           // [2 chunk]
    DeviceBuf<int> cand;              // [chunk]
    DeviceBuf<int2> hits;             // [chunk]
    DeviceBuf<int> cnt;               // [2]
    DeviceBuf<unsigned long long> tt; // [3]
  } b;
  Event ev[2];
  long long rays = 0, traced = 0;  // since create/reset (kdpt_cast_stats)
  double ms = 0;                   // the last call's device time
};

// Path-traced ray queries (kdpt_trace_rays, kdpt_camera_rays): an iteration state of their own, made on first
// use (query_state) -- its batches gather into the query's radiance buffer, their segment and intersect totals go to
// `totals` instead of the context's -- and a staging buffer for host arrays; kdpt_trace_rays_moments' partial buffer (each
// iteration gathers into it, zeroed by a fill) and second moments.  Nothing is shared with the render path.
struct RayQuery {
  std::unique_ptr<IterState> state;
  DeviceBuf<float> image;   // [3 npix]
  DeviceBuf<float> stage;   // [6 npix] origins, then directions (inputs of host callers, camera rays on their way out)
  DeviceBuf<unsigned long long> totals;  // [0] ShadeArgs::total_segments, [1..3] trace_total / trace_rays
  DeviceBuf<float> partial, sumsq;       // [3 npix] each
  long long segments = 0, traced = 0;  // of the last kdpt_trace_rays (kdpt_trace_rays_stats)
  double ms = 0;                       // ... and its device time
};

// Adaptive sampling (kdpt_trace_adaptive, kdpt_active_pixels): the per-pixel count of samples added beyond the
// uniform ones, the active list and the list kernels' buffers, the call's own segment and intersect totals (a ray
// query's layout) and its events.  Made by the first adaptive call (adaptive_state); part of the moments, so they
// go with them.  extra is the state: null means every pixel has Moments::samples samples.
struct Adaptive {
  DeviceBuf<uint32_t> extra;               // [npix]
  DeviceBuf<int> list;                     // [npix] the active pixels, ascending
  DeviceBuf<unsigned long long> masks;     // [4 workgroups] k_adapt_flags' ballots
  DeviceBuf<int> blocks;                   // [workgroups] counts, [workgroups] offsets, then |A|
  DeviceBuf<unsigned long long> totals;    // [0] ShadeArgs::total_segments, [1..3] trace_total / trace_rays
  Event ev[2];
};

// Per-pixel second moments (kdpt_set_moments): sumsq beside the image, the partial image the solo state gathers
// into while they are on (added with k_accumulate_moments at nb = 1), the number of iterations added since both
// were zeroed, and kdpt_noise_map's / kdpt_noise_estimate's buffers.  All null / 0 while moments are off.
struct Moments {
  bool on = false;
  DeviceBuf<float> sumsq, partial;  // [3 npix]
  long long samples = 0;
  DeviceBuf<float> noise_stage;         // [npix] kdpt_noise_map into host memory
  DeviceBuf<NoisePartial> noise_parts;  // [workgroups + 1] k_noise_partials' partials, then k_noise_final's result
  Adaptive adapt;
};

// Denoising (kdpt_denoise): the filter's records and the guide pass's working set -- the pinhole rays, a ray query's
// queue, hit records and counters (CastArgs' layout, one chunk of W*H rays) and its results -- made on first use
// (denoise_buffers) and dropped by kdpt_set_tuning; nothing here is shared with the render path, kdpt_cast_rays or
// kdpt_trace_rays.  `b = {}` drops the buffers.
struct Denoiser {
  struct Buffers {
    int npix = 0;                      // the pixel count the buffers were made for (0: none)
    DeviceBuf<float4> g0, g1;          // [npix] {normal, depth}, {point, id}
    DeviceBuf<float4> cv[2];           // [npix] {colour, variance}, ping-pong
    DeviceBuf<float> rays;             // [6 npix] origins, then directions
    DeviceBuf<kdpt_ray_hit> hits_out;  // [npix]
    DeviceBuf<float4> cray;            // [2 npix]
    DeviceBuf<int> cand;               // [npix]
    DeviceBuf<int2> hits;              // [npix]
    DeviceBuf<int> cnt;                // [2]
    DeviceBuf<unsigned long long> tt;  // [3]
    DeviceBuf<float> out_stage;        // [4 npix] colour, then variance, on their way to host memory
  } b;
  Event ev[3];                         // before the guides, between guides and filter, after the filter
  double guide_ms = 0, filter_ms = 0;  // the last call's (kdpt_denoise_stats)
};

// Temporal accumulation (kdpt_denoise_temporal): two frames in the denoiser's record layout plus a length per pixel
// -- set[cur] is the history (the guides, C', V' and L' of the last call, with the camera they were made under),
// set[cur ^ 1] the frame the next call builds, so that storing the new history is `cur ^= 1` and not a copy.
// Made on first use (temporal_sets), dropped by kdpt_temporal_reset and, with the denoiser's buffers, by
// kdpt_set_tuning.  `s = {}` drops the sets and the history with them.
struct Temporal {
  struct Set {
    DeviceBuf<float4> g0, g1, cv;  // [npix]
    DeviceBuf<float> len;          // [npix]
  };
  struct Sets {
    int npix = 0;      // the pixel count the sets were made for (0: none)
    Set set[2];
    DeviceBuf<unsigned int> counts;  // [2] valid pixels, of which with history
    int cur = 0;
    bool have = false;  // set[cur] holds a history
    kdpt_camera cam{};  // ... made under this camera
  } s;
  Event ev[4];  // before the guides, before the temporal stage, before the filter, after it
  double guide_ms = 0, temporal_ms = 0, filter_ms = 0;  // the last call's (kdpt_temporal_stats)
  long long valid = 0, with_history = 0;
};

struct kdpt_ctx {
  int device = 0;
  Stream stream;  // (declared before every other resource: destroyed last)
  kdpt_options opt{};
  kdpt_camera cam{};
  int traceDepth = 0;
  int W = 0, H = 0, npix = 0, ntiles = 0, nkeys = 1;
  int cap = 8;
  DevScene S{};
  Arena allocs;  // what lives as long as the context: the scene's uploads, the image, the counters
  DeviceBuf<uchar4> pbo_staging;  // kdpt_write_pbo into host memory
  IterState solo;         // kdpt_trace_iteration[_async], kdpt_debug_paths, kdpt_count_iteration; into `image`
  float* image = nullptr;  // in `allocs`, or the caller's (options.external_image: not owned)
  int tree_mode = 0;      // TreeMode
  int trace_grid = 0;     // persistent intersect workgroups (a pipelined call's launches take a share of them)
  int full_trace_grid = 0;  // the occupancy-derived grid (trace_grid before a "trace_grid_frac" knob)
  bool grid_env = false;  // trace_grid fixed by the "trace_grid_frac" tuning knob
  bool force_global_tree = false;  // "tree_global" tuning knob: keep the tree in HBM/L2
  // A triangle of shape m > 0: the KD traversal reports material mtlIdx + material_size - 1 for it
  // (src/pathtrace.cu:1142, :1205, :991), an index past the reference's own materials array, which its shading
  // then reads (and iteration 2's sort uses as a key).  There is nothing to reproduce: iterations are refused
  // (launch_batch); kdpt_cast_rays only reports the number and stays available.
  bool shade_oob = false;
  bool super_cull = true;          // "super_cull" tuning knob: 0 = no TREE_LDS16S route (one-level cull)
  CullMargin cull{};                // the scene's cluster-cull margins (kdpt_clusters.h cluster_margin)
  MaskTables masks;
  bool cull_exact = true;   // "cull_exact" knob: 0 = the fast-margin cull (not exact for such scenes)
  double create_ms = 0;     // kdpt_create's host wall time (kdpt_stats)
  bool cu_mask_streams = false;  // batch and reduce streams created with an all-CU mask (create_stream)
  bool cull_scene = true;   // false after "cluster_cull" = 0 or a fixed "cull_margin"
  int tree_format = 0;            // "tree_format" knob: 16 / 32 = LDS node records of that size only
  size_t tree_lds = 0;    // dynamic LDS bytes of the intersect kernel (TREE_LDS)
  bool no_fuse = false;         // "shade_fused" = 0: k_shade + k_scan + k_scatter instead of k_shade_fused
  bool shade_batch = true;      // "shade_batch": a batch's fused shading in one launch (k_shade_fused_b)
  bool gen_geoms = true;        // "gen_geoms": camera rays + bounce-0 k_geoms in one launch (k_gen_geoms_b)
  int chunk_width[3] = {16, 64, 64};
  Counters* counters = nullptr;
  Counters last_profile{};
  unsigned long long* total_segments = nullptr;  // device running total (async use)
  unsigned long long* trace_total = nullptr;     // [3] device-clock intersect ticks, launches, rays (shared)
  double wall_khz = 100000.0;                    // s_memrealtime frequency
  kdpt_stats stats{};
  bool sync_debug = false;  // "sync_debug" = 1: synchronise and log after every launch
  bool profile_batches = false;
  bool profile_steps = false;  // "profile_batches" = 2
  double intersect_ms_total = 0;
  long long intersect_launches_total = 0;
  bool brute = false;  // enable_kd = 0: brute-force intersect kernel over the OBJ triangles in file order
  bool viz = false;    // viz_kd: the KD node boxes drawn as boxes (k_viz)
  BruteScene bf;
  Pipeline pipe;
  ShardedFrames frames;
  CastQuery cast;
  RayQuery query;
  Moments mom;
  Denoiser den;
  Temporal tmp;
  // an iteration (or a frame) has been added into the image since create / kdpt_reset: with stats.iterations what
  // kdpt_set_moments(1) refuses on (kdpt_trace_iteration_async counts no iteration)
  bool accumulated = false;
};

namespace {

// kdpt_ctx::shade_oob: every entry point that shades ends here before it queues anything.
int refuse_shading() {
  return fail(KDPT_ERR_UNSUPPORTED,
              "the OBJ has triangles of a shape other than the first: their hits carry material mtlIdx + "
              "num_materials - 1, past the materials array (as in the reference), so the scene cannot be shaded; "
              "kdpt_cast_rays and enable_kd = 0 remain available");
}

// A context's streams (its own, the batch groups' and the frame reduce's): created with a mask of every CU, which
// gives each a hardware queue of its own instead of one of the GPU_MAX_HW_QUEUES (4 by default) in-order queues
// HIP multiplexes a process's plain streams onto -- where a waiting or long-running command of one stream holds
// the others on its queue.  C4's 32-spp frames: 6.49 -> 5.68 ms with 24 queues, and a 5 ms reduce delay per frame
// costs nothing at 4 or 24 queues (profiles/r06_ab_log.md).  Knob "cu_mask_streams" = 0 (process default):
// plain non-blocking streams; a failed creation falls back to one.
int create_stream(kdpt_ctx* c, Stream* st) {
  int cus = 0;
  if (c->cu_mask_streams) {
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, c->device));
    cus = std::max(1, prop.multiProcessorCount);
  }
  HIP_TRY(st->create(cus));
  return KDPT_OK;
}

// n elements in the arena of a context or an iteration state
template <typename Owner, typename T>
int dalloc(Owner* c, T** p, size_t n) {
  if (const hipError_t e = c->allocs.alloc(p, n)) return hip_fail("hipMalloc", e);
  return KDPT_OK;
}

// A prepared array into the context's arena, and the field (of DevScene, or a view of the context's) pointed at it.
template <typename T>
int dupload(kdpt_ctx* c, const T** field, const std::vector<T>& v) {
  T* d = nullptr;
  if (const hipError_t e = c->allocs.alloc(&d, v.size())) return hip_fail("hipMalloc", e);
  if (!v.empty()) HIP_TRY(hipMemcpy(d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
  *field = d;
  return KDPT_OK;
}

// Work queued on the context's own stream that reads or writes `image` must follow the pipelined
// accumulation (kdpt_trace_iterations adds partial images on the batch streams without a host sync) and the
// frames' image adds (kdpt_render_frames, on the reduce stream).
int join_accum(kdpt_ctx* c) {
  if (c->pipe.acc_last) HIP_TRY(hipStreamWaitEvent(c->stream, c->pipe.acc_last, 0));
  if (c->pipe.img_last) HIP_TRY(hipStreamWaitEvent(c->stream, c->pipe.img_last, 0));
  return KDPT_OK;
}

// Is p memory of the context's device?  (What a caller hands in may be host memory or another device's.)
bool on_context_device(const kdpt_ctx* c, const void* p) {
  hipPointerAttribute_t attr{};
  const bool dev = hipPointerGetAttributes(&attr, p) == hipSuccess && attr.type == hipMemoryTypeDevice &&
                   attr.device == c->device;
  (void)hipGetLastError();  // a plain host pointer is an error for hipPointerGetAttributes on some runtimes
  return dev;
}

// A caller's array on its way to the kernels and back.  Memory of the context's device (dev: on_context_device) is
// read and written where it is; anything else goes through a staging buffer of the context's and a copy on st.
template <typename T>
int stage_in(bool dev, const T** src, size_t n, T* stage, hipStream_t st) {
  if (dev) return KDPT_OK;
  HIP_TRY(hipMemcpyAsync(stage, *src, n * sizeof(T), hipMemcpyHostToDevice, st));
  *src = stage;
  return KDPT_OK;
}
// An output: the n elements the kernels left at `from` to the caller's dst (nothing to do when they wrote dst).
template <typename T>
int stage_out(bool dev, T* dst, const T* from, size_t n, hipStream_t st) {
  if (from == dst) return KDPT_OK;
  HIP_TRY(hipMemcpyAsync(dst, from, n * sizeof(T), dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, st));
  return KDPT_OK;
}

// A ray that needs more node steps than any valid tree allows sets the fault word and stops;
// the iteration then reports an error instead of returning a silently wrong image.
int fault_error(IterState* it, hipStream_t st, int code) {  // st: the (drained) stream the state runs on
  (void)hipMemsetAsync(it->fault, 0, sizeof(int), st);
  (void)hipStreamSynchronize(st);
  if (code & 32)
    return fail(KDPT_ERR_HIP, "shading: a path's survival differed from its hit record's prediction, code " +
                                  std::to_string(code));
  return fail(KDPT_ERR_HIP, "KD traversal exceeded its step bound (inconsistent tree), code " + std::to_string(code));
}

int check_fault(IterState* it, hipStream_t st) {
  int f = 0;
  HIP_TRY(hipMemcpy(&f, it->fault, sizeof(int), hipMemcpyDeviceToHost));
  return f ? fault_error(it, st, f) : KDPT_OK;
}

// Per-iteration device state: two path buffers, tile counts/offsets, live counts + fault word + work counters, and
// the events; and in a group's first state (head null: `it` is state 0 of a group of B) the group's ray queue and
// hit records, of which state b of the group (head: the first state) takes its view.  (The scene, image and
// counters live elsewhere.)
// The zero fills go on the stream st the state will run on and are waited for: every kernel of the context runs
// on a non-blocking stream, which does not order itself after the null stream, so a plain hipMemset there could
// land after the first iteration's camera-ray kernel had set its path count (that iteration would vanish).
// partial: with a partial image of its own (a pipeline state).
// A failed allocation leaves what was made in the state, for the caller to drop with it.
int alloc_iter(kdpt_ctx* c, IterState* it, hipStream_t st, bool partial, IterState* head = nullptr, int b = 0,
               int B = 1) {
  int rc;
  const size_t npix = (size_t)c->npix, ntiles = (size_t)c->ntiles, cap = (size_t)c->cap;
  for (int b = 0; b < 2; b++) {
    if ((rc = dalloc(it, &it->buf[b].p0, npix)) || (rc = dalloc(it, &it->buf[b].p1, npix)) ||
        (rc = dalloc(it, &it->buf[b].p2, npix)) || (rc = dalloc(it, &it->buf[b].pm, npix)))
      return rc;
    HIP_TRY(hipMemsetAsync(it->buf[b].pm, 0, sizeof(int) * npix, st));
  }
  // counts[0..cap+1]: live paths per bounce (rewritten every iteration); counts[cap+2]: fault flag;
  // counts[cap+3 ..]: work counters of the persistent intersect kernel
  if ((rc = dalloc(it, &it->trace_t, 4 * cap))) return rc;
  HIP_TRY(hipMemsetAsync(it->trace_t, 0, sizeof(unsigned long long) * 4 * cap, st));
  if ((rc = dalloc(it, &it->counts, 4 * cap + 5)) || (rc = dalloc(it, &it->lb, cap * ntiles)) ||
      (rc = dalloc(it, &it->prep, npix)) || (rc = dalloc(it, &it->tile_counts, (size_t)MAX_KEYS * ntiles)) ||
      (rc = dalloc(it, &it->tile_off, (size_t)MAX_KEYS * ntiles)))
    return rc;
  if (!head) {  // (B npix < 2^31: prepare_scene's shape check)
    RayQueue& q = it->own_queue;
    if ((rc = dalloc(it, &q.hits0, B * npix)) || (rc = dalloc(it, &q.cand, B * npix)) ||
        (rc = dalloc(it, &q.cray, 2 * B * npix)))
      return rc;
  }
  HIP_TRY(it->h_counts.alloc(cap + 3));
  HIP_TRY(hipMemsetAsync(it->counts, 0, sizeof(int) * (4 * cap + 5), st));
  HIP_TRY(hipMemsetAsync(it->lb, 0, sizeof(unsigned long long) * cap * ntiles, st));
  HIP_TRY(hipStreamSynchronize(st));
  it->fault = it->counts + cap + 2;
  it->work = it->counts + cap + 3;
  it->tickets = it->work + 2 * cap;
  if (!head) {  // the group's candidate counters: after the work counters, and after the tickets (2 entries, zero)
    it->own_queue.ccount = it->work + cap;
    it->own_queue.ccount0 = it->tickets + cap;
  }
  it->q = head ? head->q : &it->own_queue;
  it->qbase = b * c->npix;
  it->hits = it->q->hits0 + it->qbase;
  if (partial && (rc = dalloc(it, &it->partial, 3 * npix))) return rc;  // (k_gen_rays clears it)
  HIP_TRY(it->ev0.create());
  HIP_TRY(it->ev1.create());
  it->bounce_ev.resize(2 * cap);
  for (Event& e : it->bounce_ev) HIP_TRY(e.create());
  return KDPT_OK;
}

// One more pipeline group: its stream, then its B iteration states, the first with the group's ray queue.
int make_group(kdpt_ctx* c, int B) {
  c->pipe.groups.emplace_back();
  IterGroup& grp = c->pipe.groups.back();
  if (int rc = create_stream(c, &grp.stream)) return rc;
  for (int b = 0; b < B; b++) {
    grp.its.emplace_back(new IterState());
    int rc = alloc_iter(c, grp.its.back().get(), grp.stream, true, b ? grp.its[0].get() : nullptr, b, B);
    if (rc) return rc;
  }
  HIP_TRY(grp.acc_ev.create_untimed());
  return KDPT_OK;
}

}  // namespace
