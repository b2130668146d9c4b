// kdpt_runtime.hip -- the runtime behind the C ABI (include/kdpt.h): the context and its device memory,
// kdpt_create (upload of what kdpt_scene_prep.h prepared), the knobs, the launch sequence of an iteration
// (launch_batch), pipelined / batched iterations, the multi-GPU frame path, the ray queries and the
// caller-defined views (kdpt_set_camera, kdpt_camera_rays, kdpt_trace_rays).  One HIP
// translation unit: the kernels live in the kernels_*.h headers included below, one per stage; scene
// validation and packing live in kdpt_scene_prep.h and run before any device call.
//
// One iteration of the reference's per-sample hot path (src/pathtrace.cu:2405-2635 `pathtrace`), as queued by
// launch_batch for a batch of up to MAXB iterations in lockstep (blockIdx.y / the batch records = iteration):
//   k_gen_geoms_b   : camera rays + bounce 0's analytic geoms and root-box test, which queue the rays that
//                     meet the KD root box (k_gen_rays_b alone on the brute-force / viz routes); a path-traced ray
//                     query (kdpt_trace_rays) starts from the caller's rays instead: k_user_geoms_b / k_user_rays_b
//   then per bounce (cap 8, src/pathtrace.cu:2608):
//   k_trace         : the intersect kernel -- KD traversal of the queued rays, persistent waves pulling
//                     64-ray chunks, the tree read from LDS when a record format fits (setup_trace); k_brute /
//                     k_viz instead with enable_kd = 0 / viz_kd
//   k_shade_fused_b : scatterRay + shadeMaterial + partialGather, the stable compaction of the survivors into
//                     the other path buffer (thrust::remove_if; decoupled look-back over the tiles) and the
//                     next bounce's geoms stage and ray queue, in one launch
//   and k_final_gather after the last bounce.
// Iteration 2's stable sort by materialIdHit (thrust::sort), compaction = 0 and the "shade_fused" = 0 knob take
// the three-kernel route instead: k_shade, k_scan, k_scatter (and k_geoms_b where no hand-off prepared the rays).
// No host synchronisation inside an iteration: the live-path count lives on the device and kernels past the
// end of the live range exit at once.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include <dlfcn.h>
#include <rccl/rccl.h>

#include "../../include/kdpt.h"
#include "kdpt_error.h"
#include "kdpt_device.h"
#include "kdpt_clusters.h"
#include "kdpt_scene_prep.h"

using namespace kdpt;

namespace {

double g_reduce_spin_us = 0;  // kdpt_set_tuning(NULL, "reduce_spin_us", v): the default of new contexts
double g_cluster_chord = -1;   // kdpt_set_tuning(NULL, "cluster_chord", v): big-leaf grouping of new contexts
bool g_cu_mask_streams = true;  // kdpt_set_tuning(NULL, "cu_mask_streams", v): ... and their stream kind

}  // namespace

// The kernels, one header per stage, in the order the code object keeps them.
#include "kernels_gen.h"
#include "kernels_trace.h"
#include "kernels_brute.h"
#include "kernels_shade.h"
#include "kernels_image.h"
#include "kernels_cast.h"
#include "kernels_rays.h"
#include "kernels_selftest.h"
#include "kernels_moments.h"

// ---------------------------------------------------------------------------
// Context
// ---------------------------------------------------------------------------
// One iteration's working set (alloc_iter / free_iter).  The context has one for the one-at-a-time entry points
// and B per pipeline group; everything an iteration shares with the others (scene, options, knobs, counters)
// stays in the context.
struct IterState {
  std::vector<void*> allocs;  // the device memory below
  PathBuf buf[2]{};
  int cur = 0;
  int* counts = nullptr;  // [cap + 2] live paths per bounce, [1] fault word, then [cap] work counters, ...
  int* fault = nullptr;
  int* work = nullptr;
  int* ccount = nullptr;    // [cap] walking survivors per bounce
  int* tickets = nullptr;   // [cap] k_shade_fused's tile tickets
  int* ccount0 = nullptr;   // [2] bounce-0 candidate counters of k_gen_geoms_b (alternating uses)
  int gen_parity = 0;       // which of them the next use counts into
  int* cc0_cur = nullptr;   // this use's (bounce 0 reads it instead of ccount[0])
  int2* hits = nullptr;     // [npix] hit code + objMaterialIdx from the intersect kernel
  float4* cray = nullptr;   // [2 npix] the candidates' rays in queue order (k_geoms / shading -> k_trace)
  int* cand = nullptr;      // [npix] paths whose ray meets the KD root box (k_geoms -> k_trace)
  int2* prep = nullptr;     // [npix] next bounce's geoms record + walk flag (k_shade -> k_scatter)
  int* tile_counts = nullptr;
  int* tile_off = nullptr;
  int* tile_ccounts = nullptr;  // [ntiles] walking survivors per tile, and their offsets
  int* tile_coff = nullptr;
  unsigned long long* lb = nullptr;       // [cap][ntiles] k_shade_fused's look-back records
  unsigned long long* trace_t = nullptr;  // per-bounce intersect launch record
  int* h_counts = nullptr;  // pinned
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  std::vector<hipEvent_t> bounce_ev;
  // where the iteration's light goes: the context's image, or a pipeline state's own partial image, which
  // k_gen_rays zeroes first (zero_partial); and where its segment count is added
  float* image = nullptr;
  bool zero_partial = false;
  unsigned long long* total_segments = nullptr;

  // The state's part of each launch's arguments (launch_batch's stages).
  GenIter gen_iter(int iter) const { return {iter, buf[0], counts, work, trace_t, lb, zero_partial ? image : nullptr}; }
  // (takes this use's bounce-0 counter and hands the other one over for zeroing: flips gen_parity)
  GenGeomsIter gen_geoms_iter() {
    cc0_cur = ccount0 + gen_parity;
    gen_parity ^= 1;
    return {cc0_cur, ccount0 + gen_parity, cray, hits, cand};
  }
  GeomsIter geoms_iter() const { return {buf[cur], counts, cray, hits, cand, ccount}; }
  // The candidate counter of bounce `depth`, indexed by depth: k_gen_geoms_b counted bounce 0 into cc0_cur.
  const int* cand_count(int depth, bool gen_geoms) const { return (depth == 0 && gen_geoms) ? cc0_cur : ccount; }
  TraceIter trace_iter(int depth, bool gen_geoms) const { return {cand, cand_count(depth, gen_geoms), cray, hits}; }
  // (compaction goes into the other path buffer)
  FuseArgs fuse_args() const { return {buf[cur ^ 1], tickets, lb, counts, ccount, cray, hits, cand}; }
  ScatterPrep scatter_prep(bool on) const { return {on ? 1 : 0, prep, cray, hits, cand, tile_coff}; }
};

// A pipeline group: `batch` iterations at a time in lockstep on the group's own stream; acc_ev: its last
// batch's add into the target done.
struct IterGroup {
  hipStream_t stream = nullptr;
  hipEvent_t acc_ev = nullptr;
  std::vector<std::unique_ptr<IterState>> its;
};

struct kdpt_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  kdpt_options opt{};
  kdpt_camera cam{};
  int traceDepth = 0;
  int W = 0, H = 0, npix = 0, ntiles = 0, nkeys = 1;
  int cap = 8;
  DevScene S{};
  // owned device memory
  std::vector<void*> allocs;
  uchar4* pbo_staging = nullptr;  // kdpt_write_pbo into host memory
  IterState solo;         // kdpt_trace_iteration[_async], kdpt_debug_paths, kdpt_count_iteration; into `image`
  float* image = nullptr;
  bool image_external = false;
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
  // the exact one-level cull's direction masks (kdpt_clusters.h build_dir_masks), built when the scene's rigorous
  // margin is above the cap; S.cl_mask points at them unless a knob chose another cull
  unsigned long long* mask_dev = nullptr;
  float4* tn_dev = nullptr;  // the clusters' per-entry normal records (DevScene::cl_tn)
  int mask_n = 0;
  bool cull_exact = true;   // "cull_exact" knob: 0 = the fast-margin cull (not exact for such scenes)
  double create_ms = 0, mask_build_ms = 0;  // kdpt_create's host wall time, and the masks' (kdpt_stats)
  bool cu_mask_streams = false;  // batch and reduce streams created with an all-CU mask (create_stream)
  bool cull_scene = true;   // false after "cluster_cull" = 0 or a fixed "cull_margin"
  std::unique_ptr<ClusterSet> mask_cs;  // the clusters the masks were built from ("cull_mask_n" rebuilds)
  int tree_format = 0;             // "tree_format" knob: 16 / 32 = LDS node records of that size only
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
  // Pipelined iterations (kdpt_trace_iterations): groups of `group_batch` iteration states, each state with a
  // partial image of its own; the partial images are added into `image` in iteration order, each batch's add
  // on its group's stream after the previous batch's add (acc_ev / acc_last: the chain).
  std::vector<IterGroup> groups;
  int group_batch = 1;
  int next_group = 0;  // the group the next batch goes to
  bool profile_batches = false;
  bool profile_steps = false;  // "profile_batches" = 2
  hipEvent_t entry_ev = nullptr;   // enqueue_iterations: what the context's own stream held when the call began
  hipEvent_t acc_last = nullptr;   // the most recent add (a group's acc_ev): the next add follows it
  hipEvent_t img_last = nullptr;   // the most recent frame reduce + image add (one of frame_ev)
  // intersect-kernel timing (testing_mode) of every iteration, read back at synchronisation
  std::vector<std::vector<hipEvent_t>> pending_ev;  // per launched iteration: 2 events per bounce
  std::vector<hipEvent_t> free_ev;
  double intersect_ms_total = 0;
  long long intersect_launches_total = 0;
  // enable_kd = 0: brute-force intersect kernel over the OBJ triangles in file order
  bool brute = false;
  bool viz = false;  // viz_kd: the KD node boxes drawn as boxes (k_viz)
  BruteShape* shapes = nullptr;
  int num_shapes = 0;
  float4* chunk_lo = nullptr;  // brute force: boxes of 64 file-order triangles
  float4* chunk_hi = nullptr;
  float chunk_k_min = 0.0f;    // brute force: the smallest of the chunks' own cull coefficients (chunk_lo[j].w)
  // spp-sharded frames (kdpt_comm_init / kdpt_render_frames / kdpt_render_sharded): this context's rank, the
  // RCCL communicator (null: one rank, or the in-process copy reduce of kdpt_render_sharded), two frame
  // buffers (frame f accumulates into frame_buf[f & 1] while f - 1 is reduced) and rank 0's reduced frame
  int nranks = 1, rank = 0;
  void* comm = nullptr;  // ncclComm_t
  bool owns_comm = false;
  bool external_reduce = false;  // kdpt_comm_init without an id: each rank hands its frame shares out
  float* frame_buf[2] = {nullptr, nullptr};
  float* frame_sum = nullptr;
  hipEvent_t frame_ev[2] = {nullptr, nullptr};      // frame_buf[k] consumed by its reduce
  hipStream_t reduce_stream = nullptr;  // the frames' reduces and image adds, beside the accumulation stream
  double reduce_spin_us = 0;  // "reduce_spin_us" knob: a device spin before every frame's reduce (a slow peer)
  std::vector<void*> host_reg;  // pageable host `out` ranges pinned for kdpt_render_frames (released at synchronize)
  // ray queries (kdpt_cast_rays): buffers of one chunk, made on first use and remade when "cast_chunk" changes --
  // the input and output staging buffers (host arrays go through them), the query's own candidate queue, hit
  // records and counters (CastArgs); nothing here is shared with the render path
  int cast_chunk = 1 << 20;     // "cast_chunk" knob: rays per chunk
  int cast_alloc = 0;           // the chunk size the buffers below were made for (0: none yet)
  float* cast_in = nullptr;     // [6 chunk] origins, then directions
  kdpt_ray_hit* cast_out = nullptr;  // [chunk]
  float4* cast_cray = nullptr;  // [2 chunk]
  int* cast_cand = nullptr;     // [chunk]
  int2* cast_hits = nullptr;    // [chunk]
  int* cast_cnt = nullptr;      // [2]
  unsigned long long* cast_tt = nullptr;  // [3]
  hipEvent_t cast_ev[2] = {nullptr, nullptr};
  long long cast_rays = 0, cast_traced = 0;  // since create/reset (kdpt_cast_stats)
  double cast_ms = 0;                        // the last call's device time
  // path-traced ray queries (kdpt_trace_rays, kdpt_camera_rays): an iteration state of their own, made on first
  // use (query_state) -- its image is the query's radiance buffer, its segment and intersect totals go to
  // query_totals instead of the context's -- and a staging buffer for host arrays; nothing here is shared with
  // the render path or with kdpt_cast_rays
  IterState query;
  bool query_ready = false;
  float* query_image = nullptr;  // [3 npix]
  float* query_stage = nullptr;  // [6 npix] origins, then directions (inputs of host callers, camera rays on their way out)
  unsigned long long* query_totals = nullptr;  // [0] ShadeArgs::total_segments, [1..3] trace_total / trace_rays
  long long query_segments = 0, query_traced = 0;  // of the last kdpt_trace_rays (kdpt_trace_rays_stats)
  double query_ms = 0;                             // ... and its device time
  // kdpt_trace_rays_moments: the partial buffer each of the query's iterations gathers into (zeroed by a fill on
  // the stream) and the query's second moments, made on first use; nothing here is shared with the render's moments
  float* query_partial = nullptr;  // [3 npix]
  float* query_sumsq = nullptr;    // [3 npix]
  // per-pixel second moments (kdpt_set_moments): sumsq beside the image, the partial image the solo state gathers
  // into while they are on (added with k_accumulate_moments at nb = 1), the number of iterations added since both
  // were zeroed, and kdpt_noise_map's / kdpt_noise_estimate's buffers.  All null / 0 while moments are off.
  bool moments = false;
  float* mom_sumsq = nullptr;    // [3 npix]
  float* mom_partial = nullptr;  // [3 npix]
  long long mom_samples = 0;
  float* noise_stage = nullptr;         // [npix] kdpt_noise_map into host memory
  NoisePartial* noise_parts = nullptr;  // [workgroups + 1] k_noise_partials' partials, then k_noise_final's result
  // an iteration (or a frame) has been added into the image since create / kdpt_reset: with stats.iterations what
  // kdpt_set_moments(1) refuses on (kdpt_trace_iteration_async counts no iteration)
  bool accumulated = false;
};

namespace {

// A context's streams (its own, the batch groups' and the frame reduce's): created with a mask of every CU, which
// gives each a hardware queue of its own instead of one of the GPU_MAX_HW_QUEUES (4 by default) in-order queues
// HIP multiplexes a process's plain streams onto -- where a waiting or long-running command of one stream holds
// the others on its queue.  C4's 32-spp frames: 6.49 -> 5.68 ms with 24 queues, and a 5 ms reduce delay per frame
// costs nothing at 4 or 24 queues (profiles/r06_ab_log.md).  Knob "cu_mask_streams" = 0 (process default):
// plain non-blocking streams; a failed creation falls back to one.
// kdpt_ctx::shade_oob: every entry point that shades ends here before it queues anything.
int refuse_shading() {
  return fail(KDPT_ERR_UNSUPPORTED,
              "the OBJ has triangles of a shape other than the first: their hits carry material mtlIdx + "
              "num_materials - 1, past the materials array (as in the reference), so the scene cannot be shaded; "
              "kdpt_cast_rays and enable_kd = 0 remain available");
}

int create_stream(kdpt_ctx* c, hipStream_t* st) {
  if (c->cu_mask_streams) {
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, c->device));
    const int n = std::max(1, prop.multiProcessorCount);
    std::vector<uint32_t> mask((n + 31) / 32, 0xffffffffu);
    if (n % 32) mask.back() = (1u << (n % 32)) - 1u;
    if (hipExtStreamCreateWithCUMask(st, (uint32_t)mask.size(), mask.data()) == hipSuccess) return KDPT_OK;
    (void)hipGetLastError();
  }
  HIP_TRY(hipStreamCreateWithFlags(st, hipStreamNonBlocking));
  return KDPT_OK;
}

template <typename Owner, typename T>  // a context or an iteration state
int dalloc(Owner* c, T** p, size_t n) {
  void* q = nullptr;
  HIP_TRY(hipMalloc(&q, std::max<size_t>(n, 1) * sizeof(T)));
  c->allocs.push_back(q);
  *p = (T*)q;
  return KDPT_OK;
}

template <typename T>
int dupload(kdpt_ctx* c, T** p, const T* src, size_t n) {
  int rc = dalloc(c, p, n);
  if (rc) return rc;
  if (n) HIP_TRY(hipMemcpy(*p, src, n * sizeof(T), hipMemcpyHostToDevice));
  return KDPT_OK;
}

int launch_iteration(kdpt_ctx* c, int iter, int stop_depth, bool count);
int accumulate_iteration(kdpt_ctx* c, int iter);
void release_comm(kdpt_ctx* c);  // (multi-GPU section, end of file)
void unregister_host(kdpt_ctx* c);
void free_cast_buffers(kdpt_ctx* c);  // (ray queries, end of file)
void free_moments(kdpt_ctx* c);       // (second moments, end of file)
// A batch that starts from caller-supplied rays instead of the camera's (kdpt_trace_rays; one iteration per
// batch): the rays in device memory, and where the shading adds what it would add to the context's intersect
// totals (kdpt_ctx::trace_total's layout).
struct RaySource {
  UserRays rays;
  unsigned long long* trace_total;
};
int launch_batch(kdpt_ctx* c, IterState* const* its, const int* iters, int nb, hipStream_t st, int trace_grid,
                 int stop_depth, bool count, std::vector<hipEvent_t>* bev, const RaySource* rays = nullptr);

// Work queued on the context's own stream that reads or writes `image` must follow the pipelined
// accumulation (kdpt_trace_iterations adds partial images on the batch streams without a host sync) and the
// frames' image adds (kdpt_render_frames, on the reduce stream).
int join_accum(kdpt_ctx* c) {
  if (c->acc_last) HIP_TRY(hipStreamWaitEvent(c->stream, c->acc_last, 0));
  if (c->img_last) HIP_TRY(hipStreamWaitEvent(c->stream, c->img_last, 0));
  return KDPT_OK;
}


// stats.segments / seg_per_bounce / bounces of the iteration whose counts are in the solo state's h_counts
int segments_from_counts(kdpt_ctx* c) {
  const int* h_counts = c->solo.h_counts;
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

void free_iter(IterState* it) {
  for (void* p : it->allocs) (void)hipFree(p);
  if (it->h_counts) (void)hipHostFree(it->h_counts);
  if (it->ev0) (void)hipEventDestroy(it->ev0);
  if (it->ev1) (void)hipEventDestroy(it->ev1);
  for (auto e : it->bounce_ev)
    if (e) (void)hipEventDestroy(e);
  *it = IterState{};
}

// Per-iteration device state: two path buffers, hit records, candidate queue, tile counts/offsets,
// live counts + fault word + work counters, and the events.  (The scene, image and counters live elsewhere.)
// The zero fills go on the stream st the state will run on and are waited for: every kernel of the context runs
// on a non-blocking stream, which does not order itself after the null stream, so a plain hipMemset there could
// land after the first iteration's camera-ray kernel had set its path count (that iteration would vanish).
// partial: with a partial image of its own (a pipeline state); else the caller points `image` at its target.
// A failed allocation leaves what was made to free_iter.
int alloc_iter(kdpt_ctx* c, IterState* it, hipStream_t st, bool partial) {
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
      (rc = dalloc(it, &it->hits, npix)) || (rc = dalloc(it, &it->cand, npix)) || (rc = dalloc(it, &it->prep, npix)) ||
      (rc = dalloc(it, &it->tile_ccounts, ntiles)) || (rc = dalloc(it, &it->tile_coff, ntiles)) ||
      (rc = dalloc(it, &it->cray, 2 * npix)) || (rc = dalloc(it, &it->tile_counts, (size_t)MAX_KEYS * ntiles)) ||
      (rc = dalloc(it, &it->tile_off, (size_t)MAX_KEYS * ntiles)))
    return rc;
  HIP_TRY(hipHostMalloc((void**)&it->h_counts, sizeof(int) * (cap + 3), hipHostMallocDefault));
  HIP_TRY(hipMemsetAsync(it->counts, 0, sizeof(int) * (4 * cap + 5), st));
  HIP_TRY(hipMemsetAsync(it->lb, 0, sizeof(unsigned long long) * cap * ntiles, st));
  HIP_TRY(hipStreamSynchronize(st));
  it->fault = it->counts + cap + 2;
  it->work = it->counts + cap + 3;
  it->ccount = it->work + cap;
  it->tickets = it->ccount + cap;
  it->ccount0 = it->tickets + cap;  // 2 entries, zero
  it->gen_parity = 0;
  if (partial) {
    if ((rc = dalloc(it, &it->image, 3 * npix))) return rc;
    it->zero_partial = true;  // k_gen_rays clears the partial image
  }
  it->total_segments = c->total_segments;
  HIP_TRY(hipEventCreate(&it->ev0));
  HIP_TRY(hipEventCreate(&it->ev1));
  it->bounce_ev.resize(2 * cap);
  for (auto& e : it->bounce_ev) HIP_TRY(hipEventCreate(&e));
  return KDPT_OK;
}

// Drop the pipeline's groups (their streams drained here), last first.
void drop_groups(kdpt_ctx* c) {
  for (size_t g = c->groups.size(); g-- > 0;) {
    IterGroup& grp = c->groups[g];
    if (grp.stream) (void)hipStreamSynchronize(grp.stream);
    for (size_t k = grp.its.size(); k-- > 0;) free_iter(grp.its[k].get());
    if (grp.acc_ev) (void)hipEventDestroy(grp.acc_ev);
    if (grp.stream) (void)hipStreamDestroy(grp.stream);
  }
  c->groups.clear();
  c->acc_last = nullptr;
}

// One more pipeline group: its stream, then its B iteration states.
int make_group(kdpt_ctx* c, int B) {
  c->groups.emplace_back();
  IterGroup& grp = c->groups.back();
  if (int rc = create_stream(c, &grp.stream)) return rc;
  for (int b = 0; b < B; b++) {
    grp.its.emplace_back(new IterState());
    int rc = alloc_iter(c, grp.its.back().get(), grp.stream, true);
    if (rc) return rc;
  }
  HIP_TRY(hipEventCreateWithFlags(&grp.acc_ev, hipEventDisableTiming));
  return KDPT_OK;
}

// A batch's partial images added in iteration order (one add per pixel and iteration, as partialGather
// does), with one read and one write of the accumulation image per batch instead of one per iteration.
struct PartialImages {
  const float* p[MAXB];
  int nb;
};
__global__ void k_accumulate_batch(float* __restrict__ image, PartialImages parts, int n3) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n3) return;
  float v = image[i];
  for (int b = 0; b < parts.nb; b++) v += parts.p[b][i];
  image[i] = v;
}

// The add of nb partial images (iteration order) into `target` on stream st: k_accumulate_batch, or, when the
// context keeps second moments and the target is its image, k_accumulate_moments, which adds the squares into
// mom_sumsq in the same pass.
int launch_accumulate(kdpt_ctx* c, float* target, const float* const* partials, int nb, hipStream_t st) {
  const int n3 = 3 * c->npix;
  if (c->moments && target == c->image) {
    MomentParts parts{};
    parts.nb = nb;
    for (int b = 0; b < nb; b++) parts.p[b] = partials[b];
    hipLaunchKernelGGL(k_accumulate_moments, dim3((n3 + 255) / 256), dim3(256), 0, st, target, c->mom_sumsq, parts,
                       n3);
  } else {
    PartialImages parts{};
    parts.nb = nb;
    for (int b = 0; b < nb; b++) parts.p[b] = partials[b];
    hipLaunchKernelGGL(k_accumulate_batch, dim3((n3 + 255) / 256), dim3(256), 0, st, target, parts, n3);
  }
  HIP_TRY(hipGetLastError());
  return KDPT_OK;
}

// Read back the intersect-kernel events of finished iterations (testing_mode).
int drain_intersect_events(kdpt_ctx* c) {
  for (auto& evs : c->pending_ev) {
    for (size_t k = 0; k + 1 < evs.size(); k += 2) {
      float ms = 0;
      HIP_TRY(hipEventSynchronize(evs[k + 1]));
      if (hipEventElapsedTime(&ms, evs[k], evs[k + 1]) == hipSuccess) {
        c->intersect_ms_total += ms;
        c->intersect_launches_total++;
      }
    }
    for (auto e : evs) c->free_ev.push_back(e);
  }
  c->pending_ev.clear();
  return KDPT_OK;
}

// The scene's cull margins (kdpt_clusters.h cluster_margin) into the context and its DevScene; fixed: one
// direction-free coefficient for every level (tuning "cull_margin" / "cluster_cull" = 0, which passes inf).
void set_cull(kdpt_ctx* c, const CullMargin& cm) {
  c->cull = cm;
  c->S.cl_margin = cm.K;
  c->S.cl_margin_lo = cm.K_lo;
  c->S.cull_a = cm.a;
  c->S.cull_b = cm.b;
  c->S.cull_c = cm.c;
}
void fix_cull(kdpt_ctx* c, float K) {
  c->S.cl_margin = c->S.cl_margin_lo = K;
}
// The one-level route's cull: the exact masked one when the scene has masks and the knobs leave the scene's
// margins in place, else the margin-only cull.
void apply_cull_route(kdpt_ctx* c) {
  c->S.cl_mask = (c->mask_dev && c->cull_exact && c->cull_scene) ? c->mask_dev : nullptr;
  c->S.mask_n = c->mask_n;
  c->S.cl_tn = c->tn_dev;
}
// The masked cull's cells on the device (kdpt_device.h dir_mask_cell, the code the host builder runs): one
// workgroup per (cluster, 256 buckets), the cluster's 64 entries staged in LDS (every lane reads the same entry:
// a broadcast), one mask per lane, written bucket-major.
__global__ void __launch_bounds__(256) k_build_masks(const double* __restrict__ ent, const float* __restrict__ krig,
                                                     const double* __restrict__ bd, int ncl, int nb, float Kf,
                                                     unsigned long long* __restrict__ masks) {
  __shared__ double se[5][64];
  __shared__ float sk[64];
  const int c = blockIdx.x;
  const size_t ne = 64 * (size_t)ncl;
  if (threadIdx.x < 64) {
    for (int f = 0; f < 5; f++) se[f][threadIdx.x] = ent[f * ne + 64 * (size_t)c + threadIdx.x];
    sk[threadIdx.x] = krig[64 * (size_t)c + threadIdx.x];
  }
  __syncthreads();
  const int b = blockIdx.y * 256 + threadIdx.x;
  if (b >= nb) return;
  masks[(size_t)b * ncl + c] = dir_mask_cell(se[0], se[1], se[2], se[3], se[4], sk, bd + 4 * (size_t)b, Kf);
}

// Release one of the context's device allocations before kdpt_destroy (a rebuilt table).
void dfree(kdpt_ctx* c, void* p) {
  if (!p) return;
  auto it = std::find(c->allocs.begin(), c->allocs.end(), p);
  if (it != c->allocs.end()) c->allocs.erase(it);
  (void)hipFree(p);
}

// The direction masks of the scene's clusters at resolution n (cube-map cells per face edge), built on the device (k_build_masks) from the per-entry records and the bucket directions the host
// computes (kdpt_clusters.h mask_entries / mask_buckets; tests/test_gpu_parity.py checks the cells against the
// host builder).  A rebuild (knobs "cull_mask_n", "cull_fast_k") frees the previous table once the new one is
// filled; a failed one changes nothing in the context.
int build_masks(kdpt_ctx* c, int n) {
  const auto t0 = std::chrono::steady_clock::now();
  const ClusterSet& cs = *c->mask_cs;
  const int ncl = (int)cs.info.size(), nb = 6 * n * n;
  // the intersect kernel indexes the table with 32 bits (kdpt_device.h, S.cl_mask[bucket * num_clusters + c]): a
  // resolution whose table has 2^32 cells or more is refused here, before anything is freed or allocated
  if (n < 1 || (unsigned long long)nb * (unsigned long long)ncl >= (1ull << 32))
    return fail(KDPT_ERR_ARG, "direction masks: 6 n^2 num_clusters must be below 2^32 (n = " + std::to_string(n) +
                                  ", " + std::to_string(ncl) + " clusters: n <= " +
                                  std::to_string((int)std::sqrt((double)((1ull << 32) - 1) / (6.0 * std::max(1, ncl)))) +
                                  ")");
  const float Kf = c->cull.K;
  MaskEntries me;
  mask_entries(cs, Kf, me);
  std::vector<double> bd;
  mask_buckets(n, bd);
  const size_t ne = 64 * (size_t)ncl;
  std::vector<double> ent(5 * ne);
  for (size_t k = 0; k < ne; k++) {
    ent[k] = me.nx[k];
    ent[ne + k] = me.ny[k];
    ent[2 * ne + k] = me.nz[k];
    ent[3 * ne + k] = me.beta[k];
    ent[4 * ne + k] = me.dthr[k];
  }
  // The new table is the context's only once it is filled: until then mask_dev, mask_n and S.cl_mask keep
  // describing the previous one, which a failure below leaves in place.
  unsigned long long* dm = nullptr;
  double* d_ent = nullptr;
  float* d_krig = nullptr;
  double* d_bd = nullptr;
  auto release = [&]() {
    (void)hipFree(d_ent);
    (void)hipFree(d_krig);
    (void)hipFree(d_bd);
  };
  // (the uploads on the context's stream, ahead of the kernel; pageable sources are staged before each call
  // returns, and the stream is drained before the temporaries go)
  hipError_t e;
  if ((e = hipMalloc((void**)&dm, std::max<size_t>((size_t)nb * ncl, 1) * sizeof(unsigned long long))) != hipSuccess ||
      (e = hipMalloc(&d_ent, ent.size() * sizeof(double))) != hipSuccess ||
      (e = hipMalloc(&d_krig, me.krig.size() * sizeof(float))) != hipSuccess ||
      (e = hipMalloc(&d_bd, bd.size() * sizeof(double))) != hipSuccess ||
      (e = hipMemcpyAsync(d_ent, ent.data(), ent.size() * sizeof(double), hipMemcpyHostToDevice, c->stream)) !=
          hipSuccess ||
      (e = hipMemcpyAsync(d_krig, me.krig.data(), me.krig.size() * sizeof(float), hipMemcpyHostToDevice, c->stream)) !=
          hipSuccess ||
      (e = hipMemcpyAsync(d_bd, bd.data(), bd.size() * sizeof(double), hipMemcpyHostToDevice, c->stream)) != hipSuccess) {
    (void)hipStreamSynchronize(c->stream);
    release();
    (void)hipFree(dm);
    return hip_fail("mask build: device buffers", e);
  }
  hipLaunchKernelGGL(k_build_masks, dim3(ncl, (nb + 255) / 256), dim3(256), 0, c->stream, d_ent, d_krig, d_bd, ncl,
                     nb, Kf, dm);
  const hipError_t e1 = hipGetLastError(), e2 = hipStreamSynchronize(c->stream);
  release();
  int rc = (e1 != hipSuccess || e2 != hipSuccess) ? hip_fail("k_build_masks", e1 != hipSuccess ? e1 : e2) : KDPT_OK;
  if (!rc && !c->tn_dev) {
    std::vector<float4> tn;
    build_entry_normals(cs, tn);
    float4* d_tn = nullptr;
    if ((rc = dupload(c, &d_tn, tn.data(), tn.size()))) dfree(c, d_tn);
    else c->tn_dev = d_tn;
  }
  if (rc) {
    (void)hipFree(dm);
    return rc;
  }
  // the swap: the previous table is freed before the call returns (the stream was drained above)
  dfree(c, c->mask_dev);
  c->allocs.push_back(dm);
  c->mask_dev = dm;
  c->mask_n = n;
  c->mask_build_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  apply_cull_route(c);
  return KDPT_OK;
}

// ---------------------------------------------------------------------------
// Kernel variants: the one place where run-time choices become template arguments.  Every launch, occupancy
// query and attribute call takes its kernel from these tables as a typed pointer (a wrong argument struct stays
// a compile error); a new tree route or template flag is a new table entry and nothing else.
//
// The GPU test that reaches each entry (H / B: the hybrid / bare walk, short_stack 1 / 0):
//   k_trace, count off: TREE_WIDE, PACKED, LDS, LDS16 / LDS16G, H and B -- test_soup_cast_equals_oracle (rootleaf8200
//     "tree_global", syn20000, "tree_format" 32, "tree_format" 16); LDS16G, LDS16S, H and B -- test_cast_equals_oracle
//     (ico7, ico7-margin); in renders test_tuning_knobs_keep_parity, test_derived_box_tree_in_lds
//   k_trace, count on: TREE_WIDE, PACKED, LDS, LDS16, H and B -- test_soup_counters_on_every_route; LDS, H also
//     test_counters_match_oracle; LDS16G, LDS16S, H -- test_counters_on_the_cluster_routes (B: no test)
//   k_shade: compact + sort -- test_iteration2_sort_order (H), test_bit_exact_vs_oracle dragon_96_bare (B); compact
//     alone -- test_fused_shading_equals_scan_scatter (H); neither -- test_bit_exact_vs_oracle dragon_64_nocompact
//     (H); sort alone -- test_brute_force_bit_exact_vs_oracle sphere_48_brute_nocompact (H); B, those three --
//     test_geom_render_equals_oracle ("shade_fused" 0 and compaction 0 with short_stack 0, iterations 1 and 2)
//   k_shade_fused_b: STAGE -- every default render (H), dragon_96_bare (B); not STAGE (a scene of more than
//     ORDERED_GEOMS geoms or STAGE_MATS materials) -- test_geom_render_equals_oracle nine, mats33, mats64 (H and B);
//     k_shade_fused: H + STAGE -- test_tuning_knobs_keep_parity "shade_batch"; the other three --
//     test_geom_render_equals_oracle "shade_batch" 0 (tilted, nested, glass: STAGE; nine, mats33, mats64: not)
//   k_brute: count on -- test_brute_force_counters_match_oracle (use_bbox 0, 1); off --
//     test_brute_force_bit_exact_vs_oracle (both); k_cast_resolve: H and B -- test_cast_equals_oracle
// ---------------------------------------------------------------------------
struct TraceKernel {
  void (*fn)(TraceArgs);
  int block;
};
template <bool H, bool C, int M>
constexpr TraceKernel trace_variant() {
  return {k_trace<H, C, M>, trace_block<M>()};
}
#define TRACE_MODES(H, C)                                                                                         \
  {trace_variant<H, C, TREE_WIDE>(),  trace_variant<H, C, TREE_PACKED>(), trace_variant<H, C, TREE_LDS>(),        \
   trace_variant<H, C, TREE_LDS16>(), trace_variant<H, C, TREE_LDS16G>(), trace_variant<H, C, TREE_LDS16S>()}
// (mode: a TreeMode, the enum's values in order)
TraceKernel trace_kernel(bool hybrid, bool count, int mode) {
  static const TraceKernel table[2][2][6] = {{TRACE_MODES(false, false), TRACE_MODES(false, true)},
                                             {TRACE_MODES(true, false), TRACE_MODES(true, true)}};
  return table[hybrid][count][mode];
}
#undef TRACE_MODES

// The shading kernels compute the hit point with the offset of the traversal that found it: 1e-4 for the hybrid
// walk and the brute-force kernel, 1e-5 for traverseKDbare.
bool hybrid_shading(const kdpt_ctx* c) { return c->opt.short_stack || c->brute; }

using ShadeKernel = void (*)(ShadeArgs);
ShadeKernel shade_kernel(bool hybrid, bool compact, bool sort) {
  static const ShadeKernel table[2][2][2] = {{{k_shade<false, false, false>, k_shade<false, false, true>},
                                              {k_shade<false, true, false>, k_shade<false, true, true>}},
                                             {{k_shade<true, false, false>, k_shade<true, false, true>},
                                              {k_shade<true, true, false>, k_shade<true, true, true>}}};
  return table[hybrid][compact][sort];
}
// stage: the scene's geoms and materials fit the fused kernels' LDS copy
using FusedKernel = void (*)(ShadeArgs, FuseArgs);
FusedKernel shade_fused_kernel(bool hybrid, bool stage) {
  static const FusedKernel table[2][2] = {{k_shade_fused<false, false>, k_shade_fused<false, true>},
                                          {k_shade_fused<true, false>, k_shade_fused<true, true>}};
  return table[hybrid][stage];
}
using FusedBatchKernel = void (*)(ShadeBatch);
FusedBatchKernel shade_fused_batch_kernel(bool hybrid, bool stage) {
  static const FusedBatchKernel table[2][2] = {{k_shade_fused_b<false, false>, k_shade_fused_b<false, true>},
                                               {k_shade_fused_b<true, false>, k_shade_fused_b<true, true>}};
  return table[hybrid][stage];
}
// the fused kernels' STAGE argument: the scene's geoms and materials fit their LDS copy
bool shade_staged(const kdpt_ctx* c) {
  return c->S.num_geoms + c->S.num_boxes <= ORDERED_GEOMS && c->S.num_materials <= STAGE_MATS;
}
using BruteKernel = void (*)(BruteArgs);
BruteKernel brute_kernel(bool use_bbox, bool count) {
  static const BruteKernel table[2][2] = {{k_brute<false, false>, k_brute<false, true>},
                                          {k_brute<true, false>, k_brute<true, true>}};
  return table[use_bbox][count];
}

// The workgroups of the route's intersect kernel that fit a CU with `lds` bytes of tree: the fewest over the
// four (hybrid, count) variants, so that one grid serves whichever of them a launch picks.
int trace_blocks_per_cu(int mode, size_t lds, int* blocks) {
  int best = 0;
  for (int hyb = 0; hyb < 2; hyb++)
    for (int cnt = 0; cnt < 2; cnt++) {
      const TraceKernel k = trace_kernel(hyb, cnt, mode);
      int b = 0;
      if (lds > 0)
        HIP_TRY(hipFuncSetAttribute((const void*)k.fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
      HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&b, k.fn, k.block, lds));
      if (best == 0 || b < best) best = b;
    }
  *blocks = best;
  return KDPT_OK;
}

// Pick where the intersect kernel reads the tree from, and its persistent grid: in LDS when it fits (the
// "tree_format" knob limits the LDS records to one size) -- the candidate that keeps the most intersect waves
// on a CU wins, ties in the order below.
int setup_trace(kdpt_ctx* c) {
  hipDeviceProp_t prop;
  HIP_TRY(hipGetDeviceProperties(&prop, c->device));
  const size_t lds_max = prop.sharedMemPerBlock > 0 ? prop.sharedMemPerBlock : 65536;
  // (the counting kernel's per-wave WaveProf too: the tree must fit next to either kernel's static part)
  const size_t per_wave = sizeof(WaveLeafLDS) + sizeof(WaveProf);
  const size_t cl_bytes = 32 * (size_t)c->S.num_clusters;
  struct Cand { int mode; size_t lds; };
  std::vector<Cand> cands;
  // (in order of preference at equal occupancy: the 32-byte records need no box bookkeeping on the walk, which
  // costs the derived form 6 % on dragon_5; the derived form is what fits the C5 icosphere's tree)
  if (!c->force_global_tree) {
    if (c->S.pnodes && c->tree_format != 16) {
      const size_t t32 = 32 * (size_t)c->S.num_nodes + cl_bytes, st32 = per_wave * (TRACE_BLOCK / 64);
      if (st32 + t32 <= lds_max) cands.push_back({TREE_LDS, t32});
    }
    if (c->S.dnodes && c->tree_format != 32) {
      const size_t t16 = 16 * (size_t)c->S.num_nodes, st16 = per_wave * (TRACE_BLOCK16 / 64);
      if (st16 + t16 + cl_bytes <= lds_max) cands.push_back({TREE_LDS16, t16 + cl_bytes});
      // (leaving room for a fused-shading workgroup's LDS beside the intersect workgroup)
      const size_t sp_bytes = 16 * (size_t)c->S.num_supers;
      // (not when the one-level cull is the masked exact one: the supers' margins are not rigorous for it)
      if (c->S.snodes && c->super_cull && !c->S.cl_mask && st16 + t16 + sp_bytes + SHADE_LDS_RESERVE <= lds_max)
        cands.push_back({TREE_LDS16S, t16 + sp_bytes});
      if (st16 + t16 <= lds_max) cands.push_back({TREE_LDS16G, t16});
    }
  }
  c->tree_mode = c->S.pnodes ? TREE_PACKED : TREE_WIDE;
  c->tree_lds = 0;
  int blocks = 0, best_waves = 0, rc = KDPT_OK;
  for (const Cand& k : cands) {
    int b = 0;
    if ((rc = trace_blocks_per_cu(k.mode, k.lds, &b))) return rc;
    const int waves = b * trace_kernel(false, false, k.mode).block / 64;
    if (b > 0 && waves > best_waves) {
      best_waves = waves;
      blocks = b;
      c->tree_mode = k.mode;
      c->tree_lds = k.lds;
    }
  }
  if (c->tree_lds == 0 && (rc = trace_blocks_per_cu(c->tree_mode, 0, &blocks))) return rc;
  if (blocks < 1) return fail(KDPT_ERR_UNSUPPORTED, "intersect kernel does not fit on a CU");
  c->trace_grid = blocks * prop.multiProcessorCount;
  c->full_trace_grid = c->trace_grid;
  return KDPT_OK;
}

// setup_trace again after a knob that can change the route; a "trace_grid_frac" share of the grid is kept.
int resetup_trace(kdpt_ctx* c) {
  const double frac = (double)c->trace_grid / std::max(1, c->full_trace_grid);
  int rc = setup_trace(c);
  if (rc) return rc;
  if (c->grid_env) c->trace_grid = std::max(1, (int)(c->full_trace_grid * frac));
  return KDPT_OK;
}

// The "reduce_spin_us" knob of a context, or the process default of the contexts created later.
int set_reduce_spin(double* spin_us, double value) {
  if (!(value >= 0.0 && value <= 1e6)) return fail(KDPT_ERR_ARG, "reduce_spin_us must be in [0, 1e6]");
  *spin_us = value;
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

// The solo state's next iteration into a scratch image and a scratch segment total (zeroed on the context's
// stream), so that the accumulation image and stats.total_segments stay as they are; the scope's end puts the
// state's targets back and frees the scratch buffers.
struct ScratchTargets {
  IterState& it;
  float* const image;
  unsigned long long* const total_segments;
  void* scratch = nullptr;  // the image, then the total
  explicit ScratchTargets(IterState& s) : it(s), image(s.image), total_segments(s.total_segments) {}
  int redirect(kdpt_ctx* c) {
    const size_t img = sizeof(float) * 3 * (size_t)c->npix;
    HIP_TRY(hipMalloc(&scratch, img + sizeof(unsigned long long)));
    HIP_TRY(hipMemsetAsync(scratch, 0, img + sizeof(unsigned long long), c->stream));
    it.image = static_cast<float*>(scratch);
    it.total_segments = reinterpret_cast<unsigned long long*>(static_cast<char*>(scratch) + img);
    return KDPT_OK;
  }
  ~ScratchTargets() {
    it.image = image;
    it.total_segments = total_segments;
    if (scratch) (void)hipFree(scratch);  // (hipFree waits for whatever an early return left running)
  }
};

struct DeviceFree {
  void operator()(void* p) const { (void)hipFree(p); }
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

void kdpt_default_options(kdpt_options* o) { default_options(o); }


int kdpt_create(const kdpt_scene* sc, const kdpt_options* opt, int device, kdpt_ctx** out) {
  const auto t_create = std::chrono::steady_clock::now();
  if (!sc || !out) return fail(KDPT_ERR_ARG, "null scene/out");
  *out = nullptr;
  // every argument and scene error is reported here, before any device work (kdpt_scene_prep.h)
  PreparedScene p;
  {
    std::string err;
    const int prc = prepare_scene(sc, opt, g_cluster_chord, &p, &err);
    if (prc) return fail(prc, err);
  }
  const kdpt_options& o = p.opt;
  kdpt_ctx* c = new kdpt_ctx();
  c->shade_oob = p.shade_oob;
  c->device = device;
  c->opt = o;
  c->cam = sc->camera;
  c->traceDepth = sc->traceDepth;
  c->W = sc->camera.resolution[0];
  c->H = sc->camera.resolution[1];
  c->npix = c->W * c->H;
  c->ntiles = (c->npix + TILE - 1) / TILE;
  c->cap = o.bounce_cap;
  c->nkeys = std::max(1, sc->num_materials);
  auto bail = [&](int rc) {
    kdpt_destroy(c);
    return rc;
  };
  int rc;
  hipError_t e;
  if ((e = hipSetDevice(device)) != hipSuccess) return bail(hip_fail("hipSetDevice", e));
  c->cu_mask_streams = g_cu_mask_streams;
  if ((rc = create_stream(c, &c->stream))) return bail(rc);
  if ((e = hipEventCreateWithFlags(&c->entry_ev, hipEventDisableTiming)) != hipSuccess)
    return bail(hip_fail("hipEventCreateWithFlags", e));
  // the prepared arrays onto the device, DevScene pointed at them
  auto up = [&](auto** d, const auto& v) { return dupload(c, d, v.data(), v.size()); };
  DevScene& S = c->S;
  DevGeom* d_geoms;
  DevMaterial* d_mats;
  if ((rc = up(&d_geoms, p.geoms)) || (rc = up(&d_mats, p.materials))) return bail(rc);
  S.geoms = d_geoms;
  S.num_geoms = p.num_geoms;
  S.num_boxes = p.num_boxes;
  c->viz = p.viz;
  S.materials = d_mats;
  S.num_materials = sc->num_materials;
  S.has_obj = (p.kd || p.brute) ? 1 : 0;
  S.num_nodes = p.num_nodes;
  S.root = 0;
  S.n0_left = p.n0_left;
  S.n0_right = p.n0_right;
  S.n1_left = p.n1_left;
  S.n1_right = p.n1_right;
  S.rlo = p.rlo;
  S.rhi = p.rhi;
  S.gc = p.gc;
  S.gh = p.gh;
  set_cull(c, p.cull);
  if (p.kd || p.brute) {
    float4 *dtv, *de1, *de2, *dn0, *dn1, *dn2;
    if ((rc = up(&dtv, p.tri.tv0)) || (rc = up(&de1, p.tri.te1)) || (rc = up(&de2, p.tri.te2)) ||
        (rc = up(&dn0, p.tri.tn0)) || (rc = up(&dn1, p.tri.tn1)) || (rc = up(&dn2, p.tri.tn2)))
      return bail(rc);
    S.tv0 = dtv;
    S.te1 = de1;
    S.te2 = de2;
    S.tn0 = dn0;
    S.tn1 = dn1;
    S.tn2 = dn2;
  }
  if (p.kd) {
    const ClusterSet& cs = p.clusters;
    int4 *dnodes, *dpn = nullptr, *ddn = nullptr, *dsn = nullptr, *dsp;
    int* doff;
    int2 *dl, *di;
    float4 *dlo, *dhi, *dv0, *dce1, *dce2, *dn, *du, *dv, *dw, *dsupn, *dsupb;
    if ((rc = up(&dnodes, p.nodes)) || (rc = up(&doff, p.obj_material_offsets)) ||
        (!p.pnodes.empty() && (rc = up(&dpn, p.pnodes))) || (!p.dnodes.empty() && (rc = up(&ddn, p.dnodes))) ||
        (!p.snodes.empty() && (rc = up(&dsn, p.snodes))) ||
        (rc = up(&dl, cs.leaf_cl)) || (rc = up(&di, cs.info)) || (rc = up(&dlo, cs.lo)) || (rc = up(&dhi, cs.hi)) ||
        (rc = up(&dv0, cs.cv0)) || (rc = up(&dce1, cs.ce1)) || (rc = up(&dce2, cs.ce2)) ||
        (rc = up(&dsp, cs.sup)) || (rc = up(&dn, cs.nrm)) || (rc = up(&du, cs.obb_u)) ||
        (rc = up(&dv, cs.obb_v)) || (rc = up(&dw, cs.obb_w)) || (rc = up(&dsupn, cs.sup_n)) ||
        (rc = up(&dsupb, cs.sup_b)))
      return bail(rc);
    S.nodes = dnodes;
    S.pnodes = dpn;
    S.dnodes = ddn;
    S.snodes = dsn;
    S.obj_material_offsets = doff;
    S.leaf_cl = dl;
    S.num_clusters = (int)cs.info.size();
    S.cl_counts = p.cl_counts;
    S.cl_info = di;
    S.cl_lo = dlo;
    S.cl_hi = dhi;
    S.c_v0 = dv0;
    S.c_e1 = dce1;
    S.c_e2 = dce2;
    S.sup = dsp;
    S.num_supers = p.num_supers;
    S.cl_n = dn;
    S.cl_slab = 1;
    S.cl_u = du;
    S.cl_v = dv;
    S.cl_w = dw;
    S.cl_obb = 1;
    S.flat_obb = 1;
    S.sup_n = dsupn;
    S.sup_b = dsupb;
    S.sup_slab = 1;
    // the masked one-level cull's direction masks, for the fast margin the box levels use
    if (p.wants_masks) {
      c->mask_cs.reset(new ClusterSet(std::move(p.clusters)));
      if ((rc = build_masks(c, dir_mask_resolution(S.num_clusters)))) return bail(rc);
    }
  } else if (p.brute) {
    if ((rc = up(&c->shapes, p.shapes)) || (rc = up(&c->chunk_lo, p.chunk_lo)) || (rc = up(&c->chunk_hi, p.chunk_hi)))
      return bail(rc);
    c->num_shapes = (int)p.shapes.size();
    c->brute = true;
    c->chunk_k_min = HUGE_VALF;
    for (const float4& q : p.chunk_lo) c->chunk_k_min = std::min(c->chunk_k_min, q.w);
  }
  if (o.external_image) {
    c->image = o.external_image;
    c->image_external = true;
  } else if ((rc = dalloc(c, &c->image, 3 * (size_t)c->npix))) {
    return bail(rc);
  }
  if ((rc = dalloc(c, &c->counters, 1)) || (rc = dalloc(c, &c->total_segments, 1)) ||
      (rc = dalloc(c, &c->trace_total, 3)))
    return bail(rc);
  if ((rc = alloc_iter(c, &c->solo, c->stream, false))) return bail(rc);
  c->solo.image = c->image;
  // (the one-at-a-time launches and the ray queries report into the solo state's fault word; a pipelined
  // launch gets its own states' words, launch_batch)
  c->S.fault = c->solo.fault;
  {
    int khz = 0;
    if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, device) == hipSuccess && khz > 0)
      c->wall_khz = khz;
  }
  // The product reads no environment variables: every route is the tested default unless a caller
  // changes it explicitly with kdpt_set_tuning (A/B experiments, the three-kernel compaction test).
  c->S.trace_mode = 0;
  // leave the node phase early once at most early_walk lanes still walk and at least early_leaf wait on a
  // leaf (the walkers resume after the leaf phase; first A/B at 32 / 24: 3 390 -> 3 540 Mrays/s; 0 / 65 =
  // never)
  // re-swept after the flattened leaf phase made leaf phases cheaper (32 / 24 before: 4 505-4 530 -> 4 659-4 704
  // Mrays/s, k_trace launch 0.85 -> 0.80 ms), and again with round 5's exact cull (24 -> 16: C3 5 747-5 756 ->
  // 5 798-5 802, C5 4 487 -> 4 544; 8 / 12 / 20 / 32 below 16, early_leaf 8 / 24 neutral; profiles/r05_ab_log.md)
  c->S.early_walk = 16;
  c->S.early_leaf = 1;
  if ((rc = setup_trace(c))) return bail(rc);
  c->S.trip_limit = 8 * std::max(c->S.num_nodes, 1) + 64;
  // the scene's uploads (hipMemcpy) complete before any kernel of the context's non-blocking streams
  if ((e = hipDeviceSynchronize()) != hipSuccess) return bail(hip_fail("hipDeviceSynchronize", e));
  if ((rc = kdpt_reset(c))) return bail(rc);
  c->reduce_spin_us = g_reduce_spin_us;
  c->create_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_create).count();
  *out = c;
  return KDPT_OK;
}

int kdpt_set_options(kdpt_ctx* c, const kdpt_options* o) {
  if (!c || !o) return fail(KDPT_ERR_ARG, "null arg");
  const kdpt_options& p = c->opt;
  // these select what is uploaded or how much is allocated: a new context is needed
  if (o->enable_kd != p.enable_kd || o->viz_kd != p.viz_kd || o->use_bbox != p.use_bbox ||
      (o->bounce_cap > 0 ? o->bounce_cap : 8) != c->cap || o->block_size != p.block_size ||
      o->external_image != p.external_image)
    return fail(KDPT_ERR_UNSUPPORTED, "enable_kd, viz_kd, use_bbox, bounce_cap, block_size and external_image "
                                      "are fixed at kdpt_create");
  HIP_TRY(hipSetDevice(c->device));
  if (!c->groups.empty()) {  // iterations in flight keep the options they were enqueued with
    int rc = kdpt_synchronize(c);
    if (rc) return rc;
  }
  kdpt_options& d = c->opt;
  d.focal_length = o->focal_length;
  d.dof_angle = o->dof_angle;
  d.softness = o->softness;
  d.cacherays = o->cacherays;
  d.antialias = o->antialias;
  d.enable_sss = o->enable_sss;
  d.testing_mode = o->testing_mode;
  d.compaction = o->compaction;
  d.short_stack = o->short_stack;
  return KDPT_OK;
}

int kdpt_set_tuning(kdpt_ctx* c, const char* name, double value) {
  const std::string k(name ? name : "");
  if (!c && k == "reduce_spin_us") return set_reduce_spin(&g_reduce_spin_us, value);  // of contexts created later
  if (!c && k == "cu_mask_streams") {  // ... the kind of their batch / reduce streams
    g_cu_mask_streams = value != 0.0;
    return KDPT_OK;
  }
  if (!c && k == "cluster_chord") {  // ... and their big-leaf cluster grouping
    if (!(value >= -1.0 && value <= 4.0)) return fail(KDPT_ERR_ARG, "cluster_chord must be in [-1, 4]");
    g_cluster_chord = value;
    return KDPT_OK;
  }
  if (!name) return fail(KDPT_ERR_ARG, "kdpt_set_tuning: null name");
  if (!c) return fail(KDPT_ERR_ARG, "kdpt_set_tuning: null ctx, and no process-wide tuning knob is called " + k);
  if (k == "cast_chunk") {  // kdpt_cast_rays' chunk; its buffers are remade by the next call
    if (!(value >= 64.0 && value <= (double)(1 << 26))) return fail(KDPT_ERR_ARG, "cast_chunk must be in 64 .. 2^26");
    c->cast_chunk = (int)value;
    return KDPT_OK;
  }
  HIP_TRY(hipSetDevice(c->device));
  // queued iterations finish first: setup_trace and build_masks free and reallocate device memory their
  // kernels read.  The pipeline's states hold no knobs; they are still dropped, as include/kdpt.h documents
  // (the next kdpt_trace_iterations remakes them).
  if (!c->groups.empty()) {
    int rc = kdpt_synchronize(c);
    if (rc) return rc;
    drop_groups(c);
  }
  const int v = (int)value;
  bool route = false;  // the knob can change the intersect kernel's route: setup_trace again
  bool cull = false;   // ... and before that, which one-level cull it runs
  if (k == "shade_fused") {
    c->no_fuse = v == 0;
  } else if (k == "early_walk") {
    c->S.early_walk = v;
  } else if (k == "early_leaf") {
    c->S.early_leaf = v;
  } else if (k == "shade_batch") {
    c->shade_batch = v != 0;
  } else if (k == "gen_geoms") {
    c->gen_geoms = v != 0;
  } else if (k == "chunk_width0" || k == "chunk_width1" || k == "chunk_width2") {
    c->chunk_width[k.back() - '0'] = std::min(64, std::max(1, v));
  } else if (k == "trace_grid_frac") {
    if (!(value > 0.0 && value <= 1.0)) return fail(KDPT_ERR_ARG, "trace_grid_frac must be in (0, 1]");
    c->trace_grid = std::max(1, (int)(c->full_trace_grid * value));
    c->grid_env = value < 1.0;
  } else if (k == "cluster_obb") {
    c->S.cl_obb = v != 0;
  } else if (k == "flat_obb") {
    c->S.flat_obb = v != 0;
  } else if (k == "super_slab") {
    c->S.sup_slab = v != 0;
  } else if (k == "cluster_slab") {
    c->S.cl_slab = v != 0;
  } else if (k == "tree_format") {
    if (v != 0 && v != 16 && v != 32) return fail(KDPT_ERR_ARG, "tree_format must be 0 (best), 16 or 32");
    c->tree_format = v;
    route = true;
  } else if (k == "super_cull") {
    c->super_cull = v != 0;
    route = true;
  } else if (k == "tree_global") {
    c->force_global_tree = v != 0;
    route = true;
  } else if (k == "cluster_cull") {
    // 0: no cluster / chunk cull at all (every big-leaf cluster swept: exact by construction, whatever the
    // scene's margin); 1: the scene's margins (and masks)
    c->cull_scene = v != 0;
    if (v != 0) set_cull(c, c->cull);
    else fix_cull(c, __builtin_inff());
    cull = true;
  } else if (k == "cull_margin") {
    // > 0: one fixed margin coefficient for every level (no masks: not exact in general); 0: the scene's
    if (!(value >= 0.0)) return fail(KDPT_ERR_ARG, "cull_margin must be >= 0 (0: the scene's)");
    c->cull_scene = value == 0.0;
    if (value > 0.0) fix_cull(c, (float)value);
    else set_cull(c, c->cull);
    cull = true;
  } else if (k == "cull_exact") {
    // 0: the fast-margin one-level cull instead of the masked exact one (A/B; not exact for such scenes)
    c->cull_exact = v != 0;
    cull = true;
  } else if (k == "cull_fast_k") {
    // the masked cull's box coefficient (default CULL_MARGIN_MASKED), its direction masks rebuilt for it: a
    // wider box sweeps more clusters, a narrower one leaves more danger triangles to decide
    if (!(value > 0.0 && value < 1.0)) return fail(KDPT_ERR_ARG, "cull_fast_k must be in (0, 1)");
    if (!c->mask_cs) return fail(KDPT_ERR_ARG, "cull_fast_k: this scene has no direction masks");
    const CullMargin before = c->cull;
    c->cull.K = c->cull.K_lo = (float)value;
    if (c->cull_scene) set_cull(c, c->cull);
    int rc = build_masks(c, c->mask_n);
    if (rc) {  // the masks are still the old coefficient's: so is the margin again
      c->cull = before;
      if (c->cull_scene) set_cull(c, before);
      return rc;
    }
    cull = true;
  } else if (k == "cull_mask_n") {
    if (v < 1 || v > 512) return fail(KDPT_ERR_ARG, "cull_mask_n must be in 1 .. 512");
    if (!c->mask_cs) return fail(KDPT_ERR_ARG, "cull_mask_n: this scene has no direction masks");
    int rc = build_masks(c, v);
    if (rc) return rc;
    cull = true;
  } else if (k == "profile_batches") {
    c->profile_batches = v != 0;
    c->profile_steps = v >= 2;
  } else if (k == "sync_debug") {
    c->sync_debug = v != 0;
  } else if (k == "reduce_spin_us") {
    return set_reduce_spin(&c->reduce_spin_us, value);
  } else {
    return fail(KDPT_ERR_ARG, "unknown tuning knob " + k);
  }
  // (the route may change with the cull too: no super-cluster route under the masked cull)
  if (cull) apply_cull_route(c);
  return (cull || route) ? resetup_trace(c) : KDPT_OK;
}

int kdpt_reset(kdpt_ctx* c) {
  if (!c) return fail(KDPT_ERR_ARG, "null ctx");
  HIP_TRY(hipSetDevice(c->device));
  for (auto& grp : c->groups) HIP_TRY(hipStreamSynchronize(grp.stream));
  if (c->reduce_stream) HIP_TRY(hipStreamSynchronize(c->reduce_stream));
  drain_intersect_events(c);
  c->intersect_ms_total = 0;
  c->intersect_launches_total = 0;
  HIP_TRY(hipMemsetAsync(c->image, 0, sizeof(float) * 3 * (size_t)c->npix, c->stream));
  HIP_TRY(hipMemsetAsync(c->total_segments, 0, sizeof(unsigned long long), c->stream));
  HIP_TRY(hipMemsetAsync(c->trace_total, 0, 3 * sizeof(unsigned long long), c->stream));
  if (c->moments) HIP_TRY(hipMemsetAsync(c->mom_sumsq, 0, sizeof(float) * 3 * (size_t)c->npix, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  c->mom_samples = 0;
  c->accumulated = false;
  memset(&c->stats, 0, sizeof c->stats);
  c->stats.intersect_grid_share = 1.0f;
  c->cast_rays = c->cast_traced = 0;
  c->cast_ms = 0;
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
  for (auto& grp : c->groups) {
    HIP_TRY(hipStreamSynchronize(grp.stream));
    for (auto& it : grp.its) {
      int rc = check_fault(it.get(), grp.stream);
      if (rc) return rc;
    }
  }
  if (c->reduce_stream) HIP_TRY(hipStreamSynchronize(c->reduce_stream));
  unregister_host(c);
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
  HIP_TRY(hipMemcpyAsync(it.h_counts, it.counts, sizeof(int) * (c->cap + 3), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  if (it.h_counts[c->cap + 2]) return fault_error(&it, c->stream, it.h_counts[c->cap + 2]);
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

// Iterations first_iter + k * stride (k < count) in batches of `batch`, `pipeline` batches in flight, their
// partial images added into `target` (the context's image, or a frame buffer of kdpt_render_frames) in
// iteration order.  Each batch's add runs on the batch's own stream, after the previous batch's add (the one
// cross-stream wait of the pipeline, normally satisfied by the time it is reached): no stream ever waits for a
// whole batch, so none holds an in-order hardware queue that batch streams share (HIP multiplexes a process's
// streams onto GPU_MAX_HW_QUEUES queues, 4 by default).  zero_after: the target is first zeroed, after that
// event (a frame buffer after its previous reduce).  Returns once everything is queued.
int enqueue_iterations(kdpt_ctx* c, int first_iter, int count, int stride, int pipeline, int batch, float* target,
                       hipEvent_t zero_after = nullptr) {
  if (c->shade_oob) return refuse_shading();
  const int depth = std::min(16, std::max(1, pipeline));
  const int B = std::min(MAXB, std::max(1, batch));
  // the first add follows everything already queued on the context's own stream (reset, ...); a wait of an
  // earlier call that is still queued keeps the record it was queued after
  const hipEvent_t entry = c->entry_ev;
  HIP_TRY(hipEventRecord(entry, c->stream));
  // `depth` groups of B iteration states; a group runs one batch at a time on its stream
  if ((int)c->groups.size() < depth || c->group_batch != B) {
    if (!c->groups.empty()) {
      int rc = kdpt_synchronize(c);
      if (rc) return rc;
      drop_groups(c);
    }
    c->group_batch = B;
    c->next_group = 0;
    // One stream per group, created one after another in group order: HIP maps streams onto its hardware
    // queues (GPU_MAX_HW_QUEUES) in creation order, reusing the least-used queue once all exist, so a stream per
    // iteration state (8 x 4) had put pairs of groups -- two batches' chains -- on one in-order queue.
    while ((int)c->groups.size() < depth) {
      int rc = make_group(c, B);
      if (rc) {
        drop_groups(c);
        return rc;
      }
    }
  }
  const int ngroups = (int)c->groups.size();
  // With several batches in flight each intersect launch gets a share of the chip (2/depth of the
  // persistent grid, all of it for depth <= 2, a quarter from depth 8 on): a launch's length is set by its
  // heaviest rays, so concurrent launches on disjoint CU subsets overlap those tails instead of queueing
  // behind them.  (Sweep with every batch on its own hardware queue: a quarter is best at depths 8-12.)
  const int trace_grid =
      c->grid_env ? c->trace_grid : std::max(1, c->trace_grid * 2 / std::min(8, std::max(2, depth)));
  c->stats.intersect_grid_share = (float)trace_grid / (float)std::max(1, c->full_trace_grid);
  // diagnostic ("profile_batches" knob): the counting intersect kernel (kdpt_wave_profile after sync)
  if (c->profile_batches) HIP_TRY(hipMemsetAsync(c->counters, 0, sizeof(Counters), c->stream));
  bool first = true;
  for (int kb = 0; kb < count; kb += B) {
    const int nb = std::min(B, count - kb);
    // groups in turn, continuing across calls: kdpt_render_frames queues one call per frame, and a frame
    // shorter than the pipeline must not restart at group 0 (it would wait on that group's previous batch)
    const int g = c->next_group % ngroups;
    c->next_group = (g + 1) % ngroups;
    IterGroup& grp = c->groups[g];
    hipStream_t st = grp.stream;
    // (the group's previous batch's partial images were added on this stream, before this batch's camera rays
    // clear them)
    int iters[MAXB];
    IterState* its[MAXB];
    for (int b = 0; b < nb; b++) {
      iters[b] = first_iter + (kb + b) * stride;
      its[b] = grp.its[b].get();
    }
    std::vector<hipEvent_t>* bev = nullptr;
    if (c->opt.testing_mode) {
      std::vector<hipEvent_t> evs;
      for (int e = 0; e < 2 * c->cap; e++) {
        hipEvent_t ev;
        if (!c->free_ev.empty()) { ev = c->free_ev.back(); c->free_ev.pop_back(); }
        else HIP_TRY(hipEventCreate(&ev));
        evs.push_back(ev);
      }
      c->pending_ev.push_back(evs);
      bev = &c->pending_ev.back();
    }
    int rc = launch_batch(c, its, iters, nb, st, trace_grid, -1, c->profile_batches, bev);
    if (rc) return rc;
    // the add: after the previous add (the chain), and for the call's first batch after the context's stream,
    // the frames' image adds (when the target is the image) and the target's zeroing
    if (c->acc_last) HIP_TRY(hipStreamWaitEvent(st, c->acc_last, 0));
    if (first) {
      HIP_TRY(hipStreamWaitEvent(st, entry, 0));
      if (c->img_last && target == c->image) HIP_TRY(hipStreamWaitEvent(st, c->img_last, 0));
      if (zero_after) {
        HIP_TRY(hipStreamWaitEvent(st, zero_after, 0));
        HIP_TRY(hipMemsetAsync(target, 0, sizeof(float) * 3 * (size_t)c->npix, st));
      }
      first = false;
    }
    const float* partials[MAXB];
    for (int b = 0; b < nb; b++) partials[b] = its[b]->image;  // in iteration order
    if ((rc = launch_accumulate(c, target, partials, nb, st))) return rc;
    HIP_TRY(hipEventRecord(grp.acc_ev, st));
    c->acc_last = grp.acc_ev;
    if (target == c->image) {
      c->accumulated = true;
      if (c->moments) c->mom_samples += nb;
    }
  }
  c->stats.iterations += count;
  return KDPT_OK;
}

int kdpt_trace_iterations(kdpt_ctx* c, int frame, int first_iter, int count, int stride, int pipeline, int batch) {
  (void)frame;
  if (!c || count < 0 || first_iter < 1 || stride < 1) return fail(KDPT_ERR_ARG, "bad arguments");
  HIP_TRY(hipSetDevice(c->device));
  return enqueue_iterations(c, first_iter, count, stride, pipeline, batch, c->image);
}

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
    if (margin) *margin = c->chunk_k_min;
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
  hipPointerAttribute_t attr{};
  const bool on_device = hipPointerGetAttributes(&attr, rgba) == hipSuccess && attr.type == hipMemoryTypeDevice &&
                         attr.device == c->device;
  (void)hipGetLastError();  // a plain host pointer is an error for hipPointerGetAttributes on some runtimes
  uchar4* d = reinterpret_cast<uchar4*>(rgba);
  if (!on_device) {
    if (!c->pbo_staging) HIP_TRY(hipMalloc((void**)&c->pbo_staging, sizeof(uchar4) * (size_t)c->npix));
    d = c->pbo_staging;
  }
  hipLaunchKernelGGL(k_pbo, dim3((c->npix + 255) / 256), dim3(256), 0, c->stream, c->image, c->npix, iter, d);
  HIP_TRY(hipGetLastError());
  if (!on_device)
    HIP_TRY(hipMemcpyAsync(rgba, d, sizeof(uchar4) * (size_t)c->npix, hipMemcpyDefault, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return KDPT_OK;
}

// The saveImage pixel pass on the device; rgb (host, 3*W*H) and/or lin (host, 3*W*H floats).
static int save_image_pass(kdpt_ctx* c, float samples, uint8_t* rgb, float* lin) {
  HIP_TRY(hipSetDevice(c->device));
  for (auto& grp : c->groups) HIP_TRY(hipStreamSynchronize(grp.stream));
  if (c->reduce_stream) HIP_TRY(hipStreamSynchronize(c->reduce_stream));
  const size_t n3 = 3 * (size_t)c->npix;
  uint8_t* d_rgb = nullptr;
  float* d_lin = nullptr;
  HIP_TRY(hipMalloc((void**)&d_rgb, n3));
  hipError_t e = lin ? hipMalloc((void**)&d_lin, n3 * sizeof(float)) : hipSuccess;
  if (e != hipSuccess) {
    (void)hipFree(d_rgb);
    return hip_fail("save image: hipMalloc", e);
  }
  hipLaunchKernelGGL(k_save_image, dim3((c->npix + 255) / 256), dim3(256), 0, c->stream, c->image, c->W, c->H,
                     samples, d_rgb, d_lin);
  e = hipGetLastError();
  if (e == hipSuccess && rgb) e = hipMemcpyAsync(rgb, d_rgb, n3, hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess && lin) e = hipMemcpyAsync(lin, d_lin, n3 * sizeof(float), hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  (void)hipFree(d_rgb);
  if (d_lin) (void)hipFree(d_lin);
  return e == hipSuccess ? KDPT_OK : hip_fail("save image", e);
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
  *mask_n = c->mask_dev ? c->mask_n : 0;
  *num_clusters = c->S.num_clusters;
  if (!c->mask_dev) return KDPT_OK;
  const size_t cells = 6 * (size_t)c->mask_n * c->mask_n * (size_t)c->S.num_clusters;
  HIP_TRY(hipStreamSynchronize(c->stream));
  if (masks)
    HIP_TRY(hipMemcpyAsync(masks, c->mask_dev, cells * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
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
  c->stats.mask_build_ms = c->mask_build_ms;
  *st = c->stats;
  return KDPT_OK;
}

int kdpt_image_device_ptr(kdpt_ctx* c, void** p) {
  if (!c || !p) return fail(KDPT_ERR_ARG, "null arg");
  *p = c->image;
  return KDPT_OK;
}

int kdpt_destroy(kdpt_ctx* c) {
  if (!c) return KDPT_OK;
  (void)hipSetDevice(c->device);
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  drop_groups(c);  // (each group's stream drained first)
  for (auto& evs : c->pending_ev)
    for (auto e : evs) (void)hipEventDestroy(e);
  for (auto e : c->free_ev) (void)hipEventDestroy(e);
  // (a kdpt_render_frames that failed partway may have left a reduce queued: drain it before the communicator
  // and the frame buffers go)
  if (c->reduce_stream) (void)hipStreamSynchronize(c->reduce_stream);
  release_comm(c);
  unregister_host(c);
  for (auto e : c->frame_ev)
    if (e) (void)hipEventDestroy(e);
  if (c->reduce_stream) (void)hipStreamDestroy(c->reduce_stream);
  for (void* p : c->allocs) (void)hipFree(p);
  if (c->pbo_staging) (void)hipFree(c->pbo_staging);
  free_moments(c);
  free_cast_buffers(c);
  for (auto e : c->cast_ev)
    if (e) (void)hipEventDestroy(e);
  free_iter(&c->solo);
  free_iter(&c->query);  // (its image, staging buffer and totals were among c->allocs)
  if (c->entry_ev) (void)hipEventDestroy(c->entry_ev);
  if (c->stream) (void)hipStreamDestroy(c->stream);
  delete c;
  return KDPT_OK;
}

int kdpt_debug_paths(kdpt_ctx* c, int iter, int stop_depth, kdpt_path_segment* out, int* npaths) {
  if (!c || !out || stop_depth < 0 || stop_depth >= c->cap) return fail(KDPT_ERR_ARG, "bad arg");
  HIP_TRY(hipSetDevice(c->device));
  IterState& it = c->solo;
  ScratchTargets targets(it);
  int rc = targets.redirect(c);
  if (rc || (rc = launch_iteration(c, iter, stop_depth, false))) return rc;
  kdpt_path_segment* d = nullptr;
  HIP_TRY(hipMalloc((void**)&d, sizeof(kdpt_path_segment) * (size_t)c->npix));
  std::unique_ptr<void, DeviceFree> d_owner(d);
  const int depth_slot = stop_depth + 1;
  hipLaunchKernelGGL(k_unpack, dim3((c->npix + 255) / 256), dim3(256), 0, c->stream, it.buf[it.cur], it.counts,
                     depth_slot, d);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(it.h_counts, it.counts, sizeof(int) * (c->cap + 2), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  if ((rc = check_fault(&it, c->stream))) return rc;
  const int n = it.h_counts[depth_slot];
  *npaths = n;
  HIP_TRY(hipMemcpy(out, d, sizeof(kdpt_path_segment) * (size_t)n, hipMemcpyDeviceToHost));
  return KDPT_OK;
}

// Roofline counters: one extra (untimed) iteration with per-path AABB/triangle/hit counts.
int kdpt_count_iteration(kdpt_ctx* c, int iter, unsigned long long* aabb_tri_hit) {
  if (!c || !aabb_tri_hit) return fail(KDPT_ERR_ARG, "null arg");
  HIP_TRY(hipSetDevice(c->device));
  IterState& it = c->solo;
  ScratchTargets targets(it);
  int rc = targets.redirect(c);
  if (rc) return rc;
  HIP_TRY(hipMemsetAsync(c->counters, 0, sizeof(Counters), c->stream));
  rc = launch_iteration(c, iter, -1, true);
  Counters h{};
  if (!rc) {
    HIP_TRY(hipMemcpyAsync(&h, c->counters, sizeof h, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(it.h_counts, it.counts, sizeof(int) * (c->cap + 3), hipMemcpyDeviceToHost, c->stream));
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

int kdpt_selftest_math(const float* x, int n, float* so, float* co) {
  float *dx, *ds, *dc;
  HIP_TRY(hipMalloc((void**)&dx, sizeof(float) * n));
  HIP_TRY(hipMalloc((void**)&ds, sizeof(float) * n));
  HIP_TRY(hipMalloc((void**)&dc, sizeof(float) * n));
  HIP_TRY(hipMemcpy(dx, x, sizeof(float) * n, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(k_selftest_math, dim3((n + 255) / 256), dim3(256), 0, 0, dx, n, ds, dc);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpy(so, ds, sizeof(float) * n, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(co, dc, sizeof(float) * n, hipMemcpyDeviceToHost));
  (void)hipFree(dx); (void)hipFree(ds); (void)hipFree(dc);
  return KDPT_OK;
}

int kdpt_selftest_libm(int fn, const float* x, int n, double* out) {
  if (fn < 0 || fn > 2 || n < 0 || (n && (!x || !out))) return fail(KDPT_ERR_ARG, "kdpt_selftest_libm: bad arguments");
  if (n == 0) return KDPT_OK;
  float* dx;
  double* dout;
  HIP_TRY(hipMalloc((void**)&dx, sizeof(float) * n));
  HIP_TRY(hipMalloc((void**)&dout, sizeof(double) * n));
  HIP_TRY(hipMemcpy(dx, x, sizeof(float) * n, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(k_selftest_libm, dim3((n + 255) / 256), dim3(256), 0, 0, fn, dx, n, dout);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpy(out, dout, sizeof(double) * n, hipMemcpyDeviceToHost));
  (void)hipFree(dx); (void)hipFree(dout);
  return KDPT_OK;
}

int kdpt_selftest_libm_digest(int fn, uint32_t first, unsigned long long count, unsigned long long* digest) {
  if (fn < 0 || fn > 2 || !digest || count > (1ull << 32) || first + count > (1ull << 32))
    return fail(KDPT_ERR_ARG, "kdpt_selftest_libm_digest: bad arguments");
  unsigned long long* dacc;
  HIP_TRY(hipMalloc((void**)&dacc, sizeof(unsigned long long)));
  HIP_TRY(hipMemset(dacc, 0, sizeof(unsigned long long)));
  hipLaunchKernelGGL(k_selftest_libm_digest, dim3(4096), dim3(256), 0, 0, fn, first, (uint64_t)count, dacc);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpy(digest, dacc, sizeof(unsigned long long), hipMemcpyDeviceToHost));
  (void)hipFree(dacc);
  return KDPT_OK;
}

int kdpt_selftest_rng(const int* iid, int n, int k, float* u) {
  int* di;
  float* du;
  HIP_TRY(hipMalloc((void**)&di, sizeof(int) * 3 * n));
  HIP_TRY(hipMalloc((void**)&du, sizeof(float) * n));
  HIP_TRY(hipMemcpy(di, iid, sizeof(int) * 3 * n, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(k_selftest_rng, dim3((n + 255) / 256), dim3(256), 0, 0, di, n, k, du);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpy(u, du, sizeof(float) * n, hipMemcpyDeviceToHost));
  (void)hipFree(di); (void)hipFree(du);
  return KDPT_OK;
}

int kdpt_selftest_rng_draws(int mode, const uint32_t* in, int n, int k, float* out) {
  if (mode < 0 || mode > 2 || n < 0 || k < 0 || (n && k && (!in || !out)))
    return fail(KDPT_ERR_ARG, "bad rng selftest arguments");
  if (!n || !k) return KDPT_OK;
  const size_t nin = (size_t)n * (mode == 0 ? 3 : 1), nout = (size_t)n * k;
  uint32_t* di;
  float* dout;
  HIP_TRY(hipMalloc((void**)&di, sizeof(uint32_t) * nin));
  if (const hipError_t e = hipMalloc((void**)&dout, sizeof(float) * nout)) {
    (void)hipFree(di);
    return hip_fail("rng selftest: hipMalloc", e);
  }
  hipError_t e = hipMemcpy(di, in, sizeof(uint32_t) * nin, hipMemcpyHostToDevice);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(k_selftest_rng_draws, dim3((n + 255) / 256), dim3(256), 0, 0, mode, di, n, k, dout);
    if ((e = hipGetLastError()) == hipSuccess) e = hipMemcpy(out, dout, sizeof(float) * nout, hipMemcpyDeviceToHost);
  }
  (void)hipFree(di);
  (void)hipFree(dout);
  return e == hipSuccess ? KDPT_OK : hip_fail("rng selftest", e);
}

int kdpt_selftest_glm(int fn, const float* in, int n, float* out) {
  const int ni = glm_kat_inputs(fn), no = glm_kat_outputs(fn);
  if (!ni || n < 0 || (n && (!in || !out))) return fail(KDPT_ERR_ARG, "bad glm selftest arguments");
  if (!n) return KDPT_OK;
  float *din, *dout;
  HIP_TRY(hipMalloc((void**)&din, sizeof(float) * ni * (size_t)n));
  HIP_TRY(hipMalloc((void**)&dout, sizeof(float) * no * (size_t)n));
  HIP_TRY(hipMemcpy(din, in, sizeof(float) * ni * (size_t)n, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(dout, out, sizeof(float) * no * (size_t)n, hipMemcpyHostToDevice));  // sentinels
  hipLaunchKernelGGL(k_selftest_glm, dim3((n + 255) / 256), dim3(256), 0, 0, fn, din, n, dout);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpy(out, dout, sizeof(float) * no * (size_t)n, hipMemcpyDeviceToHost));
  (void)hipFree(din); (void)hipFree(dout);
  return KDPT_OK;
}

int kdpt_selftest_fresnel(const float* cs, int n, float ior, float* f) {
  float *dc, *df;
  HIP_TRY(hipMalloc((void**)&dc, sizeof(float) * n));
  HIP_TRY(hipMalloc((void**)&df, sizeof(float) * n));
  HIP_TRY(hipMemcpy(dc, cs, sizeof(float) * n, hipMemcpyHostToDevice));
  float rr = (1.0f - ior) / (1.0f + ior);
  hipLaunchKernelGGL(k_selftest_fresnel, dim3((n + 255) / 256), dim3(256), 0, 0, dc, n, rr * rr, df);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpy(f, df, sizeof(float) * n, hipMemcpyDeviceToHost));
  (void)hipFree(dc); (void)hipFree(df);
  return KDPT_OK;
}

}  // extern "C"

namespace {

// grid: the launch's persistent workgroups (c->trace_grid, or a pipelined call's share of it); tree_lds is 0 on
// the routes that read the tree from HBM
void launch_trace(kdpt_ctx* c, const TraceArgs& a, bool count, int grid, hipStream_t st) {
  const TraceKernel k = trace_kernel(c->opt.short_stack != 0, count, c->tree_mode);
  hipLaunchKernelGGL(k.fn, dim3(grid), dim3(k.block), c->tree_lds, st, a);
}

// The fault word is the one per-iteration member of DevScene: the batch-wide launches (camera rays + geoms,
// k_geoms, k_trace) report into the first state's word (Batch::S0), each iteration's own launches into its own.
DevScene scene_of(const kdpt_ctx* c, const IterState* it) {
  DevScene S = c->S;
  S.fault = it->fault;
  return S;
}

// What stays the same over a launch_batch call: its arguments and what follows from them and the context.
struct Batch {
  kdpt_ctx* c;
  IterState* const* its;
  const int* iters;
  int nb;
  hipStream_t st;
  int trace_grid;
  bool count;
  DevScene S0;      // scene_of the first state
  bool gen_geoms;   // camera rays and bounce 0's analytic geoms + root-box test in one launch (not for the
                    // brute-force and box-view intersect kernels, which have no first part)
  bool compact;
  ShadeArgs shade;  // the shading arguments that neither the bounce nor the iteration changes
  const RaySource* rays = nullptr;  // a ray query's batch (nb = 1): bounce 0 loads these instead of the camera's
  unsigned long long* trace_total = nullptr;  // the intersect totals the shading adds to (the context's, or the query's)
};

// The camera-ray launch's arguments but for the iteration records: the context's current camera and options.
// (ncounts, nwork, nlb: the lengths of the counters, work counters and look-back records the launch zeroes)
GenBatch gen_batch(const kdpt_ctx* c) {
  return GenBatch{{}, c->cam, c->traceDepth, c->opt.antialias, c->cap + 2, c->cap, c->cap * c->ntiles,
                  c->opt.focal_length, c->opt.dof_angle};
}

// A ray query's bounce 0: its rays loaded into the state's paths (k_user_rays_b), with bounce 0's geoms stage when
// gen_geoms (k_user_geoms_b).  The grid covers the rays, not the image.
int user_rays_stage(const Batch& B) {
  kdpt_ctx* c = B.c;
  IterState* it = B.its[0];
  it->cur = 0;
  const UserBatch ub{it->gen_iter(B.iters[0]), B.rays->rays, c->traceDepth, c->cap + 2, c->cap, c->cap * c->ntiles};
  const dim3 grid((ub.src.n + GEN_BLOCK - 1) / GEN_BLOCK);
  if (B.gen_geoms) {
    const UserGeomsBatch ug{ub, B.S0, it->gen_geoms_iter(), B.count ? c->counters : nullptr};
    hipLaunchKernelGGL(k_user_geoms_b, grid, dim3(GEN_BLOCK), 0, B.st, ug);
  } else {
    hipLaunchKernelGGL(k_user_rays_b, grid, dim3(GEN_BLOCK), 0, B.st, ub);
  }
  HIP_TRY(hipGetLastError());
  return KDPT_OK;
}

// The batch's camera rays in one launch (blockIdx.y = iteration), with bounce 0's geoms stage when gen_geoms.
int camera_stage(const Batch& B) {
  if (B.rays) return user_rays_stage(B);
  kdpt_ctx* c = B.c;
  GenBatch gb = gen_batch(c);
  for (int b = 0; b < B.nb; b++) {
    B.its[b]->cur = 0;
    gb.it[b] = B.its[b]->gen_iter(c->opt.cacherays ? 1 : B.iters[b]);
  }
  if (B.gen_geoms) {
    GenGeomsBatch gg{gb, B.S0, {}, B.count ? c->counters : nullptr};
    for (int b = 0; b < B.nb; b++) gg.it[b] = B.its[b]->gen_geoms_iter();
    hipLaunchKernelGGL(k_gen_geoms_b, dim3((c->npix + GEN_BLOCK - 1) / GEN_BLOCK, B.nb), dim3(GEN_BLOCK), 0, B.st,
                       gg);
  } else {
    hipLaunchKernelGGL(k_gen_rays_b, dim3((c->npix + 255) / 256, B.nb), dim3(256), 0, B.st, gb);
  }
  HIP_TRY(hipGetLastError());
  return KDPT_OK;
}

// enable_kd = 0: one k_brute launch per iteration.
int brute_stage(const Batch& B, int depth) {
  kdpt_ctx* c = B.c;
  const BruteKernel kernel = brute_kernel(c->opt.use_bbox != 0, B.count);
  for (int b = 0; b < B.nb; b++) {
    IterState* it = B.its[b];
    const BruteArgs ba{scene_of(c, it), it->buf[it->cur], it->counts, depth, it->hits, c->shapes, c->num_shapes,
                       c->chunk_lo, c->chunk_hi, c->cull_scene ? 0.0f : c->S.cl_margin, c->counters,
                       B.its[0]->trace_t};
    hipLaunchKernelGGL(kernel, dim3(c->ntiles), dim3(TILE), 0, B.st, ba);
    HIP_TRY(hipGetLastError());
    if (c->sync_debug) {
      BruteShape h0;
      HIP_TRY(hipStreamSynchronize(B.st));  // (the null-stream copy below does not order after st)
      HIP_TRY(hipMemcpy(&h0, c->shapes, sizeof h0, hipMemcpyDeviceToHost));
      fprintf(stderr, "[kdpt] brute depth %d use_bbox %d shapes %d lo %g %g %g hi %g %g %g n %d mat %d\n", depth,
              c->opt.use_bbox, c->num_shapes, h0.lo.x, h0.lo.y, h0.lo.z, h0.hi.x, h0.hi.y, h0.hi.z, fbits(h0.lo.w),
              fbits(h0.hi.w));
    }
  }
  return KDPT_OK;
}

// Bounce `depth`'s intersect kernel: k_viz or k_brute per iteration, else one k_trace over the whole batch,
// after the intersect stage's first part (k_geoms_b) unless the camera stage (bounce 0 with gen_geoms) or the
// previous bounce's shading (prep_ready: the hand-off) has done it already.
int intersect_stage(const Batch& B, int depth, bool prep_ready) {
  kdpt_ctx* c = B.c;
  IterState* it0 = B.its[0];
  if (c->viz) {
    for (int b = 0; b < B.nb; b++) {
      IterState* it = B.its[b];
      hipLaunchKernelGGL(k_viz, dim3(c->ntiles), dim3(TILE), 0, B.st, scene_of(c, it), it->buf[it->cur], it->counts,
                         depth, it->hits, it0->trace_t);
      HIP_TRY(hipGetLastError());
    }
    return KDPT_OK;
  }
  if (c->brute) return brute_stage(B, depth);
  if (!prep_ready && !(depth == 0 && B.gen_geoms)) {  // the batch's iterations in one launch (blockIdx.y = iteration)
    GeomsBatch gb{B.S0, {}, depth, B.count ? c->counters : nullptr, it0->trace_t + 2 * c->cap};
    for (int b = 0; b < B.nb; b++) gb.it[b] = B.its[b]->geoms_iter();
    hipLaunchKernelGGL(k_geoms_b, dim3((c->npix + GEN_BLOCK - 1) / GEN_BLOCK, B.nb), dim3(GEN_BLOCK), 0, B.st, gb);
    HIP_TRY(hipGetLastError());
  }
  TraceArgs t{B.S0, {}, B.nb, c->profile_steps ? 1 : 0, it0->work, depth, c->counters, it0->trace_t};
  for (int b = 0; b < MAXB; b++) t.it[b] = B.its[b < B.nb ? b : 0]->trace_iter(depth, B.gen_geoms);
  launch_trace(c, t, B.count, B.trace_grid, B.st);
  HIP_TRY(hipGetLastError());
  return KDPT_OK;
}

// Iteration b's shading arguments at bounce `depth`: the batch's base, then what the bounce and the state set.
ShadeArgs shade_args(const Batch& B, int b, int depth, bool prep_next) {
  const IterState* it = B.its[b];
  ShadeArgs a = B.shade;
  a.S.fault = it->fault;
  a.paths = it->buf[it->cur];
  a.hits = it->hits;
  a.image = it->image;
  a.image_zeroed = it->zero_partial ? 1 : 0;
  a.counts = it->counts;
  a.depth = depth;
  a.iter = B.iters[b];
  a.tile_counts = it->tile_counts;
  a.total_segments = it->total_segments;
  a.trace_total = b == 0 ? B.trace_total : nullptr;
  a.ccount = it->cand_count(depth, B.gen_geoms);
  a.prep_on = prep_next ? 1 : 0;
  a.prep = it->prep;
  a.tile_ccounts = it->tile_ccounts;
  return a;
}

// The three-kernel route of one iteration (iteration 2's sort, "shade_fused" = 0, compaction = 0): k_shade, then
// k_scan + k_scatter into the other path buffer, or with neither compaction nor sort the live count copied on.
int shade_scan_scatter(const Batch& B, IterState* it, const ShadeArgs& a, bool sort, bool prep_next) {
  kdpt_ctx* c = B.c;
  const int depth = a.depth;
  hipLaunchKernelGGL(shade_kernel(hybrid_shading(c), B.compact, sort), dim3(c->ntiles), dim3(TILE), 0, B.st, a);
  HIP_TRY(hipGetLastError());
  if (!B.compact && !sort) {  // the live range stays the whole image
    HIP_TRY(hipMemcpyAsync(it->counts + depth + 1, it->counts + depth, sizeof(int), hipMemcpyDeviceToDevice, B.st));
    return KDPT_OK;
  }
  // survivors' offsets + the next bounce's path count; with the hand-off also the candidate-list
  // offsets per tile + the next bounce's candidate count (a second workgroup)
  const ScanJob j0{it->tile_counts, it->tile_off, sort ? c->nkeys : 1, it->counts + depth + 1};
  const ScanJob j1{it->tile_ccounts, it->tile_coff, 1, it->ccount + depth + 1};
  hipLaunchKernelGGL(k_scan, dim3(prep_next ? 2 : 1), dim3(SCAN_TB), 0, B.st, j0, j1, it->counts, depth, c->ntiles);
  HIP_TRY(hipGetLastError());
  const auto scatter = sort ? k_scatter<true> : k_scatter<false>;
  hipLaunchKernelGGL(scatter, dim3(c->ntiles), dim3(TILE), 0, B.st, it->buf[it->cur], it->buf[it->cur ^ 1],
                     it->tile_off, it->counts, depth, c->ntiles, B.compact ? 1 : 0, it->scatter_prep(prep_next));
  HIP_TRY(hipGetLastError());
  it->cur ^= 1;
  return KDPT_OK;
}

// Bounce `depth`'s shading of every iteration: the single pass (k_shade_fused: shading, compaction into the other
// buffer and the hand-off), the batch's in one launch unless "shade_batch" = 0; the three-kernel route for
// iteration 2, "shade_fused" = 0 and compaction = 0.
int shade_stage(const Batch& B, int depth, bool prep_next) {
  kdpt_ctx* c = B.c;
  const bool hyb = hybrid_shading(c);
  const bool stage = shade_staged(c);
  const int shade_grid = (c->npix + SHADE_TB - 1) / SHADE_TB;
  ShadeBatch sbatch;
  int nfused = 0;
  for (int b = 0; b < B.nb; b++) {
    IterState* it = B.its[b];
    const bool sort = (B.iters[b] == 2);
    const ShadeArgs a = shade_args(B, b, depth, prep_next);
    if (!B.compact || sort || c->no_fuse) {
      int rc = shade_scan_scatter(B, it, a, sort, prep_next);
      if (rc) return rc;
      continue;
    }
    const FuseArgs f = it->fuse_args();
    if (c->shade_batch) {  // launched below, with the batch's other fused iterations
      sbatch.a[nfused] = a;
      sbatch.f[nfused] = f;
      nfused++;
    } else {
      hipLaunchKernelGGL(shade_fused_kernel(hyb, stage), dim3(shade_grid), dim3(SHADE_TB), 0, B.st, a, f);
      HIP_TRY(hipGetLastError());
    }
    it->cur ^= 1;
  }
  if (nfused) {
    hipLaunchKernelGGL(shade_fused_batch_kernel(hyb, stage), dim3(shade_grid, nfused), dim3(SHADE_TB), 0, B.st,
                       sbatch);
    HIP_TRY(hipGetLastError());
  }
  return KDPT_OK;
}

// One iteration in each state of its (nb <= MAXB), with the context's scene, options and knobs, in lockstep on
// stream st: per bounce the analytic geoms of each, one intersect launch of trace_grid workgroups over all of
// them, then each one's shading and compaction.  The iterations stay independent: only the intersect launch is
// shared.
int launch_batch(kdpt_ctx* c, IterState* const* its, const int* iters, int nb, hipStream_t st, int trace_grid,
                 int stop_depth, bool count, std::vector<hipEvent_t>* bev, const RaySource* rays) {
  if (c->shade_oob) return refuse_shading();
  const bool kd = !c->brute && !c->viz;
  Batch B{c, its, iters, nb, st, trace_grid, count, scene_of(c, its[0]), c->gen_geoms && kd, c->opt.compaction != 0,
          ShadeArgs{}, rays, rays ? rays->trace_total : c->trace_total};
  B.shade.S = c->S;
  B.shade.softness = c->opt.softness;
  B.shade.enable_sss = c->opt.enable_sss;
  B.shade.tile_kcounts = nullptr;
  B.shade.ntiles = c->ntiles;
  B.shade.nkeys = c->nkeys;
  B.shade.trace_t = its[0]->trace_t;
  B.shade.gspan = its[0]->trace_t + 2 * c->cap;
  B.shade.trace_rays = kd ? B.trace_total + 2 : nullptr;
  B.shade.count_aabb = count ? c->counters : nullptr;
  int rc = camera_stage(B);
  if (rc) return rc;
  const bool timed = c->opt.testing_mode && bev;
  bool prep_ready = false;  // this bounce's intersect-stage first part came with the previous bounce's shading
  for (int depth = 0; depth < c->cap; depth++) {
    const bool prep_next = B.compact && depth + 1 < c->cap && kd;
    if (timed) HIP_TRY(hipEventRecord((*bev)[2 * depth], st));
    if ((rc = intersect_stage(B, depth, prep_ready))) return rc;
    if (c->sync_debug) {
      fprintf(stderr, "[kdpt] trace depth %d launched (grid %d, mode %d, lds %zu, batch %d)\n", depth,
              trace_grid, c->tree_mode, c->tree_lds, nb);
      HIP_TRY(hipStreamSynchronize(st));
      fprintf(stderr, "[kdpt] trace depth %d done\n", depth);
    }
    if (timed) HIP_TRY(hipEventRecord((*bev)[2 * depth + 1], st));
    if ((rc = shade_stage(B, depth, prep_next))) return rc;
    if (c->sync_debug) {
      HIP_TRY(hipStreamSynchronize(st));
      fprintf(stderr, "[kdpt] shade depth %d done\n", depth);
    }
    if (stop_depth == depth) return KDPT_OK;
    prep_ready = prep_next;
  }
  if (!B.compact) {
    for (int b = 0; b < nb; b++) {
      IterState* it = its[b];
      hipLaunchKernelGGL(k_final_gather, dim3((c->npix + 255) / 256), dim3(256), 0, st, it->buf[it->cur], it->counts,
                         c->cap, it->image);
      HIP_TRY(hipGetLastError());
    }
  }
  return KDPT_OK;
}

// One iteration in the solo state, on the context's stream with the whole intersect grid.
int launch_iteration(kdpt_ctx* c, int iter, int stop_depth, bool count) {
  int rc = join_accum(c);
  if (rc) return rc;
  IterState* it = &c->solo;
  return launch_batch(c, &it, &iter, 1, c->stream, c->trace_grid, stop_depth, count, &it->bounce_ev);
}

// kdpt_trace_iteration[_async]: one whole iteration of the solo state added to the image.  With moments off the
// state gathers straight into the image; with moments on into the context's partial image (mom_partial, which the
// camera kernel clears as it clears the pipeline states'), added to the image and to the second moments on the
// same stream at nb = 1.
int accumulate_iteration(kdpt_ctx* c, int iter) {
  int rc = launch_iteration(c, iter, -1, false);
  if (rc) return rc;
  c->accumulated = true;
  if (!c->moments) return KDPT_OK;
  const float* partial = c->mom_partial;
  if ((rc = launch_accumulate(c, c->image, &partial, 1, c->stream))) return rc;
  c->mom_samples++;
  return KDPT_OK;
}

}  // namespace

// ---------------------------------------------------------------------------
// Multi-GPU: samples per pixel sharded across GPUs (the reference renders one GPU's
// iterations in pathtrace(), src/pathtrace.cu:2405-2635).  Frame f covers global iterations f * spp + 1 ..
// (f + 1) * spp; rank r of N renders those with (iteration - 1 - f * spp) % N == r, in order, into its frame
// buffer, and one reduce (sum, to rank 0) per frame combines them -- the path's only exchange step.  Every
// iteration-dependent behaviour (RNG seeds, iteration 2's sort, cacherays) uses the global numbers.
//
// The reduce is RCCL's (ncclReduce over xGMI, one communicator rank per context; multi-process:
// kdpt_comm_init, one process per GPU) or, inside one process (kdpt_render_sharded), either RCCL
// (ncclCommInitAll) or a peer-copy reduce on device 0 that adds the ranks' frames in rank order (also usable
// with several contexts on one device, which RCCL refuses).  RCCL is loaded at run time (dlopen): the library
// has no link-time dependency on it, and a process that already holds it (torch) shares that copy.  Each
// context queues its frames' reduces and rank 0's image adds on a reduce stream of its own, which waits for
// the frame's last add (the batch streams' add chain), so frames stay in flight: frame f + 1's iterations run
// while frame f is reduced.
// ---------------------------------------------------------------------------
namespace {

struct Rccl {
  ncclResult_t (*getUniqueId)(ncclUniqueId*);
  ncclResult_t (*commInitRank)(ncclComm_t*, int, ncclUniqueId, int);
  ncclResult_t (*commInitAll)(ncclComm_t*, int, const int*);
  ncclResult_t (*commDestroy)(ncclComm_t);
  ncclResult_t (*reduce)(const void*, void*, size_t, ncclDataType_t, ncclRedOp_t, int, ncclComm_t, hipStream_t);
  ncclResult_t (*groupStart)();
  ncclResult_t (*groupEnd)();
  const char* (*errorString)(ncclResult_t);
};

const Rccl* rccl() {
  static std::once_flag once;
  static Rccl r{};
  static bool ok = false;
  std::call_once(once, [] {
    void* h = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
    if (!h) h = dlopen("/opt/rocm/lib/librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
    if (!h) return;
    r.getUniqueId = (decltype(r.getUniqueId))dlsym(h, "ncclGetUniqueId");
    r.commInitRank = (decltype(r.commInitRank))dlsym(h, "ncclCommInitRank");
    r.commInitAll = (decltype(r.commInitAll))dlsym(h, "ncclCommInitAll");
    r.commDestroy = (decltype(r.commDestroy))dlsym(h, "ncclCommDestroy");
    r.reduce = (decltype(r.reduce))dlsym(h, "ncclReduce");
    r.groupStart = (decltype(r.groupStart))dlsym(h, "ncclGroupStart");
    r.groupEnd = (decltype(r.groupEnd))dlsym(h, "ncclGroupEnd");
    r.errorString = (decltype(r.errorString))dlsym(h, "ncclGetErrorString");
    ok = r.getUniqueId && r.commInitRank && r.commInitAll && r.commDestroy && r.reduce && r.groupStart &&
         r.groupEnd && r.errorString;
  });
  return ok ? &r : nullptr;
}

#define RCCL_TRY(R, x)                                                                 \
  do {                                                                                 \
    const ncclResult_t e_ = (x);                                                       \
    if (e_ != ncclSuccess) return fail(KDPT_ERR_HIP, std::string("rccl: ") + (R)->errorString(e_)); \
  } while (0)

// frame image = a + b + ... (rank order), the copy-reduce's sum
struct FrameParts {
  const float* p[8];
  int n;
};
__global__ void k_sum_frames(float* __restrict__ out, FrameParts parts, int n3) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n3) return;
  float v = parts.p[0][i];
  for (int k = 1; k < parts.n; k++) v += parts.p[k][i];
  out[i] = v;
}

// Diagnostic ("reduce_spin_us" knob): one wave that spins for `ticks` of the device's constant-rate clock on the
// reduce stream ahead of a frame's reduce -- what an ncclReduce waiting for a slower peer looks like to this
// GPU's queues (tools/reduce_spin_probe.py).
__global__ void k_spin(unsigned long long ticks) {
  const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
  while (__builtin_amdgcn_s_memrealtime() - t0 < ticks) __builtin_amdgcn_s_sleep(16);
}

int reduce_spin(kdpt_ctx* c, hipStream_t st) {
  if (!(c->reduce_spin_us > 0)) return KDPT_OK;
  const unsigned long long ticks = (unsigned long long)(c->reduce_spin_us * c->wall_khz / 1000.0);
  hipLaunchKernelGGL(k_spin, dim3(1), dim3(64), 0, st, ticks);
  HIP_TRY(hipGetLastError());
  return KDPT_OK;
}

void release_comm(kdpt_ctx* c) {
  const Rccl* R = c->comm && c->owns_comm ? rccl() : nullptr;
  if (R) (void)R->commDestroy((ncclComm_t)c->comm);
  c->comm = nullptr;
  c->owns_comm = false;
}

void unregister_host(kdpt_ctx* c) {
  for (void* p : c->host_reg) (void)hipHostUnregister(p);
  c->host_reg.clear();
}

int frame_buffers(kdpt_ctx* c) {
  const size_t n3 = 3 * (size_t)c->npix;
  if (!c->reduce_stream) {
    int rc = create_stream(c, &c->reduce_stream);
    if (rc) return rc;
  }
  for (int k = 0; k < 2; k++) {
    if (!c->frame_buf[k]) {
      int rc = dalloc(c, &c->frame_buf[k], n3);
      if (rc) return rc;
      HIP_TRY(hipEventCreateWithFlags(&c->frame_ev[k], hipEventDisableTiming));
      HIP_TRY(hipEventRecord(c->frame_ev[k], c->stream));
    }
  }
  if (!c->frame_sum && c->rank == 0) return dalloc(c, &c->frame_sum, n3);
  return KDPT_OK;
}

// A pageable host `out` is pinned in place for the frames' copies (hipHostRegister), so they run as queued
// instead of staging synchronously at every frame's enqueue (which would serialise frame f + 1's enqueue behind
// frame f's reduce); device memory, already pinned memory and failed registrations are left as they are.
void pin_host_out(kdpt_ctx* c, void* p, size_t bytes) {
  if (!p || !bytes) return;
  hipPointerAttribute_t a;
  if (hipPointerGetAttributes(&a, p) == hipSuccess && a.type != hipMemoryTypeUnregistered) return;
  (void)hipGetLastError();
  if (hipHostRegister(p, bytes, hipHostRegisterDefault) == hipSuccess) c->host_reg.push_back(p);
  else (void)hipGetLastError();
}

// Iterations of frame f for rank r of n: first, stride n, count.
void frame_share(int f, int spp, int n, int r, int* first, int* count) {
  *first = f * spp + 1 + r;
  *count = r < spp ? (spp - r + n - 1) / n : 0;
}

// Queue frame f's share of this rank into frame_buf[f & 1] (zeroed first, after its previous reduce), and make
// the reduce stream wait for it: the share's last add (c->acc_last), or, for a rank with no iterations in the
// frame, the zeroing itself, done on the reduce stream (which already follows the previous reduce).
int enqueue_frame(kdpt_ctx* c, int f, int spp, int pipeline, int batch) {
  int rc = frame_buffers(c);
  if (rc) return rc;
  float* fb = c->frame_buf[f & 1];
  int first, count;
  frame_share(f, spp, c->nranks, c->rank, &first, &count);
  if (count > 0) {
    if ((rc = enqueue_iterations(c, first, count, c->nranks, pipeline, batch, fb, c->frame_ev[f & 1]))) return rc;
    HIP_TRY(hipStreamWaitEvent(c->reduce_stream, c->acc_last, 0));
  } else {
    HIP_TRY(hipMemsetAsync(fb, 0, sizeof(float) * 3 * (size_t)c->npix, c->reduce_stream));
  }
  return KDPT_OK;
}

// Rank 0, after its frame image is in `sum`: add it into the context's image and copy it out.
int finish_frame(kdpt_ctx* c, const float* sum, float* out, int k, hipStream_t st) {
  const int n3 = 3 * c->npix;
  PartialImages parts{};
  parts.p[0] = sum;
  parts.nb = 1;
  hipLaunchKernelGGL(k_accumulate_batch, dim3((n3 + 255) / 256), dim3(256), 0, st, c->image, parts, n3);
  HIP_TRY(hipGetLastError());
  c->accumulated = true;
  if (out) HIP_TRY(hipMemcpyAsync(out + (size_t)k * n3, sum, sizeof(float) * n3, hipMemcpyDefault, st));
  return KDPT_OK;
}

int check_frames_args(kdpt_ctx* c, int first_frame, int frames, int spp) {
  if (!c || first_frame < 0 || frames < 0 || spp < 1) return fail(KDPT_ERR_ARG, "bad arguments");
  return KDPT_OK;
}

}  // namespace

int kdpt_comm_library(char* path, int len) {
  if (!path || len < 1) return fail(KDPT_ERR_ARG, "bad arguments");
  const Rccl* R = rccl();
  if (!R) return fail(KDPT_ERR_UNSUPPORTED, "librccl.so.1 not found");
  // the file that actually provides ncclReduce (in a torch process: torch's own librccl, if loaded first)
  Dl_info info{};
  const char* f = dladdr(reinterpret_cast<void*>(R->reduce), &info) && info.dli_fname ? info.dli_fname : "?";
  snprintf(path, (size_t)len, "%s", f);
  return KDPT_OK;
}

int kdpt_comm_unique_id(unsigned char* id) {
  if (!id) return fail(KDPT_ERR_ARG, "null id");
  const Rccl* R = rccl();
  if (!R) return fail(KDPT_ERR_UNSUPPORTED, "librccl.so.1 not found");
  static_assert(sizeof(ncclUniqueId) == KDPT_COMM_ID_BYTES, "ncclUniqueId size");
  ncclUniqueId u;
  RCCL_TRY(R, R->getUniqueId(&u));
  memcpy(id, &u, sizeof u);
  return KDPT_OK;
}

int kdpt_comm_init(kdpt_ctx* c, int nranks, int rank, const unsigned char* id) {
  if (!c || nranks < 1 || rank < 0 || rank >= nranks) return fail(KDPT_ERR_ARG, "bad arguments");
  HIP_TRY(hipSetDevice(c->device));
  int rc = kdpt_synchronize(c);
  if (rc) return rc;
  release_comm(c);
  const Rccl* R = rccl();
  c->nranks = nranks;
  c->rank = rank;
  c->external_reduce = nranks > 1 && !id;
  // (one rank with an id gets a communicator too: kdpt_render_frames then runs the same ncclReduce per frame
  // as on N GPUs, so one GPU exercises the multi-GPU path end to end)
  if (id) {
    if (!R) return fail(KDPT_ERR_UNSUPPORTED, "librccl.so.1 not found");
    ncclUniqueId u;
    memcpy(&u, id, sizeof u);
    ncclComm_t comm;
    RCCL_TRY(R, R->commInitRank(&comm, nranks, u, rank));
    c->comm = comm;
    c->owns_comm = true;
  }
  return KDPT_OK;
}

int kdpt_render_frames(kdpt_ctx* c, int first_frame, int frames, int spp, int pipeline, int batch, float* out) {
  int rc = check_frames_args(c, first_frame, frames, spp);
  if (rc) return rc;
  if (c->moments)
    return fail(KDPT_ERR_UNSUPPORTED,
                "kdpt_render_frames: the context keeps second moments (kdpt_set_moments), and frames reach the "
                "image through a cross-rank reduce that does not carry them; turn moments off first");
  HIP_TRY(hipSetDevice(c->device));
  const Rccl* R = c->comm ? rccl() : nullptr;
  if (c->nranks > 1 && !R && !c->external_reduce) return fail(KDPT_ERR_ARG, "kdpt_comm_init first");
  const size_t n3 = 3 * (size_t)c->npix;
  if (c->rank == 0 || c->external_reduce) pin_host_out(c, out, sizeof(float) * n3 * (size_t)frames);
  for (int k = 0; k < frames; k++) {
    const int f = first_frame + k;
    if ((rc = enqueue_frame(c, f, spp, pipeline, batch))) return rc;
    float* fb = c->frame_buf[f & 1];
    // the frame's reduce and image add run on the reduce stream once its adds are done (enqueue_frame), while
    // the batch streams go on with the next frame's (other buffer)
    const hipStream_t rs = c->reduce_stream;
    if ((rc = reduce_spin(c, rs))) return rc;
    const float* sum = fb;
    if (c->external_reduce) {  // the caller reduces: every rank's share goes out as it is
      if (out) HIP_TRY(hipMemcpyAsync(out + (size_t)k * n3, fb, sizeof(float) * n3, hipMemcpyDefault, rs));
    } else {
      if (R) {
        RCCL_TRY(R, R->reduce(fb, c->rank == 0 ? c->frame_sum : nullptr, n3, ncclFloat32, ncclSum, 0,
                              (ncclComm_t)c->comm, rs));
        sum = c->frame_sum;
      }
      if (c->rank == 0 && (rc = finish_frame(c, sum, out, k, rs))) return rc;
    }
    HIP_TRY(hipEventRecord(c->frame_ev[f & 1], rs));
    // (entry points that read or write the image, and adds into it, follow the last reduce: join_accum)
    c->img_last = c->frame_ev[f & 1];
  }
  return KDPT_OK;
}

int kdpt_render_sharded(const kdpt_scene* scene, const kdpt_options* opt, int ndev, const int* devices,
                        int first_frame, int frames, int spp, int pipeline, int batch, int reduce, float* out) {
  if (!scene || ndev < 1 || ndev > 8 || !devices || first_frame < 0 || frames < 0 || spp < 1 ||
      (reduce != KDPT_REDUCE_RCCL && reduce != KDPT_REDUCE_COPY))
    return fail(KDPT_ERR_ARG, "bad arguments");
  kdpt_options o;
  if (opt) o = *opt;
  else kdpt_default_options(&o);
  o.external_image = nullptr;
  std::vector<kdpt_ctx*> cs(ndev, nullptr);
  // every event this call records across devices (destroyed once the contexts' streams are drained)
  std::vector<std::pair<int, hipEvent_t>> xev;
  auto cleanup = [&](int rc) {
    for (auto c : cs)
      if (c) kdpt_destroy(c);  // (drains its streams, releases its communicator)
    for (auto& de : xev) {
      (void)hipSetDevice(de.first);
      (void)hipEventDestroy(de.second);
    }
    return rc;
  };
  int rc;
  for (int i = 0; i < ndev; i++) {
    if ((rc = kdpt_create(scene, &o, devices[i], &cs[i]))) return cleanup(rc);
    cs[i]->nranks = ndev;
    cs[i]->rank = i;
  }
  const Rccl* R = nullptr;
  if (reduce == KDPT_REDUCE_RCCL) {
    R = rccl();
    if (!R) return cleanup(fail(KDPT_ERR_UNSUPPORTED, "librccl.so.1 not found"));
    std::vector<ncclComm_t> comms(ndev);
    const ncclResult_t e = R->commInitAll(comms.data(), ndev, devices);
    if (e != ncclSuccess) return cleanup(fail(KDPT_ERR_HIP, std::string("rccl: ") + R->errorString(e)));
    for (int i = 0; i < ndev; i++) {
      cs[i]->comm = comms[i];
      cs[i]->owns_comm = true;
    }
  }
  kdpt_ctx* c0 = cs[0];
  const int n3 = 3 * c0->npix;
  std::vector<float*> staged(ndev, nullptr);  // copy-reduce: the other ranks' frames on device 0
  if (reduce == KDPT_REDUCE_COPY)
    for (int i = 1; i < ndev; i++)
      if ((rc = dalloc(c0, &staged[i], (size_t)n3))) return cleanup(rc);
  // a pageable host `out` pinned for the call (released by the final kdpt_synchronize of c0)
  pin_host_out(c0, out, sizeof(float) * (size_t)n3 * (size_t)frames);
  hipError_t he;  // the HIP status behind a failing step
  auto xevent = [&](int dev, hipStream_t st, hipEvent_t* e) {
    if ((he = hipSetDevice(dev)) != hipSuccess || (he = hipEventCreateWithFlags(e, hipEventDisableTiming)) != hipSuccess ||
        (he = hipEventRecord(*e, st)) != hipSuccess)
      return false;
    xev.push_back({dev, *e});
    return true;
  };
  for (int k = 0; k < frames; k++) {
    const int f = first_frame + k;
    // each rank queues its share on its batch streams; its reduce stream waits for the share (as in
    // kdpt_render_frames), so frame f + 1's adds never queue behind frame f's reduce
    std::vector<hipEvent_t> share_done(ndev, nullptr);  // each rank's last add of the frame (copy reduce)
    for (int i = 0; i < ndev; i++) {
      kdpt_ctx* ci = cs[i];
      if ((he = hipSetDevice(ci->device)) != hipSuccess) return cleanup(hip_fail("hipSetDevice", he));
      if ((rc = enqueue_frame(ci, f, spp, pipeline, batch))) return cleanup(rc);
      if ((rc = reduce_spin(ci, ci->reduce_stream))) return cleanup(rc);
      // (recorded on the rank's reduce stream, which already waits for the share)
      if (!xevent(ci->device, ci->reduce_stream, &share_done[i])) return cleanup(hip_fail("frame events", he));
    }
    if ((he = hipSetDevice(c0->device)) != hipSuccess) return cleanup(hip_fail("hipSetDevice", he));
    if ((rc = frame_buffers(c0))) return cleanup(rc);
    if (reduce == KDPT_REDUCE_RCCL) {
      R->groupStart();
      ncclResult_t e = ncclSuccess;
      for (int i = 0; i < ndev && e == ncclSuccess; i++)
        e = R->reduce(cs[i]->frame_buf[f & 1], i == 0 ? c0->frame_sum : nullptr, (size_t)n3, ncclFloat32, ncclSum,
                      0, (ncclComm_t)cs[i]->comm, cs[i]->reduce_stream);
      const ncclResult_t e2 = R->groupEnd();
      if (e != ncclSuccess || e2 != ncclSuccess)
        return cleanup(fail(KDPT_ERR_HIP, std::string("rccl: ") + R->errorString(e != ncclSuccess ? e : e2)));
    } else {
      // device 0's reduce stream waits for every rank's share and copies the others' over (peer copies: xGMI
      // between GPUs), then adds them in rank order
      FrameParts parts{};
      parts.n = ndev;
      parts.p[0] = c0->frame_buf[f & 1];
      for (int i = 1; i < ndev; i++) {
        kdpt_ctx* ci = cs[i];
        if ((he = hipSetDevice(c0->device)) != hipSuccess ||
            (he = hipStreamWaitEvent(c0->reduce_stream, share_done[i], 0)) != hipSuccess ||
            (he = hipMemcpyPeerAsync(staged[i], c0->device, ci->frame_buf[f & 1], ci->device, sizeof(float) * (size_t)n3,
                                     c0->reduce_stream)) != hipSuccess)
          return cleanup(hip_fail("copy reduce: peer copy", he));
        parts.p[i] = staged[i];
      }
      hipLaunchKernelGGL(k_sum_frames, dim3((n3 + 255) / 256), dim3(256), 0, c0->reduce_stream, c0->frame_sum, parts, n3);
      if ((he = hipGetLastError()) != hipSuccess) return cleanup(hip_fail("k_sum_frames", he));
      // the other ranks' frame_buf[f & 1] may be reused (frame f + 2) once these copies are done
      hipEvent_t done;
      if (!xevent(c0->device, c0->reduce_stream, &done)) return cleanup(hip_fail("copy reduce: done event", he));
      for (int i = 1; i < ndev; i++)
        if ((he = hipSetDevice(cs[i]->device)) != hipSuccess ||
            (he = hipStreamWaitEvent(cs[i]->reduce_stream, done, 0)) != hipSuccess)
          return cleanup(hip_fail("copy reduce: wait for the done event", he));
    }
    if ((he = hipSetDevice(c0->device)) != hipSuccess) return cleanup(hip_fail("hipSetDevice", he));
    if ((rc = finish_frame(c0, c0->frame_sum, out, k, c0->reduce_stream))) return cleanup(rc);
    for (int i = 0; i < ndev; i++) {
      if ((he = hipSetDevice(cs[i]->device)) != hipSuccess ||
          (he = hipEventRecord(cs[i]->frame_ev[f & 1], cs[i]->reduce_stream)) != hipSuccess)
        return cleanup(hip_fail("hipEventRecord", he));
    }
  }
  for (int i = 0; i < ndev; i++)
    if ((rc = kdpt_synchronize(cs[i]))) return cleanup(rc);
  return cleanup(KDPT_OK);
}

// ---------------------------------------------------------------------------
// Ray queries (include/kdpt.h "Ray queries"; kernels: k_cast_prep, k_trace, k_cast_resolve)
// ---------------------------------------------------------------------------
namespace {

void free_cast_buffers(kdpt_ctx* c) {
  void* const bufs[] = {c->cast_in, c->cast_out, c->cast_cray, c->cast_cand, c->cast_hits, c->cast_cnt, c->cast_tt};
  for (void* p : bufs)
    if (p) (void)hipFree(p);
  c->cast_in = nullptr;
  c->cast_out = nullptr;
  c->cast_cray = nullptr;
  c->cast_cand = nullptr;
  c->cast_hits = nullptr;
  c->cast_cnt = nullptr;
  c->cast_tt = nullptr;
  c->cast_alloc = 0;
}

// The query's buffers for chunks of c->cast_chunk rays (nothing is queued on the context: the caller has
// synchronised, so the old ones can go).
int cast_buffers(kdpt_ctx* c) {
  if (c->cast_alloc == c->cast_chunk) return KDPT_OK;
  free_cast_buffers(c);
  const size_t m = (size_t)c->cast_chunk;
  if (hipMalloc((void**)&c->cast_in, sizeof(float) * 6 * m) != hipSuccess ||
      hipMalloc((void**)&c->cast_out, sizeof(kdpt_ray_hit) * m) != hipSuccess ||
      hipMalloc((void**)&c->cast_cray, sizeof(float4) * 2 * m) != hipSuccess ||
      hipMalloc((void**)&c->cast_cand, sizeof(int) * m) != hipSuccess ||
      hipMalloc((void**)&c->cast_hits, sizeof(int2) * m) != hipSuccess ||
      hipMalloc((void**)&c->cast_cnt, sizeof(int) * 2) != hipSuccess ||
      hipMalloc((void**)&c->cast_tt, sizeof(unsigned long long) * 3) != hipSuccess) {
    (void)hipGetLastError();
    free_cast_buffers(c);
    return fail(KDPT_ERR_HIP, "kdpt_cast_rays: cannot allocate the buffers of a " + std::to_string(m) +
                                  "-ray chunk (knob cast_chunk)");
  }
  for (auto& e : c->cast_ev)
    if (!e) HIP_TRY(hipEventCreate(&e));
  c->cast_alloc = c->cast_chunk;
  return KDPT_OK;
}

// Is p memory of the context's device (as kdpt_write_pbo tells its pbo apart)?
bool on_context_device(const kdpt_ctx* c, const void* p) {
  hipPointerAttribute_t attr{};
  const bool dev = hipPointerGetAttributes(&attr, p) == hipSuccess && attr.type == hipMemoryTypeDevice &&
                   attr.device == c->device;
  (void)hipGetLastError();  // a plain host pointer is an error for hipPointerGetAttributes on some runtimes
  return dev;
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
  const int chunk = c->cast_alloc;
  HIP_TRY(hipMemsetAsync(c->cast_cnt, 0, sizeof(int) * 2, st));
  HIP_TRY(hipMemsetAsync(c->cast_tt, 0, sizeof(unsigned long long) * 3, st));
  HIP_TRY(hipEventRecord(c->cast_ev[0], st));
  CastArgs a;
  a.S = c->S;
  a.normalize = (flags & KDPT_CAST_NORMALIZE) ? 1 : 0;
  a.cray = c->cast_cray;
  a.hits = c->cast_hits;
  a.cand = c->cast_cand;
  a.cnt = c->cast_cnt;
  a.tt = c->cast_tt;
  // (one "iteration" at bounce 0: the query's own queue, its length in cast_cnt[1], the chunk counter in [0])
  TraceArgs t{c->S, {}, 1, 0, c->cast_cnt, 0, c->counters, c->cast_tt};
  std::fill_n(t.it, MAXB, TraceIter{c->cast_cand, c->cast_cnt + 1, c->cast_cray, c->cast_hits});
  void (*const resolve)(CastArgs) = hybrid_shading(c) ? k_cast_resolve<true> : k_cast_resolve<false>;
  for (long long off = 0; off < n; off += chunk) {
    const int m = (int)std::min<long long>(chunk, n - off);
    a.n = m;
    a.o = origins + 3 * off;
    a.d = directions + 3 * off;
    if (!o_dev) {
      HIP_TRY(hipMemcpyAsync(c->cast_in, a.o, sizeof(float) * 3 * (size_t)m, hipMemcpyHostToDevice, st));
      a.o = c->cast_in;
    }
    if (!d_dev) {
      HIP_TRY(hipMemcpyAsync(c->cast_in + 3 * (size_t)chunk, a.d, sizeof(float) * 3 * (size_t)m,
                             hipMemcpyHostToDevice, st));
      a.d = c->cast_in + 3 * (size_t)chunk;
    }
    a.out = out_dev ? out + off : c->cast_out;
    hipLaunchKernelGGL(k_cast_prep, dim3((m + GEN_BLOCK - 1) / GEN_BLOCK), dim3(GEN_BLOCK), 0, st, a);
    HIP_TRY(hipGetLastError());
    launch_trace(c, t, false, c->trace_grid, st);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(resolve, dim3((m + 255) / 256), dim3(256), 0, st, a);
    HIP_TRY(hipGetLastError());
    if (!out_dev)
      HIP_TRY(hipMemcpyAsync(out + off, c->cast_out, sizeof(kdpt_ray_hit) * (size_t)m, hipMemcpyDeviceToHost, st));
  }
  HIP_TRY(hipEventRecord(c->cast_ev[1], st));
  unsigned long long traced = 0;
  HIP_TRY(hipMemcpyAsync(&traced, c->cast_tt + 2, sizeof traced, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  float ms = 0;
  HIP_TRY(hipEventElapsedTime(&ms, c->cast_ev[0], c->cast_ev[1]));
  c->cast_ms = ms;
  c->cast_rays += n;
  c->cast_traced += (long long)traced;
  return check_fault(&c->solo, c->stream);
}

int kdpt_cast_stats(kdpt_ctx* c, long long* rays, long long* traced, double* device_ms) {
  if (!c) return fail(KDPT_ERR_ARG, "kdpt_cast_stats: null ctx");
  if (rays) *rays = c->cast_rays;
  if (traced) *traced = c->cast_traced;
  if (device_ms) *device_ms = c->cast_ms;
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
  if (c->query_ready) return KDPT_OK;
  int rc;
  if (!c->query.counts && (rc = alloc_iter(c, &c->query, c->stream, false))) {
    free_iter(&c->query);
    return rc;
  }
  const size_t npix = (size_t)c->npix;
  if ((!c->query_image && (rc = dalloc(c, &c->query_image, 3 * npix))) ||
      (!c->query_stage && (rc = dalloc(c, &c->query_stage, 6 * npix))) ||
      (!c->query_totals && (rc = dalloc(c, &c->query_totals, 4))))
    return rc;
  c->query.image = c->query_image;
  c->query.total_segments = c->query_totals;
  c->query_ready = true;
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
  IterState& q = c->query;
  q.cur = 0;
  GenBatch gb = gen_batch(c);
  gb.it[0] = q.gen_iter(c->opt.cacherays ? 1 : iter);
  hipLaunchKernelGGL(k_gen_rays_b, dim3((c->npix + 255) / 256, 1), dim3(256), 0, st, gb);
  HIP_TRY(hipGetLastError());
  // xyz of p0 / p1 (float4 records) into packed triples: a strided copy each, straight into device memory of the
  // caller's, through the staging buffer into host memory
  const size_t npix = (size_t)c->npix, row = 3 * sizeof(float);
  float* const outs[2] = {origins, directions};
  const float4* const srcs[2] = {q.buf[0].p0, q.buf[0].p1};
  for (int k = 0; k < 2; k++) {
    const bool dev = on_context_device(c, outs[k]);
    float* const packed = dev ? outs[k] : c->query_stage + 3 * npix * k;
    HIP_TRY(hipMemcpy2DAsync(packed, row, srcs[k], sizeof(float4), row, npix, hipMemcpyDeviceToDevice, st));
    if (!dev) HIP_TRY(hipMemcpyAsync(outs[k], packed, row * npix, hipMemcpyDeviceToHost, st));
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
  IterState* q = &c->query;
  const size_t m = (size_t)n, npix = (size_t)c->npix;
  if (moments && ((!c->query_partial && (rc = dalloc(c, &c->query_partial, 3 * npix))) ||
                  (!c->query_sumsq && (rc = dalloc(c, &c->query_sumsq, 3 * npix)))))
    return rc;
  q->image = moments ? c->query_partial : c->query_image;  // where this call's gathers add
  RaySource src{{origins, directions, (int)n, (flags & KDPT_CAST_NORMALIZE) ? 1 : 0}, c->query_totals + 1};
  if (!on_context_device(c, origins)) {
    HIP_TRY(hipMemcpyAsync(c->query_stage, origins, sizeof(float) * 3 * m, hipMemcpyHostToDevice, st));
    src.rays.o = c->query_stage;
  }
  if (!on_context_device(c, directions)) {
    HIP_TRY(hipMemcpyAsync(c->query_stage + 3 * npix, directions, sizeof(float) * 3 * m, hipMemcpyHostToDevice, st));
    src.rays.d = c->query_stage + 3 * npix;
  }
  HIP_TRY(hipEventRecord(q->ev0, st));
  // pixel i of the query's image is ray i: the gathers add into it in iteration order, from zero
  HIP_TRY(hipMemsetAsync(c->query_image, 0, sizeof(float) * 3 * m, st));
  HIP_TRY(hipMemsetAsync(c->query_totals, 0, sizeof(unsigned long long) * 4, st));
  if (moments) HIP_TRY(hipMemsetAsync(c->query_sumsq, 0, sizeof(float) * 3 * m, st));
  for (int k = 0; k < count; k++) {
    const int iter = first_iter + k;
    if (moments) HIP_TRY(hipMemsetAsync(c->query_partial, 0, sizeof(float) * 3 * m, st));
    if ((rc = launch_batch(c, &q, &iter, 1, st, c->trace_grid, -1, false, nullptr, &src))) return rc;
    if (moments) {
      const int m3 = 3 * (int)n;
      MomentParts parts{};
      parts.p[0] = c->query_partial;
      parts.nb = 1;
      hipLaunchKernelGGL(k_accumulate_moments, dim3((m3 + 255) / 256), dim3(256), 0, st, c->query_image,
                         c->query_sumsq, parts, m3);
      HIP_TRY(hipGetLastError());
    }
  }
  HIP_TRY(hipMemcpyAsync(radiance, c->query_image, sizeof(float) * 3 * m,
                         on_context_device(c, radiance) ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, st));
  if (moments)
    HIP_TRY(hipMemcpyAsync(sumsq, c->query_sumsq, sizeof(float) * 3 * m,
                           on_context_device(c, sumsq) ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, st));
  HIP_TRY(hipEventRecord(q->ev1, st));
  unsigned long long totals[4] = {0, 0, 0, 0};
  HIP_TRY(hipMemcpyAsync(totals, c->query_totals, sizeof totals, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  float ms = 0;
  HIP_TRY(hipEventElapsedTime(&ms, q->ev0, q->ev1));
  c->query_ms = ms;
  c->query_segments = (long long)totals[0];
  c->query_traced = (long long)totals[3];
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
  if (segments) *segments = c->query_segments;
  if (traced) *traced = c->query_traced;
  if (device_ms) *device_ms = c->query_ms;
  return KDPT_OK;
}

// ---------------------------------------------------------------------------
// Per-pixel second moments (include/kdpt.h "Second moments"): kdpt_set_moments, kdpt_read_moments,
// kdpt_noise_map and kdpt_noise_estimate.  While they are on, every add of partial images into the image goes
// through k_accumulate_moments (launch_accumulate), which adds the squares into mom_sumsq in the same pass; the
// shading, intersect and gather kernels never know.
// ---------------------------------------------------------------------------
namespace {

// The buffers of kdpt_set_moments go, and the solo state gathers straight into the image again.  (The caller has
// drained the context's streams.)
void free_moments(kdpt_ctx* c) {
  void* const bufs[] = {c->mom_sumsq, c->mom_partial, c->noise_stage, c->noise_parts};
  for (void* p : bufs)
    if (p) (void)hipFree(p);
  c->mom_sumsq = c->mom_partial = c->noise_stage = nullptr;
  c->noise_parts = nullptr;
  c->mom_samples = 0;
  c->moments = false;
  if (c->solo.zero_partial) {
    c->solo.image = c->image;
    c->solo.zero_partial = false;
  }
}

// k_noise_partials' workgroups: NOISE_BLOCK * NOISE_PER_LANE pixels each.
int noise_blocks(const kdpt_ctx* c) {
  const int per = NOISE_BLOCK * NOISE_PER_LANE;
  return (int)(((long long)c->npix + per - 1) / per);
}

// What kdpt_noise_map and kdpt_noise_estimate refuse, in the same order.
int check_noise_args(const kdpt_ctx* c, float floor, const std::string& who) {
  if (!c) return fail(KDPT_ERR_ARG, who + ": null ctx");
  if (!(std::isfinite(floor) && floor > 0.0f)) return fail(KDPT_ERR_ARG, who + ": floor must be finite and > 0");
  if (!c->moments) return fail(KDPT_ERR_UNSUPPORTED, who + ": moments are off (kdpt_set_moments)");
  if (c->mom_samples < 2)
    return fail(KDPT_ERR_ARG, who + ": " + std::to_string(c->mom_samples) +
                                  " iteration(s) accumulated, a variance needs at least 2");
  return KDPT_OK;
}

}  // namespace

int kdpt_set_moments(kdpt_ctx* c, int enable) {
  if (!c) return fail(KDPT_ERR_ARG, "kdpt_set_moments: null ctx");
  const bool on = enable != 0;
  if (on == c->moments) return KDPT_OK;
  if (on && (c->stats.iterations != 0 || c->accumulated))
    return fail(KDPT_ERR_UNSUPPORTED,
                "kdpt_set_moments: iterations have been accumulated into the image since the last kdpt_reset; "
                "call kdpt_reset first, so that the image and the moments describe the same samples");
  int rc = kdpt_synchronize(c);  // everything queued on the context first (the solo state changes its target)
  if (rc) return rc;
  if (!on) {
    free_moments(c);
    return KDPT_OK;
  }
  const size_t n3 = 3 * (size_t)c->npix;
  hipError_t e;
  if ((e = hipMalloc((void**)&c->mom_sumsq, sizeof(float) * n3)) != hipSuccess ||
      (e = hipMalloc((void**)&c->mom_partial, sizeof(float) * n3)) != hipSuccess ||
      (e = hipMalloc((void**)&c->noise_stage, sizeof(float) * (size_t)c->npix)) != hipSuccess ||
      (e = hipMalloc((void**)&c->noise_parts, sizeof(NoisePartial) * ((size_t)noise_blocks(c) + 1))) != hipSuccess ||
      (e = hipMemsetAsync(c->mom_sumsq, 0, sizeof(float) * n3, c->stream)) != hipSuccess ||
      (e = hipStreamSynchronize(c->stream)) != hipSuccess) {
    free_moments(c);
    return hip_fail("kdpt_set_moments", e);
  }
  c->solo.image = c->mom_partial;
  c->solo.zero_partial = true;  // the camera kernel clears it, as it clears a pipeline state's
  c->mom_samples = 0;
  c->moments = true;
  return KDPT_OK;
}

int kdpt_read_moments(kdpt_ctx* c, float* sumsq, long long* samples) {
  if (!c) return fail(KDPT_ERR_ARG, "kdpt_read_moments: null ctx");
  if (!c->moments) return fail(KDPT_ERR_UNSUPPORTED, "kdpt_read_moments: moments are off (kdpt_set_moments)");
  HIP_TRY(hipSetDevice(c->device));
  int rc = join_accum(c);
  if (rc) return rc;
  if (sumsq)
    HIP_TRY(hipMemcpyAsync(sumsq, c->mom_sumsq, sizeof(float) * 3 * (size_t)c->npix, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  if (samples) *samples = c->mom_samples;
  return KDPT_OK;
}

int kdpt_noise_map(kdpt_ctx* c, float floor, float* noise) {
  int rc = check_noise_args(c, floor, "kdpt_noise_map");
  if (rc) return rc;
  if (!noise) return fail(KDPT_ERR_ARG, "kdpt_noise_map: null noise");
  HIP_TRY(hipSetDevice(c->device));
  if ((rc = join_accum(c))) return rc;
  const bool dev = on_context_device(c, noise);
  float* const d = dev ? noise : c->noise_stage;
  hipLaunchKernelGGL(k_noise_map, dim3((c->npix + 255) / 256), dim3(256), 0, c->stream, c->image, c->mom_sumsq,
                     c->npix, c->mom_samples, floor, d);
  HIP_TRY(hipGetLastError());
  if (!dev) HIP_TRY(hipMemcpyAsync(noise, d, sizeof(float) * (size_t)c->npix, hipMemcpyDeviceToHost, c->stream));
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
  hipLaunchKernelGGL(k_noise_partials, dim3(nb), dim3(NOISE_BLOCK), 0, c->stream, c->image, c->mom_sumsq, c->npix,
                     c->mom_samples, floor, threshold, c->noise_parts);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(k_noise_final, dim3(1), dim3(NOISE_BLOCK), 0, c->stream, c->noise_parts, nb, c->noise_parts + nb);
  HIP_TRY(hipGetLastError());
  NoisePartial r{};
  HIP_TRY(hipMemcpyAsync(&r, c->noise_parts + nb, sizeof r, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  const long long finite = (long long)c->npix - r.nonfinite;
  memset(out, 0, sizeof *out);
  out->samples = c->mom_samples;
  out->pixels = c->npix;
  out->above = r.above;
  out->nonfinite = r.nonfinite;
  out->mean = finite > 0 ? r.sum / (double)finite : 0.0;
  out->max = r.max;
  return KDPT_OK;
}
