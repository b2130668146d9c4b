// kernels_gen.h -- the path buffers, camera rays (generateRayFromCamera), the intersect stage's launch records and tree
// modes and the analytic-geom stage (k_gen_rays_b, k_geoms_b, k_gen_geoms_b; its per-ray part, prep_ray, is in kdpt_geoms.h).
//
// A section of kdpt_runtime.hip's translation unit, not a stand-alone header: kdpt_runtime.hip includes it
// after kdpt_runtime.hip's own head, and the kernels keep that order in the code object.  Device code and launch-argument
// structs only: no HIP host call lives here (tests/test_stream_discipline.py checks that; the guards read host_*.h).
#pragma once

namespace {

// Path state, structure of arrays of float4 (coalesced 1 KiB per wave load):
//   p0 = {origin.xyz, sdepth}
//   p1 = {direction.xyz, pixelIndex | isinside << 31}
//   p2 = {color.rgb, remainingBounces}
//   pm = materialIdHit
struct PathBuf {
  float4* p0;
  float4* p1;
  float4* p2;
  int* pm;
};

struct Counters {
  unsigned long long aabb, tri, hit;
  unsigned long long aabb_prep;  // root-box tests of rays that end before the intersect kernel (k_geoms/k_shade)
  unsigned long long cand;       // rays handed to the intersect kernel
  unsigned long long wave[PROF_SLOTS + 2];  // WaveLeafLDS::prof summed over chunks, then chunks, cycles
  unsigned long long life[64];  // count mode: wave lifetimes in the intersect kernel, 10 us bins (s_memrealtime)
  unsigned long long steps[64];  // count mode: node steps per ray, bins of 4
  unsigned long long chord_steps[8], chord_n[8];  // ... summed by the ray's chord through the root box (8ths of
                                                  // the box diagonal): does the chord predict a ray's cost?
};

// ---------------------------------------------------------------------------
// generateRayFromCamera (src/pathtrace.cu:315-397)
// ---------------------------------------------------------------------------
// What the first kernel of an iteration zeroes for the later ones, whichever kernel that is (the camera's, or a
// ray query's k_user_rays_b / k_user_geoms_b): lane 0 sets the path count and clears the per-bounce counters and
// launch records, every lane its share of the look-back records.
__device__ __attribute__((always_inline)) inline void gen_prologue(int index, int npaths, int* counts, int ncounts,
                                                                   int* work, int nwork, unsigned long long* trace_t,
                                                                   unsigned long long* lb, int nlb) {
  if (index == 0) {
    counts[0] = npaths;
    for (int k = 1; k < ncounts; k++) counts[k] = 0;
    for (int k = 0; k < nwork; k++) {
      work[k] = 0;
      work[nwork + k] = 0;  // candidate counts (k_geoms), stored after the work counters
      work[2 * nwork + k] = 0;  // k_shade_fused's tile tickets
      trace_t[2 * k] = ~0ull;  // k_trace span of bounce k, then (at 2*nwork) k_geoms' span
      trace_t[2 * k + 1] = 0ull;
      trace_t[2 * nwork + 2 * k] = ~0ull;
      trace_t[2 * nwork + 2 * k + 1] = 0ull;
    }
  }
  for (int e = index; e < nlb; e += gridDim.x * blockDim.x) lb[e] = 0ull;  // k_shade_fused's look-back records
}

// Lane `index` of the launch makes path `index` of npaths -- the slot: where the path, its pixelIndex and its entry
// of zero_image go -- from the camera's ray through a pixel: pixel `index` for the camera kernels (pixels null, npaths
// = W*H), pixel pixels[index] for a launch over a list of pixels (kernels_adaptive.h).
__device__ __attribute__((always_inline)) inline bool gen_rays_body(
    const kdpt_camera& cam, int iter, int traceDepth, PathBuf out, float focalLength, float dofAngle, int antialias,
    int* counts, int ncounts, int* work, int nwork, unsigned long long* trace_t, unsigned long long* lb, int nlb,
    float* zero_image, int npaths, const int* pixels, f3& ray_o, f3& ray_d) {
  const int W = cam.resolution[0], H = cam.resolution[1];
  const int index = blockIdx.x * blockDim.x + threadIdx.x;
  gen_prologue(index, npaths, counts, ncounts, work, nwork, trace_t, lb, nlb);
  if (index >= npaths) return false;
  if (zero_image) {  // batched iterations: this iteration's partial image starts at zero (no separate fill)
    zero_image[3 * index] = 0.0f;
    zero_image[3 * index + 1] = 0.0f;
    zero_image[3 * index + 2] = 0.0f;
  }
  const int pixel = pixels ? pixels[index] : index;
  const int x = pixel % W, y = pixel / W;
  const f3 view = mk3(cam.view[0], cam.view[1], cam.view[2]);
  const f3 right = mk3(cam.right[0], cam.right[1], cam.right[2]);
  const f3 upv = mk3(cam.up[0], cam.up[1], cam.up[2]);
  Ray ray;
  ray.origin = mk3(cam.position[0], cam.position[1], cam.position[2]);
  ray.isinside = false;
  // cam.right * cam.pixelLength.x * (...): (vec * float) * float
  f3 a = scl(scl(right, cam.pixelLength[0]), ((float)x - (float)W * 0.5f));
  f3 b = scl(scl(upv, cam.pixelLength[1]), ((float)y - (float)H * 0.5f));
  ray.direction = normalize(sub(sub(view, a), b));
  Rng rng = rng_seed(utilhash((uint32_t)iter));  // same stream for every pixel (:334)
  if (antialias) {
    const float jitterscale = (float)0.002;
    float j0 = u01(rng), j1 = u01(rng), j2 = u01(rng);
    f3 v3a = normalize(mk3(j0, j1, j2));
    ray.direction = add(ray.direction, scl(v3a, jitterscale));
    ray.direction = normalize(ray.direction);
  }
  float u = kdpt_cosf(PI_F * u01(rng));
  float u2 = u * u;
  float sq = sqrtf(1 - u2);
  float theta = 2 * PI_F * u01(rng);
  f3 vv = normalize(mk3(sq * kdpt_cosf(theta), sq * kdpt_sinf(theta), u));
  (void)u01(rng);  // R1
  (void)u01(rng);  // R2
  float randangle = u01(rng) * PI_F * dofAngle;
  float qw = kdpt_cosf(randangle / 2.0f);
  float sh = kdpt_sinf(randangle / 2.0f);
  f3 qv = mk3(vv.x * sh, vv.y * sh, vv.z * sh);
  const f3 randrot = quat_rotate(qw, qv, ray.direction);  // glm::rotate(Q1, direction)
  ray.origin = sub(add(ray.origin, scl(ray.direction, focalLength)), scl(randrot, focalLength));
  ray.direction = normalize(randrot);
  out.p0[index] = make_float4(ray.origin.x, ray.origin.y, ray.origin.z, 0.0f);
  out.p1[index] = make_float4(ray.direction.x, ray.direction.y, ray.direction.z, ibits(index));
  out.p2[index] = make_float4(1.0f, 1.0f, 1.0f, ibits(traceDepth));
  ray_o = ray.origin;
  ray_d = ray.direction;
  return true;
}

// Launched for a whole batch of iterations at once (k_gen_rays_b, blockIdx.y = iteration).
struct GenIter {
  int iter;
  PathBuf out;
  int* counts;
  int* work;
  unsigned long long* trace_t;
  unsigned long long* lb;
  float* zero_image;
};

// ---------------------------------------------------------------------------
// pathTraceOneBounceKDbare (src/pathtrace.cu:1489-1662): the intersect kernel.
//
// Persistent: one 1024-thread workgroup per CU slot; every wave repeatedly takes
// the next 64 live paths from a device counter, so a wave that drew heavy rays
// never holds a CU idle.  With MODE == TREE_LDS the workgroup first copies the
// packed KD tree into LDS and every node step is an LDS read.
// Output per path: hit code (-1 none, g >= 0 analytic geom g, -(k + 2) triangle k)
// and objMaterialIdx; k_shade recomputes the winner's point and normal with the
// same functions, so nothing else needs to travel.
// ---------------------------------------------------------------------------
// TREE_LDS: 32-byte NodesPacked records in LDS (+ the cluster boxes); TREE_LDS16: 16-byte NodesDerived
// records + cluster boxes in LDS; TREE_LDS16G: NodesDerived in LDS, cluster boxes in HBM/L2 (trees whose
// clusters do not fit, e.g. the C5 icosphere: 2 655 nodes = 41 KB, 22 848 clusters = 714 KB); TREE_LDS16S:
// NodesDerived + the super-cluster boxes in LDS, cluster boxes in HBM/L2, two-level cull (the C5 icosphere:
// 1 430 supers of 16 clusters = 45 KB)
enum TreeMode { TREE_WIDE = 0, TREE_PACKED = 1, TREE_LDS = 2, TREE_LDS16 = 3, TREE_LDS16G = 4, TREE_LDS16S = 5 };
#ifndef KDPT_TRACE_BLOCK
#define KDPT_TRACE_BLOCK 1024  // tools/build_variant.sh experiments only
#endif
constexpr int TRACE_BLOCK = KDPT_TRACE_BLOCK;  // LDS mode: one workgroup per CU shares the tree copy
#ifndef KDPT_SRUN_SPREAD
#define KDPT_SRUN_SPREAD 0  // 1: static runs of ceil(n / waves) instead of 64 (experiment)
#endif
// workgroup size of the intersect kernel: with the tree in LDS every wave of a CU must share the copy,
// otherwise small workgroups let the tail of one launch hold only a quarter of a CU
// NodesDerived halves the tree copy.  Two 512-thread workgroups per CU (30 KB of per-wave leaf scratch + 46 KB
// of tree and cluster boxes each for dragon_5), so that one workgroup's launch tail would overlap the next
// one's start, measured 5.5 % slower than one 1024-thread workgroup (profiles/r03_ab_log.md)
#ifndef KDPT_TRACE_BLOCK16
#define KDPT_TRACE_BLOCK16 1024  // tools/build_variant.sh experiments only
#endif
constexpr int TRACE_BLOCK16 = KDPT_TRACE_BLOCK16;
constexpr bool tree_in_lds(int mode) { return mode >= 2; }
template <int MODE>
constexpr int trace_block() { return MODE == 2 ? TRACE_BLOCK : (MODE >= 3 ? TRACE_BLOCK16 : 256); }

// Up to MAXB iterations (each its own path buffers) at the same bounce share one intersect launch:
// more rays per launch keep the lanes of the persistent waves busy.  (MAXB: kdpt_scene_prep.h, whose shape
// check keeps MAXB x npix below 2^31.)
//
// The batch's candidate queue is one list for all its iterations: every producer (geoms_core, k_shade_fused,
// k_scatter) appends to it through the one counter of the bounce, an entry being qbase + path with qbase =
// (the iteration's place in its group) x npix -- which is also the path's place in the group's hit records
// (hits0; iteration b's own view of them starts at hits0 + b npix).  k_trace therefore never learns which
// iteration a ray belongs to.  The queue's order only decides which lane traces which ray.
struct TraceArgs {
  DevScene S;
  const int* cand;      // the producers' list of the rays that meet the KD root box (queue slot -> hits0 entry)
  const float4* cray;   // ... and their rays in queue order: [2 slot] = {origin, t_min}, [2 slot + 1] = {dir, geom}
  const int* count;     // ... and its length at this bounce
  int2* hits0;          // the group's hit records
  unsigned long long* trace_rays;  // rays handed to the intersect kernel, summed (null: not kept)
  int prof_steps;  // count mode, "profile_batches" = 2: per-ray node-step histogram
  int* work;  // chunk counters, zeroed by k_gen_rays (of iteration 0 of the batch)
  int depth;
  Counters* counters;
  unsigned long long* trace_t;  // [4 * cap]: per bounce first block start / last block end (s_memrealtime)
                                // of k_trace, then of k_geoms (at 2 * cap)
};

struct GenBatch {
  GenIter it[MAXB];
  kdpt_camera cam;
  int traceDepth, antialias, ncounts, nwork, nlb;
  float focalLength, dofAngle;
};
__global__ __launch_bounds__(256) void k_gen_rays_b(GenBatch B) {
  const GenIter& g = B.it[blockIdx.y];
  f3 o, d;
  (void)gen_rays_body(B.cam, g.iter, B.traceDepth, g.out, B.focalLength, B.dofAngle, B.antialias, g.counts,
                      B.ncounts, g.work, B.nwork, g.trace_t, g.lb, B.nlb, g.zero_image,
                      B.cam.resolution[0] * B.cam.resolution[1], nullptr, o, d);
}

__device__ inline void flush_counters(Counters* C, const TraverseCounters& cnt, WaveProf* W,
                                      unsigned long long t_k0) {
  unsigned int a = cnt.aabb, tr = cnt.tri, hi = cnt.hit;
  for (int off = 32; off > 0; off >>= 1) {
    a += __shfl_down(a, off);
    tr += __shfl_down(tr, off);
    hi += __shfl_down(hi, off);
  }
  if ((threadIdx.x & 63) == 0) {
    atomicAdd(&C->aabb, (unsigned long long)a);
    atomicAdd(&C->tri, (unsigned long long)tr);
    atomicAdd(&C->hit, (unsigned long long)hi);
    for (int k = 0; k < PROF_SLOTS; k++) {
      atomicAdd(&C->wave[k], W->prof[k]);
      W->prof[k] = 0;
    }
    atomicAdd(&C->wave[PROF_SLOTS], 1ull);
    atomicAdd(&C->wave[PROF_SLOTS + 1], __builtin_readcyclecounter() - t_k0);
  }
}

// The analytic geoms of pathTraceOneBounceKDbare (tested before the KD tree; src/pathtrace.cu:1600-1640),
// one lane per live path, consecutive paths per wave: {t_min bits, geom index} for k_trace.
//
// The KD traversal's first step tests the root's box, and a ray that misses it ends there with no other
// effect (traverseKDbareShortHybrid: `!hitGeom && parentID == -1` -> break), so such a ray's hit record
// is final here: it is written now, and only the rays that meet the root box are listed (cand, ccount)
// for the intersect kernel -- whose lanes then all hold rays that actually walk the tree.
// k_gen_geoms_b / k_geoms_b: 256-thread workgroups (one wave per SIMD), one candidate-list atomic per
// workgroup.  A 1024-thread workgroup needs 4 waves x 88 VGPRs on every SIMD of a CU, which a CU running an
// intersect workgroup (4 x 96 of 512) never has, so the batch's first launch waited for CUs free of k_trace:
// 0.93 ms per launch in the pipelined bench against 0.18 ms alone (profiles/r03_ab_log.md); one 88-VGPR
// wave fits beside the intersect workgroup
#ifndef KDPT_GEN_BLOCK
#define KDPT_GEN_BLOCK 256  // tools/build_variant.sh experiments only
#endif
constexpr int GEN_BLOCK = KDPT_GEN_BLOCK;
// One workgroup's part: the analytic geoms + root-box test of its paths (live: the lane holds a path still
// bouncing), the final hit record of the rays that end there, and the others appended to the candidate list
// through *ccnt (one atomic per workgroup; a single counter hit once per wave by ~10k waves serialises for
// ~100 us at 800x800) as entry qbase + i (see TraceArgs).  Every thread of the workgroup must call it.
template <int TB = GEN_BLOCK>
__device__ __attribute__((always_inline)) inline void geoms_core(const DevScene& S, bool live, int i, f3 o, f3 d,
                                                                 float4* __restrict__ cray, int2* __restrict__ hits,
                                                                 int* __restrict__ cand, int* __restrict__ ccnt,
                                                                 int qbase, Counters* count_aabb) {
  const bool kd = S.has_obj && S.num_nodes > 0;
  bool tested = false, walk = false;  // traversed at all / goes on to the intersect kernel
  float t_min = 0.0f;
  int hit = -1;
  if (live) {
    tested = kd;
    walk = prep_ray(S, kd, o, d, t_min, hit);
    if (!walk) hits[i] = make_int2(hit, -1);  // final: the analytic geoms' hit (code -1: none)
  }
  __shared__ int s_wcount[TB / 64], s_base;
  const unsigned long long wm = __ballot(walk);
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  if (lane == 0) s_wcount[wv] = __popcll(wm);
  if (count_aabb) {  // count mode: the root test of the rays that end here, and the candidates
    const unsigned long long miss = __ballot(tested && !walk);
    if (lane == 0 && miss) {
      atomicAdd(&count_aabb->aabb, (unsigned long long)__popcll(miss));
      atomicAdd(&count_aabb->aabb_prep, (unsigned long long)__popcll(miss));
    }
    if (lane == 0 && wm) atomicAdd(&count_aabb->cand, (unsigned long long)__popcll(wm));
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int tot = 0;
    for (int w = 0; w < TB / 64; w++) {
      const int c = s_wcount[w];
      s_wcount[w] = tot;
      tot += c;
    }
    s_base = tot ? atomicAdd(ccnt, tot) : 0;
  }
  __syncthreads();
  if (walk) {
    const int slot = s_base + s_wcount[wv] + (int)lane_prefix(wm);
    cand[slot] = qbase + i;
    cray[2 * (size_t)slot] = make_float4(o.x, o.y, o.z, t_min);
    cray[2 * (size_t)slot + 1] = make_float4(d.x, d.y, d.z, ibits(hit));
  }
}

__device__ __attribute__((always_inline)) inline void geoms_body(const DevScene& S, PathBuf paths, const int* counts,
                                                                 int depth, float4* __restrict__ cray,
                                                                 int2* __restrict__ hits, int* __restrict__ cand,
                                                                 int* __restrict__ ccount, int qbase,
                                                                 Counters* count_aabb, unsigned long long* gspan) {
  const int n = counts[depth];
  if ((int)(blockIdx.x * blockDim.x) >= n) return;  // uniform per block
  if (threadIdx.x == 0) atomicMin(&gspan[2 * depth], (unsigned long long)__builtin_amdgcn_s_memrealtime());
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  // finished paths (compaction off) are skipped, as pathTraceOneBounce* skips them
  const bool live = i < n && fbits(paths.p2[i].w) > 0;
  f3 o = mk3(0, 0, 0), d = mk3(0, 0, 1);
  if (live) {
    const float4 q0 = paths.p0[i], q1 = paths.p1[i];
    o = mk3(q0.x, q0.y, q0.z);
    d = mk3(q1.x, q1.y, q1.z);
  }
  geoms_core<GEN_BLOCK>(S, live, i, o, d, cray, hits, cand, ccount + depth, qbase, count_aabb);
  if (threadIdx.x == 0) atomicMax(&gspan[2 * depth + 1], (unsigned long long)__builtin_amdgcn_s_memrealtime());
}

// Launched for a whole batch of iterations at once (blockIdx.y = iteration).
struct GeomsIter {
  PathBuf paths;
  const int* counts;
  float4* cray;   // the group's queue
  int2* hits;     // the iteration's own hit records
  int* cand;
  int* ccount;    // the group's candidate counters
  int qbase;
};
struct GeomsBatch {
  DevScene S;
  GeomsIter it[MAXB];
  int depth;
  Counters* count_aabb;
  unsigned long long* gspan;
};
__global__ __launch_bounds__(GEN_BLOCK) void k_geoms_b(GeomsBatch B) {
  const GeomsIter& g = B.it[blockIdx.y];
  geoms_body(B.S, g.paths, g.counts, B.depth, g.cray, g.hits, g.cand, g.ccount, g.qbase, B.count_aabb, B.gspan);
}

// A batch's camera rays and their bounce-0 intersect-stage first part in one launch (blockIdx.y = iteration):
// each lane generates its pixel's ray (written out for the shading) and tests it against the analytic geoms
// and the KD root box straight from registers.  The bounce-0 candidate counter cannot be the one the
// generation zeroes (other workgroups of this launch already add to it), so bounce 0 counts into
// ccount0[parity] of the group, and the launch zeroes ccount0[!parity] for the group's next use (always
// on the same stream, so nothing still reads it).
struct GenGeomsIter {
  int* ccount0;       // this use's bounce-0 candidate counter (the group's: the same for every iteration)
  int* ccount0_next;  // the next use's (zeroed here)
  float4* cray;       // the group's queue
  int2* hits;         // the iteration's own hit records
  int* cand;
  int qbase;
};
struct GenGeomsBatch {
  GenBatch g;
  DevScene S;
  GenGeomsIter it[MAXB];
  Counters* count_aabb;
};
__global__ __launch_bounds__(GEN_BLOCK) void k_gen_geoms_b(GenGeomsBatch B) {
  const GenIter& g = B.g.it[blockIdx.y];
  const GenGeomsIter& q = B.it[blockIdx.y];
  f3 o = mk3(0, 0, 0), d = mk3(0, 0, 1);
  const bool valid = gen_rays_body(B.g.cam, g.iter, B.g.traceDepth, g.out, B.g.focalLength, B.g.dofAngle,
                                   B.g.antialias, g.counts, B.g.ncounts, g.work, B.g.nwork, g.trace_t, g.lb, B.g.nlb,
                                   g.zero_image, B.g.cam.resolution[0] * B.g.cam.resolution[1], nullptr, o, d);
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i == 0) *q.ccount0_next = 0;
  geoms_core<GEN_BLOCK>(B.S, valid && B.g.traceDepth > 0, i, o, d, q.cray, q.hits, q.cand, q.ccount0, q.qbase,
                        B.count_aabb);
}

}  // namespace
