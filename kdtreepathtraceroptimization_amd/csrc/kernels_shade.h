// kernels_shade.h -- shading: k_shade, the fused shade + compaction kernels (k_shade_fused, k_shade_fused_b), and the
// three-kernel route's k_scan and k_scatter.
//
// A section of kdpt_runtime.hip's translation unit, not a stand-alone header: kdpt_runtime.hip includes it
// after kernels_brute.h, and the kernels keep that order in the code object.  Device code and launch-argument
// structs only: no HIP host call lives here (tests/test_stream_discipline.py checks that; the guards read host_*.h).
#pragma once

namespace {

// ---------------------------------------------------------------------------
// shadeMaterial + scatterRay (src/pathtrace.cu:1885-2100, src/interactions.h) +
// partialGather, one lane per live path; writes the path in place and the tile's
// survivor count (or, when sorting, its per-material histogram).
// ---------------------------------------------------------------------------
struct ShadeArgs {
  DevScene S;
  PathBuf paths;
  const int2* hits;
  float* image;
  const int* counts;
  int depth;
  int iter;
  float softness;
  int enable_sss;
  int* tile_counts;  // [ntiles] or key-major [MAX_KEYS][ntiles] when sorting
  int ntiles;
  int nkeys;
  unsigned long long* total_segments;  // running sum of paths launched into the intersect kernel
  const unsigned long long* trace_t;   // this bounce's intersect launch record (see TraceArgs)
  const unsigned long long* gspan;     // ... and the k_geoms launches' record
  unsigned long long* trace_total;     // [2]: summed launch ticks, launches (the batch's first iteration only)
  // next bounce's intersect-stage first part (prep_ray) for every surviving path, fused here instead of a
  // k_geoms pass: {t_min bits, (geom + 1) | walks << 16} at the path's current slot (k_scatter moves it)
  int image_zeroed;  // `image` is this iteration's partial image, zeroed by its camera-ray launch: a pixel's
                     // partialGather then reads +0 (each pixel's path ends once), so its load is skipped
  int prep_on;
  int2* prep;
  Counters* count_aabb;  // count mode: root tests of the rays that end there
};

// One path's shading (shadeMaterial + scatterRay, src/pathtrace.cu), the partialGather of a path that ends
// here, and, when the hand-off runs, the next bounce's intersect-stage first part (prep_ray).
struct ShadeOut {
  float4 q0, q1, q2;
  int pm;
  bool changed, alive, walk, tested;
  float tm;
  int gh;
};

// Everything one path's shading reads from memory, loaded in one go: the path, its hit record, the pixel's
// accumulated value (COMPACT: partialGather) and the hit triangle's vertex, edge and normal records (all in
// flight together; k_shade_fused issues them before its publication barrier, and must read the hit record
// before it lets later tiles write the next bounce's records into the same array).
struct ShadeIn {
  float4 q0, q1, q2;
  int pm;
  int2 hr;
  float3 px_old;
  TriData T;
  float4 n1v, n2v, n3v;
};

template <bool COMPACT>
__device__ __attribute__((always_inline)) inline void shade_load(const ShadeArgs& A, const DevScene& S, int i,
                                                                 ShadeIn& in) {
  in.q0 = A.paths.p0[i];
  in.q1 = A.paths.p1[i];
  in.q2 = A.paths.p2[i];
  in.pm = A.paths.pm[i];
  in.hr = A.hits[i];
  in.px_old = make_float3(0.0f, 0.0f, 0.0f);
  if (COMPACT && !A.image_zeroed) {
    const float* px = A.image + 3 * (size_t)(fbits(in.q1.w) & 0x7fffffff);
    in.px_old = make_float3(px[0], px[1], px[2]);
  }
  if (in.hr.x < -1 && fbits(in.q2.w) > 0) {
    const int k = -in.hr.x - 2;
    in.T = TriData{S.tv0[k], S.te1[k], S.te2[k]};
    in.n1v = S.tn0[k];
    in.n2v = S.tn1[k];
    in.n3v = S.tn2[k];
  }
}

template <bool HYBRID, bool COMPACT>
__device__ __attribute__((always_inline)) inline void shade_one(const ShadeArgs& A, const DevScene& S, int i,
                                                                const ShadeIn& in, ShadeOut& o) {
  const float4 q0 = in.q0, q1 = in.q1, q2 = in.q2;
  int matHit = in.pm;
  const int2 hr = in.hr;
  const int pw = fbits(q1.w);
  const int pix = pw & 0x7fffffff;
  Ray ray;
  ray.origin = mk3(q0.x, q0.y, q0.z);
  ray.direction = mk3(q1.x, q1.y, q1.z);
  ray.isinside = (pw >> 31) & 1;
  ray.sdepth = q0.w;
  f3 color = mk3(q2.x, q2.y, q2.z);
  int bounces = fbits(q2.w);
  o.changed = bounces > 0;
  const float3 px_old = in.px_old;
  if (bounces > 0) {
    float isect_t = -1.0f;
    int isect_mat = 0;
    if (hr.x != -1) {
      f3 ip, nrm;
      float t;
      int mid;
      if (hr.x < -1) {  // triangle: the traversal's final recomputation, repeated
        float bx, by, bzk;
        tri_test_v(in.T, ray.origin, ray.direction, bx, by, bzk);
        t = tri_hit_t_n<HYBRID>(in.n1v, in.n2v, in.n3v, ray.origin, ray.direction, bx, by, bzk, ip, nrm);
        mid = hr.y;
      } else {
        const DevGeom& G = S.geoms[hr.x];
        t = G.type == 1 ? boxIntersectionTest(G, ray, ip, nrm) : sphereIntersectionTest(G, ray, ip, nrm);
        mid = G.materialid;
      }
      Rng rng = seeded_rng(A.iter, i, A.depth);
      matHit = mid;
      scatterRay(ray, ip, nrm, S.materials[mid], rng, A.softness);
      isect_t = t;
      isect_mat = mid;
    }
    shade(isect_t, isect_mat, S.materials, A.enable_sss != 0, ray, color, bounces);
  }
  o.q0 = make_float4(ray.origin.x, ray.origin.y, ray.origin.z, ray.sdepth);
  o.q1 = make_float4(ray.direction.x, ray.direction.y, ray.direction.z, ibits(pix | ((ray.isinside ? 1 : 0) << 31)));
  o.q2 = make_float4(color.x, color.y, color.z, ibits(bounces));
  o.pm = matHit;
  if (COMPACT && bounces == 0) {
    // partialGather: one live path per pixel, so this read-modify-write never collides
    float* px = A.image + 3 * (size_t)pix;
    px[0] = px_old.x + color.x;
    px[1] = px_old.y + color.y;
    px[2] = px_old.z + color.z;
  }
  o.alive = COMPACT ? (bounces != 0) : true;
  o.walk = o.tested = false;
  o.tm = 0.0f;
  o.gh = -1;
  if (COMPACT && A.prep_on && bounces != 0) {
    o.walk = prep_ray(S, S.has_obj && S.num_nodes > 0, ray.origin, ray.direction, o.tm, o.gh);
    o.tested = S.has_obj && S.num_nodes > 0;
  }
}

__device__ inline void shade_stats(const ShadeArgs& A, int n) {
  atomicAdd(A.total_segments, (unsigned long long)n);
  // the intersect kernel of this bounce on the device clock (first block start .. last block end; a
  // launch that had nothing to do left its record empty)
  const unsigned long long t0 = A.trace_t[2 * A.depth], t1 = A.trace_t[2 * A.depth + 1];
  const unsigned long long span = t1 > t0 ? t1 - t0 : 0ull;
  if (A.trace_total && span) {
    atomicAdd(&A.trace_total[0], span);
    atomicAdd(&A.trace_total[1], 1ull);
  }
}

__device__ inline void count_prep(const ShadeArgs& A, bool tested, bool walk) {
  const unsigned long long miss = __ballot(tested && !walk), wm = __ballot(walk);
  if ((threadIdx.x & 63) == 0 && miss) {
    atomicAdd(&A.count_aabb->aabb, (unsigned long long)__popcll(miss));
    atomicAdd(&A.count_aabb->aabb_prep, (unsigned long long)__popcll(miss));
  }
  if ((threadIdx.x & 63) == 0 && wm) atomicAdd(&A.count_aabb->cand, (unsigned long long)__popcll(wm));
}

// Shading in place, then k_scan + k_scatter (the material sort of iteration 2, or no compaction).
template <bool HYBRID, bool COMPACT, bool SORT>
__global__ __launch_bounds__(TILE) void k_shade(ShadeArgs A) {
  const int n = A.counts[A.depth];
  const int tile = blockIdx.x;
  if (tile * TILE >= n) return;  // uniform per block
  const int i = tile * TILE + threadIdx.x;
  if (i == 0) shade_stats(A, n);
  __shared__ int s_hist[MAX_KEYS];
  if (SORT) {
    for (int k = threadIdx.x; k < MAX_KEYS; k += TILE) s_hist[k] = 0;
    __syncthreads();
  }
  bool alive = false, walk = false, tested = false;
  int key = 0;
  if (i < n) {
    ShadeOut o;
    ShadeIn in;
    shade_load<COMPACT>(A, A.S, i, in);
    shade_one<HYBRID, COMPACT>(A, A.S, i, in, o);
    if (o.changed) {
      A.paths.p0[i] = o.q0;
      A.paths.p1[i] = o.q1;
      A.paths.p2[i] = o.q2;
      A.paths.pm[i] = o.pm;
    }
    alive = o.alive;
    walk = o.walk;
    tested = o.tested;
    key = o.pm;
    if (COMPACT && A.prep_on && alive) A.prep[i] = make_int2(fbits(o.tm), (o.gh + 1) | (walk ? 0x10000 : 0));
  }
  if (SORT) {
    if (alive) atomicAdd(&s_hist[key], 1);
    __syncthreads();
    for (int k = threadIdx.x; k < A.nkeys; k += TILE) A.tile_counts[k * A.ntiles + tile] = s_hist[k];
  } else {
    const int c = __syncthreads_count(alive);
    if (threadIdx.x == 0) A.tile_counts[tile] = c;
  }
  if (COMPACT && A.prep_on && A.count_aabb) count_prep(A, tested, walk);
}

// Single-pass shading + stable stream compaction (the usual case: compaction on, no material sort).
// Tiles take tickets in arrival order, publish their survivor / walker counts and find their offsets by a
// decoupled look-back over the earlier tiles' records (lb: flag << 62 | survivors << 31 | walkers; flag 1 =
// this tile's counts, 2 = inclusive prefix), then write the survivors straight into the other path buffer in
// the order the scan + scatter would give, with the next bounce's hand-off records.  A tile writes only
// after every earlier tile has published, i.e. has read its inputs, and its own slots are >= the ones it
// writes, so the hit records can be compacted in place.
struct FuseArgs {
  PathBuf dst;
  int* tickets;               // [cap] tile tickets per bounce
  unsigned long long* lb;     // [cap][ntiles] look-back records
  int* counts;                // [cap + 2] live paths per bounce
  int* ccount;                // [cap] the group's candidates per bounce
  float4* cray;               // the group's queue (TraceArgs), an entry being qbase + path
  int2* hits;                 // the iteration's own hit records
  int* cand;
  int qbase;
};

__device__ inline unsigned long long lb_load(const unsigned long long* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ inline void lb_store(unsigned long long* p, unsigned long long v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ inline unsigned long long lb_pack(unsigned long long flag, unsigned s, unsigned w) {
  return (flag << 62) | ((unsigned long long)s << 31) | (unsigned long long)w;
}

constexpr int STAGE_MATS = 32;
#ifdef KDPT_SHADE_PROF  // tools/build_variant.sh experiments only: shading phase times (s_memrealtime ticks)
__device__ unsigned long long g_shade_prof[8];
#endif
#ifndef KDPT_SHADE_TB
#define KDPT_SHADE_TB 256  // tools/build_variant.sh experiments only
#endif
#ifndef KDPT_SHADE_WAVES
#define KDPT_SHADE_WAVES 6  // fused shading: waves per SIMD it is compiled for (caps its VGPRs at 80)
#endif
constexpr int SHADE_TB = KDPT_SHADE_TB;  // paths per fused-shading workgroup (one tile ticket each)

// The LDS a shading workgroup uses: staged geoms/materials and the per-tile compaction scratch.
template <bool STAGE, int TB = TILE>
struct ShadeLDS {
  int tile, b;
  unsigned cnt[2][TB / 64];
  unsigned ex[2];
  uint32_t geoms[STAGE ? ORDERED_GEOMS * sizeof(DevGeom) / 4 : 1];
  uint32_t mats[STAGE ? STAGE_MATS * sizeof(DevMaterial) / 4 : 1];
};

// what a fused-shading workgroup needs beside a resident intersect workgroup (the LDS16S route leaves it free)
constexpr size_t SHADE_LDS_RESERVE = sizeof(ShadeLDS<true, SHADE_TB>);

// STAGE: the analytic geoms and the materials copied into LDS (small scenes: their per-lane reads, indexed
// by hit and by nearest-first order, are then LDS reads instead of L2 round trips)
// (SYNC false: the caller's next __syncthreads publishes the copy -- k_shade_fused overlaps it with the
// tile ticket's atomic round trip)
template <bool STAGE, int TB, bool SYNC = true>
__device__ __attribute__((always_inline)) inline DevScene stage_scene(const DevScene& S0, ShadeLDS<STAGE, TB>& L) {
  static_assert(sizeof(DevGeom) % 4 == 0 && sizeof(DevMaterial) % 4 == 0, "staged as dwords");
  DevScene S = S0;
  if (STAGE) {
    const int gw = S0.num_geoms * (int)(sizeof(DevGeom) / 4), mw = S0.num_materials * (int)(sizeof(DevMaterial) / 4);
    for (int k = threadIdx.x; k < gw; k += TB) L.geoms[k] = reinterpret_cast<const uint32_t*>(S0.geoms)[k];
    for (int k = threadIdx.x; k < mw; k += TB) L.mats[k] = reinterpret_cast<const uint32_t*>(S0.materials)[k];
    if (SYNC) __syncthreads();
    S.geoms = reinterpret_cast<const DevGeom*>(L.geoms);
    S.materials = reinterpret_cast<const DevMaterial*>(L.mats);
  }
  return S;
}

// shade()'s outcome for path i ahead of the shading: bounces left after this bounce != 0.  A listed hit
// has t > 0 (the traversal and k_geoms/prep_ray keep only t > 0, and shade_one recomputes the same t), so
// the path survives iff it has bounces left, hit something, the hit material does not emit, and one bounce
// remains after this one.
__device__ __attribute__((always_inline)) inline bool survives(const DevScene& S, int bounces, int2 hr) {
  if (bounces <= 0) return bounces != 0;
  if (hr.x == -1) return false;
  const int mid = hr.x < -1 ? hr.y : S.geoms[hr.x].materialid;
  return !(S.materials[mid].emittance > 0.0f) && bounces - 1 != 0;
}

// One 256-path tile of one iteration: shading, the survivors' stable compaction into the other path buffer
// (decoupled look-back over the earlier tiles' records), the next bounce's intersect-stage hand-off.  Tiles
// of an iteration must be started in increasing order (tickets), so every earlier tile is already running.
template <bool HYBRID, bool STAGE, int TB>
__device__ __attribute__((always_inline)) inline void shade_tile(const ShadeArgs& A, const FuseArgs& F, const DevScene& S, int tile, int n,
                                  ShadeLDS<STAGE, TB>& L, unsigned long long t_wg = 0ull) {
  const int i = tile * TB + threadIdx.x;
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
#ifdef KDPT_SHADE_PROF
  const unsigned long long pt0 = __builtin_amdgcn_s_memrealtime();
#endif
  if (i == 0) shade_stats(A, n);
  unsigned long long* lb = F.lb + (size_t)A.depth * A.ntiles;
  // (1) Which paths survive this bounce follows from the hit record and the hit material alone, so the
  // tile's survivor count is published (look-back aggregate) before the shading: later tiles' look-backs
  // then wait on this tile's two loads, not on its whole shading (measured: the look-back wait had grown
  // as long as the shading itself, the slowest of 64 predecessors' shading each time).
  // the hit record is read once, here: once this tile's aggregate is out, later tiles may finish their
  // look-back and write the next bounce's records (F.hits == A.hits) into this tile's index range
  ShadeIn in;
  in.hr = make_int2(-1, -1);
  if (i < n) shade_load<true>(A, S, i, in);
  const bool pred = i < n && survives(S, fbits(in.q2.w), in.hr);
  const unsigned long long ms = __ballot(pred);
#ifdef KDPT_SHADE_PROF
  const unsigned long long pa = __builtin_amdgcn_s_memrealtime();
#endif
  if (lane == 0) L.cnt[0][wid] = (unsigned)__popcll(ms);
  __syncthreads();
#ifdef KDPT_SHADE_PROF
  const unsigned long long pb = __builtin_amdgcn_s_memrealtime();
#endif
  if (wid == 0) {
    unsigned aS = 0;
    for (int w = 0; w < TB / 64; w++) aS += L.cnt[0][w];
    if (lane == 0) lb_store(lb + tile, lb_pack(tile == 0 ? 2 : 1, aS, 0));
  }
  // (2) the shading
  ShadeOut o;
  o.alive = o.walk = o.tested = false;
  if (i < n) shade_one<HYBRID, true>(A, S, i, in, o);
  if (o.alive != pred) atomicOr(S.fault, 32);  // unreachable: survives() restates shade()'s outcome
  const unsigned long long mw = __ballot(o.walk);
  if (A.count_aabb && A.prep_on) count_prep(A, o.tested, o.walk);
  if (lane == 0) L.cnt[1][wid] = (unsigned)__popcll(mw);
  __syncthreads();
#ifdef KDPT_SHADE_PROF
  const unsigned long long pt1 = __builtin_amdgcn_s_memrealtime();
#endif
  // (3) the survivors' exclusive prefix (look-back), the walkers' place in the next bounce's candidate
  // list (one counter add per tile: the list's order only decides which lane traces which ray)
  if (wid == 0) {
    unsigned aS = 0, aW = 0;
    for (int w = 0; w < TB / 64; w++) {
      aS += L.cnt[0][w];
      aW += L.cnt[1][w];
    }
    unsigned eS = 0;
    if (tile != 0) {
      for (int base = tile - 1;; base -= 64) {
        const int j = base - lane;
        unsigned long long v = j >= 0 ? lb_load(lb + j) : lb_pack(2, 0, 0);
        while (__ballot((v >> 62) == 0)) {
          __builtin_amdgcn_s_sleep(1);
          if ((v >> 62) == 0) v = lb_load(lb + j);
        }
        const unsigned long long pre = __ballot((v >> 62) == 2);
        const int upto = pre ? __ffsll((long long)pre) - 1 : 63;  // nearest inclusive prefix, and the counts before it
        unsigned sm = lane <= upto ? (unsigned)(v >> 31) & 0x7fffffffu : 0u;
        for (int off = 32; off > 0; off >>= 1) sm += __shfl_xor(sm, off);
        eS += sm;
        if (pre) break;
      }
      if (lane == 0) lb_store(lb + tile, lb_pack(2, eS + aS, 0));
    }
    if (lane == 0) {
      L.ex[0] = eS;
      L.ex[1] = (A.prep_on && aW) ? (unsigned)atomicAdd(&F.ccount[A.depth + 1], (int)aW) : 0u;
      if (tile == (n - 1) / TB) F.counts[A.depth + 1] = (int)(eS + aS);  // the last tile: the next bounce's paths
    }
  }
  __syncthreads();
#ifdef KDPT_SHADE_PROF
  const unsigned long long pt2 = __builtin_amdgcn_s_memrealtime();
#endif
  if (o.alive) {
    unsigned bS = L.ex[0], bW = L.ex[1];
    for (int w = 0; w < wid; w++) {
      bS += L.cnt[0][w];
      bW += L.cnt[1][w];
    }
    const int d = (int)(bS + lane_prefix(ms));
    F.dst.p0[d] = o.q0;
    F.dst.p1[d] = o.q1;
    F.dst.p2[d] = o.q2;
    F.dst.pm[d] = o.pm;
    if (A.prep_on) {
      if (o.walk) {
        const int slot = (int)(bW + lane_prefix(mw));
        F.cand[slot] = F.qbase + d;
        F.cray[2 * (size_t)slot] = make_float4(o.q0.x, o.q0.y, o.q0.z, o.tm);
        F.cray[2 * (size_t)slot + 1] = make_float4(o.q1.x, o.q1.y, o.q1.z, ibits(o.gh));
      } else {
        F.hits[d] = make_int2(o.gh, -1);  // final: the analytic geoms' hit (code -1: none)
      }
    }
  }
#ifdef KDPT_SHADE_PROF
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned long long pt3 = __builtin_amdgcn_s_memrealtime();
    atomicAdd(&g_shade_prof[0], pt1 - pt0);
    atomicAdd(&g_shade_prof[1], pt2 - pt1);
    atomicAdd(&g_shade_prof[2], pt3 - pt2);
    atomicAdd(&g_shade_prof[3], 1ull);
    atomicAdd(&g_shade_prof[4], (unsigned long long)min(TB, n - tile * TB));
    atomicAdd(&g_shade_prof[5], pt0 - t_wg);  // ticket + staging
    atomicAdd(&g_shade_prof[6], pa - pt0);    // the path / hit-record loads (thread 0's wave)
    atomicAdd(&g_shade_prof[7], pb - pa);     // the publication barrier (the tile's slowest wave)
  }
#endif
}

// One launch per bounce and iteration: tile = ticket (tickets start the tiles in order).
template <bool HYBRID, bool STAGE>
__device__ __attribute__((always_inline)) inline void shade_fused_body(const ShadeArgs& A, const FuseArgs& F) {
  const int n = A.counts[A.depth];
  // the grid covers every pixel, so past the first bounces most workgroups have no tile: exactly the first
  // ceil(n / SHADE_TB) take tickets (one contended atomic per tile, not per workgroup), the rest leave at once
  if ((int)blockIdx.x * SHADE_TB >= n) return;
#ifdef KDPT_SHADE_PROF
  const unsigned long long t_wg = __builtin_amdgcn_s_memrealtime();
#else
  const unsigned long long t_wg = 0ull;
#endif
  __shared__ ShadeLDS<STAGE, SHADE_TB> L;
  // the ticket's device-scope atomic and the staging copy are in flight together; one barrier for both
  if (threadIdx.x == 0) L.tile = atomicAdd(&F.tickets[A.depth], 1);
  const DevScene S = stage_scene<STAGE, SHADE_TB, false>(A.S, L);
  __syncthreads();
  const int tile = L.tile;
  shade_tile<HYBRID, STAGE, SHADE_TB>(A, F, S, tile, n, L, t_wg);
}

template <bool HYBRID, bool STAGE>
__global__ __launch_bounds__(SHADE_TB) __attribute__((amdgpu_waves_per_eu(KDPT_SHADE_WAVES))) void k_shade_fused(ShadeArgs A, FuseArgs F) {
  shade_fused_body<HYBRID, STAGE>(A, F);
}

// The same for every fused iteration of a batch in one launch (blockIdx.y = iteration): the batch's
// shading no longer runs iteration after iteration on its stream.
struct ShadeBatch {
  ShadeArgs a[MAXB];
  FuseArgs f[MAXB];
};
template <bool HYBRID, bool STAGE>
__global__ __launch_bounds__(SHADE_TB) __attribute__((amdgpu_waves_per_eu(KDPT_SHADE_WAVES))) void k_shade_fused_b(ShadeBatch B) {
  shade_fused_body<HYBRID, STAGE>(B.a[blockIdx.y], B.f[blockIdx.y]);
}

// Exclusive scan of the tile counts (one workgroup; <= MAX_KEYS * ntiles entries): the survivors, or, when
// sorting, the per-material histogram.
struct ScanJob {
  const int* tile_counts;
  int* tile_off;
  int nkeys;
  int* total_out;
};
// 256 threads: every kernel a batch launches fits beside a resident intersect workgroup (4 waves x 96 VGPRs per
// SIMD, 150 KB of LDS per CU), which a 1024-thread workgroup never does
constexpr int SCAN_TB = 256;
__global__ __launch_bounds__(SCAN_TB) void k_scan(ScanJob J, const int* counts, int depth, int ntiles_alloc) {
  const int* __restrict__ tile_counts = J.tile_counts;
  int* __restrict__ tile_off = J.tile_off;
  const int nkeys = J.nkeys;
  int* total_out = J.total_out;
  const int n = counts[depth];
  const int ntiles = (n + TILE - 1) / TILE;
  const int total_entries = nkeys * ntiles;
  __shared__ int s_wave[SCAN_TB / 64];
  __shared__ int s_carry;
  if (threadIdx.x == 0) s_carry = 0;
  __syncthreads();
  for (int base = 0; base < total_entries; base += SCAN_TB) {
    const int e = base + threadIdx.x;
    int v = 0;
    int k = 0, t = 0;
    if (e < total_entries) {
      k = e / ntiles;
      t = e - k * ntiles;
      v = tile_counts[k * ntiles_alloc + t];
    }
    // inclusive wave scan
    int x = v;
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    for (int off = 1; off < 64; off <<= 1) {
      int y = __shfl_up(x, off);
      if (lane >= off) x += y;
    }
    if (lane == 63) s_wave[wid] = x;
    __syncthreads();
    if (wid == 0) {
      int w = lane < SCAN_TB / 64 ? s_wave[lane] : 0;
      for (int off = 1; off < SCAN_TB / 64; off <<= 1) {
        int y = __shfl_up(w, off);
        if (lane >= off) w += y;
      }
      if (lane < SCAN_TB / 64) s_wave[lane] = w;
    }
    __syncthreads();
    const int carry = s_carry;
    const int excl = carry + (wid > 0 ? s_wave[wid - 1] : 0) + x - v;
    if (e < total_entries) tile_off[k * ntiles_alloc + t] = excl;
    __syncthreads();
    if (threadIdx.x == SCAN_TB - 1) s_carry = excl + v;
    __syncthreads();
  }
  if (threadIdx.x == 0 && total_out) *total_out = s_carry;
}

// Stable compaction (and, on iter 2, the stable sort by materialIdHit).
// The next bounce's intersect-stage hand-off, moved with the survivors by k_scatter: walking rays get their
// geoms record and a candidate-list entry (qbase + the new slot) in the group's queue, one add of the bounce's
// counter per tile, the others their final hit record.
struct ScatterPrep {
  int on;
  const int2* prep;
  float4* cray;   // the group's queue (TraceArgs)
  int2* hits;     // the iteration's own hit records
  int* cand;
  int* ccount;    // the next bounce's candidate counter (the group's)
  int qbase;
};

template <bool SORT>
__global__ __launch_bounds__(TILE) void k_scatter(PathBuf src, PathBuf dst, const int* __restrict__ tile_off,
                                                  const int* counts, int depth, int ntiles_alloc, int compact,
                                                  ScatterPrep P) {
  const int n = counts[depth];
  const int tile = blockIdx.x;
  if (tile * TILE >= n) return;
  const int i = tile * TILE + threadIdx.x;
  const bool valid = i < n;
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  float4 q0, q1, q2;
  int pm = 0;
  bool alive = false;
  if (valid) {
    q0 = src.p0[i];
    q1 = src.p1[i];
    q2 = src.p2[i];
    pm = src.pm[i];
    alive = compact ? (fbits(q2.w) != 0) : true;
  }
  int dst_i;
  if (!SORT) {
    __shared__ int s_wave[TILE / 64];
    const unsigned long long m = __ballot(alive);
    if (lane == 0) s_wave[wid] = __popcll(m);
    __syncthreads();
    int before = 0;
    for (int w = 0; w < wid; w++) before += s_wave[w];
    dst_i = tile_off[tile] + before + (int)lane_prefix(m);
  } else {
    __shared__ int s_key[TILE];
    s_key[threadIdx.x] = alive ? pm : -0x7fffffff;
    __syncthreads();
    int r = 0;
    for (int j = 0; j < (int)threadIdx.x; j++) r += (s_key[j] == pm);
    dst_i = tile_off[pm * ntiles_alloc + tile] + r;
  }
  if (alive) {
    dst.p0[dst_i] = q0;
    dst.p1[dst_i] = q1;
    dst.p2[dst_i] = q2;
    dst.pm[dst_i] = pm;
  }
  if (P.on) {
    __shared__ int s_walk[TILE / 64], s_cbase;
    const int2 pr = alive ? P.prep[i] : make_int2(0, 0);
    const bool w = alive && (pr.y & 0x10000);
    const int geom = (pr.y & 0xffff) - 1;
    const unsigned long long m = __ballot(w);
    if (lane == 0) s_walk[wid] = __popcll(m);
    __syncthreads();
    if (threadIdx.x == 0) {
      int tot = 0;
      for (int k = 0; k < TILE / 64; k++) tot += s_walk[k];
      s_cbase = tot ? atomicAdd(P.ccount, tot) : 0;
    }
    __syncthreads();
    if (alive) {
      if (w) {
        int before = 0;
        for (int k = 0; k < wid; k++) before += s_walk[k];
        const int slot = s_cbase + before + (int)lane_prefix(m);
        P.cand[slot] = P.qbase + dst_i;
        P.cray[2 * (size_t)slot] = make_float4(q0.x, q0.y, q0.z, u2f((uint32_t)pr.x));
        P.cray[2 * (size_t)slot + 1] = make_float4(q1.x, q1.y, q1.z, ibits(geom));
      } else {
        P.hits[dst_i] = make_int2(geom, -1);  // final: the analytic geoms' hit (code -1: none)
      }
    }
  }
}

}  // namespace
