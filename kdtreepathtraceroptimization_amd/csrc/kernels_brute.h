// kernels_brute.h -- k_brute (enable_kd = 0) and k_viz (viz_kd), the two intersect kernels without a tree walk.
//
// A section of kdpt_runtime.hip's translation unit, not a stand-alone header: kdpt_runtime.hip includes it
// after kernels_trace.h, and the kernels keep that order in the code object.  Device code and launch-argument
// structs only: no HIP host call lives here (tests/test_stream_discipline.py checks that; the guards read host_*.h).
#pragma once

namespace {

// ---------------------------------------------------------------------------
// pathTraceOneBounce (src/pathtrace.cu:402-628, enable_kd = false): the brute-force intersect kernel,
// the reference's "bruteforce" / "bbox" benchmark columns.  One lane per live path, consecutive paths
// per wave; the analytic geoms, then every OBJ triangle in file order, shape after shape.
//
// The triangle index is wave-uniform (every lane of a wave tests the same triangle), so the triangle
// is fetched with scalar loads once per wave.  Each lane first evaluates, without the division,
// the exact values the reference's Moller-Trumbore divides (a, u = dot(s,p), v = dot(d,q),
// w = dot(e2,q): same operations, same order, so the same bits) and rejects the triangle when the
// decision is certain whatever f = 1/a rounds to; only the remaining lanes (the line crosses the
// triangle, or a decision sits within a few ulps of its threshold) run the reference's exact test and
// hit point.  Output: the same hit record as k_trace (code, objMaterialIdx).
// ---------------------------------------------------------------------------
struct BruteArgs {
  DevScene S;  // tv0/te1/te2/tn0..2: the OBJ triangles in file order
  PathBuf paths;
  const int* counts;
  int depth;
  int2* hits;
  const BruteShape* shapes;  // kdpt_scene_prep.h
  int num_shapes;
  const float4* chunk_lo;  // boxes of the file-order triangles [64j, 64j + 64) (the tested triangles
  const float4* chunk_hi;  // v0, v0 + e1, v0 + e2, rounded outward); chunk_lo[j].w: the chunk's cull coefficient
  float chunk_k;           // 0: the chunks' own coefficients; > 0: one for all ("cull_margin", "cluster_cull" = 0)
  Counters* counters;
  unsigned long long* trace_t;
};

template <bool COUNT>
__device__ inline void brute_triangle(const DevScene& S, int k, const TriData& T, f3 o, f3 d, float& t_min, int& best,
                                      bool take, TraverseCounters& cnt) {
  const f3 v0 = mk3(T.v0.x, T.v0.y, T.v0.z), e1 = mk3(T.e1.x, T.e1.y, T.e1.z), e2 = mk3(T.e2.x, T.e2.y, T.e2.z);
  const f3 p = cross(d, e2);
  const float a = dot(e1, p);
  const f3 s = sub(o, v0);
  const float u = dot(s, p);
  const f3 q = cross(s, e1);
  const float v = dot(d, q);
  const float w = dot(e2, q);
  if (take && !tri_certain_miss(a, u, v, w)) {
    float bx, by, bz;
    if (tri_test_v(T, o, d, bx, by, bz) == 2) {  // intersected: bary.z >= 0
      if (COUNT) cnt.hit++;
      f3 hp, nn;
      const float t = tri_hit_t<true>(S, k, o, d, bx, by, bz, hp, nn);  // hit += norm * 0.0001f
      if (t > 0.0f && t_min > t) {
        t_min = t;
        best = k;
      }
    }
  }
}

template <bool USEBBOX, bool COUNT>
__global__ __launch_bounds__(TILE) void k_brute(BruteArgs A) {
  const int n = A.counts[A.depth];
  if ((int)blockIdx.x * TILE >= n) return;  // uniform per block
  if (threadIdx.x == 0) atomicMin(&A.trace_t[2 * A.depth], (unsigned long long)__builtin_amdgcn_s_memrealtime());
  const DevScene& S = A.S;
  const int i = blockIdx.x * TILE + threadIdx.x;
  bool live = false;
  f3 o = mk3(0.0f, 0.0f, 0.0f), d = mk3(0.0f, 0.0f, 1.0f);
  if (i < n) {
    const float4 q0 = A.paths.p0[i], q1 = A.paths.p1[i];
    live = fbits(A.paths.p2[i].w) > 0;
    o = mk3(q0.x, q0.y, q0.z);
    d = mk3(q1.x, q1.y, q1.z);
  }
  // the analytic geoms (src/pathtrace.cu:461-483)
  float t_min = FLT_MAXV;
  int geom = -1;
  if (live) {
    Ray ray;
    ray.origin = o;
    ray.direction = d;
    ray.isinside = false;
    ray.sdepth = 0.0f;
    f3 tmp_i, tmp_n;
    float t = 0;
    const f3 inv = mk3(1.0f / d.x, 1.0f / d.y, 1.0f / d.z);
    const bool finite = fabsf(inv.x) < FLT_INFV && fabsf(inv.y) < FLT_INFV && fabsf(inv.z) < FLT_INFV;
    for (int g = 0; g < S.num_geoms; g++) {
      const DevGeom& G = S.geoms[g];
      if (finite && !geom_may_hit(G, o, inv)) t = -1.0f;
      else if (G.type == 1) t = boxIntersectionTest(G, ray, tmp_i, tmp_n);
      else if (G.type == 0) t = sphereIntersectionTest(G, ray, tmp_i, tmp_n);
      if (t > 0.0f && t_min > t) {
        t_min = t;
        geom = g;
      }
    }
  }
  // the polygon loop (src/pathtrace.cu:485-576)
  const f3 inv = mk3(1.0f / d.x, 1.0f / d.y, 1.0f / d.z);
  const bool cull = __all(!live || (fabsf(inv.x) < FLT_INFV && fabsf(inv.y) < FLT_INFV && fabsf(inv.z) < FLT_INFV));
  TraverseCounters cnt{};
  int best = -1;
  int objMat = -1;
  int iterator = 0;  // in vertex indices, like the reference; advances only past shapes whose bbox passed
  if (S.has_obj) {
    for (int sh = 0; sh < A.num_shapes; sh++) {
      const BruteShape B = A.shapes[sh];
      objMat = fbits(B.hi.w);
      const int nidx = fbits(B.lo.w);
      bool take = live;
      if (USEBBOX) take = live && intersectBbox(o, d, B.lo, B.hi) > -1.0f;
      const unsigned long long tm = __ballot(take);
      if (tm) {
        const int it0 = __shfl(iterator, __builtin_ctzll(tm));
        if (__all(!take || iterator == it0)) {
          // every lane that tests this shape starts at the same triangle: scalar triangle fetches
          const int k0 = __builtin_amdgcn_readfirstlane(it0 / 3);
          const int nt = nidx / 3;
          // 64-triangle chunks: no triangle of a chunk whose box the lane's line misses passes glm's u/v tests --
          // the box is widened by the chunk's own rigorous coefficient (brute_chunk_may_pass; a chunk of
          // triangles too large for one that culls is never skipped) -- so those lanes skip it, and the wave
          // skips a chunk no lane can hit; the others test its triangles in file order as before
          for (int k = k0; k < k0 + nt;) {
            const int j = k >> 6, kend = min(k0 + nt, (j + 1) << 6);
            const bool may = take && (!cull || brute_chunk_may_pass(A.chunk_lo, A.chunk_hi, j, o, inv, A.chunk_k));
            if (__any(may)) {
              for (; k < kend; k++) {
                const TriData T = tri_load(S, k);
                brute_triangle<COUNT>(S, k, T, o, d, t_min, best, may, cnt);
              }
            }
            k = kend;
          }
        } else {
          const int nt = nidx / 3;
          for (int j = 0; j < nt; j++) {
            const int k = iterator / 3 + j;
            if (take) {
              const TriData T = tri_load(S, k);
              brute_triangle<COUNT>(S, k, T, o, d, t_min, best, true, cnt);
            }
          }
        }
        if (COUNT && take) cnt.tri += nidx / 3;
      }
      if (take) iterator += nidx;
    }
  }
  if (i < n && live) {
    const int code = best >= 0 ? -(best + 2) : geom;
    A.hits[i] = make_int2(code, objMat);
  }
  if (COUNT) {
    unsigned int tr = cnt.tri, hi = cnt.hit;
    for (int off = 32; off > 0; off >>= 1) {
      tr += __shfl_down(tr, off);
      hi += __shfl_down(hi, off);
    }
    if ((threadIdx.x & 63) == 0) {
      atomicAdd(&A.counters->tri, (unsigned long long)tr);
      atomicAdd(&A.counters->hit, (unsigned long long)hi);
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) atomicMax(&A.trace_t[2 * A.depth + 1], (unsigned long long)__builtin_amdgcn_s_memrealtime());
}

// ---------------------------------------------------------------------------
// pathTraceOneBounceKDbareBoxes (src/pathtrace.cu:1738-1885, viz_kd): the analytic geoms, then every KD
// node's box as a box (boxIntersectionTestBox = boxIntersectionTest of the node's unit-cube transform).
// One lane per path; the node index is wave-uniform, so each box's matrices are scalar loads.  A winning
// node box k is reported as geom num_geoms + k (its record carries material num_materials - 1), which
// k_shade recomputes like any analytic geom.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(TILE) void k_viz(DevScene S, PathBuf paths, const int* counts, int depth, int2* hits,
                                               unsigned long long* trace_t) {
  const int n = counts[depth];
  if ((int)blockIdx.x * TILE >= n) return;
  if (threadIdx.x == 0) atomicMin(&trace_t[2 * depth], (unsigned long long)__builtin_amdgcn_s_memrealtime());
  const int i = blockIdx.x * TILE + threadIdx.x;
  if (i < n && fbits(paths.p2[i].w) > 0) {
    const float4 q0 = paths.p0[i], q1 = paths.p1[i];
    Ray ray;
    ray.origin = mk3(q0.x, q0.y, q0.z);
    ray.direction = mk3(q1.x, q1.y, q1.z);
    ray.isinside = false;
    ray.sdepth = q0.w;
    const f3 inv = mk3(1.0f / ray.direction.x, 1.0f / ray.direction.y, 1.0f / ray.direction.z);
    const bool finite = fabsf(inv.x) < FLT_INFV && fabsf(inv.y) < FLT_INFV && fabsf(inv.z) < FLT_INFV;
    float t_min = FLT_MAXV, t = 0;
    int hit = -1;
    f3 tmp_i, tmp_n;
    const int total = S.num_geoms + (S.has_obj ? S.num_boxes : 0);
    for (int g = 0; g < total; g++) {
      const DevGeom& G = S.geoms[g];
      if (finite && !geom_may_hit(G, ray.origin, inv)) t = -1.0f;
      else if (G.type == 1) t = boxIntersectionTest(G, ray, tmp_i, tmp_n);
      else if (G.type == 0) t = sphereIntersectionTest(G, ray, tmp_i, tmp_n);
      if (t > 0.0f && t_min > t) {
        t_min = t;
        hit = g;
      }
    }
    hits[i] = make_int2(hit, -1);
  }
  __syncthreads();
  if (threadIdx.x == 0) atomicMax(&trace_t[2 * depth + 1], (unsigned long long)__builtin_amdgcn_s_memrealtime());
}

}  // namespace
