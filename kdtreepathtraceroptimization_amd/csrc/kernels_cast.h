// kernels_cast.h -- the ray queries' kernels (kdpt_cast_rays): k_cast_prep and k_cast_resolve.
//
// A section of kdpt_runtime.hip's translation unit, not a stand-alone header: kdpt_runtime.hip includes it
// after kernels_image.h, and the kernels keep that order in the code object.  Device code and launch-argument
// structs only: no HIP host call lives here (tests/test_stream_discipline.py checks that; the guards read host_*.h).
#pragma once

namespace {

// ---------------------------------------------------------------------------
// Ray queries (kdpt_cast_rays): caller-supplied rays through the intersect stage of the path tracer, one
// chunk at a time -- k_cast_prep (validation + the stage's first part, geoms_core), k_trace (unchanged, over the
// query's own queue, a group of one at depth 0) and k_cast_resolve (the hit code turned into a
// kdpt_ray_hit with the calls shade_one makes).  No PathSegment, iteration number or image is involved.
// ---------------------------------------------------------------------------
struct CastArgs {
  DevScene S;
  const float* o;  // the chunk's origins and directions (3 n floats each), device memory
  const float* d;
  int n;
  int normalize;   // KDPT_CAST_NORMALIZE
  float4* cray;    // the query's own candidate queue and hit records (one chunk)
  int2* hits;
  int* cand;
  int* cnt;        // [0] k_trace's work counter, [1] the chunk's candidate count
  unsigned long long* tt;  // [0..1] k_trace's launch record (TraceArgs::trace_t), [2] candidates summed over the call
  kdpt_ray_hit* out;
};
constexpr int CAST_REJECTED = (int)0x80000000;  // hits[i].y of a rejected ray (objMaterialIdx never takes it)

// The chunk's ray i as it is traced: false = rejected (a non-finite component, a zero direction or one whose
// normalisation is not finite, or a direction that is not unit length: |dot(d, d) - 1| > 1e-6 in float).
// (RayArgs: CastArgs, or kernels_rays.h's UserRays -- anything with o, d and normalize.)
template <typename RayArgs>
__device__ __attribute__((always_inline)) inline bool cast_load(const RayArgs& A, int i, f3& o, f3& d) {
  o = mk3(A.o[3 * (size_t)i], A.o[3 * (size_t)i + 1], A.o[3 * (size_t)i + 2]);
  d = mk3(A.d[3 * (size_t)i], A.d[3 * (size_t)i + 1], A.d[3 * (size_t)i + 2]);
  bool ok = fabsf(o.x) < FLT_INFV && fabsf(o.y) < FLT_INFV && fabsf(o.z) < FLT_INFV && fabsf(d.x) < FLT_INFV &&
            fabsf(d.y) < FLT_INFV && fabsf(d.z) < FLT_INFV;
  if (A.normalize) d = normalize(d);  // glm::normalize, as the camera and the scatter form their directions
  ok = ok && fabsf(d.x) < FLT_INFV && fabsf(d.y) < FLT_INFV && fabsf(d.z) < FLT_INFV;
  return ok && fabsf(dot(d, d) - 1.0f) <= 1e-6f;
}

// One lane per ray of the chunk; zeroes the work counter and the launch record of the k_trace that follows
// (as gen_rays_body does for an iteration).  The candidate count is zero on entry: k_cast_resolve of the
// previous chunk (or the call's fill on the context's stream) left it so.
__global__ __launch_bounds__(GEN_BLOCK) void k_cast_prep(CastArgs A) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i == 0) {
    A.cnt[0] = 0;
    A.tt[0] = ~0ull;
    A.tt[1] = 0ull;
  }
  f3 o = mk3(0, 0, 0), d = mk3(0, 0, 1);
  bool live = false;
  if (i < A.n) {
    live = cast_load(A, i, o, d);
    if (!live) A.hits[i] = make_int2(-1, CAST_REJECTED);
  }
  geoms_core<GEN_BLOCK>(A.S, live, i, o, d, A.cray, A.hits, A.cand, A.cnt + 1, 0, nullptr);
}

// (code, objMaterialIdx) + the ray -> kdpt_ray_hit: t, point and normal recomputed exactly as shade_one
// recomputes them for scatterRay.  A triangle's code indexes tv0 / tn0, the TriBare order of scene->tris (the
// clustered routes carry that index in e1.w).
template <bool HYBRID>
__global__ __launch_bounds__(256) void k_cast_resolve(CastArgs A) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i == 0) {  // k_trace is done with the chunk's candidate count: add it up, and zero it for the next chunk
    A.tt[2] += (unsigned long long)A.cnt[1];
    A.cnt[1] = 0;
  }
  if (i >= A.n) return;
  const DevScene& S = A.S;
  const int2 hr = A.hits[i];
  f3 o, d;
  (void)cast_load(A, i, o, d);
  float t = -1.0f;
  int kind = hr.y == CAST_REJECTED ? KDPT_HIT_INVALID : KDPT_HIT_NONE, prim = -1, mid = -1;
  f3 ip = mk3(0, 0, 0), nrm = mk3(0, 0, 0);
  if (hr.x < -1) {  // triangle: the traversal's final recomputation, repeated
    const int k = -hr.x - 2;
    float bx, by, bzk;
    tri_test_v(TriData{S.tv0[k], S.te1[k], S.te2[k]}, o, d, bx, by, bzk);
    t = tri_hit_t_n<HYBRID>(S.tn0[k], S.tn1[k], S.tn2[k], o, d, bx, by, bzk, ip, nrm);
    kind = KDPT_HIT_TRIANGLE;
    prim = k;
    mid = hr.y;
  } else if (hr.x >= 0) {
    const DevGeom& G = S.geoms[hr.x];
    Ray ray;
    ray.origin = o;
    ray.direction = d;
    ray.isinside = false;
    ray.sdepth = 0.0f;
    t = G.type == 1 ? boxIntersectionTest(G, ray, ip, nrm) : sphereIntersectionTest(G, ray, ip, nrm);
    kind = KDPT_HIT_GEOM;
    prim = hr.x;
    mid = G.materialid;
  }
  kdpt_ray_hit r;
  r.t = t;
  r.kind = kind;
  r.prim = prim;
  r.material = mid;
  r.point[0] = ip.x; r.point[1] = ip.y; r.point[2] = ip.z;
  r.normal[0] = nrm.x; r.normal[1] = nrm.y; r.normal[2] = nrm.z;
  A.out[i] = r;
}

}  // namespace
