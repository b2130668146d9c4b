// kernels_rays.h -- bounce 0 of a path-traced ray query (kdpt_trace_rays): k_user_rays_b and k_user_geoms_b, the
// counterparts of k_gen_rays_b and k_gen_geoms_b that load the caller's rays instead of computing the camera's.
//
// A section of kdpt_runtime.hip's translation unit, not a stand-alone header: kdpt_runtime.hip includes it
// after kernels_cast.h, and the kernels keep that order in the code object.  Device code and launch-argument
// structs only: no HIP host call lives here (tests/test_stream_discipline.py checks that; the guards read host_*.h).
#pragma once

namespace {

// ---------------------------------------------------------------------------
// The camera stage is the only stage of an iteration that knows about the camera: every later kernel reads
// counts[depth] and the path buffers.  These two start an iteration from n <= W H rays in device memory: path i
// = {origin_i, direction_i, colour (1, 1, 1), pixelIndex i, remainingBounces traceDepth}, counts[0] = n.
//
// A rejected ray (cast_load: a non-finite component, a zero or non-unit direction) is born finished --
// remainingBounces 0, colour NaN -- and is never queued for the intersect stage.  The rest of the iteration
// treats it as it treats a traceDepth == 0 path: shade_one leaves it alone and the partial gather (compaction
// on) or the final gather (off) adds its colour, so its pixel reads NaN in all three channels.  Its origin and
// direction are stored as (0, 0, 0) / (0, 0, 1): nothing traces them, and nothing downstream meets a NaN ray.
// Like the camera kernels, these leave materialIdHit (pm) as the state's previous use left it.
// ---------------------------------------------------------------------------
struct UserRays {
  const float* o;  // 3 n floats each, device memory
  const float* d;
  int n;
  int normalize;   // KDPT_CAST_NORMALIZE
};
struct UserBatch {  // (one iteration per launch: a query's iterations run one after another in one state)
  GenIter g;
  UserRays src;
  int traceDepth, ncounts, nwork, nlb;
};

__device__ __attribute__((always_inline)) inline bool user_rays_body(const UserBatch& B, f3& ray_o, f3& ray_d) {
  const GenIter& g = B.g;
  const int index = blockIdx.x * blockDim.x + threadIdx.x;
  gen_prologue(index, B.src.n, g.counts, B.ncounts, g.work, B.nwork, g.trace_t, g.lb, B.nlb);
  if (index >= B.src.n) return false;
  f3 o, d;
  const bool ok = cast_load(B.src, index, o, d);  // kdpt_cast_rays' acceptance rule
  if (!ok) {
    o = mk3(0, 0, 0);
    d = mk3(0, 0, 1);
  }
  const float c = ok ? 1.0f : __builtin_nanf("");
  g.out.p0[index] = make_float4(o.x, o.y, o.z, 0.0f);
  g.out.p1[index] = make_float4(d.x, d.y, d.z, ibits(index));
  g.out.p2[index] = make_float4(c, c, c, ibits(ok ? B.traceDepth : 0));
  ray_o = o;
  ray_d = d;
  return ok;
}

// gen_geoms = 0, brute-force and box-view contexts: the paths alone.
__global__ __launch_bounds__(GEN_BLOCK) void k_user_rays_b(UserBatch B) {
  f3 o, d;
  (void)user_rays_body(B, o, d);
}

// The paths and their bounce-0 intersect-stage first part (geoms_core straight from registers), counting the
// candidates into this use's ccount0 and zeroing the next use's, as k_gen_geoms_b does.
struct UserGeomsBatch {
  UserBatch u;
  DevScene S;
  GenGeomsIter q;
  Counters* count_aabb;
};
__global__ __launch_bounds__(GEN_BLOCK) void k_user_geoms_b(UserGeomsBatch B) {
  f3 o = mk3(0, 0, 0), d = mk3(0, 0, 1);
  const bool ok = user_rays_body(B.u, o, d);
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i == 0) *B.q.ccount0_next = 0;
  geoms_core<GEN_BLOCK>(B.S, ok && B.u.traceDepth > 0, i, o, d, B.q.cray, B.q.hits, B.q.cand, B.q.ccount0,
                        B.q.qbase, B.count_aabb);
}

}  // namespace
