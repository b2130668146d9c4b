// kernels_trace.h -- k_trace, the persistent KD-traversal (intersect) kernel.
//
// A section of kdpt_runtime.hip's translation unit, not a stand-alone header: kdpt_runtime.hip includes it
// after kernels_gen.h, and the kernels keep that order in the code object.  Device code and launch-argument
// structs only: no HIP host call lives here (tests/test_stream_discipline.py checks that; the guards read host_*.h).
#pragma once

namespace {

#ifdef KDPT_TAIL_PROF  // tools/build_variant.sh experiments only: intersect workgroup life / tail (ticks)
__device__ unsigned long long g_tail_prof[4];
#endif

// KD traversal of every live path.  Each lane holds one ray; whenever rays finish, the idle lanes take
// the next paths of the bounce from a device counter, so a wave stays full until the bounce runs out
// of paths (the per-ray algorithm is unchanged -- only which lane runs it, and when).
// Compiled for 5 waves per SIMD although a workgroup brings only 4 (its LDS tree copy keeps it alone on the
// CU): the cap (96 VGPRs instead of 108, a few spilled to scratch outside the hot loops) leaves 128 VGPRs per
// SIMD, room for a fused-shading wave of another batch on the same CU while the traversal runs -- and its LDS
// (WaveProf only in the counting kernel) leaves room for that workgroup's 4.2 KB.  A/B +2.8 %.
#ifndef KDPT_TRACE_WAVES
#define KDPT_TRACE_WAVES 5  // tools/build_variant.sh experiments
#endif
// (only with the tree in LDS: the 256-thread workgroups of the other modes share CUs anyway, and the C5
// icosphere, whose tree lives in HBM, lost 3.5 % to the cap)
#define KDPT_TRACE_ATTR __attribute__((amdgpu_waves_per_eu(tree_in_lds(MODE) ? KDPT_TRACE_WAVES : 1)))
template <bool HYBRID, bool COUNT, int MODE>
__global__ __launch_bounds__(trace_block<MODE>()) KDPT_TRACE_ATTR void k_trace(TraceArgs A) {
  constexpr int TB = trace_block<MODE>();
  extern __shared__ int4 s_tree[];
  __shared__ WaveLeafLDS s_leaf[TB / 64];
  __shared__ WaveProf s_prof[COUNT ? TB / 64 : 1];
  const DevScene& S = A.S;
  const int n = *A.count;  // the batch's rays: one queue for all its iterations (TraceArgs)
  // tree copy: NodesPacked (2 x 16 bytes per node) or NodesDerived (16 bytes), then the cluster boxes
  constexpr int NODE_WORDS = MODE == TREE_LDS ? 2 : 1;
  if (tree_in_lds(MODE)) {
    if (n == 0) return;  // uniform: nothing to trace
    const int words = NODE_WORDS * S.num_nodes;
    const int4* src = MODE == TREE_LDS ? S.pnodes : (MODE == TREE_LDS16S ? S.snodes : S.dnodes);
    for (int k = threadIdx.x; k < words; k += TB) s_tree[k] = src[k];
    if (MODE == TREE_LDS16S) {
      for (int k = threadIdx.x; k < S.num_supers; k += TB) s_tree[words + k] = S.sup[k];
    } else if (MODE != TREE_LDS16G) {
      float4* s_cl = reinterpret_cast<float4*>(s_tree + words);
      for (int k = threadIdx.x; k < S.num_clusters; k += TB) {
        s_cl[2 * k] = S.cl_lo[k];
        s_cl[2 * k + 1] = S.cl_hi[k];
      }
    }
    __syncthreads();
  }
  const int lane = threadIdx.x & 63;
  WaveLeafLDS* W = &s_leaf[threadIdx.x >> 6];
  WaveProf* P = &s_prof[COUNT ? (threadIdx.x >> 6) : 0];
  if (COUNT && lane < PROF_SLOTS) P->prof[lane] = 0;
  if (COUNT && lane == 0) P->tail_t0 = 0;
  W->slot[lane] = 0;  // pair_owner's invariant
  // launch duration on the device clock (first block start .. last block end); the HIP events around
  // the launch also count time spent queued behind other streams' kernels when iterations overlap
  __shared__ int s_waves_done;
#ifdef KDPT_TAIL_PROF
  __shared__ unsigned long long s_t0, s_tex;
#endif
  if (threadIdx.x == 0) {
    s_waves_done = 0;
    atomicMin(&A.trace_t[2 * A.depth], (unsigned long long)__builtin_amdgcn_s_memrealtime());
    if (blockIdx.x == 0 && A.trace_rays) atomicAdd(A.trace_rays, (unsigned long long)n);
#ifdef KDPT_TAIL_PROF
    s_t0 = __builtin_amdgcn_s_memrealtime();
    s_tex = ~0ull;
#endif
  }
  __syncthreads();
  int* work = A.work + A.depth;
  const unsigned long long rt0 = COUNT ? __builtin_amdgcn_s_memrealtime() : 0ull;
  const unsigned long long t_k0 = COUNT ? __builtin_readcyclecounter() : 0ull;
  TraverseCounters cnt{};
  WaveRay R;  // every field defined: idle lanes take part in the wave-level code with a finished ray
  wave_ray_start(S, R, mk3(0.0f, 0.0f, 0.0f), mk3(0.0f, 0.0f, 1.0f), FLT_MAXV, -1, W);
  R.done = true;
  int pidx = -1;  // the lane's ray: its entry of hits0 (-1: idle)
  // Path slots: each wave first takes a static run of 64 consecutive slots, the runs dealt out wave-major
  // across the workgroups (run r goes to wave r / grid of workgroup r % grid): a bounce with few rays then
  // still fills every CU (the kernel is issue-bound: rays piled onto a few CUs would leave the others idle)
  // while each wave stays dense (a node trip costs the same whatever the number of walking lanes).  A device
  // counter hands out the rest, exactly as many as the wave has idle lanes, so the tail stays balanced.
  const int nwaves = gridDim.x * (TB / 64);
  const int wid = (threadIdx.x >> 6) * gridDim.x + blockIdx.x;
  const int srun = KDPT_SRUN_SPREAD ? min(64, max(1, (n + nwaves - 1) / nwaves)) : 64;
  bool first = true, exhausted = false;
  long long rounds = 0;
#ifdef KDPT_TAIL_PROF
  unsigned long long tex_seen = 0;
#endif
  while (true) {
    if (__ballot(1) != ~0ull) {  // the refill protocol needs the whole wave here
      atomicOr(S.fault, 4);
      break;
    }
    // ---- refill idle lanes ----
    if (COUNT) prof_lap(P, -1);
    const unsigned long long im = exhausted ? 0ull : __ballot(pidx < 0);
    if (im) {
      const int p = (int)lane_prefix(im);
      int k;
      if (first) {  // static run: slots [wid*srun, wid*srun + srun)
        first = false;
        k = p < srun ? wid * srun + p : n;
        exhausted = (long long)nwaves * srun >= n;
      } else {
        int b = 0;
        if (lane == 0) b = nwaves * srun + atomicAdd(work, __popcll(im));
        const int base = __builtin_amdgcn_readfirstlane(b);  // lane 0 is active: the whole wave is here
        k = base + p;
        exhausted = base + __popcll(im) >= n;  // the counter only grows: later rounds find nothing
      }
      if (COUNT && exhausted && lane == 0 && !P->tail_t0) P->tail_t0 = __builtin_readcyclecounter();
#ifdef KDPT_TAIL_PROF
      if (exhausted && !tex_seen) tex_seen = __builtin_amdgcn_s_memrealtime();
#endif
      if (pidx < 0 && k < n) {
        // the slot's entry and its ray (written in queue order with the slot): three independent loads
        // of consecutive slots from uniform bases, not a slot load followed by scattered path loads
        const int i = A.cand[k];
        const float4 q0 = A.cray[2 * (size_t)k], q1 = A.cray[2 * (size_t)k + 1];
        pidx = i;
        wave_ray_start(S, R, mk3(q0.x, q0.y, q0.z), mk3(q1.x, q1.y, q1.z), q0.w, fbits(q1.w), W);
      }
    }
    if (COUNT) prof_lap(P, PROF_SETUP_CYC);
    const bool busy = pidx >= 0 && !R.done;
    if (__any(busy)) {
      const bool fastAABB = __all(!busy || (fabsf(R.invdir.x) < FLT_INFV && fabsf(R.invdir.y) < FLT_INFV &&
                                            fabsf(R.invdir.z) < FLT_INFV));
      if (MODE == TREE_LDS)
        trace_phase<HYBRID, COUNT>(S, NodesPacked{s_tree},
                                   ClustersInterleaved{reinterpret_cast<const float4*>(s_tree + 2 * S.num_nodes)}, R,
                                   fastAABB, S.num_materials, cnt, W, P);
      else if (MODE == TREE_LDS16)
        trace_phase<HYBRID, COUNT>(S, NodesDerived{s_tree},
                                   ClustersInterleaved{reinterpret_cast<const float4*>(s_tree + S.num_nodes)}, R,
                                   fastAABB, S.num_materials, cnt, W, P);
      else if (MODE == TREE_LDS16G)
        trace_phase<HYBRID, COUNT>(S, NodesDerived{s_tree}, ClustersSplit{S.cl_lo, S.cl_hi}, R, fastAABB,
                                   S.num_materials, cnt, W, P);
      else if (MODE == TREE_LDS16S)
        trace_phase<HYBRID, COUNT>(
            S, NodesDerived{s_tree},
            ClustersSuper{s_tree + S.num_nodes, S.cl_lo, S.cl_hi, S.cl_n, S.cl_u, S.cl_v, S.cl_w}, R, fastAABB,
            S.num_materials, cnt, W, P);
      else if (MODE == TREE_PACKED)
        trace_phase<HYBRID, COUNT>(S, NodesPacked{S.pnodes}, ClustersSplit{S.cl_lo, S.cl_hi}, R, fastAABB,
                                   S.num_materials, cnt, W, P);
      else
        trace_phase<HYBRID, COUNT>(S, NodesWide{S.nodes}, ClustersSplit{S.cl_lo, S.cl_hi}, R, fastAABB,
                                   S.num_materials, cnt, W, P);
    }
    // ---- finished rays: their hit record (what ShadeableIntersection would carry) ----
    if (pidx >= 0 && R.done) {
      if (COUNT && A.prof_steps) {  // (its atomics distort the cycle profile: a separate run)
        const int st = R.guard;
        atomicAdd(&A.counters->steps[min(st >> 2, 63)], 1ull);
        const float4 lo = S.rlo, hi = S.rhi;
        const float ax = (lo.x - R.o.x) * R.invdir.x, bx = (hi.x - R.o.x) * R.invdir.x;
        const float ay = (lo.y - R.o.y) * R.invdir.y, by = (hi.y - R.o.y) * R.invdir.y;
        const float az = (lo.z - R.o.z) * R.invdir.z, bz2 = (hi.z - R.o.z) * R.invdir.z;
        const float t0 = fmaxf(fmaxf(fminf(ax, bx), fminf(ay, by)), fmaxf(fminf(az, bz2), 0.0f));
        const float t1 = fminf(fminf(fmaxf(ax, bx), fmaxf(ay, by)), fmaxf(az, bz2));
        const float dx = hi.x - lo.x, dy = hi.y - lo.y, dz = hi.z - lo.z;
        const float diag = sqrtf(dx * dx + dy * dy + dz * dz);
        const float f = diag > 0.0f ? 8.0f * fmaxf(t1 - t0, 0.0f) / diag : 0.0f;
        const int cb = f >= 7.0f || !(f == f) ? 7 : (int)f;
        atomicAdd(&A.counters->chord_steps[cb], (unsigned long long)st);
        atomicAdd(&A.counters->chord_n[cb], 1ull);
      }
      const Hit& h = R.h;
      const int code = h.hit_geom_index == -1 ? -1 : (h.obj_intersect ? -(R.objTri + 2) : h.hit_geom_index);
      A.hits0[pidx] = make_int2(code, h.objMaterialIdx);
      pidx = -1;
    }
    if (exhausted && !__any(pidx >= 0)) break;
    if (++rounds > (1ll << 20)) {  // unreachable: every round finishes or advances some ray
      if (lane == 0) atomicOr(S.fault, 8);
      break;
    }
  }
  if (COUNT) {
    prof_lap(P, PROF_POST_CYC);
    if (lane == 0 && P->tail_t0) P->prof[PROF_TAIL_CYC] += __builtin_readcyclecounter() - P->tail_t0;
    flush_counters(A.counters, cnt, P, t_k0);
    if (lane == 0) {
      const unsigned long long us10 = (__builtin_amdgcn_s_memrealtime() - rt0) / 1000;  // 100 MHz ticks
      atomicAdd(&A.counters->life[us10 < 63 ? us10 : 63], 1ull);
    }
  }
#ifdef KDPT_TAIL_PROF
  if (lane == 0 && tex_seen) atomicMin(&s_tex, tex_seen);
#endif
  if (lane == 0 && atomicAdd(&s_waves_done, 1) == TB / 64 - 1) {
    atomicMax(&A.trace_t[2 * A.depth + 1], (unsigned long long)__builtin_amdgcn_s_memrealtime());
#ifdef KDPT_TAIL_PROF
    // this workgroup's life, and its part after its first wave found the ray queue empty
    const unsigned long long t1 = __builtin_amdgcn_s_memrealtime();
    const unsigned long long tex = s_tex == ~0ull ? t1 : s_tex;
    atomicAdd(&g_tail_prof[0], t1 - s_t0);
    atomicAdd(&g_tail_prof[1], t1 - (tex < s_t0 ? s_t0 : tex));
    atomicAdd(&g_tail_prof[2], 1ull);
#endif
  }
}

}  // namespace
