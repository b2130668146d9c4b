// kdpt_trace_phase.h -- the wave-cooperative traversal k_trace runs (HIP only): node and cluster sources, the
// wave's LDS record, one lane's ray state (WaveRay) and trace_phase.
#pragma once

#include "kdpt_cull.h"
#include "kdpt_traverse.h"
#include "kdpt_wave.h"

namespace kdpt {

// ---------------------------------------------------------------------------
// Wave-cooperative form of traverseKD for gfx950 (64-lane waves).
//
// The per-ray algorithm and visited state are exactly traverseKD's; only the
// SIMT schedule changes ("while-while"): a node phase advances every lane until
// it reaches a leaf whose triangles must be tested (or finishes), then a leaf
// phase spreads ALL (ray, triangle) pairs of the lanes sitting on leaves over the
// 64 lanes.  A leaf's triangle tests are independent of each other; their
// sequential effects are recombined per ray through LDS:
//   bary.z        = that of the LAST triangle (in leaf order) passing the u/v tests
//   objMaterialIdx= mtlIdx of the LAST intersected triangle
//   hit record    = FIRST triangle reaching the minimum t with t > 0 && t_min > t
//   skip marks    = applied min(#intersected, 2) times (idempotent from the 2nd on)
// ---------------------------------------------------------------------------

// intersectAABB's decision (hit, and dist when hit) with IEEE min/max (v_min3/v_max3).
// Equal to the std::min/max ternaries whenever no product is NaN -- i.e. whenever every
// invdir component is finite -- because the results only feed comparisons (+-0 alike).
__device__ inline bool intersectAABB_fast(f3 o, f3 invdir, float4 b0, float4 b1, float& dist) {
  const float v1 = (b0.x - o.x) * invdir.x, v2 = (b0.w - o.x) * invdir.x;
  const float v3 = (b0.y - o.y) * invdir.y, v4 = (b1.x - o.y) * invdir.y;
  const float v5 = (b0.z - o.z) * invdir.z, v6 = (b1.y - o.z) * invdir.z;
  // v_min/v_max straight from the products: the compiler's fminf/fmaxf would first quiet each input
  // (six v_max x, x, x per node step) although a product is never a signalling NaN
  float l1, l2, l3, h1, h2, h3, dmin, dmax;
  asm("v_min_f32 %0, %1, %2" : "=v"(l1) : "v"(v1), "v"(v2));
  asm("v_min_f32 %0, %1, %2" : "=v"(l2) : "v"(v3), "v"(v4));
  asm("v_min_f32 %0, %1, %2" : "=v"(l3) : "v"(v5), "v"(v6));
  asm("v_max_f32 %0, %1, %2" : "=v"(h1) : "v"(v1), "v"(v2));
  asm("v_max_f32 %0, %1, %2" : "=v"(h2) : "v"(v3), "v"(v4));
  asm("v_max_f32 %0, %1, %2" : "=v"(h3) : "v"(v5), "v"(v6));
  asm("v_max3_f32 %0, %1, %2, %3" : "=v"(dmin) : "v"(l1), "v"(l2), "v"(l3));
  asm("v_min3_f32 %0, %1, %2, %3" : "=v"(dmax) : "v"(h1), "v"(h2), "v"(h3));
  dist = dmin;
  return !(dmax < 0.0f) && !(dmin > dmax);
}

// ---------------------------------------------------------------------------
// Node sources.  The traversal reads one node per step; where it reads it from
// is a template parameter:
//   NodesWide   : 64-byte records in HBM (any tree the validator accepts)
//   NodesPacked : 32-byte records (4 per 128-byte line), in HBM or -- when the
//                 kernel has copied the tree there -- in LDS.  Packing:
//     w0..w5 = min.xyz, max.xyz (float bits)
//     w6     = left | right << 16 (0xffff = -1), or triStart for a leaf with triangles
//     w7     = parent (16 bits, 0xffff = -1) | axis << 16 | hasTris << 18 | triSize << 19 (leaf with
//              triangles), else hasLeft << 19 | hasRight << 20 (the node step reads them as one field)
//   eligible when num_nodes < 65535, axis in 0..2, and every node with triangles
//   is childless with triSize < 8192 (checked on the host, else NodesWide).
// ---------------------------------------------------------------------------
struct NodeRec {
  float4 b0;     // min.xyz, max.x
  float4 b1;     // max.y, max.z, -, -
  int left, right, parent, axis, triStart, triSize;  // left / right: child index when hasL / hasR
  bool hasL, hasR;
  uint32_t has;  // hasL | hasR << 1
  bool tris;     // triSize > 0
  // NodesDerived only: the value both children write into their copy of this box (the centre along
  // `axis`), the value of the box coordinate this node changed in its parent's box, and that coordinate's
  // slot kc (0-2 min.xyz, 3-5 max.xyz; 7 for the root)
  float center, restore;
  uint32_t kc;
};

struct NodesWide {
  static constexpr bool kLeafHoldsCluster = false;  // big leaves: clusters from DevScene::leaf_cl
  static constexpr bool kDerivedBox = false;        // the record holds the node's box
  const int4* p;
  __device__ NodeRec operator()(int i) const {
    const int4 q0 = p[4 * i], q1 = p[4 * i + 1], q2 = p[4 * i + 2];
    NodeRec r;
    r.b0 = make_float4(ibits(q0.x), ibits(q0.y), ibits(q0.z), ibits(q0.w));
    r.b1 = make_float4(ibits(q1.x), ibits(q1.y), 0.0f, 0.0f);
    r.left = q1.z;
    r.right = q1.w;
    r.hasL = q1.z != -1;
    r.hasR = q1.w != -1;
    r.has = (r.hasL ? 1u : 0u) | (r.hasR ? 2u : 0u);
    r.parent = q2.x;
    r.triStart = q2.y;
    r.triSize = q2.z;
    r.tris = r.triSize > 0;
    r.axis = q2.w;
    return r;
  }
};

__device__ inline int link16(uint32_t v) { return v == 0xffffu ? -1 : (int)v; }

struct NodesPacked {
  static constexpr bool kLeafHoldsCluster = true;  // big leaves: triStart holds the first cluster
  static constexpr bool kDerivedBox = false;
  const int4* p;  // global or LDS (address space inferred after inlining)
  __device__ NodeRec operator()(int i) const {
    // two 16-byte vector loads (as int4 fields the compiler reads the record in four pieces)
    typedef int v4i __attribute__((ext_vector_type(4)));
    const v4i q0 = reinterpret_cast<const v4i*>(p)[2 * i], q1 = reinterpret_cast<const v4i*>(p)[2 * i + 1];
    NodeRec r;
    r.b0 = make_float4(ibits(q0.x), ibits(q0.y), ibits(q0.z), ibits(q0.w));
    r.b1 = make_float4(ibits(q1.x), ibits(q1.y), 0.0f, 0.0f);
    const uint32_t w6 = (uint32_t)q1.z, w7 = (uint32_t)q1.w;
    const bool tris = (w7 >> 18) & 1u;
    r.left = (int)(w6 & 0xffffu);  // raw: only read when hasL / hasR
    r.right = (int)(w6 >> 16);
    r.has = tris ? 0u : (w7 >> 19) & 3u;
    r.hasL = (r.has & 1u) != 0u;
    r.hasR = (r.has & 2u) != 0u;
    r.tris = tris;
    r.parent = link16(w7 & 0xffffu);
    r.axis = (int)((w7 >> 16) & 3u);
    r.triStart = (int)w6;
    r.triSize = tris ? (int)(w7 >> 19) : 0;
    return r;
  }
};

// NodesDerived: 16-byte records (LDS), half of NodesPacked, so that two intersect workgroups share a CU and
// the C5 icosphere's tree fits in LDS.  The reference's builder gives every child its parent's box with ONE
// coordinate replaced by the parent's centre along the parent's axis (src/KDnode.cpp:209-213,235-239: max
// for the left child, min for the right), and the traversal only ever moves parent <-> child, so a lane
// keeps the current node's box in registers and updates that one coordinate per move -- the same float
// bits the record would have held (kdpt_create checks the derivation on every node, else no NodesDerived).
//     w0 = restore: the parent's value of the coordinate this node replaced (climbing puts it back)
//     w1 = centre along axis (the value a descent writes), or the first triangle / cluster of a leaf
//     w2 = left | right << 16 (0xffff = -1), or triSize of a leaf with triangles
//     w3 = parent (16 bits) | axis << 16 | hasTris << 18 | hasLeft << 19 | hasRight << 20 | kc << 21
struct NodesDerived {
  static constexpr bool kLeafHoldsCluster = true;
  static constexpr bool kDerivedBox = true;
  const int4* p;
  __device__ NodeRec operator()(int i) const {
    typedef int v4i __attribute__((ext_vector_type(4)));
    const v4i q = reinterpret_cast<const v4i*>(p)[i];  // one 16-byte load
    const uint32_t w2 = (uint32_t)q.z, w3 = (uint32_t)q.w;
    const bool tris = (w3 >> 18) & 1u;
    NodeRec r;
    r.b0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    r.b1 = r.b0;
    r.restore = ibits(q.x);
    r.center = ibits(q.y);
    r.triStart = q.y;
    r.left = (int)(w2 & 0xffffu);  // raw: only read when hasL / hasR
    r.right = (int)(w2 >> 16);
    r.triSize = tris ? (int)w2 : 0;
    r.has = tris ? 0u : (w3 >> 19) & 3u;
    r.hasL = (r.has & 1u) != 0u;
    r.hasR = (r.has & 2u) != 0u;
    r.tris = tris;
    r.parent = link16(w3 & 0xffffu);
    r.axis = (int)((w3 >> 16) & 3u);
    r.kc = (w3 >> 21) & 7u;
    return r;
  }
};

// wave-profile slots (count mode): trips / cycles of each part of the intersect kernel
enum ProfSlot {
  PROF_NODE_TRIPS, PROF_NODE_CYC, PROF_BIG_SWEEPS, PROF_BIG_CYC, PROF_SMALL_PHASES, PROF_SMALL_ROUNDS,
  PROF_SMALL_CYC, PROF_FINAL_CYC, PROF_SETUP_CYC, PROF_GEOM_CYC, PROF_POST_CYC, PROF_SPARE,
  PROF_BIG_LEAVES, PROF_BIG_CLUSTERS, PROF_BIG_PASS, PROF_BIG_MULTI, PROF_SMALL_PAIRS, PROF_NODE_LEAFWAIT,
  PROF_NODE_DONE, PROF_TAIL_CYC, PROF_TAIL_NODE_DONE, PROF_BIG_SUPERS, PROF_BIG_CULL_CYC, PROF_SLOTS
};

// Cluster boxes of the big leaves: separate lo/hi arrays (HBM) or interleaved lo, hi (LDS copy).
struct ClustersSplit {
  static constexpr bool kSuper = false;
  const float4* lo;
  const float4* hi;
  __device__ float4 lo_of(int c) const { return lo[c]; }
  __device__ float4 hi_of(int c) const { return hi[c]; }
};
struct ClustersInterleaved {
  static constexpr bool kSuper = false;
  const float4* p;
  __device__ float4 lo_of(int c) const { return p[2 * c]; }
  __device__ float4 hi_of(int c) const { return p[2 * c + 1]; }
};
// Two-level: the super-cluster records in LDS (16 bytes: half-precision box rounded outward, first cluster
// and count), the cluster boxes in HBM/L2.
struct ClustersSuper {
  static constexpr bool kSuper = true;
  const int4* sp;
  const float4* lo;
  const float4* hi;
  const float4* n;  // slab normals (DevScene::cl_n)
  const float4* u;  // the oriented box's in-plane slabs (DevScene::cl_u, cl_v, cl_w)
  const float4* v;
  const float4* w;
  __device__ float4 n_of(int c) const { return n[c]; }
  // box of super k, and its first cluster << 5 | count - 1
  __device__ uint32_t sup(int k, float4& l, float4& h) const {
    typedef int v4i __attribute__((ext_vector_type(4)));
    const v4i q = reinterpret_cast<const v4i*>(sp)[k];  // one 16-byte LDS load
    const uint32_t w0 = (uint32_t)q.x, w1 = (uint32_t)q.y, w2 = (uint32_t)q.z;
    l = make_float4(half_lo(w0), half_hi(w0), half_lo(w1), 0.0f);
    h = make_float4(half_hi(w1), half_lo(w2), half_hi(w2), 0.0f);
    return (uint32_t)q.w;
  }
  __device__ float4 lo_of(int c) const { return lo[c]; }
  __device__ float4 hi_of(int c) const { return hi[c]; }
};

struct WaveLeafLDS {
  int slot[64];    // pair_owner's scatter slots (all zero between calls)
  int tbase[64];   // item (cluster / triangle) index = tbase[owner] + pair index
  float4 od[64];   // ray origin.xyz, direction.x
  float2 dd[64];   // direction.y, direction.z
  unsigned long long lastPass[64];  // ((tri + 1) << 32) | bary.z bits, max
  int lastHit[64];
  int nhit[64];
  unsigned long long best[64];  // (t bits << 32) | triangle index, min
};

// Count mode only (the counting intersect kernel allocates one per wave, the others one unused record, so
// their LDS stays small enough for a shading workgroup to share the CU), kept by lane 0: slots PROF_*,
// the wave's clock when its ray queue ran dry, last timestamp.
struct WaveProf {
  unsigned long long prof[PROF_SLOTS];
  unsigned long long tail_t0;
  unsigned long long tlast;
};

__device__ inline void prof_add(WaveProf* P, int k, unsigned long long v) {
  if ((threadIdx.x & 63) == 0) P->prof[k] += v;
}
__device__ inline void prof_lap(WaveProf* P, int k) {  // cycles since the last lap into prof[k]
  const unsigned long long now = __builtin_readcyclecounter();
  if ((threadIdx.x & 63) == 0) {
    if (k >= 0) P->prof[k] += now - P->tlast;
    P->tlast = now;
  }
}

__device__ inline TriData tri_load(const DevScene& S, int i) { return TriData{S.tv0[i], S.te1[i], S.te2[i]}; }


__device__ inline int tri_test(const DevScene& S, int i, f3 o, f3 d, float& bx, float& by, float& bz) {
  return tri_test_v(tri_load(S, i), o, d, bx, by, bz);
}


template <bool HYBRID>
__device__ inline float tri_hit_t(const DevScene& S, int i, f3 o, f3 d, float bx, float by, float bz, f3& hit,
                                  f3& norm) {
  return tri_hit_t_n<HYBRID>(S.tn0[i], S.tn1[i], S.tn2[i], o, d, bx, by, bz, hit, norm);
}

// One lane's ray and traversal state: exactly traverseKD's locals, kept across trace_phase calls so
// that the intersect kernel can give a lane a new ray whenever its previous one is finished.
struct WaveRay {
  f3 o, d, invdir;
  int cur, L;
  uint32_t cb, ps, g;
  bool rootv, sink, hitGeom, done, fault;
  float bz;
  int guard;
  Hit h;
  int objTri;  // the triangle whose hit record won (valid when h.obj_intersect)
  float lx, ly, lz, hx, hy, hz;  // NodesDerived: the box of node cur (min.xyz, max.xyz)
};

// Replace box slot k (0-2 min.xyz, 3-5 max.xyz; anything else: none) by v.
__device__ __attribute__((always_inline)) inline void box_set(WaveRay& R, uint32_t k, float v) {
  R.lx = k == 0u ? v : R.lx;
  R.ly = k == 1u ? v : R.ly;
  R.lz = k == 2u ? v : R.lz;
  R.hx = k == 3u ? v : R.hx;
  R.hy = k == 4u ? v : R.hy;
  R.hz = k == 5u ? v : R.hz;
}

// Start a ray: t_min / hit_geom_index come from the analytic geoms (k_geoms), tested first as in
// pathTraceOneBounceKDbare.
__device__ inline void wave_ray_start(const DevScene& S, WaveRay& R, f3 o, f3 d, float t_geom, int geom,
                                      WaveLeafLDS* W) {
  const int lane = threadIdx.x & 63;
  R.o = o;
  R.d = d;
  R.invdir = mk3(1.0f / d.x, 1.0f / d.y, 1.0f / d.z);
  R.cur = S.root;
  R.L = 0;
  R.cb = R.ps = R.g = 0;
  R.rootv = R.sink = R.hitGeom = R.done = R.fault = false;
  R.bz = FLT_MAXV;
  R.guard = 0;
  R.h.t_min = t_geom;
  R.h.hit_geom_index = geom;
  R.h.obj_intersect = false;
  R.h.objMaterialIdx = -1;
  R.h.ip = mk3(0, 0, 0);
  R.h.normal = mk3(0, 0, 0);
  R.objTri = -1;
  R.lx = S.rlo.x;  // the root's box (NodesDerived)
  R.ly = S.rlo.y;
  R.lz = S.rlo.z;
  R.hx = S.rhi.x;
  R.hy = S.rhi.y;
  R.hz = S.rhi.z;
  W->od[lane] = make_float4(o.x, o.y, o.z, d.x);
  W->dd[lane] = make_float2(d.y, d.z);
}

// ---------------------------------------------------------------------------
// trace_phase, in the order it runs: node_phase -> leaf_record -> big leaves (cull_two_level or cull_one_level,
// both sweeping their survivors with sweep_clusters) -> small_leaves -> leaf_commit.  The leaf's record (LeafRec)
// and the fold of its triangles' results (LeafFold) are the state the parts share; the ray's own state is WaveRay.
// Every part is inlined into trace_phase.
// ---------------------------------------------------------------------------

// What the node phase leaves a lane with: it sits on a leaf whose triangles must be tested, and the side the
// hybrid walk takes first there (the skip line's operand).
struct LeafFlags {
  bool leaf, lfirst;
};

// The leaf's own record, read once after the node phase rather than carried through every node trip.
struct LeafRec {
  int start, size, parent;  // first triangle (first cluster / super of a big leaf: NodeSrc), triangles, parent node
  int clusters;             // a big leaf's cluster count
  uint32_t kc;              // NodesDerived: the box slot this node replaced, and its parent's value
  float restore;
};

// A leaf's results folded per ray, order-free: the last u/v pass as ((tri + 1) << 32) | bary.z bits (max; 0 = none),
// the best hit as (t bits << 32) | tri (min; ~0 = none), the last intersected triangle (max) and the number of
// intersected ones.  The big-leaf sweeps fold into the owner lane's record, the small leaves through
// WaveLeafLDS's slots; leaf_commit alone unpacks it.  The sweeps and the culls take the record by value and
// return it, small_leaves by reference, and the big leaves fold into a record of their own that their lanes then
// take: the forms that keep every k_trace's registers and scratch (the sweep's by reference spills one register
// more on every LDS-tree route; profiles/trace_phase_split_ab_log.md).
struct LeafFold {
  unsigned long long pass, best;
  int lasthit, nhit;
};
constexpr LeafFold kNoFold{0ull, ~0ull, -1, 0};

// The ray of a pair's owner lane: origin and direction from the wave's LDS copy (wave_ray_start), the
// reciprocal from the owner's registers.  Wave-uniform call (ds_bpermute).
struct PairRay {
  f3 o, d, inv;
};
__device__ __attribute__((always_inline)) inline PairRay pair_ray(const WaveLeafLDS* W, f3 invdir, int own) {
  const float4 od = W->od[own];
  const float2 d2 = W->dd[own];
  PairRay p;
  p.o = mk3(od.x, od.y, od.z);
  p.d = mk3(od.w, d2.x, d2.y);
  p.inv = mk3(bpermute_f(invdir.x, own), bpermute_f(invdir.y, own), bpermute_f(invdir.z, own));
  return p;
}

// One node phase of traverseKD for every lane of the wave with an unfinished ray: lanes walk until they sit on
// a leaf with triangles or finish (R.done).  Only this function knows the packed flag word.
template <bool HYBRID, bool COUNT, typename NodeSrc>
__device__ __attribute__((always_inline)) inline LeafFlags node_phase(
    const DevScene& S, const NodeSrc& nodes, WaveRay& R, bool fastAABB, TraverseCounters& cnt, WaveProf* WP) {
  const int lane = threadIdx.x & 63;
  const f3 o = R.o, d = R.d, invdir = R.invdir;
  int& cur = R.cur;
  int& L = R.L;
  uint32_t& cb = R.cb;
  uint32_t& ps = R.ps;
  const uint32_t g = R.g;
  const float bz = R.bz;
  int& guard = R.guard;
  int trips = 0;
  if (COUNT) prof_lap(WP, -1);
  // One trip = one step of the reference's loop for every lane still walking nodes.  The
  // body runs for the whole wave and commits by selects on `walk`, and the per-lane flags
  // live in one register, so a trip carries no exec-mask bookkeeping.  Exact for a
  // validated tree (only the root has parentID == -1): at the root `up` ends the walk (the
  // reference exits before or after its test, or climbs to -1), so hitGeom only feeds the
  // AABB count.
  enum : uint32_t { F_ROOTV = 1, F_SINK = 2, F_HITGEOM = 4, F_DONE = 8, F_LEAF = 16, F_LFIRST = 32, F_FAULT = 64 };
  uint32_t fl = (R.rootv ? F_ROOTV : 0u) | (R.sink ? F_SINK : 0u) | (R.hitGeom ? F_HITGEOM : 0u) |
                (R.done ? F_DONE : 0u) | F_LFIRST;
  // leftFirst = d[axis] > 0 (comp: axis 0, 1, anything else z) as one bit test per trip
  const uint32_t dpos = (d.x > 0.0f ? 1u : 0u) | (d.y > 0.0f ? 2u : 0u) | (d.z > 0.0f ? 4u : 0u);
  while (true) {
    const bool walk = (fl & (F_DONE | F_LEAF)) == 0u;
    const unsigned long long wmask = __ballot(walk);
    if (!wmask) break;
    // Few lanes still walking and many waiting on leaves: test those leaves now; the walkers keep
    // their state and resume in the next node phase (their own sequence of steps is unchanged).
    if (__popcll(wmask) <= S.early_walk && __popcll(__ballot((fl & F_LEAF) != 0u)) >= S.early_leaf) break;
    if (COUNT) {
      trips += walk ? 1 : 0;
      prof_add(WP, PROF_SPARE, (unsigned long long)__popcll(wmask));  // lane-steps: SIMD efficiency
      prof_add(WP, PROF_NODE_LEAFWAIT, (unsigned long long)__popcll(__ballot((fl & F_LEAF) != 0u)));
      const unsigned long long nd_done = (unsigned long long)__popcll(__ballot((fl & F_DONE) != 0u));
      prof_add(WP, PROF_NODE_DONE, nd_done);
      if (WP->tail_t0) prof_add(WP, PROF_TAIL_NODE_DONE, nd_done);
    }
    const NodeRec nd = nodes(cur < 0 ? 0 : cur);
    const int left = nd.left, right = nd.right;
    const uint32_t Lu = (uint32_t)L;
    const uint32_t vb = (2u * Lu - 2u + ((ps >> ((Lu - 1u) & 31u)) & 1u)) & 31u;  // own flag (L > 0)
    const bool curVis = (L == 0) ? ((fl & F_ROOTV) != 0u) : (((cb >> vb) & 1u) != 0u);
    const bool isRoot = cur == S.root;
    const float4 nb0 = NodeSrc::kDerivedBox ? make_float4(R.lx, R.ly, R.lz, R.hx) : nd.b0;
    const float4 nb1 = NodeSrc::kDerivedBox ? make_float4(R.hy, R.hz, 0.0f, 0.0f) : nd.b1;
    float dd;
    const bool hg = fastAABB ? intersectAABB_fast(o, invdir, nb0, nb1, dd)
                             : intersectAABB(o, invdir, nb0, nb1, dd);
    const bool up = curVis || !hg || dd > bz;
    // Child choice on bit masks: `has` = children present (bit 0 left, bit 1 right), `avail` = present and not
    // yet visited at this level; the near side (fside: 0 left, 1 right) is taken when available, else the far
    // one.  takeFirst / takeSecond of traverseKDbareShortHybrid are avail's fside / far bits, so descend =
    // avail != 0 and the child is simply the one on side nside.
    const uint32_t fside = HYBRID ? (((dpos >> min((uint32_t)nd.axis, 2u)) & 1u) ^ 1u) : 0u;
    const uint32_t has = nd.has;
    const uint32_t sh2 = (2u * Lu) & 31u;
    const uint32_t avail = has & ~(cb >> sh2);  // (bits 0-1 only: has is)
    const uint32_t nside = ((avail >> fside) & 1u) ? fside : (fside ^ 1u);
    const bool descend = !up && avail != 0u;
    const bool lf = !up && avail == 0u && nd.tris;
    // "Mark and stay" on a node without triangles is always followed by a trip on the same
    // node that finds it visited and climbs (same box, so same hitGeom): do both now.
    const bool stay = !up && avail == 0u && !nd.tris;
    const bool climb = up || stay;
    if (COUNT && walk) cnt.aabb += (isRoot && curVis && !(fl & F_HITGEOM)) ? 0u : (stay ? 2u : 1u);
    // nodeIDs[ID] = true unless descending; nodeIDs[left] = nodeIDs[right] = true when climbing (neither
    // when descending: then only the new level's child flags are cleared, and the root's own flag moves
    // into g's slot)
    // (both forms computed, then one select: as an if/else the compiler branches on exec masks)
    const uint32_t cb_down = (cb & ~(3u << ((2u * Lu + 2u) & 31u))) | ((L == 0 && nside == 0u) ? (g << 2) : 0u);
    const uint32_t cb_here = cb | (L > 0 ? (1u << vb) : 0u) | (climb ? (has << sh2) : 0u);
    const uint32_t ncb = descend ? cb_down : cb_here;
    const bool runaway = guard >= S.trip_limit;
    uint32_t nfl = fl & ~(F_HITGEOM | F_LFIRST);
    nfl |= (!descend && L == 0) ? F_ROOTV : 0u;
    nfl |= (climb && has != 3u) ? F_SINK : 0u;
    nfl |= hg ? F_HITGEOM : 0u;
    nfl |= ((isRoot && climb) || runaway) ? F_DONE : 0u;
    nfl |= runaway ? F_FAULT : 0u;
    nfl |= lf ? F_LEAF : 0u;
    nfl |= fside == 0u ? F_LFIRST : 0u;
    if (walk) {  // commit (selects)
      cb = ncb;
      ps = descend ? ((ps & ~(1u << (Lu & 31u))) | (nside << (Lu & 31u))) : ps;
      cur = climb ? nd.parent : (descend ? (nside ? right : left) : cur);
      L += descend ? 1 : (climb ? -1 : 0);
      guard++;
      fl = nfl;
      if (NodeSrc::kDerivedBox) {
        // descending: the child's box is this one with max[axis] (left child) / min[axis] (right) set to the
        // centre; climbing: the parent's box is this one with the coordinate this node replaced put back
        const uint32_t kd = (nside ? 0u : 3u) + (uint32_t)nd.axis;
        box_set(R, descend ? kd : (climb ? nd.kc : 7u), descend ? nd.center : nd.restore);
      }
    }
  }
  R.rootv = (fl & F_ROOTV) != 0u;
  R.sink = (fl & F_SINK) != 0u;
  R.hitGeom = (fl & F_HITGEOM) != 0u;
  R.done = (fl & F_DONE) != 0u;
  R.fault = R.fault || (fl & F_FAULT) != 0u;
  if (COUNT) {
    prof_lap(WP, PROF_NODE_CYC);
    for (int off = 32; off > 0; off >>= 1) trips = max(trips, __shfl_xor(trips, off));
    prof_add(WP, PROF_NODE_TRIPS, (unsigned long long)trips);  // wave-level trips = the slowest lane's
  }
  if (__any(R.fault) && lane == 0) atomicOr(S.fault, 1);
  return LeafFlags{(fl & F_LEAF) != 0u, (fl & F_LFIRST) != 0u};
}

// The record of the leaf a lane sits on (a lane that reaches a leaf neither climbs nor descends, so cur is the
// leaf).
template <typename NodeSrc>
__device__ __attribute__((always_inline)) inline LeafRec leaf_record(
    const DevScene& S, const NodeSrc& nodes, int cur, bool leaf) {
  LeafRec lf{0, 0, -1, 0, 7u, 0.0f};
  if (leaf) {
    const NodeRec ln = nodes(cur);
    lf.start = ln.triStart;
    lf.size = ln.triSize;
    lf.parent = ln.parent;
    if (NodeSrc::kDerivedBox) {
      lf.kc = ln.kc;
      lf.restore = ln.restore;
    }
    // a big leaf's cluster count: Morton runs of CLUSTER fill all but the last, unless the scene groups by
    // normal cones (S.cl_counts: the count from leaf_cl, requested here, read at the leaf phase)
    lf.clusters = (lf.size + CLUSTER - 1) / CLUSTER;
    if (S.cl_counts && lf.size >= BIG_LEAF) lf.clusters = S.leaf_cl[cur].y;
  }
  return lf;
}

// Sweeps of the (ray, cluster) pairs `pass` marks: cluster c with the ray of lane own, each surviving
// cluster by the whole wave, the next survivor's triangles fetched while this one is tested; the results
// are folded into the owner lane's F (order-free).  Wave-uniform call.
template <bool HYBRID, bool COUNT>
__device__ __attribute__((always_inline)) inline LeafFold sweep_clusters(
    const DevScene& S, const WaveRay& R, LeafFold F, WaveProf* WP, bool pass, int c, int own) {
  const int lane = threadIdx.x & 63;
  const f3 o = R.o, d = R.d;
  unsigned long long sm = __ballot(pass);
  int s = -1;
  TriData T{};
  if (sm) {
    s = __builtin_ctzll(sm);
    sm &= sm - 1;
    const int ct = __builtin_amdgcn_readlane(c, s) * 64 + lane;
    T = TriData{S.c_v0[ct], S.c_e1[ct], S.c_e2[ct]};
  }
  while (s >= 0) {
    int sn = -1;
    TriData Tn{};
    if (sm) {
      sn = __builtin_ctzll(sm);
      sm &= sm - 1;
      const int ctn = __builtin_amdgcn_readlane(c, sn) * 64 + lane;
      Tn = TriData{S.c_v0[ctn], S.c_e1[ctn], S.c_e2[ctn]};
    }
    if (COUNT) prof_add(WP, PROF_BIG_SWEEPS, 1);
    const int j = __builtin_amdgcn_readlane(own, s);  // the cluster's ray: lane j's, wave-uniform
    const f3 jo = mk3(readlane_f(o.x, j), readlane_f(o.y, j), readlane_f(o.z, j));
    const f3 jd = mk3(readlane_f(d.x, j), readlane_f(d.y, j), readlane_f(d.z, j));
    const int orig = fbits(T.e1.w);
    float bx = 0, by = 0, bzk = 0;
    const int r = tri_test_v(T, jo, jd, bx, by, bzk);
    const unsigned long long m1 = __ballot(r >= 1);
    if (COUNT && m1) {
      prof_add(WP, PROF_BIG_PASS, 1);
      prof_add(WP, PROF_BIG_MULTI, (m1 & (m1 - 1)) ? 1 : 0);
    }
    if (m1) {
      const unsigned long long pk =
          r >= 1 ? ((unsigned long long)(unsigned int)(orig + 1) << 32) | f2u(bzk) : 0ull;
      // usually one lane of the cluster passes: read its key instead of reducing over the wave
      const unsigned long long wm = (m1 & (m1 - 1)) == 0ull ? readlane_u64(pk, __builtin_ctzll(m1))
                                                            : wave_max_u64(pk);
      if (lane == j) F.pass = wm > F.pass ? wm : F.pass;
      const unsigned long long m2 = __ballot(r == 2);
      if (m2) {
        const bool one = (m2 & (m2 - 1)) == 0ull;
        const int jh = __builtin_ctzll(m2);
        const int lh = one ? __builtin_amdgcn_readlane(orig, jh) : wave_max_i32(r == 2 ? orig : -1);
        unsigned long long key = ~0ull;
        if (r == 2) {
          f3 hp, nn;
          const float t = tri_hit_t<HYBRID>(S, orig, jo, jd, bx, by, bzk, hp, nn);
          if (t > 0.0f) key = ((unsigned long long)f2u(t) << 32) | (unsigned int)orig;
        }
        const unsigned long long wb = one ? readlane_u64(key, jh) : wave_min_u64(key);
        if (lane == j) {
          F.nhit += __builtin_popcountll(m2);
          F.lasthit = max(F.lasthit, lh);
          F.best = wb < F.best ? wb : F.best;
        }
      }
    }
    s = sn;
    T = Tn;
  }
  return F;
}

// Big leaves, two levels (leaves of thousands of triangles, e.g. the C5 icosphere's): the (ray, super-cluster)
// pairs are culled first, 64 per pass, against the supers' boxes (LDS); each surviving super's SUPER clusters
// are then culled against their own boxes, 64 / SUPER supers per round, and the survivors swept.  A
// super's box holds its clusters' boxes, so the second level sees every cluster the one-level cull
// would pass.  ncl: the lane's cluster count (0: not on a big leaf); first: its leaf's first super.
template <bool HYBRID, bool COUNT, typename ClusterSrc>
__device__ __attribute__((always_inline)) inline LeafFold cull_two_level(
    const DevScene& S, const ClusterSrc& clusters, const WaveRay& R, bool fastAABB, int first, int ncl, LeafFold F,
    WaveLeafLDS* W, WaveProf* WP) {
  const int lane = threadIdx.x & 63;
  const int nsp = (ncl + SUPER - 1) / SUPER;
  const int incl = wave_incl_scan<false>(nsp);
  const int P = __builtin_amdgcn_readlane(incl, 63);
  const int excl = incl - nsp;
  W->tbase[lane] = first - excl;  // super of pair q = tbase[owner] + q
  wave_lds_sync();
  if (COUNT) {
    prof_add(WP, PROF_BIG_LEAVES, (unsigned long long)__popcll(__ballot(ncl > 0)));
    prof_add(WP, PROF_BIG_SUPERS, (unsigned long long)P);
  }
  // one pass's surviving supers, {owner << 32 | first cluster << 5 | count - 1}, in W->best (the
  // small-leaf phase initialises it afresh)
  static_assert(SUPER <= 32 && 64 % SUPER == 0, "super-cluster size");
  unsigned long long* slist = W->best;
  int carry = 0;
  for (int B = 0; B < P; B += 64) {
    const int own = pair_owner(W->slot, excl, nsp, B, carry);
    const int sp = W->tbase[own] + B + lane;
    bool pass = B + lane < P;
    float4 slo = make_float4(0.0f, 0.0f, 0.0f, 0.0f), shi = slo, sn = slo, sb = slo;
    uint32_t sinfo = 0u;
    // the super's slab record (L2) is requested for every pair before the box test, so its latency
    // overlaps the LDS record, the ray exchange and the box test
    if (fastAABB && S.sup_slab && pass) {
      sn = S.sup_n[sp];
      sb = S.sup_b[sp];
    }
    if (pass) sinfo = clusters.sup(sp, slo, shi);
    if (fastAABB) {
      const PairRay pr = pair_ray(W, R.invdir, own);
      if (pass) pass = cluster_may_pass(slo, shi, pr.o, pr.inv, S.cl_margin);
      // the boxes' survivors against the super's slab (its record from L2), with the margin its normal
      // spread allows for this direction
      if (S.sup_slab && __any(pass)) {
        const CullK ck{S.cl_margin, S.cl_margin_lo, S.cull_a, S.cull_b, S.cull_c};
        if (pass) {
          pass = cluster_may_pass_slab(make_float4(slo.x, slo.y, slo.z, sb.x), make_float4(shi.x, shi.y, shi.z, sb.y),
                                       sn, pr.o, pr.inv, pr.d, ck);
        }
      }
    }
    const unsigned long long sm = __ballot(pass);
    const int nsv = __popcll(sm);
    if (pass)
      slist[lane_prefix(sm)] = ((unsigned long long)(uint32_t)own << 32) | sinfo;
    wave_lds_sync();
    for (int q = 0; q < nsv; q += 64 / SUPER) {
      const int e = q + lane / SUPER, k = lane % SUPER;
      bool cp = e < nsv;
      int cown = 0, c = 0;
      if (cp) {
        const unsigned long long ent = slist[e];
        cown = (int)(ent >> 32);
        c = (int)((uint32_t)ent >> 5) + k;
        cp = k <= (int)((uint32_t)ent & 31u);
      }
      if (COUNT) prof_add(WP, PROF_BIG_CLUSTERS, (unsigned long long)__popcll(__ballot(cp)));
      if (fastAABB) {
        // the oriented-box records (L2) requested before the ray exchange, so their latency overlaps it
        const float4 z4 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        float4 rlo = z4, rhi = z4, rn = z4, ru = z4, rv = z4, rw = z4;
        if (S.cl_slab && S.cl_obb && cp) {
          rlo = clusters.lo_of(c);
          rhi = clusters.hi_of(c);
          rn = clusters.n_of(c);
          ru = clusters.u[c];
          rv = clusters.v[c];
          rw = clusters.w[c];
        }
        const PairRay pr = pair_ray(W, R.invdir, cown);
        if (S.cl_slab) {
          const CullK ck{S.cl_margin, S.cl_margin_lo, S.cull_a, S.cull_b, S.cull_c};
          if (cp) {
            if (S.cl_obb)
              cp = cluster_may_pass_obb(rlo, rhi, rn, ru, rv, rw, pr.o, pr.inv, pr.d, ck);
            else
              cp = cluster_may_pass_slab(clusters.lo_of(c), clusters.hi_of(c), clusters.n_of(c), pr.o, pr.inv, pr.d,
                                         ck);
          }
        } else {
          if (cp) cp = cluster_may_pass(clusters.lo_of(c), clusters.hi_of(c), pr.o, pr.inv, S.cl_margin);
        }
      }
      if (COUNT) prof_lap(WP, PROF_BIG_CULL_CYC);
      F = sweep_clusters<HYBRID, COUNT>(S, R, F, WP, cp, c, cown);
      if (COUNT) prof_lap(WP, PROF_BIG_CYC);
    }
    wave_lds_sync();  // slist is rewritten by the next pass
  }
  return F;
}

// The masked cull's danger walk for the pairs the one-level cull missed (m: the pair's danger mask, 0 for a lane
// with none): the lane walks the mask's bits, deciding each triangle from its unit normal and the line's
// box_miss distance (danger_needs_test); the rare one that needs it gets glm's u/v tests.  true: a danger
// triangle passed them, the cluster must be swept.  Wave-uniform call.
template <typename ClusterSrc>
__device__ __attribute__((always_inline)) inline bool danger_walk(
    const DevScene& S, const ClusterSrc& clusters, const WaveLeafLDS* W, f3 invdir, int own, int c,
    unsigned long long m) {
  bool late = false;
  // (the line, its direction and its box recomputed rather than kept live across the sweep)
  const PairRay pr = pair_ray(W, invdir, own);
  unsigned long long nm = 0ull;  // the danger triangles danger_needs_test keeps
  if (m) {
    // one normal record per trip, the first requested before box_miss (the cluster box from LDS, the
    // line's reciprocal from its lane), so that its latency overlaps it (profiles/r06_ab_log.md r06l/r06m:
    // +1 % against two records per trip)
    const int e0 = c * 64;
    int k0 = __builtin_ctzll(m);
    m &= m - 1;
    float4 t0 = S.cl_tn[e0 + k0];
    const float D = box_miss(clusters.lo_of(c), clusters.hi_of(c), pr.o, pr.inv);
    while (true) {
      if (danger_needs_test(t0, pr.d, D, S.cull_c)) nm |= 1ull << k0;
      if (!m) break;
      k0 = __builtin_ctzll(m);
      m &= m - 1;
      t0 = S.cl_tn[e0 + k0];
    }
  }
  if (__any(nm != 0ull)) {  // (rare) glm's u/v tests on the kept ones
    while (nm && !late) {
      const int e = c * 64 + __builtin_ctzll(nm);
      nm &= nm - 1;
      float bx, by, bz;
      late = tri_test_v(TriData{S.c_v0[e], S.c_e1[e], S.c_e2[e]}, pr.o, pr.d, bx, by, bz) >= 1;
    }
  }
  return late;
}

// Big leaves, one level: lane L owns the (ray, cluster) pairs [excl_L, excl_L + ncl_L); one pass culls 64 of them
// against the cluster boxes (LDS) and the box survivors against the clusters' oriented boxes (L2), both
// widened at the fast coefficient cl_margin; the hits are swept by the whole wave.
// With direction masks (S.cl_mask: the exact cull, DESIGN.md 4 "Cluster cull") a miss may still hide a
// u/v pass of a triangle nearly parallel to the line: the cluster's danger mask for the ray's direction
// bucket (kdpt_clusters.h build_dir_masks) lists every triangle that can need more than cl_margin for
// some direction of the bucket.  The mask is requested with the box test and read after the pass's
// sweeps (its latency hidden behind them); danger_walk then decides the missed pairs.  A pass sweeps the whole
// cluster late, as the uncull'd walk would have: the sweep's results fold by max / min / sum, so a late sweep is
// the same as an early one.  ncl: the lane's cluster count (0: not on a big leaf); first: its leaf's first cluster.
template <bool HYBRID, bool COUNT, typename ClusterSrc>
__device__ __attribute__((always_inline)) inline LeafFold cull_one_level(
    const DevScene& S, const ClusterSrc& clusters, const WaveRay& R, bool fastAABB, int first, int ncl, LeafFold F,
    WaveLeafLDS* W, WaveProf* WP) {
  const int lane = threadIdx.x & 63;
  const bool exact = S.cl_mask != nullptr;
  const int incl = wave_incl_scan<false>(ncl);
  const int P = __builtin_amdgcn_readlane(incl, 63);
  const int excl = incl - ncl;
  W->tbase[lane] = first - excl;  // cluster of pair q = tbase[owner] + q
  wave_lds_sync();
  if (COUNT) {
    prof_add(WP, PROF_BIG_LEAVES, (unsigned long long)__popcll(__ballot(ncl > 0)));
    prof_add(WP, PROF_BIG_CLUSTERS, (unsigned long long)P);
  }
  int carry = 0;
  for (int B = 0; B < P; B += 64) {
    const int own = pair_owner(W->slot, excl, ncl, B, carry);
    const int c = W->tbase[own] + B + lane;
    bool hit = B + lane < P;  // (no cull: every pair swept)
    unsigned long long m = 0ull;  // a missed pair's danger mask (exact cull)
    if (fastAABB) {
      const PairRay pr = pair_ray(W, R.invdir, own);
      float4 clo = make_float4(0.0f, 0.0f, 0.0f, 0.0f), chi = clo;
      unsigned long long dm = 0ull;
      const bool valid = hit;
      if (valid) {
        if (exact) dm = S.cl_mask[(uint32_t)dir_bucket(pr.d, S.mask_n) * (uint32_t)S.num_clusters + (uint32_t)c];
        clo = clusters.lo_of(c);
        chi = clusters.hi_of(c);
        hit = cluster_may_pass(clo, chi, pr.o, pr.inv, S.cl_margin);
      }
      // the box's survivors against the cluster's oriented box (its slabs from L2)
      if (S.flat_obb && __any(hit)) {
        if (hit) {
          const float4 cn = S.cl_n[c];
          hit = cluster_may_pass_obb_k(clo, chi, cn, S.cl_u[c], S.cl_v[c], S.cl_w[c], pr.o, pr.inv, pr.d,
                                       cn.x * pr.d.x + cn.y * pr.d.y + cn.z * pr.d.z, S.cl_margin);
        }
      }
      if (exact && valid && !hit) m = dm;
    }
    if (COUNT) prof_lap(WP, PROF_BIG_CULL_CYC);
    F = sweep_clusters<HYBRID, COUNT>(S, R, F, WP, hit, c, own);
    if (COUNT) prof_lap(WP, PROF_BIG_CYC);
    if (!exact || !__any(m != 0ull)) continue;
    // a danger triangle passed glm's u/v tests: sweep the cluster now
    const bool late = danger_walk(S, clusters, W, R.invdir, own, c, m);
    if (COUNT) prof_lap(WP, PROF_BIG_CULL_CYC);
    if (__any(late)) F = sweep_clusters<HYBRID, COUNT>(S, R, F, WP, late, c, own);
    if (COUNT) prof_lap(WP, PROF_BIG_CYC);
  }
  return F;
}

// Small leaves: the items are triangles, every (ray, triangle) pair tested by one lane; results recombine
// through LDS atomics on the owner's slots.  sz: the lane's triangle count (0: not on a small leaf); first: its
// leaf's first triangle.
template <bool HYBRID, bool COUNT>
__device__ __attribute__((always_inline)) inline void small_leaves(
    const DevScene& S, int first, int sz, LeafFold& F, WaveLeafLDS* W, WaveProf* WP) {
  const int lane = threadIdx.x & 63;
  if (COUNT) prof_add(WP, PROF_SMALL_PHASES, 1);
  const int incl = wave_incl_scan<false>(sz);
  const int P = __builtin_amdgcn_readlane(incl, 63);
  const int excl = incl - sz;
  W->tbase[lane] = first - excl;  // triangle of pair q = tbase[owner] + q
  W->lastPass[lane] = 0ull;
  W->lastHit[lane] = -1;
  W->nhit[lane] = 0;
  W->best[lane] = ~0ull;
  wave_lds_sync();
  if (COUNT) {
    prof_add(WP, PROF_SMALL_ROUNDS, (unsigned long long)((P + 63) / 64));
    prof_add(WP, PROF_SMALL_PAIRS, (unsigned long long)P);
  }
  // the next round's owners are found and its triangles loaded while the current round is tested (two
  // rounds ahead spilled: -8 %, profiles/r04_ab_log.md)
  int carry = 0;
  int owner = pair_owner(W->slot, excl, sz, 0, carry);
  int tri = W->tbase[owner] + lane;
  TriData nxt{};
  if (lane < P) nxt = tri_load(S, tri);
  for (int B = 0; B < P; B += 64) {
    const TriData cur_t = nxt;
    const int cowner = owner, ctri = tri;
    const bool valid = B + lane < P;
    if (B + 64 < P) {
      owner = pair_owner(W->slot, excl, sz, B + 64, carry);
      tri = W->tbase[owner] + B + 64 + lane;
      if (B + 64 + lane < P) nxt = tri_load(S, tri);
    }
    if (valid) {
      // (the owner's origin and direction only: no reciprocal, so no lane exchange under this branch)
      const float4 q0 = W->od[cowner];
      const float2 q1 = W->dd[cowner];
      const f3 oo = mk3(q0.x, q0.y, q0.z), dd = mk3(q0.w, q1.x, q1.y);
      float bx, by, bzk;
      const int r = tri_test_v(cur_t, oo, dd, bx, by, bzk);
      if (r >= 1)
        atomicMax(&W->lastPass[cowner], ((unsigned long long)(unsigned int)(ctri + 1) << 32) | f2u(bzk));
      if (r == 2) {
        atomicMax(&W->lastHit[cowner], ctri);
        atomicAdd(&W->nhit[cowner], 1);
        f3 hp, nn;
        const float t = tri_hit_t<HYBRID>(S, ctri, oo, dd, bx, by, bzk, hp, nn);
        if (t > 0.0f) atomicMin(&W->best[cowner], ((unsigned long long)f2u(t) << 32) | (unsigned int)ctri);
      }
    }
  }
  wave_lds_sync();
  if (sz > 0) F = LeafFold{W->lastPass[lane], W->best[lane], W->lastHit[lane], W->nhit[lane]};
  wave_lds_sync();  // the LDS slots are rewritten by the next leaf phase
}

// A lane's leaf applied to its ray as the reference's sequential loop over the leaf's triangles would have:
// bary.z of the last u/v pass, the material of the last intersected triangle, the skip line, the best hit; then
// the climb out of the leaf.  The one place that unpacks LeafFold.
template <bool HYBRID, bool COUNT, typename NodeSrc>
__device__ __attribute__((always_inline)) inline void leaf_commit(
    const DevScene& S, WaveRay& R, const LeafRec& lf, const LeafFold& F, bool lfirst, int material_size,
    TraverseCounters& cnt) {
  if (COUNT) cnt.tri += lf.size;
  if ((int)(F.pass >> 32) > 0) R.bz = u2f((uint32_t)(F.pass & 0xffffffffu));
  const int nh = F.nhit;
  if (nh > 0) {
    if (COUNT) cnt.hit += nh;
    R.h.objMaterialIdx = fbits(S.tv0[F.lasthit].w) + material_size - 1;
    if (HYBRID) {
      for (int rep = 0; rep < (nh > 1 ? 2 : 1); rep++) skip_line_mark(S, R.L, lfirst, R.ps, R.rootv, R.cb, R.g, R.sink);
    }
    if (F.best != ~0ull) {
      const float tb = u2f((uint32_t)(F.best >> 32));
      const int k = (int)(uint32_t)(F.best & 0xffffffffu);
      if (R.h.t_min > tb) {  // tb is tri_hit_t's value for triangle k (the winner's point and
        R.h.t_min = tb;      // normal are recomputed from k by the shading kernel)
        R.h.hit_geom_index = S.obj_material_offsets[fbits(S.tv0[k].w)];
        R.h.obj_intersect = true;
        R.objTri = k;
      }
    }
  }
  // The reference's next trip finds the leaf visited and climbs (leaves have no children,
  // validated: nodeIDs[-1] = true twice); do it here instead of in the node phase.
  if (COUNT) cnt.aabb++;
  R.sink = true;
  R.done = R.cur == S.root;
  R.cur = lf.parent;
  R.L--;
  if (NodeSrc::kDerivedBox) box_set(R, lf.kc, lf.restore);  // back to the parent's box
}

// One node phase and one leaf phase of traverseKD for every lane of the wave with an unfinished ray
// (R.done false); lanes finish by setting R.done.  fastAABB must be wave-uniform (every active lane's
// invdir finite).
// The leaf phase is wave-cooperative.  Both leaf kinds enumerate (lane, item) pairs flattened over the wave:
// lane L owns pairs [excl_L, excl_L + count_L), and lane k of a round takes pair B + k, whichever ray it belongs
// to.  Big leaves: the items are 64-triangle clusters.  One pass culls 64 (ray, cluster) pairs (clusters
// whose box the ray's line misses, when every invdir is finite); each surviving cluster is then swept by
// the whole wave with its ray, 64 triangles at a time.  Recombination by ORIGINAL index into the owner lane
// (order-free): last u/v pass = max index, last hit = max, best = min (t, index).
template <bool HYBRID, bool COUNT, typename NodeSrc, typename ClusterSrc>
__device__ void trace_phase(const DevScene& S, const NodeSrc& nodes, const ClusterSrc& clusters, WaveRay& R,
                            bool fastAABB, int material_size, TraverseCounters& cnt, WaveLeafLDS* W,
                            WaveProf* WP) {
  const LeafFlags at = node_phase<HYBRID, COUNT>(S, nodes, R, fastAABB, cnt, WP);
  if (!__any(at.leaf)) return;
  const LeafRec lf = leaf_record(S, nodes, R.cur, at.leaf);
  LeafFold F = kNoFold;
  const bool big = at.leaf && lf.size >= BIG_LEAF;
  if (__any(big)) {
    const int ncl = big ? lf.clusters : 0;
    LeafFold K = kNoFold;  // the big leaves' results, folded into their owner lanes
    if constexpr (ClusterSrc::kSuper) {
      K = cull_two_level<HYBRID, COUNT>(S, clusters, R, fastAABB, lf.start, ncl, K, W, WP);
    } else {
      const int cfirst = big ? (NodeSrc::kLeafHoldsCluster ? lf.start : S.leaf_cl[R.cur].x) : 0;
      K = cull_one_level<HYBRID, COUNT>(S, clusters, R, fastAABB, cfirst, ncl, K, W, WP);
    }
    if (big) F = K;
  }
  if (COUNT) prof_lap(WP, PROF_BIG_CYC);
  const int sz = (at.leaf && !big) ? lf.size : 0;
  if (__any(sz > 0)) small_leaves<HYBRID, COUNT>(S, lf.start, sz, F, W, WP);
  if (COUNT) prof_lap(WP, PROF_SMALL_CYC);
  if (at.leaf) leaf_commit<HYBRID, COUNT, NodeSrc>(S, R, lf, F, at.lfirst, material_size, cnt);
  if (COUNT) prof_lap(WP, PROF_FINAL_CYC);
}

}  // namespace kdpt
