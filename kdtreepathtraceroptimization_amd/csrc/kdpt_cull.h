// kdpt_cull.h -- the cluster cull's predicates as __host__ __device__ functions: cluster sizes, half floats,
// the box / slab / oriented-box tests with their margins, kd_rcp, the direction buckets and the masked cull's
// per-triangle decision.
#pragma once

#include "kdpt_math.h"

namespace kdpt {

// ---------------------------------------------------------------------------
// Big leaves (>= BIG_LEAF triangles) are swept in clusters of 64; the C5 route groups SUPER clusters under
// one half-precision box.  The cluster cull below is host-compilable so that tests/native/cull_diff.cpp
// can check it against tri_test_v on adversarial lines ("Cluster cull").
// ---------------------------------------------------------------------------
constexpr int CLUSTER = 64;  // triangles per cluster: one per lane of the wave that sweeps it
static_assert(CLUSTER == 64, "cluster size: the sweep, the danger masks and the padding are one wave wide");
constexpr int SUPER = 1024 / CLUSTER;  // clusters per super-cluster (a power of two <= 32)
#ifndef KDPT_BIG_LEAF
#define KDPT_BIG_LEAF 48  // tools/build_variant.sh experiments only
#endif
constexpr int BIG_LEAF = KDPT_BIG_LEAF;  // leaves this size or larger are tested cluster by cluster

// IEEE half bits -> float (exact).  The device converts in one instruction; g++ 11 has no _Float16.
KDPT_HD float half_to_float(uint32_t h) {
#if defined(__clang__)
  return (float)__builtin_bit_cast(_Float16, (unsigned short)(h & 0xffffu));
#else
  const uint32_t s = (h & 0x8000u) << 16, e = (h >> 10) & 0x1fu, m = h & 0x3ffu;
  uint32_t b;
  if (e == 0x1fu) b = s | 0x7f800000u | (m << 13);
  else if (e) b = s | ((e + 112u) << 23) | (m << 13);
  else if (!m) b = s;
  else {  // subnormal half: m x 2^-24, exact in float
    const float v = (float)m * 5.9604644775390625e-8f;
    return s ? -v : v;
  }
  float f;
  memcpy(&f, &b, 4);
  return f;
#endif
}
KDPT_HD float half_lo(uint32_t w) { return half_to_float(w & 0xffffu); }
KDPT_HD float half_hi(uint32_t w) { return half_to_float(w >> 16); }

// May the LINE through o (both directions: glm's u/v tests ignore the sign of t) cross the cluster's
// triangles?  The box is widened by 1e-4 x (distance + size), orders of magnitude above the rounding
// of the Moller-Trumbore u/v tests, so a culled cluster holds no triangle that would pass them.
KDPT_HD bool cluster_may_pass(float4 lo, float4 hi, f3 o, f3 inv, float K) {
  const float cx = 0.5f * (lo.x + hi.x), cy = 0.5f * (lo.y + hi.y), cz = 0.5f * (lo.z + hi.z);
  const float m = K * (1.0f + fabsf(o.x - cx) + fabsf(o.y - cy) + fabsf(o.z - cz) + (hi.x - lo.x) +
                           (hi.y - lo.y) + (hi.z - lo.z));
  const float t1x = (lo.x - m - o.x) * inv.x, t2x = (hi.x + m - o.x) * inv.x;
  const float t1y = (lo.y - m - o.y) * inv.y, t2y = (hi.y + m - o.y) * inv.y;
  const float t1z = (lo.z - m - o.z) * inv.z, t2z = (hi.z + m - o.z) * inv.z;
  const float tmin = fmaxf(fmaxf(fminf(t1x, t2x), fminf(t1y, t2y)), fminf(t1z, t2z));
  const float tmax = fminf(fminf(fmaxf(t1x, t2x), fmaxf(t1y, t2y)), fmaxf(t1z, t2z));
  return tmin <= tmax;
}

// The brute-force route's chunk decision (kernels_brute.h k_brute; tests/native/brute_diff.cpp runs the same):
// may the line through o cross a triangle of file-order chunk j?  The box is chunk_lo[j] / chunk_hi[j], the
// coefficient the chunk's own rigorous one, chunk_lo[j].w (kdpt_clusters.h build_chunk_boxes: no triangle of a
// culled chunk passes glm's u/v tests, for any line; +inf, never culled, for a chunk whose coefficient could cull
// nothing) -- or `fixed` when that is > 0: the one coefficient of the tuning knobs "cull_margin" (not exact) and
// "cluster_cull" = 0 (+inf).
KDPT_HD bool brute_chunk_may_pass(const float4* chunk_lo, const float4* chunk_hi, int j, f3 o, f3 inv, float fixed) {
  const float4 lo = chunk_lo[j];
  return cluster_may_pass(lo, chunk_hi[j], o, inv, fixed > 0.0f ? fixed : lo.w);
}

// The brute-force route's per-shape bbox test: intersectBbox (src/interactions.h:136-165), std::min/max as in
// intersectAABBarrays
KDPT_HD float intersectBbox(f3 o, f3 d, float4 lo, float4 hi) {
  const f3 invdir = mk3(1.0f / d.x, 1.0f / d.y, 1.0f / d.z);
  const float v1 = (lo.x - o.x) * invdir.x, v2 = (hi.x - o.x) * invdir.x;
  const float v3 = (lo.y - o.y) * invdir.y, v4 = (hi.y - o.y) * invdir.y;
  const float v5 = (lo.z - o.z) * invdir.z, v6 = (hi.z - o.z) * invdir.z;
  const float dmin = std_max(std_max(std_min(v1, v2), std_min(v3, v4)), std_min(v5, v6));
  const float dmax = std_min(std_min(std_max(v1, v2), std_max(v3, v4)), std_max(v5, v6));
  if (dmax < 0) return dmax;
  if (dmin > dmax) return dmax;
  return dmin;
}

// Is glm::intersectRayTriangle certain to return false?  a, u, v, w are the reference's exact values;
// f = RN(1/a) > 0 (a >= eps).  bx = RN(f*u) < 0 for u < -a*2^-100 (|f*u| >= 2^-101, far from rounding
// to -0); bx > 1 for u > RN(a*(1+2^-20)) (then u/a > 1 + 2^-21 and two roundings cannot bring it to 1);
// likewise by, the sum (u + v > a*(1+2^-18) with u, v >= 0) and bz = RN(f*w) < 0.
KDPT_HD bool tri_certain_miss(float a, float u, float v, float w) {
  const float tiny = a * 0x1p-100f;
  const float one_u = a * 1.00000095367431640625f;  // a * (1 + 2^-20)
  const float one_s = a * 1.000003814697265625f;    // a * (1 + 2^-18)
  return !(a >= FLT_EPS) || u < -tiny || u > one_u || v < -tiny || w < -tiny ||
         (u >= 0.0f && v >= 0.0f && u + v > one_s);
}

// The margin coefficient of the slab level for a line of direction d and a cluster of normal n (n.w = the
// largest chord |N_t / |N_t| - n| over the cluster's triangles): glm's determinant of every triangle t of the
// cluster is then at least |N_t| (|n . d| - n.w - cull_b), which bounds the float u/v error and so the margin a
// u/v pass can need ("Cluster cull"); min with the direction-free rigorous cl_margin, max with
// the fast floor cl_margin_lo.  A line nearly parallel to the cluster's patch gets the direction-free one.
struct CullK {
  float hi, lo, a, b, c;  // DevScene::cl_margin, cl_margin_lo, cull_a, cull_b, cull_c
};
KDPT_HD float cull_margin_dir(float nd, float spread, const CullK& k) {
  const float g = fabsf(nd) - spread - k.b;
  const float kd = g > 0.0f ? k.a / g + k.c : k.hi;
  return fmaxf(k.lo, fminf(k.hi, kd));
}

// cluster_may_pass and the cluster's slab {q : n . (q - c) in [lo.w, hi.w]}: the line's parameter interval
// through the slab, widened by the same margin, must meet its interval through the box.  A triangle the line
// crosses has its crossing point in both (a convex combination of its vertices), so the cull stays
// conservative; a line (nearly) parallel to the slab passes it.  A curved-surface patch is thin along its
// normal, so a line that only grazes the patch's box is culled.
KDPT_HD bool cluster_may_pass_slab(float4 lo, float4 hi, float4 n, f3 o, f3 inv, f3 d, const CullK& k) {
  const float nd = n.x * d.x + n.y * d.y + n.z * d.z;
  const float K = cull_margin_dir(nd, n.w, k);
  const float cx = 0.5f * (lo.x + hi.x), cy = 0.5f * (lo.y + hi.y), cz = 0.5f * (lo.z + hi.z);
  const float m = K * (1.0f + fabsf(o.x - cx) + fabsf(o.y - cy) + fabsf(o.z - cz) + (hi.x - lo.x) +
                           (hi.y - lo.y) + (hi.z - lo.z));
  const float t1x = (lo.x - m - o.x) * inv.x, t2x = (hi.x + m - o.x) * inv.x;
  const float t1y = (lo.y - m - o.y) * inv.y, t2y = (hi.y + m - o.y) * inv.y;
  const float t1z = (lo.z - m - o.z) * inv.z, t2z = (hi.z + m - o.z) * inv.z;
  float tmin = fmaxf(fmaxf(fminf(t1x, t2x), fminf(t1y, t2y)), fminf(t1z, t2z));
  float tmax = fminf(fminf(fmaxf(t1x, t2x), fmaxf(t1y, t2y)), fmaxf(t1z, t2z));
  const float no = n.x * (o.x - cx) + n.y * (o.y - cy) + n.z * (o.z - cz);
  if (fabsf(nd) > 1e-12f) {
    const float rn = 1.0f / nd;
    const float s1 = (lo.w - m - no) * rn, s2 = (hi.w + m - no) * rn;
    tmin = fmaxf(tmin, fminf(s1, s2));
    tmax = fminf(tmax, fmaxf(s1, s2));
  }
  return tmin <= tmax;
}

// cluster_may_pass_slab and the patch's u and v slabs: the line's interval through the cluster's oriented box
// (n, u, v) must meet its interval through the axis-aligned one, every slab widened by the same margin.  A
// point the float u/v tests accept lies within the margin of the line and inside every one of them, so the
// cull stays as conservative as the box alone.
KDPT_HD void slab_clip(float lo, float hi, float m, float sd, float so, float& tmin, float& tmax) {
  if (fabsf(sd) > 1e-12f) {
    const float rs = 1.0f / sd;
    const float s1 = (lo - m - so) * rs, s2 = (hi + m - so) * rs;
    tmin = fmaxf(tmin, fminf(s1, s2));
    tmax = fminf(tmax, fmaxf(s1, s2));
  }
}
KDPT_HD bool cluster_may_pass_obb_k(float4 lo, float4 hi, float4 n, float4 u, float4 v, float4 w, f3 o, f3 inv, f3 d,
                                    float nd, float K) {
  const float cx = 0.5f * (lo.x + hi.x), cy = 0.5f * (lo.y + hi.y), cz = 0.5f * (lo.z + hi.z);
  const float m = K * (1.0f + fabsf(o.x - cx) + fabsf(o.y - cy) + fabsf(o.z - cz) + (hi.x - lo.x) +
                           (hi.y - lo.y) + (hi.z - lo.z));
  const float t1x = (lo.x - m - o.x) * inv.x, t2x = (hi.x + m - o.x) * inv.x;
  const float t1y = (lo.y - m - o.y) * inv.y, t2y = (hi.y + m - o.y) * inv.y;
  const float t1z = (lo.z - m - o.z) * inv.z, t2z = (hi.z + m - o.z) * inv.z;
  float tmin = fmaxf(fmaxf(fminf(t1x, t2x), fminf(t1y, t2y)), fminf(t1z, t2z));
  float tmax = fminf(fminf(fmaxf(t1x, t2x), fmaxf(t1y, t2y)), fmaxf(t1z, t2z));
  const float ox = o.x - cx, oy = o.y - cy, oz = o.z - cz;
  slab_clip(lo.w, hi.w, m, nd, n.x * ox + n.y * oy + n.z * oz, tmin, tmax);
  slab_clip(u.w, w.x, m, u.x * d.x + u.y * d.y + u.z * d.z, u.x * ox + u.y * oy + u.z * oz, tmin, tmax);
  slab_clip(v.w, w.y, m, v.x * d.x + v.y * d.y + v.z * d.z, v.x * ox + v.y * oy + v.z * oz, tmin, tmax);
  return tmin <= tmax;
}
KDPT_HD bool cluster_may_pass_obb(float4 lo, float4 hi, float4 n, float4 u, float4 v, float4 w, f3 o, f3 inv, f3 d,
                                  const CullK& k) {
  const float nd = n.x * d.x + n.y * d.y + n.z * d.z;
  return cluster_may_pass_obb_k(lo, hi, n, u, v, w, o, inv, d, nd, cull_margin_dir(nd, n.w, k));
}

// Direction buckets of the exact one-level cull (kdpt_clusters.h build_dir_masks): a cube map of n x n cells
// per face.  The face is the largest |component| (ties: x before y before z), (u, v) the other two components
// over it, cell (floor((u + 1) n / 2), floor((v + 1) n / 2)) clamped to n - 1.  The host bounds each cell's
// directions (grown by 1e-5 in u and v, far above this function's rounding), so any float d maps to a cell
// whose bound holds it.  Any finite nonzero d works (the cull only runs for lanes whose 1 / d components are
// all finite).
// 1 / x for box_miss and dir_bucket: the hardware reciprocal (1 ulp) on the device, the division on the host;
// box_miss's 1e-5 slack and the masks' 1e-5 cell growth cover either.  A float within 1 ulp of 1 / x is the
// rounded quotient or one of its two neighbours: the cull harness (tests/native/cull_diff.cpp, KDPT_RCP_ULP)
// evaluates every line with each of the three.
#if !defined(__HIP_DEVICE_COMPILE__) && defined(KDPT_RCP_ULP)
extern thread_local int kdpt_rcp_ulp;  // -1, 0, +1: the host quotient moved by that many ulps
#endif
KDPT_HD float kd_rcp(float x) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_rcpf(x);
#elif defined(KDPT_RCP_ULP)
  const float r = 1.0f / x;
  return kdpt_rcp_ulp == 0 ? r : std::nextafter(r, kdpt_rcp_ulp > 0 ? HUGE_VALF : -HUGE_VALF);
#else
  return 1.0f / x;
#endif
}
KDPT_HD int dir_bucket(f3 d, int n) {
  const float ax = fabsf(d.x), ay = fabsf(d.y), az = fabsf(d.z);
  int face;
  float a, b, m;
  if (ax >= ay && ax >= az) {
    face = d.x > 0.0f ? 0 : 1;
    a = d.y;
    b = d.z;
    m = ax;
  } else if (ay >= az) {
    face = d.y > 0.0f ? 2 : 3;
    a = d.x;
    b = d.z;
    m = ay;
  } else {
    face = d.z > 0.0f ? 4 : 5;
    a = d.x;
    b = d.y;
    m = az;
  }
  const float h = 0.5f * (float)n * kd_rcp(m);
  int i = (int)((a + m) * h), j = (int)((b + m) * h);
  i = i < 0 ? 0 : (i > n - 1 ? n - 1 : i);
  j = j < 0 ? 0 : (j > n - 1 ? n - 1 : j);
  return (face * n + j) * n + i;
}

// How far the LINE through o (direction 1 / inv, every component finite) misses the box [lo, hi], in the units
// of cluster_may_pass's margin coefficient: the smallest K for which cluster_may_pass(lo, hi, o, inv, K) holds.
// With the margin m = K W (W = 1 + |o - c|_1 + size_1), each slab's parameter interval [a_i, b_i] grows by
// m |inv_i| at both ends, so the intervals meet once m >= (a_i - b_j) / (|inv_i| + |inv_j|) for every pair of
// axes.  The line's distance from the box is at least that m (an L-infinity distance), so a point the float u/v
// tests accept lies within K_t W of the line only if K_t >= the result.  Rounded down by 1e-5 relative; 0 when
// the line meets the box.
KDPT_HD float box_miss(float4 lo, float4 hi, f3 o, f3 inv) {
  const float cx = 0.5f * (lo.x + hi.x), cy = 0.5f * (lo.y + hi.y), cz = 0.5f * (lo.z + hi.z);
  const float W = 1.0f + fabsf(o.x - cx) + fabsf(o.y - cy) + fabsf(o.z - cz) + (hi.x - lo.x) + (hi.y - lo.y) +
                  (hi.z - lo.z);
  const float tlx = (lo.x - o.x) * inv.x, thx = (hi.x - o.x) * inv.x;
  const float tly = (lo.y - o.y) * inv.y, thy = (hi.y - o.y) * inv.y;
  const float tlz = (lo.z - o.z) * inv.z, thz = (hi.z - o.z) * inv.z;
  const float ax = fminf(tlx, thx), bx = fmaxf(tlx, thx), ay = fminf(tly, thy), by = fmaxf(tly, thy);
  const float az = fminf(tlz, thz), bz = fmaxf(tlz, thz);
  const float wx = fabsf(inv.x), wy = fabsf(inv.y), wz = fabsf(inv.z);
  const float mxy = fmaxf(ax - by, ay - bx) * kd_rcp(wx + wy);
  const float mxz = fmaxf(ax - bz, az - bx) * kd_rcp(wx + wz);
  const float myz = fmaxf(ay - bz, az - by) * kd_rcp(wy + wz);
  const float m = fmaxf(0.0f, fmaxf(mxy, fmaxf(mxz, myz)));
  return m * kd_rcp(W) * 0.99999f;
}

// The exact cull's per-triangle decision for a (line, cluster) pair whose line misses the cluster's box by D
// (box_miss): may triangle tn (its float unit normal, w = 17.5 u rho, the u/v error coefficient; w < 0: never
// passes; w = +inf: may pass for any line) pass glm's u/v tests?  Its float determinant is below -|N| (N . d -
// beta) with beta = 5.8 u rho (1 + 1e-3) + 40 u (+ the float normal's and nd's rounding), so it cannot pass when
// nd > beta (back-facing); otherwise a passing point lies within K_t = w / g + c (times the margin's distance
// term) of the line, g = -nd - beta ("Cluster cull"), which needs K_t >= D, i.e. w >= (D - c) g.
// g <= 0: no bound, the triangle is tested.
KDPT_HD bool danger_needs_test(float4 tn, f3 d, float D, float c) {
  if (!(tn.w >= 0.0f)) return false;
  const float nd = tn.x * d.x + tn.y * d.y + tn.z * d.z;
  const float beta = 0.3318f * tn.w + 3.5e-6f;
  if (nd > beta) return false;
  const float g = -nd - beta;
  return !(g > 0.0f) || tn.w * 1.00001f >= (D - c) * g;
}

// One (bucket, cluster) cell of the masked cull (kdpt_clusters.h build_dir_masks on the host and k_build_masks on
// the device run this same code, -ffp-contract=off, so both give the same bits).  Per entry k of the cluster: its
// unit normal n_k, beta_k and dthr_k (kdpt_clusters.h mask_entries) and its rigorous coefficient krig_k; the
// bucket: its centre direction D[0..2] and radius D[3].  Entry k is in the danger mask when some direction of the
// bucket makes it front-facing (n_k . d <= beta_k) and needing more than Kf (n_k . d >= dthr_k), and its own
// direction-free rigorous coefficient K_t = 8.75 |e1||e2| + c exceeds Kf (a line glm's float u/v tests accept for
// t passes within K_t W of any region holding t -- DESIGN.md 4, "Cluster cull" -- so a pair that missed the box
// or the oriented box at Kf >= K_t cannot need t).
KDPT_HD unsigned long long dir_mask_cell(const double* nx, const double* ny, const double* nz, const double* beta,
                                         const double* dthr, const float* krig, const double* D, float Kf) {
  unsigned long long md = 0ull;
  for (int k = 0; k < 64; k++) {
    const double x = nx[k] * D[0] + ny[k] * D[1] + nz[k] * D[2];
    if (x - D[3] <= beta[k] && x + D[3] >= dthr[k] && krig[k] > Kf) md |= 1ull << k;
  }
  return md;
}

}  // namespace kdpt
