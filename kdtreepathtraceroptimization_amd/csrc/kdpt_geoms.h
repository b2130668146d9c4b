// kdpt_geoms.h -- the analytic geoms of the reference as __host__ __device__ functions: what a ray may conclude
// from a geom's bounds, the exact box / sphere tests (src/intersections.h), the node-box test intersectAABB and
// prep_ray, the intersect stage's first part for one ray (src/pathtrace.cu:1600-1640).
#pragma once

#include "kdpt_scene.h"

namespace kdpt {

// The analytic geoms' bounds: what a ray may conclude from them, and when.
//
// boxIntersectionTest / sphereIntersectionTest work in object space, in float: they transform the origin by the
// float inverseTransform, intersect the unit cube / the sphere of radius 0.5 there, step back 1e-4 along the
// object-space direction, transform that point by `transform` and report t = |origin - point|.  The reported
// point is a point of the ray and of the object only up to rounding, and that rounding is not small everywhere:
//   (a) the object-space origin is formed from products of size |inverse| x |coordinate|, so it -- and through
//       `transform` the reported point -- is off by u x (the magnitude of the world coordinates involved),
//       u = 2^-24, whatever the size of the object: a geom translated far from the world origin, or a ray that
//       starts far away, is tested against an object displaced by that much;
//   (b) the float inverse is not the inverse of the float transform: E = inverse x transform - 1 (linear part)
//       and e = inverse x translation + inverse's translation displace the object by E q + e at object-space
//       distance q;
//   (c) the sphere test's radicand (ro.rd)^2 - (ro.ro - 0.25) cancels two terms of size D^2 (D the origin's
//       object-space distance): its rounding, <= 16 u (D + 1)^2 (6 u for the squared dot product, 3 u for ro.ro,
//       2 u for the two differences, 3 u for |rd|^2 - 1, rounded up), is a ray reported to hit a sphere of
//       radius^2 0.25 + that much -- at D = 1e4 a radius of up to 10 instead of 0.5 -- and a hit point up to the
//       square root of it before the true one along the ray (sqrt(u) x D x scale in world units);
//   (d) the 1e-4 step back, up to 1e-4 x the world extent;
//   (e) a direction cast without the normalize flag has |d|^2 = 1 +- 1e-6, so the parameter of a point exceeds
//       its distance by up to 5.1e-7 of it.
// So "the exact test hits only rays that enter the bounds, at a t no smaller than the entry parameter" holds
// only where the sum of these stays below the bounds' margin, 1e-3 x extent + 1e-3 (a sphere's, whose radicand
// needs the room and which fills only half of its bounds anyway: 1e-2 x extent + 1e-3).  prepare_geom
// (kdpt_scene_prep.h, geom_safe_range) evaluates that sum in double from the geom's own float matrices for
// origins within Chebyshev distance R of the bounds, and stores in wlo[3] the largest R (of a halving sequence)
// for which
//     4 x (a + b + c + e, mapped to world axes through |transform|, + 16 u x coordinates) + (d) <= margin;
// the factor: a point X within `a` of the ray's point at parameter s and within `b` of the true box puts that
// ray point inside the box enlarged by a + b, whose entry parameter exceeds the entry into the box enlarged by
// the margin m by at least m - a - b (each slab plane moves by that much, and |d_k| <= 1), while |o - X| >=
// s - sqrt(3) a: t >= entry needs m >= (1 + sqrt(3)) a + b.  R = -inf when not even R = 0 satisfies it (a geom
// whose translation is large against its size, matrices that are not each other's inverse).
//
// A ray whose origin lies farther than R from the bounds concludes nothing from them: geom_may_hit says true,
// and the geom is tested as the reference tests every geom.  prep_ray decides once per ray instead of once per
// geom: for an origin inside DevScene::gc +- gh, the intersection of the geoms' ranges (each its bounds grown
// by R; empty when some R is -inf) it runs as before -- the nearest-first loop, or the index-order loop with the
// skip test -- and for any other origin every geom is tested, in index order.  The fixture scenes keep
// R >= 24 around their 10-unit room, so their rays all stay on the nearest-first path.  tests/test_geom_diff.py
// compares the loops built on this with the reference's index-order loop on 400 000 rays per generator of
// tests/geoms.py, origins up to 3 000 units away and scenes at 1e5 included.

// The ray against the geom's enlarged bounds (invdir finite): false = it misses them.  For an origin within the
// geom's proven range (above) the exact test then misses as well.
KDPT_HD bool geom_bounds_hit(const DevGeom& G, f3 o, f3 invdir) {
  const float t1x = (G.wlo[0] - o.x) * invdir.x, t2x = (G.whi[0] - o.x) * invdir.x;
  const float t1y = (G.wlo[1] - o.y) * invdir.y, t2y = (G.whi[1] - o.y) * invdir.y;
  const float t1z = (G.wlo[2] - o.z) * invdir.z, t2z = (G.whi[2] - o.z) * invdir.z;
  const float tmin = fmaxf(fmaxf(fminf(t1x, t2x), fminf(t1y, t2y)), fminf(t1z, t2z));
  const float tmax = fminf(fminf(fmaxf(t1x, t2x), fmaxf(t1y, t2y)), fmaxf(t1z, t2z));
  return tmax >= tmin && tmax >= 0.0f;
}

// Conservative skip test for one analytic geom (invdir finite), for any origin: false only when the exact test
// would miss (k_brute, k_viz; prep_ray decides once per ray, geoms_hold_for).
KDPT_HD bool geom_may_hit(const DevGeom& G, f3 o, f3 invdir) {
  // the origin's Chebyshev distance from the bounds (negative inside) against the proven range
  const float away = fmaxf(fmaxf(fmaxf(G.wlo[0] - o.x, o.x - G.whi[0]), fmaxf(G.wlo[1] - o.y, o.y - G.whi[1])),
                           fmaxf(G.wlo[2] - o.z, o.z - G.whi[2]));
  return !(away <= G.wlo[3]) || geom_bounds_hit(G, o, invdir);
}

// Entry parameter of the ray into the geom's enlarged world bounds: a lower bound of the exact test's t
// whenever that test hits, for an origin within the geom's proven range (above; prep_ray asks
// geoms_hold_for).  false: the exact test would miss.
KDPT_HD bool geom_entry_bound(const DevGeom& G, f3 o, f3 invdir, float& lo) {
  const float t1x = (G.wlo[0] - o.x) * invdir.x, t2x = (G.whi[0] - o.x) * invdir.x;
  const float t1y = (G.wlo[1] - o.y) * invdir.y, t2y = (G.whi[1] - o.y) * invdir.y;
  const float t1z = (G.wlo[2] - o.z) * invdir.z, t2z = (G.whi[2] - o.z) * invdir.z;
  const float tmin = fmaxf(fmaxf(fminf(t1x, t2x), fminf(t1y, t2y)), fminf(t1z, t2z));
  const float tmax = fminf(fminf(fmaxf(t1x, t2x), fmaxf(t1y, t2y)), fmaxf(t1z, t2z));
  lo = tmin;
  return tmax >= tmin && tmax >= 0.0f;
}

KDPT_HD f3 getPointOnRay(const Ray& r, float t) {  // src/intersections.h:30-32
  return add(r.origin, scl(normalize(r.direction), t - .0001f));
}

// src/intersections.h:107-149
KDPT_HD float boxIntersectionTest(const DevGeom& box, const Ray& r, f3& ip, f3& nrm) {
  Ray q;
  q.origin = mulMV(box.inverseTransform, f4{r.origin.x, r.origin.y, r.origin.z, 1.0f});
  q.direction = normalize(mulMV(box.inverseTransform, f4{r.direction.x, r.direction.y, r.direction.z, 0.0f}));
  float tmin = -1e38f, tmax = 1e38f;
  int tmin_axis = -1, tmax_axis = -1;
  float tmin_s = 0.0f, tmax_s = 0.0f;
#pragma unroll
  for (int xyz = 0; xyz < 3; ++xyz) {
    float qd = comp(q.direction, xyz);
    float qo = comp(q.origin, xyz);
    float t1 = (-0.5f - qo) / qd;
    float t2 = (+0.5f - qo) / qd;
    float ta = glm_min(t1, t2);
    float tb = glm_max(t1, t2);
    float ns = t2 < t1 ? +1.0f : -1.0f;
    if (ta > 0 && ta > tmin) { tmin = ta; tmin_axis = xyz; tmin_s = ns; }
    if (tb < tmax) { tmax = tb; tmax_axis = xyz; tmax_s = ns; }
  }
  if (tmax >= tmin && tmax > 0) {
    if (tmin <= 0) { tmin = tmax; tmin_axis = tmax_axis; tmin_s = tmax_s; }
    f3 n = mk3(tmin_axis == 0 ? tmin_s : 0.0f, tmin_axis == 1 ? tmin_s : 0.0f, tmin_axis == 2 ? tmin_s : 0.0f);
    f3 p = getPointOnRay(q, tmin);
    ip = mulMV(box.transform, f4{p.x, p.y, p.z, 1.0f});
    nrm = normalize(mulMV(box.transform, f4{n.x, n.y, n.z, 0.0f}));
    return length(sub(r.origin, ip));
  }
  return -1;
}

// "boxIntersectionTest(box, {o, d}) returns -1", proven from that test's own first steps: true only when it
// does, false when this cannot tell (the exact test then decides as ever).
//
// qo is the exact test's q.origin: the same mulMV of the same operands, so the same bits.  Its q.direction is
// qu scaled by f = 1 / sqrtf(dot(qu, qu)) (glm's normalize).  With l2 = dot(qu, qu) finite and > 0, f is finite
// and > 0 (sqrtf(l2) lies in [2^-75, 2^64]; float denormals are kept on both targets), so qd_k = qu_k * f has
// the sign of qu_k: a product that underflows becomes a zero of that sign, one that overflows an infinity of
// that sign, and with qu_k != 0 and f > 0 it is never NaN.
// Take an axis k with qo_k > 0.5 and qu_k > 0.  Both numerators, -0.5 - qo_k and 0.5 - qo_k, are < 0 (the
// second because qo_k != 0.5 and a difference of two distinct floats of this size is not zero), and the divisor
// qd_k is +0, positive or +inf: t1 and t2 are each -inf, negative or -0, never NaN and never > 0.  So
// tb = glm_max(t1, t2) <= -0, `tb < tmax` holds against the initial 1e38 or tmax is already below it: after
// axis k tmax <= -0, the other axes can only lower it (a NaN tb fails `tb < tmax` and leaves it), and the
// final `tmax > 0` fails: -1.  The mirrored case, qo_k < -0.5 and qu_k < 0: both numerators > 0, the divisor
// -0, negative or -inf, the same quotients.
// The comparisons are strict, so a NaN coordinate, a numerator of 0 (qo_k = +-0.5) and a zero component of
// the direction all abstain, as does an l2 that is 0, infinite or NaN (f would be inf, 0 or NaN, and 0 * inf
// a NaN divisor).  Nothing here depends on the geom's bounds, so it holds for any origin.
KDPT_HD bool box_provably_missed(const DevGeom& box, f3 o, f3 d) {
  const f3 qo = mulMV(box.inverseTransform, f4{o.x, o.y, o.z, 1.0f});
  const f3 qu = mulMV(box.inverseTransform, f4{d.x, d.y, d.z, 0.0f});
  const float l2 = dot(qu, qu);
  const bool leaves = (qo.x > 0.5f && qu.x > 0.0f) || (qo.x < -0.5f && qu.x < 0.0f) ||
                      (qo.y > 0.5f && qu.y > 0.0f) || (qo.y < -0.5f && qu.y < 0.0f) ||
                      (qo.z > 0.5f && qu.z > 0.0f) || (qo.z < -0.5f && qu.z < 0.0f);
  return leaves && l2 > 0.0f && l2 < FLT_INFV;
}

// src/intersections.h:161-203
KDPT_HD float sphereIntersectionTest(const DevGeom& sphere, const Ray& r, f3& ip, f3& nrm) {
  float radius = .5f;
  f3 ro = mulMV(sphere.inverseTransform, f4{r.origin.x, r.origin.y, r.origin.z, 1.0f});
  f3 rd = normalize(mulMV(sphere.inverseTransform, f4{r.direction.x, r.direction.y, r.direction.z, 0.0f}));
  Ray rt;
  rt.origin = ro;
  rt.direction = rd;
  float vDotDirection = dot(rt.origin, rt.direction);
  float radicand = vDotDirection * vDotDirection - (dot(rt.origin, rt.origin) - radius * radius);
  if (radicand < 0) return -1;
  float squareRoot = sqrtf(radicand);
  float firstTerm = -vDotDirection;
  float t1 = firstTerm + squareRoot, t2 = firstTerm - squareRoot;
  float t = 0;
  bool outside;
  if (t1 < 0 && t2 < 0) return -1;
  else if (t1 > 0 && t2 > 0) { t = std_min(t1, t2); outside = true; }
  else { t = std_max(t1, t2); outside = false; }
  f3 os = getPointOnRay(rt, t);
  ip = mulMV(sphere.transform, f4{os.x, os.y, os.z, 1.f});
  nrm = normalize(mulMV(sphere.invTranspose, f4{os.x, os.y, os.z, 0.f}));
  if (!outside) nrm = neg(nrm);
  return length(sub(r.origin, ip));
}

// src/intersections.h:253-286 with invdir hoisted per ray (same values)
KDPT_HD bool intersectAABB(f3 o, f3 invdir, float4 b0, float4 b1, float& dist) {
  float v1 = (b0.x - o.x) * invdir.x;
  float v2 = (b0.w - o.x) * invdir.x;
  float v3 = (b0.y - o.y) * invdir.y;
  float v4 = (b1.x - o.y) * invdir.y;
  float v5 = (b0.z - o.z) * invdir.z;
  float v6 = (b1.y - o.z) * invdir.z;
  float dmin = std_max(std_max(std_min(v1, v2), std_min(v3, v4)), std_min(v5, v6));
  float dmax = std_min(std_min(std_max(v1, v2), std_max(v3, v4)), std_max(v5, v6));
  if (dmax < 0) { dist = dmax; return false; }
  if (dmin > dmax) { dist = dmax; return false; }
  dist = dmin;
  return true;
}

// The intersect stage's first part for one ray: the analytic geoms of pathTraceOneBounceKDbare (tested
// before the KD tree; src/pathtrace.cu:1600-1640) -> t_min / hit, and the traversal's first step, the
// KD root's box (same intersectAABB, same invdir): false = the traversal ends there.
KDPT_HD bool geoms_hold_for(const DevScene& S, f3 o) {
  return fmaxf(fmaxf(fabsf(o.x - S.gc.x) - S.gh.x, fabsf(o.y - S.gc.y) - S.gh.y), fabsf(o.z - S.gc.z) - S.gh.z) <= 0.0f;
}
constexpr int ORDERED_GEOMS = 8;  // scenes with at most this many analytic geoms test them nearest-first
// prep_ray's two test-only switches, both for the host harness tests/native/geom_pretest_diff.cpp and for A/B
// builds (tools/build_variant.sh); the product defines neither:
//   KDPT_PREP_EVENT(kind, geom)  what the nearest-first branch does to one geom: 0 an exact test, 1 the pre-test
//                                rules it out, 2 the pre-test abstains.  Empty here; the harness defines it to count.
//   KDPT_NO_GEOM_PRETEST         compiles the pre-pass out: the loop as it was before, for the efficacy ratio.
#ifndef KDPT_PREP_EVENT
#define KDPT_PREP_EVENT(kind, geom) ((void)0)
#endif
KDPT_HDI bool prep_ray(const DevScene& S, bool kd, f3 o, f3 d, float& t_min, int& hit) {
  Ray ray;
  ray.origin = o;
  ray.direction = d;
  ray.isinside = false;
  ray.sdepth = 0.0f;
  t_min = FLT_MAXV;
  hit = -1;
  f3 tmp_i = mk3(0, 0, 0), tmp_n = mk3(0, 0, 0);
  const f3 inv = mk3(1.0f / d.x, 1.0f / d.y, 1.0f / d.z);
  const bool finite = fabsf(inv.x) < FLT_INFV && fabsf(inv.y) < FLT_INFV && fabsf(inv.z) < FLT_INFV;
  const int ng = S.num_geoms;
  const bool held = geoms_hold_for(S, o);  // the geoms' bounds say something about this ray
  if (finite && ng <= ORDERED_GEOMS) {
    // Nearest-first: the reference keeps the first geom (index order) reaching the smallest t > 0; here
    // the geoms whose bounds the ray enters are tested in order of their entry bound, stopping once that
    // bound exceeds the best t, and ties go to the lower index -- the same winner and the same t, with
    // typically one or two exact tests per ray instead of one per geom the wave's rays come near.
    // An origin the bounds do not hold for enters every geom at -inf: all are tested, in index order.
    float lo[ORDERED_GEOMS];
    uint32_t pending = 0, inside = 0;
#pragma unroll
    for (int g = 0; g < ORDERED_GEOMS; g++) {
      lo[g] = FLT_INFV;
      if (g < ng) {
        const bool enters = geom_entry_bound(S.geoms[g], o, inv, lo[g]);
        if (!held) lo[g] = -FLT_INFV;
        if (enters || !held) pending |= 1u << g;
        if ((enters || !held) && lo[g] <= 0.0f) inside |= 1u << g;
      }
    }
#ifndef KDPT_NO_GEOM_PRETEST
    // The geoms whose enlarged bounds hold the origin (entry bound <= 0) come first in the loop below whatever
    // they are: after a bounce that is the box the path has just left, which the ray cannot hit, and the loop's
    // trip count is the wave's largest.  A box that box_provably_missed rules out is taken off the list here,
    // for a fraction of an exact test; the loop then starts at the geom the ray may really hit.  Removing a
    // geom whose exact test returns -1 changes neither the winner nor its t.  One step per lane, for the first
    // such geom, so that the pre-pass is straight-line code and adds no loop-carried state: at the room's edges
    // and corners, where two or three walls hold the origin, the others stay on the list as before (DESIGN
    // section 4 has the measurement).  A wave of rays that start outside every geom's bounds, the camera's,
    // skips the step.
    if (inside) {
      const int g = __builtin_ctz(inside);
      const DevGeom& G = S.geoms[g];
      const bool missed = G.type == 1 && box_provably_missed(G, o, d);
      KDPT_PREP_EVENT(missed ? 1 : 2, g);
      if (missed) pending &= ~(1u << g);
    }
#endif
    while (pending) {
      int gb = 0;
      float lb = FLT_INFV;
#pragma unroll
      for (int g = 0; g < ORDERED_GEOMS; g++)
        if (((pending >> g) & 1u) && lo[g] < lb) {
          lb = lo[g];
          gb = g;
        }
      if (lb > t_min) break;  // every remaining geom's exact t exceeds the best
      pending &= ~(1u << gb);
      const DevGeom& G = S.geoms[gb];
      KDPT_PREP_EVENT(0, gb);
      const float t = G.type == 1 ? boxIntersectionTest(G, ray, tmp_i, tmp_n)
                                  : sphereIntersectionTest(G, ray, tmp_i, tmp_n);
      if (t > 0.0f && (t < t_min || (t == t_min && gb < hit))) {
        t_min = t;
        hit = gb;
      }
    }
  } else {
    float t = 0;
    for (int g = 0; g < ng; g++) {
      const DevGeom& G = S.geoms[g];
      if (finite && held && !geom_bounds_hit(G, o, inv)) {
        t = -1.0f;  // the exact test would miss
      } else if (G.type == 1) {
        t = boxIntersectionTest(G, ray, tmp_i, tmp_n);
      } else if (G.type == 0) {
        t = sphereIntersectionTest(G, ray, tmp_i, tmp_n);
      }
      if (t > 0.0f && t_min > t) {
        t_min = t;
        hit = g;
      }
    }
  }
  if (!kd) return false;
  float dist;
  return intersectAABB(o, inv, make_float4(S.rlo.x, S.rlo.y, S.rlo.z, S.rhi.x),
                       make_float4(S.rhi.y, S.rhi.z, 0.0f, 0.0f), dist);
}

}  // namespace kdpt
