// kdpt_scene_prep.h -- everything kdpt_create does with a caller's kdpt_scene before it touches a device:
// whether the (untrusted) scene and options are accepted, and the conversion of the scene into the arrays and
// numbers the kernels read (DevScene, kdpt_scene.h).  Host code only: no HIP runtime header, no HIP call, no
// globals.  Included by kdpt_runtime.hip under hipcc, which only uploads what prepare_scene returns, and by the
// native test programs under g++ (tests/native/scene_prep_host.cpp runs it under ASan + UBSan;
// asan_host.cpp, traverse_diff.cpp and cull_diff.cpp take the product's wide node and triangle arrays from
// pack_wide_nodes / pack_triangles).  A header like kdpt_clusters.h, not an object file of its own: float4 and
// int4 are kdpt_math.h's structs under g++ and HIP's vector types under hipcc.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <string>
#include <utility>
#include <vector>

#include "../../include/kdpt.h"
#include "kdpt_device.h"
#include "kdpt_clusters.h"

namespace kdpt_host {
void node_box_matrices(const float* mins, const float* maxs, float* transform16, float* inverseTransform16);
}

namespace kdpt {

constexpr int TILE = 256;  // paths per workgroup (4 waves of 64): the only block_size
constexpr int MAX_KEYS = 64;  // materials (the keys of iteration 2's sort)
// Iterations per batch (kdpt_trace_iterations): they share one intersect launch and one ray queue of
// MAXB x npix int entries (kernels_gen.h TraceArgs).
#ifndef KDPT_MAXB
#define KDPT_MAXB 16  // tools/build_variant.sh experiments only
#endif
constexpr int MAXB = KDPT_MAXB;

// One OBJ shape of the brute-force route (BruteArgs::shapes).
struct BruteShape {
  float4 lo;  // bbox min (the reference's float(obj_polysbboxes[i + k] - 0.01)), w = index count bits
  float4 hi;  // bbox max (+ 0.01), w = obj_materialOffsets[i] bits
};

// The triangles as the kernels read them: v0 (w = mtlIdx bits on the tree route), e1 = v1 - v0, e2 = v2 - v0
// (exactly glm::intersectRayTriangle's e1 / e2 in float), and the three vertex normals.
struct TriArrays {
  std::vector<float4> tv0, te1, te2, tn0, tn1, tn2;
};

struct PreparedScene {
  kdpt_options opt{};  // the caller's (or the defaults) with bounce_cap 0 -> 8
  // which intersect route the scene takes: the KD tree, the brute force over the OBJ arrays (enable_kd = 0),
  // or the analytic geoms only; viz: the KD node boxes drawn as boxes (k_viz) instead of the tree walk
  bool kd = false, brute = false, viz = false;
  bool shade_oob = false;  // kdpt_ctx::shade_oob: a triangle of a shape other than the first
  std::vector<DevGeom> geoms;  // the analytic geoms, then (viz) one box per KD node with the last material
  int num_geoms = 0, num_boxes = 0;
  std::vector<DevMaterial> materials;
  int num_nodes = 0;  // DevScene::num_nodes
  std::vector<int4> nodes;   // 64-byte wide records; the three below are empty when the tree does not fit them
  std::vector<int4> pnodes;  // NodesPacked
  std::vector<int4> dnodes;  // NodesDerived
  std::vector<int4> snodes;  // ... with a big leaf's first super-cluster (only when num_supers > 0)
  TriArrays tri;             // tree order (kd) or file order (brute)
  std::vector<int> obj_material_offsets;  // kd: one per shape
  ClusterSet clusters;  // kd: the big leaves' clusters, Morton runs or normal cones (choose_clusters)
  CullMargin cull = cluster_margin({}, {}, {});  // of the route's triangles (none: the fast margin)
  bool wants_masks = false;  // no margin makes the cull exact: the masked one-level cull (build_masks)
  int num_supers = 0;        // 0 as well when a super box is not finite in half precision
  int cl_counts = 0;         // DevScene::cl_counts
  float4 rlo = make_float4(0, 0, 0, 0), rhi = make_float4(0, 0, 0, 0);  // the root's box
  float4 gc = make_float4(0, 0, 0, 0), gh = make_float4(0, 0, 0, 0);  // geoms_safe_region of the scene's geoms
  int n0_left = -1, n0_right = -1, n1_left = -1, n1_right = -1;
  std::vector<BruteShape> shapes;         // brute
  std::vector<float4> chunk_lo, chunk_hi;  // brute: boxes of 64 file-order triangles
};

inline void default_options(kdpt_options* o) {
  memset(o, 0, sizeof *o);
  o->focal_length = 6.0f;
  o->dof_angle = 0.0f;
  o->softness = 0.0f;
  o->cacherays = 0;
  o->antialias = 1;
  o->enable_sss = 0;
  o->testing_mode = 0;
  o->compaction = 1;
  o->enable_kd = 1;
  o->viz_kd = 0;
  o->use_bbox = 0;
  o->short_stack = 1;
  o->bounce_cap = 8;
  o->block_size = 0;
  o->external_image = nullptr;
}

// DevScene::nodes: one 64-byte record per node (one cache line per visit).
inline void pack_wide_nodes(const kdpt_node_bare* N, int nn, std::vector<int4>& out) {
  out.resize(4 * (size_t)nn);
  for (int i = 0; i < nn; i++) {
    const kdpt_node_bare& n = N[i];
    out[4 * (size_t)i + 0] = make_int4(fbits(n.mins[0]), fbits(n.mins[1]), fbits(n.mins[2]), fbits(n.maxs[0]));
    out[4 * (size_t)i + 1] = make_int4(fbits(n.maxs[1]), fbits(n.maxs[2]), n.leftID, n.rightID);
    out[4 * (size_t)i + 2] = make_int4(n.parentID, n.triIdStart, n.triIdSize, n.axis);
    out[4 * (size_t)i + 3] = make_int4(0, 0, 0, 0);
  }
}

// The tree's triangles (DevScene::tv0 ... tn2).
inline void pack_triangles(const kdpt_tri_bare* T, int nt, TriArrays& out) {
  for (std::vector<float4>* v : {&out.tv0, &out.te1, &out.te2, &out.tn0, &out.tn1, &out.tn2}) v->resize((size_t)nt);
  for (int i = 0; i < nt; i++) {
    const kdpt_tri_bare& t = T[i];
    // glm::intersectRayTriangle's e1 = v1 - v0, e2 = v2 - v0 in float: same bits here
    out.tv0[i] = make_float4(t.x1, t.y1, t.z1, ibits(t.mtlIdx));
    out.te1[i] = make_float4(t.x2 - t.x1, t.y2 - t.y1, t.z2 - t.z1, 0.0f);
    out.te2[i] = make_float4(t.x3 - t.x1, t.y3 - t.y1, t.z3 - t.z1, 0.0f);
    out.tn0[i] = make_float4(t.nx1, t.ny1, t.nz1, 0.0f);
    out.tn1[i] = make_float4(t.nx2, t.ny2, t.nz2, 0.0f);
    out.tn2[i] = make_float4(t.nx3, t.ny3, t.nz3, 0.0f);
  }
}

// NodesPacked records (kdpt_trace_phase.h); false when the tree does not fit the format.
inline bool pack_nodes(const kdpt_node_bare* N, int nn, const std::vector<int2>& leaf_cl, std::vector<int4>& out) {
  if (nn >= 0xffff) return false;
  out.assign(2 * (size_t)nn, make_int4(0, 0, 0, 0));
  auto l16 = [](int v) { return v == -1 ? 0xffffu : (uint32_t)v; };
  for (int i = 0; i < nn; i++) {
    const kdpt_node_bare& n = N[i];
    const bool tris = n.triIdSize > 0;
    if (tris && (n.leftID != -1 || n.rightID != -1 || n.triIdSize >= (1 << 13))) return false;
    const uint32_t axis = n.axis == 0 ? 0u : (n.axis == 1 ? 1u : 2u);  // comp(): anything else reads z
    // a big leaf keeps its first cluster instead of its first triangle (its clusters carry the triangles)
    const uint32_t first = n.triIdSize >= BIG_LEAF ? (uint32_t)leaf_cl[i].x : (uint32_t)n.triIdStart;
    const uint32_t w6 = tris ? first : (l16(n.leftID) | (l16(n.rightID) << 16));
    const uint32_t kids = (n.leftID != -1 ? 1u : 0u) | (n.rightID != -1 ? 2u : 0u);
    const uint32_t w7 = l16(n.parentID) | (axis << 16) | ((tris ? 1u : 0u) << 18) |
                        ((tris ? (uint32_t)n.triIdSize : kids) << 19);
    out[2 * i] = make_int4(fbits(n.mins[0]), fbits(n.mins[1]), fbits(n.mins[2]), fbits(n.maxs[0]));
    out[2 * i + 1] = make_int4(fbits(n.maxs[1]), fbits(n.maxs[2]), (int)w6, (int)w7);
  }
  return true;
}

// NodesDerived records (kdpt_trace_phase.h); false unless every node's box is its parent's with exactly the one
// coordinate the reference's split replaces (checked bit for bit), both children write the same centre, and
// the tree fits the 16-bit links.
inline bool pack_nodes16(const kdpt_node_bare* N, int nn, const std::vector<int2>& leaf_cl, std::vector<int4>& out) {
  if (nn < 1 || nn >= 0xffff || N[0].parentID != -1) return false;
  out.assign((size_t)nn, make_int4(0, 0, 0, 0));
  auto l16 = [](int v) { return v == -1 ? 0xffffu : (uint32_t)v; };
  auto same = [](float a, float b) { return fbits(a) == fbits(b); };
  for (int i = 0; i < nn; i++) {
    const kdpt_node_bare& n = N[i];
    const bool tris = n.triIdSize > 0;
    if (tris && (n.leftID != -1 || n.rightID != -1)) return false;
    if (n.axis < 0 || n.axis > 2) return false;
    for (int ch : {n.leftID, n.rightID})
      if (ch != -1 && (ch <= 0 || ch >= nn || N[ch].parentID != i)) return false;
    uint32_t kc = 7u;
    float restore = 0.0f;
    if (i > 0) {
      const int p = n.parentID;
      if (p < 0 || p >= nn) return false;
      const kdpt_node_bare& P = N[p];
      const bool isL = P.leftID == i, isR = P.rightID == i;
      if (isL == isR) return false;
      const int a = P.axis;
      for (int k = 0; k < 3; k++) {
        if (!(k == a && isR) && !same(n.mins[k], P.mins[k])) return false;
        if (!(k == a && isL) && !same(n.maxs[k], P.maxs[k])) return false;
      }
      kc = isR ? (uint32_t)a : 3u + (uint32_t)a;
      restore = isR ? P.mins[a] : P.maxs[a];
    }
    float center = 0.0f;
    if (n.leftID != -1) center = N[n.leftID].maxs[n.axis];
    if (n.rightID != -1) {
      if (n.leftID != -1 && !same(center, N[n.rightID].mins[n.axis])) return false;
      center = N[n.rightID].mins[n.axis];
    }
    const uint32_t first = n.triIdSize >= BIG_LEAF ? (uint32_t)leaf_cl[i].x : (uint32_t)n.triIdStart;
    const uint32_t w1 = tris ? first : fbits(center);
    const uint32_t w2 = tris ? (uint32_t)n.triIdSize : (l16(n.leftID) | (l16(n.rightID) << 16));
    const uint32_t kids = (n.leftID != -1 ? 1u : 0u) | (n.rightID != -1 ? 2u : 0u);
    const uint32_t w3 = l16(n.parentID) | ((uint32_t)n.axis << 16) | ((tris ? 1u : 0u) << 18) |
                        ((tris ? 0u : kids) << 19) | (kc << 21);
    out[i] = make_int4(fbits(restore), (int)w1, (int)w2, (int)w3);
  }
  return true;
}

// Big leaves as clusters of <= 64 triangles, super-clusters and slabs (kdpt_clusters.h).
// Meshes of small triangles (a rigorous margin: the two-level cull of the C5 icosphere) group each big leaf's
// triangles into normal cones of chord CLUSTER_CHORD_EXACT first, then Morton runs per cone: flatter clusters
// whose oriented boxes the lines miss more often -- C5's sweeps per ray 1.83 -> 1.30 (host simulation), C5
// 4 568 / 4 377 -> 5 110 / 5 087 Mrays/s (profiles/r06_ab_log.md).  Only the order of a leaf's sweeps changes
// (the results fold order-free); such leaves hold more clusters than ceil(size / 64) (DevScene::cl_counts).  Not
// for meshes of large triangles: dragon_5's leaves split into 4-8x as many clusters.  Kept only while the
// super-clusters grow by at most 40 % (they must fit the LDS route); cluster_chord (knob "cluster_chord", the
// process default): < 0 = this rule, 0 = Morton runs only, > 0 = that chord for every mesh.
inline void choose_clusters(const kdpt_node_bare* nodes, int nn, const kdpt_tri_bare* tris, const TriArrays& t,
                            double cluster_chord, ClusterSet& cs) {
  build_cluster_set(nodes, nn, tris, t.tv0, t.te1, t.te2, cs);
  const double chord = cluster_chord >= 0 ? cluster_chord
                                          : (cluster_margin(cs.cv0, cs.ce1, cs.ce2).exact ? CLUSTER_CHORD_EXACT : 0.0);
  if (chord > 0 && !cs.info.empty()) {
    ClusterGrouping g;
    g.mode = 1;
    g.chord = chord;
    ClusterSet cones;
    build_cluster_set(nodes, nn, tris, t.tv0, t.te1, t.te2, cones, g);
    if (cluster_chord > 0 || cones.sup.size() * 10 <= cs.sup.size() * 14) cs = std::move(cones);
  }
}

// The Chebyshev distance from a geom's enlarged bounds within which a ray origin may rely on them: the largest R
// of a halving sequence for which the exact test's error, bounded as kdpt_geoms.h derives it ("The analytic
// geoms' bounds"), fits the margin; -inf when none does.  m, mi: transform and inverseTransform (column-major);
// lo, hi: the exact world bounds.
inline float geom_safe_range(int type, const float* m, const float* mi, const double* lo, const double* hi,
                             double margin) {
  const double u = 5.9604644775390625e-8;  // 2^-24
  const double inf = std::numeric_limits<double>::infinity();
  for (int k = 0; k < 16; k++)
    if (!std::isfinite(m[k]) || !std::isfinite(mi[k])) return (float)-inf;
  // (the exact tests read the first three rows of either matrix only: mulMV)
  double A[3][3], Ai[3][3], E[3][3], e[3], gi[3], ext = 0, cmax = 0, fro = 0, emax = 0;
  for (int r = 0; r < 3; r++)
    for (int j = 0; j < 3; j++) {
      A[r][j] = m[4 * j + r];
      Ai[r][j] = mi[4 * j + r];
    }
  for (int r = 0; r < 3; r++) {
    gi[r] = std::fabs(Ai[r][0]) + std::fabs(Ai[r][1]) + std::fabs(Ai[r][2]);
    fro += Ai[r][0] * Ai[r][0] + Ai[r][1] * Ai[r][1] + Ai[r][2] * Ai[r][2];
    e[r] = Ai[r][0] * m[12] + Ai[r][1] * m[13] + Ai[r][2] * m[14] + mi[12 + r];
    for (int j = 0; j < 3; j++)
      E[r][j] = Ai[r][0] * A[0][j] + Ai[r][1] * A[1][j] + Ai[r][2] * A[2][j] - (r == j ? 1.0 : 0.0);
    ext = std::max(ext, hi[r] - lo[r]);
    cmax = std::max(cmax, std::max(std::fabs(lo[r]), std::fabs(hi[r])) + margin);
    emax = std::max(emax, std::fabs(e[r]));
  }
  fro = std::sqrt(fro);
  auto fits = [&](double R) {
    const double reach = R + margin + ext;  // of the origin from any point of the object, per axis
    const double W = cmax + R;              // magnitude of every world coordinate involved
    const double Dw = 2.0 * reach;          // >= sqrt(3) reach: the world distance from the origin to the hit
    double Dq[3];
    for (int j = 0; j < 3; j++) Dq[j] = gi[j] * reach + std::fabs(e[j]) + 1.0;  // object-space coordinates up to the hit
    // (c): the origin's object-space distance, |inverse (o - centre)| <= |inverse|_F sqrt(3) (R + margin + ext / 2);
    // radius^2 grows by at most 16 u (D + 1)^2 (kdpt_geoms.h), the radius 0.5 by no more than that
    const double D2 = 1.7320508075688772 * (fro * (R + margin + 0.5 * ext) + emax) + 1.0;
    const double radicand = type == 0 ? 16.0 * u * D2 * D2 : 0.0;
    double dq[3];
    for (int j = 0; j < 3; j++)
      dq[j] = 8.0 * u * (gi[j] * (W + Dw) + std::fabs((double)mi[12 + j]) + Dq[j])                     // (a)
              + std::fabs(E[j][0]) * Dq[0] + std::fabs(E[j][1]) * Dq[1] + std::fabs(E[j][2]) * Dq[2]  // (b)
              + std::fabs(e[j]) + radicand;
    double err = 0;
    for (int r = 0; r < 3; r++)
      err = std::max(err, std::fabs(A[r][0]) * dq[0] + std::fabs(A[r][1]) * dq[1] + std::fabs(A[r][2]) * dq[2]);
    err += 16.0 * u * W + 5.1e-7 * Dw;  // the point through `transform`, t = |o - point|, the entry parameter; (e)
    return 4.0 * err + 1.0001e-4 * ext <= margin;  // (d)
  };
  if (!(margin > 0) || !fits(0.0)) return (float)-inf;
  double R = 1024.0 * (ext + 1.0);
  while (!fits(R) && R > 1e-30) R *= 0.5;
  return fits(R) ? (float)R : 0.0f;
}

// DevGeom of a kdpt_geom: its matrices and the world bounds of the transformed unit cube (which contains the
// transformed unit sphere), + margin, and the range of ray origins the bounds hold for.
inline DevGeom prepare_geom(const kdpt_geom& g) {
  DevGeom d{};
  d.type = g.type;
  d.materialid = g.materialid;
  memcpy(d.transform, g.transform, 64);
  memcpy(d.inverseTransform, g.inverseTransform, 64);
  memcpy(d.invTranspose, g.invTranspose, 64);
  const float* m = g.transform;  // column-major
  double lo[3] = {1e300, 1e300, 1e300}, hi[3] = {-1e300, -1e300, -1e300};
  for (int k = 0; k < 8; k++) {
    const double v[3] = {(k & 1) ? 0.5 : -0.5, (k & 2) ? 0.5 : -0.5, (k & 4) ? 0.5 : -0.5};
    for (int r = 0; r < 3; r++) {
      const double w = (double)m[r] * v[0] + (double)m[4 + r] * v[1] + (double)m[8 + r] * v[2] + (double)m[12 + r];
      lo[r] = std::min(lo[r], w);
      hi[r] = std::max(hi[r], w);
    }
  }
  const double ext = std::max(std::max(hi[0] - lo[0], hi[1] - lo[1]), hi[2] - lo[2]);
  // (a sphere fills half of these bounds; its wider margin buys the range the sphere test's radicand needs)
  const double margin = (g.type == 0 ? 1e-2 : 1e-3) * ext + 1e-3;
  for (int r = 0; r < 3; r++) {
    d.wlo[r] = (float)(lo[r] - margin);
    d.whi[r] = (float)(hi[r] + margin);
  }
  d.wlo[3] = geom_safe_range(g.type, g.transform, g.inverseTransform, lo, hi, margin);
  d.whi[3] = 0.0f;
  return d;
}

// The ray origins for which the bounds of all n geoms hold: the intersection of their bounds grown by their
// ranges (wlo[3]), as centre and half-sizes (shrunk by more than their and the test's rounding); a negative
// half-size when there is none.
inline void geoms_safe_region(const DevGeom* g, int n, float4& centre, float4& half) {
  const double inf = std::numeric_limits<double>::infinity();
  float c[3], h[3];
  for (int r = 0; r < 3; r++) {
    double l = -1e30, u = 1e30;  // (no geoms: every finite origin)
    for (int i = 0; i < n; i++) {
      l = std::max(l, (double)g[i].wlo[r] - (double)g[i].wlo[3]);
      u = std::min(u, (double)g[i].whi[r] + (double)g[i].wlo[3]);
    }
    const bool none = !(l <= u) || l == inf || u == -inf;
    c[r] = none ? 0.0f : (float)(0.5 * (l + u));
    // |o - c| - h in float is off by a few 2^-24 of |o| + |c| + h, and |o| <= |c| + h where it matters
    const double hh = 0.5 * (u - l) - 1e-6 * (std::fabs(0.5 * (l + u)) + 0.5 * (u - l));
    h[r] = none || !(hh >= 0) ? -1.0f : (float)hh;
  }
  centre = make_float4(c[0], c[1], c[2], 0.0f);
  half = make_float4(h[0], h[1], h[2], 0.0f);
}

inline DevMaterial prepare_material(const kdpt_material& m) {
  DevMaterial d{};
  memcpy(d.color, m.color, 12);
  d.spec_exponent = m.specular_exponent;
  memcpy(d.spec_color, m.specular_color, 12);
  d.hasReflective = m.hasReflective;
  d.hasRefractive = m.hasRefractive;
  d.indexOfRefraction = m.indexOfRefraction;
  d.emittance = m.emittance;
  memcpy(d.transmittance, m.transmittance, 12);
  // glm::pow((1.0f - ior) / (1.0f + ior), 2.0f): powf(x, 2) folds to x * x
  const float rr = (1.0f - m.indexOfRefraction) / (1.0f + m.indexOfRefraction);
  d.fresnel_R0 = rr * rr;
  return d;
}

// The brute-force route's triangles: pathTraceOneBounce's file-order OBJ triangles (vertex / normal gathers done
// here once; the values are the ones the reference's kernel gathers per test), their chunk boxes and the shapes.
inline void prepare_brute(const kdpt_scene* sc, bool use_bbox, PreparedScene& p) {
  const int nt = sc->polyidxcount / 3;
  TriArrays& t = p.tri;
  for (std::vector<float4>* v : {&t.tv0, &t.te1, &t.te2, &t.tn0, &t.tn1, &t.tn2}) v->resize((size_t)nt);
  for (int k = 0; k < nt; k++) {
    const int* ix = sc->obj_polysidxflat + 3 * (size_t)k;
    const float* a = sc->obj_verts + 3 * (size_t)ix[0];
    const float* b = sc->obj_verts + 3 * (size_t)ix[1];
    const float* c = sc->obj_verts + 3 * (size_t)ix[2];
    t.tv0[k] = make_float4(a[0], a[1], a[2], 0.0f);
    t.te1[k] = make_float4(b[0] - a[0], b[1] - a[1], b[2] - a[2], 0.0f);
    t.te2[k] = make_float4(c[0] - a[0], c[1] - a[1], c[2] - a[2], 0.0f);
    const float* na = sc->obj_norms + 3 * (size_t)ix[0];
    const float* nb = sc->obj_norms + 3 * (size_t)ix[1];
    const float* nc = sc->obj_norms + 3 * (size_t)ix[2];
    t.tn0[k] = make_float4(na[0], na[1], na[2], 0.0f);
    t.tn1[k] = make_float4(nb[0], nb[1], nb[2], 0.0f);
    t.tn2[k] = make_float4(nc[0], nc[1], nc[2], 0.0f);
  }
  build_chunk_boxes(t.tv0, t.te1, t.te2, nt, p.chunk_lo, p.chunk_hi);
  p.cull = cluster_margin(t.tv0, t.te1, t.te2);
  p.shapes.resize((size_t)sc->num_shapes);
  for (int i = 0; i < sc->num_shapes; i++) {
    // glm::vec3(obj_polysbboxes[i] - 0.01, ...): double arithmetic, rounded to float by the constructor
    const float* bb = sc->obj_bboxes;
    float l[3] = {0, 0, 0}, h[3] = {0, 0, 0};
    if (use_bbox)
      for (int k = 0; k < 3; k++) {
        l[k] = (float)((double)bb[i + k] - 0.01);
        h[k] = (float)((double)bb[i + 3 + k] + 0.01);
      }
    p.shapes[i].lo = make_float4(l[0], l[1], l[2], ibits(sc->obj_polyoffsets[i]));
    p.shapes[i].hi = make_float4(h[0], h[1], h[2], ibits(sc->obj_materialOffsets[i]));
  }
}

// The tree route: the wide records and triangles, the clusters, and the narrower record formats the tree fits
// (which decide where setup_trace may put the tree).
inline void prepare_tree(const kdpt_scene* sc, double cluster_chord, PreparedScene& p) {
  const kdpt_node_bare* N = sc->nodes;
  const int nn = sc->num_nodes;
  pack_wide_nodes(N, nn, p.nodes);
  pack_triangles(sc->tris, sc->num_tris, p.tri);
  p.obj_material_offsets.assign(sc->obj_materialOffsets, sc->obj_materialOffsets + sc->num_shapes);
  ClusterSet& cs = p.clusters;
  choose_clusters(N, nn, sc->tris, p.tri, cluster_chord, cs);
  p.cull = cluster_margin(cs.cv0, cs.ce1, cs.ce2);
  p.wants_masks = !p.cull.exact && !cs.info.empty();
  // a super box past the half range (+-65504) would be infinite, its centre NaN and the cull wrong: such a
  // scene gets no super-cluster route (TREE_LDS16S needs num_supers > 0)
  p.num_supers = cs.supers_finite ? (int)cs.sup.size() : 0;
  for (int i = 0; i < nn; i++)
    if (cs.leaf_cl[i].y != 0 && cs.leaf_cl[i].y != (N[i].triIdSize + CLUSTER - 1) / CLUSTER) p.cl_counts = 1;
  if (!pack_nodes(N, nn, cs.leaf_cl, p.pnodes)) p.pnodes.clear();
  if (!pack_nodes16(N, nn, cs.leaf_cl, p.dnodes)) p.dnodes.clear();
  // the same records with a big leaf's first super-cluster (TREE_LDS16S), when the scene has supers
  if (p.dnodes.empty() || p.num_supers <= 0 || !pack_nodes16(N, nn, cs.leaf_sp, p.snodes)) p.snodes.clear();
  p.rlo = make_float4(N[0].mins[0], N[0].mins[1], N[0].mins[2], 0.0f);
  p.rhi = make_float4(N[0].maxs[0], N[0].maxs[1], N[0].maxs[2], 0.0f);
  p.n0_left = N[0].leftID;
  p.n0_right = N[0].rightID;
  if (nn > 1) {
    p.n1_left = N[1].leftID;
    p.n1_right = N[1].rightID;
  }
}

// KDPT_OK and *out filled, or the KDPT_ERR_* code and message kdpt_create reports (*err; *out untouched).
// opt null: the defaults.  cluster_chord: choose_clusters (the runtime passes its "cluster_chord" default).
inline int prepare_scene(const kdpt_scene* sc, const kdpt_options* opt, double cluster_chord, PreparedScene* out,
                         std::string* err) {
  auto fail = [&](int code, const char* msg) {
    if (err) *err = msg;
    return code;
  };
  if (!sc || !out) return fail(KDPT_ERR_ARG, "null scene/out");
  PreparedScene p;
  kdpt_options& o = p.opt;
  if (opt) o = *opt; else default_options(&o);
  if (o.bounce_cap <= 0) o.bounce_cap = 8;
  if (o.bounce_cap > 30) return fail(KDPT_ERR_ARG, "bounce_cap > 30");
  if (o.block_size && o.block_size != TILE) return fail(KDPT_ERR_UNSUPPORTED, "block_size must be 0 or 256");
  const int W = sc->camera.resolution[0], H = sc->camera.resolution[1];
  if (W <= 0 || H <= 0 || (long long)W * H >= (1ll << 30)) return fail(KDPT_ERR_ARG, "bad resolution");
  if ((long long)MAXB * W * H >= (1ll << 31))  // a batch's ray-queue entries are ints
    return fail(KDPT_ERR_UNSUPPORTED,
                "resolution too large for a batch's ray queue: (iterations per batch) x width x height >= 2^31");
  if (sc->num_materials > MAX_KEYS) return fail(KDPT_ERR_UNSUPPORTED, "more than 64 materials");
  p.brute = !o.enable_kd && sc->has_obj;
  p.kd = sc->has_obj && sc->num_nodes > 0 && !p.brute;
  if (p.brute) {
    // the arrays pathTraceOneBounce reads (src/pathtrace.cu:485-576) must be in bounds
    if (sc->num_shapes < 1 || !sc->obj_materialOffsets || !sc->obj_polyoffsets || !sc->obj_polysidxflat ||
        !sc->obj_verts || !sc->obj_norms)
      return fail(KDPT_ERR_ARG, "enable_kd=0 needs the OBJ arrays (obj_verts, obj_norms, obj_polysidxflat, ...)");
    long long total = 0;
    for (int i = 0; i < sc->num_shapes; i++) {
      if (sc->obj_polyoffsets[i] < 0 || sc->obj_polyoffsets[i] % 3)
        return fail(KDPT_ERR_UNSUPPORTED, "OBJ shapes must be triangulated (index counts multiple of 3)");
      if (sc->obj_materialOffsets[i] < 0 || sc->obj_materialOffsets[i] >= sc->num_materials)
        return fail(KDPT_ERR_ARG, "obj_materialOffsets out of range");
      total += sc->obj_polyoffsets[i];
    }
    if (total != sc->polyidxcount) return fail(KDPT_ERR_ARG, "obj_polyoffsets do not sum to polyidxcount");
    for (int j = 0; j < sc->polyidxcount; j++) {
      const long long v = sc->obj_polysidxflat[j];
      if (v < 0 || 3 * v + 2 >= sc->num_obj_verts || 3 * v + 2 >= sc->num_obj_norms)
        return fail(KDPT_ERR_ARG, "OBJ vertex index out of range (vertex or normal array)");
    }
    if (o.use_bbox && (!sc->obj_bboxes || sc->num_bbox_floats < sc->num_shapes + 5))
      return fail(KDPT_ERR_ARG, "use_bbox needs obj_bboxes[num_shapes + 5]");
  }
  if (p.kd) {
    // The compact visited-state traversal needs the reference builder's shape:
    // nodes[i].ID == i, root == node 0, node 1 == root's left child, <= 15 levels.
    const kdpt_node_bare* N = sc->nodes;
    int root = -1;
    for (int i = 0; i < sc->num_nodes; i++)
      if (N[i].parentID == -1) { root = N[i].ID; break; }
    if (root != 0) return fail(KDPT_ERR_UNSUPPORTED, "root must be node 0");
    for (int i = 0; i < sc->num_nodes; i++) {
      if (N[i].ID != i) return fail(KDPT_ERR_UNSUPPORTED, "nodes must be stored in ID order");
      for (int ch : {N[i].leftID, N[i].rightID})
        if (ch != -1 && (ch <= i || ch >= sc->num_nodes || N[ch].parentID != i))
          return fail(KDPT_ERR_ARG, "inconsistent KD node links");
      if (N[i].triIdSize > 0 && (N[i].triIdStart < 0 || N[i].triIdStart + N[i].triIdSize > sc->num_tris))
        return fail(KDPT_ERR_ARG, "triangle range out of bounds");
      if (N[i].triIdSize > 0 && (N[i].leftID != -1 || N[i].rightID != -1))
        return fail(KDPT_ERR_UNSUPPORTED, "KD node with both triangles and children");
    }
    if (sc->num_nodes > 1 && N[0].leftID != 1) return fail(KDPT_ERR_UNSUPPORTED, "node 1 must be root's left child");
    std::vector<int> level(sc->num_nodes, 0);
    for (int i = 1; i < sc->num_nodes; i++) {
      // only the root has no parent (the traversal tests `parentID == -1` as `cur == root`)
      if (N[i].parentID < 0 || N[i].parentID >= i) return fail(KDPT_ERR_ARG, "inconsistent KD parent links");
      level[i] = level[N[i].parentID] + 1;
      if (level[i] > 15) return fail(KDPT_ERR_UNSUPPORTED, "KD tree deeper than 15 levels");
    }
    for (int i = 0; i < sc->num_tris; i++) {
      const int m = sc->tris[i].mtlIdx;
      if (m < 0 || m >= sc->num_shapes) return fail(KDPT_ERR_ARG, "triangle mtlIdx out of range");
      if (m > 0 && !o.viz_kd) p.shade_oob = true;
    }
    // (a copy the device would refuse anyway)
    if (sc->num_shapes < 0 || (sc->num_shapes > 0 && !sc->obj_materialOffsets))
      return fail(KDPT_ERR_ARG, "num_shapes without obj_materialOffsets");
  }
  // viz_kd: the KD node boxes follow the analytic geoms, as boxes with the last material
  // (src/pathtrace.cu:1813-1831)
  p.viz = o.viz_kd && o.enable_kd && sc->has_obj && sc->num_nodes > 0;
  if (p.viz && sc->num_materials < 1) return fail(KDPT_ERR_ARG, "viz_kd needs a material");
  for (int i = 0; i < sc->num_geoms; i++) {
    if (sc->geoms[i].type != 0 && sc->geoms[i].type != 1)  // SPHERE / CUBE: the only types the scene parser creates
      return fail(KDPT_ERR_UNSUPPORTED, "geom type other than sphere (0) or cube (1)");
    if (sc->geoms[i].materialid < 0 || sc->geoms[i].materialid >= sc->num_materials)
      return fail(KDPT_ERR_ARG, "geom materialid out of range");
  }

  // accepted: the packing
  p.num_geoms = sc->num_geoms;
  p.num_boxes = p.viz ? sc->num_nodes : 0;
  p.geoms.reserve((size_t)std::max(0, p.num_geoms) + (size_t)p.num_boxes);
  for (int i = 0; i < sc->num_geoms; i++) p.geoms.push_back(prepare_geom(sc->geoms[i]));
  geoms_safe_region(p.geoms.data(), p.num_geoms, p.gc, p.gh);
  for (int k = 0; k < p.num_boxes; k++) {
    kdpt_geom g{};
    g.type = 1;
    g.materialid = sc->num_materials - 1;
    kdpt_host::node_box_matrices(sc->nodes[k].mins, sc->nodes[k].maxs, g.transform, g.inverseTransform);
    p.geoms.push_back(prepare_geom(g));
  }
  p.materials.reserve((size_t)std::max(0, sc->num_materials));
  for (int i = 0; i < sc->num_materials; i++) p.materials.push_back(prepare_material(sc->materials[i]));
  p.num_nodes = sc->has_obj && !p.brute ? sc->num_nodes : 0;
  if (p.kd) prepare_tree(sc, cluster_chord, p);
  else if (p.brute) prepare_brute(sc, o.use_bbox != 0, p);
  *out = std::move(p);
  return KDPT_OK;
}

}  // namespace kdpt
