// kdpt_traverse.h -- the reference's KD walk for one ray as a __host__ __device__ function, and its triangle
// tests.  Follows src/pathtrace.cu:1023-1235 (traverseKDbareShortHybrid), :881-1020 (traverseKDbare) and glm's
// intersectRayTriangle.
//
// KD traversal state.  The reference keeps a per-thread `bool nodeIDs[4000]`
// visited bitmap (4 KB zeroed per ray per bounce).  Traversal only moves
// parent<->child, a node is marked before control leaves it upward, so it is
// never re-entered, and the only flags ever read belong to the current node,
// its parent and its two children.  The only writes to nodes off the current
// root-to-node path are the hybrid "skip other side" marks, which land on the
// children of nodes[0] or nodes[1] (the bug `nodes[nodeIDs[parentID]]`).
// So the bitmap is exactly representable by
//   cb    : 2 bits per level L = visited flags of the two children of the
//           path node at level L (reset when that level is (re)entered),
//   ps    : bit L = which child the path took at level L,
//   rootv : visited flag of the root,
//   g     : flags of nodes[1]'s two children while the path is outside
//           node 1's subtree (loaded into cb level 1 on entering node 1),
//   sink  : nodeIDs[-1] (written by leaf "children" marks, read by the skip
//           line when the current leaf is the root).
// Everything lives in 4 scalars per lane -- no LDS, no scratch.
#pragma once

#include "kdpt_geoms.h"

namespace kdpt {

struct Hit {
  float t_min;
  int hit_geom_index;
  f3 ip, normal;
  bool obj_intersect;
  int objMaterialIdx;
};

struct TraverseCounters {
  uint32_t aabb, tri, hit;
};

// The hybrid walk's skip line after an intersected triangle of the leaf at level L (leftFirst: the leaf's side
// order), on the compact visited state: nodeIDs[nodes[nodeIDs[node->parentID]].(right|left)ID] = true.  The host
// walk marks once per hit; k_trace's commit marks min(hits, 2) times (the same state from the second on).
KDPT_HDI void skip_line_mark(const DevScene& S, int L, bool leftFirst, uint32_t ps, bool rootv, uint32_t& cb,
                             uint32_t& g, bool& sink) {
  const bool parVis = (L == 0) ? sink
                      : (L == 1 ? rootv
                                : (((cb >> (2 * (L - 2) + (int)((ps >> (L - 2)) & 1u))) & 1u) != 0u));
  const int b = parVis ? 1 : 0;
  int target = -1;
  if (b < S.num_nodes) target = (b == 0) ? (leftFirst ? S.n0_right : S.n0_left) : (leftFirst ? S.n1_right : S.n1_left);
  if (target == -1) {
    sink = true;
  } else if (b == 0) {
    cb |= 1u << (leftFirst ? 1 : 0);
  } else {
    const uint32_t bit = leftFirst ? 1u : 0u;
    if (L >= 1 && (ps & 1u) == 0u) cb |= 1u << (2 + bit);
    else g |= 1u << bit;
  }
}

// traverseKDbareShortHybrid (HYBRID) / traverseKDbare, with the compact visited state.  on_leaf(node) is
// called for every leaf whose triangles are tested (host tools: tests/native/cull_diff.cpp --sim).
struct NoLeafHook {
#if defined(__HIPCC__) || defined(__HIP__)
  __host__ __device__
#endif
  void operator()(int) const {}
};
template <bool HYBRID, bool COUNT, typename LeafHook = NoLeafHook>
KDPT_HD void traverseKD(const DevScene& S, const Ray& ray, Hit& h, int material_size, TraverseCounters& cnt,
                        LeafHook on_leaf = LeafHook{}) {
  if (S.num_nodes == 0) return;
  const f3 o = ray.origin, d = ray.direction;
  const f3 invdir = mk3(1.0f / d.x, 1.0f / d.y, 1.0f / d.z);
  const float hit_eps = HYBRID ? 0.0001f : 0.00001f;
  int cur = S.root;
  int L = 0;
  uint32_t cb = 0, ps = 0, g = 0;
  bool rootv = false, sink = false;
  bool hitGeom = false;
  float dist = -1.0f;
  float bz = FLT_MAXV;  // bary.z
  while (true) {
    if (cur == -1) break;
    const int4 q0 = S.nodes[4 * cur];
    const int4 q1 = S.nodes[4 * cur + 1];
    const int4 meta = S.nodes[4 * cur + 2];
    const float4 b0 = make_float4(ibits(q0.x), ibits(q0.y), ibits(q0.z), ibits(q0.w));
    const float4 b1 = make_float4(ibits(q1.x), ibits(q1.y), 0.0f, 0.0f);
    const int left = q1.z, right = q1.w, parent = meta.x;
    const int lvlbit = (L > 0) ? (2 * (L - 1) + (int)((ps >> (L - 1)) & 1u)) : 0;
    const bool curVis = (L == 0) ? rootv : (((cb >> lvlbit) & 1u) != 0u);
    if (!hitGeom && cur == S.root && curVis) break;
    hitGeom = intersectAABB(o, invdir, b0, b1, dist);
    if (COUNT) cnt.aabb++;
    bool up = false;
    if (curVis) {
      up = true;
    } else {
      if (!hitGeom && cur == S.root) break;
      if (!hitGeom || dist > bz) up = true;
    }
    if (up) {
      // nodeIDs[ID] = nodeIDs[leftID] = nodeIDs[rightID] = true; currID = parentID
      if (L == 0) rootv = true; else cb |= 1u << lvlbit;
      if (left == -1) sink = true; else cb |= 1u << (2 * L);
      if (right == -1) sink = true; else cb |= 1u << (2 * L + 1);
      cur = parent;
      L--;
      continue;
    }
    const bool leftFirst = HYBRID ? (comp(d, meta.w) > 0.0f) : true;
    const uint32_t fside = leftFirst ? 0u : 1u;
    const int first = leftFirst ? left : right, second = leftFirst ? right : left;
    int next = -1;
    uint32_t nside = 0;
    if (first != -1 && !((cb >> (2 * L + fside)) & 1u)) { next = first; nside = fside; }
    else if (second != -1 && !((cb >> (2 * L + (fside ^ 1u))) & 1u)) { next = second; nside = fside ^ 1u; }
    if (next != -1) {
      ps = (ps & ~(1u << L)) | (nside << L);
      const uint32_t lv = 2u * (uint32_t)(L + 1);
      cb &= ~(3u << lv);
      if (L == 0 && nside == 0u) cb |= g << 2;  // entering nodes[1]: its children may carry skip marks
      L++;
      cur = next;
      continue;
    }
    // nodeIDs[node->ID] == false here (the visited branch above took the true case)
    if (L == 0) rootv = true; else cb |= 1u << lvlbit;
    const int size = meta.z;
    if (size > 0) {
      on_leaf(cur);
      const int start = meta.y, end = start + size;
      for (int i = start; i < end; i++) {
        const float4 tv = S.tv0[i];
        const float4 e1v = S.te1[i];
        const float4 e2v = S.te2[i];
        const f3 v0 = mk3(tv.x, tv.y, tv.z), e1 = mk3(e1v.x, e1v.y, e1v.z), e2 = mk3(e2v.x, e2v.y, e2v.z);
        if (COUNT) cnt.tri++;
        // glm::intersectRayTriangle (gtx/intersect.inl:37-74)
        const f3 p = cross(d, e2);
        const float a = dot(e1, p);
        if (a < FLT_EPS) continue;
        const float f = 1.0f / a;
        const f3 s = sub(o, v0);
        const float bx = f * dot(s, p);
        if (bx < 0.0f) continue;
        if (bx > 1.0f) continue;
        const f3 q = cross(s, e1);
        const float by = f * dot(d, q);
        if (by < 0.0f) continue;
        if (by + bx > 1.0f) continue;
        bz = f * dot(e2, q);
        if (!(bz >= 0.0f)) continue;
        if (COUNT) cnt.hit++;
        if (HYBRID) skip_line_mark(S, L, leftFirst, ps, rootv, cb, g, sink);
        const float4 n1v = S.tn0[i], n2v = S.tn1[i], n3v = S.tn2[i];
        const int mtl = fbits(tv.w);
        h.objMaterialIdx = mtl + material_size - 1;
        f3 hit = add(o, scl(d, bz));
        const float w0 = 1 - bx - by;
        const f3 norm = normalize(add(add(scl(mk3(n1v.x, n1v.y, n1v.z), w0), scl(mk3(n2v.x, n2v.y, n2v.z), bx)),
                                      scl(mk3(n3v.x, n3v.y, n3v.z), by)));
        hit = add(hit, scl(norm, hit_eps));
        const float t = distance(o, hit);
        if (t > 0.0f && h.t_min > t) {
          h.t_min = t;
          h.hit_geom_index = S.obj_material_offsets[mtl];
          h.ip = hit;
          h.normal = norm;
          h.obj_intersect = true;
        }
      }
    }
    // stay on this node: the next trip finds it visited and climbs
  }
}

// glm::intersectRayTriangle on (o, d) and triangle i; returns 0 = miss before the u/v
// tests passed, 1 = passed u/v but t < 0 (bary.z still written), 2 = intersected.
struct TriData {
  float4 v0, e1, e2;
};
KDPT_HD int tri_test_v(const TriData& T, f3 o, f3 d, float& bx, float& by, float& bz) {
  const float4 tv = T.v0, e1v = T.e1, e2v = T.e2;
  const f3 v0 = mk3(tv.x, tv.y, tv.z), e1 = mk3(e1v.x, e1v.y, e1v.z), e2 = mk3(e2v.x, e2v.y, e2v.z);
  const f3 p = cross(d, e2);
  const float a = dot(e1, p);
  if (a < FLT_EPS) return 0;
  const float f = 1.0f / a;
  const f3 s = sub(o, v0);
  bx = f * dot(s, p);
  if (bx < 0.0f) return 0;
  if (bx > 1.0f) return 0;
  const f3 q = cross(s, e1);
  by = f * dot(d, q);
  if (by < 0.0f) return 0;
  if (by + bx > 1.0f) return 0;
  bz = f * dot(e2, q);
  return (bz >= 0.0f) ? 2 : 1;
}

// The hit point of an intersected triangle (barycentrics bx, by, parameter bz; vertex normals n1v .. n3v), moved
// along the interpolated normal as the reference moves it, and its distance from the origin: the t it compares.
template <bool HYBRID>
KDPT_HD float tri_hit_t_n(float4 n1v, float4 n2v, float4 n3v, f3 o, f3 d, float bx, float by, float bz, f3& hit,
                          f3& norm) {
  const float w0 = 1 - bx - by;
  norm = normalize(add(add(scl(mk3(n1v.x, n1v.y, n1v.z), w0), scl(mk3(n2v.x, n2v.y, n2v.z), bx)),
                       scl(mk3(n3v.x, n3v.y, n3v.z), by)));
  hit = add(add(o, scl(d, bz)), scl(norm, HYBRID ? 0.0001f : 0.00001f));
  return distance(o, hit);
}

}  // namespace kdpt
