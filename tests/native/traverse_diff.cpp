// TEST INFRASTRUCTURE: differential test of the product's compact-state KD
// traversal (kdpt_traverse.h, compiled here for the host) against the oracle's
// literal visited-bitmap restatement of traverseKDbareShortHybrid /
// traverseKDbare (oracle/liboracle.so).  Every output must match bit for bit.
//   traverse_diff SCENE.txt OBJ NRAYS SEED HYBRID          -> prints mismatch count
//   traverse_diff --desc DESC TREE NRAYS SEED HYBRID       (no scene files: tests/soups.py write_desc / write_tree)
// The second form reads a parsed scene description (the oracle builds its own scene and tree from it,
// orc_build_scene) and the product host builder's tree, the "<ii> nodes tris" file tests/native/cull_diff.cpp
// reads: the product's traversal walks the product's tree, the oracle's walks the oracle's, and the two trees are
// compared byte for byte first ("tree_equal").  A fifth of its rays are aimed exactly at a vertex or an edge
// midpoint of a random triangle (ties between triangles that share them).
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../../kdtreepathtraceroptimization_amd/csrc/kdpt_scene_prep.h"
#include "../../kdtreepathtraceroptimization_amd/csrc/kdpt_traverse.h"
extern "C" {
#include "../../oracle/kdpt_oracle.h"
}

using namespace kdpt;

static_assert(sizeof(orc_node) == 64 && sizeof(orc_tri) == 76 && sizeof(orc_material) == 56, "file record sizes");
// the oracle's records are the product's (the tree file holds kdpt_node_bare / kdpt_tri_bare): the product's own
// packing (kdpt_scene_prep.h) reads them as such
static_assert(sizeof(orc_node) == sizeof(kdpt_node_bare) && sizeof(orc_tri) == sizeof(kdpt_tri_bare) &&
              offsetof(orc_node, mins) == offsetof(kdpt_node_bare, mins) &&
              offsetof(orc_node, triIdSize) == offsetof(kdpt_node_bare, triIdSize) &&
              offsetof(orc_tri, mtlIdx) == offsetof(kdpt_tri_bare, mtlIdx), "record layouts");

static bool read_file(const char* path, std::vector<char>& out) {
  FILE* f = fopen(path, "rb");
  if (!f) return false;
  fseek(f, 0, SEEK_END);
  const long n = ftell(f);
  fseek(f, 0, SEEK_SET);
  out.resize((size_t)n);
  const bool ok = n == 0 || fread(out.data(), 1, (size_t)n, f) == (size_t)n;
  fclose(f);
  return ok;
}

// tests/soups.py write_desc's file into an orc_scene_desc whose arrays point into `buf`.
static bool parse_desc(const std::vector<char>& buf, orc_scene_desc& d) {
  size_t at = 0;
  bool ok = true;
  auto take = [&](size_t bytes) -> const char* {
    if (at + bytes > buf.size()) { ok = false; return buf.data(); }
    const char* p = buf.data() + at;
    at += bytes;
    return p;
  };
  auto geti = [&]() { int v = 0; memcpy(&v, take(4), ok ? 4 : 0); return v; };
  memset(&d, 0, sizeof d);
  d.res[0] = geti(); d.res[1] = geti();
  memcpy(&d.fovy, take(4), ok ? 4 : 0);
  d.iterations = geti(); d.traceDepth = geti();
  memcpy(d.eye, take(12), ok ? 12 : 0); memcpy(d.lookAt, take(12), ok ? 12 : 0); memcpy(d.up, take(12), ok ? 12 : 0);
  d.num_materials = geti();
  if (!ok || d.num_materials < 0) return false;
  d.materials = (const orc_material*)take(sizeof(orc_material) * (size_t)d.num_materials);
  d.num_geoms = geti();
  if (!ok || d.num_geoms < 0) return false;
  d.geom_type = (const int*)take(4 * (size_t)d.num_geoms);
  d.geom_material = (const int*)take(4 * (size_t)d.num_geoms);
  d.geom_trs = (const float*)take(36 * (size_t)d.num_geoms);
  d.ntri = geti();
  if (!ok || d.ntri < 0) return false;
  d.verts9 = (const float*)take(36 * (size_t)d.ntri);
  d.norms9 = (const float*)take(36 * (size_t)d.ntri);
  d.shape_of_tri = (const int*)take(4 * (size_t)d.ntri);
  d.num_shapes = geti();
  if (!ok || d.num_shapes < 0) return false;
  d.shape_materials = (const orc_material*)take(sizeof(orc_material) * (size_t)d.num_shapes);
  return ok && at == buf.size();
}

int main(int argc, char** argv) {
  if (argc < 6) return 2;
  const bool from_desc = strcmp(argv[1], "--desc") == 0;
  if (from_desc && argc < 7) return 2;
  orc_scene s;
  std::vector<char> desc_buf, tree_buf;
  const orc_node* PN = nullptr;  // the tree the product's traversal walks
  const orc_tri* PT = nullptr;
  int nn = 0, nt = 0, tree_equal = -1;
  if (from_desc) {
    orc_scene_desc d;
    if (!read_file(argv[2], desc_buf) || !parse_desc(desc_buf, d)) return 3;
    if (orc_build_scene(&d, &s)) return 3;
    if (!read_file(argv[3], tree_buf) || tree_buf.size() < 8) return 4;
    memcpy(&nn, tree_buf.data(), 4);
    memcpy(&nt, tree_buf.data() + 4, 4);
    if (nn < 1 || nt < 0 || tree_buf.size() != 8 + 64 * (size_t)nn + 76 * (size_t)nt) return 4;
    PN = (const orc_node*)(tree_buf.data() + 8);
    PT = (const orc_tri*)(tree_buf.data() + 8 + 64 * (size_t)nn);
    tree_equal = nn == s.num_nodes && nt == s.num_tris && memcmp(PN, s.nodes, 64 * (size_t)nn) == 0 &&
                 memcmp(PT, s.tris, 76 * (size_t)nt) == 0;
    argv += 1;
  } else {
    if (orc_load_scene(argv[1], argv[2], 0, 0, 0, &s)) return 3;
    PN = s.nodes; PT = s.tris;
    nn = s.num_nodes; nt = s.num_tris;
  }
  const long nrays = atol(argv[3]);
  const unsigned seed = (unsigned)atoi(argv[4]);
  const bool hybrid = atoi(argv[5]) != 0;
  std::vector<int4> nodes;  // the arrays kdpt_create uploads
  TriArrays T;
  pack_wide_nodes(reinterpret_cast<const kdpt_node_bare*>(PN), nn, nodes);
  pack_triangles(reinterpret_cast<const kdpt_tri_bare*>(PT), nt, T);
  std::vector<DevGeom> geoms(s.num_geoms);
  for (int i = 0; i < s.num_geoms; i++) {
    geoms[i].type = s.geoms[i].type;
    geoms[i].materialid = s.geoms[i].materialid;
    memcpy(geoms[i].transform, s.geoms[i].transform, 64);
    memcpy(geoms[i].inverseTransform, s.geoms[i].inverseTransform, 64);
    memcpy(geoms[i].invTranspose, s.geoms[i].invTranspose, 64);
  }
  DevScene S{};
  S.geoms = geoms.data();
  S.num_geoms = s.num_geoms;
  S.num_materials = s.num_materials;
  S.has_obj = s.has_obj;
  S.num_nodes = nn;
  S.root = 0;
  S.nodes = nodes.data();
  S.tv0 = T.tv0.data(); S.te1 = T.te1.data(); S.te2 = T.te2.data();
  S.tn0 = T.tn0.data(); S.tn1 = T.tn1.data(); S.tn2 = T.tn2.data();
  S.obj_material_offsets = s.obj_materialOffsets;
  S.n0_left = PN[0].leftID; S.n0_right = PN[0].rightID;
  S.n1_left = nn > 1 ? PN[1].leftID : -1; S.n1_right = nn > 1 ? PN[1].rightID : -1;
  // rays: origins anywhere in the box (incl. inside the mesh bbox), aimed at points of the mesh bbox
  std::mt19937 rng(seed);
  std::uniform_real_distribution<float> U(0.f, 1.f);
  const float* mn = PN[0].mins;
  const float* mx = PN[0].maxs;
  long bad = 0, hits = 0;
  unsigned long long aabb = 0, tri = 0;
  for (long r = 0; r < nrays; r++) {
    float o[3], tgt[3], d[3];
    for (int k = 0; k < 3; k++) {
      const float lo = k == 1 ? 0.0f : -4.9f, hi = k == 1 ? 9.9f : 4.9f;
      o[k] = (r & 3) == 0 ? mn[k] + (mx[k] - mn[k]) * U(rng) : lo + (hi - lo) * U(rng);
      tgt[k] = mn[k] + (mx[k] - mn[k]) * U(rng);
    }
    if (from_desc && nt > 0 && (r % 5) == 1) {  // exactly at a vertex (w = 3: an edge midpoint) of a triangle
      const orc_tri& T = PT[(size_t)(U(rng) * nt) % (size_t)nt];
      const float vx[3] = {T.x1, T.x2, T.x3}, vy[3] = {T.y1, T.y2, T.y3}, vz[3] = {T.z1, T.z2, T.z3};
      const int k = (int)(U(rng) * 3) % 3, w = (int)(U(rng) * 4) % 4, k2 = (k + 1) % 3;
      tgt[0] = w == 3 ? 0.5f * (vx[k] + vx[k2]) : vx[k];
      tgt[1] = w == 3 ? 0.5f * (vy[k] + vy[k2]) : vy[k];
      tgt[2] = w == 3 ? 0.5f * (vz[k] + vz[k2]) : vz[k];
    }
    f3 dd = normalize(mk3(tgt[0] - o[0], tgt[1] - o[1], tgt[2] - o[2]));
    if ((r % 7) == 0) dd = normalize(mk3(U(rng) - 0.5f, U(rng) - 0.5f, U(rng) - 0.5f));
    d[0] = dd.x; d[1] = dd.y; d[2] = dd.z;
    double ref[14];
    orc_trace_ray(&s, o, d, hybrid ? 1 : 0, ref);
    Ray ray;
    ray.origin = mk3(o[0], o[1], o[2]);
    ray.direction = dd;
    ray.isinside = false;
    ray.sdepth = 0;
    Hit h;
    h.t_min = FLT_MAXV; h.hit_geom_index = -1; h.obj_intersect = false; h.objMaterialIdx = -1;
    h.ip = mk3(0, 0, 0); h.normal = mk3(0, 0, 0);
    f3 ti = mk3(0, 0, 0), tn = mk3(0, 0, 0);
    float t = 0;
    for (int g = 0; g < S.num_geoms; g++) {
      if (geoms[g].type == 1) t = boxIntersectionTest(geoms[g], ray, ti, tn);
      else if (geoms[g].type == 0) t = sphereIntersectionTest(geoms[g], ray, ti, tn);
      if (t > 0.0f && h.t_min > t) { h.t_min = t; h.hit_geom_index = g; h.ip = ti; h.normal = tn; }
    }
    TraverseCounters cnt{0, 0, 0};
    if (hybrid) traverseKD<true, true>(S, ray, h, S.num_materials, cnt);
    else traverseKD<false, true>(S, ray, h, S.num_materials, cnt);
    const double got[13] = {h.t_min, (double)h.hit_geom_index, h.ip.x, h.ip.y, h.ip.z, h.normal.x, h.normal.y,
                            h.normal.z, (double)h.obj_intersect, (double)h.objMaterialIdx, (double)cnt.aabb,
                            (double)cnt.tri, (double)cnt.hit};
    bool ok = true;
    for (int k = 0; k < 13; k++)
      if (memcmp(&got[k], &ref[k], sizeof(double)) != 0 && !(got[k] != got[k] && ref[k] != ref[k])) ok = false;
    if (!ok) {
      if (bad < 5) {
        printf("mismatch ray %ld:", r);
        for (int k = 0; k < 13; k++) printf(" %g/%g", got[k], ref[k]);
        printf("\n");
      }
      bad++;
    }
    if (h.obj_intersect) hits++;
    aabb += cnt.aabb;
    tri += cnt.tri;
  }
  printf("{\"rays\": %ld, \"mismatches\": %ld, \"obj_hits\": %ld, \"aabb\": %llu, \"tri\": %llu, \"nodes\": %d, "
         "\"tris\": %d, \"tree_equal\": %d}\n", nrays, bad, hits, aabb, tri, nn, nt, tree_equal);
  orc_free_scene(&s);
  return bad || tree_equal == 0 ? 1 : 0;
}
