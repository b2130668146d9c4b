// TEST INFRASTRUCTURE: the product's host code under AddressSanitizer + UBSan (CPU only).
//   asan_host SCENE.txt OBJ|- NRAYS
// Parses the scene and OBJ with the product's C++ parsers and builds the KD tree (csrc/scene_host.cpp),
// encodes a PNG and an HDR of a small image (csrc/image_io.cpp), and walks NRAYS random rays through the
// compact-state traversal (csrc/kdpt_traverse.h compiled for the host).  Exits non-zero on a parse error
// code; the sanitizers abort on any memory or UB finding.  Prints a JSON summary; for a refused input it holds
// the code and kdpt_last_error()'s message.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "kdpt.h"
#include "../../kdtreepathtraceroptimization_amd/csrc/kdpt_scene_prep.h"
#include "../../kdtreepathtraceroptimization_amd/csrc/kdpt_traverse.h"

using namespace kdpt;

int main(int argc, char** argv) {
  if (argc != 4) return 2;
  kdpt_scene_data* sd = nullptr;
  const char* obj = strcmp(argv[2], "-") ? argv[2] : nullptr;
  int rc = kdpt_scene_load(argv[1], obj, 0, 0, 0, &sd);
  if (rc) {
    printf("{\"load_rc\": %d, \"error\": \"", rc);
    for (const char* p = kdpt_last_error(); *p; p++) {  // as a JSON string
      if (*p == '"' || *p == '\\') printf("\\%c", *p);
      else if ((unsigned char)*p < 0x20) printf("\\u%04x", *p);
      else putchar(*p);
    }
    printf("\"}\n");
    return 0;  // a refused input is a valid outcome; the sanitizers judge how it was refused
  }
  kdpt_scene s;
  kdpt_scene_view(sd, &s);
  // encoders on a small gradient image
  const int w = 17, h = 5;
  std::vector<float> img(3 * w * h);
  std::vector<uint8_t> rgb(3 * w * h);
  for (int i = 0; i < 3 * w * h; i++) {
    img[i] = (float)i / (3 * w * h) * 1.5f;
    rgb[i] = (uint8_t)(i * 7);
  }
  uint8_t* out = nullptr;
  size_t len = 0, png_len = 0;
  if (kdpt_png_encode(rgb.data(), w, h, &out, &png_len)) return 4;
  kdpt_free(out);
  if (kdpt_hdr_encode(img.data(), w, h, &out, &len)) return 4;
  kdpt_free(out);
  long hits = 0;
  unsigned long long aabb = 0, tri = 0;
  const long nrays = atol(argv[3]);
  if (s.has_obj && s.num_nodes > 0) {
    const int nn = s.num_nodes, nt = s.num_tris;
    std::vector<int4> nodes;  // the arrays kdpt_create uploads (kdpt_scene_prep.h)
    TriArrays T;
    pack_wide_nodes(s.nodes, nn, nodes);
    pack_triangles(s.tris, nt, T);
    DevScene S{};
    S.num_geoms = 0;
    S.num_materials = s.num_materials;
    S.has_obj = 1;
    S.num_nodes = nn;
    S.root = 0;
    S.nodes = nodes.data();
    S.tv0 = T.tv0.data(); S.te1 = T.te1.data(); S.te2 = T.te2.data();
    S.tn0 = T.tn0.data(); S.tn1 = T.tn1.data(); S.tn2 = T.tn2.data();
    S.obj_material_offsets = s.obj_materialOffsets;
    S.n0_left = s.nodes[0].leftID; S.n0_right = s.nodes[0].rightID;
    S.n1_left = nn > 1 ? s.nodes[1].leftID : -1; S.n1_right = nn > 1 ? s.nodes[1].rightID : -1;
    std::mt19937 rng(5);
    std::uniform_real_distribution<float> U(0.f, 1.f);
    const float* mn = s.nodes[0].mins;
    const float* mx = s.nodes[0].maxs;
    for (long r = 0; r < nrays; r++) {
      float o[3], t[3];
      for (int k = 0; k < 3; k++) {
        const float ext = mx[k] - mn[k] + 1.0f;
        o[k] = mn[k] - ext + 3 * ext * U(rng);
        t[k] = mn[k] + (mx[k] - mn[k]) * U(rng);
      }
      Ray ray;
      ray.origin = mk3(o[0], o[1], o[2]);
      ray.direction = normalize(mk3(t[0] - o[0], t[1] - o[1], t[2] - o[2]));
      ray.isinside = false;
      ray.sdepth = 0;
      for (int hyb = 0; hyb < 2; hyb++) {
        Hit hh;
        hh.t_min = FLT_MAXV; hh.hit_geom_index = -1; hh.obj_intersect = false; hh.objMaterialIdx = -1;
        hh.ip = mk3(0, 0, 0); hh.normal = mk3(0, 0, 0);
        TraverseCounters cnt{0, 0, 0};
        if (hyb) traverseKD<true, true>(S, ray, hh, S.num_materials, cnt);
        else traverseKD<false, true>(S, ray, hh, S.num_materials, cnt);
        hits += hh.obj_intersect;
        aabb += cnt.aabb;
        tri += cnt.tri;
      }
    }
  }
  printf("{\"load_rc\": 0, \"geoms\": %d, \"nodes\": %d, \"tris\": %d, \"png_len\": %zu, \"hits\": %ld, "
         "\"aabb\": %llu, \"tri\": %llu}\n", s.num_geoms, s.num_nodes, s.num_tris, png_len, hits, aabb, tri);
  kdpt_scene_free(sd);
  return 0;
}
