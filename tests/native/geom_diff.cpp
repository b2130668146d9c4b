// TEST INFRASTRUCTURE: differential test of the product's analytic-geom stage (kdpt_geoms.h prep_ray: the
// nearest-first loop over geom_entry_bound for at most ORDERED_GEOMS geoms, the index-order loop with the
// geom_may_hit skip above that, over kdpt_scene_prep.h prepare_geom's bounds; all compiled here for the host)
// against the oracle's plain index-order loop (orc_trace_ray, oracle/liboracle.so): the winning geom and the
// bits of t must be equal for every ray.
//   geom_diff DESC [--ties] [--dump-mismatches K FILE] NAME=RAYS ...
// DESC is tests/geoms.py write_desc's file (the oracle builds its scene from it, the product's DevGeoms are
// prepare_geom of that scene's geoms); each RAYS file is tests/geoms.py write_rays' (int32 n, n origins, n
// directions as traced).  One JSON line per RAYS file.  "ordered" counts the rays that met prep_ray's
// condition for the nearest-first loop with the bounds in force; "winners", "ties" and "inside" are the oracle's
// alone: per geom the rays it wins; with --ties the rays on which two geoms report the same t > 0 (each geom
// traced alone, as a one-geom oracle scene); the hits whose origin lies inside the winner (the oracle's
// inverseTransform of the origin, in double).  The scene's triangles are left out (prep_ray with kd = false).
// --dump-mismatches: the first K differing rays (float32 o[3] d[3] each) over all the RAYS files, to FILE.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../kdtreepathtraceroptimization_amd/csrc/kdpt_scene_prep.h"
#include "../../kdtreepathtraceroptimization_amd/csrc/kdpt_geoms.h"
extern "C" {
#include "../../oracle/kdpt_oracle.h"
}

using namespace kdpt;

static_assert(sizeof(orc_geom) == sizeof(kdpt_geom) && offsetof(orc_geom, transform) == offsetof(kdpt_geom, transform) &&
              offsetof(orc_geom, invTranspose) == offsetof(kdpt_geom, invTranspose), "geom record layouts");
static_assert(sizeof(orc_material) == 56, "file record sizes");

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

// tests/soups.py write_desc's file into an orc_scene_desc whose arrays point into `buf` (as traverse_diff.cpp)
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
  if (argc < 3) return 2;
  std::vector<char> desc_buf;
  orc_scene_desc d;
  if (!read_file(argv[1], desc_buf) || !parse_desc(desc_buf, d)) return 3;
  d.ntri = 0;  // the analytic geoms alone
  d.num_shapes = 0;
  orc_scene s;
  if (orc_build_scene(&d, &s)) return 3;
  const int ng = s.num_geoms;
  bool ties = false;
  long dump_k = 0, dumped = 0;
  FILE* dump = nullptr;
  std::vector<std::pair<std::string, std::string>> files;
  for (int a = 2; a < argc; a++) {
    if (strcmp(argv[a], "--ties") == 0) {
      ties = true;
    } else if (strcmp(argv[a], "--dump-mismatches") == 0 && a + 2 < argc) {
      dump_k = atol(argv[a + 1]);
      dump = fopen(argv[a + 2], "wb");
      if (!dump) return 4;
      a += 2;
    } else {
      const char* eq = strchr(argv[a], '=');
      if (!eq) return 2;
      files.emplace_back(std::string(argv[a], (size_t)(eq - argv[a])), std::string(eq + 1));
    }
  }
  std::vector<orc_scene> alone;  // each geom as a scene of its own
  if (ties) {
    alone.resize((size_t)ng);
    for (int g = 0; g < ng; g++) {
      orc_scene_desc one = d;
      one.num_geoms = 1;
      one.geom_type = d.geom_type + g;
      one.geom_material = d.geom_material + g;
      one.geom_trs = d.geom_trs + 9 * (size_t)g;
      if (orc_build_scene(&one, &alone[(size_t)g])) return 3;
    }
  }
  std::vector<DevGeom> geoms((size_t)ng);
  for (int i = 0; i < ng; i++) {
    kdpt_geom g;
    memcpy(&g, &s.geoms[i], sizeof g);
    geoms[(size_t)i] = prepare_geom(g);
  }
  DevScene S{};
  S.geoms = geoms.data();
  S.num_geoms = ng;
  S.num_materials = s.num_materials;
  geoms_safe_region(geoms.data(), ng, S.gc, S.gh);
  printf("ranges:");  // each geom's proven range, then the region of the nearest-first loop
  for (int i = 0; i < ng; i++) printf(" %g", geoms[(size_t)i].wlo[3]);
  printf(" region: [%g %g %g] +- [%g %g %g]\n", S.gc.x, S.gc.y, S.gc.z, S.gh.x, S.gh.y, S.gh.z);
  long total_bad = 0;
  for (const auto& nf : files) {
    std::vector<char> rb;
    int n = 0;
    if (!read_file(nf.second.c_str(), rb) || rb.size() < 4) return 5;
    memcpy(&n, rb.data(), 4);
    if (n < 0 || rb.size() != 4 + 24 * (size_t)n) return 5;
    const float* O = (const float*)(rb.data() + 4);
    const float* D = O + 3 * (size_t)n;
    long bad = 0, hits = 0, ntie = 0, inside = 0, ordered = 0;
    std::vector<long> winners((size_t)ng, 0);
    for (long r = 0; r < n; r++) {
      const float* o = O + 3 * r;
      const float* dd = D + 3 * r;
      double ref[14];
      orc_trace_ray(&s, o, dd, 1, ref);
      float t_min = 0.0f;
      int hit = -2;
      (void)prep_ray(S, false, mk3(o[0], o[1], o[2]), mk3(dd[0], dd[1], dd[2]), t_min, hit);
      // the rays that take the nearest-first loop (prep_ray's condition)
      if (ng <= ORDERED_GEOMS && geoms_hold_for(S, mk3(o[0], o[1], o[2])) && std::isfinite(1.0f / dd[0]) &&
          std::isfinite(1.0f / dd[1]) && std::isfinite(1.0f / dd[2]))
        ordered++;
      const float want_t = (float)ref[0];
      const int want = (int)ref[1];
      if (want >= 0) {
        hits++;
        winners[(size_t)want]++;
        const float* m = s.geoms[want].inverseTransform;  // column-major
        double q[3];
        for (int k = 0; k < 3; k++)
          q[k] = (double)m[k] * o[0] + (double)m[4 + k] * o[1] + (double)m[8 + k] * o[2] + (double)m[12 + k];
        const bool in = s.geoms[want].type == 1
                            ? std::fabs(q[0]) < 0.5 && std::fabs(q[1]) < 0.5 && std::fabs(q[2]) < 0.5
                            : q[0] * q[0] + q[1] * q[1] + q[2] * q[2] < 0.25;
        if (in) inside++;
      }
      if (ties) {
        bool tie = false;
        std::vector<float> ts;
        for (int g = 0; g < ng && !tie; g++) {
          double one[14];
          orc_trace_ray(&alone[(size_t)g], o, dd, 1, one);
          if ((int)one[1] != 0) continue;
          for (float t : ts) tie = tie || t == (float)one[0];
          ts.push_back((float)one[0]);
        }
        if (tie) ntie++;
      }
      if (hit != want || memcmp(&t_min, &want_t, 4) != 0) {
        if (bad < 5) printf("mismatch %s ray %ld: geom %d/%d t %.9g/%.9g\n", nf.first.c_str(), r, hit, want, t_min, want_t);
        bad++;
        if (dump && dumped < dump_k) {
          fwrite(o, 4, 3, dump);
          fwrite(dd, 4, 3, dump);
          dumped++;
        }
      }
    }
    printf("{\"gen\": \"%s\", \"rays\": %d, \"mismatches\": %ld, \"hits\": %ld, \"ties\": %ld, \"inside\": %ld, \"ordered\": %ld, \"winners\": [",
           nf.first.c_str(), n, bad, hits, ties ? ntie : -1L, inside, ordered);
    for (int g = 0; g < ng; g++) printf("%s%ld", g ? ", " : "", winners[(size_t)g]);
    printf("]}\n");
    total_bad += bad;
  }
  if (dump) fclose(dump);
  for (orc_scene& a : alone) orc_free_scene(&a);
  orc_free_scene(&s);
  return total_bad ? 1 : 0;
}
