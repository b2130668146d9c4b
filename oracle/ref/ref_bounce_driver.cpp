// ref_bounce_driver.cpp -- TEST INFRASTRUCTURE ONLY.
//
// Known answers for the bounce from the reference's OWN src/interactions.h and src/intersections.h,
// compiled in place, host-only, from /root/reference by oracle/ref/Makefile (target ref_bounce, output in
// oracle/_ref/): scatterRay, boxIntersectionTest and sphereIntersectionTest are the reference's functions,
// its Ray / Geom / Material its structs, glm its vendored 0.9.6.3, and the engine rocThrust's
// thrust::default_random_engine (oracle/ref/thrust_rng_driver.cpp says why rocThrust).  Nothing of the
// product or the oracle is linked in.  The one stand-in is oracle/ref/stub/cuda_runtime.h, an empty file
// for sceneStructs.h's #include.  shadeMaterial is a __global__ of src/pathtrace.cu and is not reachable
// this way.
//
// Rows of 32-bit words, float unless said otherwise (tests/kat_inputs.py has the same table):
//   ref_bounce scatter N IN OUT   IN: origin 0-2, direction 3-5, isinside 6 (0 / 1), sdepth 7, intersect
//                                 8-10, normal 11-13, hasReflective 14, hasRefractive 15, indexOfRefraction
//                                 16, transmittance 17-19, softness 20, seed 21 (uint32).
//                                 scatterRay with thrust::default_random_engine(seed).  OUT: origin 0-2,
//                                 direction 3-5, isinside 6, sdepth 7, one further u01 draw 8 (so the
//                                 number of draws a branch consumes is pinned too)
//   ref_bounce geom N IN OUT      IN: type 0 (int32: 0 sphere, 1 cube), transform / inverseTransform /
//                                 invTranspose 1-48, origin 49-51, direction 52-54.  OUT (read first: the
//                                 point and the normal keep their words where the test leaves them
//                                 unwritten): t 0, hit point 1-3, normal 4-6
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include <thrust/random.h>

using std::max;
using std::min;

#include "interactions.h"

static std::vector<float> read_f32(const char* path, size_t n) {
  std::vector<float> v(n);
  FILE* f = fopen(path, "rb");
  if (!f || fread(v.data(), sizeof(float), n, f) != n) {
    fprintf(stderr, "cannot read %zu words from %s\n", n, path);
    exit(3);
  }
  fclose(f);
  return v;
}

static void write_f32(const char* path, const std::vector<float>& v) {
  FILE* f = fopen(path, "wb");
  if (!f || fwrite(v.data(), sizeof(float), v.size(), f) != v.size()) {
    fprintf(stderr, "cannot write %s\n", path);
    exit(3);
  }
  fclose(f);
}

static glm::vec3 vec3_at(const float* p) { return glm::vec3(p[0], p[1], p[2]); }

int main(int argc, char** argv) {
  if (argc != 5) {
    fprintf(stderr, "usage: %s scatter|geom N IN OUT\n", argv[0]);
    return 2;
  }
  const size_t n = (size_t)atol(argv[2]);
  if (!strcmp(argv[1], "scatter")) {
    const std::vector<float> in = read_f32(argv[3], 22 * n);
    std::vector<float> out(9 * n);
    for (size_t i = 0; i < n; i++) {
      const float* a = &in[22 * i];
      float* o = &out[9 * i];
      Ray r;
      r.origin = vec3_at(a);
      r.direction = vec3_at(a + 3);
      r.isinside = a[6] != 0.0f;
      r.sdepth = a[7];
      Material m;
      memset(&m, 0, sizeof m);
      m.hasReflective = a[14];
      m.hasRefractive = a[15];
      m.indexOfRefraction = a[16];
      m.transmittance = vec3_at(a + 17);
      unsigned int seed;
      memcpy(&seed, a + 21, 4);
      thrust::default_random_engine rng(seed);
      glm::vec3 color(1.0f);
      scatterRay(r, color, vec3_at(a + 8), vec3_at(a + 11), m, rng, a[20]);
      thrust::uniform_real_distribution<float> u01(0, 1);
      o[0] = r.origin.x, o[1] = r.origin.y, o[2] = r.origin.z;
      o[3] = r.direction.x, o[4] = r.direction.y, o[5] = r.direction.z;
      o[6] = r.isinside ? 1.0f : 0.0f;
      o[7] = r.sdepth;
      o[8] = u01(rng);
    }
    write_f32(argv[4], out);
    return 0;
  }
  if (!strcmp(argv[1], "geom")) {
    const std::vector<float> in = read_f32(argv[3], 55 * n);
    std::vector<float> out = read_f32(argv[4], 7 * n);
    for (size_t i = 0; i < n; i++) {
      const float* a = &in[55 * i];
      float* o = &out[7 * i];
      Geom g;
      memset(&g, 0, sizeof g);
      int type;
      memcpy(&type, a, 4);
      g.type = type == 1 ? CUBE : SPHERE;
      memcpy(&g.transform, a + 1, 64);
      memcpy(&g.inverseTransform, a + 17, 64);
      memcpy(&g.invTranspose, a + 33, 64);
      Ray r;
      r.origin = vec3_at(a + 49);
      r.direction = vec3_at(a + 52);
      r.isinside = false;
      r.sdepth = 0.0f;
      glm::vec3 ip = vec3_at(o + 1), nrm = vec3_at(o + 4);
      bool outside = false;
      o[0] = g.type == CUBE ? boxIntersectionTest(g, r, ip, nrm, outside)
                            : sphereIntersectionTest(g, r, ip, nrm, outside);
      o[1] = ip.x, o[2] = ip.y, o[3] = ip.z, o[4] = nrm.x, o[5] = nrm.y, o[6] = nrm.z;
    }
    write_f32(argv[4], out);
    return 0;
  }
  return 2;
}
