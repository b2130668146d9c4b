// kdpt_bounce_kat.h -- known answers for the bounce as units: scatterRay, shade and the analytic geom tests
// on one record each (kernels_selftest.h runs scatter and shade on gfx950, tests/native/bounce_host.cpp all
// three on the host).
#pragma once

#include "kdpt_geoms.h"
#include "kdpt_scatter.h"

namespace kdpt {

// Records are rows of 32-bit words, float unless said otherwise; tests/kat_inputs.py generates them and
// oracle/ref/ref_bounce_driver.cpp feeds the same rows to the reference's own src/interactions.h and
// src/intersections.h.
constexpr int SCATTER_KAT_IN = 22, SCATTER_KAT_OUT = 9;
constexpr int SHADE_KAT_IN = 19, SHADE_KAT_OUT = 4;
constexpr int GEOM_KAT_IN = 55, GEOM_KAT_OUT = 7;

// in: origin 0-2, direction 3-5, isinside 6 (0 / 1), sdepth 7, intersect 8-10, normal 11-13, hasReflective 14,
// hasRefractive 15, indexOfRefraction 16, transmittance 17-19, softness 20, seed 21 (uint32).  scatterRay with
// engine(seed).  out: origin 0-2, direction 3-5, isinside 6, sdepth 7, the engine's next u01 draw 8 (which pins
// how many draws the branch consumed).
KDPT_HD void scatter_kat(const float* in, float* out) {
  Ray r;
  r.origin = mk3(in[0], in[1], in[2]);
  r.direction = mk3(in[3], in[4], in[5]);
  r.isinside = in[6] != 0.0f;
  r.sdepth = in[7];
  DevMaterial m{};
  m.hasReflective = in[14];
  m.hasRefractive = in[15];
  m.indexOfRefraction = in[16];
  m.transmittance[0] = in[17];
  m.transmittance[1] = in[18];
  m.transmittance[2] = in[19];
  const float rr = (1.0f - m.indexOfRefraction) / (1.0f + m.indexOfRefraction);  // as prepare_material
  m.fresnel_R0 = rr * rr;
  Rng rng = rng_seed(f2u(in[21]));
  scatterRay(r, mk3(in[8], in[9], in[10]), mk3(in[11], in[12], in[13]), m, rng, in[20]);
  out[0] = r.origin.x;
  out[1] = r.origin.y;
  out[2] = r.origin.z;
  out[3] = r.direction.x;
  out[4] = r.direction.y;
  out[5] = r.direction.z;
  out[6] = r.isinside ? 1.0f : 0.0f;
  out[7] = r.sdepth;
  out[8] = u01(rng);
}

// in: t 0, material colour 1-3, specular colour 4-6, hasReflective 7, hasRefractive 8, emittance 9,
// transmittance 10-12, enable_sss 13 (0 / 1), ray sdepth 14, path colour 15-17, remainingBounces 18 (int32).
// out: path colour 0-2, remainingBounces 3 (int32).
KDPT_HD void shade_kat(const float* in, float* out) {
  DevMaterial m{};
  m.color[0] = in[1];
  m.color[1] = in[2];
  m.color[2] = in[3];
  m.spec_color[0] = in[4];
  m.spec_color[1] = in[5];
  m.spec_color[2] = in[6];
  m.hasReflective = in[7];
  m.hasRefractive = in[8];
  m.emittance = in[9];
  m.transmittance[0] = in[10];
  m.transmittance[1] = in[11];
  m.transmittance[2] = in[12];
  Ray r;
  r.origin = r.direction = mk3(0.0f, 0.0f, 0.0f);
  r.isinside = false;
  r.sdepth = in[14];
  f3 color = mk3(in[15], in[16], in[17]);
  int bounces = fbits(in[18]);
  shade(in[0], 0, &m, in[13] != 0.0f, r, color, bounces);
  out[0] = color.x;
  out[1] = color.y;
  out[2] = color.z;
  out[3] = ibits(bounces);
}

// in: type 0 (int32: 0 sphere, 1 cube), transform / inverseTransform / invTranspose 1-48, origin 49-51,
// direction 52-54.  out (read first: hit point and normal keep the caller's words where the test does not write
// them): t 0, hit point 1-3, normal 4-6.
KDPT_HD void geom_test_kat(const float* in, float* out) {
  DevGeom g{};
  g.type = fbits(in[0]);
  for (int k = 0; k < 16; k++) {
    g.transform[k] = in[1 + k];
    g.inverseTransform[k] = in[17 + k];
    g.invTranspose[k] = in[33 + k];
  }
  Ray r;
  r.origin = mk3(in[49], in[50], in[51]);
  r.direction = mk3(in[52], in[53], in[54]);
  r.isinside = false;
  r.sdepth = 0.0f;
  f3 ip = mk3(out[1], out[2], out[3]), nrm = mk3(out[4], out[5], out[6]);
  out[0] = g.type == 1 ? boxIntersectionTest(g, r, ip, nrm) : sphereIntersectionTest(g, r, ip, nrm);
  out[1] = ip.x;
  out[2] = ip.y;
  out[3] = ip.z;
  out[4] = nrm.x;
  out[5] = nrm.y;
  out[6] = nrm.z;
}

}  // namespace kdpt
