// kdpt_glm_kat.h -- known answers for the glm pieces on the path (kernels_selftest.h runs the table on gfx950,
// tests/native/glm_host.cpp on the host).
#pragma once

#include "kdpt_traverse.h"

namespace kdpt {

// Known answers for the glm pieces on the path, checked against the reference's vendored glm 0.9.6.3
// (oracle/ref) on the host and on gfx950 (kdpt_selftest_glm):
//   fn 0 intersectRayTriangle (gtx/intersect.inl:37-74) as tri_test_v runs it: in o, d, v0, v1, v2 (15
//        floats), out {passed, bary.x, bary.y, bary.z}; bary slots the test does not reach keep the
//        caller's values (out[1..3] are read first), which pins glm's partial writes;
//   fn 1 normalize (3 -> 3), fn 2 reflect (I, N -> 3), fn 3 refract (I, N, eta -> 3),
//   fn 4 glm::rotate(quat, vec3) (w, x, y, z, v -> 3).
KDPT_HD int glm_kat_inputs(int fn) {
  return fn == 0 ? 15 : fn == 1 ? 3 : fn == 2 ? 6 : fn == 3 ? 7 : fn == 4 ? 7 : 0;
}
KDPT_HD int glm_kat_outputs(int fn) { return fn == 0 ? 4 : (fn >= 1 && fn <= 4) ? 3 : 0; }
KDPT_HD void glm_kat(int fn, const float* in, float* out) {
  f3 r = mk3(0.0f, 0.0f, 0.0f);
  switch (fn) {
    case 0: {
      const TriData T{make_float4(in[6], in[7], in[8], 0.0f),
                      make_float4(in[9] - in[6], in[10] - in[7], in[11] - in[8], 0.0f),
                      make_float4(in[12] - in[6], in[13] - in[7], in[14] - in[8], 0.0f)};
      float bx = out[1], by = out[2], bz = out[3];
      const int k = tri_test_v(T, mk3(in[0], in[1], in[2]), mk3(in[3], in[4], in[5]), bx, by, bz);
      out[0] = k == 2 ? 1.0f : 0.0f;
      out[1] = bx;
      out[2] = by;
      out[3] = bz;
      return;
    }
    case 1: r = normalize(mk3(in[0], in[1], in[2])); break;
    case 2: r = reflect(mk3(in[0], in[1], in[2]), mk3(in[3], in[4], in[5])); break;
    case 3: r = refract(mk3(in[0], in[1], in[2]), mk3(in[3], in[4], in[5]), in[6]); break;
    case 4: r = quat_rotate(in[0], mk3(in[1], in[2], in[3]), mk3(in[4], in[5], in[6])); break;
    default: return;
  }
  out[0] = r.x;
  out[1] = r.y;
  out[2] = r.z;
}

}  // namespace kdpt
