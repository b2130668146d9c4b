// kdpt_scatter.h -- the reference's scattering and shading as __host__ __device__ functions
// (src/interactions.h, src/pathtrace.cu:2304-2369 shadeMaterial).
#pragma once

#include "kdpt_scene.h"

namespace kdpt {

// ---------------- src/interactions.h ----------------
KDPT_HD f3 calculateRandomDirectionInHemisphere(f3 normal, Rng& rng) {  // :9-41
  float up = sqrtf(u01(rng));
  float over = sqrtf(1 - up * up);
  float around = u01(rng) * TWO_PI_F;
  f3 dnn;
  if (fabsf(normal.x) < SQRT_OF_ONE_THIRD_F) dnn = mk3(1, 0, 0);
  else if (fabsf(normal.y) < SQRT_OF_ONE_THIRD_F) dnn = mk3(0, 1, 0);
  else dnn = mk3(0, 0, 1);
  f3 p1 = normalize(cross(normal, dnn));
  f3 p2 = normalize(cross(normal, p1));
  float ca = kdpt_cosf(around), sa = kdpt_sinf(around);
  return add(add(scl(normal, up), scl(p1, ca * over)), scl(p2, sa * over));
}
KDPT_HD f3 rotateVector(f3 n1, f3 axis, float angle) {  // :44-65
  axis = normalize(axis);
  float u = axis.x, v = axis.y, w = axis.z, x = n1.x, y = n1.y, z = n1.z;
  float ca = kdpt_cosf(angle), sa = kdpt_sinf(angle);
  float dd = -u * x - v * y - w * z;
  return mk3((-u * dd) * (1 - ca) + x * ca + (-w * y + v * z) * sa,
             (-v * dd) * (1 - ca) + y * ca + (w * x - u * z) * sa,
             (-w * dd) * (1 - ca) + z * ca + (-v * x + u * y) * sa);
}
// :67-83.  theta and phi are float values widened to double; glm::cos/glm::sin on them are glibc's
// double cos/sin and glm::acos(float) is acosf -- all three restated bit-exactly (kdpt_math.h).
// Reached with default flags by any material with transmittance > 0 (e.g. the reference's own
// scenes/stanford_bunny.mtl, Tf 1.0 0.7 0.7) and by the soft lobes when softness > 0.
KDPT_HD f3 randSphericalVec(float angle, Rng& rng) {
  double theta = 2 * PI_F * u01(rng);
  double phi = kdpt_acosf((angle * PI_F * u01(rng) - 1.0f));
  f3 V = mk3((float)(kdpt_cos(theta) * kdpt_sin(phi)), (float)(kdpt_sin(theta) * kdpt_sin(phi)), (float)kdpt_cos(phi));
  return normalize(V);
}
KDPT_HD float getFresnelVal(f3 I, f3 N, float R0) {  // :127-133
  double F = (double)R0 + (double)(1.0f - R0) * pow5((double)(1.0f - dot(N, neg(I))));
  return (float)F;
}
KDPT_HD f3 soft_lobe(f3 dir, Rng& rng) {
  f3 v = randSphericalVec(0.02f, rng);
  float angle = kdpt_acosf(dot(mk3(0.0f, 0.0f, -1.0f), dir));
  f3 axis = normalize(cross(mk3(0.0f, 0.0f, -1.0f), dir));
  return rotateVector(v, axis, angle);
}
// :195-358
KDPT_HD void scatterRay(Ray& ray, f3 intersect, f3 normal, const DevMaterial& m, Rng& rng, float softness) {
  if (m.transmittance[0] > 0.0f || m.transmittance[1] > 0.0f || m.transmittance[2] > 0.0f) {
    float randval = u01(rng);
    if (randval < 0.5f && !ray.isinside) {
      f3 v = randSphericalVec(0.0001f, rng);
      float angle = kdpt_acosf(dot(mk3(0.0f, 0.0f, -1.0f), ray.direction));
      f3 axis = normalize(cross(mk3(0.0f, 0.0f, -1.0f), ray.direction));
      ray.direction = rotateVector(v, axis, angle);
      ray.origin = add(ray.origin, scl(ray.direction, 0.0001f));
      ray.sdepth = distance(ray.origin, intersect);
      ray.isinside = true;
    } else {
      ray.direction = calculateRandomDirectionInHemisphere(normal, rng);
      ray.origin = add(intersect, scl(normal, 0.00001f));
      ray.sdepth = 0.0f;
    }
  } else if (m.hasRefractive != 0.0f) {
    float randval = u01(rng);
    ray.direction = normalize(ray.direction);
    normal = normalize(normal);
    float fresn = getFresnelVal(ray.direction, normal, m.fresnel_R0);
    if (randval < 1.0f - fresn) {
      float ior = m.indexOfRefraction;
      if (!ray.isinside) ior = 1.0f / m.indexOfRefraction;
      double dd = (double)dot(normal, ray.direction);
      float angle = (float)(1.0f - ((double)ior * (double)ior) * (1.0f - dd * dd));
      if (angle < 0.0f) {
        float val = u01(rng);
        if (val < m.hasReflective) {
          ray.direction = reflect(ray.direction, normal);
          if (softness > 0.0f) ray.direction = soft_lobe(ray.direction, rng);
          ray.origin = add(intersect, scl(normal, 0.00001f));
        } else {
          ray.direction = calculateRandomDirectionInHemisphere(normal, rng);
          ray.origin = add(intersect, scl(normal, 0.00001f));
        }
      } else {
        float val = u01(rng);
        if (val < m.hasRefractive) {
          ray.direction = refract(ray.direction, normal, ior);
          if (softness > 0.0f) ray.direction = soft_lobe(ray.direction, rng);
          ray.origin = sub(intersect, scl(normal, 0.001f));
          ray.isinside = !ray.isinside;
        } else {
          ray.direction = calculateRandomDirectionInHemisphere(normal, rng);
          ray.origin = add(intersect, scl(normal, 0.00001f));
        }
      }
    } else {
      ray.direction = reflect(ray.direction, normal);
      ray.origin = add(intersect, scl(normal, 0.00001f));
      ray.isinside = false;
    }
  } else if (m.hasReflective != 0.0f) {
    float randval = u01(rng);
    if (randval < m.hasReflective) {
      ray.direction = reflect(ray.direction, normal);
      if (softness > 0.0f) ray.direction = soft_lobe(ray.direction, rng);
      ray.origin = add(intersect, scl(normal, 0.0001f));
      ray.isinside = false;
    } else {
      ray.direction = calculateRandomDirectionInHemisphere(normal, rng);
      ray.origin = add(intersect, scl(normal, 0.00001f));
    }
  } else {
    ray.direction = calculateRandomDirectionInHemisphere(normal, rng);
    ray.origin = add(intersect, scl(normal, 0.00001f));
    ray.isinside = false;
  }
}

// shadeMaterial body for a path with remainingBounces > 0 (src/pathtrace.cu:2318-2366)
KDPT_HD void shade(float t, int materialId, const DevMaterial* mats, bool enablesss, const Ray& ray, f3& color,
                   int& bounces) {
  if (t > 0.0f) {
    const DevMaterial& m = mats[materialId];
    f3 c = mk3(m.color[0], m.color[1], m.color[2]);
    f3 spec = mk3(m.spec_color[0], m.spec_color[1], m.spec_color[2]);
    if (m.emittance > 0.0f) {
      color = mul(color, scl(c, m.emittance));
      bounces = 0;
    } else {
      if (enablesss && (m.transmittance[0] > 0.0f || m.transmittance[1] > 0.0f || m.transmittance[2] > 0.0f)) {
        float scenescale = 1.0f;
        float sss = (double)(scenescale * ray.sdepth) > 1.0 ? 1.0f : ray.sdepth;
        sss = (double)(1.0f - sss) < 0.0 ? 0.0f : sss;
        sss = (float)((double)sss * (double)sss);
        f3 tr = mk3(m.transmittance[0], m.transmittance[1], m.transmittance[2]);
        color = mul(color, add(add(scl(c, 1.0f), scl(spec, m.hasRefractive)), scl(tr, sss)));
      } else if (m.hasRefractive > 0.0f) {
        color = mul(color, add(scl(c, 1.0f), scl(spec, m.hasRefractive)));
      } else if (m.hasReflective > 0.0f) {
        color = mul(color, add(scl(c, 1.0f), scl(spec, m.hasReflective)));
      } else {
        color = mul(color, scl(c, 1.0f));
      }
      bounces--;
    }
  } else {
    color = mk3(0.0f, 0.0f, 0.0f);
    bounces = 0;
  }
}

}  // namespace kdpt
