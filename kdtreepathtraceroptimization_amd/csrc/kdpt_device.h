// kdpt_device.h -- the per-path bounce of the reference, as __host__ __device__
// functions over the gfx950 data layout (SoA float4 nodes/triangles): the umbrella over its parts.
//
// Follows src/pathtrace.cu:1571-1734 (pathTraceOneBounceKDbare),
// :1023-1235 (traverseKDbareShortHybrid), :881-1020 (traverseKDbare),
// :2304-2369 (shadeMaterial), src/intersections.h and src/interactions.h.
#pragma once

#include "kdpt_scene.h"     // materials, geoms, DevScene, Ray
#include "kdpt_geoms.h"     // analytic geoms, intersectAABB, prep_ray
#include "kdpt_traverse.h"  // the host walk traverseKD and the triangle tests
#include "kdpt_cull.h"      // cluster sizes, cull predicates, half floats, kd_rcp, direction masks
#if defined(__HIPCC__) || defined(__HIP__)
#include "kdpt_wave.h"         // wave primitives
#include "kdpt_trace_phase.h"  // k_trace's wave-cooperative traversal
#endif
#include "kdpt_scatter.h"  // scatterRay, shade
#include "kdpt_glm_kat.h"  // glm known-answer table
#include "kdpt_bounce_kat.h"  // scatterRay / shade / geom tests on known-answer records
