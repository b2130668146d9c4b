// kdpt_runtime.hip -- the runtime behind the C ABI (include/kdpt.h).  One HIP translation unit (one hipcc command,
// one code object), and this file is its list of sections in order: the kernels in the kernels_*.h sections, one
// per stage, then the host code in the host_*.h sections, one per feature, each with its own structs, helpers and
// entry points.  No function is defined here.  Scene validation and packing live in kdpt_scene_prep.h and run
// before any device call.
//
// One iteration of the reference's per-sample hot path (src/pathtrace.cu:2405-2635 `pathtrace`), as queued by
// launch_batch for a batch of up to MAXB iterations in lockstep (blockIdx.y / the batch records = iteration):
//   k_gen_geoms_b   : camera rays + bounce 0's analytic geoms and root-box test, which queue the rays that
//                     meet the KD root box (k_gen_rays_b alone on the brute-force / viz routes); a path-traced ray
//                     query (kdpt_trace_rays) starts from the caller's rays instead: k_user_geoms_b / k_user_rays_b,
//                     an adaptive round (kdpt_trace_adaptive) from its list of pixels: k_adapt_geoms_b /
//                     k_adapt_rays_b
//   then per bounce (cap 8, src/pathtrace.cu:2608):
//   k_trace         : the intersect kernel -- KD traversal of the queued rays, persistent waves pulling
//                     64-ray chunks, the tree read from LDS when a record format fits (setup_trace); k_brute /
//                     k_viz instead with enable_kd = 0 / viz_kd
//   k_shade_fused_b : scatterRay + shadeMaterial + partialGather, the stable compaction of the survivors into
//                     the other path buffer (thrust::remove_if; decoupled look-back over the tiles) and the
//                     next bounce's geoms stage and ray queue, in one launch
//   and k_final_gather after the last bounce.
// Iteration 2's stable sort by materialIdHit (thrust::sort), compaction = 0 and the "shade_fused" = 0 knob take
// the three-kernel route instead: k_shade, k_scan, k_scatter (and k_geoms_b where no hand-off prepared the rays).
// No host synchronisation inside an iteration: the live-path count lives on the device and kernels past the
// end of the live range exit at once.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include <dlfcn.h>
#include <rccl/rccl.h>

#include "../../include/kdpt.h"
#include "kdpt_error.h"
#include "kdpt_owned.h"
#include "kdpt_device.h"
#include "kdpt_clusters.h"
#include "kdpt_scene_prep.h"

using namespace kdpt;

// The kernels, one section per stage; the argument structs of a stage's launches live with its kernels.
#include "kernels_gen.h"
#include "kernels_trace.h"
#include "kernels_brute.h"
#include "kernels_shade.h"
#include "kernels_image.h"
#include "kernels_cast.h"
#include "kernels_rays.h"
#include "kernels_selftest.h"
#include "kernels_masks.h"
#include "kernels_frames.h"
#include "kernels_adaptive.h"
#include "kernels_denoise.h"
#include "kernels_temporal.h"
#include "kernels_moments.h"

// The host code, one section per feature; a section uses what the sections before it define.
#include "host_context.h"
#include "host_variants.h"
#include "host_create.h"
#include "host_launch.h"
#include "host_pipeline.h"
#include "host_output.h"
#include "host_frames.h"
#include "host_queries.h"
#include "host_moments.h"
#include "host_denoise.h"
#include "host_temporal.h"
#include "host_group.h"
#include "host_selftest.h"
