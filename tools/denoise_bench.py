"""What denoising costs, on C3 (cornell + dragon_5, 800 x 800) after 16 iterations with moments on:
   python tools/denoise_bench.py [--rounds 9] [--passes 5] [--iterations 16]
  denoise  kdpt_denoise into device memory with passes = 0 .. --passes, the pass counts alternating inside every
           round (two untimed rounds first: the buffers, every kernel once); the device times kdpt_denoise_stats
           reports (hipEvents on the context's stream), median of --rounds each.  guide_ms: the pinhole rays, their
           traversal and hit records.  filter_ms[k]: packing, k passes and the copy out, so pass k alone (step 1 << k)
           is the median over the rounds of filter_ms[k + 1] - filter_ms[k], and filter_ms[0] is what packing and
           unpacking cost.  Per pass the kernel must move 64 unique bytes per pixel (three 16-byte records read, one
           written); that over the pass's time is set against HBM's 8.0 TB/s peak and the 6.29 TB/s a float4 copy
           reaches -- a floor, not a claim about where the bytes come from: the whole working set (31 MB) fits the
           256 MB Infinity Cache, and the 25 taps of a pixel are served from L2 or LDS.
  render   the same context's kdpt_trace_iterations(pipeline 8, batch 16) of 128 iterations, moments on, wall time
           around enqueue + synchronize, median of 5: the ms per render iteration the denoise times stand beside.
One JSON line per part."""
import argparse
import json
import os
import statistics
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=9)
ap.add_argument("--passes", type=int, default=5)
ap.add_argument("--iterations", type=int, default=16)
ap.add_argument("--device", type=int, default=0)
a = ap.parse_args()
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402  (one HIP runtime, torch's; the outputs live in its tensors)
from kdtreepathtraceroptimization_amd import _build, runtime as kdpt  # noqa: E402
from kdtreepathtraceroptimization_amd.fixtures import load_fixture_scene  # noqa: E402

W = H = 800
HBM_PEAK, HBM_COPY = 8.0e12, 6.29e12  # bytes/s: the spec, and a float4 copy's measured rate
sd = kdpt.SceneData.from_description(load_fixture_scene("cornell", "dragon_5", res=(W, H), depth=8))
dev = torch.device("cuda", a.device)
med = statistics.median

with kdpt.PathTracer(sd, kdpt.default_options(), device=a.device) as pt:
    pt.set_moments(True)
    pt.trace_iterations(1, a.iterations, pipeline=8, batch=16)
    pt.synchronize()
    col = torch.empty((H, W, 3), dtype=torch.float32, device=dev)
    var = torch.empty((H, W), dtype=torch.float32, device=dev)
    torch.cuda.synchronize(dev)
    counts = list(range(a.passes + 1))
    guide, filt = [], {k: [] for k in counts}
    for rnd in range(a.rounds + 2):
        for k in counts:
            pt.denoise_ptr(kdpt.default_denoise_params(passes=k), col.data_ptr(), var.data_ptr())
            st = pt.denoise_stats()
            if rnd >= 2:
                guide.append(st.guide_ms)
                filt[k].append(st.filter_ms)
    per_pass = [med([filt[k + 1][r] - filt[k][r] for r in range(a.rounds)]) for k in range(a.passes)]
    unique = 64 * W * H
    print(json.dumps({
        "part": "denoise", "resolution": [W, H], "samples": a.iterations, "rounds": a.rounds,
        "guide_ms_median": round(med(guide), 4), "guide_ms_min_max": [round(min(guide), 4), round(max(guide), 4)],
        "filter_ms_median_by_passes": [round(med(filt[k]), 4) for k in counts],
        "pack_unpack_ms": round(med(filt[0]), 4),
        "pass_ms": [round(t, 4) for t in per_pass], "pass_step": [1 << k for k in range(a.passes)],
        "unique_bytes_per_pass": unique,
        "pass_fraction_of_hbm_peak": [round(unique / (t * 1e-3) / HBM_PEAK, 4) if t > 0 else None for t in per_pass],
        "pass_fraction_of_hbm_copy": [round(unique / (t * 1e-3) / HBM_COPY, 4) if t > 0 else None for t in per_pass],
        "total_ms_default": round(med(guide) + med(filt[a.passes]), 4),
        "finite": bool(torch.isfinite(col).all().item())}), flush=True)

    n = 128
    times = []
    for rnd in range(6):  # the first round makes the pipeline's states: not timed
        t0 = time.perf_counter()
        pt.trace_iterations(1 + a.iterations + rnd * n, n, pipeline=8, batch=16)
        pt.synchronize()
        if rnd:
            times.append(1e3 * (time.perf_counter() - t0))
    print(json.dumps({"part": "render", "iterations": n, "pipeline": 8, "batch": 16,
                      "ms_per_iteration_median": round(med(times) / n, 4),
                      "wall_ms": [round(t, 3) for t in times]}), flush=True)
    print(json.dumps({"scene": "cornell+dragon_5", "code_object_sha": _build.code_object_sha(kdpt.LIB_PATH)}),
          flush=True)
