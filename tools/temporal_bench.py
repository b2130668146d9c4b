"""What temporal accumulation costs, on C3 (cornell + dragon_5, 800 x 800) along a camera path:
   python tools/temporal_bench.py [--rounds 9] [--spp 4] [--degrees 1.0]
  temporal  every round is one frame of the path -- the camera orbits by --degrees, kdpt_set_camera, kdpt_reset,
            --spp iterations with moments on -- then kdpt_denoise_temporal into device memory with the default
            parameters (two untimed rounds first: the buffers, every kernel once, a history to reproject); the device
            times kdpt_temporal_stats reports (hipEvents on the context's stream), median of --rounds each.
            guide_ms: the pinhole rays, their traversal and hit records.  temporal_ms: k_denoise_pack_render and
            k_temporal.  filter_ms: the five passes and the copy out.  Unique bytes per pixel of temporal_ms' two
            kernels: packing reads 64 (image 12, sumsq 12, the hit record 40) and writes 48 (three records);
            k_temporal reads 48 (the frame's records) and the history's 52 (four taps per pixel, but for a small move
            every history pixel is some pixel's tap about once: the rest is reuse in L2), and writes 20 (C', V', L').
            232 bytes per pixel over temporal_ms is set against HBM's 8.0 TB/s peak and the 6.29 TB/s a float4 copy
            reaches -- a floor, not a claim about where the bytes come from: the working set fits the Infinity Cache.
  render    the same context's kdpt_trace_iterations(pipeline 8, batch 16) of 128 iterations, moments on, wall time
            around enqueue + synchronize, median of 5: the ms per render iteration the stage's times stand beside.
One JSON line per part."""
import argparse
import json
import os
import statistics
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=9)
ap.add_argument("--spp", type=int, default=4)
ap.add_argument("--degrees", type=float, default=1.0)
ap.add_argument("--device", type=int, default=0)
a = ap.parse_args()
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402  (one HIP runtime, torch's; the outputs live in its tensors)
from kdtreepathtraceroptimization_amd import _build, runtime as kdpt  # noqa: E402
from kdtreepathtraceroptimization_amd.fixtures import load_fixture_scene  # noqa: E402

W = H = 800
HBM_PEAK, HBM_COPY = 8.0e12, 6.29e12  # bytes/s: the spec, and a float4 copy's measured rate
PACK_BYTES, STAGE_BYTES = 64 + 48, 48 + 52 + 20
sd = kdpt.SceneData.from_description(load_fixture_scene("cornell", "dragon_5", res=(W, H), depth=8))
dev = torch.device("cuda", a.device)
med = statistics.median

with kdpt.PathTracer(sd, kdpt.default_options(), device=a.device) as pt:
    pt.set_moments(True)
    col = torch.empty((H, W, 3), dtype=torch.float32, device=dev)
    var = torch.empty((H, W), dtype=torch.float32, device=dev)
    torch.cuda.synchronize(dev)
    cam = sd.view.camera
    rows = []
    for rnd in range(a.rounds + 2):
        cam = kdpt.orbit_camera(cam, a.degrees)
        pt.synchronize()
        pt.set_camera(cam)
        pt.reset()
        pt.trace_iterations(1 + rnd * a.spp, a.spp, pipeline=8, batch=16)  # fresh samples every frame
        pt.synchronize()
        pt.denoise_temporal_ptr(None, None, col.data_ptr(), var.data_ptr())
        st = pt.temporal_stats()
        print(json.dumps({"part": "frame", "round": rnd, "timed": rnd >= 2, "guide_ms": round(st.guide_ms, 4),
                          "temporal_ms": round(st.temporal_ms, 4), "filter_ms": round(st.filter_ms, 4),
                          "valid": st.valid, "with_history": st.with_history}), flush=True)
        if rnd >= 2:
            rows.append(st)
    t_ms = med([r.temporal_ms for r in rows])
    unique = (PACK_BYTES + STAGE_BYTES) * W * H
    print(json.dumps({
        "part": "temporal", "resolution": [W, H], "spp": a.spp, "degrees_per_frame": a.degrees, "rounds": a.rounds,
        "guide_ms_median": round(med([r.guide_ms for r in rows]), 4), "temporal_ms_median": round(t_ms, 4),
        "temporal_ms_min_max": [round(min(r.temporal_ms for r in rows), 4), round(max(r.temporal_ms for r in rows), 4)],
        "filter_ms_median": round(med([r.filter_ms for r in rows]), 4),
        "with_history_fraction_median": round(med([r.with_history / max(1, r.valid) for r in rows]), 4),
        "unique_bytes_per_pixel": {"pack": PACK_BYTES, "k_temporal": STAGE_BYTES},
        "fraction_of_hbm_peak": round(unique / (t_ms * 1e-3) / HBM_PEAK, 4) if t_ms > 0 else None,
        "fraction_of_hbm_copy": round(unique / (t_ms * 1e-3) / HBM_COPY, 4) if t_ms > 0 else None,
        "finite": bool(torch.isfinite(col).all().item())}), flush=True)

    n = 128
    times = []
    for rnd in range(6):  # the first round makes the pipeline's states: not timed
        t0 = time.perf_counter()
        pt.trace_iterations(1 + (a.rounds + 2) * a.spp + rnd * n, n, pipeline=8, batch=16)
        pt.synchronize()
        if rnd:
            times.append(1e3 * (time.perf_counter() - t0))
    print(json.dumps({"part": "render", "iterations": n, "pipeline": 8, "batch": 16,
                      "ms_per_iteration_median": round(med(times) / n, 4),
                      "wall_ms": [round(t, 3) for t in times]}), flush=True)
    print(json.dumps({"scene": "cornell+dragon_5", "code_object_sha": _build.code_object_sha(kdpt.LIB_PATH)}),
          flush=True)
