"""What second moments cost, on C3 (cornell + dragon_5, 800 x 800):
   python tools/moments_bench.py [--rounds 7] [--iterations 128]
  render   kdpt_trace_iterations(pipeline 8, batch 16) of --iterations iterations, moments off and moments on
           alternating in one process and one context (reset between rounds); wall time around enqueue +
           synchronize, median of --rounds each.  With moments on every batch's add reads and writes sumsq beside
           the image: one more read and write of a 7.7 MB buffer per 16 iterations.
  estimate kdpt_noise_estimate and kdpt_noise_map (into device memory) on the last moments-on state: wall time of
           the synchronous calls (launches, kernels, and the 48-byte result's copy), median of 20 -- an upper
           bound of their device time.
  query    kdpt_trace_rays_moments beside kdpt_trace_rays on tools/cast_bench.py's radiance set (the render's own
           camera rays of iteration 1, cacherays, count = 16, device-resident arrays), alternating; the device times
           kdpt_trace_rays_stats reports, median of --rounds each.
One JSON line per part."""
import argparse
import json
import os
import statistics
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--iterations", type=int, default=128)
ap.add_argument("--device", type=int, default=0)
a = ap.parse_args()
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402  (one HIP runtime, torch's; the query's arrays live in its tensors)
from kdtreepathtraceroptimization_amd import _build, runtime as kdpt  # noqa: E402
from kdtreepathtraceroptimization_amd.fixtures import load_fixture_scene  # noqa: E402

W = H = 800
sd = kdpt.SceneData.from_description(load_fixture_scene("cornell", "dragon_5", res=(W, H), depth=8))
dev = torch.device("cuda", a.device)
med = statistics.median


def render_round(pt, on):
    pt.reset()
    pt.set_moments(on)
    t0 = time.perf_counter()
    pt.trace_iterations(1, a.iterations, pipeline=8, batch=16)
    pt.synchronize()
    return 1e3 * (time.perf_counter() - t0)


with kdpt.PathTracer(sd, kdpt.default_options(), device=a.device) as pt:
    render_round(pt, False)  # the pipeline's states, and both code paths once: not timed
    render_round(pt, True)
    off, on = [], []
    for _ in range(a.rounds):
        off.append(render_round(pt, False))
        on.append(render_round(pt, True))
    print(json.dumps({"part": "render", "resolution": [W, H], "iterations": a.iterations, "pipeline": 8, "batch": 16,
                      "rounds": a.rounds, "off_ms_median": round(med(off), 3), "on_ms_median": round(med(on), 3),
                      "off_ms": [round(t, 3) for t in off], "on_ms": [round(t, 3) for t in on],
                      "cost_percent": round(100.0 * (med(on) / med(off) - 1.0), 3)}), flush=True)

    noise = torch.empty(W * H, dtype=torch.float32, device=dev)
    torch.cuda.synchronize(dev)
    est_ms, map_ms = [], []
    for rep in range(21):
        t0 = time.perf_counter()
        est = pt.noise_estimate(1e-2, 0.05)
        t1 = time.perf_counter()
        pt.noise_map(1e-2, out_ptr=noise.data_ptr())
        t2 = time.perf_counter()
        if rep:
            est_ms.append(1e3 * (t1 - t0))
            map_ms.append(1e3 * (t2 - t1))
    print(json.dumps({"part": "estimate", "samples": int(est.samples), "mean": est.mean, "max": est.max,
                      "above_0.05": int(est.above), "nonfinite": int(est.nonfinite),
                      "estimate_wall_ms_median": round(med(est_ms), 4), "estimate_wall_ms_best": round(min(est_ms), 4),
                      "map_wall_ms_median": round(med(map_ms), 4), "map_wall_ms_best": round(min(map_ms), 4)}),
          flush=True)

    pt.reset()
    pt.set_moments(False)
    pt.set_options(kdpt.default_options(cacherays=1))
    n, spp = W * H, 16
    to, td, rad, sq = (torch.empty((n, 3), dtype=torch.float32, device=dev) for _ in range(4))
    torch.cuda.synchronize(dev)
    pt.camera_rays_ptr(1, to.data_ptr(), td.data_ptr())
    plain, moments = [], []
    for rep in range(a.rounds + 1):  # the first round allocates the query's buffers: not timed
        pt.trace_rays_ptr(to.data_ptr(), td.data_ptr(), n, rad.data_ptr(), first_iter=1, count=spp, normalize=False)
        p = pt.trace_rays_stats().device_ms
        want = rad.clone()
        pt.trace_rays_moments_ptr(to.data_ptr(), td.data_ptr(), n, rad.data_ptr(), sq.data_ptr(), first_iter=1,
                                  count=spp, normalize=False)
        m = pt.trace_rays_stats().device_ms
        if rep:
            plain.append(p)
            moments.append(m)
    same = bool(torch.equal(want.view(torch.int32), rad.view(torch.int32)))
    print(json.dumps({"part": "query", "rays": n, "iterations": spp, "radiance_equal": same,
                      "trace_rays_device_ms_median": round(med(plain), 4),
                      "trace_rays_moments_device_ms_median": round(med(moments), 4),
                      "cost_percent": round(100.0 * (med(moments) / med(plain) - 1.0), 3)}), flush=True)
    print(json.dumps({"scene": "cornell+dragon_5", "code_object_sha": _build.code_object_sha(kdpt.LIB_PATH)}),
          flush=True)
