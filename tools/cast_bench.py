"""Throughput of ray queries (kdpt_cast_rays) on C3 (cornell + dragon_5) with device-resident inputs and outputs:

  camera   the 800 x 800 un-jittered camera rays (coherent)
  bounce1  the live rays after bounce 1 of iteration 1, from kdpt_debug_paths (what the path tracer traces next)
  bounce3  ... after bounce 3 (fewer, and as incoherent as the path tracer's rays get)
  random   uniformly random origins and unit directions inside the room

  radiance the device's own 800 x 800 camera rays of iteration 1 path traced by one kdpt_trace_rays(count = 16), next
           to 16 kdpt_trace_iteration calls on the same context (cacherays = 1: both legs trace those rays, and the
           line says whether the two images are bit-equal): wall and device ms of each leg

One JSON line per set: rays, the share that reached the KD traversal, the best and median wall time of --reps
synchronous calls (host clock around kdpt_cast_rays, which returns with the records written), rays per second
from the median, and kdpt_cast_stats' device time of the last call; then a line with the library's code-object
hash.  Sets no target: it records what the path does.

    python tools/cast_bench.py [--reps 7] [--random 1000000] [--chunk N] [--bare]
"""
import argparse
import json
import os
import statistics
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--random", type=int, default=1_000_000, help="rays of the random set")
ap.add_argument("--chunk", type=int, default=None, help="knob cast_chunk (default: the library's, 1 << 20)")
ap.add_argument("--bare", action="store_true", help="traverseKDbare instead of the short-stack hybrid")
ap.add_argument("--device", type=int, default=0)
a = ap.parse_args()
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402  (one HIP runtime, torch's; the inputs live in its tensors)
from kdtreepathtraceroptimization_amd import _build, runtime as kdpt  # noqa: E402
from kdtreepathtraceroptimization_amd.cast_cli import camera_rays  # noqa: E402
from kdtreepathtraceroptimization_amd.fixtures import load_fixture_scene  # noqa: E402

sd = kdpt.SceneData.from_description(load_fixture_scene("cornell", "dragon_5", res=(800, 800), depth=8))
dev = torch.device("cuda", a.device)
with kdpt.PathTracer(sd, kdpt.default_options(short_stack=0 if a.bare else 1), device=a.device) as pt:
    if a.chunk:
        pt.set_tuning("cast_chunk", a.chunk)
    sets = {"camera": camera_rays(sd.camera_bytes())}
    for depth in (1, 3):
        p = pt.debug_paths(1, depth)
        p = p[p["remainingBounces"] > 0]
        sets[f"bounce{depth}"] = (np.ascontiguousarray(p["origin"]), np.ascontiguousarray(p["direction"]))
    rs = np.random.RandomState(7)
    d = rs.normal(size=(a.random, 3))
    d /= np.sqrt(np.sum(d * d, axis=1))[:, None]
    sets["random"] = (rs.uniform([-4.95, 0.05, -4.95], [4.95, 9.95, 4.95], (a.random, 3)).astype(np.float32),
                      d.astype(np.float32))
    cfg = pt.trace_config()
    for name, (o, d) in sets.items():
        n = len(o)
        to, td = torch.from_numpy(np.ascontiguousarray(o)).to(dev), torch.from_numpy(np.ascontiguousarray(d)).to(dev)
        out = torch.empty(n * kdpt.RAY_HIT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize(dev)
        times = []
        traced0 = pt.cast_stats().traced
        for rep in range(a.reps + 1):  # the first call allocates the query's buffers: not timed
            t0 = time.perf_counter()
            pt.cast_rays_ptr(to.data_ptr(), td.data_ptr(), n, out.data_ptr(), normalize=True)
            if rep:
                times.append(time.perf_counter() - t0)
        st = pt.cast_stats()
        hits = np.frombuffer(out.cpu().numpy().tobytes(), dtype=kdpt.RAY_HIT_DTYPE)
        med = statistics.median(times)
        print(json.dumps({"set": name, "rays": n, "traced_share": round((st.traced - traced0) / (a.reps + 1) / n, 4),
                          "kinds": {k: int(np.sum(hits["kind"] == v)) for k, v in
                                    (("invalid", -1), ("none", 0), ("geom", 1), ("triangle", 2))},
                          "wall_ms_best": round(1e3 * min(times), 4), "wall_ms_median": round(1e3 * med, 4),
                          "mrays_per_s": round(n / med / 1e6, 1), "device_ms_last": round(st.device_ms, 4)}),
              flush=True)
    # The radiance set: the render's own 800 x 800 camera rays of iteration 1 (cacherays, so that every iteration
    # of both legs traces them) through one kdpt_trace_rays(count = 16), next to 16 kdpt_trace_iteration calls --
    # the same launches behind another bounce-0 kernel, plus the query's 24 bytes in and 12 out per ray.  Wall: the
    # host clock around the synchronous calls; device: kdpt_trace_rays_stats / the sum of ms_last_iteration.
    spp = 16
    pt.set_options(kdpt.default_options(short_stack=0 if a.bare else 1, cacherays=1))
    n = 800 * 800
    to = torch.empty((n, 3), dtype=torch.float32, device=dev)
    td = torch.empty((n, 3), dtype=torch.float32, device=dev)
    rad = torch.empty((n, 3), dtype=torch.float32, device=dev)
    torch.cuda.synchronize(dev)
    pt.camera_rays_ptr(1, to.data_ptr(), td.data_ptr())
    legs = {"query": [], "solo": []}
    for rep in range(a.reps + 1):  # the first round allocates the query's state: not timed
        t0 = time.perf_counter()
        pt.trace_rays_ptr(to.data_ptr(), td.data_ptr(), n, rad.data_ptr(), first_iter=1, count=spp, normalize=False)
        t1 = time.perf_counter()
        q_dev = pt.trace_rays_stats().device_ms
        pt.reset()
        t2 = time.perf_counter()
        for it in range(1, spp + 1):
            pt.trace_iteration(it)
        t3 = time.perf_counter() - t2
        pt.reset()
        s_dev = 0.0
        for it in range(1, spp + 1):  # (again for the device times: reading the stats is not part of the wall time)
            pt.trace_iteration(it)
            s_dev += pt.stats().ms_last_iteration
        if rep:
            legs["query"].append((t1 - t0, q_dev))
            legs["solo"].append((t3, s_dev))
    same = bool(np.array_equal(rad.cpu().numpy().view(np.uint32).reshape(-1), pt.image().view(np.uint32).reshape(-1)))
    print(json.dumps({"set": "radiance", "rays": n, "iterations": spp, "query_equals_solo_image": same,
                      **{f"{leg}_{what}_ms_{stat}": round(f([1e3 * t[0] if k == 0 else t[1] for t in ts]), 4)
                         for leg, ts in legs.items() for k, what in enumerate(("wall", "device"))
                         for stat, f in (("best", min), ("median", statistics.median))}}), flush=True)
    print(json.dumps({"scene": "cornell+dragon_5", "tree": cfg["tree"], "cull_exact": cfg.get("cull_exact"),
                      "short_stack": 0 if a.bare else 1, "chunk": a.chunk or (1 << 20), "reps": a.reps,
                      "code_object_sha": _build.code_object_sha(kdpt.LIB_PATH)}), flush=True)
