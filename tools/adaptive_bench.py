"""What adaptive sampling saves and costs, on C3 (cornell + dragon_5, 800 x 800):
   python tools/adaptive_bench.py [--target-noise 0.2] [--min-spp 16] [--limit 2048] [--rounds 7]
  stop      the same stopping rule twice, from a reset context with moments on: rounds of pipeline 8 x batch 16
            iterations until kdpt_noise_estimate's mean is <= --target-noise (or --limit iterations) -- uniform
            (kdpt_trace_iterations over every pixel, the estimate from --min-spp on), and adaptive (--min-spp uniform
            iterations, then kdpt_trace_adaptive rounds over the pixels above the same value).  Reported for each:
            pixel-samples, path segments, wall time to the stop (enqueue + synchronize + estimates), the adaptive
            rounds' device time and active fraction, and the final estimate.
  overhead  kdpt_trace_adaptive with the full list (threshold -1, count 16, pipeline 8, batch 16) beside
            kdpt_trace_iterations of 16 iterations on the same context, alternating; wall time around each call
            (+ synchronize), median of --rounds: the list indirection, the scatter and the list build.
One JSON line per part."""
import argparse
import json
import os
import statistics
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--target-noise", type=float, default=0.2)
ap.add_argument("--noise-floor", type=float, default=1e-2)
ap.add_argument("--min-spp", type=int, default=16)
ap.add_argument("--limit", type=int, default=2048)
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--device", type=int, default=0)
a = ap.parse_args()
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from kdtreepathtraceroptimization_amd import _build, runtime as kdpt  # noqa: E402
from kdtreepathtraceroptimization_amd.fixtures import load_fixture_scene  # noqa: E402

W = H = 800
PIPELINE, BATCH = 8, 16
PER_ROUND = PIPELINE * BATCH
sd = kdpt.SceneData.from_description(load_fixture_scene("cornell", "dragon_5", res=(W, H), depth=8))
med = statistics.median


def estimate(pt):
    e = pt.noise_estimate(a.noise_floor, a.target_noise)
    return {"mean": e.mean, "max": e.max, "above": int(e.above), "nonfinite": int(e.nonfinite)}


def uniform_stop(pt):
    pt.reset()
    done, est = 0, None
    t0 = time.perf_counter()
    while done < a.limit:
        n = min(PER_ROUND, a.limit - done)
        pt.trace_iterations(1 + done, n, pipeline=PIPELINE, batch=BATCH)
        pt.synchronize()
        done += n
        if done >= a.min_spp:
            est = estimate(pt)
            if est["mean"] <= a.target_noise:
                break
    wall = 1e3 * (time.perf_counter() - t0)
    return {"part": "stop", "mode": "uniform", "iterations": done, "pixel_samples": done * W * H,
            "segments": int(pt.stats().total_segments), "wall_ms": round(wall, 3), "noise": est}


def adaptive_stop(pt):
    pt.reset()
    t0 = time.perf_counter()
    pt.trace_iterations(1, a.min_spp, pipeline=PIPELINE, batch=BATCH)
    pt.synchronize()
    done, samples, segments, device_ms, rounds = a.min_spp, a.min_spp * W * H, 0, 0.0, []
    while True:
        est = estimate(pt)
        if est["mean"] <= a.target_noise or est["above"] == 0 or done >= a.limit:
            break
        n = min(PER_ROUND, a.limit - done)
        r = pt.trace_adaptive(1 + done, n, pipeline=PIPELINE, batch=BATCH, floor=a.noise_floor,
                              threshold=a.target_noise)
        done += n
        samples += int(r.pixel_samples)
        segments += int(r.segments)
        device_ms += r.device_ms
        rounds.append({"active_fraction": round(r.active / (W * H), 4), "iterations": n,
                       "device_ms": round(r.device_ms, 3), "segments": int(r.segments)})
    wall = 1e3 * (time.perf_counter() - t0)
    counts = pt.sample_counts()
    return {"part": "stop", "mode": "adaptive", "iterations": done, "pixel_samples": samples,
            "segments": int(pt.stats().total_segments) + segments, "wall_ms": round(wall, 3),
            "adaptive_device_ms": round(device_ms, 3), "mean_spp": float(counts.mean()), "max_spp": int(counts.max()),
            "rounds": rounds, "noise": est}


with kdpt.PathTracer(sd, kdpt.default_options(), device=a.device) as pt:
    pt.set_moments(True)
    pt.trace_iterations(1, PER_ROUND, pipeline=PIPELINE, batch=BATCH)  # the pipeline's states, both code paths once:
    pt.trace_adaptive(1 + PER_ROUND, BATCH, pipeline=PIPELINE, batch=BATCH, floor=a.noise_floor, threshold=-1.0)
    u, ad = uniform_stop(pt), adaptive_stop(pt)
    for rec in (u, ad):
        print(json.dumps(rec), flush=True)
    print(json.dumps({"part": "stop", "mode": "ratio", "target_noise": a.target_noise, "noise_floor": a.noise_floor,
                      "min_spp": a.min_spp, "pixel_samples": round(ad["pixel_samples"] / u["pixel_samples"], 4),
                      "segments": round(ad["segments"] / u["segments"], 4),
                      "wall_ms": round(ad["wall_ms"] / u["wall_ms"], 4)}), flush=True)

    pt.reset()
    pt.trace_iterations(1, a.min_spp, pipeline=PIPELINE, batch=BATCH)
    pt.synchronize()
    uni, full, full_dev, it = [], [], [], 1 + a.min_spp
    for rep in range(a.rounds + 1):  # the first round is not timed
        t0 = time.perf_counter()
        pt.trace_iterations(it, BATCH, pipeline=PIPELINE, batch=BATCH)
        pt.synchronize()
        t1 = time.perf_counter()
        r = pt.trace_adaptive(it + BATCH, BATCH, pipeline=PIPELINE, batch=BATCH, floor=a.noise_floor, threshold=-1.0)
        t2 = time.perf_counter()
        it += 2 * BATCH
        assert r.active == W * H
        if rep:
            uni.append(1e3 * (t1 - t0))
            full.append(1e3 * (t2 - t1))
            full_dev.append(r.device_ms)
    print(json.dumps({"part": "overhead", "iterations": BATCH, "pipeline": PIPELINE, "batch": BATCH,
                      "rounds": a.rounds, "trace_iterations_wall_ms_median": round(med(uni), 4),
                      "trace_adaptive_full_wall_ms_median": round(med(full), 4),
                      "trace_adaptive_full_device_ms_median": round(med(full_dev), 4),
                      "ratio": round(med(full) / med(uni), 4),
                      "trace_iterations_wall_ms": [round(t, 4) for t in uni],
                      "trace_adaptive_full_wall_ms": [round(t, 4) for t in full]}), flush=True)
    print(json.dumps({"scene": "cornell+dragon_5", "resolution": [W, H],
                      "code_object_sha": _build.code_object_sha(kdpt.LIB_PATH)}), flush=True)
