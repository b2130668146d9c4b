"""What the persistent render group saves and costs, on C3 (cornell + dragon_5, 800 x 800), with every rank on one
device (the copy reduce; so nothing here says anything about xGMI or scaling):
   python tools/group_bench.py [--ranks 2] [--frames 4] [--spp 128] [--rounds 5]
  create    kdpt_render_sharded per call (create the contexts, render, destroy) beside kdpt_group_render_frames +
            kdpt_group_synchronize on a live group, for the same frames, alternating; wall time around each, median
            of --rounds.  The difference is the create cost the group amortises.
  moments   a KDPT_GROUP_MOMENTS group beside a moments-off group for the same frames, alternating, the same way:
            6 W H floats per frame buffer and reduce instead of 3 W H, k_frame_moments instead of k_sum_frames +
            k_accumulate_batch + the copy.
  adaptive  one adaptive round of a one-rank group (kdpt_group_trace_adaptive) beside kdpt_trace_adaptive on a single
            context with the same list (both states are the same 16 uniform iterations; threshold = the median noise),
            count 16, pipeline 8, batch 16, alternating; wall and device time, median of --rounds.
One JSON line per part."""
import argparse
import json
import os
import statistics
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--ranks", type=int, default=2)
ap.add_argument("--frames", type=int, default=4)
ap.add_argument("--spp", type=int, default=128)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--device", type=int, default=0)
a = ap.parse_args()
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from kdtreepathtraceroptimization_amd import _build, runtime as kdpt  # noqa: E402
from kdtreepathtraceroptimization_amd.fixtures import load_fixture_scene  # noqa: E402

W = H = 800
PIPELINE, BATCH = 8, 16
FLOOR = 1e-2
sd = kdpt.SceneData.from_description(load_fixture_scene("cornell", "dragon_5", res=(W, H), depth=8))
med = statistics.median
devices = [a.device] * a.ranks


def ms(fn):
    t0 = time.perf_counter()
    fn()
    return 1e3 * (time.perf_counter() - t0)


def frames_on(grp, first):
    grp.render_frames(first, a.frames, a.spp, pipeline=PIPELINE, batch=BATCH)
    grp.synchronize()


# ---- create: the sharded call beside a live group
with kdpt.RenderGroup(sd, devices, reduce=kdpt.REDUCE_COPY) as grp:
    frames_on(grp, 0)  # the pipeline's states
    sharded, live = [], []
    for rep in range(a.rounds + 1):  # the first round is not timed
        t_s = ms(lambda: kdpt.render_sharded(sd, devices, 0, a.frames, a.spp, pipeline=PIPELINE, batch=BATCH,
                                             reduce=kdpt.REDUCE_COPY))
        t_l = ms(lambda: frames_on(grp, (rep + 1) * a.frames))
        if rep:
            sharded.append(t_s)
            live.append(t_l)
    create_ms = [grp.context(r).stats().create_ms for r in range(a.ranks)]
print(json.dumps({"part": "create", "ranks": a.ranks, "frames": a.frames, "spp": a.spp, "rounds": a.rounds,
                  "render_sharded_wall_ms_median": round(med(sharded), 3),
                  "group_frames_wall_ms_median": round(med(live), 3),
                  "difference_ms": round(med(sharded) - med(live), 3),
                  "context_create_ms": [round(v, 3) for v in create_ms],
                  "render_sharded_wall_ms": [round(t, 3) for t in sharded],
                  "group_frames_wall_ms": [round(t, 3) for t in live]}), flush=True)

# ---- moments: a moments-on group beside a moments-off one
with kdpt.RenderGroup(sd, devices, reduce=kdpt.REDUCE_COPY) as off, \
        kdpt.RenderGroup(sd, devices, reduce=kdpt.REDUCE_COPY, moments=True) as on:
    frames_on(off, 0)
    frames_on(on, 0)
    t_off, t_on = [], []
    for rep in range(a.rounds):
        t_off.append(ms(lambda: frames_on(off, (rep + 1) * a.frames)))
        t_on.append(ms(lambda: frames_on(on, (rep + 1) * a.frames)))
    same = bool(np.array_equal(on.context(0).image().view(np.uint32), off.context(0).image().view(np.uint32)))
print(json.dumps({"part": "moments", "ranks": a.ranks, "frames": a.frames, "spp": a.spp, "rounds": a.rounds,
                  "moments_off_wall_ms_median": round(med(t_off), 3), "moments_on_wall_ms_median": round(med(t_on), 3),
                  "ratio": round(med(t_on) / med(t_off), 4), "image_bits_equal": same,
                  "moments_off_wall_ms": [round(t, 3) for t in t_off],
                  "moments_on_wall_ms": [round(t, 3) for t in t_on]}), flush=True)

# ---- adaptive: a one-rank group's round beside the single context's, the same list
with kdpt.RenderGroup(sd, [a.device], reduce=kdpt.REDUCE_COPY, moments=True) as grp, \
        kdpt.PathTracer(sd, kdpt.default_options(), device=a.device) as pt:
    pt.set_moments(True)
    g_wall, g_dev, s_wall, s_dev, active = [], [], [], [], None
    for rep in range(a.rounds + 1):  # the first round is not timed; every round starts from the same 16 iterations
        grp.reset()
        pt.reset()
        grp.render_frames(0, 1, BATCH, pipeline=PIPELINE, batch=BATCH)
        grp.synchronize()
        pt.trace_iterations(1, BATCH, pipeline=PIPELINE, batch=BATCH)
        pt.synchronize()
        thr = float(np.median(pt.noise_map(FLOOR)))
        rec = {}
        t_g = ms(lambda: rec.update(g=grp.trace_adaptive(1 + BATCH, BATCH, pipeline=PIPELINE, batch=BATCH, floor=FLOOR,
                                                         threshold=thr)))
        t_s = ms(lambda: rec.update(s=pt.trace_adaptive(1 + BATCH, BATCH, pipeline=PIPELINE, batch=BATCH, floor=FLOOR,
                                                        threshold=thr)))
        same_list = rec["g"].active == rec["s"].active and rec["g"].segments == rec["s"].segments
        active = int(rec["g"].active)
        if rep:
            g_wall.append(t_g)
            s_wall.append(t_s)
            g_dev.append(rec["g"].device_ms)
            s_dev.append(rec["s"].device_ms)
print(json.dumps({"part": "adaptive", "count": BATCH, "pipeline": PIPELINE, "batch": BATCH, "rounds": a.rounds,
                  "active_fraction": round(active / (W * H), 4), "same_list_and_segments": bool(same_list),
                  "group_wall_ms_median": round(med(g_wall), 3), "single_wall_ms_median": round(med(s_wall), 3),
                  "group_device_ms_median": round(med(g_dev), 3), "single_device_ms_median": round(med(s_dev), 3),
                  "ratio_wall": round(med(g_wall) / med(s_wall), 4),
                  "group_wall_ms": [round(t, 3) for t in g_wall],
                  "single_wall_ms": [round(t, 3) for t in s_wall]}), flush=True)
print(json.dumps({"scene": "cornell+dragon_5", "resolution": [W, H],
                  "code_object_sha": _build.code_object_sha(kdpt.LIB_PATH)}), flush=True)
