"""Headless command line of the path tracer: the reference's `main(argc, argv)` (src/main.cpp:1013-1038)
without the GLFW window.

    python -m kdtreepathtraceroptimization_amd SCENE.txt [MESH.obj] [options]

The reference loads the scene (and the OBJ with its KD tree), renders ITERATIONS samples per pixel with
the flag state of src/main.cpp:35-60 (changed interactively by the keys of src/main.cpp:1187-1306), then
saveImage()s a PNG (src/main.cpp:1087-1108) and exits (runCuda, src/main.cpp:1110-1185).  Here the flags
are options, the iterations run on the GPU through the C-ABI (kdpt_trace_iterations keeps several in
flight; bit-identical to one pathtrace() call per iteration), and the output is the same PNG (and
optionally the Radiance HDR image::saveHDR writes).  Flag -> reference variable:

    --dof-angle A      dofAngle (0; keys -/=)          --focal F        dofDistance (6; keys [ ])
    --softness S       softness (0; keys 1/2)          --sss            SSS (false)
    --cacherays        rayCaching (false; key C)       --no-aa          antialias = false (key A)
    --no-compaction    COMPACTION = false              --bare           SHORTSTACK = false
    --brute            ENABLEKD = false                --bbox           USEBBOX = true (with --brute)
    --viz-kd           VIZKD = true                    --testing        TESTINGMODE (per-bounce timing)
    --iterations N     the scene's ITERATIONS          --res W H / --depth D   scene overrides

Not in the reference: --target-noise E renders until the image's mean relative standard error (kdpt_noise_estimate
over the per-pixel second moments, --noise-floor F) is <= E, checking after each round of pipeline x batch
iterations from --min-spp N on, with --iterations as the upper limit; --noise-map also writes BASE.noise.npy.  The
PNG / HDR are divided by the samples actually rendered.  Without --target-noise nothing changes.

--adaptive (with --target-noise E) re-traces only the noisy pixels: uniform rounds up to --min-spp, then rounds of
kdpt_trace_adaptive over the pixels whose own noise is above --pixel-noise T (default E) until the mean is <= E, no
pixel is above T or --iterations is reached.  The PNG / HDR then divide each pixel by its own sample count
(kdpt_save_counted).  A pixel whose noise reads 0 after --min-spp samples is never revisited: --min-spp is the guard.

--devices 0,1,... renders on a persistent group of contexts, one per listed device (kdpt_group; --reduce rccl, or copy,
which also lets a device repeat): samples per pixel sharded over the ranks in frames of pipeline x batch x ndev
iterations, the rest of --iterations in shorter frames that keep the iteration numbers.  --target-noise checks rank
0's estimate after every frame, --adaptive switches to kdpt_group_trace_adaptive rounds after --min-spp, and the
output comes from rank 0's context through the same save paths; the JSON gains "devices" and "frames".  Without
--devices nothing changes.

--denoise [PASSES] also writes BASE.denoised.png (BASE.denoised.hdr with --hdr): the per-pixel means through
kdpt_denoise's variance-guided edge-avoiding filter (PASSES a-trous passes, default 5), then saveImage's pixel pass
with samples = 1 (save_pixels).  It keeps second moments while rendering, as --target-noise does, works with --adaptive
(the per-pixel counts are inside the means) and --devices (rank 0's context), and needs at least 2 iterations.

--orbit FRAMES DEGREES renders a camera path: FRAMES views, view f the scene's camera turned about its lookAt point
around its up axis by f * DEGREES / FRAMES (runtime.orbit_camera; view 0 is the scene's own, and 360 degrees close the
turntable), each with --iterations samples of its own after a reset (view f takes the iteration numbers after
view f - 1's, so no two views draw the same samples), written as BASE.fNNNN.png (and .hdr, and with --denoise
BASE.fNNNN.denoised.png / .hdr).  --temporal (with --denoise) denoises each frame with kdpt_denoise_temporal: the
previous frame's result is reprojected into the new view before the filter runs; the history is reset before frame 0,
and every frame prints how many of its valid pixels found history.  Both work with --devices (kdpt_group_set_camera,
kdpt_group_reset; rank 0's context denoises).  Without them nothing changes.
"""
from __future__ import annotations

import argparse
import json
import math
import os
import sys
import time


def scene_header(path: str) -> dict:
    """ITERATIONS and FILE of the scene's CAMERA block (Scene::loadCamera, src/scene.cpp:190-223)."""
    out = {"iterations": None, "file": None}
    with open(path) as f:
        for line in f:
            tok = line.split()
            if len(tok) >= 2 and tok[0] == "ITERATIONS":
                out["iterations"] = int(float(tok[1]))
            elif len(tok) >= 2 and tok[0] == "FILE":
                out["file"] = tok[1]
    return out


def device_list(text: str):
    """--devices: "0,1,2" -> [0, 1, 2] (1 to 8 entries, each >= 0)."""
    try:
        devs = [int(t) for t in text.split(",")]
    except ValueError:
        raise argparse.ArgumentTypeError(f"not a comma-separated list of device numbers: {text!r}")
    if not 1 <= len(devs) <= 8 or min(devs) < 0:
        raise argparse.ArgumentTypeError("1 to 8 device numbers, each >= 0")
    return devs


def parse_args(argv=None) -> argparse.Namespace:
    ap = argparse.ArgumentParser(prog="python -m kdtreepathtraceroptimization_amd",
                                 description="Headless KD-tree path tracer on MI355X (reference: src/main.cpp).")
    ap.add_argument("scene", help="scene text file (scenes/*.txt)")
    ap.add_argument("mesh", nargs="?", default=None, help="optional OBJ mesh (KD tree built on the host)")
    ap.add_argument("--iterations", "--spp", type=int, default=None, help="samples per pixel (default: ITERATIONS)")
    ap.add_argument("--res", type=int, nargs=2, default=None, metavar=("W", "H"))
    ap.add_argument("--depth", type=int, default=None, help="traceDepth override")
    ap.add_argument("--bounce-cap", type=int, default=8, help="bounces per iteration (reference: 8)")
    ap.add_argument("--dof-angle", type=float, default=0.0)
    ap.add_argument("--focal", type=float, default=6.0)
    ap.add_argument("--softness", type=float, default=0.0)
    ap.add_argument("--sss", action="store_true")
    ap.add_argument("--cacherays", action="store_true")
    ap.add_argument("--no-aa", action="store_true")
    ap.add_argument("--no-compaction", action="store_true")
    ap.add_argument("--bare", action="store_true", help="traverseKDbare instead of the short-stack hybrid")
    ap.add_argument("--brute", action="store_true", help="no KD tree: every OBJ triangle (pathTraceOneBounce)")
    ap.add_argument("--bbox", action="store_true", help="brute force: each shape's bbox test first")
    ap.add_argument("--viz-kd", action="store_true", help="draw the KD node boxes")
    ap.add_argument("--testing", action="store_true", help="TESTINGMODE: time the intersect kernel per bounce")
    ap.add_argument("--first-iteration", type=int, default=1, help="first (1-based) iteration number")
    ap.add_argument("--out", default=None, help="output base name (default: the scene's FILE + samples)")
    ap.add_argument("--no-png", action="store_true")
    ap.add_argument("--hdr", action="store_true", help="also write BASE.hdr (image::saveHDR)")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--pipeline", type=int, default=8, help="batches in flight (throughput only)")
    ap.add_argument("--batch", type=int, default=16,
                    help="iterations sharing an intersect launch (<= 16, MAXB); 8 x 16 is bench.py's shape")
    ap.add_argument("--kd-build", choices=["gpu", "host"], default="gpu",
                    help="build the KD tree on the GPU (default; byte-identical) or with the host recursion")
    ap.add_argument("--dry-run", action="store_true", help="load and build the scene, print it, render nothing")
    ap.add_argument("--target-noise", type=float, default=None, metavar="E",
                    help="adaptive stop: render in rounds of pipeline x batch iterations and stop once the mean "
                         "relative standard error of the pixel means (kdpt_noise_estimate) is <= E; --iterations "
                         "becomes the upper limit")
    ap.add_argument("--noise-floor", type=float, default=1e-2, metavar="F",
                    help="the noise estimate's floor on the pixel mean (default 1e-2)")
    ap.add_argument("--min-spp", type=int, default=2, metavar="N",
                    help="with --target-noise: no estimate before N samples per pixel (at least 2)")
    ap.add_argument("--noise-map", action="store_true",
                    help="with --target-noise: also write BASE.noise.npy (H x W float32, kdpt_noise_map)")
    ap.add_argument("--adaptive", action="store_true",
                    help="with --target-noise: after --min-spp uniform samples re-trace only the pixels whose noise "
                         "is above --pixel-noise (kdpt_trace_adaptive)")
    ap.add_argument("--pixel-noise", type=float, default=None, metavar="T",
                    help="with --adaptive: a pixel goes again while its noise is above T (default: E)")
    ap.add_argument("--devices", type=device_list, default=None, metavar="0,1,...",
                    help="render on a persistent group of contexts, one per listed device (kdpt_group): samples per "
                         "pixel sharded over them in frames of pipeline x batch x ndev iterations")
    ap.add_argument("--reduce", choices=["rccl", "copy"], default="rccl",
                    help="with --devices: the frames' cross-rank reduce (copy: peer copies to the first device, which "
                         "also lets a device repeat)")
    ap.add_argument("--denoise", type=int, nargs="?", const=5, default=None, metavar="PASSES",
                    help="also write BASE.denoised.png (and BASE.denoised.hdr with --hdr): the per-pixel means through "
                         "the variance-guided edge-avoiding filter (kdpt_denoise), PASSES a-trous passes (0 .. 8, "
                         "default 5); keeps second moments while rendering and needs at least 2 iterations")
    ap.add_argument("--orbit", nargs=2, default=None, metavar=("FRAMES", "DEGREES"),
                    help="render FRAMES views, view f turned about the camera's lookAt point around its up axis by "
                         "f * DEGREES / FRAMES, each with --iterations samples after a reset; writes BASE.fNNNN.png "
                         "(with --denoise also BASE.fNNNN.denoised.png)")
    ap.add_argument("--temporal", action="store_true",
                    help="with --denoise: denoise each frame with kdpt_denoise_temporal (the previous frame's result "
                         "reprojected into the new view first) and print each frame's with_history / valid")
    a = ap.parse_args(argv)
    if a.orbit is not None:
        try:
            a.orbit = (int(a.orbit[0]), float(a.orbit[1]))
        except ValueError:
            ap.error("--orbit: FRAMES must be an integer and DEGREES a number")
        if a.orbit[0] < 1 or not math.isfinite(a.orbit[1]):
            ap.error("--orbit: FRAMES must be >= 1 and DEGREES finite")
        if a.target_noise is not None or a.adaptive or a.testing:
            ap.error("--orbit renders a fixed number of samples per view; it cannot be combined with --target-noise, "
                     "--adaptive or --testing")
    if a.temporal and a.denoise is None:
        ap.error("--temporal needs --denoise")
    if a.denoise is not None:
        if not 0 <= a.denoise <= 8:
            ap.error("--denoise: PASSES must be in 0 .. 8")
        if a.brute or a.viz_kd:
            ap.error("--denoise takes its guides from the KD traversal; it cannot be combined with --brute or --viz-kd")
    if a.devices is not None:
        if a.testing:
            ap.error("--devices renders in pipelined frames; it cannot be combined with --testing")
        if a.first_iteration != 1:
            ap.error("--devices numbers its frames' iterations from 1; --first-iteration cannot be combined with it")
    if a.adaptive and a.target_noise is None:
        ap.error("--adaptive needs --target-noise")
    if a.pixel_noise is not None and not a.adaptive:
        ap.error("--pixel-noise needs --adaptive")
    if a.pixel_noise is not None and not a.pixel_noise >= 0:
        ap.error("--pixel-noise must be >= 0")
    if a.target_noise is None and a.noise_map:
        ap.error("--noise-map needs --target-noise")
    if a.target_noise is not None:
        if not a.target_noise >= 0:
            ap.error("--target-noise must be >= 0")
        if not (a.noise_floor > 0 and a.noise_floor < float("inf")):
            ap.error("--noise-floor must be finite and > 0")
        if a.min_spp < 2:
            ap.error("--min-spp must be >= 2 (a variance needs two samples)")
        if a.testing:
            ap.error("--target-noise renders in pipelined rounds; it cannot be combined with --testing")
    return a


def options_from_args(a: argparse.Namespace):
    from .runtime import default_options
    return default_options(focal_length=a.focal, dof_angle=a.dof_angle, softness=a.softness,
                           cacherays=int(a.cacherays), antialias=0 if a.no_aa else 1, enable_sss=int(a.sss),
                           testing_mode=int(a.testing), compaction=0 if a.no_compaction else 1,
                           enable_kd=0 if a.brute else 1, viz_kd=int(a.viz_kd), use_bbox=int(a.bbox),
                           short_stack=0 if a.bare else 1, bounce_cap=a.bounce_cap)


def render_to_noise(pt, a: argparse.Namespace, limit: int):
    """--target-noise E: rounds of pipeline x batch iterations (one full pipeline each), with second moments on;
    after every round from --min-spp on, kdpt_noise_estimate, and the render stops once its mean is <= E or `limit`
    iterations are done.  Returns the samples per pixel rendered and the last estimate (None: fewer than --min-spp
    were allowed)."""
    pt.set_moments(True)
    per_round = max(1, min(16, a.pipeline)) * max(1, min(16, a.batch))
    done, est = 0, None
    while done < limit:
        n = min(per_round, limit - done)
        pt.trace_iterations(a.first_iteration + done, n, pipeline=a.pipeline, batch=a.batch)
        pt.synchronize()
        done += n
        if done >= a.min_spp:
            est = pt.noise_estimate(a.noise_floor, a.target_noise)
            if est.mean <= a.target_noise:
                break
    return done, est


def render_adaptive(pt, a: argparse.Namespace, limit: int):
    """--adaptive: uniform rounds up to --min-spp samples per pixel, then, while the estimate's mean is above E, a
    pixel is above T and fewer than `limit` iterations are done, one kdpt_trace_adaptive round of (at most) pipeline x
    batch iterations over the pixels above T, continuing the iteration numbers.  Returns the iterations done (the
    largest per-pixel count), the last estimate and the adaptive rounds' totals."""
    pt.set_moments(True)
    thr = a.target_noise if a.pixel_noise is None else a.pixel_noise
    per_round = max(1, min(16, a.pipeline)) * max(1, min(16, a.batch))
    done, est = 0, None
    totals = {"pixel_samples": 0, "segments": 0, "rounds": []}
    uniform = min(a.min_spp, limit)
    while done < uniform:
        n = min(per_round, uniform - done)
        pt.trace_iterations(a.first_iteration + done, n, pipeline=a.pipeline, batch=a.batch)
        pt.synchronize()
        done += n
    totals["pixel_samples"] = done * pt.width * pt.height
    while done >= 2:
        est = pt.noise_estimate(a.noise_floor, thr)
        if est.mean <= a.target_noise or est.above == 0 or done >= limit:
            break
        n = min(per_round, limit - done)
        r = pt.trace_adaptive(a.first_iteration + done, n, pipeline=a.pipeline, batch=a.batch, floor=a.noise_floor,
                              threshold=thr)
        done += n
        totals["pixel_samples"] += int(r.pixel_samples)
        totals["segments"] += int(r.segments)
        totals["rounds"].append({"active": int(r.active), "iterations": n, "device_ms": round(r.device_ms, 4)})
    return done, est, totals


def frame_plan(done: int, limit: int, per_frame: int):
    """The next kdpt_group_render_frames call after `done` iterations (a multiple of per_frame) with `limit` as the
    end: (first_frame, frames, spp).  A whole frame of per_frame iterations while one fits; the rest in frames of
    gcd(per_frame, rest) iterations, whose numbering continues where the whole frames ended."""
    rest = limit - done
    if rest >= per_frame:
        return done // per_frame, 1, per_frame
    g = math.gcd(per_frame, rest)
    return done // g, rest // g, g


def render_group(grp, a: argparse.Namespace, limit: int):
    """--devices: frames through the group up to `limit` iterations, or with --target-noise until rank 0's estimate
    is <= E (checked after every call from --min-spp on), or with --adaptive uniform frames up to --min-spp and then
    kdpt_group_trace_adaptive rounds as render_adaptive runs them on one context.  Returns the iterations done, the
    last estimate, the adaptive totals (None without --adaptive) and the frames rendered."""
    ndev = len(grp.devices)
    per_frame = max(1, min(16, a.pipeline)) * max(1, min(16, a.batch)) * ndev
    pt = grp.context(0)
    thr = a.target_noise if a.pixel_noise is None else a.pixel_noise
    uniform = min(a.min_spp, limit) if a.adaptive else limit
    done, frames, est = 0, 0, None
    while done < uniform:
        first, n, spp = frame_plan(done, uniform, per_frame)
        grp.render_frames(first, n, spp, pipeline=a.pipeline, batch=a.batch)
        grp.synchronize()
        done += n * spp
        frames += n
        if a.target_noise is not None and not a.adaptive and done >= a.min_spp:
            est = pt.noise_estimate(a.noise_floor, a.target_noise)
            if est.mean <= a.target_noise:
                break
    if not a.adaptive:
        return done, est, None, frames
    totals = {"pixel_samples": done * pt.width * pt.height, "segments": 0, "rounds": []}
    while done >= 2:
        est = pt.noise_estimate(a.noise_floor, thr)
        if est.mean <= a.target_noise or est.above == 0 or done >= limit:
            break
        n = min(per_frame, limit - done)
        r = grp.trace_adaptive(1 + done, n, pipeline=a.pipeline, batch=a.batch, floor=a.noise_floor, threshold=thr)
        done += n
        totals["pixel_samples"] += int(r.pixel_samples)
        totals["segments"] += int(r.segments)
        totals["rounds"].append({"active": int(r.active), "iterations": n, "device_ms": round(r.device_ms, 4)})
    return done, est, totals, frames


def save_pixels(mean):
    """saveImage's pixel pass (src/main.cpp:1087-1108, image::savePNG) on an (H, W, 3) float32 image of per-pixel
    means, samples = 1: (rgb, lin) -- lin the image flipped in x (what image::saveHDR writes), rgb its bytes,
    clamp(v, 0, 1) * 255.f in float32 truncated to uint8 (a NaN gives 0)."""
    import numpy as np
    lin = np.ascontiguousarray(np.asarray(mean, np.float32)[:, ::-1, :])
    with np.errstate(invalid="ignore"):
        cl = np.where(lin < 0, np.float32(0), lin)
        cl = np.where(cl > 1, np.float32(1), cl) * np.float32(255)
    return np.nan_to_num(cl, nan=0.0).astype(np.uint8), lin


def write_denoised(pt, a: argparse.Namespace, base: str):
    """--denoise: BASE.denoised.png / BASE.denoised.hdr from kdpt_denoise's means (the context's per-pixel sample
    counts are inside them), with --temporal from kdpt_denoise_temporal's: the files written."""
    from .runtime import default_denoise_params, hdr_encode, png_encode
    params = default_denoise_params(passes=a.denoise)
    rgb, lin = save_pixels(pt.denoise_temporal(dparams=params) if a.temporal else pt.denoise(params))
    written = []
    for ext, on, encode, pixels in ((".denoised.png", not a.no_png, png_encode, rgb),
                                    (".denoised.hdr", a.hdr, hdr_encode, lin)):
        if on:
            with open(base + ext, "wb") as f:
                f.write(encode(pixels))
            written.append(base + ext)
    return written


def write_outputs(pt, a: argparse.Namespace, base: str, spp: int, counted: bool):
    """The PNG / HDR / noise map of a context's image: the files written.  counted: every pixel divided by its own
    sample count (after adaptive rounds), then the same host encoders."""
    written = []
    if counted:
        from .runtime import hdr_encode, png_encode
        rgb, lin = pt.save_counted(lin=True)
        for ext, on, encode, pixels in ((".png", not a.no_png, png_encode, rgb), (".hdr", a.hdr, hdr_encode, lin)):
            if on:
                with open(base + ext, "wb") as f:
                    f.write(encode(pixels))
                written.append(base + ext)
    else:
        if not a.no_png:
            pt.save_png(base + ".png", float(spp))
            written.append(base + ".png")
        if a.hdr:
            pt.save_hdr(base + ".hdr", float(spp))
            written.append(base + ".hdr")
    if a.noise_map and spp >= 2:
        import numpy as np
        np.save(base + ".noise.npy", pt.noise_map(a.noise_floor))
        written.append(base + ".noise.npy")
    if a.denoise is not None:
        written += write_denoised(pt, a, base)
    return written


def orbit_frame_name(base: str, frame: int) -> str:
    return f"{base}.f{frame:04d}"


def main_orbit(a: argparse.Namespace, sd, hdr: dict, iterations: int, info: dict) -> int:
    """main() with --orbit: FRAMES views of `iterations` samples each, on one context or (--devices) a group whose
    rank 0 writes the outputs.  A view is "set camera, reset, render, write"; with --temporal the denoiser's history
    is reset before view 0 and carried from view to view."""
    from .runtime import REDUCE_COPY, REDUCE_RCCL, PathTracer, RenderGroup, orbit_camera
    nframes, degrees = a.orbit
    base = a.out or f"{hdr['file'] or os.path.splitext(os.path.basename(a.scene))[0]}.{iterations}samp"
    moments = a.denoise is not None
    if a.devices is not None:
        owner = RenderGroup(sd, a.devices, options_from_args(a), moments=moments,
                            reduce=REDUCE_COPY if a.reduce == "copy" else REDUCE_RCCL)
    else:
        owner = PathTracer(sd, options_from_args(a), device=a.device)
    written, temporal, segments = [], [], 0
    with owner:
        pt = owner.context(0) if a.devices is not None else owner
        if moments and a.devices is None:
            pt.set_moments(True)
        if a.temporal:
            pt.temporal_reset()
        t0 = time.perf_counter()
        for f in range(nframes):
            owner.synchronize()
            owner.set_camera(orbit_camera(sd.view.camera, degrees * f / nframes))
            owner.reset()
            # view f takes iterations f * N + 1 .. (f + 1) * N (from --first-iteration on one context): an iteration
            # number is a random seed, and the temporal blend wants every view's samples to be its own
            if a.devices is not None:
                per_frame = max(1, min(16, a.pipeline)) * max(1, min(16, a.batch)) * len(a.devices)
                spp = iterations if iterations <= per_frame else math.gcd(per_frame, iterations)
                owner.render_frames(f * (iterations // spp), iterations // spp, spp, pipeline=a.pipeline,
                                    batch=a.batch)
                owner.synchronize()
            else:
                pt.trace_iterations(a.first_iteration + f * iterations, iterations, pipeline=a.pipeline,
                                    batch=a.batch)
                pt.synchronize()
            ranks = range(len(a.devices)) if a.devices is not None else (0,)
            segments += sum(int((owner.context(r) if a.devices is not None else pt).stats().total_segments)
                            for r in ranks)
            written += write_outputs(pt, a, orbit_frame_name(base, f), iterations, False)
            if a.temporal:
                st = pt.temporal_stats()
                temporal.append({"frame": f, "with_history": st.with_history, "valid": st.valid})
                print(f"frame {f}: with_history / valid = {st.with_history} / {st.valid}", flush=True)
        dt = time.perf_counter() - t0
    info.update({"orbit": {"frames": nframes, "degrees": degrees}, "segments": segments, "seconds": round(dt, 4),
                 "ms_per_iteration": round(dt * 1e3 / (iterations * nframes), 4), "written": written})
    if a.devices is not None:
        info.update({"devices": a.devices, "reduce": a.reduce})
    if a.temporal:
        info["temporal"] = temporal
    print(json.dumps(info), flush=True)
    return 0


def main_group(a: argparse.Namespace, sd, hdr: dict, iterations: int, info: dict) -> int:
    """main() with --devices: the render through a RenderGroup, the output from rank 0's context."""
    from .runtime import REDUCE_COPY, REDUCE_RCCL, RenderGroup
    moments = a.target_noise is not None or a.denoise is not None
    with RenderGroup(sd, a.devices, options_from_args(a), reduce=REDUCE_COPY if a.reduce == "copy" else REDUCE_RCCL,
                     moments=moments) as grp:
        t0 = time.perf_counter()
        spp, est, adaptive, frames = render_group(grp, a, iterations)
        dt = time.perf_counter() - t0
        pt = grp.context(0)
        segments = sum(int(grp.context(r).stats().total_segments) for r in range(len(a.devices)))
        base = a.out or f"{hdr['file'] or os.path.splitext(os.path.basename(a.scene))[0]}.{spp}samp"
        written = write_outputs(pt, a, base, spp, adaptive is not None)
        counts = pt.sample_counts() if adaptive is not None else None
    segments += adaptive["segments"] if adaptive is not None else 0
    info.update({"devices": a.devices, "reduce": a.reduce, "frames": frames, "segments": segments,
                 "seconds": round(dt, 4), "mrays_per_s": round(segments / dt / 1e6, 2) if dt > 0 else None,
                 "ms_per_iteration": round(dt * 1e3 / spp, 4), "written": written})
    if a.target_noise is not None:
        info.update({"spp": spp, "target_noise": a.target_noise, "noise_floor": a.noise_floor,
                     "noise": None if est is None else {
                         "mean": est.mean, "max": est.max, "above": int(est.above), "nonfinite": int(est.nonfinite),
                         "pixels": int(est.pixels), "samples": int(est.samples)}})
    if adaptive is not None:
        info.update({"pixel_noise": a.target_noise if a.pixel_noise is None else a.pixel_noise,
                     "pixel_samples": adaptive["pixel_samples"], "mean_spp": float(counts.mean()),
                     "max_spp": int(counts.max()), "adaptive_rounds": adaptive["rounds"]})
    print(json.dumps(info), flush=True)
    return 0


def main(argv=None) -> int:
    a = parse_args(argv)
    from .runtime import PathTracer, SceneData
    hdr = scene_header(a.scene)
    iterations = a.iterations if a.iterations is not None else (hdr["iterations"] or 1)
    if iterations < 1:
        raise SystemExit("--iterations must be >= 1")
    build_dev = a.devices[0] if a.devices is not None else a.device
    kd_dev = build_dev if (a.kd_build == "gpu" and not a.dry_run) else None  # --dry-run needs no GPU
    sd = SceneData.from_files(a.scene, a.mesh, res=tuple(a.res) if a.res else None, depth=a.depth, kd_device=kd_dev)
    W, H = sd.resolution
    info = {"scene": a.scene, "mesh": a.mesh, "resolution": [W, H], "iterations": iterations,
            "geoms": sd.view.num_geoms, "materials": sd.view.num_materials, "kd_nodes": sd.view.num_nodes,
            "kd_tri_refs": sd.view.num_tris, "kd_build": a.kd_build if kd_dev is not None else "host",
            "kd_build_ms": round(sd.kd_build_ms(), 3) if kd_dev is not None else None}
    if a.dry_run:
        print(json.dumps(info), flush=True)
        sd.close()
        return 0
    if a.denoise is not None and iterations < 2:
        raise SystemExit("--denoise needs at least 2 iterations: the filter is guided by the per-pixel variance, "
                         f"and {iterations} iteration gives none (raise --iterations)")
    if a.orbit is not None:
        return main_orbit(a, sd, hdr, iterations, info)
    if a.devices is not None:
        return main_group(a, sd, hdr, iterations, info)
    opt = options_from_args(a)
    spp, est = iterations, None  # the samples per pixel actually rendered, and the adaptive stop's last estimate
    with PathTracer(sd, opt, device=a.device) as pt:
        t0 = time.perf_counter()
        adaptive = None  # --adaptive: the adaptive rounds' totals
        if a.denoise is not None:  # the filter's variance: second moments from the first iteration on
            pt.set_moments(True)
        if a.adaptive:
            spp, est, adaptive = render_adaptive(pt, a, iterations)
        elif a.target_noise is not None:
            spp, est = render_to_noise(pt, a, iterations)
        elif a.testing:  # one synchronous pathtrace() per iteration, like TESTINGMODE
            for it in range(a.first_iteration, a.first_iteration + iterations):
                pt.trace_iteration(it)
        else:
            pt.trace_iterations(a.first_iteration, iterations, pipeline=a.pipeline, batch=a.batch)
            pt.synchronize()
        dt = time.perf_counter() - t0
        st = pt.stats()
        base = a.out or f"{hdr['file'] or os.path.splitext(os.path.basename(a.scene))[0]}.{spp}samp"
        written = []
        if adaptive is not None:  # every pixel divided by its own sample count, then the same host encoders
            from .runtime import hdr_encode, png_encode
            rgb, lin = pt.save_counted(lin=True)
            counts = pt.sample_counts()
            for ext, on, encode, pixels in ((".png", not a.no_png, png_encode, rgb), (".hdr", a.hdr, hdr_encode, lin)):
                if on:
                    with open(base + ext, "wb") as f:
                        f.write(encode(pixels))
                    written.append(base + ext)
        else:
            if not a.no_png:
                pt.save_png(base + ".png", float(spp))
                written.append(base + ".png")
            if a.hdr:
                pt.save_hdr(base + ".hdr", float(spp))
                written.append(base + ".hdr")
        if a.noise_map and spp >= 2:
            import numpy as np
            np.save(base + ".noise.npy", pt.noise_map(a.noise_floor))
            written.append(base + ".noise.npy")
        if a.denoise is not None:
            written += write_denoised(pt, a, base)
    segments = int(st.total_segments) + (adaptive["segments"] if adaptive is not None else 0)
    info.update({"segments": segments, "seconds": round(dt, 4),
                 "mrays_per_s": round(segments / dt / 1e6, 2) if dt > 0 else None,
                 "ms_per_iteration": round(dt * 1e3 / spp, 4), "written": written})
    if a.target_noise is not None:
        info.update({"spp": spp, "target_noise": a.target_noise, "noise_floor": a.noise_floor,
                     "noise": None if est is None else {
                         "mean": est.mean, "max": est.max, "above": int(est.above), "nonfinite": int(est.nonfinite),
                         "pixels": int(est.pixels), "samples": int(est.samples)}})
    if adaptive is not None:
        info.update({"pixel_noise": a.target_noise if a.pixel_noise is None else a.pixel_noise,
                     "pixel_samples": adaptive["pixel_samples"], "mean_spp": float(counts.mean()),
                     "max_spp": int(counts.max()), "adaptive_rounds": adaptive["rounds"]})
    if a.testing:
        info["intersect_ms_total"] = round(st.intersect_ms_total, 4)
    print(json.dumps(info), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
