"""Ray queries from the command line: closest hits for a file of rays, or for the scene camera's rays.

    python -m kdtreepathtraceroptimization_amd.cast_cli SCENE.txt [MESH.obj] --rays RAYS.npy --out HITS.npy
    python -m kdtreepathtraceroptimization_amd.cast_cli SCENE.txt [MESH.obj] --camera --out BASE

--rays takes an n x 6 float32 array (origin, direction per row) and writes the n hit records
(runtime.RAY_HIT_DTYPE: t, kind, prim, material, point, normal) to --out.  --camera casts the scene camera's
un-jittered pinhole rays (generateRayFromCamera, src/pathtrace.cu:315-397, without antialiasing and depth of
field) and writes BASE.depth.npy (H x W float32, t; -1 where nothing is hit), BASE.normal.npy (H x W x 3) and
BASE.prim.npy (H x W x 2 int32: kind, prim).  Rows are in the path tracer's pixel order (index = y W + x; the
saved PNGs are that image flipped in x).  One JSON line reports the counts and the rate.

With --radiance SPP the rays are path traced instead (kdpt_trace_rays, iterations 1 .. SPP): --rays writes the mean
radiance (n x 3 float32; n at most the context's W H, which --res sets) to --out, and --camera traces the rays the
device itself generates for each iteration (kdpt_camera_rays: jitter and depth of field included) and writes
BASE.radiance.npy (H x W x 3), the render's image divided by SPP.  A rejected ray's radiance is NaN.  With --stderr
(SPP >= 2) the per-ray, per-channel standard error of that mean is written beside it (OUT.stderr.npy /
BASE.stderr.npy, float64), computed from the sum and the sum of squares (kdpt_trace_rays_moments).

Directions are normalised with the reference's glm::normalize unless --no-normalize is given; then a direction
that is not unit length (|dot(d, d) - 1| > 1e-6) is rejected, like any ray with a non-finite component (kind -1).
"""
from __future__ import annotations

import argparse
import json
import sys
import time

import numpy as np


def camera_rays(camera_bytes: bytes):
    """(origins, directions), each (W H, 3) float32: the pinhole ray of every pixel of a kdpt_camera (84 bytes,
    runtime.Camera), index = y W + x, with the float32 operations of generateRayFromCamera in its order --
    normalize(view - right * pixelLength.x * (x - W / 2) - up * pixelLength.y * (y - H / 2)) from the eye."""
    from .runtime import Camera
    cam = Camera.from_buffer_copy(camera_bytes)
    f32 = np.float32
    W, H = int(cam.resolution[0]), int(cam.resolution[1])
    view, up, right = (np.array(v[:], f32) for v in (cam.view, cam.up, cam.right))
    px, py = f32(cam.pixelLength[0]), f32(cam.pixelLength[1])
    ys, xs = np.divmod(np.arange(W * H, dtype=np.int64), W)
    fx = xs.astype(f32) - f32(W) * f32(0.5)
    fy = ys.astype(f32) - f32(H) * f32(0.5)
    a = (right * px)[None, :] * fx[:, None]  # (vec * float) * float
    b = (up * py)[None, :] * fy[:, None]
    v = (view[None, :] - a) - b
    sq = v * v
    inv = f32(1.0) / np.sqrt((sq[:, 0] + sq[:, 1]) + sq[:, 2])  # glm::normalize = x * inversesqrt(dot(x, x))
    d = (v * inv[:, None]).astype(f32)
    o = np.broadcast_to(np.array(cam.position[:], f32), (W * H, 3)).copy()
    return o, d


def parse_args(argv=None) -> argparse.Namespace:
    ap = argparse.ArgumentParser(prog="python -m kdtreepathtraceroptimization_amd.cast_cli",
                                 description="Closest hits of caller-supplied rays (kdpt_cast_rays) on MI355X.")
    ap.add_argument("scene", help="scene text file (scenes/*.txt)")
    ap.add_argument("mesh", nargs="?", default=None, help="optional OBJ mesh")
    src = ap.add_mutually_exclusive_group(required=True)
    src.add_argument("--rays", default=None, metavar="RAYS.npy", help="n x 6 float32: origin, direction per row")
    src.add_argument("--camera", action="store_true", help="the scene camera's un-jittered pinhole rays")
    ap.add_argument("--out", required=True, help="HITS.npy (--rays) or the base name of the passes (--camera)")
    ap.add_argument("--res", type=int, nargs=2, default=None, metavar=("W", "H"), help="camera resolution override")
    ap.add_argument("--bare", action="store_true", help="traverseKDbare instead of the short-stack hybrid")
    ap.add_argument("--no-normalize", action="store_true", help="directions are unit length already")
    ap.add_argument("--radiance", type=int, default=None, metavar="SPP",
                    help="path trace the rays instead (kdpt_trace_rays): mean radiance over SPP iterations, written "
                         "as float32 .npy -- n x 3 to --out with --rays (n <= W H of the context: see --res), "
                         "H x W x 3 to BASE.radiance.npy with --camera (the device's own camera rays)")
    ap.add_argument("--stderr", action="store_true",
                    help="with --radiance SPP (>= 2): also write the standard error of the mean per ray and channel "
                         "(float64 .npy; OUT.stderr.npy / BASE.stderr.npy), from kdpt_trace_rays_moments' two sums")
    ap.add_argument("--chunk", type=int, default=None, help="rays per chunk (knob cast_chunk)")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--kd-build", choices=["gpu", "host"], default="gpu")
    return ap.parse_args(argv)


def radiance_main(a: argparse.Namespace, sd, rays) -> int:
    """--radiance SPP: the mean over iterations 1 .. SPP of kdpt_trace_rays' radiance, for the given rays (o, d) or,
    with rays = None, for the rays kdpt_camera_rays reports for each iteration (jitter and depth of field included:
    the render's own rays, so the result is the render's image)."""
    from .runtime import PathTracer, default_options
    if a.radiance < 1:
        raise SystemExit("--radiance: SPP must be >= 1")
    if a.stderr and a.radiance < 2:
        raise SystemExit("--stderr: a standard error needs --radiance SPP >= 2")
    W, H = sd.resolution
    sumsq = None
    with PathTracer(sd, default_options(short_stack=0 if a.bare else 1), device=a.device) as pt:
        t0 = time.perf_counter()
        if rays is not None:
            if len(rays[0]) > W * H:
                raise SystemExit(f"--radiance: {len(rays[0])} rays exceed the context's {W} x {H} paths (raise --res)")
            if a.stderr:
                total, sumsq = pt.trace_rays(rays[0], rays[1], 1, a.radiance, normalize=not a.no_normalize,
                                             moments=True)
            else:
                total = pt.trace_rays(rays[0], rays[1], 1, a.radiance, normalize=not a.no_normalize)
        else:
            total = np.zeros((W * H, 3), np.float32)
            sumsq = np.zeros((W * H, 3), np.float32) if a.stderr else None
            for it in range(1, a.radiance + 1):
                o, d = pt.camera_rays(it)
                r = pt.trace_rays(o, d, it, 1, normalize=False)
                total += r
                if a.stderr:
                    sumsq += r * r
        dt = time.perf_counter() - t0
    mean = total / np.float32(a.radiance)
    out = a.out if rays is not None else a.out + ".radiance.npy"
    np.save(out, mean if rays is not None else mean.reshape(H, W, 3))
    written = [out]
    if a.stderr:
        se = standard_error(total, sumsq, a.radiance)
        se_out = (out[:-4] if out.endswith(".npy") else out) + ".stderr.npy" if rays is not None else a.out + ".stderr.npy"
        np.save(se_out, se if rays is not None else se.reshape(H, W, 3))
        written.append(se_out)
    print(json.dumps({"scene": a.scene, "mesh": a.mesh, "n": len(mean), "spp": a.radiance,
                      "invalid": int(np.sum(np.isnan(mean).all(axis=1))), "seconds": round(dt, 4),
                      "written": written}), flush=True)
    return 0


def standard_error(total: np.ndarray, sumsq: np.ndarray, samples: int) -> np.ndarray:
    """The standard error of the mean per ray and channel, in float64 from the two float32 sums, with
    kdpt_noise_map's formula without its division by the floored mean: m = S / n, v = max((Q - S m) / (n - 1), 0),
    sqrt(v / n)."""
    n = float(samples)
    s, q = total.astype(np.float64), sumsq.astype(np.float64)
    m = s / n
    v = (q - s * m) / (n - 1.0)
    v = np.where(v < 0, 0.0, v)  # (NaN stays NaN)
    return np.sqrt(v / n)


def main(argv=None) -> int:
    a = parse_args(argv)
    from .runtime import HIT_GEOM, HIT_INVALID, HIT_NONE, HIT_TRIANGLE, PathTracer, SceneData, default_options
    if a.rays:
        rays = np.load(a.rays)
        if rays.ndim != 2 or rays.shape[1] != 6:
            raise SystemExit(f"--rays: expected an n x 6 array, got shape {rays.shape}")
        rays = np.ascontiguousarray(rays, np.float32)
    sd = SceneData.from_files(a.scene, a.mesh, res=tuple(a.res) if a.res else None,
                              kd_device=a.device if a.kd_build == "gpu" else None)
    W, H = sd.resolution
    if a.camera:
        o, d = camera_rays(sd.camera_bytes())
    else:
        o, d = rays[:, :3], rays[:, 3:]
    if a.radiance is not None:
        return radiance_main(a, sd, None if a.camera else (o, d))
    with PathTracer(sd, default_options(short_stack=0 if a.bare else 1), device=a.device) as pt:
        if a.chunk:
            pt.set_tuning("cast_chunk", a.chunk)
        t0 = time.perf_counter()
        hits = pt.cast_rays(o, d, normalize=not a.no_normalize)
        dt = time.perf_counter() - t0
        st = pt.cast_stats()
    written = []
    if a.camera:
        np.save(a.out + ".depth.npy", hits["t"].reshape(H, W))
        np.save(a.out + ".normal.npy", hits["normal"].reshape(H, W, 3))
        np.save(a.out + ".prim.npy", np.stack([hits["kind"], hits["prim"]], -1).reshape(H, W, 2))
        written = [a.out + s for s in (".depth.npy", ".normal.npy", ".prim.npy")]
    else:
        np.save(a.out, hits)
        written = [a.out]
    n = len(hits)
    kind = hits["kind"]
    print(json.dumps({"scene": a.scene, "mesh": a.mesh, "n": n, "traced": st.traced,
                      "invalid": int(np.sum(kind == HIT_INVALID)),
                      "hits": {"none": int(np.sum(kind == HIT_NONE)), "geom": int(np.sum(kind == HIT_GEOM)),
                               "triangle": int(np.sum(kind == HIT_TRIANGLE))},
                      "seconds": round(dt, 4), "device_ms": round(st.device_ms, 4),
                      "mrays_per_s": round(n / dt / 1e6, 3) if dt > 0 else None, "written": written}), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
