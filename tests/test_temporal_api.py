"""Temporal accumulation (kdpt_default_temporal_params, kdpt_temporal_buffers, kdpt_denoise_temporal,
kdpt_temporal_reset, kdpt_temporal_stats): what can be checked without a device -- the symbols against the header,
kdpt_temporal_params' layout and defaults, every argument refusal of kdpt_temporal_buffers (reported before any device
call, so it reads the same here) with a message that names its reason, the Python mirror, orbit_camera, the command
line's --orbit / --temporal, the sources' place in the runtime, and the documents that must speak of it."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from kdtreepathtraceroptimization_amd import cli

KDPT_ERR_ARG = -1
ENTRY_POINTS = ["kdpt_default_temporal_params", "kdpt_temporal_buffers", "kdpt_denoise_temporal",
                "kdpt_temporal_reset", "kdpt_temporal_stats"]
FIELDS = ["alpha", "sigma_z", "normal_min", "max_history", "pad_"]
CURRENT = ["color", "variance", "normal", "point", "depth", "id"]
HISTORY = ["h_color", "h_variance", "h_normal", "h_point", "h_depth", "h_id", "h_length", "h_camera"]
OUTPUTS = ["out_color", "out_variance", "out_length"]
CSRC = os.path.join(ROOT, "kdtreepathtraceroptimization_amd", "csrc")


def test_symbols_are_exported_declared_and_mirrored(kdpt):
    lib = kdpt.load_library()
    out = subprocess.run(["nm", "-D", "--defined-only", kdpt.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "kdpt.h")).read(), flags=re.S)
    for n in ENTRY_POINTS:
        assert hasattr(lib, n), n
        assert re.search(rf"\bT {n}\b", out), n
        assert n in kdpt.EXPORTS
        assert re.search(rf"\b{n}\s*\(", header), n
    P = C.POINTER
    assert lib.kdpt_default_temporal_params.argtypes == [P(kdpt.TemporalParams)]
    assert len(lib.kdpt_temporal_buffers.argtypes) == 3 + 6 + 7 + 2 + 3
    assert lib.kdpt_temporal_buffers.argtypes[16:18] == [P(kdpt.Camera), P(kdpt.TemporalParams)]
    assert lib.kdpt_denoise_temporal.argtypes == [C.c_void_p, P(kdpt.TemporalParams), P(kdpt.DenoiseParams),
                                                  C.c_void_p, C.c_void_p]
    for method in ("denoise_temporal", "temporal_reset", "temporal_stats"):
        assert callable(getattr(kdpt.PathTracer, method)), method
    assert callable(kdpt.temporal_buffers) and callable(kdpt.default_temporal_params) and callable(kdpt.orbit_camera)


def test_params_layout_and_defaults_agree_with_the_header(kdpt, tmp_path):
    """A C program compiled against include/kdpt.h prints sizeof(kdpt_temporal_params) and every field's offset; the
    ctypes mirror must say the same (24 bytes, as the header states).  The defaults are the documented ones."""
    src = tmp_path / "layout.c"
    src.write_text("#include <stdio.h>\n#include <stddef.h>\n#include \"kdpt.h\"\nint main(void) {\n"
                   "  printf(\"%zu\", sizeof(kdpt_temporal_params));\n" +
                   "".join(f"  printf(\" %zu\", offsetof(kdpt_temporal_params, {f}));\n" for f in FIELDS) +
                   "  printf(\"\\n\");\n  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o",
                    str(exe)], check=True)
    vals = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert vals[0] == 24 == C.sizeof(kdpt.TemporalParams)
    assert vals[1:] == [0, 4, 8, 12, 16] == [getattr(kdpt.TemporalParams, f).offset for f in FIELDS]
    assert [n for n, _ in kdpt.TemporalParams._fields_] == FIELDS
    header = open(os.path.join(ROOT, "include", "kdpt.h")).read()
    assert re.search(r"typedef struct kdpt_temporal_params \{\s*/\* 24 bytes \*/", header)
    p = kdpt.TemporalParams(-1.0, -1.0, -5.0, -1, (C.c_float * 2)(-1.0, -1.0))
    kdpt.load_library().kdpt_default_temporal_params(C.byref(p))
    f32 = np.float32
    assert (p.alpha, p.sigma_z, p.normal_min, p.max_history) == (float(f32(0.2)), float(f32(0.02)), float(f32(0.9)), 32)
    assert list(p.pad_) == [0.0, 0.0]
    kdpt.load_library().kdpt_default_temporal_params(None)  # (a null pointer is ignored)
    q = kdpt.default_temporal_params(alpha=0.5, max_history=8)
    assert (q.alpha, q.max_history, q.sigma_z) == (0.5, 8, float(f32(0.02)))
    with pytest.raises(KeyError):
        kdpt.default_temporal_params(sigma=1.0)


def _buffers(kdpt, w=4, h=3, drop=(), history=True, cam_res=None, **params):
    lib = kdpt.load_library()
    n = 12
    arrs = {}
    for k in CURRENT + HISTORY[:-1] + OUTPUTS:
        per = 3 if k.endswith(("color", "normal", "point")) else 1
        arrs[k] = ((C.c_int if k.endswith("id") else C.c_float) * (per * n))()
    cam = kdpt.Camera()
    cam.resolution[0], cam.resolution[1] = cam_res if cam_res is not None else (w, h)
    arrs["h_camera"] = C.byref(cam)
    p = kdpt.default_temporal_params(**params)
    arrs["params"] = C.byref(p)
    if not history:
        drop = tuple(drop) + tuple(HISTORY)
    a = {k: (None if k in drop else v) for k, v in arrs.items()}
    return lib.kdpt_temporal_buffers(0, w, h, *[a[k] for k in CURRENT], *[a[k] for k in HISTORY], a["params"],
                                     *[a[k] for k in OUTPUTS])


CASES = (
    [(dict(drop=(k,)), f"null {k}".encode()) for k in CURRENT + ["params"] + OUTPUTS] +
    [(dict(drop=(k,), history=False), f"null {k}".encode()) for k in ("color", "out_length")] +
    # a history given only in part: each one missing, all but one missing, and the camera alone
    [(dict(drop=(k,)), f"partial history: null {k}".encode()) for k in HISTORY] +
    [(dict(drop=tuple(k for k in HISTORY if k != "h_length")), b"partial history"),
     (dict(drop=tuple(HISTORY[:-1])), b"partial history: null h_color")] +
    [(dict(w=0), b"w must be"), (dict(h=0), b"h must be"), (dict(w=-3), b"w must be"), (dict(h=-1), b"h must be"),
     (dict(w=1 << 13, h=(1 << 13) + 1), b"w * h must be"), (dict(w=1 << 30, h=1 << 30), b"w * h must be"),
     (dict(w=0, history=False), b"w must be"),
     (dict(alpha=0.0), b"alpha"), (dict(alpha=-0.5), b"alpha"), (dict(alpha=1.5), b"alpha"),
     (dict(alpha=math.nan), b"alpha"), (dict(alpha=math.inf), b"alpha"),
     (dict(sigma_z=0.0), b"sigma_z"), (dict(sigma_z=-1.0), b"sigma_z"), (dict(sigma_z=math.nan), b"sigma_z"),
     (dict(sigma_z=math.inf), b"sigma_z"),
     (dict(normal_min=-1.5), b"normal_min"), (dict(normal_min=1.25), b"normal_min"),
     (dict(normal_min=math.nan), b"normal_min"), (dict(normal_min=-math.inf), b"normal_min"),
     (dict(max_history=0), b"max_history"), (dict(max_history=-1), b"max_history"),
     (dict(max_history=4097), b"max_history"),
     (dict(alpha=0.0, history=False), b"alpha"),
     (dict(cam_res=(3, 4)), b"h_camera.resolution is 3 x 4"), (dict(cam_res=(4, 4)), b"h_camera.resolution"),
     (dict(cam_res=(0, 0)), b"h_camera.resolution")])


@pytest.mark.parametrize("kw, word", CASES, ids=[f"{i:02d}_" + w.decode().replace(" ", "_").replace(":", "")
                                                 for i, (_, w) in enumerate(CASES)])
def test_temporal_buffers_argument_errors_need_no_device(kdpt, kw, word):
    lib = kdpt.load_library()
    assert lib.kdpt_create(None, None, 0, C.byref(C.c_void_p())) != 0  # another call's message is current
    assert _buffers(kdpt, **kw) == KDPT_ERR_ARG
    msg = lib.kdpt_last_error()
    assert msg.startswith(b"kdpt_temporal_buffers:") and word in msg, msg


def test_context_entry_points_refuse_null_arguments_by_name(kdpt):
    lib = kdpt.load_library()
    tp, dp, out = kdpt.default_temporal_params(), kdpt.default_denoise_params(), (C.c_float * 12)()
    assert lib.kdpt_denoise_temporal(None, C.byref(tp), C.byref(dp), C.cast(out, C.c_void_p), None) == KDPT_ERR_ARG
    assert lib.kdpt_last_error().startswith(b"kdpt_denoise_temporal:") and b"null ctx" in lib.kdpt_last_error()
    assert lib.kdpt_temporal_reset(None) == KDPT_ERR_ARG
    assert lib.kdpt_last_error().startswith(b"kdpt_temporal_reset:") and b"null ctx" in lib.kdpt_last_error()
    assert lib.kdpt_temporal_stats(None, None, None, None, None, None) == KDPT_ERR_ARG
    assert lib.kdpt_last_error().startswith(b"kdpt_temporal_stats:") and b"null ctx" in lib.kdpt_last_error()
    z = np.zeros
    with pytest.raises(ValueError):  # colour without its channel axis
        kdpt.temporal_buffers(z((3, 4)), z((3, 4)), z((3, 4, 3)), z((3, 4, 3)), z((3, 4)), z((3, 4)))
    with pytest.raises(ValueError):  # a history of another shape
        kdpt.temporal_buffers(z((3, 4, 3)), z((3, 4)), z((3, 4, 3)), z((3, 4, 3)), z((3, 4)), z((3, 4)),
                              history=(z((3, 5, 3)), z((3, 5)), z((3, 5, 3)), z((3, 5, 3)), z((3, 5)), z((3, 5)),
                                       z((3, 5)), kdpt.Camera()))


def test_orbit_camera_is_the_documented_rotation(kdpt):
    f32 = np.float32
    cam = kdpt.Camera()
    cam.resolution[0], cam.resolution[1] = 64, 48
    for name, v in (("position", (0.0, 5.0, 10.5)), ("lookAt", (0.0, 5.0, 0.0)), ("up", (0.0, 1.0, 0.0)),
                    ("view", (0.0, 0.0, -1.0)), ("right", (1.0, 0.0, 0.0)), ("fov", (30.0, 25.0)),
                    ("pixelLength", (0.01, 0.012))):
        setattr(cam, name, (C.c_float * len(v))(*v))
    same = kdpt.orbit_camera(cam, 0.0)  # (as values: the cross product writes a zero of either sign)
    assert all(list(getattr(same, n)) == list(getattr(cam, n)) for n, _ in kdpt.Camera._fields_)
    q = kdpt.orbit_camera(cam, 90.0)
    pos, view, right = (np.array(a[:], f32) for a in (q.position, q.view, q.right))
    assert np.allclose(pos, [10.5, 5.0, 0.0], atol=1e-5) and np.allclose(view, [-1, 0, 0], atol=1e-6)
    assert np.allclose(right, [0, 0, -1], atol=1e-6)
    for keep in ("resolution", "lookAt", "up", "fov", "pixelLength"):
        assert list(getattr(q, keep)) == list(getattr(cam, keep)), keep
    s = kdpt.orbit_camera(cam, 1.0)  # a small step: the distance to lookAt and the frame's orthonormality stay
    pos, view, right, up = (np.array(a[:], np.float64) for a in (s.position, s.view, s.right, s.up))
    assert abs(np.linalg.norm(pos - [0, 5, 0]) - 10.5) < 1e-5
    assert abs(np.dot(view, right)) < 1e-6 and abs(np.dot(right, up)) < 1e-6 and abs(np.linalg.norm(right) - 1) < 1e-6
    assert abs(math.degrees(math.atan2(pos[0], pos[2])) - 1.0) < 1e-4
    assert bytes(cam.position) == bytes((C.c_float * 3)(0.0, 5.0, 10.5))  # the argument is not changed


def test_cli_parses_orbit_and_temporal():
    a = cli.parse_args(["s.txt"])
    assert a.orbit is None and a.temporal is False
    a = cli.parse_args(["s.txt", "--orbit", "3", "4.5", "--denoise", "--temporal", "--iterations", "4"])
    assert a.orbit == (3, 4.5) and a.temporal and a.denoise == 5
    a = cli.parse_args(["s.txt", "--orbit", "2", "-10", "--devices", "0,0", "--reduce", "copy", "--denoise", "2",
                        "--temporal"])
    assert a.orbit == (2, -10.0) and a.devices == [0, 0]
    assert cli.parse_args(["s.txt", "--orbit", "1", "0"]).orbit == (1, 0.0)
    for bad in (["--temporal"], ["--temporal", "--orbit", "2", "1"], ["--orbit", "0", "1"], ["--orbit", "x", "1"],
                ["--orbit", "2", "nan"], ["--orbit", "2"], ["--orbit", "2", "1", "--adaptive", "--target-noise", "1"],
                ["--orbit", "2", "1", "--target-noise", "0.5"], ["--orbit", "2", "1", "--testing"]):
        with pytest.raises(SystemExit):
            cli.parse_args(["s.txt", *bad])
    assert cli.orbit_frame_name("out", 7) == "out.f0007"


def test_the_sections_are_part_of_the_runtime():
    from kdtreepathtraceroptimization_amd import _build
    from test_stream_discipline import RUNTIME, _functions, _strip
    runtime = open(os.path.join(CSRC, "kdpt_runtime.hip")).read()
    kernels = re.findall(r'#include "(kernels_\w+\.h)"', runtime)
    hosts = re.findall(r'#include "(host_\w+\.h)"', runtime)
    assert kernels.index("kernels_temporal.h") > kernels.index("kernels_denoise.h")
    assert hosts.index("host_temporal.h") > hosts.index("host_denoise.h")
    assert os.path.join(CSRC, "host_temporal.h") in RUNTIME and "kernels_temporal.h" in _build.KERNEL_SOURCES
    ksrc = re.sub(r"//[^\n]*", "", open(os.path.join(CSRC, "kernels_temporal.h")).read())
    assert not re.search(r"\bhip[A-Z]\w*\s*\(", ksrc) and "__shared__" not in ksrc
    for kernel in ("k_temporal", "k_temporal_pack_history"):
        assert re.search(r"__global__[^;{]*\b" + kernel + r"\b", ksrc), kernel
    assert re.findall(r"\batomic\w*", ksrc) == ["atomicAdd", "atomicAdd"]  # the two integer counters, nothing else
    assert re.search(r"unsigned int\s*\*\s*counts", ksrc)
    # the history: handles inside the context, dropped where the header says
    ctx = _strip(open(os.path.join(CSRC, "host_context.h")).read())
    body = ctx[ctx.index("struct Temporal {"):ctx.index("struct kdpt_ctx {")]
    assert "DeviceBuf<float4> g0, g1, cv" in body and "DeviceBuf<float> len" in body and "*" not in body
    assert re.search(r"\bTemporal tmp\s*;", ctx[ctx.index("struct kdpt_ctx {"):])
    funcs = {n: b for n, b, _ in _functions(_strip(open(os.path.join(CSRC, "host_create.h")).read()))}
    assert re.search(r"c->tmp\.s\s*=\s*\{\s*\}", funcs["kdpt_set_tuning"])
    funcs = {n: b for n, b, _ in _functions(_strip(open(os.path.join(CSRC, "host_temporal.h")).read()))}
    assert re.search(r"c->tmp\.s\s*=\s*\{\s*\}", funcs["kdpt_temporal_reset"])
    buffers = funcs["kdpt_temporal_buffers"]
    assert buffers.index("Stream st") < buffers.index("DeviceBuf<")
    assert buffers.rindex("KDPT_ERR_ARG") < buffers.index("hipSetDevice")  # every refusal before any device call
    assert buffers.index("h_camera->resolution") < buffers.index("hipSetDevice")


@pytest.mark.parametrize("kernel", ["k_temporal", "k_temporal_pack_history"])
def test_temporal_kernels_scratch_and_occupancy_within_budget(kdpt, kernel):
    """The stage is bound by its gathers' latency: it must spill nothing, use no LDS and keep 8 waves per SIMD."""
    from test_build_resources import _report
    from test_group_resources import _lds
    rep = _report()
    ks = [k for k in rep if kernel + "E" in k]
    assert len(ks) == 1, ks
    assert rep[ks[0]].get("ScratchSize", 0) == 0 and rep[ks[0]].get("Occupancy", 0) >= 8, rep[ks[0]]
    assert _lds()[ks[0]] == 0


def test_documents_speak_of_it():
    docs = {n: open(os.path.join(ROOT, n)).read() for n in ("DESIGN.md", "README.md", "PAPERS.md")}
    assert re.search(r"^## 18\.", docs["DESIGN.md"], flags=re.M)
    sec = docs["DESIGN.md"][docs["DESIGN.md"].index("## 18."):]
    for word in ("kdpt_denoise_temporal", "k_temporal", "VGPR", "moving geometry", "albedo", "mirrors", "w^2"):
        assert word in sec, word
    for word in ("--orbit", "--temporal", "kernels_temporal.h", "host_temporal.h"):
        assert word in docs["README.md"], word
    assert "kdpt_denoise_temporal" in docs["PAPERS.md"]
    header = open(os.path.join(ROOT, "include", "kdpt.h")).read()
    assert "Temporal accumulation" in header
    group = header[header.index("kdpt_group_context lends"):]
    lent = group[:group.index("A borrowed context must not")]
    assert "kdpt_denoise_temporal" in lent and "kdpt_temporal_reset" in lent
