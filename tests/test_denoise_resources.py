"""The denoiser's device resources and kernels, from the sources and the gfx950 build's resource report
(build/kdpt_runtime.build.log, see test_build_resources.py).

Ownership, read from the sources as tests/test_resource_ownership.py reads them: every device buffer and event of
kdpt_denoise is a kdpt_owned.h handle inside the context's Denoiser, so `delete c` in kdpt_destroy releases them and
no path can free one twice or not at all; kdpt_denoise_buffers' temporaries are handles on its stack.  Kernels: the
filter pass is latency-bound on its loads (memory or LDS), so both routes must keep several waves per SIMD and spill
nothing, and the tiled route's LDS must be the three staged records of a 36 x 12 tile + halo."""
import os
import re

import pytest

from conftest import ROOT
from test_build_resources import _report
from test_group_resources import _lds
from test_stream_discipline import RUNTIME, _functions, _strip

CSRC = os.path.join(ROOT, "kdtreepathtraceroptimization_amd", "csrc")
NEW = ("k_denoise_rays", "k_denoise_pack", "k_denoise_pack_render", "k_denoise_unpack", "k_denoise_pass")


def _src(name):
    return _strip(open(os.path.join(CSRC, name)).read())


def _struct(src, name):
    m = re.search(r"\bstruct " + name + r"\s*\{", src)
    assert m, name
    depth, i = 0, m.end() - 1
    while True:
        depth += {"{": 1, "}": -1}.get(src[i], 0)
        if depth == 0:
            return src[m.end():i]
        i += 1


def test_the_context_owns_the_denoisers_buffers_through_handles():
    ctx = _src("host_context.h")
    body = _struct(ctx, "Denoiser")
    members = [d.strip() for d in re.sub(r"struct Buffers\s*\{|\}\s*b\s*;", ";", body).split(";") if d.strip()]
    assert len(members) >= 10
    for decl in members:
        if re.match(r"(int|double)\b", decl):  # the size the buffers were made for, the last call's times
            assert "*" not in decl, decl
            continue
        assert re.match(r"(DeviceBuf<[\w ]+>|Event)\s+\w+", decl), decl  # a handle: no raw pointer, no raw event
    assert re.search(r"\bDenoiser den\s*;", _struct(ctx, "kdpt_ctx"))
    assert "kdpt_owned.h" in open(os.path.join(CSRC, "kdpt_runtime.hip")).read()


def test_kdpt_destroy_frees_them_and_no_other_path_does():
    destroy = {n: b for n, b, _ in _functions(_src("host_frames.h"))}["kdpt_destroy"]
    assert re.search(r"\bdelete c\s*;", destroy)  # the context's members go with it, the Denoiser among them
    host = os.path.join(CSRC, "host_denoise.h")
    assert host in RUNTIME  # so tests/test_resource_ownership.py and test_stream_discipline.py read it
    src = _src("host_denoise.h")
    assert not re.search(r"\b(hipFree\w*|hipMalloc\w*|hipEventCreate\w*|hipEventDestroy|hipStreamCreate\w*|"
                         r"hipStreamDestroy)\s*\(", src)
    assert not re.search(r"\bnew\b|\bmalloc\s*\(", src)
    # dropped (for the next call to remake) where the header says: kdpt_set_tuning
    tuning = {n: b for n, b, _ in _functions(_src("host_create.h"))}["kdpt_set_tuning"]
    assert re.search(r"c->den\.b\s*=\s*\{\s*\}", tuning)
    # the stand-alone entry point's temporaries are handles too, its stream declared before them (destroyed last)
    buffers = {n: b for n, b, _ in _functions(src)}["kdpt_denoise_buffers"]
    assert buffers.index("Stream st") < buffers.index("DeviceBuf<")
    assert "hipMemcpy(" not in src and "hipMemset(" not in src


def test_kernel_section_holds_device_code_only():
    src = re.sub(r"//[^\n]*", "", open(os.path.join(CSRC, "kernels_denoise.h")).read())
    assert not re.search(r"\bhip[A-Z]\w*\s*\(", src)
    for kernel in NEW:
        assert re.search(r"__global__[^;{]*\b" + kernel + r"\b", src), kernel
    assert "atomic" not in src
    runtime = open(os.path.join(CSRC, "kdpt_runtime.hip")).read()
    assert "kernels_denoise.h" in re.findall(r'#include "(kernels_\w+\.h)"', runtime)
    assert "host_denoise.h" in re.findall(r'#include "(host_\w+\.h)"', runtime)
    from kdtreepathtraceroptimization_amd import _build
    assert "kernels_denoise.h" in _build.KERNEL_SOURCES


@pytest.mark.parametrize("frag", NEW)
def test_denoise_kernels_scratch_and_occupancy_within_budget(kdpt, frag):
    rep = _report()
    ks = [k for k in rep if frag + "E" in k or frag + "I" in k]  # (the mangled name: not k_denoise_pack_render's)
    assert ks, frag
    assert len(ks) == (2 if frag == "k_denoise_pass" else 1), ks  # the tiled route and the gather
    for k in ks:
        assert rep[k].get("ScratchSize", 0) == 0, (k, rep[k])
        assert rep[k].get("Occupancy", 0) >= 4, (k, rep[k])
    if frag == "k_denoise_pass":
        lds = sorted(_lds()[k] for k in ks)
        assert lds == [0, 3 * 16 * 36 * 12], lds


def test_new_kernel_names_stay_out_of_the_existing_budgets():
    from test_adaptive_resources import NEW as ADAPTIVE
    from test_build_resources import HOT
    from test_group_resources import NEW as GROUP
    from test_moments_resources import NEW as MOMENTS
    from test_trace_rays_resources import NEW as RAYS
    for name in NEW:
        assert not any(frag in name for frag in (*HOT, *ADAPTIVE, *GROUP, *MOMENTS, *RAYS)), name
