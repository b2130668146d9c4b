"""Static guard for the library's resource ownership: csrc/kdpt_owned.h is the only place that creates or
releases a HIP resource.

The runtime (csrc/kdpt_runtime.hip) and the device KD build (csrc/kd_build.hip) hold device memory, pinned host
memory, events, streams and host registrations through the handles of kdpt_owned.h, which release in their
destructors.  So neither file calls a release function (a hand-kept free list is how a buffer gets leaked on one
path and freed twice on another) or a creation function (a raw handle has no owner).  The check runs on the
sources with comments and strings stripped, like tests/test_stream_discipline.py.
"""
import os
import re

import pytest

from conftest import ROOT
from test_stream_discipline import RUNTIME, _strip

CSRC = os.path.join(ROOT, "kdtreepathtraceroptimization_amd", "csrc")
SOURCES = RUNTIME + [os.path.join(CSRC, "kd_build.hip")]  # (the runtime with the host sections it includes)
OWNER = os.path.join(CSRC, "kdpt_owned.h")
RELEASE = ("hipFree", "hipHostFree", "hipEventDestroy", "hipStreamDestroy", "hipHostUnregister")
CREATE = ("hipMalloc", "hipHostMalloc", "hipEventCreate", "hipEventCreateWithFlags", "hipStreamCreate",
          "hipStreamCreateWithFlags", "hipStreamCreateWithPriority", "hipExtStreamCreateWithCUMask", "hipHostRegister")
# (hipMalloc\w*, hipEventCreate\w*, hipStreamCreate\w*: every variant, the managed / async / pitched ones too)
CALL = re.compile(r"\b(hipFree\w*|hipHostFree|hipEventDestroy|hipStreamDestroy|hipHostUnregister|hipMalloc\w*|"
                  r"hipHostMalloc|hipHostAlloc|hipEventCreate\w*|hipStreamCreate\w*|hipExtStreamCreateWithCUMask|"
                  r"hipHostRegister)\s*\(")


def _raw_calls(src: str):
    src = _strip(src)  # (keeps the line structure)
    return [(m.group(1), src.count("\n", 0, m.start()) + 1) for m in CALL.finditer(src)]


@pytest.mark.parametrize("path", SOURCES, ids=os.path.basename)
def test_no_resource_is_created_or_released_outside_the_owner(path):
    bad = [f"{os.path.basename(path)}:{line}: {fn}" for fn, line in _raw_calls(open(path).read())]
    assert not bad, "raw HIP resource calls (use a handle of kdpt_owned.h):\n" + "\n".join(bad)


def test_the_owner_holds_every_kind():
    """The other half: the header does name each of them (a release function as a handle's template argument), so
    the guard above is not vacuous about a renamed API."""
    seen = set(re.findall(r"\bhip[A-Z]\w*", _strip(open(OWNER).read())))
    assert set(RELEASE) <= seen
    assert {"hipMalloc", "hipHostMalloc", "hipEventCreate", "hipEventCreateWithFlags", "hipStreamCreateWithFlags",
            "hipExtStreamCreateWithCUMask", "hipHostRegister"} <= seen


def test_the_guard_sees_the_pattern():
    """The checker itself: every release and creation call is reported with its line; a mention in a comment or a
    string, a longer identifier and a member named like a call are not."""
    src = """
    int f(kdpt_ctx* c) { HIP_TRY(hipMalloc(&p, 4)); (void)hipFree (p); return 0; }
    // hipFree(p) in a comment
    int g() { return fail(1, "hipEventDestroy(e) in a string"); }  /* hipStreamDestroy(s) */
    int h(Stream* st) { HIP_TRY(st->create(0)); my_hipFree(p); c->masks.dev = {}; return 0; }
    int k() { hipEventCreateWithFlags(&e, 2); hipStreamCreateWithFlags(&s, 1); hipHostUnregister(q); return 0; }
    """
    assert _raw_calls(src) == [("hipMalloc", 2), ("hipFree", 2), ("hipEventCreateWithFlags", 6),
                               ("hipStreamCreateWithFlags", 6), ("hipHostUnregister", 6)]
    for fn in RELEASE + CREATE:
        assert _raw_calls(f"void f() {{ {fn}(x); }}") == [(fn, 1)]
