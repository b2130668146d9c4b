"""One error channel (csrc/kdpt_error.h): every failing kdpt_* call leaves ITS message in kdpt_last_error(), whichever
translation unit it fails in (scene_host.cpp, image_io.cpp, kd_build.hip, kdpt_runtime.hip), so the Python
exceptions runtime._check builds from it never carry an earlier call's text.  No GPU needed.

Each case first makes an unrelated failing call that leaves a known message ("unknown tuning knob no_such_knob"),
then the call under test, and asserts the code, the named text, and that the stale message is gone."""
import ctypes as C
import dataclasses
import re

import numpy as np
import pytest

from kdtreepathtraceroptimization_amd import load_fixture_scene
from scene_text import write_scene_text

KDPT_ERR_ARG, KDPT_ERR_HIP, KDPT_ERR_IO = -1, -2, -4
STALE = b"no_such_knob"


@pytest.fixture
def lib(kdpt):
    """The library, with another call's failure message in the slot."""
    lib = kdpt.load_library()
    assert lib.kdpt_set_tuning(None, STALE, 0.0) == KDPT_ERR_ARG
    assert STALE in lib.kdpt_last_error()
    return lib


def _refused(lib, rc, code, *texts):
    msg = lib.kdpt_last_error()
    assert rc == code, (rc, msg)
    assert STALE not in msg, msg
    for t in texts:
        assert (t if isinstance(t, bytes) else str(t).encode()) in msg, (t, msg)
    return msg


def test_scene_load_names_the_missing_scene_file(lib, tmp_path):
    path = str(tmp_path / "nowhere" / "scene.txt")
    h = C.c_void_p()
    _refused(lib, lib.kdpt_scene_load(path.encode(), None, 0, 0, 0, C.byref(h)), KDPT_ERR_IO, path, "No such file")


def test_scene_load_names_the_missing_obj_file(lib, tmp_path):
    scene = write_scene_text("cornell", str(tmp_path / "scene.txt"), res=(32, 32))
    obj = str(tmp_path / "missing.obj")
    h = C.c_void_p()
    msg = _refused(lib, lib.kdpt_scene_load(scene.encode(), obj.encode(), 0, 0, 0, C.byref(h)), KDPT_ERR_IO, obj)
    assert scene.encode() not in msg


def test_scene_build_names_res(lib, kdpt):
    d, keep = dataclasses.replace(load_fixture_scene("cornell"), res=(0, 8)).to_c()
    h = C.c_void_p()
    _refused(lib, lib.kdpt_scene_build(C.byref(d), C.byref(h)), KDPT_ERR_ARG, "res", "0 x 8")


def test_scene_build_device_names_device(lib, kdpt):
    d, keep = load_fixture_scene("cornell").to_c()
    h = C.c_void_p()
    _refused(lib, lib.kdpt_scene_build_device(C.byref(d), -1, C.byref(h)), KDPT_ERR_ARG, "device", "-1")
    assert lib.kdpt_set_tuning(None, STALE, 0.0) == KDPT_ERR_ARG
    _refused(lib, lib.kdpt_scene_load_device(b"x", None, 0, 0, 0, -1, C.byref(h)), KDPT_ERR_ARG, "device")


def test_scene_view_names_the_null_argument(lib, kdpt):
    _refused(lib, lib.kdpt_scene_view(None, C.byref(kdpt.Scene())), KDPT_ERR_ARG, "kdpt_scene_view", "null sd")


def test_write_png_names_the_path(lib, tmp_path):
    path = str(tmp_path / "no_such_dir" / "a.png")
    rgb = np.zeros((2, 2, 3), np.uint8)
    rc = lib.kdpt_write_png(path.encode(), rgb.ctypes.data_as(C.POINTER(C.c_uint8)), 2, 2)
    _refused(lib, rc, KDPT_ERR_IO, path, "No such file")


def test_png_encode_names_w(lib):
    rgb = np.zeros((2, 2, 3), np.uint8)
    out, n = C.POINTER(C.c_uint8)(), C.c_size_t()
    rc = lib.kdpt_png_encode(rgb.ctypes.data_as(C.POINTER(C.c_uint8)), 0, 2, C.byref(out), C.byref(n))
    msg = _refused(lib, rc, KDPT_ERR_ARG, "kdpt_png_encode")
    assert re.search(rb"\bw\b", msg), msg


def test_python_exceptions_carry_the_message(lib, kdpt, tmp_path):
    with pytest.raises(kdpt.KdptError) as e:
        kdpt.SceneData.from_description(dataclasses.replace(load_fixture_scene("cornell"), res=(0, 8)))
    assert "res" in str(e.value) and "0 x 8" in str(e.value) and STALE.decode() not in str(e.value)
    assert lib.kdpt_set_tuning(None, STALE, 0.0) == KDPT_ERR_ARG
    path = str(tmp_path / "nowhere.txt")
    with pytest.raises(kdpt.KdptError) as e:
        kdpt.SceneData.from_files(path)
    assert "cannot open scene file " + path in str(e.value) and STALE.decode() not in str(e.value)


def test_device_kd_build_failure_names_its_call(lib):
    """A device ordinal no machine has: hipSetDevice refuses it (with or without a GPU), and the KD build's HIP_TRY
    says which call failed, at which stage."""
    v = np.array([[0, 1, 0, 1, 1, 0, 0, 2, 0]], np.float32)
    n, m = np.zeros_like(v), np.zeros(1, np.int32)
    nodes, tris, nn, nt, ms = C.c_void_p(), C.c_void_p(), C.c_int(), C.c_int(), C.c_double()
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    rc = lib.kdpt_build_kd_device(fp(v), fp(n), m.ctypes.data_as(C.POINTER(C.c_int)), 1, 13, 1 << 20, C.byref(nodes),
                                  C.byref(nn), C.byref(tris), C.byref(nt), C.byref(ms))
    _refused(lib, rc, KDPT_ERR_HIP, "hipSetDevice", "device KD build")


def test_a_successful_call_leaves_the_message_alone(lib):
    out = C.POINTER(C.c_uint8)()
    n = C.c_size_t()
    rgb = np.zeros((2, 2, 3), np.uint8)
    assert lib.kdpt_png_encode(rgb.ctypes.data_as(C.POINTER(C.c_uint8)), 2, 2, C.byref(out), C.byref(n)) == 0
    lib.kdpt_free(out)
    assert STALE in lib.kdpt_last_error()
