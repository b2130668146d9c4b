"""The bounce as units, pinned to the reference's own code: scatterRay (src/interactions.h:195-358), the box and
sphere tests (src/intersections.h:107-203) and shadeMaterial's body (src/pathtrace.cu:2318-2366), on 2^18 seeded
rows each (tests/kat_inputs.py scatter_inputs / geom_test_inputs / shade_inputs) that hold what a render of the
fixtures never produces: reflected and refracted directions of exactly +-z under softness > 0 (the soft lobe's
axis, and with it the new direction, is NaN), dots beyond +-1 into acosf, the internal-reflection decision at its
float / double boundary, normal components one ulp either side of SQRT_OF_ONE_THIRD, ior = 1, fractional and
negative hasReflective / hasRefractive / transmittance, sdepth at 1, nextafter(1), inf and NaN, |d|^2 = 1 +- 1e-6.

tests/golden/ref_pins.json "scatter" and "geom_tests" hold digests of what oracle/_ref/ref_bounce computes: the
reference's interactions.h (which includes intersections.h) compiled in place, host-only, with rocThrust's
engine (oracle/ref/ref_bounce_driver.cpp; tests/golden/make_ref_pins.py --bounce).  The oracle
(orc_scatter_array / orc_geom_test_array), the product's device source compiled for the host
(tests/native/bounce_host.cpp) and (-m gpu) the gfx950 code (kdpt_selftest_scatter) give those digests.  NaN
rows are compared like any other.

Which digest.  The geom tests produce no NaN on these rows: plain sha256 everywhere.  A scatter that ends in a
NaN direction carries that NaN through rotateVector's sums and products, and which operand's sign an x86
`addss` / `mulss` of two NaNs keeps is the compiler's choice of operand order, not the source's: the reference
binary (clang), the oracle (gcc, C) and the host-compiled product (g++) agree on every word that is not a NaN
and on where the NaNs are, and differ pairwise in the sign bit of NaNs in 4 671 of the 262 144 rows (5 057 end
in a NaN direction; measured on the CPU when the fixture was made).  So scatter is compared by
sha256_nan_canonical (every NaN as one pattern) and by sha256_nan_masked (NaN words zeroed), which together say:
same NaN positions, same bits everywhere else.  The plain scatter digest is recorded and checked only against
the reference binary itself.

shadeMaterial is a __global__ of src/pathtrace.cu and cannot be compiled in place, so `shade` is compared with
the oracle's restatement (orc_shade_array, the loop body of the oracle's shadeMaterial) only: host and gfx950,
bit for bit.
"""
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import kat_inputs as K
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
from conftest import HAS_REFERENCE, ROOT, TESTS

PINS = json.load(open(os.path.join(TESTS, "golden", "ref_pins.json")))
REF_BOUNCE = os.path.join(ROOT, "oracle", "_ref", "ref_bounce")
has_ref_bin = pytest.mark.skipif(not (HAS_REFERENCE and os.path.exists(REF_BOUNCE)),
                                 reason="reference sources / oracle/_ref/ref_bounce not present")
N = K.BOUNCE_N


def _masked(a):
    return K.sha256(K.nan_words_masked(a, a))


@pytest.fixture(scope="module")
def bounce_host():
    exe = os.path.join(ROOT, "build", "bounce_host")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    tmp = exe + f".{os.getpid()}"  # parallel workers may be running the previous one
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-I",
                    os.path.join(ROOT, "include"), os.path.join(TESTS, "native", "bounce_host.cpp"), "-o", tmp],
                   check=True)
    os.replace(tmp, exe)
    return exe


def _host(exe, mode, x, out):
    with tempfile.TemporaryDirectory() as tmp:
        xin, xout = os.path.join(tmp, "in"), os.path.join(tmp, "out")
        x.tofile(xin)
        out.tofile(xout)
        subprocess.run([exe, mode, str(len(x)), xin, xout], check=True, timeout=300)
        return np.fromfile(xout, np.float32).reshape(out.shape)


@pytest.fixture(scope="module")
def scatter_rows():
    x = K.scatter_inputs()
    x.setflags(write=False)
    return x


@pytest.fixture(scope="module")
def shade_rows():
    x = K.shade_inputs()
    x.setflags(write=False)
    return x


@pytest.fixture(scope="module")
def geom_rows(oracle):
    x = K.geom_test_inputs(oracle.geom_matrices)
    x.setflags(write=False)
    return x


@pytest.fixture(scope="module")
def shade_want(oracle, shade_rows):
    out = oracle.shade_array(shade_rows)
    out.setflags(write=False)
    return out


def test_scatter_oracle_and_host_device_source_equal_reference(oracle, bounce_host, scatter_rows):
    rec = PINS["scatter"]
    assert len(scatter_rows) == rec["n"] == N
    orc, leaf = oracle.scatter_array(scatter_rows)
    host = _host(bounce_host, "scatter", scatter_rows, np.zeros((N, K.SCATTER_OUT), np.float32))
    for name, out in (("oracle", orc), ("kdpt_scatter.h scatterRay compiled for the host", host)):
        assert K.sha256_nan_canonical(out) == rec["sha256_nan_canonical"], name
        assert _masked(out) == rec["sha256_nan_masked"], name
        assert int(np.isnan(out).sum()) == rec["nan_values"], name
    assert {str(c): int((leaf == c).sum()) for c in sorted(set(leaf.tolist()))} == rec["leaves"]


def test_geom_tests_oracle_and_host_device_source_equal_reference(oracle, bounce_host, geom_rows):
    rec = PINS["geom_tests"]
    assert len(geom_rows) == rec["n"] == N
    sent = K.sentinels(N, K.GEOM_TEST_OUT)
    orc = K.mask_missed(oracle.geom_test_array(geom_rows, sent.copy()))
    host = K.mask_missed(_host(bounce_host, "geom", geom_rows, sent))
    for name, out in (("oracle", orc), ("kdpt_geoms.h box / sphere tests compiled for the host", host)):
        assert K.sha256(out) == rec["sha256"], name
        assert K.sha256_nan_canonical(out) == rec["sha256_nan_canonical"], name
        assert int((out[:, 0] > 0).sum()) == rec["hits"], name


def test_shade_host_device_source_equals_oracle(bounce_host, shade_rows, shade_want):
    """shadeMaterial cannot be compiled in place (a __global__ of src/pathtrace.cu): against the oracle only."""
    host = _host(bounce_host, "shade", shade_rows, np.zeros((N, K.SHADE_OUT), np.float32))
    assert np.array_equal(host.view(np.uint32), shade_want.view(np.uint32))


def test_scatter_inputs_reach_every_leaf():
    """From the recorded counts: every leaf of scatterRay, with the soft lobe on and off where the leaf has
    one, holds at least 0.5 % of the rows; at most 10 % of the rows end in a NaN direction (and some do)."""
    rec = PINS["scatter"]
    want = set(K.SCATTER_LEAVES) | {c + K.SCATTER_SOFT for c in K.SCATTER_SOFT_LEAVES}
    assert {int(c) for c in rec["leaves"]} == want
    assert sum(rec["leaves"].values()) == rec["n"]
    for c, count in rec["leaves"].items():
        assert count >= 0.005 * rec["n"], (c, count)
    assert 0 < rec["nan_directions"] <= 0.10 * rec["n"]


def test_geom_test_inputs_hit_and_miss():
    rec = PINS["geom_tests"]
    assert 0.30 * rec["n"] <= rec["hits"] <= 0.95 * rec["n"]


def test_bounce_inputs_hold_the_edges(scatter_rows, shade_rows):
    """The rows named in the issue are there: exact +-z directions, normal components at and one ulp either
    side of SQRT_OF_ONE_THIRD, ior = 1, negative material fields, the raw seeding edges; t, emittance and sdepth
    kinds of the shade rows, bounces 1..16."""
    x, u = scatter_rows, scatter_rows.view(np.uint32)
    assert ((x[:, 3] == 0) & (x[:, 4] == 0) & (np.abs(x[:, 5]) == 1)).sum() > 0.05 * N
    s = K.SQRT_OF_ONE_THIRD
    for edge in (np.nextafter(s, np.float32(0)), s, np.nextafter(s, np.float32(1))):
        assert (np.abs(x[:, 11:14]) == edge).any(axis=1).sum() > 1000
    assert ((x[:, 15] != 0) & (x[:, 16] == 1)).sum() > 1000
    assert (x[:, 14] < 0).sum() > 1000 and (x[:, 15] < 0).sum() > 1000 and (x[:, 17:20] < 0).any(axis=1).sum() > 1000
    assert set(np.unique(x[:, 20]).tolist()) == {0.0, float(np.float32(0.02)), 0.5}
    assert set(np.unique(x[:, 6]).tolist()) == {0.0, 1.0}
    assert set(K.rng_inputs("raw")[:13].tolist()) <= set(u[:, 21].tolist())
    n2 = np.sum(x[:, 3:6].astype(np.float64) ** 2, axis=1)
    assert (n2 > 1 + 1e-6).sum() > 1000 and (n2 < 1 - 1e-6).sum() > 1000
    y = shade_rows
    t = y[:, 0]
    assert min((t > 0).sum(), ((t == 0) & ~np.signbit(t)).sum(), ((t == 0) & np.signbit(t)).sum(), (t == -1).sum(),
               np.isnan(t).sum()) > 0.05 * N
    assert min((y[:, 9] == 0).sum(), (y[:, 9] > 0).sum(), (y[:, 9] < 0).sum()) > 0.1 * N
    for v in (0.0, 0.5, 1.0, np.nextafter(np.float32(1), np.float32(2)), 2.0, np.inf):
        assert (y[:, 14] == np.float32(v)).sum() > 0.05 * N
    assert np.isnan(y[:, 14]).sum() > 0.05 * N
    assert set(y.view(np.int32)[:, 18].tolist()) == set(range(1, 17))
    assert set(np.unique(y[:, 13]).tolist()) == {0.0, 1.0}


@has_ref_bin
def test_scatter_fixture_matches_reference_binary(scatter_rows):
    import make_ref_pins as M
    with tempfile.TemporaryDirectory() as tmp:
        out = M.ref_scatter(scatter_rows, tmp)
    rec = PINS["scatter"]
    assert M.digests(out) == {k: rec[k] for k in ("n", "sha256", "sha256_nan_canonical", "sha256_nan_masked")}
    assert int(np.isnan(out[:, 3:6]).any(axis=1).sum()) == rec["nan_directions"]


@has_ref_bin
def test_geom_tests_fixture_matches_reference_binary(geom_rows):
    import make_ref_pins as M
    with tempfile.TemporaryDirectory() as tmp:
        out = M.ref_geom_tests(geom_rows, tmp)
    rec = PINS["geom_tests"]
    assert M.digests(out) == {k: rec[k] for k in ("n", "sha256", "sha256_nan_canonical", "sha256_nan_masked")}


def test_oracle_survives_the_degenerate_soft_mirror_rays(oracle):
    """The CPU side of tests/test_gpu_trace_rays.py's soft-mirror case: the rays that reflect to exactly +z off
    the probe tableau's mirror cube leave with a NaN direction when softness > 0 (with the reflected one when it
    is 0), hit nothing, and end after 2 segments each with a finite radiance."""
    import geoms
    o, d, deg = geoms.soft_mirror_rays()
    assert deg.sum() == len(o) // 4
    osc = oracle.OracleScene.from_description(geoms.geom_scene("far", res=(64, 64), depth=8))
    for softness in (0.0, 0.5):
        rad, st = osc.render_rays(o[deg], d[deg], 1, 1, softness=softness)
        assert np.isfinite(rad).all() and not rad.any()
        assert st.segments == 2 * int(deg.sum())
    # ... and the others do reach the light
    rad, _ = osc.render_rays(o, d, 1, 1, softness=0.5)
    assert np.isfinite(rad).all() and (rad[~deg].max(axis=1) > 0).mean() > 0.5


def _device(fn, x, width):
    out = np.zeros((len(x), width), np.float32)
    P = C.POINTER(C.c_float)
    rc = fn(np.ascontiguousarray(x).ctypes.data_as(P), len(x), out.ctypes.data_as(P))
    assert rc == 0
    return out


@pytest.mark.gpu
def test_device_scatter_equals_reference(kdpt, scatter_rows):
    """kdpt_selftest_scatter on gfx950: the reference's NaN positions and, outside them, its bits (a generated
    NaN carries gfx950's sign and payload, as in test_device_glm_equals_reference)."""
    out = _device(kdpt.load_library().kdpt_selftest_scatter, scatter_rows, K.SCATTER_OUT)
    rec = PINS["scatter"]
    assert K.sha256_nan_canonical(out) == rec["sha256_nan_canonical"]
    assert _masked(out) == rec["sha256_nan_masked"]


@pytest.mark.gpu
def test_device_shade_equals_oracle(kdpt, shade_rows, shade_want):
    out = _device(kdpt.load_library().kdpt_selftest_shade, shade_rows, K.SHADE_OUT)
    assert K.sha256_nan_canonical(out) == K.sha256_nan_canonical(shade_want)
    assert np.array_equal(K.nan_words_masked(out, out).view(np.uint32),
                          K.nan_words_masked(shade_want, shade_want).view(np.uint32))
