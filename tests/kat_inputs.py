"""TEST INFRASTRUCTURE: deterministic inputs of the reference-pinned known-answer tests.

The same seeded generators feed tests/golden/make_ref_pins.py (which runs the reference's own code,
compiled by oracle/ref, and commits digests of its outputs) and the CPU/GPU tests (which run the
oracle, the host-compiled device code and the gfx950 code on them).  numpy's PCG64 stream for a fixed
seed is stable across numpy versions.
"""
import hashlib

import numpy as np

GLM_FNS = {0: "intersectRayTriangle", 1: "normalize", 2: "reflect", 3: "refract", 4: "rotate_quat_vec3"}
GLM_IN = {0: 15, 1: 3, 2: 6, 3: 7, 4: 7}
GLM_OUT = {0: 4, 1: 3, 2: 3, 3: 3, 4: 3}
GLM_N = 1 << 20
# bary slots glm leaves unwritten keep this quiet-NaN payload (no arithmetic produces it)
SENTINEL_BITS = np.uint32(0x7FC0DEAD)


def _unit(rng, n):
    v = rng.normal(size=(n, 3))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


def glm_inputs(fn: int, n: int = GLM_N, seed: int = 20261016) -> np.ndarray:
    rng = np.random.default_rng(seed + 97 * fn)
    if fn == 0:  # rays at triangles: every exit of glm's test (det < eps, u/v out of range, t < 0, hit)
        v0 = rng.uniform(-1, 1, (n, 3))
        v1 = v0 + rng.uniform(-1, 1, (n, 3))
        v2 = v0 + rng.uniform(-1, 1, (n, 3))
        deg = rng.random(n) < 0.03  # degenerate (collinear) triangles
        v2[deg] = v0[deg] + (v1[deg] - v0[deg]) * rng.uniform(-2, 2, (deg.sum(), 1))
        b = rng.uniform(-0.3, 1.3, (n, 2))
        target = v0 + (v1 - v0) * b[:, :1] + (v2 - v0) * b[:, 1:]
        orig = rng.uniform(-3, 3, (n, 3))
        d = target - orig
        d[rng.random(n) < 0.1] *= -1.0  # triangle behind the ray
        rnd = rng.random(n) < 0.1
        d[rnd] = rng.normal(size=(rnd.sum(), 3))
        d = d / np.linalg.norm(d, axis=1, keepdims=True)
        axis0 = rng.random(n) < 0.02  # axis-aligned directions (zero components)
        d[axis0] = np.eye(3)[rng.integers(0, 3, axis0.sum())] * rng.choice([-1, 1], (axis0.sum(), 1))
        x = np.concatenate([orig, d, v0, v1, v2], axis=1)
    elif fn == 1:  # magnitudes from 1e-30 to 1e30, zeros, axis vectors
        v = rng.normal(size=(n, 3)) * (10.0 ** rng.uniform(-30, 30, (n, 1)))
        v[rng.random(n) < 0.01] = 0.0
        x = v
    elif fn == 2:
        x = np.concatenate([_unit(rng, n), _unit(rng, n) * rng.uniform(0.5, 1.5, (n, 1))], axis=1)
    elif fn == 3:  # eta around the reference's 1 / ior and ior (incl. total internal reflection)
        eta = rng.uniform(0.3, 2.5, (n, 1))
        x = np.concatenate([_unit(rng, n), _unit(rng, n), eta], axis=1)
    elif fn == 4:  # unit quaternions (w = cos a/2, xyz = axis sin a/2) as generateRayFromCamera builds
        a = rng.uniform(0, np.pi, (n, 1)).astype(np.float32)
        ax = _unit(rng, n)
        x = np.concatenate([np.cos(a / 2), ax * np.sin(a / 2), _unit(rng, n)], axis=1)
    else:
        raise ValueError(fn)
    return np.ascontiguousarray(x, np.float32)


def glm_sentinels(fn: int, n: int) -> np.ndarray:
    out = np.zeros((n, GLM_OUT[fn]), np.float32)
    out.view(np.uint32)[:] = SENTINEL_BITS
    return out


def geom_trs(seed: int = 7, n: int = 20000) -> np.ndarray:
    """translation / rotation (degrees) / scale triples: the scene files' kinds of values and random ones,
    incl. rotations about several axes, negative and tiny scales."""
    rng = np.random.default_rng(seed)
    t = rng.uniform(-20, 20, (n, 3))
    r = rng.uniform(-360, 360, (n, 3))
    r[: n // 4] = np.round(r[: n // 4] / 15.0) * 15.0  # the scene files' multiples of 15/45/90
    s = rng.uniform(0.01, 10, (n, 3)) * rng.choice([-1, 1], (n, 3), p=[0.05, 0.95])
    return np.ascontiguousarray(np.concatenate([t, r, s], axis=1), np.float32)


def images(seed: int = 3):
    """(name, float image HxWx3) inputs of the PNG/HDR writers: ragged sizes, values below 0, above 1,
    tiny and huge (RGBE exponent range), exact multiples of 1/255."""
    rng = np.random.default_rng(seed)
    out = []
    for (h, w) in ((1, 1), (3, 7), (64, 64), (5, 257), (96, 80)):
        im = rng.uniform(-0.2, 1.3, (h, w, 3))
        k = rng.random((h, w)) < 0.1
        im[k] = rng.integers(0, 256, (k.sum(), 3)) / 255.0
        big = rng.random((h, w)) < 0.05
        im[big] = 10.0 ** rng.uniform(-30, 30, (big.sum(), 3))
        out.append((f"rand_{h}x{w}", np.ascontiguousarray(im, np.float32)))
    return out


RNG_K = 8  # draws per engine: scatterRay's deepest branch (fake SSS + soft lobe) draws fewer


def rng_inputs(mode: str, seed: int = 62) -> np.ndarray:
    """Inputs of the RNG pin (tests/golden/make_ref_pins.py, oracle/ref/thrust_rng_driver.cpp):
    "seeded" (iter, index, depth) int32 rows for makeSeededRandomEngine (src/pathtrace.cu:62-66): the
    grid of small iterations x every depth 0..16 x the first/last pixels of 800^2 and 1600^2, plus random
    rows; "camera" iterations for engine(utilhash(iter)) (src/pathtrace.cu:334); "raw" uint32 seeds,
    incl. the seeding edge cases (0, multiples of m = 2^31 - 1, m +- 1, 2^32 - 1)."""
    rng = np.random.default_rng(seed)
    if mode == "seeded":
        it = np.arange(0, 33)
        idx = np.array([0, 1, 2, 63, 64, 799, 800, 639999, 640000 - 1, 2559999, 2 ** 21, 2 ** 22 - 1])
        d = np.arange(0, 17)
        grid = np.stack(np.meshgrid(it, idx, d, indexing="ij"), -1).reshape(-1, 3)
        n = 1 << 18
        rnd = np.stack([rng.integers(1, 1 << 22, n), rng.integers(0, 1 << 22, n), rng.integers(0, 17, n)], 1)
        return np.ascontiguousarray(np.concatenate([grid, rnd]), np.int32)
    if mode == "camera":
        return np.ascontiguousarray(np.concatenate([np.arange(0, 1 << 16), rng.integers(0, 1 << 31, 1 << 14)]),
                                    np.int32)
    if mode == "raw":
        m = 2 ** 31 - 1
        edge = [0, 1, 2, m - 1, m, m + 1, 2 * m - 1, 2 * m, 2 * m + 1, 2 ** 31, 2 ** 32 - 1, 48271, 16807]
        return np.ascontiguousarray(np.concatenate([edge, rng.integers(0, 1 << 32, 1 << 16, dtype=np.uint64)]),
                                    np.uint32)
    raise ValueError(mode)


def sha256(a: np.ndarray) -> str:
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def sha256_nan_canonical(a: np.ndarray) -> str:
    """sha256 with every NaN replaced by one bit pattern: IEEE 754 leaves a generated NaN's sign and
    payload open (x86 SSE makes 0xffc00000, gfx950 0x7fc00000); NaN positions still count."""
    b = np.ascontiguousarray(a, np.float32).copy()
    b.view(np.uint32)[np.isnan(b)] = np.uint32(0x7FC00000)
    return sha256(b)


# ---- the bounce: scatterRay, shade and the analytic geom tests as units (tests/test_bounce_pins.py) ----
# Records are rows of 32-bit words, float32 unless said otherwise; the reference driver
# (oracle/ref/ref_bounce_driver.cpp), the oracle (orc_*_array), the host-compiled product
# (tests/native/bounce_host.cpp) and the gfx950 kernels (kdpt_selftest_scatter / _shade) read the same rows.
BOUNCE_N = 1 << 18
# origin 0-2, direction 3-5, isinside 6 (0 / 1), sdepth 7, intersect 8-10, normal 11-13, hasReflective 14,
# hasRefractive 15, indexOfRefraction 16, transmittance 17-19, softness 20, seed 21 (uint32)
SCATTER_IN = 22
# origin 0-2, direction 3-5, isinside 6 (0 / 1), sdepth 7, the engine's next u01 draw 8
SCATTER_OUT = 9
# t 0, material colour 1-3, specular colour 4-6, hasReflective 7, hasRefractive 8, emittance 9,
# transmittance 10-12, enable_sss 13 (0 / 1), ray sdepth 14, path colour 15-17, remainingBounces 18 (int32)
SHADE_IN = 19
# path colour 0-2, remainingBounces 3 (int32)
SHADE_OUT = 4
# type 0 (int32: 0 sphere, 1 cube), transform / inverseTransform / invTranspose 1-48, origin 49-51,
# direction 52-54
GEOM_TEST_IN = 55
# t 0, hit point 1-3, normal 4-6 (point and normal: SENTINEL_BITS unless t > 0, see mask_missed)
GEOM_TEST_OUT = 7
SQRT_OF_ONE_THIRD = np.float32(0.5773502691896257645091487805019574556476)

# scatterRay's leaves, as orc_scatter_array numbers them; + SCATTER_SOFT when the soft lobe ran
SCATTER_LEAVES = {0: "transmittance: enter", 1: "transmittance: diffuse", 2: "refractive: internal reflection",
                  3: "refractive: internal reflection declined, diffuse", 4: "refractive: refract",
                  5: "refractive: refract declined, diffuse", 6: "refractive: Fresnel reflect", 7: "reflective: reflect",
                  8: "reflective: diffuse", 9: "diffuse"}
SCATTER_SOFT = 16
SCATTER_SOFT_LEAVES = (2, 4, 7)
N_MATERIAL_KINDS = 11


def _material_kinds(rng, kind):
    """hasReflective, hasRefractive, indexOfRefraction, transmittance[3] per row for the material kinds:
    0 diffuse, 1 mirror, 2 hasReflective 0.5, 3 glass 1.5, 4 glass with fractional reflect / refract and ior
    in (1, 2), 5 ior = 1, 6 transmittance > 0 with hasRefractive, 7 ... without, 8 negative hasReflective,
    9 negative hasRefractive, 10 transmittance with negative components (half of them with none > 0)."""
    n = len(kind)
    m = np.zeros((n, 6))
    m[:, 2] = 1.0
    m[kind == 1, 0] = 1.0
    m[kind == 2, 0] = 0.5
    m[kind == 3, :3] = (1.0, 1.0, 1.5)
    k = kind == 4
    m[k, 0], m[k, 1], m[k, 2] = rng.uniform(0, 1, k.sum()), rng.uniform(0.05, 1, k.sum()), rng.uniform(1, 2, k.sum())
    m[kind == 5, :3] = (1.0, 1.0, 1.0)
    m[kind == 6] = (0.0, 1.0, 1.5, 1.0, 0.7, 0.7)
    m[kind == 7] = (0.0, 0.0, 1.0, 1.0, 0.7, 0.7)
    k = kind == 8
    m[k, 0] = -rng.uniform(0.1, 1, k.sum())
    k = kind == 9
    m[k, 0], m[k, 1], m[k, 2] = rng.uniform(0, 1, k.sum()), -rng.uniform(0.1, 1, k.sum()), 1.5
    k = kind == 10
    tr = -rng.uniform(0.1, 1, (k.sum(), 3))
    some = rng.random(k.sum()) < 0.5
    tr[some, rng.integers(0, 3, some.sum())] = 0.5
    m[k, 3:] = tr
    m[k, 0] = rng.choice([0.0, 1.0], k.sum())
    return m


def _perp(rng, v):
    """A random unit vector perpendicular to each row of v."""
    p = np.cross(v, rng.normal(size=v.shape))
    return p / np.linalg.norm(p, axis=1, keepdims=True)


def scatter_inputs(n: int = BOUNCE_N, seed: int = 20261021) -> np.ndarray:
    """Rows for scatterRay (src/interactions.h:195-358).  The weights are chosen so that every leaf, with the
    soft lobe on and off, holds at least 0.5 % of the rows and at most 10 % end in a NaN direction
    (tests/test_bounce_pins.py asserts both from the reference's recorded counts)."""
    rng = np.random.default_rng(seed)
    f32 = np.float32
    mk = rng.choice(N_MATERIAL_KINDS, n, p=[.07, .10, .10, .17, .17, .06, .08, .06, .05, .07, .07])
    mat = _material_kinds(rng, mk)
    inside = rng.random(n) < 0.5
    # normals: random unit, +- an axis, components at nextafter(SQRT_OF_ONE_THIRD, +-)
    nk = rng.choice(3, n, p=[.6, .25, .15])
    nrm = _unit(rng, n).astype(np.float64)
    k = nk == 1
    nrm[k] = np.eye(3)[rng.integers(0, 3, k.sum())] * rng.choice([-1.0, 1.0], (k.sum(), 1))
    k = nk == 2
    edge = np.array([np.nextafter(SQRT_OF_ONE_THIRD, f32(0)), SQRT_OF_ONE_THIRD, np.nextafter(SQRT_OF_ONE_THIRD, f32(1))])
    nrm[k] = edge[rng.integers(0, 3, (k.sum(), 3))] * rng.choice([-1.0, 1.0], (k.sum(), 3))
    # directions: 0 random unit (most facing the normal, as a hit's are), 1 exactly +-z, 2 within 1e-4 of +-z,
    # 3 grazing the normal to 1e-4, 4 |d| = 1 +- 1e-6, 5 reflect(d, n) exactly +-z (axis-aligned normal),
    # 6 at the critical angle of the row's ior (the internal-reflection decision's boundary)
    dk = rng.choice(7, n, p=[.40, .05, .08, .10, .12, .07, .18])
    d = _unit(rng, n).astype(np.float64)
    face = (np.sum(d * nrm, axis=1) > 0) & (rng.random(n) < 0.8)
    d[face] *= -1.0
    zs = rng.choice([-1.0, 1.0], (n, 1))
    k = dk == 1
    d[k] = np.array([0.0, 0.0, 1.0]) * zs[k]
    k = dk == 2
    near = np.concatenate([rng.uniform(-1e-4, 1e-4, (k.sum(), 2)), np.ones((k.sum(), 1))], axis=1)
    d[k] = near / np.linalg.norm(near, axis=1, keepdims=True) * zs[k]
    k = dk == 3
    g = _perp(rng, nrm[k]) - nrm[k] / np.linalg.norm(nrm[k], axis=1, keepdims=True) * rng.uniform(-1e-4, 1e-4, (k.sum(), 1))
    d[k] = g / np.linalg.norm(g, axis=1, keepdims=True)
    k = dk == 5
    ax = rng.integers(0, 3, k.sum())
    sg = rng.choice([-1.0, 1.0], k.sum())
    nrm[k] = np.eye(3)[ax] * sg[:, None]
    d[k] = np.array([0.0, 0.0, 1.0]) * zs[k]  # n = +-z: d flips to -d; n = +-x, +-y: dot = 0, d stays
    k = dk == 6
    ior = np.where(mat[k, 2] > 1.0, mat[k, 2], 1.5)
    cosc = np.sqrt(1.0 - 1.0 / (ior * ior))  # inside: 1 - ior^2 (1 - cos^2) = 0
    cosc = cosc * (1.0 + rng.integers(-4, 5, k.sum()) * 2.0 ** -24)
    nn = nrm[k] / np.linalg.norm(nrm[k], axis=1, keepdims=True)
    d[k] = -cosc[:, None] * nn + np.sqrt(1.0 - cosc * cosc)[:, None] * _perp(rng, nn)
    inside[k] = rng.random(k.sum()) < 0.9
    k = (dk == 4) | ((dk == 2) & (rng.random(n) < 0.5))
    d[k] *= 1.0 + rng.choice([-1e-6, 1e-6], (k.sum(), 1))
    hit = rng.uniform(-5, 5, (n, 3))
    org = hit - d * rng.uniform(0.01, 10, (n, 1))
    soft = rng.choice([0.0, 0.02, 0.5], n)
    x = np.zeros((n, SCATTER_IN), f32)
    x[:, 0:3], x[:, 3:6], x[:, 6] = org, d, inside
    x[:, 7] = rng.choice([0.0, 0.3, 2.0], n)
    x[:, 8:11], x[:, 11:14], x[:, 14:20], x[:, 20] = hit, nrm, mat, soft
    seeds = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    edges = rng_inputs("raw")[:13]
    at = rng.choice(n, 13 * 64, replace=False)
    seeds[at] = np.tile(edges, 64)
    x.view(np.uint32)[:, 21] = seeds
    return np.ascontiguousarray(x)


def shade_inputs(n: int = BOUNCE_N, seed: int = 20261022) -> np.ndarray:
    """Rows for shadeMaterial's body (src/pathtrace.cu:2318-2366): t in {positive, +0, -0, -1, NaN}, emittance
    {0, > 0, < 0}, enable_sss 0 / 1, sdepth {0, 0.5, 1, nextafter(1, 2), 2, inf, NaN, random}, bounces 1..16,
    scatter_inputs' material kinds."""
    rng = np.random.default_rng(seed)
    f32 = np.float32
    mat = _material_kinds(rng, rng.integers(0, N_MATERIAL_KINDS, n))
    x = np.zeros((n, SHADE_IN), f32)
    tk = rng.choice(5, n, p=[.6, .1, .1, .1, .1])
    t = rng.uniform(1e-3, 50, n).astype(f32)
    t[tk == 1], t[tk == 2], t[tk == 3], t[tk == 4] = 0.0, -0.0, -1.0, np.nan
    x[:, 0] = t
    x[:, 1:4], x[:, 4:7] = rng.uniform(0, 1, (n, 3)), rng.uniform(0, 1, (n, 3))
    x[:, 7], x[:, 8] = mat[:, 0], mat[:, 1]
    ek = rng.choice(3, n, p=[.6, .2, .2])
    x[:, 9] = np.where(ek == 0, 0.0, np.where(ek == 1, 1.0, -1.0) * rng.uniform(0.5, 15, n))
    x[:, 10:13] = mat[:, 3:6]
    x[:, 13] = rng.integers(0, 2, n)
    sd = np.array([0.0, 0.5, 1.0, np.nextafter(f32(1), f32(2)), 2.0, np.inf, np.nan, -1.0], f32)
    sk = rng.integers(0, len(sd), n)
    x[:, 14] = np.where(sk == len(sd) - 1, rng.uniform(0, 1.5, n).astype(f32), sd[sk])
    x[:, 15:18] = rng.uniform(0, 2, (n, 3))
    x.view(np.int32)[:, 18] = rng.integers(1, 17, n)
    return np.ascontiguousarray(x)


def geom_test_trs(n: int = 4000, seed: int = 20261023) -> np.ndarray:
    """translation / rotation / scale triples of the geom tests: translations up to 5e4 (a quarter of them;
    the rest within 50), any rotation, scales 0.01 .. 10 (log-uniform)."""
    rng = np.random.default_rng(seed)
    t = rng.uniform(-50, 50, (n, 3))
    far = rng.random(n) < 0.25
    t[far] = rng.uniform(-5e4, 5e4, (far.sum(), 3))
    r = rng.uniform(-360, 360, (n, 3))
    r[: n // 4] = np.round(r[: n // 4] / 45.0) * 45.0
    s = 10.0 ** rng.uniform(-2, 1, (n, 3))
    return np.ascontiguousarray(np.concatenate([t, r, s], axis=1), np.float32)


def geom_test_inputs(matrices, n: int = BOUNCE_N, seed: int = 20261024) -> np.ndarray:
    """Rows for boxIntersectionTest / sphereIntersectionTest (src/intersections.h:107-203).  `matrices` maps
    geom_test_trs() to the (len, 48) float32 Geom matrices (oracle_lib.geom_matrices, itself pinned to the
    reference by ref_pins.json's "geom" section): every side is fed these same floats.  Origins on the
    object's surface, inside it, near it and 3 000 units away; directions aimed at the object (with a spread
    that makes part of them miss), axis-aligned, with zero components, and |d|^2 = 1 +- 1e-6."""
    rng = np.random.default_rng(seed)
    m = np.asarray(matrices(geom_test_trs()), np.float32).reshape(-1, 48)
    g = rng.integers(0, len(m), n)
    typ = rng.integers(0, 2, n).astype(np.int32)
    tr = m[g, :16].astype(np.float64).reshape(n, 4, 4)  # column-major: tr[i, c, r]

    def to_world(p):
        return np.einsum("ncr,nc->nr", tr[:, :3, :3], p) + tr[:, 3, :3]

    def surface(k):
        p = rng.uniform(-0.5, 0.5, (k, 3))
        ax = rng.integers(0, 3, k)
        p[np.arange(k), ax] = rng.choice([-0.5, 0.5], k)
        return p

    target = to_world(rng.uniform(-0.75, 0.75, (n, 3)))
    ok = rng.choice(4, n, p=[.2, .2, .4, .2])
    obj = rng.uniform(-0.5, 0.5, (n, 3))  # 1: inside
    k = ok == 0
    obj[k] = surface(k.sum())
    sph = k & (typ == 0)
    obj[sph] = 0.5 * obj[sph] / np.linalg.norm(obj[sph], axis=1, keepdims=True)
    k = ok >= 2  # near (a few object sizes away) and far (3 000 world units)
    obj[k] = _unit(rng, k.sum()) * rng.uniform(0.8, 6, (k.sum(), 1))
    org = to_world(obj)
    k = ok == 3
    org[k] = target[k] + _unit(rng, k.sum()) * 3000.0
    d = target - org
    degenerate = np.linalg.norm(d, axis=1) < 1e-12
    d[degenerate] = (1.0, 0.0, 0.0)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    dk = rng.choice(5, n, p=[.66, .08, .08, .08, .10])
    k = dk == 1
    d[k] = _unit(rng, k.sum())
    k = dk == 2
    d[k] = np.eye(3)[rng.integers(0, 3, k.sum())] * rng.choice([-1.0, 1.0], (k.sum(), 1))
    k = dk == 3
    d[k, rng.integers(0, 3, k.sum())] = 0.0
    d[k] /= np.maximum(np.linalg.norm(d[k], axis=1, keepdims=True), 1e-30)
    k = dk == 4
    d[k] *= 1.0 + rng.choice([-5e-7, 5e-7], (k.sum(), 1))
    x = np.zeros((n, GEOM_TEST_IN), np.float32)
    x.view(np.int32)[:, 0] = typ
    x[:, 1:49], x[:, 49:52], x[:, 52:55] = m[g], org, d
    return np.ascontiguousarray(x)


def sentinels(n: int, width: int) -> np.ndarray:
    out = np.zeros((n, width), np.float32)
    out.view(np.uint32)[:] = SENTINEL_BITS
    return out


def mask_missed(out: np.ndarray) -> np.ndarray:
    """A geom test that missed (t not > 0) leaves the hit point and the normal unwritten: SENTINEL_BITS there,
    on every side, before hashing."""
    out = np.ascontiguousarray(out, np.float32).copy()
    missed = ~(out[:, 0] > 0)
    out.view(np.uint32)[missed, 1:] = SENTINEL_BITS
    return out


def nan_words_masked(a: np.ndarray, nan_of: np.ndarray) -> np.ndarray:
    """a with the words that are NaN in nan_of zeroed: two results with the same NaN positions have equal
    plain digests once those words are masked out of both."""
    b = np.ascontiguousarray(a, np.float32).copy()
    b.view(np.uint32)[np.isnan(nan_of)] = 0
    return b
