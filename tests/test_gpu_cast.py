"""Ray queries on the GPU (kdpt_cast_rays): every record against the CPU oracle's orc_trace_ray, bit for bit,
on every tree route; the rejected-ray rule; chunking; isolation from the render path; device pointers.

Every context is created at 32 x 32 (the resolution only sizes the render buffers: the query's chunks do not
depend on it).  Each scene's 2 048 rays and the oracle's records for them are computed once and shared.
"""
import ctypes

import numpy as np
import pytest

from kdtreepathtraceroptimization_amd.fixtures import load_fixture_scene

pytestmark = pytest.mark.gpu

RES = (32, 32)
NRAYS = 2048
NNORM = 1536  # rays [0, NNORM) are cast with normalize=True, the rest (the tracer's own rays) without
ROOM_LO, ROOM_HI = np.array([-5.0, 0.0, -5.0]), np.array([5.0, 10.0, 5.0])  # scenes/cornell.txt's box

# (id, scene key, knobs, trace_config()["tree"] to expect or None, assert cull_exact)
ROUTES = [
    ("dragon5", "dragon_5", {}, None, True),
    ("dragon5-fmt16", "dragon_5", {"tree_format": 16}, "lds-16B-derived", False),
    ("dragon5-global", "dragon_5", {"tree_global": 1}, None, False),
    ("ico6", "ico6", {}, "lds-16B-derived", False),
    ("ico7", "ico7", {}, "lds-16B-derived+hbm-clusters", False),
    ("ico7-margin", "ico7", {"cull_exact": 0}, "lds-16B-derived+supers", False),
    ("cornell", "cornell", {}, None, False),
]

_scenes, _rays, _oracle = {}, {}, {}


def _scene(kdpt, oracle, key):
    """(description, SceneData, OracleScene) of a scene key, built once."""
    if key not in _scenes:
        if key.startswith("ico"):
            from kdtreepathtraceroptimization_amd.meshes import attach_icosphere
            desc = attach_icosphere(load_fixture_scene("cornell", None, res=RES, depth=8), int(key[3:]))
        else:
            desc = load_fixture_scene("cornell", None if key == "cornell" else key, res=RES, depth=8)
        _scenes[key] = (desc, kdpt.SceneData.from_description(desc), oracle.OracleScene.from_description(desc))
    return _scenes[key]


def _unit(v):
    return v / np.sqrt(np.sum(v * v, axis=1))[:, None]


def _scene_rays(kdpt, oracle, key):
    """The scene's 2 048 rays (float32 origins and directions), from a seeded generator: [0, 512) camera rays of a
    32 x 16 grid, [512, 1024) random origins in the room with random unit directions, [1024, 1536) edge cases,
    [1536, 2048) the live rays after bounces 1 and 3 of iteration 1 (cast as they are, without normalisation)."""
    if key in _rays:
        return _rays[key]
    from kdtreepathtraceroptimization_amd.cast_cli import camera_rays
    desc, sd, _ = _scene(kdpt, oracle, key)
    rs = np.random.RandomState(20261019)
    f32 = np.float32

    def in_room(n):
        return rs.uniform(ROOM_LO + 0.05, ROOM_HI - 0.05, (n, 3))

    cam_sd = kdpt.SceneData.from_description(load_fixture_scene("cornell", None, res=(32, 16), depth=8))
    co, cd = camera_rays(cam_sd.camera_bytes())
    assert len(co) == 512
    ro, rd = in_room(512), _unit(rs.normal(size=(512, 3)))
    # ---- edge cases ----
    eo, ed = [], []
    d1 = _unit(rs.normal(size=(96, 3)))  # one zero component: 1 / d is infinite on that axis (the slow AABB path)
    d1[np.arange(96), rs.randint(0, 3, 96)] = 0.0
    eo.append(in_room(96)), ed.append(d1)
    d2 = np.zeros((96, 3))               # two zero components: axis-aligned
    d2[np.arange(96), rs.randint(0, 3, 96)] = rs.choice([-1.0, 1.0], 96)
    eo.append(in_room(96)), ed.append(d2)
    if desc.verts9 is not None:          # origins inside the mesh's root box
        v = np.asarray(desc.verts9, np.float64).reshape(-1, 3)
        lo, hi = v.min(0), v.max(0)
    else:
        lo, hi = np.array([-2.0, 0.0, -2.0]), np.array([2.0, 4.0, 2.0])
    eo.append(rs.uniform(lo, hi, (96, 3))), ed.append(_unit(rs.normal(size=(96, 3))))
    oo = rs.uniform(-1.0, 1.0, (64, 3)) * 4.0 + np.array([0.0, 5.0, 0.0])  # outside the room, pointing away
    side = rs.choice([-1.0, 1.0], 64)
    oo[:, 0] = side * rs.uniform(8.0, 30.0, 64)
    da = _unit(rs.normal(size=(64, 3)))
    da[:, 0] = side * np.abs(da[:, 0]) + side * 0.1
    eo.append(oo), ed.append(da)
    wo = in_room(64)                     # origins on a wall's plane (x = -5, x = 5, y = 0, z = -5 in turn)
    for k, (ax, val) in enumerate([(0, -5.0), (0, 5.0), (1, 0.0), (2, -5.0)]):
        wo[k::4, ax] = val
    eo.append(wo), ed.append(_unit(rs.normal(size=(64, 3))))
    eo.append(in_room(48)), ed.append(_unit(rs.normal(size=(48, 3))) * 1e-3)  # unnormalised directions
    eo.append(in_room(48)), ed.append(_unit(rs.normal(size=(48, 3))) * 1e3)
    eo, ed = np.concatenate(eo), np.concatenate(ed)
    assert len(eo) == 512
    # ---- the tracer's own rays: what iteration 1 traces at bounces 2 and 4 ----
    with kdpt.PathTracer(sd, kdpt.default_options()) as pt:
        p1, p3 = pt.debug_paths(1, 1), pt.debug_paths(1, 3)
    p1, p3 = p1[p1["remainingBounces"] > 0], p3[p3["remainingBounces"] > 0]
    n3 = min(256, len(p3))
    assert len(p1) > 0
    p1 = p1[rs.choice(len(p1), 512 - n3, replace=len(p1) < 512 - n3)]
    p3 = p3[rs.choice(len(p3), n3, replace=False)]
    po = np.concatenate([p1["origin"], p3["origin"]])
    pd = np.concatenate([p1["direction"], p3["direction"]])
    o = np.concatenate([co, ro.astype(f32), eo.astype(f32), po]).astype(f32)
    d = np.concatenate([cd, rd.astype(f32), ed.astype(f32), pd]).astype(f32)
    assert o.shape == d.shape == (NRAYS, 3)
    _rays[key] = (np.ascontiguousarray(o), np.ascontiguousarray(d))
    return _rays[key]


def _traced_dirs(oracle, d):
    """The directions the query traces: glm's normalize (as the oracle pins it) of [0, NNORM), the rest as given."""
    dn = d.copy()
    n = min(NNORM, len(d))
    out = np.zeros((n, 3), np.float32)
    dn[:n] = oracle.glm_array(1, np.ascontiguousarray(d[:n]), out)
    return dn


def _oracle_records(kdpt, oracle, key, hybrid):
    """orc_trace_ray's 14 doubles for each of the scene's rays, computed once per (scene, traversal)."""
    if (key, hybrid) in _oracle:
        return _oracle[(key, hybrid)]
    _, _, osc = _scene(kdpt, oracle, key)
    o, d = _scene_rays(kdpt, oracle, key)
    dn = _traced_dirs(oracle, d)
    L = oracle.lib()
    rec = np.zeros((len(o), 14), np.float64)
    fp, dp = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_double)
    for i in range(len(o)):
        L.orc_trace_ray(ctypes.byref(osc.s), o[i].ctypes.data_as(fp), dn[i].ctypes.data_as(fp), int(hybrid),
                        rec[i].ctypes.data_as(dp))
    _oracle[(key, hybrid)] = rec
    return rec


def _cast_scene_rays(pt, o, d):
    """The scene's rays through the context: [0, NNORM) with the normalize flag, the rest without."""
    a = pt.cast_rays(o[:NNORM], d[:NNORM], normalize=True)
    if len(o) <= NNORM:
        return a
    return np.concatenate([a, pt.cast_rays(o[NNORM:], d[NNORM:], normalize=False)])


def _bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def _assert_equals_oracle(kdpt, hits, rec, desc):
    """Bitwise: t, point and normal as float32 bit patterns; kind, geom index and material by value."""
    n = len(hits)
    rec = rec[:n]
    gi, obj = rec[:, 1].astype(np.int64), rec[:, 8].astype(np.int64)
    want_kind = np.where(gi == -1, kdpt.HIT_NONE, np.where(obj != 0, kdpt.HIT_TRIANGLE, kdpt.HIT_GEOM))
    bad = np.flatnonzero(hits["kind"] != want_kind)
    assert len(bad) == 0, (bad[:8], hits["kind"][bad[:8]], want_kind[bad[:8]])
    hit = want_kind != kdpt.HIT_NONE
    miss = hits[~hit]
    assert np.all(miss["t"] == -1) and np.all(miss["prim"] == -1) and np.all(miss["material"] == -1)
    assert not miss["point"].any() and not miss["normal"].any()
    h, r = hits[hit], rec[hit]
    assert np.array_equal(_bits(h["t"]), _bits(r[:, 0].astype(np.float32)))
    assert np.array_equal(_bits(h["point"]), _bits(r[:, 2:5].astype(np.float32)))
    assert np.array_equal(_bits(h["normal"]), _bits(r[:, 5:8].astype(np.float32)))
    geom = want_kind[hit] == kdpt.HIT_GEOM
    assert np.array_equal(h["prim"][geom], r[geom, 1].astype(np.int32))
    assert np.array_equal(h["material"][geom], np.asarray(desc.geom_material, np.int32)[h["prim"][geom]])
    assert np.array_equal(h["material"][~geom], r[~geom, 9].astype(np.int32))


def _assert_prims_are_the_hit_triangles(kdpt, sd, hits, o, dn, hybrid):
    """Every TRIANGLE record's prim, by a float64 Moller-Trumbore on scene.tris[prim]: the ray crosses that
    triangle and |t64 - t| <= 1e-4 max(1, t), the scale of the reference's own 1e-4 hit offsets.

    t64 is the record's quantity in float64: the reference's t_min of a triangle hit is not Moller-Trumbore's
    parameter but the distance from the origin to the hit point it hands to scatterRay, o + d t_mt + n 1e-4
    (1e-5 in traverseKDbare), n the interpolated normal.  Against the bare t_mt a head-on hit differs by the
    whole offset plus float rounding -- measured on the MI355X, cornell + dragon_5's 2 048 rays:
    max |t_mt - t| / max(1, t) = 1.00018e-4 -- so the bare parameter would leave the bound no room for rounding
    at t <= 1; both figures are printed.

    Crossing tolerance: the float test forms u = dot(s, p) / a with p = d x e2, a = dot(e1, p); the cross and
    dot products are each off by a few units of 2^-24 relative to |s||d||e2| and |e1||d||e2|, so
    |u - u64| <= 5 * 2^-24 (|s| / |e1| + |u|) / c with c = |a| / (|e1||e2|), and likewise v with |e2|.  The
    check allows 8 * 2^-23 (|s| / |e| + 1) / c, three times that."""
    sel = np.flatnonzero(hits["kind"] == kdpt.HIT_TRIANGLE)
    if len(sel) == 0:
        return 0
    tris = np.frombuffer(sd.tris_bytes(), dtype=np.dtype([("v", "<f4", (3, 3)), ("n", "<f4", (3, 3)), ("m", "<i4")]))
    prim = hits["prim"][sel]
    assert prim.min() >= 0 and prim.max() < len(tris)
    T = tris["v"][prim].astype(np.float64)  # [k, axis, vertex]: x1 x2 x3, y1 y2 y3, z1 z2 z3
    v0, v1, v2 = T[:, :, 0], T[:, :, 1], T[:, :, 2]
    oo, dd = o[sel].astype(np.float64), dn[sel].astype(np.float64)
    e1, e2 = v1 - v0, v2 - v0
    p = np.cross(dd, e2)
    a = np.sum(e1 * p, 1)
    s = oo - v0
    u = np.sum(s * p, 1) / a
    q = np.cross(s, e1)
    v = np.sum(dd * q, 1) / a
    t64 = np.sum(e2 * q, 1) / a
    ln = lambda x: np.sqrt(np.sum(x * x, 1))  # noqa: E731
    c = np.maximum(np.abs(a) / (ln(e1) * ln(e2)), 1e-300)
    eps = 8.0 * 2.0 ** -23
    tu, tv = eps * (ln(s) / ln(e1) + 1.0) / c, eps * (ln(s) / ln(e2) + 1.0) / c
    assert np.all(u >= -tu) and np.all(v >= -tv) and np.all(u + v <= 1.0 + tu + tv), \
        (float(np.min(u + tu)), float(np.min(v + tv)), float(np.max(u + v - tu - tv)))
    t_mt = t64
    N = tris["n"][prim].astype(np.float64)  # vertex normals, [k, axis, vertex]
    nrm = N[:, :, 0] * (1.0 - u - v)[:, None] + N[:, :, 1] * u[:, None] + N[:, :, 2] * v[:, None]
    nrm /= ln(nrm)[:, None]
    t64 = ln(dd * t_mt[:, None] + nrm * (1e-4 if hybrid else 1e-5))
    t = hits["t"][sel].astype(np.float64)
    err = np.abs(t64 - t) / np.maximum(1.0, t)
    print(f"triangle hits {len(sel)}: max |t64 - t| / max(1, t) = {err.max():.3e} "
          f"(against Moller-Trumbore's bare parameter: {(np.abs(t_mt - t) / np.maximum(1.0, t)).max():.5e})")
    assert np.all(err <= 1e-4), float(err.max())
    return len(sel)


@pytest.mark.parametrize("short_stack", [1, 0], ids=["hybrid", "bare"])
@pytest.mark.parametrize("route", ROUTES, ids=[r[0] for r in ROUTES])
def test_cast_equals_oracle(kdpt, oracle, route, short_stack):
    _, key, knobs, want_tree, want_exact = route
    desc, sd, _ = _scene(kdpt, oracle, key)
    o, d = _scene_rays(kdpt, oracle, key)
    rec = _oracle_records(kdpt, oracle, key, short_stack)
    with kdpt.PathTracer(sd, kdpt.default_options(short_stack=short_stack)) as pt:
        for k, v in knobs.items():
            pt.set_tuning(k, v)
        cfg = pt.trace_config()
        if want_tree is not None:
            assert cfg["tree"] == want_tree, cfg
        if want_exact:
            assert pt.cull_margin()["cull_exact"], pt.cull_margin()
        hits = _cast_scene_rays(pt, o, d)
        st = pt.cast_stats()
    assert len(hits) == NRAYS and st.rays == NRAYS
    assert not np.any(hits["kind"] == kdpt.HIT_INVALID)
    _assert_equals_oracle(kdpt, hits, rec, desc)
    counts = {k: int(np.sum(hits["kind"] == k)) for k in (kdpt.HIT_NONE, kdpt.HIT_GEOM, kdpt.HIT_TRIANGLE)}
    print(f"{route[0]} short_stack={short_stack}: {cfg['tree']}, kinds {counts}, traced {st.traced}")
    ntri = _assert_prims_are_the_hit_triangles(kdpt, sd, hits, o, _traced_dirs(oracle, d), short_stack)
    if key != "cornell":  # a kernel that only ever reports misses (or never a triangle) cannot pass
        assert min(counts.values()) >= 50, counts
        assert ntri == counts[kdpt.HIT_TRIANGLE] and 0 < st.traced <= NRAYS
    else:
        assert counts[kdpt.HIT_TRIANGLE] == 0 and st.traced == 0  # no OBJ: every ray ends in the first part


def test_cast_invalid_rays(kdpt, oracle):
    desc, sd, _ = _scene(kdpt, oracle, "dragon_5")
    # four waves of unit-length rays from the eye towards points inside the mesh's box: every one of them meets
    # the KD root box, so every one that is not rejected reaches the KD traversal
    rs = np.random.RandomState(5)
    v = np.asarray(desc.verts9, np.float64).reshape(-1, 3)
    mid, half = 0.5 * (v.min(0) + v.max(0)), 0.5 * (v.max(0) - v.min(0))
    o = np.broadcast_to(np.asarray(desc.eye, np.float32), (256, 3)).copy()
    d = _unit(rs.uniform(mid - 0.5 * half, mid + 0.5 * half, (256, 3)) - o.astype(np.float64)).astype(np.float32)
    with kdpt.PathTracer(sd, kdpt.default_options()) as pt:
        base = pt.cast_rays(o, d, normalize=False)
        assert not np.any(base["kind"] == kdpt.HIT_INVALID)
        assert pt.cast_stats().traced == len(o)
        need = 18 + 1 + 2  # NaN / +inf / -inf per component, a zero direction, two non-unit directions
        bad = np.sort(rs.choice(len(o), need, replace=False))
        for normalize in (True, False):
            oo, dd = o.copy(), d.copy()
            cases = [(arr, c, val) for arr in (oo, dd) for c in range(3) for val in (np.nan, np.inf, -np.inf)]
            for i, (arr, c, val) in zip(bad, cases):
                arr[i, c] = val
            used = len(cases)
            dd[bad[used]] = 0.0          # a zero direction
            used += 1
            if not normalize:
                dd[bad[used]] *= 2.0     # length 2: only the normalize flag makes it a ray
                dd[bad[used + 1]] *= np.float32(1.0 + 1e-5)  # dot(d, d) = 1 + 2e-5: outside the 1e-6 bound too
                used += 2
            rejected = np.sort(bad[:used])
            valid = np.setdiff1d(np.arange(len(o)), rejected)
            t0 = pt.cast_stats().traced
            hits = pt.cast_rays(oo, dd, normalize=normalize)
            t1 = pt.cast_stats().traced
            only_valid = pt.cast_rays(oo[valid], dd[valid], normalize=normalize)
            t2 = pt.cast_stats().traced
            r = hits[rejected]
            assert np.all(r["kind"] == kdpt.HIT_INVALID) and np.all(r["t"] == -1) and np.all(r["prim"] == -1)
            assert np.all(r["material"] == -1) and not r["point"].any() and not r["normal"].any()
            # the valid neighbours in the same waves: the bytes of the undisturbed cast
            assert hits[valid].tobytes() == only_valid.tobytes()
            if not normalize:
                assert hits[valid].tobytes() == base[valid].tobytes()
            # none of the rejected rays was traced; every other ray was
            assert t1 - t0 == t2 - t1 == len(o) - len(rejected), (t0, t1, t2)


def test_cast_sizes_and_chunks(kdpt, oracle):
    desc, sd, _ = _scene(kdpt, oracle, "dragon_5")
    o, d = _scene_rays(kdpt, oracle, "dragon_5")
    rec = _oracle_records(kdpt, oracle, "dragon_5", 1)
    with kdpt.PathTracer(sd, kdpt.default_options()) as pt:
        ref = pt.cast_rays(o[:1000], d[:1000])
        _assert_equals_oracle(kdpt, ref, rec, desc)
        with pytest.raises(kdpt.KdptError):
            pt.set_tuning("cast_chunk", 63)
        pt.set_tuning("cast_chunk", 256)
        for n in (0, 1, 63, 64, 65, 255, 256, 257, 1000):
            before = pt.cast_stats().rays
            got = pt.cast_rays(o[:n], d[:n])
            assert len(got) == n and got.tobytes() == ref[:n].tobytes(), n
            assert pt.cast_stats().rays == before + n
        pt.set_tuning("cast_chunk", 64)  # remade again: 16 chunks
        assert pt.cast_rays(o[:1000], d[:1000]).tobytes() == ref.tobytes()


def test_cast_leaves_render_state_alone(kdpt, oracle):
    desc, sd, _ = _scene(kdpt, oracle, "dragon_5")
    o, d = _scene_rays(kdpt, oracle, "dragon_5")
    with kdpt.PathTracer(sd, kdpt.default_options()) as pt:
        ref_hits = pt.cast_rays(o[:1000], d[:1000])
        for it in (1, 2, 3):
            pt.trace_iteration(it)
        ref_img, ref_seg = pt.image(), pt.stats().total_segments
    with kdpt.PathTracer(sd, kdpt.default_options()) as pt:
        pt.trace_iteration(1)
        pt.trace_iteration(2)
        s0 = pt.stats()
        hits = pt.cast_rays(o[:1000], d[:1000])
        s1 = pt.stats()
        assert (s1.total_segments, s1.iterations, s1.segments) == (s0.total_segments, s0.iterations, s0.segments)
        assert hits.tobytes() == ref_hits.tobytes()
        pt.trace_iteration(3)
        assert pt.stats().total_segments == ref_seg and pt.stats().iterations == 3
        assert np.array_equal(pt.image().view(np.uint32), ref_img.view(np.uint32))
    # around pipelined frames, with no synchronize between the enqueue and the cast: the cast waits
    with kdpt.PathTracer(sd, kdpt.default_options()) as pt:
        pt.render_frames(0, 1, 32, pipeline=4, batch=8)
        pt.synchronize()
        frame_img, frame_seg = pt.image(), pt.stats().total_segments
    with kdpt.PathTracer(sd, kdpt.default_options()) as pt:
        pt.render_frames(0, 1, 32, pipeline=4, batch=8)
        hits = pt.cast_rays(o[:1000], d[:1000])
        assert hits.tobytes() == ref_hits.tobytes()
        pt.synchronize()
        assert pt.stats().total_segments == frame_seg and pt.stats().iterations == 32
        assert np.array_equal(pt.image().view(np.uint32), frame_img.view(np.uint32))


def test_cast_device_pointers(kdpt, oracle):
    import torch
    desc, sd, _ = _scene(kdpt, oracle, "dragon_5")
    o, d = _scene_rays(kdpt, oracle, "dragon_5")
    o, d = o[:1000], d[:1000]
    dev = torch.device("cuda", 0)
    with kdpt.PathTracer(sd, kdpt.default_options(), device=0) as pt:
        pt.set_tuning("cast_chunk", 384)  # three chunks, the last one partial
        host = pt.cast_rays(o, d)
        to, td = torch.from_numpy(o).to(dev), torch.from_numpy(d).to(dev)
        out = torch.zeros(len(o) * 40, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize(dev)
        pt.cast_rays_ptr(to.data_ptr(), td.data_ptr(), len(o), out.data_ptr())
        assert out.cpu().numpy().tobytes() == host.tobytes()
        # mixed: device inputs, host output
        mixed = np.zeros(len(o), kdpt.RAY_HIT_DTYPE)
        pt.cast_rays_ptr(to.data_ptr(), td.data_ptr(), len(o), mixed.ctypes.data)
        assert mixed.tobytes() == host.tobytes()


def test_cast_cli_writes_the_passes(kdpt, tmp_path, capsys):
    """The command-line tool end to end on scene and OBJ files: --camera writes the depth / normal / primitive
    passes of the camera's pinhole rays, --rays the records of a ray file; both equal cast_rays on the same rays."""
    import json
    from kdtreepathtraceroptimization_amd import cast_cli
    from kdtreepathtraceroptimization_amd.meshes import write_obj
    from scene_text import write_scene_text
    W, H = 48, 40
    scene = write_scene_text("cornell", str(tmp_path / "cornell.txt"))
    obj = str(tmp_path / "ico.obj")
    write_obj(obj, 3)
    base = str(tmp_path / "pass")
    assert cast_cli.main([scene, obj, "--camera", "--res", str(W), str(H), "--out", base]) == 0
    info = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    sd = kdpt.SceneData.from_files(scene, obj, res=(W, H))
    o, d = cast_cli.camera_rays(sd.camera_bytes())
    with kdpt.PathTracer(sd, kdpt.default_options()) as pt:
        want = pt.cast_rays(o, d)
        depth, normal, prim = (np.load(base + s) for s in (".depth.npy", ".normal.npy", ".prim.npy"))
        assert depth.shape == (H, W) and normal.shape == (H, W, 3) and prim.shape == (H, W, 2)
        assert np.array_equal(_bits(depth.ravel()), _bits(want["t"]))
        assert np.array_equal(_bits(normal.reshape(-1, 3)), _bits(want["normal"]))
        assert np.array_equal(prim.reshape(-1, 2), np.stack([want["kind"], want["prim"]], -1))
        assert info["n"] == W * H and info["invalid"] == 0
        assert info["hits"] == {"none": int(np.sum(want["kind"] == 0)), "geom": int(np.sum(want["kind"] == 1)),
                                "triangle": int(np.sum(want["kind"] == 2))}
        assert info["hits"]["triangle"] > 0 and info["hits"]["geom"] > 0
        rays = np.concatenate([o, d * np.float32(3.0)], 1)[::7].copy()  # unnormalised on purpose
        rays[5, 3:] = 0.0  # one zero direction: rejected
        np.save(str(tmp_path / "rays.npy"), rays)
        out = str(tmp_path / "hits.npy")
        assert cast_cli.main([scene, obj, "--rays", str(tmp_path / "rays.npy"), "--res", str(W), str(H), "--out",
                              out, "--chunk", "64"]) == 0
        info = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
        got = np.load(out)
        assert got.dtype == kdpt.RAY_HIT_DTYPE and info["n"] == len(rays) and info["invalid"] == 1
        assert got[5]["kind"] == kdpt.HIT_INVALID
        assert got.tobytes() == pt.cast_rays(rays[:, :3], rays[:, 3:]).tobytes()


@pytest.mark.parametrize("opts", [{"enable_kd": 0}, {"viz_kd": 1}], ids=["brute", "viz"])
def test_cast_unsupported_contexts(kdpt, oracle, opts):
    desc = load_fixture_scene("cornell", "sphere_low_1", res=RES, depth=8)
    sd = kdpt.SceneData.from_description(desc)
    o = np.array([[0, 5, 10.5]], np.float32)
    d = np.array([[0, 0, -1]], np.float32)
    out = np.zeros(1, kdpt.RAY_HIT_DTYPE)
    with kdpt.PathTracer(sd, kdpt.default_options(**opts)) as pt:
        rc = pt.lib.kdpt_cast_rays(pt._ctx, o.ctypes.data, d.ctypes.data, 1, kdpt.CAST_NORMALIZE, out.ctypes.data)
        assert rc == -3  # KDPT_ERR_UNSUPPORTED
        assert b"enable_kd" in pt.lib.kdpt_last_error()
        with pytest.raises(kdpt.KdptError):
            pt.cast_rays(o, d)
