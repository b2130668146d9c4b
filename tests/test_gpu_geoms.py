"""The analytic-geom path on adversarial scenes (tests/geoms.py) against the CPU oracle, bit for bit: ray queries on
every scene (the nearest-first loop, the skip test, ties, origins inside, far away and at 1e5), renders through every
shading route (the unstaged fused kernels of scenes with 9 geoms or 33 / 64 materials, the bare-walk k_shade
variants, analytic refraction), path state with 64 sort keys, and the counting intersect kernel on the two cluster
routes.

Contexts are 32 x 32 for the queries and 40 x 24 for the renders; each scene's rays and the oracle's records and
images are computed once and shared.
"""
import ctypes

import numpy as np
import pytest

import geoms
from test_gpu_cast import _assert_equals_oracle

pytestmark = pytest.mark.gpu

_scenes, _rays, _records, _renders = {}, {}, {}, {}


def _scene(kdpt, oracle, name, res=(32, 32)):
    key = (name, res)
    if key not in _scenes:
        desc = geoms.geom_scene(name, res=res, depth=8)
        _scenes[key] = (desc, kdpt.SceneData.from_description(desc), oracle.OracleScene.from_description(desc))
    return _scenes[key]


def _scene_rays(oracle, name, desc):
    """(origins, directions as given to the cast, directions as traced, rays cast with the normalize flag): the
    scene's 2 048 rays, then for `far` and `translated` the 512 fixture rays (unit length, cast as they are)."""
    if name not in _rays:
        o, d = geoms.geom_rays(name, desc)
        dn = d.copy()
        dn[:geoms.NNORM] = oracle.glm_array(1, np.ascontiguousarray(d[:geoms.NNORM]),
                                            np.zeros((geoms.NNORM, 3), np.float32))
        if name in ("far", "translated"):
            fo, fd = geoms.load_fixture_rays(name)
            o, d, dn = np.concatenate([o, fo]), np.concatenate([d, fd]), np.concatenate([dn, fd])
        assert not np.isnan(dn).any()
        _rays[name] = (np.ascontiguousarray(o), np.ascontiguousarray(d), np.ascontiguousarray(dn), geoms.NNORM)
    return _rays[name]


def _oracle_records(oracle, name, osc, o, dn, hybrid):
    if (name, hybrid) not in _records:
        L = oracle.lib()
        rec = np.zeros((len(o), 14), np.float64)
        fp, dp = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_double)
        for i in range(len(o)):
            L.orc_trace_ray(ctypes.byref(osc.s), o[i].ctypes.data_as(fp), dn[i].ctypes.data_as(fp), int(hybrid),
                            rec[i].ctypes.data_as(dp))
        assert not np.isnan(rec).any()
        _records[(name, hybrid)] = rec
    return _records[(name, hybrid)]


@pytest.mark.parametrize("short_stack", [1, 0], ids=["hybrid", "bare"])
@pytest.mark.parametrize("scene", geoms.SCENES)
def test_geom_cast_equals_oracle(kdpt, oracle, scene, short_stack):
    desc, sd, osc = _scene(kdpt, oracle, scene)
    o, d, dn, nnorm = _scene_rays(oracle, scene, desc)
    rec = _oracle_records(oracle, scene, osc, o, dn, short_stack)
    # ---- the oracle's records alone: the rays reach the geoms, and the scene makes its point ----
    gi, obj = rec[:, 1].astype(np.int64), rec[:, 8].astype(np.int64)
    on_geom = (gi != -1) & (obj == 0)
    assert np.sum(on_geom) >= 150, int(np.sum(on_geom))
    won = np.bincount(gi[on_geom], minlength=len(desc.geom_type))
    print(f"{scene} short_stack={short_stack}: winners {won.tolist()}, triangles {int(np.sum(obj != 0))}, "
          f"none {int(np.sum(gi == -1))}")
    if scene == "coplanar":
        # 3 == 4 and 5 == 6 exactly: the lower index wins every tie, and its material (not the copy's) is reported
        assert won[3] >= 20 and won[5] >= 20 and won[4] == 0 and won[6] == 0, won
        gm = np.asarray(desc.geom_material)
        assert gm[3] != gm[4] and gm[5] != gm[6]
        mats = set(gm[gi[on_geom]].tolist())
        assert gm[3] in mats and gm[5] in mats
    if scene == "nine":
        assert won[8] >= 20, won
    if scene in ("glass", "tilted+mesh"):
        # the mesh is hidden inside the glass sphere (behind the geoms in tilted+mesh): few rays end on it, but
        # the scene has a KD tree, so prep_ray's root-box test decides which rays walk it
        assert np.sum(obj != 0) >= 1
    with kdpt.PathTracer(sd, kdpt.default_options(short_stack=short_stack)) as pt:
        hits = np.concatenate([pt.cast_rays(o[:nnorm], d[:nnorm], normalize=True),
                               pt.cast_rays(o[nnorm:], d[nnorm:], normalize=False)])
        traced = pt.cast_stats().traced
    assert len(hits) == len(o) and not np.any(hits["kind"] == kdpt.HIT_INVALID)
    assert (traced > 0) == (desc.verts9 is not None)
    _assert_equals_oracle(kdpt, hits, rec, desc)


RENDER_SCENES = ["tilted", "nested", "glass", "nine", "mats33", "mats64"]
# (id, options, tuning): the fused batch kernel, the fused kernel per iteration, k_shade with compaction, k_shade alone
RENDER_ROUTES = [("default", {}, {}), ("nobatch", {}, {"shade_batch": 0}), ("unfused", {}, {"shade_fused": 0}),
                 ("nocompact", {"compaction": 0}, {})]
UNSTAGED = ("nine", "mats33", "mats64")


def _oracle_render(oracle, scene, short_stack, compaction):
    """(image of iterations 1 + 2, segments of each, paths with isinside set at some bounce of either) at 40 x 24."""
    key = (scene, short_stack, compaction)
    if key not in _renders:
        s = oracle.OracleScene.from_description(geoms.geom_scene(scene, res=(40, 24), depth=8))
        img, segs = None, []
        for it in (1, 2):
            im, st = s.render(it, 1, shortstack=short_stack, compaction=compaction)
            segs.append(st.segments)
            img = im if img is None else (img + im)
        inside = set()
        if scene == "glass":
            for it in (1, 2):
                for depth in range(8):
                    p = s.paths_after(it, depth, shortstack=short_stack, compaction=compaction)
                    inside |= {(it, int(i)) for i in p["pixelIndex"][p["isinside"] != 0]}
        _renders[key] = (img, segs, len(inside))
    return _renders[key]


@pytest.mark.parametrize("short_stack", [1, 0], ids=["hybrid", "bare"])
@pytest.mark.parametrize("route", RENDER_ROUTES, ids=[r[0] for r in RENDER_ROUTES])
@pytest.mark.parametrize("scene", RENDER_SCENES)
def test_geom_render_equals_oracle(kdpt, oracle, scene, route, short_stack):
    """Iterations 1 and 2 at 40 x 24, depth 8: image bits and segment counts, through each shading route."""
    _, opts, tuning = route
    desc = geoms.geom_scene(scene, res=(40, 24), depth=8)
    o_img, o_segs, n_inside = _oracle_render(oracle, scene, short_stack, opts.get("compaction", 1))
    assert o_img.any() and min(o_segs) > 40 * 24, o_segs
    if scene == "glass":
        assert n_inside >= 50, n_inside  # paths travelling inside a refractive geom or the mesh
    with kdpt.PathTracer(kdpt.SceneData.from_description(desc),
                         kdpt.default_options(short_stack=short_stack, **opts)) as pt:
        for k, v in tuning.items():
            pt.set_tuning(k, v)
        assert pt.trace_config()["shade_staged"] == (scene not in UNSTAGED)
        segs = []
        for it in (1, 2):
            pt.trace_iteration(it)
            segs.append(pt.stats().segments)
        img = pt.image()
    assert segs == o_segs
    assert np.array_equal(img.view(np.uint32), o_img.view(np.uint32)), \
        f"{int(np.sum(img.view(np.uint32) != o_img.view(np.uint32)))} values differ"


@pytest.mark.parametrize("stop_depth", [0, 2])
@pytest.mark.parametrize("scene", ["glass", "mats64"])
def test_geom_path_state(kdpt, oracle, scene, stop_depth):
    """Iteration 2's path array after bounce d (compacted, then sorted by material: 64 keys on mats64; glass: the
    refracted rays and isinside): the oracle's order and bits."""
    desc = geoms.geom_scene(scene, res=(40, 24), depth=8)
    with kdpt.PathTracer(kdpt.SceneData.from_description(desc), kdpt.default_options()) as pt:
        g = pt.debug_paths(2, stop_depth)
    p = oracle.OracleScene.from_description(desc).paths_after(2, stop_depth)
    assert len(p) > 100 and len(g) == len(p)
    if scene == "mats64" and stop_depth == 0:
        # every geom's material is a sort key here; the light's (0) ends its paths, which are compacted away (the
        # render test's non-zero image is those hits)
        assert sorted(np.unique(p["materialIdHit"]).tolist()) == list(range(1, 64))
    for f in ("pixelIndex", "remainingBounces", "materialIdHit", "isinside"):
        assert np.array_equal(g[f], p[f]), f
    for f in ("origin", "direction", "color"):
        assert np.array_equal(np.ascontiguousarray(g[f]).view(np.uint32), np.ascontiguousarray(p[f]).view(np.uint32)), f


@pytest.mark.parametrize("knobs,tree", [({}, "lds-16B-derived+hbm-clusters"), ({"cull_exact": 0}, "lds-16B-derived+supers")],
                         ids=["masked", "supers"])
def test_counters_on_the_cluster_routes(kdpt, oracle, knobs, tree):
    """The counting intersect kernel on the two routes whose leaves' clusters stay in HBM (a level-7 icosphere at
    32 x 32): iteration 1's AABB tests, triangle tests and hits are the oracle's."""
    import test_gpu_cast
    desc, sd, osc = test_gpu_cast._scene(kdpt, oracle, "ico7")
    with kdpt.PathTracer(sd, kdpt.default_options()) as pt:
        for k, v in knobs.items():
            pt.set_tuning(k, v)
        assert pt.trace_config()["tree"] == tree
        got = pt.count_iteration(1)
    if "ico7" not in _renders:
        _, st = osc.render(1, 1)
        _renders["ico7"] = (st.aabb_tests, st.tri_tests, st.tri_hits)
    assert got == _renders["ico7"]
    assert _renders["ico7"][2] > 0
