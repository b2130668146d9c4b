"""The intersect kernel on adversarial triangle soups (tests/soups.py), on every tree route, against the CPU oracle.

The reference's closed meshes never produce these tree shapes: a root that is a leaf (the nodeIDs[-1] sink of the
compact visited state), a leaf of >= 8 192 triangles (no 32-byte packed record: the 64-byte "hbm-64B" route), a
tree too large for LDS ("hbm-32B" by default), exact ties in t between triangles of different normals and
materials (the big-leaf sweep's order-free fold must keep the reference's first-in-leaf-order winner, and its
last-in-leaf-order objMaterialIdx), clusters of zero area and of zero thickness under the masked exact cull.

Every context is 32 x 32 for the ray queries (kdpt_cast_rays: 2 048 seeded rays per soup, knobs flipped in place on
one context per soup and traversal); the oracle's records are computed once per (soup, traversal).
"""
import ctypes

import numpy as np
import pytest

import soups
from test_gpu_cast import _assert_equals_oracle, _assert_prims_are_the_hit_triangles

pytestmark = pytest.mark.gpu

NRAYS = 2048
# every route include/kdpt.h documents as exact (not "cull_exact" = 0 or a fixed "cull_margin": inexact for such
# meshes by design), with the value that puts the knob back
KNOBS = [{}, {"tree_format": 16}, {"tree_format": 32}, {"tree_global": 1}, {"cluster_cull": 0}, {"super_cull": 0},
         {"cluster_obb": 0}, {"cluster_slab": 0}, {"flat_obb": 0}, {"super_slab": 0}]
DEFAULTS = {"tree_format": 0, "tree_global": 0, "cluster_cull": 1, "super_cull": 1, "cluster_obb": 1, "cluster_slab": 1,
            "flat_obb": 1, "super_slab": 1}

# trace_config()["tree"] per (soup, knob), from setup_trace (kdpt_runtime.hip):
#  - rootleaf8200's one leaf holds 8 200 >= 8 192 triangles, so pack_nodes fails and there are no 32-byte records:
#    without the LDS routes ("tree_global"), or with the 16-byte LDS records excluded ("tree_format" = 32), the walk
#    reads the 64-byte NodeBare records;
#  - syn20000's 30 797 nodes x 16 B = 493 KB do not fit LDS in any format: the packed 32-byte records from HBM;
#  - the other big-leaf soups' trees (1 - 311 nodes) fit LDS in either format.  Under the masked exact cull the
#    super-cluster route is no candidate, so the 16-byte routes are the one-level ones.
WANT_TREE = {
    ("rootleaf8200", "tree_global"): ("hbm-64B",), ("rootleaf8200", "tree_format32"): ("hbm-64B",),
    ("syn20000", ""): ("hbm-32B",),
    **{(s, "tree_format16"): ("lds-16B-derived", "lds-16B-derived+hbm-clusters")
       for s in ("rootleaf8200", "growth", "coincident", "flat")},
    **{(s, "tree_format32"): ("lds-32B",) for s in ("growth", "coincident", "flat")},
}

_scenes, _rays, _oracle = {}, {}, {}


def _scene(kdpt, oracle, name):
    if name not in _scenes:
        desc = soups.soup_scene(name, res=(32, 32), depth=8)
        _scenes[name] = (desc, kdpt.SceneData.from_description(desc), oracle.OracleScene.from_description(desc))
    return _scenes[name]


def _soup_rays(kdpt, oracle, name):
    """(origins, directions as given to the cast, directions as traced: glm's normalize as the oracle pins it)."""
    if name not in _rays:
        desc, _, _ = _scene(kdpt, oracle, name)
        o, d = soups.soup_rays(name, desc)
        dn = oracle.glm_array(1, d, np.zeros((len(d), 3), np.float32))
        assert len(o) == NRAYS and not np.isnan(dn).any()
        _rays[name] = (o, d, dn)
    return _rays[name]


def _oracle_records(kdpt, oracle, name, hybrid):
    if (name, hybrid) not in _oracle:
        _, _, osc = _scene(kdpt, oracle, name)
        o, _, dn = _soup_rays(kdpt, oracle, name)
        L = oracle.lib()
        rec = np.zeros((len(o), 14), np.float64)
        fp, dp = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_double)
        for i in range(len(o)):
            L.orc_trace_ray(ctypes.byref(osc.s), o[i].ctypes.data_as(fp), dn[i].ctypes.data_as(fp), int(hybrid),
                            rec[i].ctypes.data_as(dp))
        assert not np.isnan(rec).any()
        _oracle[(name, hybrid)] = rec
    return _oracle[(name, hybrid)]


def _mask_sizes(pt):
    """(cells per face edge, clusters) of the context's direction masks, without copying the table."""
    n, ncl = ctypes.c_int(), ctypes.c_int()
    assert pt.lib.kdpt_cull_masks(pt._ctx, ctypes.byref(n), ctypes.byref(ncl), None) == 0
    return n.value, ncl.value


def _kinds(kdpt, rec):
    gi, obj = rec[:, 1].astype(np.int64), rec[:, 8].astype(np.int64)
    return {"none": int(np.sum(gi == -1)), "geom": int(np.sum((gi != -1) & (obj == 0))),
            "triangle": int(np.sum((gi != -1) & (obj != 0)))}


@pytest.mark.parametrize("short_stack", [1, 0], ids=["hybrid", "bare"])
@pytest.mark.parametrize("soup", soups.SOUPS)
def test_soup_cast_equals_oracle(kdpt, oracle, soup, short_stack):
    desc, sd, _ = _scene(kdpt, oracle, soup)
    o, d, dn = _soup_rays(kdpt, oracle, soup)
    rec = _oracle_records(kdpt, oracle, soup, short_stack)
    # ---- the oracle's records alone: the rays do reach the soup, the walls and (for coincident) every material.
    # Measured from the oracle, TRIANGLE / GEOM / NONE (the same for both walks except syn20000's): rootleaf8200
    # 1554 / 422 / 72, growth 194 / 1743 / 111, syn20000 1535 / 436 / 77 (bare 1568 / 404 / 76), coincident
    # 1085 / 855 / 108, flat 1302 / 602 / 144, one 709 / 1177 / 162, two 590 / 1277 / 181, three 400 / 1489 / 159,
    # identical 708 / 1169 / 171, signed_zero_root 666 / 1218 / 164; 148 - 470 of the 512 edge rays end on a triangle
    kinds = _kinds(kdpt, rec)
    assert kinds["triangle"] >= 150 and kinds["geom"] >= 50, kinds
    if soup == "coincident":
        tri = (rec[:, 1] != -1) & (rec[:, 8] != 0)
        assert len(np.unique(rec[tri, 9])) == 3, np.unique(rec[tri, 9])
    if soup == "syn20000":
        # the two walks end differently: by kind on 33 of the rays at least (the counts above); every triangle hit
        # differs in t anyway (the hit offsets, 1e-4 and 1e-5), so t alone would say nothing
        other = _oracle_records(kdpt, oracle, soup, 1 - short_stack)
        assert np.sum((other[:, 8] != 0) != (rec[:, 8] != 0)) >= 16
    base = None
    with kdpt.PathTracer(sd, kdpt.default_options(short_stack=short_stack)) as pt:
        if soup in soups.BIG:
            n, ncl = _mask_sizes(pt)
            assert pt.cull_margin()["cull_exact"] and n > 0 and ncl > 0, (pt.cull_margin(), n, ncl)
        for knobs in KNOBS:
            for k, v in knobs.items():
                pt.set_tuning(k, v)
            cfg = pt.trace_config()
            tag = "".join(f"{k}{v}" if k == "tree_format" else k for k, v in knobs.items())
            print(f"route {soup} short_stack={short_stack} {knobs}: {cfg['tree']} (masks {_mask_sizes(pt)})")
            want = WANT_TREE.get((soup, tag))
            if want is not None:
                assert cfg["tree"] in want, (soup, knobs, cfg)
            hits = pt.cast_rays(o, d, normalize=True)
            assert len(hits) == NRAYS and not np.any(hits["kind"] == kdpt.HIT_INVALID)
            if knobs == {}:
                base = hits.tobytes()
            try:
                _assert_equals_oracle(kdpt, hits, rec, desc)
            except AssertionError as e:
                raise AssertionError(f"{soup} {knobs} on {cfg['tree']}: differs from the oracle") from e
            if knobs == {}:
                ntri = _assert_prims_are_the_hit_triangles(kdpt, sd, hits, o, dn, short_stack)
                assert ntri == kinds["triangle"]
            if knobs == {"cluster_cull": 0}:
                # no cluster is culled on this route: where both routes fail the oracle alike the walk is at fault,
                # where only the default one does, the cull
                assert hits.tobytes() == base, "the culled and the unculled sweep disagree"
            for k in knobs:
                pt.set_tuning(k, DEFAULTS[k])
        assert pt.cast_rays(o, d, normalize=True).tobytes() == base  # the knobs are back


# (coincident as one shape: with three, a hit's material index is past the materials array, see
# test_shading_past_the_materials_is_refused)
RENDERS = [("rootleaf8200", {}, {}), ("coincident_one_shape", {}, {}), ("flat", {}, {}), ("growth", {}, {}),
           ("one", {}, {}), ("coincident_one_shape", {"short_stack": 0}, {}), ("rootleaf8200", {}, {"shade_fused": 0})]


@pytest.mark.parametrize("case", RENDERS, ids=["-".join([c[0], *c[1], *c[2]]) for c in RENDERS])
def test_soup_render_equals_oracle(kdpt, oracle, case):
    """Iterations 1 and 2 at 40 x 24, depth 8: the tie-broken normal and material through scatterRay and compaction
    (and iteration 2's sort by material): image bits and segment counts."""
    soup, opts, tuning = case
    desc = soups.soup_scene(soup, res=(40, 24), depth=8)
    with kdpt.PathTracer(kdpt.SceneData.from_description(desc), kdpt.default_options(**opts)) as pt:
        for k, v in tuning.items():
            pt.set_tuning(k, v)
        segs = []
        for it in (1, 2):
            pt.trace_iteration(it)
            segs.append(pt.stats().segments)
        img = pt.image()
    s = oracle.OracleScene.from_description(desc)
    o_img, o_segs = None, []
    for it in (1, 2):
        im, st = s.render(it, 1, **({"shortstack": opts["short_stack"]} if "short_stack" in opts else {}))
        o_segs.append(st.segments)
        o_img = im if o_img is None else (o_img + im)
    assert segs == o_segs
    assert np.array_equal(img.view(np.uint32), o_img.view(np.uint32)), \
        f"{int(np.sum(img.view(np.uint32) != o_img.view(np.uint32)))} values differ"
    assert o_img.any() and min(o_segs) > 40 * 24


@pytest.mark.parametrize("soup", ["rootleaf8200", "coincident_one_shape"])
def test_soup_counters_match_oracle(kdpt, oracle, soup):
    """AABB tests, triangle tests and hits of iteration 1 are the reference's, whatever the cull skips."""
    desc = soups.soup_scene(soup, res=(40, 24), depth=8)
    with kdpt.PathTracer(kdpt.SceneData.from_description(desc), kdpt.default_options()) as pt:
        got = pt.count_iteration(1)
    _, st = oracle.OracleScene.from_description(desc).render(1, 1)
    assert got == (st.aabb_tests, st.tri_tests, st.tri_hits)
    assert st.tri_hits > 1000 and st.tri_tests > st.segments  # (measured hits: 6 337 and 6 720)


# the counting intersect kernel (k_trace<.., COUNT = true, ..>) on the routes the two tests above do not take:
# (soup, knobs, WANT_TREE tag)
COUNT_ROUTES = [("rootleaf8200", {"tree_global": 1}, "tree_global"),
                ("rootleaf8200", {"tree_format": 16}, "tree_format16"), ("syn20000", {}, ""),
                ("growth", {"tree_format": 32}, "tree_format32"), ("growth", {"tree_format": 16}, "tree_format16")]
_oracle_counts = {}


@pytest.mark.parametrize("short_stack", [1, 0], ids=["hybrid", "bare"])
@pytest.mark.parametrize("route", COUNT_ROUTES, ids=["-".join([r[0], r[2] or "default"]) for r in COUNT_ROUTES])
def test_soup_counters_on_every_route(kdpt, oracle, route, short_stack):
    """Iteration 1's AABB tests, triangle tests and hits at 40 x 24, depth 8, are the oracle's on the hbm-64B, hbm-32B,
    lds-32B and lds-16B routes too, on both walks: the counters do not depend on where the tree is read from."""
    soup, knobs, tag = route
    desc = soups.soup_scene(soup, res=(40, 24), depth=8)
    with kdpt.PathTracer(kdpt.SceneData.from_description(desc), kdpt.default_options(short_stack=short_stack)) as pt:
        for k, v in knobs.items():
            pt.set_tuning(k, v)
        tree = pt.trace_config()["tree"]
        got = pt.count_iteration(1)
    if (soup, short_stack) not in _oracle_counts:
        _, st = oracle.OracleScene.from_description(desc).render(1, 1, shortstack=short_stack)
        _oracle_counts[(soup, short_stack)] = (st.aabb_tests, st.tri_tests, st.tri_hits)
    want = _oracle_counts[(soup, short_stack)]
    print(f"counters {soup} short_stack={short_stack} {knobs} on {tree}: {got} (oracle {want})")
    assert tree in WANT_TREE[(soup, tag)], (soup, knobs, tree)
    assert got == want
    assert want[2] > 0


def test_shading_past_the_materials_is_refused(kdpt, oracle):
    """`coincident` has three shapes.  The KD traversal reports material mtlIdx + num_materials - 1 for a triangle
    hit (src/pathtrace.cu:1142): 7, 8 and 9 here, in a materials array of 8.  The ray query only reports the
    number (test_soup_cast_equals_oracle); shading would read materials[8] and [9] and sort iteration 2's paths by
    keys past the key range -- in the reference too, so there is nothing to reproduce.  Every entry point that
    shades returns KDPT_ERR_UNSUPPORTED before it launches anything, the oracle refuses as well, and the context
    still answers ray queries afterwards."""
    desc, sd, osc = _scene(kdpt, oracle, "coincident")
    o, d, _ = _soup_rays(kdpt, oracle, "coincident")
    rec = _oracle_records(kdpt, oracle, "coincident", 1)
    assert len(desc.materials) + len(desc.shape_materials) == 8 and rec[:, 9].max() == 9
    with kdpt.PathTracer(sd, kdpt.default_options()) as pt:
        for call in (lambda: pt.trace_iteration(1), lambda: pt.count_iteration(1), lambda: pt.debug_paths(1, 0)):
            with pytest.raises(kdpt.KdptError, match="materials array"):
                call()
        with pytest.raises(kdpt.KdptError, match="materials array"):
            pt.trace_iterations(1, 2, pipeline=2, batch=1)
        pt.synchronize()
        _assert_equals_oracle(kdpt, pt.cast_rays(o, d, normalize=True), rec, desc)
    with pytest.raises(RuntimeError):
        osc.render(1, 1)
    # the brute-force kernel takes the material from the shapes' offsets instead: in range, and rendered
    with kdpt.PathTracer(sd, kdpt.default_options(enable_kd=0)) as pt:
        pt.trace_iteration(1)
        img, seg = pt.image(), pt.stats().segments
    ref, st = osc.render(1, 1, enable_kd=0)
    assert seg == st.segments and np.array_equal(img.view(np.uint32), ref.view(np.uint32))


def test_mask_resolution_overflow_is_rejected(kdpt, oracle):
    """syn20000 has 5 032 clusters: at 512 cells per face edge the table would hold 6 * 512^2 * 5 032 = 7.9e9 >=
    2^32 cells, past the kernel's 32-bit index (and 63 GB).  The knob is refused with the limit in the message,
    before the current masks are freed: their sizes stay and a cast still equals the oracle."""
    desc, sd, _ = _scene(kdpt, oracle, "syn20000")
    o, d, _ = _soup_rays(kdpt, oracle, "syn20000")
    rec = _oracle_records(kdpt, oracle, "syn20000", 1)
    with kdpt.PathTracer(sd, kdpt.default_options()) as pt:
        n, ncl = _mask_sizes(pt)
        assert n > 0 and ncl == 5032 and 6 * 512 * 512 * ncl >= 2 ** 32 > 6 * n * n * ncl
        with pytest.raises(kdpt.KdptError, match=r"2\^32"):
            pt.set_tuning("cull_mask_n", 512)
        assert _mask_sizes(pt) == (n, ncl) and pt.cull_margin()["cull_exact"]
        _assert_equals_oracle(kdpt, pt.cast_rays(o, d, normalize=True), rec, desc)
        # the largest resolution below the limit for this scene is still accepted ... at 5 032 clusters that is
        # n <= 377; a small one is rebuilt here (n = 8), and the cast stays the oracle's
        pt.set_tuning("cull_mask_n", 8)
        assert _mask_sizes(pt) == (8, ncl)
        _assert_equals_oracle(kdpt, pt.cast_rays(o, d, normalize=True), rec, desc)
