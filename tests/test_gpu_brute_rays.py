"""GPU: chosen rays through the brute-force intersect kernel (enable_kd = 0, k_brute), against the CPU oracle.

kdpt_cast_rays refuses brute contexts, so the rays go through kdpt_trace_rays (path traced: radiance bits and segment
counts) and are compared with the oracle's render_rays, the reference's bounce loop started from the same rays.

  - Adversarial rays from the host differential (tests/native/brute_diff.cpp --emit, tests/test_brute_diff.py): 4 096
    per fixture mesh, first those that need exactness -- the reference's winner is a triangle whose 64-triangle
    chunk box the ray misses at the box coefficient 1e-3 the chunk cull once ran at, so a kernel that culled chunks
    at that coefficient would lose the hit.  The test asserts how many there are, so it cannot pass vacuously.
  - The same rays with "cluster_cull" = 0 (no chunk cull at all): equal bits, the in-product A/B.
  - Shape plumbing on the soup shapes_ragged (5 shapes of 1, 63, 64, 65, 130 triangles): chunks straddle shape
    boundaries, and with use_bbox the rays of one wave disagree about shape 0's bbox, which sends the wave through
    the divergent-`iterator` branch with more than 64 triangles and the reference's lagging `iterator`.
  - KD contexts: the seeded soup rays of tests/test_gpu_soups.py through kdpt_trace_rays on a default context.
"""
import numpy as np
import pytest

import brute_diff_lib as bd
import soups

pytestmark = pytest.mark.gpu

NRAYS = 4096
# (lines, seed, rays that must need exactness).  The rate per line of the rounding-targeted generator is about
# 3e-3 (sphere_low_1), 5e-5 (stanford_bunny) and 3e-7 (dragon_5) once the origin must lie inside the room in front of
# the triangle; of seeds 1 .. 9 at 4 * 10^6 lines, dragon_5 yields 0 for 1, 3, 4, 5 and 7 and two rays for seed 6.
EMIT = {"sphere_low_1": (1_000_000, 7, 256), "stanford_bunny": (8_000_000, 7, 256), "dragon_5": (4_000_000, 6, 1)}

_rays, _ctx_scene, _oracle = {}, {}, {}


@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    return tmp_path_factory.mktemp("brute_rays")


def _adversarial(workdir, mesh):
    if mesh not in _rays:
        lines, seed, _ = EMIT[mesh]
        _rays[mesh] = bd.emit_rays(bd.scene_file(mesh, workdir), lines, seed, NRAYS, str(workdir / f"{mesh}.rays"))
    return _rays[mesh]


def _scene(kdpt, oracle, name, res):
    if (name, res) not in _ctx_scene:
        desc = bd.scene_desc(name, res=res)
        _ctx_scene[(name, res)] = (desc, kdpt.SceneData.from_description(desc), oracle.OracleScene.from_description(desc))
    return _ctx_scene[(name, res)]


def _oracle_rays(osc, key, o, d, it, **opts):
    """render_rays of iteration `it`, computed once per key and left unchanged."""
    k = (key, it, tuple(sorted(opts.items())))
    if k not in _oracle:
        rad, st = osc.render_rays(o, d, it, 1, **opts)
        rad.setflags(write=False)
        _oracle[k] = (rad, int(st.segments))
    return _oracle[k]


def _assert_rays_equal(pt, rad_ref, seg_ref, o, d, it):
    rad = pt.trace_rays(o, d, first_iter=it, count=1, normalize=False)
    assert not np.isnan(rad).any(), "a ray was rejected"
    diff = np.flatnonzero((rad.view(np.uint32) != rad_ref.view(np.uint32)).any(axis=1))
    assert len(diff) == 0, f"{len(diff)} rays differ, first {diff[:8]}: {rad[diff[:3]]} vs {rad_ref[diff[:3]]}"
    assert pt.trace_rays_stats().segments == seg_ref


@pytest.mark.parametrize("use_bbox", [0, 1], ids=["brute", "bbox"])
@pytest.mark.parametrize("mesh", bd.MESHES)
def test_adversarial_rays_equal_the_oracle(kdpt, oracle, workdir, mesh, use_bbox):
    o, d, need = _adversarial(workdir, mesh)
    print(mesh, "rays that need exactness:", need)
    assert need >= EMIT[mesh][2], need
    _, sd, osc = _scene(kdpt, oracle, mesh, (64, 64))
    rad_ref, seg_ref = _oracle_rays(osc, mesh, o, d, 3, enable_kd=0, usebbox=use_bbox)
    assert seg_ref > NRAYS and float(rad_ref.sum()) > 0
    with kdpt.PathTracer(sd, kdpt.default_options(enable_kd=0, use_bbox=use_bbox), device=0) as pt:
        assert pt.cull_margin()["cull_exact"]
        _assert_rays_equal(pt, rad_ref, seg_ref, o, d, 3)


@pytest.mark.parametrize("mesh", bd.MESHES)
def test_adversarial_rays_sorted_and_uncompacted(kdpt, oracle, workdir, mesh):
    """Iteration 2 (the sort by material between bounces) and compaction = 0 (finished paths stay in their slots,
    the final gather)."""
    o, d, _ = _adversarial(workdir, mesh)
    _, sd, osc = _scene(kdpt, oracle, mesh, (64, 64))
    with kdpt.PathTracer(sd, kdpt.default_options(enable_kd=0), device=0) as pt:
        _assert_rays_equal(pt, *_oracle_rays(osc, mesh, o, d, 2, enable_kd=0), o, d, 2)
    with kdpt.PathTracer(sd, kdpt.default_options(enable_kd=0, compaction=0), device=0) as pt:
        _assert_rays_equal(pt, *_oracle_rays(osc, mesh, o, d, 3, enable_kd=0, compaction=0), o, d, 3)


@pytest.mark.parametrize("mesh", bd.MESHES)
def test_chunk_cull_equals_no_cull(kdpt, oracle, workdir, mesh):
    """The in-product A/B (as test_cluster_cull_equals_no_cull_at_scale does for k_trace): the same rays on a second
    context with "cluster_cull" = 0, where no chunk is ever skipped -- equal radiance bits and segments."""
    o, d, _ = _adversarial(workdir, mesh)
    _, sd, _ = _scene(kdpt, oracle, mesh, (64, 64))
    out = []
    for cull in (1, 0):
        with kdpt.PathTracer(sd, kdpt.default_options(enable_kd=0), device=0) as pt:
            pt.set_tuning("cluster_cull", cull)
            rad = pt.trace_rays(o, d, first_iter=3, count=1, normalize=False)
            out.append((rad, pt.trace_rays_stats().segments))
    assert out[0][1] == out[1][1]
    assert np.array_equal(out[0][0].view(np.uint32), out[1][0].view(np.uint32))


def _passes_bbox(sd, shape, o, d):
    """intersectBbox(...) > -1 of `shape`'s box as the reference reads it (obj_bboxes[shape .. shape + 5], -+ 0.01),
    in float32 like the kernel: which rays test the shape's triangles when use_bbox is on."""
    f32 = np.float32
    bb = np.ctypeslib.as_array(sd.view.obj_bboxes, (sd.view.num_bbox_floats,)).astype(np.float64)
    lo, hi = (bb[shape:shape + 3] - 0.01).astype(f32), (bb[shape + 3:shape + 6] + 0.01).astype(f32)
    with np.errstate(all="ignore"):
        inv = f32(1.0) / d
        a, b = (lo - o) * inv, (hi - o) * inv
        mn, mx = np.where(b < a, b, a), np.where(a < b, b, a)  # std::min(a, b), std::max(a, b)
        dmin, dmax = mn[:, 0], mx[:, 0]
        for k in (1, 2):
            dmin = np.where(dmin < mn[:, k], mn[:, k], dmin)  # std::max(dmin, mn)
            dmax = np.where(mx[:, k] < dmax, mx[:, k], dmax)  # std::min(dmax, mx)
        t = np.where(dmax < 0, dmax, np.where(dmin > dmax, dmax, dmin))
        return t > f32(-1.0)


@pytest.mark.parametrize("use_bbox", [0, 1], ids=["brute", "bbox"])
def test_shapes_ragged_rays_equal_the_oracle(kdpt, oracle, use_bbox):
    desc, sd, osc = _scene(kdpt, oracle, "shapes_ragged", (64, 32))
    assert list(np.ctypeslib.as_array(sd.view.obj_polyoffsets, (5,))) == [3, 189, 192, 195, 390]
    o, dr = soups.soup_rays("shapes_ragged", desc)
    d = oracle.glm_array(1, dr, np.zeros((len(dr), 3), np.float32))
    # within one wave (64 consecutive rays) some lanes pass shape 0's bbox and others miss it -- and the same for a
    # later shape, whose first triangle then differs between the lanes that passed shape 0 and those that did not
    for shape in (0, 1, 3):
        p = _passes_bbox(sd, shape, o, d).reshape(-1, 64).sum(axis=1)
        assert np.sum((p > 0) & (p < 64)) >= 8, (shape, p)
    for it in (1, 2):
        with kdpt.PathTracer(sd, kdpt.default_options(enable_kd=0, use_bbox=use_bbox), device=0) as pt:
            _assert_rays_equal(pt, *_oracle_rays(osc, "shapes_ragged", o, d, it, enable_kd=0, usebbox=use_bbox), o, d, it)


@pytest.mark.parametrize("use_bbox", [0, 1], ids=["brute", "bbox"])
@pytest.mark.parametrize("soup", ["shapes_ragged", "coincident", "flat", "syn20000"])
def test_soup_camera_renders_and_counters(kdpt, oracle, soup, use_bbox):
    """Camera renders of the soups at 40 x 24 on the brute-force route: image bits, segments and the intersect
    counters (triangles tested, glm "intersected" returns) of iteration 1 equal the oracle's."""
    _, sd, osc = _scene(kdpt, oracle, soup, (40, 24))
    img_ref, st = osc.render(1, 1, enable_kd=0, usebbox=use_bbox)
    with kdpt.PathTracer(sd, kdpt.default_options(enable_kd=0, use_bbox=use_bbox), device=0) as pt:
        pt.trace_iteration(1)
        assert pt.stats().segments == st.segments
        assert np.array_equal(pt.image().view(np.uint32), img_ref.view(np.uint32))
    with kdpt.PathTracer(sd, kdpt.default_options(enable_kd=0, use_bbox=use_bbox), device=0) as pt:
        _, tri, hit = pt.count_iteration(1)
    assert (tri, hit) == (st.tri_tests, st.tri_hits) and hit > 0


@pytest.mark.parametrize("soup", ["flat", "growth"])
def test_kd_contexts_trace_soup_rays(kdpt, oracle, soup):
    """Caller rays on the tree route: test_gpu_soups.py's 2 048 seeded rays (edge rays, in-plane and grazing rays,
    axis directions) through kdpt_trace_rays on a default context against render_rays, iterations 1 and 2."""
    desc, sd, osc = _scene(kdpt, oracle, soup, (64, 32))
    o, dr = soups.soup_rays(soup, desc)
    d = oracle.glm_array(1, dr, np.zeros((len(dr), 3), np.float32))
    with kdpt.PathTracer(sd, device=0) as pt:
        for it in (1, 2):
            rad = pt.trace_rays(o, dr, first_iter=it, count=1, normalize=True)
            rad_ref, seg_ref = _oracle_rays(osc, soup, o, d, it)
            assert np.array_equal(rad.view(np.uint32), rad_ref.view(np.uint32)), \
                f"iteration {it}: {int((rad != rad_ref).any(axis=1).sum())} rays differ"
            assert pt.trace_rays_stats().segments == seg_ref
