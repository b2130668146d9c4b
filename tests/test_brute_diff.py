"""Host differential of the brute-force intersect route (enable_kd = 0, kernels_brute.h k_brute).

k_brute is the reference's loop over every OBJ triangle with two shortcuts: a lane skips a 64-triangle file-order
chunk whose box its line misses (kdpt_cull.h brute_chunk_may_pass, the box widened by the chunk's own rigorous
coefficient), and it rejects a triangle without glm's division when glm's answer is certain (tri_certain_miss).
tests/native/brute_diff.cpp compiles both for the host, calls kdpt_scene_prep.h prepare_brute on the scene's raw
OBJ arrays -- so it runs on the kernel's triangles, chunk boxes, coefficients and shapes, in file order -- and checks,
on adversarial lines,
  (a) per line: the chunk of the triangle the line was aimed at is not culled while one of its triangles returns
      tri_test_v == 2 with tri_hit_t_n > 0 ("dropped"), and tri_certain_miss never holds for a triangle with
      tri_test_v == 2 ("cm_viol");
  (b) on every line with a chunk-local event and every 256th other: one emulated lane of k_brute (shape loop,
      `iterator`, bbox, chunk cull, tri_certain_miss, exact test, first-minimum rule) against the reference's plain
      loop over the raw arrays: winner, t bits and hit count equal ("route_viol");
  and tri_certain_miss alone on triangles scaled by 2^+-40, 2^+-60 and to a determinant near FLT_EPSILON, and on
      (a, u, v, w) within 4 ulps of each of its thresholds over the float range ("cm_alone_viol").
Lines: cull_diff's generators with the chunk's box as the box (the in-plane, beyond-a-vertex, determinant 1 .. 100
eps family included, and one aimed at the shape's bbox), rays through a vertex or edge midpoint shared with a
triangle of another chunk (ties in t across chunks), origins on and one float step off chunk-box faces, rays at
barycentrics 0 and 1 with the origin moved by -4 .. 4 ulps.
"""
import pytest

import brute_diff_lib as bd

SEED = 7
LINES = {"sphere_low_1": 1_000_000, "stanford_bunny": 2_000_000, "dragon_5": 10_000_000, "coincident": 1_000_000,
         "flat": 1_000_000, "syn20000": 1_000_000, "shapes_ragged": 1_000_000}


@pytest.fixture(scope="module")
def scenes(tmp_path_factory):
    d = tmp_path_factory.mktemp("brute_scenes")
    out = {}

    def get(name):
        if name not in out:
            out[name] = bd.scene_file(name, d)
        return out[name]
    return get


def _summary(r):
    return {k: v for k, v in r.items() if k != "gens"}


@pytest.mark.parametrize("use_bbox", [0, 1], ids=["brute", "bbox"])
@pytest.mark.parametrize("name", list(LINES))
def test_brute_route_equals_the_plain_loop(scenes, name, use_bbox):
    """Zero violations of (a) and (b) at the shipped coefficients, use_bbox 0 and 1: the three fixture meshes
    (sphere_low_1 10^6 lines, stanford_bunny 2 * 10^6, dragon_5 10^7) and the soups coincident (3 shapes: 64-way
    ties in t), flat (chunk boxes of zero thickness), syn20000 (zero-area and duplicated triangles) and
    shapes_ragged (5 shapes of 1, 63, 64, 65, 130 triangles: chunks straddle shapes, `iterator` lags behind missed
    bboxes), 10^6 lines each."""
    r = bd.run(scenes(name), LINES[name], SEED, *(["--bbox"] if use_bbox else []))
    print(name, use_bbox, _summary(r))
    assert r["lines"] == LINES[name] and r["use_bbox"] == use_bbox and r["fixed"] == 0, _summary(r)
    assert r["dropped"] == 0 and r["cm_viol"] == 0 and r["route_viol"] == 0 and r["cm_alone_viol"] == 0, r
    # the lines do reach what they are aimed at: hits in the line's own chunk from every generator, whole-route
    # comparisons on all of those, and tri_certain_miss cases glm accepts
    assert all(g["hit_own"] > 0 for g in r["gens"].values()), r
    assert r["route_runs"] >= r["hit_own"] > LINES[name] // 100, _summary(r)
    assert r["cm_accepted"] > r["cm_cases"] // 10 > 0, _summary(r)


# (a)'s "dropped" per mesh with every chunk at the coefficient 1e-3 the chunk cull used to run at (--margin 1e-3),
# as measured: the mix of generators at SEED for the first two, 10^7 lines of the rounding-targeted generator alone
# for dragon_5 (the mix at 10^6 lines, about 10^5 of them from that generator, finds none in dragon_5's small chunks)
DROPPED_AT_1E3 = {"sphere_low_1": 408, "stanford_bunny": 8, "dragon_5": 10}


@pytest.mark.parametrize("mesh", bd.MESHES)
def test_generator_bites_at_the_fast_margin(scenes, mesh):
    """The condition that the lines bite: with --margin 1e-3 (the box coefficient the chunk cull ran at before each
    chunk got its own rigorous one) every fixture mesh shows dropped hits in (a) -- chunks culled although a triangle
    of them returns glm "intersected".  Measured: sphere_low_1 408 in 10^6 lines (402 of them from the
    rounding-targeted generator's 111 112 lines), stanford_bunny 8 in 10^6, dragon_5 10 in 10^7 lines of the
    rounding-targeted generator (same seed).  tri_certain_miss stays clean: it does not depend on the margin."""
    args = ["--margin", "1e-3", "--no-route"]
    if mesh == "dragon_5":
        r = bd.run(scenes(mesh), 10_000_000, SEED, *args, "--only", "round")
    else:
        r = bd.run(scenes(mesh), 1_000_000, SEED, *args)
    print(mesh, _summary(r))
    assert abs(r["fixed"] - 1e-3) < 1e-9 and r["route_runs"] == 0, _summary(r)
    assert r["dropped"] > 0, _summary(r)
    assert r["dropped"] == DROPPED_AT_1E3[mesh], _summary(r)  # (deterministic: seeded lines, IEEE float arithmetic)
    assert r["cm_viol"] == 0 and r["cm_alone_viol"] == 0, _summary(r)


def test_whole_route_sees_the_dropped_hits(scenes):
    """(b) at --margin 1e-3 on sphere_low_1: every dropped hit of (a) changes the emulated lane's result (one chunk:
    the dropped triangle is the only candidate), so the whole-route comparison reports as many."""
    r = bd.run(scenes("sphere_low_1"), 1_000_000, SEED, "--margin", "1e-3")
    assert r["dropped"] == DROPPED_AT_1E3["sphere_low_1"] and r["route_viol"] == r["dropped"], _summary(r)


def test_chunk_coefficients(scenes):
    """What the shipped coefficients are: sphere_low_1's and stanford_bunny's triangles are too large for a
    coefficient below the cap (no chunk of theirs is ever culled); dragon_5's 196 chunks have 0.30 .. 1.0, 178 of
    them below the cap."""
    for mesh, chunks, culling in [("sphere_low_1", 1, 0), ("stanford_bunny", 5, 0), ("dragon_5", 196, 178)]:
        r = bd.run(scenes(mesh), 9, SEED, "--no-route")
        assert (r["chunks"], r["chunks_culling"]) == (chunks, culling), _summary(r)
        if culling:
            assert 0.3 < r["k_min"] <= r["k_max"] < 1.0, _summary(r)
