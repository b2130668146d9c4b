"""Host differential test of the analytic-geom stage: the product's prep_ray (kdpt_geoms.h: the nearest-first loop
over geom_entry_bound, the index-order loop with the geom_may_hit skip; kdpt_scene_prep.h prepare_geom's bounds),
compiled for the host, against the oracle's plain index-order loop on the adversarial scenes and generators of
tests/geoms.py: the winning geom and the bits of t, 400 000 rays per (scene, generator).  No reference file is read."""
import json
import os
import subprocess

import numpy as np
import pytest

import geoms
from conftest import ROOT as REPO

NRAYS = 400000


@pytest.fixture(scope="module")
def geom_diff(oracle):
    exe = os.path.join(REPO, "build", "geom_diff")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-I", os.path.join(REPO, "include"),
                    os.path.join(REPO, "tests", "native", "geom_diff.cpp"), "-L", os.path.join(REPO, "oracle"),
                    "-loracle", "-Wl,-rpath," + os.path.join(REPO, "oracle"), "-o", exe + f".{os.getpid()}"], check=True)
    os.replace(exe + f".{os.getpid()}", exe)  # parallel workers may be running the old one
    return exe


def traced(oracle, gen, d):
    """The directions as traced: glm's normalize (as the oracle pins it), except `nearunit`'s, cast as they are."""
    if gen == "nearunit":
        return d
    return oracle.glm_array(1, d, np.zeros((len(d), 3), np.float32))


def run_diff(exe, oracle, scene, tmp, n=NRAYS, extra=()):
    """geom_diff's JSON lines for every generator of a scene, by generator name."""
    desc = geoms.geom_scene(scene)
    args = [exe, geoms.write_desc(desc, os.path.join(tmp, f"{scene}.desc")), *extra]
    for gen, _ in geoms.GENERATORS:
        o, d = geoms.generator_rays(scene, desc, gen, n)
        d = traced(oracle, gen, d)
        assert not np.isnan(d).any()
        args.append(f"{gen}=" + geoms.write_rays(os.path.join(tmp, f"{scene}.{gen}.rays"), o, d))
    p = subprocess.run(args, capture_output=True, text=True, timeout=1200)
    assert p.returncode in (0, 1), (p.returncode, p.stderr)
    out = {}
    for line in p.stdout.splitlines():
        if line.startswith("{"):
            r = json.loads(line)
            out[r["gen"]] = r
    assert list(out) == [g for g, _ in geoms.GENERATORS], p.stdout[-2000:]
    return out, p.stdout


@pytest.mark.parametrize("scene", [s for s in geoms.SCENES if "+" not in s])
def test_prep_ray_equals_index_order_loop(geom_diff, oracle, tmp_path, scene):
    out, text = run_diff(geom_diff, oracle, scene, str(tmp_path), extra=("--ties",) if scene == "coplanar" else ())
    ng = len(geoms.geom_scene(scene).geom_type)
    won = np.zeros(ng, np.int64)
    for gen, r in out.items():
        print(scene, r)
        won += np.asarray(r["winners"])
    for gen, r in out.items():
        # ---- from the oracle's results alone: the rays do what they are there for ----
        assert r["rays"] == NRAYS
        assert r["hits"] >= 0.2 * NRAYS, r
        if scene == "coplanar":
            assert r["ties"] >= 1000, r
    if scene == "nested":  # over the scene's generators (`distant` starts outside by construction)
        assert sum(r["inside"] for r in out.values()) >= 0.2 * sum(r["hits"] for r in out.values())
    if scene == "coplanar":
        # geoms 4 and 6 are exact copies of 3 and 5: every hit of theirs is a tie, which the reference's
        # `t_min > t` gives to the lower index, so they never win -- and every other geom does
        assert won[4] == 0 and won[6] == 0 and np.all(np.delete(won, [4, 6]) > 0), won
    else:
        assert np.all(won > 0), won
    # the loop under test is the nearest-first one wherever the scene's geoms have a proven range around them
    # (geom_diff's "ordered": prep_ray's own condition); the translated scenes have none (the reference's loop as
    # it stands), and nine / mats64 have more than 8 geoms: the index-order loop with the skip test
    if scene in ("tilted", "coplanar", "nested", "eight", "mats33", "glass", "far"):
        assert out["inside"]["ordered"] >= 0.25 * NRAYS and out["random"]["ordered"] >= 0.05 * NRAYS, out["inside"]
    else:
        assert sum(r["ordered"] for r in out.values()) == 0
    for gen, r in out.items():
        assert r["mismatches"] == 0, (r, text[-3000:])


@pytest.mark.parametrize("scene", ["far", "translated"])
def test_fixture_rays_agree_now(geom_diff, oracle, tmp_path, scene):
    """tests/golden/geom_far_rays.npz: 512 rays per scene on which the loop differed from the reference's before
    the bound was corrected (geoms.load_fixture_rays says how they were made)."""
    o, d = geoms.load_fixture_rays(scene)
    assert o.shape == d.shape == (512, 3)
    desc = geoms.geom_scene(scene)
    p = subprocess.run([geom_diff, geoms.write_desc(desc, str(tmp_path / "s.desc")),
                        "fixture=" + geoms.write_rays(str(tmp_path / "f.rays"), o, d)], capture_output=True, text=True,
                       timeout=300)
    assert p.returncode in (0, 1), (p.returncode, p.stderr)
    r = json.loads(p.stdout.strip().splitlines()[-1])
    assert r["rays"] == 512 and r["hits"] >= 256, r
    assert r["mismatches"] == 0, p.stdout[-3000:]
