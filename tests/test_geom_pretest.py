"""Host differential test of the analytic-geom stage's box pre-test (kdpt_geoms.h: box_provably_missed and the
pre-pass of prep_ray's nearest-first branch), compiled for the host (tests/native/geom_pretest_diff.cpp), against the
oracle: prep_ray's winner and the bits of its t against the oracle's index-order loop, and the pre-test's verdict
per (ray, box) against the oracle's exact test of that box alone -- on every scene and generator of tests/geoms.py
and on the rays of tests/geoms_leaving.py (origins where a bounce leaves them, float steps across the face,
degenerate directions), 400 000 rays per (scene, generator).  No reference file is read.

Efficacy (cornell, leaving_cosine, 400 000 rays, this harness): the loop without the pre-pass runs 1.440 exact tests
per ray, the loop behind it 0.773, a ratio of 0.537 (the bound is 0.6), for one pre-test per ray.  A third of these
rays start inside the box they left (the refraction offset), where the box is hit and nothing can be ruled out; a
model with outside origins only gave 0.45."""
import json
import os
import subprocess

import numpy as np
import pytest

import geoms
import geoms_leaving
from conftest import ROOT as REPO

NRAYS = 400000
_rays = {}


@pytest.fixture(scope="module")
def pretest_diff(oracle):
    """(the harness, the same harness with prep_ray's pre-pass compiled out)."""
    exes = []
    for name, flags in (("geom_pretest_diff", []), ("geom_pretest_diff_base", ["-DKDPT_NO_GEOM_PRETEST"])):
        exe = os.path.join(REPO, "build", name)
        os.makedirs(os.path.dirname(exe), exist_ok=True)
        subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", *flags, "-I",
                        os.path.join(REPO, "include"), os.path.join(REPO, "tests", "native", "geom_pretest_diff.cpp"),
                        "-L", os.path.join(REPO, "oracle"), "-loracle", "-Wl,-rpath," + os.path.join(REPO, "oracle"),
                        "-o", exe + f".{os.getpid()}"], check=True)
        os.replace(exe + f".{os.getpid()}", exe)  # parallel workers may be running the old one
        exes.append(exe)
    return tuple(exes)


def harness_tracer(exe, desc_path, tmp):
    """geoms_leaving's tracer: the oracle's records of the first rays, through the harness's --first-hits."""
    def trace(o, d):
        rays, out = os.path.join(tmp, "first.rays"), os.path.join(tmp, "first.hits")
        subprocess.run([exe, desc_path, "--first-hits", geoms.write_rays(rays, o, d), out], check=True, timeout=600)
        raw = np.fromfile(out, np.uint8)
        assert len(raw) == 4 + 32 * len(o) and int(raw[:4].view(np.int32)[0]) == len(o)
        rec = raw[4:].reshape(len(o), 32)
        gi = np.ascontiguousarray(rec[:, :8]).view(np.int32)
        fl = np.ascontiguousarray(rec[:, 8:]).view(np.float32)
        return gi[:, 0].copy(), gi[:, 1].copy(), fl[:, 0:3].copy(), fl[:, 3:6].copy()
    return trace


def run(exe, desc_path, files):
    p = subprocess.run([exe, desc_path, *[f"{g}={f}" for g, f in files]], capture_output=True, text=True, timeout=2400)
    assert p.returncode in (0, 1), (p.returncode, p.stderr)
    out = {}
    for line in p.stdout.splitlines():
        if line.startswith("{"):
            r = json.loads(line)
            out[r["gen"]] = r
    assert list(out) == [g for g, _ in files], p.stdout[-2000:]
    return out, p.stdout


def leaving_files(exe, oracle, scene, tmp):
    """The scene's ray files of geoms_leaving.GENERATORS (made once per scene) and each generator's info."""
    if scene not in _rays:
        desc = geoms_leaving.scene(scene)
        desc_path = geoms.write_desc(desc, os.path.join(tmp, f"{scene}.desc"))
        tracer = harness_tracer(exe, desc_path, tmp)
        files, infos = [], {}
        for gen in geoms_leaving.GENERATORS:
            o, d, infos[gen] = geoms_leaving.leaving_rays(scene, desc, gen, NRAYS, tracer)
            unit = ~infos[gen].get("as_is", np.zeros(len(d), bool))  # as traced: glm's normalize, as the oracle pins it
            d[unit] = oracle.glm_array(1, np.ascontiguousarray(d[unit]), np.zeros((int(unit.sum()), 3), np.float32))
            assert not np.isnan(d).any()
            files.append((gen, geoms.write_rays(os.path.join(tmp, f"{scene}.{gen}.rays"), o, d)))
        _rays[scene] = (desc_path, files, infos)
    return _rays[scene]


def check_common(out, text):
    for gen, r in out.items():
        print(r)
        assert r["rays"] == NRAYS
        assert r["hits"] >= 0.2 * NRAYS, r  # (the oracle's results alone)
    for gen, r in out.items():
        assert r["mismatches"] == 0, (r, text[-3000:])
        assert r["false_miss"] == 0, (r, text[-3000:])


@pytest.mark.parametrize("scene", [s for s in geoms.SCENES if "+" not in s])
def test_pretest_on_the_geom_scenes(pretest_diff, oracle, tmp_path, scene):
    """tests/geoms.py's scenes and generators: prep_ray with the pre-pass equals the oracle's loop, and no box the
    pre-test rules out is hit by the oracle's exact test."""
    from test_geom_diff import traced
    desc = geoms.geom_scene(scene)
    desc_path = geoms.write_desc(desc, str(tmp_path / f"{scene}.desc"))
    files = []
    for gen, _ in geoms.GENERATORS:
        o, d = geoms.generator_rays(scene, desc, gen, NRAYS)
        d = traced(oracle, gen, d)
        assert not np.isnan(d).any()
        files.append((gen, geoms.write_rays(str(tmp_path / f"{scene}.{gen}.rays"), o, d)))
    out, text = run(pretest_diff[0], desc_path, files)
    check_common(out, text)
    # the pre-test is exercised: it rules boxes out on these rays too
    assert sum(r["ruled_out"] for r in out.values()) > 0


@pytest.mark.parametrize("scene", geoms_leaving.SCENES)
def test_pretest_on_leaving_rays(pretest_diff, oracle, tmp_path_factory, scene):
    tmp = str(tmp_path_factory.mktemp(f"leaving_{scene}"))
    desc_path, files, infos = leaving_files(pretest_diff[0], oracle, scene, tmp)
    out, text = run(pretest_diff[0], desc_path, files)
    # ---- from the oracle and the generators alone: the rays are the ones the pre-test exists for ----
    for gen, r in out.items():
        if gen.startswith("leaving"):
            assert r["left_behind"] >= 0.2 * NRAYS, r
    outside = infos["ulps"]["outside"]
    assert 0.1 <= outside.mean() <= 0.9, outside.mean()
    check_common(out, text)
    # the pre-pass ran on them (every scene here keeps its geoms on the nearest-first loop)
    assert out["leaving_cosine"]["ordered"] >= 0.9 * NRAYS and out["leaving_cosine"]["pre_miss"] >= 0.2 * NRAYS, out


def test_pretest_saves_exact_tests_on_cornell(pretest_diff, oracle, tmp_path_factory):
    """Exact tests per ray on the cornell fixture's leaving_cosine rays: at most 0.6 of what prep_ray without the
    pre-pass (the parent's loop, the same harness and rays) runs."""
    tmp = str(tmp_path_factory.mktemp("leaving_cornell_ratio"))
    desc_path, files, _ = leaving_files(pretest_diff[0], oracle, "cornell", tmp)
    files = [f for f in files if f[0] == "leaving_cosine"]
    new, _ = run(pretest_diff[0], desc_path, files)
    base, _ = run(pretest_diff[1], desc_path, files)
    new, base = new["leaving_cosine"], base["leaving_cosine"]
    print("exact tests per ray: parent's loop", base["exact"] / NRAYS, "with the pre-pass", new["exact"] / NRAYS,
          "ratio", new["exact"] / base["exact"], "pre-tests per ray", (new["pre_miss"] + new["pre_abstain"]) / NRAYS)
    assert base["mismatches"] == 0 and new["mismatches"] == 0
    assert base["pre_miss"] == 0 and base["pre_abstain"] == 0
    assert new["exact"] <= 0.6 * base["exact"], (new, base)
