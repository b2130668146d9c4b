"""The render group's two kernels in the gfx950 build's resource report (build/kdpt_runtime.build.log, see
test_build_resources.py): k_frame_moments (rank 0's finish of a frame that carries second moments) and k_adapt_slots
(rank 0's add of a group's adaptive round) are bandwidth-bound one-pass kernels -- no scratch, no LDS, and the
figures DESIGN.md section 16 quotes."""
import os
import re

import pytest

from conftest import ROOT
from kdtreepathtraceroptimization_amd import _build
from test_build_resources import _report

# kernel -> (VGPRs, LDS bytes per workgroup, waves per SIMD), as DESIGN.md section 16 states them
NEW = {"k_frame_moments": (8, 0, 8), "k_adapt_slots": (22, 0, 8)}


def _lds():
    out, cur = {}, None
    for line in open(_build.RESOURCE_LOG):
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = m.group(1)
            continue
        m = re.search(r"remark:\s+LDS Size \[bytes/block\]: (\d+)", line)
        if m and cur:
            out[cur] = int(m.group(1))
    return out


@pytest.mark.parametrize("frag", sorted(NEW))
def test_group_kernels_have_no_scratch_and_the_documented_figures(kdpt, frag):
    rep = _report()
    ks = [k for k in rep if frag in k]
    assert len(ks) == 1, (frag, ks)
    vgprs, lds, occupancy = NEW[frag]
    r = rep[ks[0]]
    assert r.get("ScratchSize", 0) == 0, r
    assert (r.get("VGPRs"), _lds().get(ks[0]), r.get("Occupancy")) == (vgprs, lds, occupancy), r


@pytest.mark.parametrize("frag", sorted(NEW))
def test_design_section_16_quotes_the_figures(frag):
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    sec = design[design.index("## 16."):]
    vgprs, lds, occupancy = NEW[frag]
    row = [ln.strip() for ln in sec.splitlines() if ln.strip().startswith("|") and frag in ln]
    assert len(row) == 1, row
    cells = [c.strip().strip("`") for c in row[0].strip("|").split("|")]
    assert cells[:5] == [frag, str(vgprs), "0", str(lds), str(occupancy)], cells


def test_new_kernel_names_stay_out_of_the_existing_budgets():
    """The other resource tests match kernels by name fragment: the new names must not fall under one."""
    from test_adaptive_resources import NEW as ADAPTIVE
    from test_build_resources import HOT
    from test_moments_resources import NEW as MOMENTS
    from test_trace_rays_resources import NEW as RAYS
    for name in NEW:
        assert not any(frag in name for frag in (*HOT, *ADAPTIVE, *MOMENTS, *RAYS)), name
