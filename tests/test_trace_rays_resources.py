"""The ray queries' bounce-0 kernels in the gfx950 build's resource report (build/kdpt_runtime.build.log, see
test_build_resources.py): no scratch and at least 4 waves per SIMD, the figures k_gen_rays / k_geoms are held to,
so that one of their waves still fits beside a resident intersect workgroup."""
import pytest

from test_build_resources import _report

NEW = ("k_user_rays_b", "k_user_geoms_b")


@pytest.mark.parametrize("frag", NEW)
def test_ray_query_kernels_scratch_and_occupancy_within_budget(kdpt, frag):
    rep = _report()
    ks = [k for k in rep if frag in k]
    assert ks, frag
    for k in ks:
        assert rep[k].get("ScratchSize", 0) == 0, (k, rep[k])
        assert rep[k].get("Occupancy", 0) >= 4, (k, rep[k])


def test_new_kernel_names_stay_out_of_the_existing_budgets():
    """test_build_resources.py matches kernels by name fragment: the new names must not fall under one."""
    from test_build_resources import HOT
    for name in NEW:
        assert not any(frag in name for frag in HOT), name
