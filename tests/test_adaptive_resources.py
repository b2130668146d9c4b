"""The adaptive-sampling kernels in the gfx950 build's resource report (build/kdpt_runtime.build.log, see
test_build_resources.py): the list kernels, the add and the save pass are bandwidth-bound one-pass kernels, and the
two camera-stage kernels must fit beside a resident intersect workgroup as k_gen_geoms_b does -- so no scratch and at
least 4 waves per SIMD for every one of them."""
import pytest

from test_build_resources import _report

NEW = ("k_adapt_flags", "k_adapt_scan", "k_adapt_list", "k_adapt_rays_b", "k_adapt_geoms_b", "k_accumulate_adapt",
       "k_save_counted", "k_noise_map_counted", "k_noise_partials_counted")


@pytest.mark.parametrize("frag", NEW)
def test_adaptive_kernels_scratch_and_occupancy_within_budget(kdpt, frag):
    rep = _report()
    ks = [k for k in rep if frag in k]
    assert ks, frag
    if frag == "k_adapt_flags":  # the context's instantiation and the self test's
        assert len(ks) == 2, ks
    for k in ks:
        assert rep[k].get("ScratchSize", 0) == 0, (k, rep[k])
        assert rep[k].get("Occupancy", 0) >= 4, (k, rep[k])


def test_new_kernel_names_stay_out_of_the_existing_budgets():
    """test_build_resources.py matches kernels by name fragment: the new names must not fall under one.  (The two
    counted noise kernels do fall under test_moments_resources.py's fragments, whose budget is this one.)"""
    from test_build_resources import HOT
    for name in NEW:
        assert not any(frag in name for frag in HOT), name
