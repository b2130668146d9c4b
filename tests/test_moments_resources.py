"""The second-moment kernels in the gfx950 build's resource report (build/kdpt_runtime.build.log, see
test_build_resources.py): bandwidth-bound one-pass kernels, so no scratch and at least 4 waves per SIMD."""
import pytest

from test_build_resources import _report

NEW = ("k_accumulate_moments", "k_noise_map", "k_noise_partials", "k_noise_final")


@pytest.mark.parametrize("frag", NEW)
def test_moment_kernels_scratch_and_occupancy_within_budget(kdpt, frag):
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
