"""GPU (-m gpu): the checks of tests/test_readout_truth_host.py on the device -- k_scan_moments_partial, k_analysis_place /
k_analysis_moments / k_analysis_fold and the fused read-out's statistics against the long-double truth of
tests/readout_truth_common.py (bars, scenes and which check catches which change: there and in the host file).  Every
scene is traced once per module; the largest holds 300 001 rays."""
import pytest

import readout_truth_common as rt
from conftest import report

pytestmark = pytest.mark.gpu
SCENES = ("tight_2nm", "tight_180nm", "relay4")


@pytest.fixture(scope="module")
def hip():
    import torch
    import __graft_entry__
    from attosecondraytracing_amd import _lib
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    __graft_entry__.ensure_built()
    _lib._BACKEND = None
    be = _lib.get_backend()
    assert be.name == "hip"
    return be


@pytest.fixture(scope="module")
def scenes(hip):
    assert rt.HAVE_LD, "numpy.longdouble has no extended precision on this platform"
    yield rt.build_scenes()
    for line in rt.worst_lines("MI355X"):
        report(line)


@pytest.mark.parametrize("name", SCENES)
def test_gpu_per_ray_readout_against_the_truth(scenes, name):
    rt.check_per_ray(name, scenes[name])


@pytest.mark.parametrize("name", SCENES)
def test_gpu_spot_size_and_duration_at_the_detector(scenes, name):
    rt.check_at_the_detector(name, scenes[name])


@pytest.mark.parametrize("name", SCENES)
def test_gpu_spot_size_and_duration_on_shifted_planes(scenes, name):
    rt.check_shifted(name, scenes[name])


@pytest.mark.parametrize("n", rt.SIZES)
def test_gpu_masked_bundle_sizes(scenes, n):
    rt.check_size(n)


def test_gpu_batches_give_the_bytes_of_single_calls(scenes):
    rt.check_batches(scenes)
