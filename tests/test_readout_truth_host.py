"""CPU twin: spot size and duration of every path that forms them from raw second moments -- Detector._scan_moments,
analysis.analyse / GetResultSummary, the fused read-out's statistics -- and the per-ray read-out, against the long-double
truth of tests/readout_truth_common.py (bars and scenes there), on detectors whose centre lies up to 100 mm from the spot,
on shifted planes, with weights, at sizes from one ray to more slots than the moments grid has lanes, alone and in
batches.  tests/test_gpu_readout_truth.py runs the same checks on the device.

Which check catches which change (each assertion stops at the first pose that fails; the later ones fail too): without
the in-plane recentring of Detector._scan_moments, "(a) scan" fails the spot of tight_2nm from off1 on (1e-5 at 1 mm, growing
with the square of the distance) and of tight_180nm at off100 (2.2e-6); without the 1 / <cos> in analysis_place's path centre, "(b) manual", "(b) auto"
and "(c) summary" fail tight_2nm's duration on every pose, shifted or not (3.3e-5); without the (cx, cy) centring of
art_analyse_bundles' X and Y sums, "(b) manual" and "(c) summary" fail the same spots as the scan path did, at s = 0 and on
the shifted planes.  Figures measured on the CPU twin; DESIGN.md 5 has the worst ratios to the bars with all three in."""
import pytest

import readout_truth_common as rt
from conftest import report

pytestmark = pytest.mark.skipif(not rt.HAVE_LD, reason="numpy.longdouble has no extended precision on this platform")
SCENES = ("tight_2nm", "tight_180nm", "relay4")


@pytest.fixture(scope="module")
def scenes():
    from twin_backend import TwinBackend
    from attosecondraytracing_amd import _lib
    old = _lib._BACKEND
    _lib._BACKEND = TwinBackend()
    yield rt.build_scenes()
    _lib._BACKEND = old
    for line in rt.worst_lines("twin"):
        report(line)


@pytest.mark.parametrize("name", SCENES)
def test_per_ray_readout_against_the_truth(scenes, name):
    rt.check_per_ray(name, scenes[name])


@pytest.mark.parametrize("name", SCENES)
def test_spot_size_and_duration_at_the_detector(scenes, name):
    rt.check_at_the_detector(name, scenes[name])


@pytest.mark.parametrize("name", SCENES)
def test_spot_size_and_duration_on_shifted_planes(scenes, name):
    rt.check_shifted(name, scenes[name])


@pytest.mark.parametrize("n", rt.SIZES)
def test_masked_bundle_sizes(scenes, n):
    rt.check_size(n)


def test_batches_give_the_bytes_of_single_calls(scenes):
    rt.check_batches(scenes)
