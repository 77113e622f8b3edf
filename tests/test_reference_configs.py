"""CPU: the scenes of the reference's shipped CONFIG_*.py scripts, run on this package through `ARTmain` (CPU twin of
the kernels as backend).  Each scene is rebuilt here with the package's own classes, the way the script builds it
(same optics, distances, angles, loop lists and post-placement moves); the scripts' SourceProperties / DetectorOptions /
AnalysisOptions dictionaries are the fixture tests/golden/reference_configs.json
(tests/golden/generate_reference_configs.py).  Numbers are compared with the golden
fixtures / survey anchors of the same scenes."""
import json
import os
import types

import numpy as np
import pytest

from conftest import GOLDEN_DIR, load_golden

with open(os.path.join(GOLDEN_DIR, "reference_configs.json")) as _f:
    OPTIONS = json.load(_f)


@pytest.fixture()
def twin(monkeypatch, tmp_path):
    from twin_backend import TwinBackend
    from attosecondraytracing_amd import _lib
    monkeypatch.setattr(_lib, "_BACKEND", TwinBackend())
    monkeypatch.chdir(tmp_path)            # save_results writes archives into the cwd
    # the reference's complete_defaults mutates module-level dicts: restore them after the test
    from attosecondraytracing_amd import DefaultOptions as D
    saved = {k: dict(getattr(D, k)) for k in ("DefaultAnalysisOptions", "DefaultSourceProperties", "DefaultDetectorOptions")}
    yield
    for k, v in saved.items():
        getattr(D, k).clear()
        getattr(D, k).update(v)


def _singleparabola(SP, ns):
    import ART.ModuleMirror as mmirror, ART.ModuleSupport as msupp, ART.ModuleProcessing as mp
    Parabola = mmirror.MirrorParabolic(100, 90, msupp.SupportRoundHole(30, 5, 10, 5))
    chain = mp.OEPlacement(SP, [Parabola], [200], [0.00], Description="single parabola")
    chain.optical_elements[0].rotate_roll_by(np.rad2deg(50e-6))        # misaligned out of the incidence plane
    ns.OpticalChainList = chain


def _two_toroids(SP, ns, mask, support, focal, distances, planes, label):
    """mask -> toroid -> toroid with a loop list in one entry; the scripts pass a 7th positional `render` argument."""
    import ART.ModuleMirror as mmirror, ART.ModuleMask as mmask, ART.ModuleProcessing as mp
    R, r = mmirror.ReturnOptimalToroidalRadii(focal, 80)
    Tor = mmirror.MirrorToroidal(R, r, support)
    ns.OpticalChainList = mp.OEPlacement(SP, [mmask.Mask(mask), Tor, Tor], distances, [0, 80, -80], planes, label, False)


def _fxf(SP, ns):
    import ART.ModuleSupport as msupp
    _two_toroids(SP, ns, msupp.SupportRoundHole(Radius=20, RadiusHole=14 / 2, CenterHoleX=0, CenterHoleY=0),
                 msupp.SupportRectangle(150, 32), 500, [400, 500 - 400, np.linspace(500 - 200, 500 + 200, 11)], [0, 0, 0],
                 "two toroids f-x-f")


def _twisted(SP, ns):
    import ART.ModuleSupport as msupp
    _two_toroids(SP, ns, msupp.SupportRoundHole(30, 41e-3 / 2 * 500, 0, 0), msupp.SupportRectangle(200, 30), 600,
                 [500, 600 - 500, 600], [0, 0, np.linspace(-90, 90, 10)], "two toroids, twisted")


def _toroidal_2f2f(SP, ns):
    import ART.ModuleMirror as mmirror, ART.ModuleSupport as msupp, ART.ModuleProcessing as mp
    R, r = mmirror.ReturnOptimalToroidalRadii(500, 80)
    Mirror = mmirror.MirrorToroidal(R, r, msupp.SupportRectangle(300, 50))
    aligned = mp.OEPlacement(SP, [Mirror], [2 * 500], [80], Description="toroid 2f-2f")
    ns.OpticalChainList = aligned.get_OE_loop_list(0, "roll", np.linspace(-0.5, 0.5, 11))


def _toroidal_2f2f_byhand(SP, ns):
    """The mirror at the origin, the source placed by hand at 2 f along the incidence direction."""
    import ART.ModuleMirror as mmirror, ART.ModuleSupport as msupp, ART.ModuleSource as msource
    import ART.ModuleOpticalElement as moe, ART.ModuleOpticalChain as moc
    focal, incidence, misalign = 300, 80, 0.00
    R, r = mmirror.ReturnOptimalToroidalRadii(focal, incidence)
    Mirror = mmirror.MirrorToroidal(R, r, msupp.SupportRectangle(120, 30))
    Element1 = moe.OpticalElement(Mirror, np.array([0, 0, 0]), np.array([0, 0, 1]), np.array([1, 0, 0]))
    S = np.array([2 * focal * np.sqrt(1 - np.cos(np.deg2rad(incidence + misalign)) ** 2), 0,
                  2 * focal * np.cos(np.deg2rad(incidence + misalign))])
    rays = msource.PointSource(S, -S, SP["Divergence"], SP["NumberRays"])
    rays = msource.ApplyGaussianIntensityToRayList(rays, 1 / np.e ** 2)
    ns.OpticalChainList = moc.OpticalChain(rays, [Element1], "toroid 2f-2f, placed by hand",
                                           loop_variable_name="incidence misalignment (deg)", loop_variable_value=misalign)


def _collimating_telescope(SP, ns):
    import ART.ModuleMirror as mmirror, ART.ModuleSupport as msupp, ART.ModuleProcessing as mp
    MirrorCX = mmirror.MirrorSpherical(-1500, msupp.SupportRound(25))
    MirrorCC = mmirror.MirrorSpherical(2500, msupp.SupportRound(25))
    Parabola = mmirror.MirrorParabolic(100, 90, msupp.SupportRound(25))
    ns.OpticalChainList = mp.OEPlacement(SP, [MirrorCX, MirrorCC, Parabola], [5000, 598, 1000], [5, 3.4, 0.04],
                                         Description="collimating telescope")


def _deformed(SP, ns):
    import ART.ModuleMirror as mmirror, ART.ModuleSupport as msupp, ART.ModuleProcessing as mp, ART.ModuleDefects as mdef
    Support = msupp.SupportRectangle(40, 40)
    Mirror = mmirror.MirrorParabolic(25.4, 0, Support)
    Defect = mdef.Fourrier(Support, RMS=1e-1, smallest=0.01)
    ns.DeformedMirror = mmirror.DeformedMirror(Mirror, [Defect])
    ns.OpticalChainList = mp.OEPlacement(SP, [ns.DeformedMirror], [15], [0], Description="deformed parabola")


SCENES = {"CONFIG_singleparabola.py": _singleparabola, "CONFIG_2toroidals_f-x-f.py": _fxf,
          "CONFIG_2toroidals_twisted.py": _twisted, "CONFIG_toroidal2f-2f.py": _toroidal_2f2f,
          "CONFIG_toroidal2f-2f_byhand.py": _toroidal_2f2f_byhand,
          "CONFIG_CollimatingTelescope.py": _collimating_telescope, "CONFIG_deformed.py": _deformed}


def _load(name):
    """A stand-in for the imported CONFIG module: its chain(s) and its three option dictionaries."""
    opts = json.loads(json.dumps(OPTIONS[name]))       # fresh dictionaries: ARTmain completes them in place
    ns = types.SimpleNamespace(**opts)
    SCENES[name](ns.SourceProperties, ns)
    return ns


def _run(mod):
    import ARTmain
    chains, src, det, ana = ARTmain.load_config(mod)
    ana = dict(ana)
    ana["save_results"] = False
    return ARTmain.main(chains, src, det, ana)


def test_config_singleparabola(twin):
    kept = _run(_load("CONFIG_singleparabola.py"))
    scene, a = load_golden("c1_singleparabola")
    chain = kept["OpticalChain"][0]
    out = chain.get_output_rays()[-1]
    assert len(chain.source_rays) == 999 and len(out) == scene["n_out"][-1] == 957
    assert np.array_equal(out.numbers(), a["out0_number"])
    assert np.abs(out.points() - a["out0_point"]).max() <= 1e-10 * 200
    assert abs(kept["SpotSizeSD"][0] - scene["SpotSizeSD"]) <= 1e-9
    assert abs(kept["DurationSD"][0] - scene["DurationSD"]) <= 1e-7      # 14.355 fs (survey anchor)
    assert abs(kept["DurationSD"][0] - 14.355) < 1e-3
    assert abs(kept["ETransmission"][0] - scene["ETransmission"]) <= 1e-9


def test_config_2toroidals_fxf(twin):
    """This script passes a 7th positional `render` argument to OEPlacement (TypeError in the reference itself)."""
    kept = _run(_load("CONFIG_2toroidals_f-x-f.py"))
    assert len(kept["OpticalChain"]) == 11
    for i, name in ((0, "c2_fxf_chain00"), (5, "c2_fxf_chain05"), (10, "c2_fxf_chain10")):
        scene, a = load_golden(name)
        out = kept["OpticalChain"][i].get_output_rays()
        assert [len(o) for o in out] == scene["n_out"] == [490, 490, 490]
        assert np.abs(out[-1].points() - a["out2_point"]).max() <= 1e-10 * 2000
        assert abs(kept["ETransmission"][i] - scene["ETransmission"]) <= 1e-9
        if i == 5:   # detector at 500 mm = the focus for d = 500: summary comparable with the fixture's detector
            pass


def test_config_2toroidals_twisted(twin):
    kept = _run(_load("CONFIG_2toroidals_twisted.py"))
    assert len(kept["OpticalChain"]) == 10
    for i, name in ((0, "c3_twisted_chain00"), (4, "c3_twisted_chain04"), (9, "c3_twisted_chain09")):
        scene, a = load_golden(name)
        out = kept["OpticalChain"][i].get_output_rays()
        assert [len(o) for o in out] == [673, 673, 673]
        for k in range(3):
            assert np.array_equal(out[k].numbers(), a[f"out{k}_number"])
            assert np.abs(out[k].points() - a[f"out{k}_point"]).max() <= 1e-10 * 2000
        assert abs(kept["ETransmission"][i] - 85.58) < 0.01
    # autofocus ran (AutoDetectorDistance=True): finite optimum near the nominal 600 mm
    for d, s, t in zip(kept["Detector"], kept["SpotSizeSD"], kept["DurationSD"]):
        assert 500 < d.get_distance() < 700 and np.isfinite(s) and np.isfinite(t)


@pytest.mark.parametrize("name", ["CONFIG_toroidal2f-2f.py", "CONFIG_toroidal2f-2f_byhand.py",
                                  "CONFIG_CollimatingTelescope.py"])
def test_other_configs_run(twin, name):
    kept = _run(_load(name))
    assert len(kept["OpticalChain"]) >= 1
    for ch, et in zip(kept["OpticalChain"], kept["ETransmission"]):
        assert len(ch.get_output_rays()[-1]) > 0
        assert 0 < et <= 100.0 + 1e-9


def test_config_deformed(twin):
    """CONFIG_deformed.py: a Fourrier height map with smallest = 0.01 mm on a 40 x 40 mm support = 8000 x 8000
    samples (0.5 GB as fp64, synthesised with a 4001 x 8000 complex FFT).  Slow-ish on CPU."""
    np.random.seed(1)
    mod = _load("CONFIG_deformed.py")
    D = mod.DeformedMirror.DeformationList[0]
    assert D.deformation.shape == (8000, 8000) and abs(D.rms - 0.1) < 1e-12
    kept = _run(mod)
    out = kept["OpticalChain"][0].get_output_rays()[-1]
    assert len(kept["OpticalChain"][0].source_rays) == 999 and len(out) == 202      # same count as the Zernike fixtures
    assert np.isfinite(kept["SpotSizeSD"][0]) and kept["SpotSizeSD"][0] > 0
