"""Result summaries and plots, API of ART/ModuleAnalysisAndPlots.py.

`getETransmission` and `GetResultSummary` (the two functions ARTmain needs for its numbers) are built on the
device reductions.  SpotDiagram, DelayGraph and MirrorProjection are matplotlib adaptors fed from the device
(_plots.py: statistics over all rays, markers for a down-sampled subset); RayRenderGraph, a PyVista scene in the
reference, is drawn on matplotlib's 3-D axes from the same geometry (the image has no PyVista)."""

from . import ModuleGeometry as mgeo
from . import ModuleProcessing as mp
from .bundle import RayBundle

def _sum_intensity(rays):
    if isinstance(rays, RayBundle):
        if rays.intensity is None:
            raise TypeError("rays carry no intensity")
        # the sum of a bundle's intensities is remembered with the bundle (per version): the chains of a loop list share
        # their source, and ARTmain asks for its sum once per chain
        hit = getattr(rays, "_sum_w", None)
        if hit is None or hit[0] != rays.version:
            hit = rays._sum_w = (rays.version, float(rays.backend.bundle_sums(rays.view(), rays.intensity, rays.n_slots)[7]))
        return hit[1]
    return sum(r.intensity for r in rays)


def getETransmission(RayListIn, RayListOut) -> float:
    """Energy transmission in percent (ART/ModuleAnalysisAndPlots.py:62-77)."""
    return 100 * _sum_intensity(RayListOut) / _sum_intensity(RayListIn)


def _summary_from_analysis(Detector, ana, verbose=False):
    """GetResultSummary's numbers from a device analysis of the bundle on `Detector` (analysis.BundleAnalysis)."""
    from .ModuleDetector import LightSpeed
    FocalSpotSizeSD, DurationSD = ana.spot_duration(0.0, False)
    if verbose:
        s = ana.bbox
        FocalSpotSize = max(s[1] - s[0], s[3] - s[2])
        delay_range = (s[5] - s[4]) / LightSpeed * 1e15
        print("At the detector distance of " + "{:.3f}".format(Detector.get_distance()) + " mm we get:\n"
              + "Spatial std : " + "{:.3f}".format(FocalSpotSizeSD * 1e3) + " μm and min-max: "
              + "{:.3f}".format(FocalSpotSize * 1e3) + " μm\n"
              + "Temporal std : " + "{:.3e}".format(DurationSD) + " fs and min-max : "
              + "{:.3e}".format(delay_range) + " fs")
    return FocalSpotSizeSD, DurationSD


def GetResultSummary(Detector, RayListAnalysed, verbose=False):
    """Spot-size and duration standard deviations at the detector (ART/ModuleAnalysisAndPlots.py:81-129).
    For a RayBundle everything is reduced on the device (analysis.analyse: moment sums + bounding box in one pass, reused
    if `Detector.autoplace` has just analysed this bundle); no per-ray array is copied."""
    if isinstance(RayListAnalysed, RayBundle):
        return _summary_from_analysis(Detector, Detector._analysis_of(RayListAnalysed), verbose)
    P = Detector.get_PointList2DCentre(RayListAnalysed)
    FocalSpotSizeSD = mp.StandardDeviation(P)
    DelayList = Detector.get_Delays(RayListAnalysed)
    DurationSD = mp.StandardDeviation(DelayList)
    if verbose:
        FocalSpotSize = mgeo.DiameterPointList(P)
        delay_range = max(DelayList) - min(DelayList)
        print("At the detector distance of " + "{:.3f}".format(Detector.get_distance()) + " mm we get:\n"
              + "Spatial std : " + "{:.3f}".format(FocalSpotSizeSD * 1e3) + " μm and min-max: "
              + "{:.3f}".format(FocalSpotSize * 1e3) + " μm\n"
              + "Temporal std : " + "{:.3e}".format(DurationSD) + " fs and min-max : "
              + "{:.3e}".format(delay_range) + " fs")
    return FocalSpotSizeSD, DurationSD


def _getDetectorPoints(RayListAnalysed, Detector):
    from . import _plots
    return _plots._getDetectorPoints(RayListAnalysed, Detector)


def SpotDiagram(RayListAnalysed, Detector, DrawAiryAndFourier=False, ColorCoded=None):
    """Spot diagram on the detector, optionally colour-coded by "Intensity", "Incidence" or "Delay"; left/right keys
    move the detector (ART/ModuleAnalysisAndPlots.py:133-281)."""
    from . import _plots
    return _plots.SpotDiagram(RayListAnalysed, Detector, DrawAiryAndFourier, ColorCoded)


def DelayGraph(RayListAnalysed, Detector, DeltaFT, DrawAiryAndFourier=False, ColorCoded=None):
    """3-D spot diagram with the ray delays on the third axis (ART/ModuleAnalysisAndPlots.py:360-441)."""
    from . import _plots
    return _plots.DelayGraph(RayListAnalysed, Detector, DeltaFT, DrawAiryAndFourier, ColorCoded)


def MirrorProjection(OpticalChain, ReflectionNumber: int, Detector=None, ColorCoded=None):
    """Impact points on one optical element in its support frame (ART/ModuleAnalysisAndPlots.py:444-525)."""
    from . import _plots
    return _plots.MirrorProjection(OpticalChain, ReflectionNumber, Detector, ColorCoded)


def SpotImage(RayListAnalysed, Detector, Bins=200):
    """Image of the X-Y histogram of all rays on the detector, binned on the device; left/right move the detector."""
    from . import _plots
    return _plots.SpotImage(RayListAnalysed, Detector, Bins)


def DelayProfile(RayListAnalysed, Detector, Bins=200):
    """Histogram of the delays of all rays on the detector, binned on the device; left/right move the detector."""
    from . import _plots
    return _plots.DelayProfile(RayListAnalysed, Detector, Bins)


def SpectrometerImage(OpticalChain, Detector, Wavelengths, Bins=200, Range=None, Show=True):
    """What a spectrometer's camera sees: the spot images of `Wavelengths` (mm) behind a chain with one grating
    (OpticalChain.get_SpectralRays: one fan-out launch), summed on the device into one X-Y histogram on Detector.
    Returns (figure or None with Show=False, histogram.Histogram)."""
    from . import histogram
    h = histogram.spectrometer_histogram(Detector, OpticalChain.get_SpectralRays(Wavelengths), Bins, Range)
    if not Show:
        return None, h
    from . import _plots
    plt = _plots._plt()
    fig, ax = plt.subplots()
    img = h.intensity if h.intensity is not None else h.counts
    im = ax.imshow(np.asarray(img).T, origin="lower", aspect="auto", interpolation="nearest",
                   extent=[h.edges[0][0], h.edges[0][-1], h.edges[1][0], h.edges[1][-1]])
    fig.colorbar(im).set_label("Intensity (arb.u.)" if h.intensity is not None else "Rays per bin")
    ax.set_title("Spectrometer image, {} wavelengths".format(len(np.atleast_1d(Wavelengths))))
    ax.set_xlabel("X (mm)")
    ax.set_ylabel("Y (mm)")
    fig._art_hist = h
    return fig, h


def MirrorFootprint(OpticalChain, ReflectionNumber: int, Bins=200):
    """Image of the footprint of all rays on one optical element, binned on the device, over its support outline."""
    from . import _plots
    return _plots.MirrorFootprint(OpticalChain, ReflectionNumber, Bins)


def FocalSpot(RayListAnalysed, Detector, Size=None, Pixels=128, Log=False):
    """Image of the coherent focal intensity (Detector.get_FocalField) with the Airy circle and the Strehl ratio;
    left/right move the detector and re-sum."""
    from . import _plots
    return _plots.FocalSpot(RayListAnalysed, Detector, Size, Pixels, Log)


def SourceImage(RayListAnalysed, Detector, RaysPerSource=None, Groups=None, Size=None, Pixels=128, Log=False):
    """The partially coherent image of an extended source (Detector.get_FocalImage) beside the fully coherent
    |get_FocalField|^2 of the same bundle on the same grid."""
    from . import _plots
    return _plots.SourceImage(RayListAnalysed, Detector, RaysPerSource, Groups, Size, Pixels, Log)


def ThroughFocus(RayListAnalysed, Detector, Shifts, Size=None, Pixels=64):
    """Strehl ratio and peak position of the coherent focal field against the detector shift (all planes in one call)."""
    from . import _plots
    return _plots.ThroughFocus(RayListAnalysed, Detector, Shifts, Size, Pixels)


def PulseAtFocus(RayListAnalysed, Detector, DeltaFT, Size=None, Pixels=64):
    """The pulse at focus (Detector.get_FocalPulse): I(X, t) along the peak row, I(Y, t) along the peak column, and the
    on-peak and pixel-integrated temporal profiles against the Fourier-limited Gaussian of DeltaFT (fs)."""
    from . import _plots
    return _plots.PulseAtFocus(RayListAnalysed, Detector, DeltaFT, Size, Pixels)


def CoatedPulseAtFocus(OpticalChain, Coatings, Detector, DeltaFT, Polarisation, Size=None, Pixels=64, Centre=None):
    """The pulse at focus behind the chain's coatings (OpticalChain.get_FocalPulse): sum_c |A_c|^2 through the peak in
    X and Y, and its temporal profile against the one an ideal coating gives and the Fourier limit of DeltaFT (fs)."""
    from . import _plots
    return _plots.CoatedPulseAtFocus(OpticalChain, Coatings, Detector, DeltaFT, Polarisation, Size, Pixels, Centre)


def PulseThroughFocus(RayListAnalysed, Detector, DeltaFT, Shifts, Size=None, Pixels=64):
    """Space-time Strehl ratio and on-peak duration of the pulse against the detector shift (all planes in one call)."""
    from . import _plots
    return _plots.PulseThroughFocus(RayListAnalysed, Detector, DeltaFT, Shifts, Size, Pixels)


def ChromaticFocus(result):
    """The focus of a chromatic source (the result of get_ChromaticFocalPulse with several Shifts): the on-axis spectral
    intensity over (detector shift, omega) with the plane of best focus of every frequency drawn over it, and the
    pulse duration per plane."""
    from . import _plots
    return _plots.ChromaticFocus(result)


def SensitivityChart(result, Quantity="centroid_x", PerUnit=None):
    """The alignment sensitivities of a chain (the result of OpticalChain.get_Sensitivities) as a bar chart of one quantity
    (sensitivity.QUANTITIES: centroid, delay, spot and path variance, spread) per degree of freedom, shifts and rotations
    on axes of their own; PerUnit = (mm, rad) rescales the bars to moves of that size."""
    from . import _plots
    return _plots.SensitivityChart(result, Quantity, PerUnit)


def CompensationChart(result, After=None):
    """A compensator solve (the result of OpticalChain.get_Compensation) as bar charts: the singular values of the solved
    matrix, and the variances of X, Y and the path before, predicted and -- with After, the variances of a re-trace --
    after the moves."""
    from . import _plots
    return _plots.CompensationChart(result, After)


def EncircledEnergyCurve(result):
    """The encircled-energy curves of a focus (the result of Detector.get_EncircledEnergy with Radii): the enclosed share
    of the power over the radii, one line per plane, with the requested fractions marked at their radii."""
    from . import _plots
    return _plots.EncircledEnergyCurve(result)


def WavefrontMap(RayListAnalysed, Detector, Order=8, Pixels=128, Remove=("piston", "tilt")):
    """The fitted wavefront (Detector.get_Wavefront) on the pupil, in waves, with the terms in `Remove` taken out, and a
    bar chart of the Zernike terms' rms contributions in waves."""
    from . import _plots
    return _plots.WavefrontMap(RayListAnalysed, Detector, Order, Pixels, Remove)


def WavefrontScan(OpticalChainList, Detectors, Terms=((2, 0), (2, 1), (2, 2), (3, 1), (3, 2)), Order=8):
    """Chosen Zernike terms (waves) and the rms at the best reference point against each chain's loop_variable_value,
    for the last bundle of every chain on its detector, all chains in one device call."""
    from . import _plots
    return _plots.WavefrontScan(OpticalChainList, Detectors, Terms, Order)


def RayRenderGraph(OpticalChain, EndDistance=None, maxRays=300, OEpoints=3000, scale_spheres=5.0, draw_mesh=False,
                   cycle_ray_colors=False):
    """3-D picture of the optical setup and the traced rays (ART/ModuleAnalysisAndPlots.py:616-673)."""
    from . import _plots
    return _plots.RayRenderGraph(OpticalChain, EndDistance, maxRays, OEpoints, scale_spheres, draw_mesh, cycle_ray_colors)


def generate_distinct_colors(num_colors):
    from . import _plots
    return _plots.generate_distinct_colors(num_colors)


def show():
    from . import _plots
    return _plots.show()
