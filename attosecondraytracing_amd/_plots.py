"""matplotlib adaptors for the plot entry points of ART/ModuleAnalysisAndPlots.py (SpotDiagram :133-281, DelayGraph
:284-441, MirrorProjection :444-525, RayRenderGraph :529-673), fed from device-resident bundles.

Numbers shown in the legends (spot size, standard deviations, numerical aperture) are reduced on the device over
ALL rays; the scatter itself shows at most MAX_POINTS survivors, evenly spaced in ray order, because a figure cannot
resolve more and 1e7 markers would take minutes to draw.  matplotlib is imported on first use only, so the tracing
path never depends on it.  The 3-D scene render (RayRenderGraph) is PyVista's in the reference; the image has no
PyVista, so the same geometry (`render_scene`) is drawn on matplotlib's 3-D axes."""
import numpy as np

from . import ModuleProcessing as mp
from .bundle import RayBundle

MAX_POINTS = 20000
_COLOUR_LABELS = {"Intensity": "Intensity (arb.u.)", "Incidence": "Incidence angle (deg)", "Delay": "Delay (fs)"}


def _plt():
    import matplotlib.pyplot as plt
    return plt


def _sample_positions(m, cap=None):
    cap = cap or MAX_POINTS
    return np.arange(m) if m <= cap else np.unique(np.linspace(0, m - 1, cap).astype(np.int64))


def _detector_sample(B, Detector, pos):
    """Read-out of the bundle on the detector: per-ray values of the sampled survivors + statistics of all rays."""
    import torch
    from .ModuleDetector import LightSpeed
    ro = Detector.readout(B, sync=True)
    s = ro["stats"]
    slots = B.index().index_select(0, torch.as_tensor(pos, device=B.backend.device))
    take = lambda t: t.index_select(0, slots).cpu().numpy()
    cx, cy = 0.5 * (s[2] + s[3]), 0.5 * (s[4] + s[5])          # CentrePointList: bounding-box centre
    mean_opl = s[1] / s[0]
    spot_sd, dur_sd = Detector._spot_duration_from_moments(Detector._scan_moments(B), 0.0, False)
    return {"x_um": (take(ro["X"]) - cx) * 1e3, "y_um": (take(ro["Y"]) - cy) * 1e3,
            "delay_fs": (take(ro["opl"]) - mean_opl) / LightSpeed * 1e15,
            "size": max(s[3] - s[2], s[5] - s[4]), "spot_sd": spot_sd, "dur_sd": dur_sd, "slots": slots}


def _ray_property(B, slots, which):
    if which == "Intensity":
        if B.intensity is None:
            raise TypeError("rays carry no intensity")
        return B.intensity.index_select(0, slots).cpu().numpy()
    if which == "Incidence":
        return np.rad2deg(B.data[7].index_select(0, slots).cpu().numpy())
    raise ValueError(which)


def _getDetectorPoints(RayListAnalysed, Detector):
    """(x in um, y in um, spot diameter in mm, spot standard deviation in mm), ART/ModuleAnalysisAndPlots.py:28-58;
    the coordinate arrays hold the displayed sample, the two numbers describe all rays."""
    B = RayBundle.of(RayListAnalysed)
    d = _detector_sample(B, Detector, _sample_positions(len(B)))
    return d["x_um"], d["y_um"], d["size"], d["spot_sd"]


def _dist_step(size, NA):
    return min(50, max(0.0005, round(size / 8 / np.arcsin(NA) * 10000) / 10000))


def _shift(moving, dist, step, key):
    """Cursor-key handling shared by the interactive figures: returns the new distance or None."""
    if key == "right":
        moving.shiftByDistance(step)
        return dist + step
    if key == "left":
        if dist > 1.5 * step:
            moving.shiftByDistance(-step)
            return dist - step
        moving.shiftToDistance(0.5 * step)
        return 0.5 * step
    return None


def SpotDiagram(RayListAnalysed, Detector, DrawAiryAndFourier=False, ColorCoded=None):
    plt = _plt()
    B = RayBundle.of(RayListAnalysed)
    NA = mp.ReturnNumericalAperture(B, 1)
    airy = mp.ReturnAiryRadius(B.wavelength, NA) * 1e3 if DrawAiryAndFourier else 0
    pos = _sample_positions(len(B))
    state = {"dist": Detector.get_distance(), "det": Detector.copy_detector()}

    def colours(d):
        if ColorCoded == "Delay":
            return d["delay_fs"]
        if ColorCoded in ("Intensity", "Incidence"):
            return _ray_property(B, d["slots"], ColorCoded)
        return "red"

    def label(d):
        extra = "\n{:.2f} fs SD".format(d["dur_sd"]) if ColorCoded == "Delay" else ""
        return "{:.3f} mm\n{:.1f} μm SD".format(state["dist"], d["spot_sd"] * 1e3) + extra

    d = _detector_sample(B, Detector, pos)
    state["step"] = _dist_step(d["size"], NA)
    plt.ion()
    fig, ax = plt.subplots()
    if DrawAiryAndFourier:
        th = np.linspace(0, 2 * np.pi, 100)
        ax.plot(airy * np.cos(th), airy * np.sin(th), c="black")
    sc = ax.scatter(d["x_um"], d["y_um"], c=colours(d), s=15, label=label(d))
    cbar = None
    if ColorCoded in _COLOUR_LABELS:
        cbar = fig.colorbar(sc)
        cbar.set_label(_COLOUR_LABELS[ColorCoded])
    head = {None: "Spot Diagram", "Intensity": "Intensity + Spot Diagram", "Incidence": "Ray Incidence + Spot Diagram",
            "Delay": "Delay + Spot Diagram"}.get(ColorCoded, "Spot Diagram")
    ax.set_title(head + "\n press left/right to move detector position")
    ax.set_xlabel("X (µm)")
    ax.set_ylabel("Y (µm)")

    def frame(d):
        lim = 1.1 * max(airy, 0.5 * d["size"] * 1000)
        ax.set_xlim(-lim, lim)
        ax.set_ylim(-lim, lim)
        ax.legend(loc="upper right")

    frame(d)

    def press(event):
        new = _shift(state["det"], state["dist"], state["step"], event.key)
        if new is None:
            return
        state["dist"] = new
        d = _detector_sample(B, state["det"], pos)
        sc.set_offsets(np.column_stack([d["x_um"], d["y_um"]]))
        if ColorCoded == "Delay":
            sc.set_array(d["delay_fs"])
            sc.set_clim(d["delay_fs"].min(), d["delay_fs"].max())
            cbar.update_normal(sc)
        sc.set_label(label(d))
        frame(d)
        state["step"] = _dist_step(d["size"], NA)
        fig.canvas.draw_idle()

    fig.canvas.mpl_connect("key_press_event", press)
    fig._art_press = press          # lets tests drive the handler without a GUI event loop
    plt.show()
    return fig


def _draw_delay_graph(B, Detector, dist, DeltaFT, DrawAiryAndFourier, ColorCoded, fig, pos, NA):
    plt = _plt()
    airy = mp.ReturnAiryRadius(B.wavelength, NA) * 1e3
    d = _detector_sample(B, Detector, pos)
    if fig is None:
        fig = plt.figure()
    else:
        fig.clear(keep_observers=True)
    ax = fig.add_subplot(111, projection="3d")
    ax.set_xlabel("X (µm)")
    ax.set_ylabel("Y (µm)")
    ax.set_zlabel("Delay (fs)")
    lab = "{:.3f} mm\n{:.1f} μm SD\n{:.2f} fs SD".format(dist, d["spot_sd"] * 1e3, d["dur_sd"])
    c = _ray_property(B, d["slots"], ColorCoded) if ColorCoded in ("Intensity", "Incidence") else d["delay_fs"]
    ax.scatter(d["x_um"], d["y_um"], d["delay_fs"], s=4, c=c, label=lab)
    ax.set_title({"Intensity": "Delay + Intensity graph", "Incidence": "Delay + Incidence graph"}.get(ColorCoded, "Delay graph")
                 + "\n press left/right to move detector position")
    ax.legend(loc="upper right")
    if DrawAiryAndFourier:
        x = np.linspace(-airy, airy, 40)
        z = np.linspace(d["delay_fs"].mean() - DeltaFT * 0.5, d["delay_fs"].mean() + DeltaFT * 0.5, 40)
        x, z = np.meshgrid(x, z)
        y = np.sqrt(np.maximum(airy ** 2 - x ** 2, 0.0))
        ax.plot_wireframe(x, y, z, color="grey", alpha=0.1)
        ax.plot_wireframe(x, -y, z, color="grey", alpha=0.1)
    lim = 1.1 * max(airy, 0.5 * d["size"] * 1000)
    ax.set_xlim(-lim, lim)
    ax.set_ylim(-lim, lim)
    return fig, d["size"]


def DelayGraph(RayListAnalysed, Detector, DeltaFT, DrawAiryAndFourier=False, ColorCoded=None):
    plt = _plt()
    B = RayBundle.of(RayListAnalysed)
    NA = mp.ReturnNumericalAperture(B, 1)
    pos = _sample_positions(len(B))
    state = {"dist": Detector.get_distance(), "det": Detector.copy_detector()}
    plt.ion()
    fig, size = _draw_delay_graph(B, Detector, state["dist"], DeltaFT, DrawAiryAndFourier, ColorCoded, None, pos, NA)
    state["step"] = _dist_step(size, NA)

    def press(event):
        new = _shift(state["det"], state["dist"], state["step"], event.key)
        if new is None:
            return
        state["dist"] = new
        ax = fig.axes[0]
        view = (ax.azim, ax.elev)
        _, size = _draw_delay_graph(B, state["det"], new, DeltaFT, DrawAiryAndFourier, ColorCoded, fig, pos, NA)
        fig.axes[0].view_init(elev=view[1], azim=view[0])
        state["step"] = _dist_step(size, NA)
        fig.canvas.draw_idle()

    fig.canvas.mpl_connect("key_press_event", press)
    fig._art_press = press
    plt.show()
    return fig


def MirrorProjection(OpticalChain, ReflectionNumber: int, Detector=None, ColorCoded=None):
    plt = _plt()
    import torch
    from mpl_toolkits.axes_grid1 import make_axes_locatable
    from . import ModuleGeometry as mgeo
    oe = OpticalChain.optical_elements[ReflectionNumber]
    B = OpticalChain.get_output_rays()[ReflectionNumber]
    pos = _sample_positions(len(B))
    slots = B.index().index_select(0, torch.as_tensor(pos, device=B.backend.device))
    # hit points in the support frame: the optic frame without the shift to the mirror centre
    fwd, _ = mgeo.frame_maps(oe.normal, oe.majoraxis)
    P = B.data[0:3].index_select(1, slots).cpu().numpy().T - np.asarray(oe.position, dtype=float)
    xy = P @ fwd.T
    if ColorCoded in ("Intensity", "Incidence"):
        z = _ray_property(B, slots, ColorCoded)
    elif ColorCoded == "Delay":
        if Detector is None:
            raise ValueError("If you want to project ray delays, you must specify a detector.")
        z = _detector_sample(B, Detector, pos)["delay_fs"]
    else:
        z = "red"
    title = {"Intensity": "Ray intensity projected on mirror              ",
             "Incidence": "Ray incidence projected on mirror              ",
             "Delay": "Ray delay at detector projected on mirror              "}.get(ColorCoded, "Ray impact points projected on mirror")
    plt.ion()
    fig = plt.figure()
    ax = oe.type.support._ContourSupport(fig)
    p = ax.scatter(xy[:, 0], xy[:, 1], c=z, s=15)
    if ColorCoded in _COLOUR_LABELS:
        cax = make_axes_locatable(ax).append_axes("right", size="5%", pad=0.05)
        fig.colorbar(p, cax=cax).set_label(_COLOUR_LABELS[ColorCoded])
    ax.set_xlabel("x (mm)")
    ax.set_ylabel("y (mm)")
    ax.set_title(title, loc="right")
    ax.autoscale_view()
    fig.tight_layout()
    plt.show()
    return fig


def _binned(h):
    """What a histogram plot shows: the intensity when the rays carry it, else the counts."""
    return h.counts if h.intensity is None else h.intensity


def _spot_image_data(B, Detector, Bins):
    """X-Y histogram of all rays on the detector + the bounding-box centre, its size and the spot SD."""
    h = Detector.get_Histogram(B, ("X", "Y"), Bins)
    s = Detector.readout(B, store=False, lite=True)["stats"]
    cx, cy = 0.5 * (s[2] + s[3]), 0.5 * (s[4] + s[5])
    spot_sd, _ = Detector._spot_duration_from_moments(Detector._scan_moments(B), 0.0, False)
    extent = ((h.edges[0][0] - cx) * 1e3, (h.edges[0][-1] - cx) * 1e3, (h.edges[1][0] - cy) * 1e3,
              (h.edges[1][-1] - cy) * 1e3)
    return h, extent, max(s[3] - s[2], s[5] - s[4]), spot_sd


def _interactive(fig, B, Detector, size, redraw):
    """left/right move a copy of the detector as in SpotDiagram; redraw(detector, distance) re-bins and returns the size."""
    NA = mp.ReturnNumericalAperture(B, 1)
    state = {"dist": Detector.get_distance(), "det": Detector.copy_detector(), "step": _dist_step(size, NA)}

    def press(event):
        new = _shift(state["det"], state["dist"], state["step"], event.key)
        if new is None:
            return
        state["dist"] = new
        state["step"] = _dist_step(redraw(state["det"], new), NA)
        fig.canvas.draw_idle()

    fig.canvas.mpl_connect("key_press_event", press)
    fig._art_press = press
    fig._art_state = state          # (tests: the distance and step of the next press)


def SpotImage(RayListAnalysed, Detector, Bins=200):
    """Image of the X-Y histogram of ALL rays on the detector (intensity, or counts without intensities), in µm about
    the bounding-box centre; left/right move the detector and re-bin."""
    plt = _plt()
    B = RayBundle.of(RayListAnalysed)
    h, extent, size, spot_sd = _spot_image_data(B, Detector, Bins)
    plt.ion()
    fig, ax = plt.subplots()
    im = ax.imshow(_binned(h).T, origin="lower", extent=extent, aspect="auto", interpolation="nearest")
    fig.colorbar(im).set_label("Intensity (arb.u.)" if h.intensity is not None else "Rays per bin")
    key, = ax.plot([], [], " ", label="{:.3f} mm\n{:.1f} μm SD".format(Detector.get_distance(), spot_sd * 1e3))
    ax.legend(loc="upper right")
    ax.set_title("Spot image\n press left/right to move detector position")
    ax.set_xlabel("X (µm)")
    ax.set_ylabel("Y (µm)")
    fig._art_hist = h

    def redraw(det, dist):
        h, extent, size, spot_sd = _spot_image_data(B, det, Bins)
        im.set_data(_binned(h).T)
        im.set_extent(extent)
        im.autoscale()
        key.set_label("{:.3f} mm\n{:.1f} μm SD".format(dist, spot_sd * 1e3))
        ax.legend(loc="upper right")
        fig._art_hist = h
        return size

    _interactive(fig, B, Detector, size, redraw)
    plt.show()
    return fig


def _delay_profile_data(B, Detector, Bins):
    h = Detector.get_Histogram(B, ("Delay",), Bins)
    s = Detector.readout(B, store=False, lite=True)["stats"]
    _, dur_sd = Detector._spot_duration_from_moments(Detector._scan_moments(B), 0.0, False)
    return h, max(s[3] - s[2], s[5] - s[4]), dur_sd


def DelayProfile(RayListAnalysed, Detector, Bins=200):
    """Step plot of the delay histogram of ALL rays on the detector (fs about the mean path; intensity, or counts
    without intensities); left/right move the detector and re-bin."""
    plt = _plt()
    B = RayBundle.of(RayListAnalysed)
    h, size, dur_sd = _delay_profile_data(B, Detector, Bins)
    plt.ion()
    fig, ax = plt.subplots()
    st = ax.stairs(_binned(h), h.edges[0], label="{:.3f} mm\n{:.2f} fs SD".format(Detector.get_distance(), dur_sd))
    ax.legend(loc="upper right")
    ax.set_title("Delay profile\n press left/right to move detector position")
    ax.set_xlabel("Delay (fs)")
    ax.set_ylabel("Intensity (arb.u.)" if h.intensity is not None else "Rays per bin")
    fig._art_hist = h

    def redraw(det, dist):
        h, size, dur_sd = _delay_profile_data(B, det, Bins)
        st.set_data(_binned(h), h.edges[0])
        st.set_label("{:.3f} mm\n{:.2f} fs SD".format(dist, dur_sd))
        ax.relim()
        ax.autoscale_view()
        ax.legend(loc="upper right")
        fig._art_hist = h
        return size

    _interactive(fig, B, Detector, size, redraw)
    plt.show()
    return fig


def _focal_spot_data(B, Detector, Size, Pixels, Log):
    """The focal field on the detector, the image to show (log10 of the intensity over its peak with Log) and its
    extent in µm, and the size of the geometric spot (for the step of the next detector move)."""
    f = Detector.get_FocalField(B, Size=Size, Pixels=Pixels)
    img = f.intensity[0]
    if Log:
        img = np.log10(np.maximum(img / max(img.max(), np.finfo(float).tiny), 1e-12))
    dx = 0.5 * (f.x[1] - f.x[0]) if len(f.x) > 1 else 0.5
    dy = 0.5 * (f.y[1] - f.y[0]) if len(f.y) > 1 else 0.5
    extent = ((f.x[0] - dx) * 1e3, (f.x[-1] + dx) * 1e3, (f.y[0] - dy) * 1e3, (f.y[-1] + dy) * 1e3)
    s = Detector.readout(B, store=False, lite=True)["stats"]
    return f, img, extent, max(s[3] - s[2], s[5] - s[4], f.x[-1] - f.x[0])


def FocalSpot(RayListAnalysed, Detector, Size=None, Pixels=128, Log=False):
    """Image of the coherent focal intensity (Detector.get_FocalField) in µm, detector coordinates, with the Airy circle
    about the grid centre and the Strehl ratio in the title; left/right move the detector and re-sum."""
    plt = _plt()
    B = RayBundle.of(RayListAnalysed)
    f, img, extent, size = _focal_spot_data(B, Detector, Size, Pixels, Log)
    airy = mp.ReturnAiryRadius(f.wavelength, mp.ReturnNumericalAperture(B, 1)) * 1e3
    cx, cy = 0.5 * (extent[0] + extent[1]), 0.5 * (extent[2] + extent[3])
    plt.ion()
    fig, ax = plt.subplots()
    im = ax.imshow(img, origin="lower", extent=extent, aspect="equal", interpolation="nearest")
    fig.colorbar(im).set_label("log10 intensity / peak" if Log else "Intensity (arb.u.)")
    if airy > 0:
        ax.add_patch(plt.Circle((cx, cy), airy, facecolor="none", edgecolor="w", linestyle="--", label="Airy radius"))
    title = "Focal spot, {:.3f} mm, Strehl {:.3f}\n press left/right to move detector position"
    ax.set_title(title.format(Detector.get_distance(), f.strehl[0]))
    ax.set_xlabel("X (µm)")
    ax.set_ylabel("Y (µm)")
    fig._art_focal = f

    def redraw(det, dist):
        f, img, extent, size = _focal_spot_data(B, det, Size, Pixels, Log)
        im.set_data(img)
        im.set_extent(extent)
        im.autoscale()
        ax.set_title(title.format(dist, f.strehl[0]))
        fig._art_focal = f
        return size

    _interactive(fig, B, Detector, size, redraw)
    plt.show()
    return fig


def SourceImage(RayListAnalysed, Detector, RaysPerSource=None, Groups=None, Size=None, Pixels=128, Log=False):
    """Two images in µm, detector coordinates, on one grid: the partially coherent image of an extended source
    (Detector.get_FocalImage, its Strehl ratio and rms widths in the title) and the fully coherent |get_FocalField|^2
    of the same bundle, each over its own maximum."""
    plt = _plt()
    B = RayBundle.of(RayListAnalysed)
    g = Detector.get_FocalImage(B, RaysPerSource=RaysPerSource, Groups=Groups, Size=Size, Pixels=Pixels)
    centre = (0.5 * (g.x[0] + g.x[-1]), 0.5 * (g.y[0] + g.y[-1]))
    size = (max(g.x[-1] - g.x[0], np.finfo(float).tiny), max(g.y[-1] - g.y[0], np.finfo(float).tiny))
    f = Detector.get_FocalField(B, Size=size, Pixels=(len(g.x), len(g.y)), Centre=centre, RefPath=g.ref_path)
    dx = 0.5 * (g.x[1] - g.x[0]) if len(g.x) > 1 else 0.5
    dy = 0.5 * (g.y[1] - g.y[0]) if len(g.y) > 1 else 0.5
    extent = ((g.x[0] - dx) * 1e3, (g.x[-1] + dx) * 1e3, (g.y[0] - dy) * 1e3, (g.y[-1] + dy) * 1e3)

    def shown(img):
        img = img / max(img.max(), np.finfo(float).tiny)
        return np.log10(np.maximum(img, 1e-12)) if Log else img

    plt.ion()
    fig, (a1, a2) = plt.subplots(1, 2, sharex=True, sharey=True)
    for ax, img, name in ((a1, g.intensity[0].cpu().numpy(), "Partially coherent, {} groups".format(g.groups)),
                          (a2, f.intensity[0], "Coherent")):
        im = ax.imshow(shown(img), origin="lower", extent=extent, aspect="equal", interpolation="nearest")
        fig.colorbar(im, ax=ax, shrink=0.6).set_label("log10 intensity / peak" if Log else "Intensity / peak")
        ax.set_title(name)
        ax.set_xlabel("X (µm)")
    a1.set_ylabel("Y (µm)")
    fig.suptitle("Source image, {:.3f} mm, Strehl {:.3f}, rms {:.3f} x {:.3f} µm".format(
        Detector.get_distance(), g.strehl[0], g.rms[0, 0] * 1e3, g.rms[0, 1] * 1e3))
    fig._art_image = g
    fig._art_focal = f
    plt.show()
    return fig


def ThroughFocus(RayListAnalysed, Detector, Shifts, Size=None, Pixels=64):
    """Strehl ratio and peak position (µm, detector coordinates) of the coherent focal field against the detector shift
    (mm, Detector.shiftByDistance's sign); all planes are summed in one device call."""
    plt = _plt()
    B = RayBundle.of(RayListAnalysed)
    f = Detector.get_FocalField(B, Size=Size, Pixels=Pixels, Shifts=Shifts)
    plt.ion()
    fig, (a1, a2) = plt.subplots(2, 1, sharex=True)
    a1.plot(f.shifts, f.strehl, "o-")
    a1.set_ylabel("Strehl ratio")
    a1.set_title("Through focus, {:.3f} mm".format(Detector.get_distance()))
    a2.plot(f.shifts, f.peak[:, 0] * 1e3, "o-", label="X")
    a2.plot(f.shifts, f.peak[:, 1] * 1e3, "s-", label="Y")
    a2.set_ylabel("Peak position (µm)")
    a2.set_xlabel("Detector shift (mm)")
    a2.legend(loc="upper right")
    fig._art_focal = f
    plt.show()
    return fig


def PulseAtFocus(RayListAnalysed, Detector, DeltaFT, Size=None, Pixels=64):
    """Three panels of the pulse at focus (Detector.get_FocalPulse): I(X, t) along the row of the space-time peak,
    I(Y, t) along its column (µm, fs), and the on-peak and pixel-integrated temporal profiles, each over its maximum,
    against the Fourier-limited Gaussian of DeltaFT centred on the peak."""
    plt = _plt()
    B = RayBundle.of(RayListAnalysed)
    p = Detector.get_FocalPulse(B, DeltaFT, Size=Size, Pixels=Pixels)
    I = p.intensity[0]
    n, l, j = np.unravel_index(int(np.argmax(I)), I.shape)
    t = p.t
    dt = 0.5 * (t[1] - t[0]) if len(t) > 1 else 0.5

    def extent(a):
        da = 0.5 * (a[1] - a[0]) if len(a) > 1 else 0.5
        return ((a[0] - da) * 1e3, (a[-1] + da) * 1e3, t[0] - dt, t[-1] + dt)

    plt.ion()
    fig, (a1, a2, a3) = plt.subplots(1, 3, figsize=(15, 4.5))
    for ax, img, axis, name in ((a1, I[:, l, :], p.x, "X"), (a2, I[:, :, j], p.y, "Y")):
        im = ax.imshow(img, origin="lower", extent=extent(axis), aspect="auto", interpolation="nearest")
        fig.colorbar(im, ax=ax).set_label("Intensity (arb.u.)")
        ax.set_xlabel(f"{name} (µm)")
        ax.set_ylabel("t (fs)")
        ax.set_title(f"I({name}, t) through the peak")
    peak_t = p.peak[0, 2] if np.isfinite(p.peak[0, 2]) else 0.0
    a3.plot(t, I[:, l, j] / max(I[:, l, j].max(), np.finfo(float).tiny), label=f"on peak, FWHM {p.duration[0]:.3g} fs")
    a3.plot(t, p.profile[0] / max(p.profile[0].max(), np.finfo(float).tiny),
            label=f"integrated, FWHM {p.duration_integrated[0]:.3g} fs")
    a3.plot(t, np.exp(-4 * np.log(2) * (t - peak_t) ** 2 / DeltaFT ** 2), "k--",
            label=f"Fourier limit, {DeltaFT:.3g} fs")
    a3.set_xlabel("t (fs)")
    a3.set_ylabel("Intensity / maximum")
    a3.legend(loc="upper right")
    a3.set_title("Pulse at {:.3f} mm, Strehl {:.3f}".format(Detector.get_distance(), p.strehl[0]))
    fig._art_pulse = p
    plt.show()
    return fig


def CoatedPulseAtFocus(OpticalChain, Coatings, Detector, DeltaFT, Polarisation, Size=None, Pixels=64, Centre=None):
    """Three panels of the pulse at focus behind the chain's coatings (OpticalChain.get_FocalPulse): sum_c |A_c|^2 as
    I(X, t) along the row of the space-time peak and I(Y, t) along its column (µm, fs), and the on-peak temporal
    profile against the one Coating.ideal() on every mirror gives on the same pixel (both over the ideal maximum, so
    the loss shows) and the Fourier-limited Gaussian of DeltaFT."""
    from .coating import Coating
    plt = _plt()
    kw = dict(Size=Size, Pixels=Pixels, Centre=Centre)
    p = OpticalChain.get_FocalPulse(Coatings, Detector, DeltaFT, Polarisation, **kw)
    ideal = OpticalChain.get_FocalPulse(Coating.ideal(), Detector, DeltaFT, Polarisation, RefPath=p.ref_path,
                                        TimeWindow=p.time_window, Times=len(p.t), **kw)
    I = p.intensity[0]
    n, l, j = np.unravel_index(int(np.argmax(I)), I.shape)
    t = p.t
    dt = 0.5 * (t[1] - t[0]) if len(t) > 1 else 0.5

    def extent(a):
        da = 0.5 * (a[1] - a[0]) if len(a) > 1 else 0.5
        return ((a[0] - da) * 1e3, (a[-1] + da) * 1e3, t[0] - dt, t[-1] + dt)

    plt.ion()
    fig, (a1, a2, a3) = plt.subplots(1, 3, figsize=(15, 4.5))
    for ax, img, axis, name in ((a1, I[:, l, :], p.x, "X"), (a2, I[:, :, j], p.y, "Y")):
        im = ax.imshow(img, origin="lower", extent=extent(axis), aspect="auto", interpolation="nearest")
        fig.colorbar(im, ax=ax).set_label("Intensity (arb.u.)")
        ax.set_xlabel(f"{name} (µm)")
        ax.set_ylabel("t (fs)")
        ax.set_title(f"sum |A_c|^2 ({name}, t) through the peak")
    ref = ideal.intensity[0][:, l, j]
    top = max(ref.max(), np.finfo(float).tiny)
    peak_t = ideal.t[int(np.argmax(ref))]
    a3.plot(t, I[:, l, j] / top, label=f"coated, FWHM {p.duration[0]:.3g} fs")
    a3.plot(t, ref / top, label=f"ideal coating, FWHM {ideal.duration[0]:.3g} fs")
    a3.plot(t, np.exp(-4 * np.log(2) * (t - peak_t) ** 2 / DeltaFT ** 2), "k--", label=f"Fourier limit, {DeltaFT:.3g} fs")
    a3.set_xlabel("t (fs)")
    a3.set_ylabel("Intensity / ideal maximum")
    a3.legend(loc="upper right")
    a3.set_title("Pulse at {:.3f} mm, Strehl {:.3g} (ideal coating {:.3g})".format(Detector.get_distance(), p.strehl[0],
                                                                                 ideal.strehl[0]))
    fig._art_pulse, fig._art_ideal = p, ideal
    plt.show()
    return fig


def PulseThroughFocus(RayListAnalysed, Detector, DeltaFT, Shifts, Size=None, Pixels=64):
    """Space-time Strehl ratio and on-peak duration (fs) of the pulse against the detector shift (mm,
    Detector.shiftByDistance's sign); all planes and frequencies are summed in one device call."""
    plt = _plt()
    B = RayBundle.of(RayListAnalysed)
    p = Detector.get_FocalPulse(B, DeltaFT, Size=Size, Pixels=Pixels, Shifts=Shifts)
    plt.ion()
    fig, (a1, a2) = plt.subplots(2, 1, sharex=True)
    a1.plot(p.shifts, p.strehl, "o-")
    a1.set_ylabel("Space-time Strehl ratio")
    a1.set_title("Pulse through focus, {:.3f} mm".format(Detector.get_distance()))
    a2.plot(p.shifts, p.duration, "o-", label="on peak")
    a2.plot(p.shifts, p.duration_integrated, "s-", label="integrated")
    a2.axhline(DeltaFT, color="k", linestyle="--", label="Fourier limit")
    a2.set_ylabel("Duration (fs)")
    a2.set_xlabel("Detector shift (mm)")
    a2.legend(loc="upper right")
    fig._art_pulse = p
    plt.show()
    return fig


def ChromaticFocus(result):
    """A chromatic.ChromaticFocalPulse, or a chromatic.ChromaticVectorFocalPulse (behind coatings), through focus: the
    spectral intensity |E_j|^2 (the vector result: sum_c |F_c|^2) at the pixel nearest the grid's centre over (detector
    shift, omega) with best_focus drawn over it, and the on-peak and integrated duration (fs) per plane.  Frequencies of
    weight 0 are blank."""
    plt = _plt()
    p = result
    ny, nx = p.spectrum.shape[-2:]
    if p.spectrum.dim() == 5:
        on_axis = (np.abs(p.spectrum[:, :, :, (ny - 1) // 2, (nx - 1) // 2].cpu().numpy()) ** 2).sum(axis=2)   # [P, J]
    else:
        on_axis = np.abs(p.spectrum[:, :, (ny - 1) // 2, (nx - 1) // 2].cpu().numpy()) ** 2        # [P, J]
    used = np.abs(p.weights) > 0
    image = np.where(used[None, :], on_axis, np.nan)
    order = np.argsort(p.shifts)
    plt.ion()
    fig, (a1, a2) = plt.subplots(2, 1)
    if len(order) > 1 and len(p.omega) > 1:
        mesh = a1.pcolormesh(p.shifts[order], p.omega, image[order].T, shading="nearest")
        fig.colorbar(mesh, ax=a1, label="|E|^2 on axis")
    else:
        a1.plot(p.omega, image[0], ".")
    a1.plot(p.best_focus[used], p.omega[used], "w.", markersize=3, label="best focus")
    a1.set_xlabel("Detector shift (mm)")
    a1.set_ylabel("omega (rad/fs)")
    a1.set_title("Chromatic focus")
    a1.legend(loc="upper right")
    a2.plot(p.shifts[order], p.duration[order], "o-", label="on peak")
    a2.plot(p.shifts[order], p.duration_integrated[order], "s-", label="integrated")
    a2.set_xlabel("Detector shift (mm)")
    a2.set_ylabel("Duration (fs)")
    a2.legend(loc="upper right")
    fig._art_pulse = p
    plt.show()
    return fig


def SensitivityChart(result, Quantity="centroid_x", PerUnit=None):
    """A sensitivity.Sensitivities as a bar chart: `Quantity` (one of sensitivity.QUANTITIES) per degree of freedom, the
    shifts (per mm) and the rotations (per rad) on axes of their own.  PerUnit = (mm, rad) rescales the bars to the
    effect of moves of that size, e.g. (0.01, 1e-6) for 10 um and 1 urad."""
    plt = _plt()
    v = np.asarray(result.quantity(Quantity), dtype=float)
    scale = (1.0, 1.0) if PerUnit is None else (float(PerUnit[0]), float(PerUnit[1]))
    plt.ion()
    fig, axes = plt.subplots(2, 1)
    for ax, unit, k in zip(axes, ("mm", "rad"), scale):
        pick = [c for c, u in enumerate(result.units) if u == unit]
        ax.bar(range(len(pick)), v[pick] * k)
        ax.set_xticks(range(len(pick)))
        ax.set_xticklabels([f"{who}\n{dof}" for who, dof in (result.names[c] for c in pick)], rotation=90, fontsize=6)
        ax.set_ylabel(f"{Quantity} per {unit}" if PerUnit is None else f"{Quantity} for {k:g} {unit}")
        ax.axhline(0.0, color="k", linewidth=0.5)
    axes[0].set_title(f"Alignment sensitivities, {result.count} rays")
    fig.tight_layout()
    fig._art_sensitivities = result
    plt.show()
    return fig


def CompensationChart(result, After=None):
    """An alignment.Compensation as two bar charts: the singular values of the solved matrix (log scale; the ones below
    the truncation are the directions the adjusters cannot or need not move along) and the variances of X, Y and the path
    before, as the solve predicts them and -- with After = the [3] variances of a re-trace, e.g. the last entry of an
    AlignmentReport's `variance` -- after the moves."""
    plt = _plt()
    plt.ion()
    fig, axes = plt.subplots(2, 1)
    sv = np.asarray(result.singular_values, dtype=float)
    axes[0].bar(range(len(sv)), sv)
    if (sv > 0).any():
        axes[0].set_yscale("log")
    axes[0].set_xticks(range(len(sv)))
    axes[0].set_ylabel("singular values")
    axes[0].set_title(f"Compensation over {len(result.names)} degrees of freedom, rank {result.rank}, {result.count} rays")
    series = [("before", result.variance), ("predicted", result.variance_predicted)]
    if After is not None:
        series.append(("re-traced", np.asarray(After, dtype=float).reshape(3)))
    width = 0.8 / len(series)
    for k, (label, v) in enumerate(series):
        axes[1].bar(np.arange(3) + k * width, np.asarray(v, dtype=float), width, label=label)
    axes[1].set_xticks(np.arange(3) + 0.4 - width / 2)
    axes[1].set_xticklabels(["X", "Y", "path"])
    if (np.asarray(result.variance) > 0).any():
        axes[1].set_yscale("log")
    axes[1].set_ylabel("variance (mm$^2$)")
    axes[1].legend()
    fig.tight_layout()
    fig._art_compensation = result
    plt.show()
    return fig


def EncircledEnergyCurve(result):
    """A quantile.EncircledEnergy as curves: the enclosed share of the power over `Radii`, one step line per plane, with
    every requested fraction marked at its radius.  Needs a result made with Radii."""
    plt = _plt()
    if result.enclosed is None:
        raise ValueError("EncircledEnergyCurve needs a result of get_EncircledEnergy(..., Radii=...)")
    unit = "fs" if result.metric == "Delay" else "mm"
    plt.ion()
    fig, ax = plt.subplots()
    for p, s in enumerate(result.shifts):
        line, = ax.step(result.Radii, result.enclosed[p], where="post", label=f"shift {s:g} mm")
        ax.plot(result.radii[p], result.fractions, "o", color=line.get_color())
    for f in result.fractions:
        ax.axhline(f, color="k", linewidth=0.5, linestyle=":")
    ax.set_xlabel({"radius": "radius", "X": "half width in X", "Y": "half width in Y", "Delay": "half window"}[result.metric]
                  + f" ({unit})")
    ax.set_ylabel("enclosed share of the power")
    ax.set_ylim(0.0, 1.05)
    ax.legend()
    if result.hew is not None:
        ax.set_title("HEW " + ", ".join(f"{v:.4g}" for v in result.hew) + f" {unit}")
    fig._art_encircled = result
    plt.show()
    return fig


def WavefrontMap(RayListAnalysed, Detector, Order=8, Pixels=128, Remove=("piston", "tilt")):
    """The fitted wavefront on the unit pupil in waves (Detector.get_Wavefront, `Remove`d terms taken out) beside a bar
    chart of every term's rms contribution in waves; rms, rms at the best reference point and the Marechal Strehl ratio
    in the title.  Without a wavelength the numbers are in nm."""
    plt = _plt()
    B = RayBundle.of(RayListAnalysed)
    wf = Detector.get_Wavefront(B, Order=Order)
    scale, unit = (1.0 / wf.wavelength, "waves") if np.isfinite(wf.wavelength) else (1e6, "nm")
    img = wf.map(Pixels, remove=Remove) * scale
    plt.ion()
    fig, (a1, a2) = plt.subplots(1, 2, figsize=(12, 5))
    im = a1.imshow(img, origin="lower", extent=(-1, 1, -1, 1), aspect="equal", interpolation="nearest")
    fig.colorbar(im, ax=a1).set_label(f"W ({unit})")
    a1.set_xlabel("pupil x")
    a1.set_ylabel("pupil y")
    a1.set_title("Wavefront, {:.3f} mm, without {}".format(Detector.get_distance(), ", ".join(Remove) or "nothing"))
    keys = [k for k in wf.coefficients if k != (0, 0)]
    a2.bar(range(len(keys)), [wf.term_rms[k] * scale for k in keys])
    a2.set_xticks(range(len(keys)))
    a2.set_xticklabels([f"{n},{m}" for n, m in keys], rotation=90, fontsize=7)
    a2.set_xlabel("Zernike term (n, m)")
    a2.set_ylabel(f"rms on the pupil ({unit})")
    a2.set_title("rms {:.3g}, best focus {:.3g} {}, Strehl (Marechal) {:.3f}".format(
        wf.rms * scale, wf.rms_best * scale, unit, wf.strehl_marechal))
    fig._art_wavefront = wf
    plt.show()
    return fig


def WavefrontScan(OpticalChainList, Detectors, Terms=((2, 0), (2, 1), (2, 2), (3, 1), (3, 2)), Order=8):
    """Chosen Zernike terms and the rms at the best reference point (waves, or nm without a wavelength) against each
    chain's loop_variable_value (its index if it has none), for the last bundle of every chain on its detector
    (`Detectors`: one for all chains, or one per chain); all bundles in one device call (wavefront.wavefronts)."""
    from . import wavefront
    plt = _plt()
    chains = list(OpticalChainList)
    dets = list(Detectors) if isinstance(Detectors, (list, tuple)) else [Detectors] * len(chains)
    if len(dets) != len(chains):
        raise ValueError("Detectors: one detector, or one per chain")
    wfs = wavefront.wavefronts([(c.get_output_rays()[-1], d, {"Order": Order}) for c, d in zip(chains, dets)])
    xs = [c.loop_variable_value if c.loop_variable_value is not None else k for k, c in enumerate(chains)]
    name = chains[0].loop_variable_name if chains and chains[0].loop_variable_name else "chain"
    wl = wfs[0].wavelength if wfs else float("nan")
    scale, unit = (1.0 / wl, "waves") if np.isfinite(wl) else (1e6, "nm")
    plt.ion()
    fig, (a1, a2) = plt.subplots(2, 1, sharex=True)
    for key in Terms:
        a1.plot(xs, [w.coefficients.get(tuple(key), np.nan) * scale for w in wfs], "o-", label="Z{},{}".format(*key))
    a1.set_ylabel(f"coefficient ({unit})")
    a1.legend(loc="upper right", fontsize=8)
    a1.set_title("Wavefront terms against " + str(name))
    a2.plot(xs, [w.rms_best * scale for w in wfs], "o-", label="rms at best focus")
    a2.plot(xs, [w.rms * scale for w in wfs], "s--", label="rms at the detector centre")
    a2.set_ylabel(f"rms ({unit})")
    a2.set_xlabel(str(name))
    a2.legend(loc="upper right")
    fig._art_wavefronts = wfs
    plt.show()
    return fig


def MirrorFootprint(OpticalChain, ReflectionNumber: int, Bins=200):
    """Image of the footprint of ALL rays on one optical element (OpticalChain.get_Footprint) over its support
    outline."""
    plt = _plt()
    h = OpticalChain.get_Footprint(ReflectionNumber, Bins)
    oe = OpticalChain.optical_elements[ReflectionNumber]
    plt.ion()
    fig = plt.figure()
    ax = oe.type.support._ContourSupport(fig)
    im = ax.imshow(_binned(h).T, origin="lower", extent=(h.edges[0][0], h.edges[0][-1], h.edges[1][0], h.edges[1][-1]),
                   aspect="auto", interpolation="nearest", zorder=0)
    fig.colorbar(im, ax=ax).set_label("Intensity (arb.u.)" if h.intensity is not None else "Rays per bin")
    ax.set_xlabel("x (mm)")
    ax.set_ylabel("y (mm)")
    ax.set_title("Footprint on mirror")
    fig._art_hist = h
    plt.show()
    return fig


def _same_slots(a, b):
    """Slot i of both bundles is the same source ray (bundles of one trace share their `number` tensor)."""
    return a.n_slots == b.n_slots and a.number is b.number


def _ray_segments(history, EndDistance, maxRays):
    """Per stage k of the history a (2 m, 3) array of segment end points, pairs in ray order: from the ray's point in
    bundle k to its point in bundle k + 1 for the rays that are still alive there; for the last bundle, from the point
    along the direction over EndDistance (ART/ModuleAnalysisAndPlots.py:563-602).  At most maxRays rays per stage --
    evenly spaced in ray order here, a random draw in the reference.  Only the drawn rays leave the device."""
    import torch
    out = []
    for k, B in enumerate(history):
        last = k == len(history) - 1
        nxt = B if last else history[k + 1]
        pos = _sample_positions(len(nxt), cap=maxRays)
        slots = nxt.index().index_select(0, torch.as_tensor(pos, device=nxt.backend.device))
        P2 = nxt.data[0:3].index_select(1, slots).cpu().numpy().T
        if last:
            P1, P2 = P2, P2 + nxt.data[3:6].index_select(1, slots).cpu().numpy().T * EndDistance
        elif _same_slots(B, nxt):
            P1 = B.data[0:3].index_select(1, slots).cpu().numpy().T
        else:       # bundles that do not share their slots (e.g. built from Ray lists): match the ray numbers
            mine = B.numbers()
            order = np.argsort(mine, kind="stable")
            want = nxt.numbers()[pos]
            at = order[np.searchsorted(mine, want, sorter=order)]
            if not np.array_equal(mine[at], want):
                raise ValueError("a ray of bundle %d has no ancestor in bundle %d" % (k + 1, k))
            P1 = B.points()[at]
        seg = np.empty((2 * len(pos), 3))
        seg[0::2], seg[1::2] = P1, P2
        out.append(seg)
    return out


def _optic_cloud(OE, OEpoints, draw_mesh=False):
    """Sample points of one optical element's surface in the lab frame and the closed index loops of its hole outlines
    (ART/ModuleAnalysisAndPlots.py:529-561).  Without a mesh the cloud sits 0.5 mm behind the surface, so that the ray
    ends on it stay visible."""
    from . import ModuleGeometry as mgeo
    pts, loops = OE.type.get_grid3D(OEpoints, edges=True)
    P = np.asarray(pts, dtype=float).reshape(-1, 3) - np.asarray(OE.type.get_centre(), dtype=float)
    _, bwd = mgeo.frame_maps(OE.normal, OE.majoraxis)
    P = P @ bwd.T + np.asarray(OE.position, dtype=float)
    if not draw_mesh:
        P = P - 0.5 * np.asarray(OE.normal, dtype=float)
    return P, loops


def _optic_triangles(OE, OEpoints):
    """Triangles (index triples into the cloud of _optic_cloud) of the optic's surface for draw_mesh=True: a Delaunay
    triangulation of the sample points in the plane of the support, without the triangles that bridge a hole or a
    concave outline (the reference asks PyVista for a Delaunay mesh constrained by the hole outlines, :544-560)."""
    from matplotlib.tri import Triangulation
    pts = np.asarray(OE.type.get_grid3D(OEpoints), dtype=float).reshape(-1, 3)
    xy = pts[:, :2] - np.asarray(OE.type.get_centre(), dtype=float)[:2]
    if len(xy) < 3:
        return np.empty((0, 3), dtype=np.int64)
    tri = Triangulation(xy[:, 0], xy[:, 1]).triangles
    mid = xy[tri].mean(axis=1)
    inside = np.fromiter((bool(OE.type.support._IncludeSupport(m)) for m in mid), dtype=bool, count=len(mid))
    return tri[inside].astype(np.int64)


def render_scene(OpticalChain, EndDistance=None, maxRays=300, OEpoints=3000, draw_mesh=False):
    """The geometry RayRenderGraph draws, as host arrays (for any renderer): {"segments": one (2 m, 3) array of
    segment end points per stage (source -> element 0, ..., last element -> EndDistance further), "optics": one
    (p, 3) lab-frame point cloud per optical element, "loops": their hole outlines as index loops, "EndDistance",
    "triangles": with draw_mesh, the surface mesh of every optic as index triples into its cloud}."""
    history = [RayBundle.of(OpticalChain.source_rays)] + [RayBundle.of(b) for b in OpticalChain.get_output_rays()]
    if EndDistance is None:
        EndDistance = float(np.linalg.norm(np.asarray(OpticalChain.source_rays[0].point, dtype=float)
                                           - np.asarray(OpticalChain.optical_elements[0].position, dtype=float)))
    clouds = [_optic_cloud(OE, OEpoints, draw_mesh) for OE in OpticalChain.optical_elements]
    return {"segments": _ray_segments(history, EndDistance, maxRays), "optics": [c[0] for c in clouds],
            "loops": [c[1] for c in clouds], "EndDistance": EndDistance,
            "triangles": [_optic_triangles(OE, OEpoints) for OE in OpticalChain.optical_elements] if draw_mesh else None}


def generate_distinct_colors(num_colors):
    """num_colors visually distinct colours (the reference takes colorcet's glasbey palette, :604-614; matplotlib's
    tab20 here)."""
    cmap = _plt().get_cmap("tab20")
    return [cmap(i % 20)[:3] for i in range(num_colors)]


def RayRenderGraph(OpticalChain, EndDistance=None, maxRays=300, OEpoints=3000, scale_spheres=5.0, draw_mesh=False,
                   cycle_ray_colors=False):
    """3-D picture of the optical setup and of at most maxRays traced rays (ART/ModuleAnalysisAndPlots.py:616-673), on
    matplotlib's 3-D axes.  Returns the figure; `fig._art_scene` holds the arrays that were drawn (render_scene)."""
    import colorsys
    from mpl_toolkits.mplot3d.art3d import Line3DCollection
    plt = _plt()
    print("...rendering image of optical chain...", end="", flush=True)
    scene = render_scene(OpticalChain, EndDistance, maxRays, OEpoints, draw_mesh)
    n_stage = len(scene["segments"])
    colors = generate_distinct_colors(n_stage) if cycle_ray_colors else [(0.7, 0.0, 0.0)] * n_stage
    fig = plt.figure(figsize=(15, 5))
    ax = fig.add_subplot(111, projection="3d")
    ax.view_init(elev=20, azim=-75)
    ax.set_proj_type("ortho")           # (a perspective camera clips the near end of a zoomed, elongated box)
    for seg, color in zip(scene["segments"], colors):
        ax.add_collection3d(Line3DCollection(seg.reshape(-1, 2, 3), colors=[color], linewidths=0.6))
    everything = [seg for seg in scene["segments"] if len(seg)]
    for i, (cloud, loops) in enumerate(zip(scene["optics"], scene["loops"])):
        h, sat, v = colorsys.rgb_to_hsv(*colors[min(i + 1, n_stage - 1)])
        pale = colorsys.hsv_to_rgb(h, 0.2 * sat, v)        # the optic in the pale shade of the rays that leave it
        ax.scatter(cloud[:, 0], cloud[:, 1], cloud[:, 2], s=scale_spheres, color=[pale], depthshade=False)
        if draw_mesh:
            tri = scene["triangles"][i]
            if len(tri):
                ax.plot_trisurf(cloud[:, 0], cloud[:, 1], cloud[:, 2], triangles=tri, color=pale, alpha=0.6, linewidth=0)
            for loop in loops:
                ax.plot(*cloud[loop].T, color=pale, linewidth=1.0)
        everything.append(cloud)
    lo, hi = np.concatenate(everything).min(axis=0), np.concatenate(everything).max(axis=0)
    span = np.maximum(hi - lo, 0.08 * float((hi - lo).max()))      # a beam line is thin: no axis flatter than 8 % of the longest
    mid = 0.5 * (lo + hi)
    for setter, c, w in zip((ax.set_xlim, ax.set_ylim, ax.set_zlim), mid, span):
        setter(c - 0.5 * w, c + 0.5 * w)
    ax.set_box_aspect(tuple(span), zoom=1.9)               # equal scales on the three axes, the box shaped like the setup
    fig.subplots_adjust(left=0.0, right=1.0, bottom=0.0, top=1.0)
    ax.set_xlabel("x (mm)")
    ax.set_ylabel("y (mm)")
    ax.set_zlabel("z (mm)")
    fig._art_scene = scene
    print("\r\033[K", end="", flush=True)
    return fig


def show():
    plt = _plt()
    plt.show(block=False)
