"""CPU: ModuleAnalysisAndPlots.EncircledEnergyCurve draws what the result holds -- checked on the DATA inside the figure,
on the Agg backend, with a result built from the NumPy restatement's numbers (no device)."""
import matplotlib
matplotlib.use("Agg")
import numpy as np
import pytest

import quantile_common as qc


def test_encircled_energy_curve_shows_the_result():
    import matplotlib.pyplot as plt
    import ART.ModuleAnalysisAndPlots as mplots
    from attosecondraytracing_amd import quantile
    rng = np.random.default_rng(3)
    n, shift, fr = 300, 30, [0.5, 0.9]
    keys = np.stack([np.abs(rng.normal(size=n)), 2 * np.abs(rng.normal(size=n))])
    radii = np.linspace(0.0, 6.0, 25)
    r = qc.restate(keys, None, None, fr, shift, radii)
    q = quantile.Quantiles(r["values"], r["below"], r["upto"], r["totals"], shift, fr, np.tile(radii, (2, 1)),
                           r["rank_sums"], r["rank_counts"])
    res = quantile.EncircledEnergy(q, np.zeros((2, 4)), [0.0, 0.5], "radius", radii)
    fig = mplots.EncircledEnergyCurve(res)
    ax = fig.axes[0]
    steps = [l for l in ax.lines if len(l.get_xdata()) == len(radii)]
    marks = [l for l in ax.lines if l.get_marker() == "o"]
    assert len(steps) == 2 and len(marks) == 2
    for p in range(2):
        assert np.array_equal(np.asarray(steps[p].get_ydata()), res.enclosed[p])
        assert np.array_equal(np.asarray(marks[p].get_xdata()), res.radii[p])
        assert np.array_equal(np.asarray(marks[p].get_ydata()), fr)
    assert "HEW" in ax.get_title() and "mm" in ax.get_xlabel()
    assert fig._art_encircled is res
    plt.close(fig)
    bare = quantile.EncircledEnergy(quantile.Quantiles(r["values"], r["below"], r["upto"], r["totals"], shift, fr),
                                    np.zeros((2, 4)), [0.0, 0.5], "Delay")
    with pytest.raises(ValueError, match="Radii"):
        mplots.EncircledEnergyCurve(bare)
