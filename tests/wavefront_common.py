"""NumPy statement of the wavefront model of art_wavefront (include/art_hip.h): the oracle of tests/test_wavefront_host.py
and tests/test_gpu_wavefront.py.  W, the pupil coordinates and d.n in the header's operation order, the Andersen
polynomials from ModuleDefects.zernike_monomials, the Gram matrix G, and a host solve by weighted least squares on the
design matrix itself (not on G)."""
import numpy as np

from attosecondraytracing_amd.ModuleDefects import zernike_monomials


def zernike_matrix(x, y, order):
    """[J, n]: Z_j(x, y) in column order j = n (n + 1) / 2 + m."""
    tables = zernike_monomials(max(order, 2))
    return np.stack([np.polynomial.polynomial.polyval2d(x, y, tables[(n, m)].astype(float))
                     for n in range(order + 1) for m in range(n + 1)])


def rays(P, D, path, alive, w, centre, normal, rot, ref=(0.0, 0.0, 0.0), L_ref=0.0, pupil=(0.0, 0.0, 0.0)):
    """dict: used (mask over the slots), outside (count), rho, and over the used rays W, x, y, dn, w."""
    alive = np.asarray(alive).astype(bool)
    P, D, L = np.asarray(P, float), np.asarray(D, float), np.asarray(path, float)
    C, nr = np.asarray(centre, float), np.asarray(normal, float)
    Rm = np.asarray(rot, float).reshape(3, 3)
    e1, e2 = Rm[0], Rm[1]
    X, Y, s = ref
    R = ((C + X * e1) + Y * e2) - s * nr
    dx, dy, dz = D[:, 0], D[:, 1], D[:, 2]
    W = (L - L_ref) + ((dx * (R[0] - P[:, 0]) + dy * (R[1] - P[:, 1])) + dz * (R[2] - P[:, 2]))
    xr = ((dx * e1[0] + dy * e1[1]) + dz * e1[2]) - pupil[0]
    yr = ((dx * e2[0] + dy * e2[1]) + dz * e2[2]) - pupil[1]
    dn = (dx * nr[0] + dy * nr[1]) + dz * nr[2]
    rho = pupil[2]
    if not rho > 0:
        m = (xr[alive] ** 2 + yr[alive] ** 2).max() if alive.any() else 0.0
        rho = np.sqrt(m) if m > 0 else 1.0
    with np.errstate(invalid="ignore"):
        x, y = xr / rho, yr / rho
    used = alive & ((x * x + y * y <= 1.0) if pupil[2] > 0 else True)
    ww = np.ones(len(P)) if w is None else np.asarray(w, float)
    return {"used": used, "outside": int((alive & ~used).sum()), "rho": rho, "W": W[used], "x": x[used],
            "y": y[used], "dn": dn[used], "w": ww[used], "W_all": W, "x_all": x, "y_all": y}


def gram(r, order):
    """G [K, K] of the rows [Z_0 .. Z_{J-1}, d.n, W] of the used rays."""
    V = np.vstack([zernike_matrix(r["x"], r["y"], order), r["dn"][None, :], r["W"][None, :]])
    return (V * r["w"][None, :]) @ V.T


def out_row(r, order):
    """art_wavefront's output row for the rays r."""
    import attosecondraytracing_amd._abi as abi
    K = (order + 1) * (order + 2) // 2 + 2
    row = np.zeros(abi.ART_WAVEFRONT_DOUBLES)
    n = len(r["W"])
    G = gram(r, order)
    row[0], row[1], row[6] = n, r["outside"], K
    if n:
        row[2], row[3], row[4], row[5] = r["w"].sum(), r["rho"], r["W"].min(), r["W"].max()
        row[8:8 + K * (K + 1) // 2] = G[np.triu_indices(K)]
    return row


def fit(r, order):
    """(coefficients [J], rms_residual, (dX, dY, dZ) of the best point, rms_best) by weighted least squares on the design
    matrices.  The best point solves min || W + p + dX d.e1 + dY d.e2 + dZ d.n ||_w."""
    sw = np.sqrt(r["w"])
    Z = zernike_matrix(r["x"], r["y"], order).T
    c = np.linalg.lstsq(Z * sw[:, None], r["W"] * sw, rcond=None)[0]
    res = r["W"] - Z @ c
    rms_residual = np.sqrt((r["w"] * res ** 2).sum() / r["w"].sum())
    A = np.stack([np.ones_like(r["x"]), r["x"] * r["rho"], r["y"] * r["rho"], r["dn"]], axis=1)
    beta = np.linalg.lstsq(A * sw[:, None], -r["W"] * sw, rcond=None)[0]
    res = r["W"] + A @ beta
    rms_best = np.sqrt((r["w"] * res ** 2).sum() / r["w"].sum() - ((r["w"] * res).sum() / r["w"].sum()) ** 2)
    return c, rms_residual, (beta[1], beta[2], beta[3]), rms_best


def of_bundle(B, det, wf, radius=0.0):
    """The oracle's rays for bundle B on det with the arguments a Wavefront wf was computed with (radius: the explicit
    PupilRadius, 0 for the default)."""
    import focal_common as fc
    d = det._desc()
    P, D, L, alive, w = fc.bundle_arrays(B)
    return rays(P, D, L, alive, w, np.array(d.centre[:]), np.array(d.normal[:]), np.array(d.rot[:]),
                (wf.centre[0], wf.centre[1], wf.shift), wf.ref_path,
                (wf.pupil_centre[0], wf.pupil_centre[1], radius))
