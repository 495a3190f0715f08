"""An independent evaluation of a normalised likelihood term (csrc/dz_ode.h, NORMALISED READOUTS), for test_ode_normalize_cpu: from the
UN-normalised simulate of the twin object without `normalize` -- existing code with the same bits of m -- it normalises in
numpy.longdouble and sums the residuals (m' - d)^2 / sd^2 directly, never through the expanded form; and it evaluates the first-order
rounding bound of the expanded form.  Nothing here is collected."""
import numpy as np

LD = np.longdouble
U = 2.0 ** -53
LOG_2PI_HALF = LD(0.5) * np.log(LD(2.0) * LD(np.pi))


def _normaliser(m, z, t):
    """(lo, g) of one trajectory m[T] in longdouble: m' = (m - lo) / g"""
    if z.kind == "max":
        return LD(0.0), np.max(m)
    if z.kind == "ref":
        return LD(0.0), m[int(np.flatnonzero(np.asarray(t) == z.t)[0])]
    return np.min(m), np.max(m) - np.min(m)


def terms(twin_sim, normalize, t, data, sd, sigma=None):
    """(value, bound) per point for an object whose observables are ALL normalised: twin_sim [n, T, O] un-normalised, data and sd
    O x T (sd: the weights where sigma is given), sigma [n] or None.  value: sum over the observed entries of
    -r^2 / 2 - ln s - ln(2 pi) / 2, r = (m' - d) / s, s = sd (sigma * sd with a Noise), summed directly in longdouble.  bound: per point
    the sum over the observables of 4 (T + 8) 2^-53 (A z^2 + 2 |B| z + D) -- for "minmax" with the primed sums plus
    |A| + 2 |lo C| + lo^2 W (times z^2: the unit of A') --, under a Noise divided by sigma^2, the unit in which Q enters the term."""
    n, T, O = twin_sim.shape
    seen = np.isfinite(data)
    d = np.where(seen, data, 0.0).astype(LD)
    iw = np.where(seen, 1.0 / np.where(seen, sd, 1.0), 0.0).astype(LD)
    value, bound = np.zeros(n, dtype=LD), np.zeros(n, dtype=LD)
    for i in range(n):
        a = LD(1.0) if sigma is None else LD(sigma[i])
        for q, z in enumerate(normalize):
            m = twin_sim[i, :, q].astype(LD)
            lo, g = _normaliser(m, z, t)
            r = ((m - lo) / g - d[q]) * iw[q] / a
            ln_s = np.where(seen[q], np.log(np.where(seen[q], sd[q], 1.0).astype(LD)), LD(0.0))
            nq = LD(np.sum(seen[q]))
            value[i] += np.sum(-LD(0.5) * r * r) - np.sum(ln_s) - nq * np.log(a) - nq * LOG_2PI_HALF
            zz = LD(1.0) / g
            p, e = m * iw[q], d[q] * iw[q]
            A, B, C, D, W = np.sum(p * p), np.sum(p * e), np.sum(p * iw[q]), np.sum(e * e), np.sum(iw[q] * iw[q])
            size = np.sum(((m - lo) * iw[q]) ** 2) * zz * zz + 2 * abs(np.sum((m - lo) * iw[q] * e)) * zz + D
            if z.kind == "minmax":
                size += (abs(A) + 2 * abs(lo * C) + lo * lo * W) * zz * zz
            bound[i] += 4 * (T + 8) * U * size / (a * a)
    return value, bound
