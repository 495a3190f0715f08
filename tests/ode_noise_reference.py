"""An independent reference for the sampled-noise likelihood (likelihoods.Noise): from the observables that like.simulate returns and
the noise constants resolved in mpmath (40 digits), the DEFINITION as a sum of log densities -- norm(m, s) or laplace(m, s) at the
data on the linear scale, the same density at ln d around ln m minus ln d on the log scale, norm(m, sd) for an observable without a
Noise.  Nothing here reads the generated code or the data block."""
import mpmath as mp
import numpy as np

from pydream_amd.likelihoods import Monomial

mp.mp.dps = 40
_INT = (int, np.integer)


def constant(c, x, log10):
    """A parameter index, a float or a Monomial at the point x, in mpmath"""
    if isinstance(c, Monomial):
        return mp.mpf(10) ** (mp.mpf(c.log10_factor) + sum(mp.mpf(e) * mp.mpf(float(x[i])) for i, e in c.exponents))
    if isinstance(c, _INT):
        return mp.mpf(10) ** mp.mpf(float(x[c])) if log10 else mp.mpf(float(x[c]))
    return mp.mpf(float(c))


def experiments(like):
    """[(data, sd)] of the object's conditions, or of its single experiment"""
    return [(c["data"], c["sd"]) for c in like.conditions] if like.conditions is not None else [(like.data, like.sd)]


def experiment_loglike(like, x, sim, data, sd):
    """(value, A, N) of one experiment at one point: sim [T, O] from like.simulate; A = |C| + sum |term_i| with C the sum of the
    entries' constants (what does not depend on the point) and term_i the rest of entry i's log density; N: the observed entries."""
    C, terms = mp.mpf(0), []
    half_log_2pi = mp.log(2 * mp.pi) / 2
    for q, z in enumerate(like.noise or [None] * len(like.observables)):
        for j in range(len(like.t)):
            if not np.isfinite(data[q, j]):
                continue
            m, d, w = mp.mpf(float(sim[j, q])), mp.mpf(float(data[q, j])), mp.mpf(float(sd[q, j]))
            if z is None:
                C += -mp.log(w) - half_log_2pi
                terms.append(-((d - m) / w) ** 2 / 2)
                continue
            s = constant(z.sigma, x, like.log10)
            if z.rel is not None:
                s += constant(z.rel, x, like.log10) * abs(m)
            s *= w
            if z.scale == "log":
                C += -mp.log(d)
                m, d = mp.log(m), mp.log(d)
            if z.dist == "normal":
                C += -half_log_2pi
                terms.append(-mp.log(s) - ((d - m) / s) ** 2 / 2)
            else:
                C += -mp.log(2)
                terms.append(-mp.log(s) - abs(d - m) / s)
    return C + sum(terms), abs(C) + sum(abs(t) for t in terms), len(terms)


def loglike(like, X):
    """(value, A, N) per row of X, float arrays: the sum over the object's experiments.  Rows whose simulation is not finite: NaN."""
    X = np.atleast_2d(np.asarray(X, dtype=float))
    sims = like.simulate(X)
    if like.conditions is None:
        sims = sims[:, None]
    out = np.full((len(X), 3), np.nan)
    for i, x in enumerate(X):
        if not np.all(np.isfinite(sims[i])):
            continue
        parts = [experiment_loglike(like, x, sims[i, c], data, sd) for c, (data, sd) in enumerate(experiments(like))]
        out[i] = [float(sum(p[k] for p in parts)) for k in range(3)]
    return out[:, 0], out[:, 1], out[:, 2]


def tolerance(A, N):
    """(32 + N) 2^-52 A: a few roundings per term (the residual, its square or modulus, the log of s and the additions), dexp's
    argument error for sigma within 1e-3 .. 1e3, and N sequential additions whose partial sums A bounds"""
    return (32 + N) * 2.0 ** -52 * A
