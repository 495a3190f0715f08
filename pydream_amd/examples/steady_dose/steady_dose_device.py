"""A dose-response curve read at steady state, on the device: measurements "after the system has settled", an output time of +inf
(MassActionODELogLike(t=[..., inf], settle=...)).

    X + E -> Xp + E     k1      the kinase E modifies X
    Xp -> X             k2      the modification is removed

At a kinase dose E the modified fraction settles at Xp = Xtot k1 E / (k1 E + k2).  Six doses, one condition per dose.  Five of them are
pure steady-state read-outs: only the row at t = inf carries data.  A steady state fixes the ratio k1 / k2 and nothing else, so the sixth
condition is a short time course at one dose, which fixes the time scale k1 E + k2.  The output times are shared by the conditions of an
object, so t = [0.25, 0.5, ..., 2.0, inf] for all six and the five steady-state conditions carry the time course's rows unobserved (NaN);
`horizon`, the length of time over which the state is to stand still, is given: it is a statement about the assay ("read after 30 time
units at the earliest"), not about the time course's two units.  The read-out is in arbitrary units (scale = Monomial({2: 1})):

    theta = log10 [k1, k2, scale]

sd 4 % + 0.02; a uniform prior two decades wide around the nominal values.  The data are the closed form at the nominal values with one
draw of the measurement error; the closed form is also checked against simulate at every point of a box (check_closed_form).  The run
ends with the posterior-predictive dose-response curve.

    python -m pydream_amd.examples.steady_dose.steady_dose_device [niterations] [nchains] [--host]

--host: the same run with the likelihood's host twin as a plain Python callable (run_dream's host path) and the prediction by the host
build, which gives the same bits.
"""
import hashlib
import sys

import numpy as np

from pydream_amd.likelihoods import MassActionODELogLike, Monomial, posterior_predictive

X_, XP, E = range(3)
K1, K2, SCALE = range(3)
REACTIONS = [({X_: 1, E: 1}, {XP: 1, E: 1}, K1), ({XP: 1}, {X_: 1}, K2)]
NOMINAL = np.log10([1.5, 0.6, 20.0])
WIDTH = 1.0
XTOT = 1.0
DOSES = (0.03, 0.1, 0.3, 1.0, 3.0, 0.5)         # the last one is the time course's
COURSE = len(DOSES) - 1
TSPAN = np.r_[np.linspace(0.25, 2.0, 8), np.inf]
HORIZON = 30.0
OBSERVABLES = np.zeros((1, 3))
OBSERVABLES[0, XP] = 1.0
SD_REL, SD_ABS = 0.04, 0.02


def steady_xp(x, dose):
    """Xtot k1 E / (k1 E + k2) for the rows of x"""
    x = np.asarray(x, dtype=float)
    k1, k2 = 10.0 ** x[..., K1], 10.0 ** x[..., K2]
    return XTOT * k1 * dose / (k1 * dose + k2)


def simulated_data(seed=11):
    """The scaled read-out [doses, 1, T] at the nominal values from the closed form -- Xp(t) = Xp* (1 - exp(-(k1 E + k2) t)), Xp(inf) =
    Xp* -- with one draw of the measurement error; the finite rows of the steady-state conditions are NaN (not observed)."""
    k1, k2, scale = 10.0 ** NOMINAL
    rng = np.random.default_rng(seed)
    data = np.full((len(DOSES), 1, len(TSPAN)), np.nan)
    for c, dose in enumerate(DOSES):
        clean = scale * steady_xp(NOMINAL, dose) * (1.0 - np.exp(-(k1 * dose + k2) * TSPAN))
        noisy = clean + (SD_REL * np.abs(clean) + SD_ABS) * rng.standard_normal(len(TSPAN))
        data[c, 0, -1] = noisy[-1]
        if c == COURSE:
            data[c, 0] = noisy
    return data


def make_likelihood(data=None, **kw):
    data = simulated_data() if data is None else np.asarray(data, dtype=float)
    sd = SD_REL * np.abs(np.nan_to_num(data)) + SD_ABS
    conditions = [dict(y0=[XTOT, 0.0, dose], data=data[c], sd=sd[c]) for c, dose in enumerate(DOSES)]
    kw.setdefault("settle", dict(horizon=HORIZON))
    return MassActionODELogLike(3, REACTIONS, None, TSPAN, OBSERVABLES, None, None, rate_scale="log10", conditions=conditions,
                                scale=[Monomial({SCALE: 1})], **kw)


def check_closed_form(like, X):
    """simulate's steady row against the closed form, for the rows of X.  X + Xp and E do not move, so the system is one linear
    equation, f = -(k1 E + k2) (Xp - Xp*), and the steady-state test |f| horizon <= sqrt(S) (atol + rtol Xp) bounds the distance from
    Xp*.  Returns the largest distance in units of that bound (<= 1 up to rounding)."""
    X = np.asarray(X, dtype=float).reshape(-1, len(NOMINAL))
    sim, y = like.simulate(X), like.settled_state(X)
    scale = 10.0 ** X[:, SCALE]
    worst = 0.0
    for c, (dose, cond) in enumerate(zip(DOSES, like.conditions)):
        st = cond["settle"]
        assert np.all(np.isfinite(sim[:, c])) and np.all(y[:, c, E] == dose)
        rate = 10.0 ** X[:, K1] * dose + 10.0 ** X[:, K2]
        bound = np.sqrt(3.0) * (st["atol"] + st["rtol"] * np.abs(y[:, c, XP])) / (rate * st["horizon"])
        worst = max(worst, float(np.max(np.abs(sim[:, c, -1, 0] - scale * steady_xp(X, dose)) / (scale * bound))))
    assert worst <= 1.0 + 1e-6, worst
    return worst


class HostTwin:
    """The likelihood as a plain Python callable: run_dream takes the host path"""
    def __init__(self, like):
        self.like = like

    def __call__(self, x):
        return self.like(x)


def main(niterations=400, nchains=64, host=False, like=None, seed=43):
    from scipy.stats import uniform
    from pydream_amd.core import run_dream
    from pydream_amd.parameters import SampledParam
    like = make_likelihood() if like is None else like
    rng = np.random.default_rng(seed)
    worst = check_closed_form(like, NOMINAL - WIDTH + 2 * WIDTH * rng.uniform(size=(64, len(NOMINAL))))
    starts = [NOMINAL + 0.25 * WIDTH * rng.uniform(-1, 1, len(NOMINAL)) for _ in range(nchains)]
    sampled, log_ps = run_dream([SampledParam(uniform, loc=NOMINAL - WIDTH, scale=2 * WIDTH)], HostTwin(like) if host else like,
                                niterations=niterations, nchains=nchains, multitry=5, start=starts, model_name="steady_dose_device", verbose=False,
                                save_history=False, seed=seed + 1, nseedchains=max(10 * like.d, 2 * nchains))
    S, L = np.concatenate(sampled), np.concatenate(log_ps)
    print("a dose-response curve read at steady state on %s (%d doses per proposal, each settled; host check against Xtot k1 E / (k1 E + k2): "
          "%.3f of the test's bound): %d chains x %d iterations; best log p %.3f at log10 [k1, k2, scale] = %s (true %s)"
          % ("the host twin" if host else "the device", len(DOSES), worst, nchains, niterations, L.max(), np.round(S[np.argmax(L)], 3), np.round(NOMINAL, 3)))
    rows, sim = posterior_predictive(sampled, like, burnin=niterations // 2, thin=5, device=not host)
    sim = sim[np.all(np.isfinite(sim), axis=(1, 2, 3))]
    bands = np.percentile(sim[:, :, -1, 0], [5, 50, 95], axis=0)         # [3, doses]: the steady row
    print("posterior predictive on the %s: %d rows x %d doses; median steady read-out by dose %s: %s; bands digest %s"
          % ("host" if host else "device", len(sim), len(DOSES), list(DOSES), np.round(bands[1], 3), hashlib.sha256(bands.tobytes()).hexdigest()[:16]))
    return sampled, log_ps, bands


if __name__ == "__main__":
    argv = [a for a in sys.argv[1:] if a != "--host"]
    main(*(int(a) for a in argv[:2]), host="--host" in sys.argv[1:])
