"""Networks for the tests of NORMALISED READOUTS, MassActionODELogLike(normalize=[...]): ode_networks' Michaelis-Menten (substrate and
product observed) with its readouts normalised to their own time course, alone, with a steady row and under conditions (one of them
without enzyme: a product that is identically zero), the lane-group and wave networks of ode_equilibrate_networks, and
ode_settle_networks' combined case with `normalize` on top of every other feature.  All synthetic: the data are the un-normalised twin's
own simulation at the nominal constants, normalised in numpy -- they only define a likelihood on the normalised scale; what the tests
compare against is ode_normalize_reference, scipy's Radau and the host build's bits.  Nothing here is collected."""
import functools

import numpy as np

from pydream_amd.likelihoods import MassActionODELogLike, Noise, Normalize

from . import ode_equilibrate_networks as EQ
from . import ode_networks as NW
from . import ode_settle_networks as SN

INF = np.inf
MM_OBS = [[0, 1, 0, 0], [0, 0, 0, 1]]
KINDS = ("max", "ref", "minmax")
MM_SIGMA = 3                # the coordinate of the sampled noise level, behind MM's three rates
MM_LOG_SIGMA = -1.2


def mm_points():
    """the issue's point set: all 259 integrate, hi >= 0.19, hi - lo >= 0.18, the first row >= 0.0033"""
    return NW.box_points(NW.MM_NOMINAL, 259, 21, width=1.0, outside=0.05)


def with_sigma(X, value=MM_LOG_SIGMA, spread=0.3):
    """the rows of X with a fourth coordinate, log10 sigma in value +- spread (seeded)"""
    rng = np.random.default_rng(5)
    return np.ascontiguousarray(np.c_[X, value + spread * rng.uniform(-1, 1, len(X))])


def normalized(m, z, t):
    """numpy's restatement of a Normalize on the rows m[..., T] (double precision; the tests' reference works in longdouble)"""
    if z is None:
        return m
    if z.kind == "max":
        return m / np.max(m, axis=-1, keepdims=True)
    if z.kind == "ref":
        return m / m[..., [int(np.flatnonzero(np.asarray(t) == z.t)[0])]]
    lo, hi = np.min(m, axis=-1, keepdims=True), np.max(m, axis=-1, keepdims=True)
    return (m - lo) / (hi - lo)


def mm_normalize(kind, steady=False):
    """[substrate's, product's] Normalize of a kind: a "ref" is the first output time on the substrate (it falls to 1e-28 at the end)
    and the last one -- the steady row where there is one -- on the product"""
    if kind == "ref":
        return [Normalize("ref", float(NW.MM_T[0])), Normalize("ref", INF if steady else float(NW.MM_T[-1]))]
    return [Normalize(kind), Normalize(kind)]


@functools.lru_cache(maxsize=None)
def _mm_trajectory(y0, steady):
    """[O, T] of the un-normalised observables at the nominal constants: the host build at tight tolerances"""
    t = SN.with_steady_row(NW.MM_T) if steady else NW.MM_T
    tight = MassActionODELogLike(4, NW.MM_REACTIONS, list(y0), t, MM_OBS, np.full((2, len(t)), np.nan), 1.0, rtol=1e-10, atol=1e-12, max_steps=20000)
    sim = tight.simulate(NW.MM_NOMINAL)[0]
    assert np.all(np.isfinite(sim))
    return sim.T.copy()


def mm_experiment(normalize, y0=NW.MM_Y0, steady=False, noisy=False):
    """dict(y0, data, sd): data on the normalised scale with one entry not observed; sd 5 % + 0.01, or with a Noise weights around 1"""
    t = SN.with_steady_row(NW.MM_T) if steady else NW.MM_T
    m = _mm_trajectory(tuple(float(v) for v in y0), bool(steady))
    with np.errstate(invalid="ignore", divide="ignore"):
        data = np.array([normalized(m[q], z, t) for q, z in enumerate(normalize or [None, None])])
    data = np.where(np.isfinite(data), data, 0.5)                  # (a trajectory that is identically zero: any number, the item fails)
    data[0, 3] = np.nan
    sd = 1.0 + 0.25 * np.cos(np.arange(data.size).reshape(data.shape)) if noisy else 0.05 * np.abs(data) + 0.01
    return dict(y0=np.asarray(y0, dtype=float), data=data, sd=sd)


def mm(normalize, steady=False, noisy=False, **kw):
    """Michaelis-Menten with both readouts normalised (normalize: the two entries, or None: the twin without the keyword, same data);
    noisy: Noise(sigma) with sigma = 10**x[3] on both observables"""
    e = mm_experiment(kw.pop("data_like", normalize), steady=steady, noisy=noisy)
    t = SN.with_steady_row(NW.MM_T) if steady else NW.MM_T
    if noisy:
        kw.setdefault("noise", [Noise(MM_SIGMA), Noise(MM_SIGMA)])
    return MassActionODELogLike(4, NW.MM_REACTIONS, e["y0"], t, MM_OBS, e["data"], e["sd"], normalize=normalize, **kw)


def mm_twin(normalize, **kw):
    """the object of mm(normalize, ...) without the keyword: existing code with the same bits of m"""
    return mm(None, data_like=normalize, **kw)


# the three conditions: the plain experiment, a double dose of substrate, and no enzyme -- the product is identically zero
MM_CONDITION_Y0 = ([0.5, 2.0, 0.0, 0.0], [0.5, 4.0, 0.0, 0.0], [0.0, 2.0, 0.0, 0.0])


def mm_conditions(normalize, y0s=MM_CONDITION_Y0, params=None, **kw):
    """(multi, one): MM under conditions; one(c) is the single-experiment object of condition c (made without "params").
    params: {condition: mapping} -- a condition's view of the point"""
    exps = [mm_experiment(normalize, y0=y0) for y0 in y0s]
    conds = [dict(e, **({"params": params[c]} if params and c in params else {})) for c, e in enumerate(exps)]
    multi = MassActionODELogLike(4, NW.MM_REACTIONS, None, NW.MM_T, MM_OBS, None, None, conditions=conds, normalize=normalize, **kw)

    def one(c, **kw2):
        e = exps[c]
        return MassActionODELogLike(4, NW.MM_REACTIONS, e["y0"], NW.MM_T, MM_OBS, e["data"], e["sd"], normalize=normalize, **dict(kw, **kw2))
    return multi, one


# ---------------------------------------------------------------- lane groups and the wave
def group_normalize(O, t):
    """the observables of a group network cycle through "max", "ref" at the last time, "minmax" and None"""
    cycle = (Normalize("max"), Normalize("ref", float(t[-1])), Normalize("minmax"), None)
    return [cycle[q % 4] for q in range(O)]


def group(name, noisy=True):
    """(like, nominal): the named network of ode_equilibrate_networks (enzyme13 @ 16, chain17 @ 32, chain33 @ 64) with its readouts
    normalised; noisy: every second normalised observable carries Noise(0.05)"""
    S, rx, y0, t, obs, nominal, sd_rel, lanes = EQ.network(name)
    t, obs = np.asarray(t, dtype=float), np.asarray(obs, dtype=float)
    norm = group_normalize(len(obs), t)
    m = EQ._data(name, tuple(np.asarray(y0, dtype=float)), (), False, 0.0)
    data = np.array([normalized(m[q], z, t) for q, z in enumerate(norm)])
    noise = [Noise(0.05) if z is not None and q % 2 else None for q, z in enumerate(norm)] if noisy else None
    data[0, 1] = np.nan
    like = MassActionODELogLike(S, rx, y0, t, obs, data, sd_rel * np.abs(data) + 0.01, lanes_per_point=lanes, normalize=norm, noise=noise)
    return like, nominal


# ---------------------------------------------------------------- everything together
def combined(lanes):
    """ode_settle_networks' combined case of the build -- conditions, Monomials, events, equilibrate, rate laws, noise, inputs, a view and
    the steady row -- with `normalize`: observable 2 (no Noise) as fold change over the steady row, observable 3 with Noise(sigma) rescaled
    to [0, 1], the input's own trajectory as a fraction of its maximum.  (The case's data stay on the natural scale: they only define a
    likelihood.)"""
    from . import ode_combined_networks as CB
    case = SN.steady_case(lanes)
    O = len(case.observables)
    noise = list(case.noise)
    noise[3], noise[O - 1] = Noise(CB.P_SIGMA), None
    norm = [None] * O
    norm[2], norm[3], norm[O - 1] = Normalize("ref", INF), Normalize("minmax"), Normalize("max")
    return case, case.steady_like(noise=noise, normalize=norm)
