"""CONDITION-SPECIFIC PARAMETERS on the device: one enzyme, measured on three gels, in control cells, under siRNA against the enzyme and
with an inhibitor -- experiments that differ in the SYSTEM and not only in what is done to it (MassActionODELogLike with a "params" key
in its conditions: a view of the point per condition, csrc/dz_ode.h, VIEWS).

    E + S <-> ES        kf, kr
    ES -> E + P         kcat

The product P is read out in arbitrary units.  What varies between the six experiments, and how it is written:

    control against siRNA        the enzyme's start amount is Monomial({E_TOT: 1, EFF: 1}) = E_tot * 10**eff, eff the sampled log10 of
                                 the fraction that survives the knock-down; the control conditions fix EFF at 0.0
    control against inhibitor    the inhibitor is known to lower kcat tenfold: the rate is Monomial({KCAT: 1, FACTOR: 1}) and FACTOR is a
                                 FORMAL index -- every condition fixes it, at 0.0 or at -1.0 --, so it costs no sampled coordinate
    three gels                   every gel has its own sampled readout scale: scale=[Monomial({SCALE: 1})] with SCALE -> SCALE + gel

    theta = log10 [kf, kr, kcat, E_tot, eff, scale_0, scale_1, scale_2]

eight coordinates under a uniform prior one decade on each side of the generating values (eff: -1.5 .. 0); 12 readings per experiment,
sd 4 % + 0.02, simulated by the solver itself at tight tolerances with seeded errors of that size.  After the run posterior_predictive
integrates the posterior's rows on a denser grid and numpy makes the 5 / 95 % bands per experiment.

    python -m pydream_amd.examples.knockdown.knockdown_device [niterations] [nchains] [--host]

--host: the same run with the likelihood's host twin as a plain Python callable (run_dream's host path) and the bands from the host
build, which give the same bits.
"""
import sys

import numpy as np

from pydream_amd.likelihoods import MassActionODELogLike, Monomial, posterior_predictive

SPECIES = ("E", "S", "ES", "P")
E, S, ES, P = range(4)
KF, KR, KCAT, E_TOT, EFF, SCALE = range(6)     # SCALE: gel 0's coordinate; gel g reads SCALE + g
FACTOR = SCALE + 3                             # a formal index: fixed in every condition, never read from the point
NDIM = SCALE + 3
REACTIONS = [({E: 1, S: 1}, {ES: 1}, KF), ({ES: 1}, {E: 1, S: 1}, KR), ({ES: 1}, {E: 1, P: 1}, Monomial({KCAT: 1, FACTOR: 1}))]
TRUE = np.log10([2.0, 0.5, 1.0, 0.2, 0.25, 30.0, 45.0, 20.0])      # (a knock-down to a quarter)
LOWER = np.r_[TRUE[:4] - 1.0, -1.5, TRUE[5:] - 1.0]
WIDTH = np.r_[np.full(4, 2.0), 1.5, np.full(3, 2.0)]
TSPAN = np.linspace(0.5, 6.0, 12)
OBSERVABLES = np.zeros((1, 4))
OBSERVABLES[0, P] = 1.0
# (gel, siRNA, inhibitor) per experiment
EXPERIMENTS = ((0, False, False), (0, True, False), (1, False, False), (1, False, True), (2, False, False), (2, True, True))
Y0 = [Monomial({E_TOT: 1, EFF: 1}), 2.0, 0.0, 0.0]


def params_of(gel, sirna, inhibitor):
    """The experiment's view of the point: its gel's scale, the knock-down's efficiency (or none: 0.0), the inhibitor's known factor."""
    view = {SCALE: SCALE + gel, FACTOR: -1.0 if inhibitor else 0.0}
    if not sirna:
        view[EFF] = 0.0
    return view


def _model(data, sd, **kw):
    conditions = [dict(data=data[c], sd=sd[c], params=params_of(*exp)) for c, exp in enumerate(EXPERIMENTS)]
    return MassActionODELogLike(4, REACTIONS, Y0, TSPAN, OBSERVABLES, None, None, rate_scale="log10", conditions=conditions,
                                scale=[Monomial({SCALE: 1})], **kw)


def simulated_data(seed=7):
    """The scaled readout of every experiment at TSPAN for TRUE, [experiments, 1, T], by the host build at rtol = atol = 1e-12, with
    seeded normal errors of sd 4 % + 0.02."""
    shape = (len(EXPERIMENTS), 1, len(TSPAN))
    clean = np.swapaxes(_model(np.full(shape, np.nan), np.ones(shape), rtol=1e-12, atol=1e-12).simulate(TRUE)[0], 1, 2)
    return clean + (0.04 * np.abs(clean) + 0.02) * np.random.default_rng(seed).standard_normal(shape)


def make_likelihood(data=None, lanes_per_point=1, **kw):
    """lanes_per_point: 1 (a lane per experiment) or 16 (a lane group per experiment)."""
    data = simulated_data() if data is None else np.asarray(data, dtype=float)
    return _model(data, 0.04 * np.abs(data) + 0.02, lanes_per_point=lanes_per_point, **kw)


class HostTwin:
    """The likelihood as a plain Python callable: run_dream takes the host path"""
    def __init__(self, like):
        self.like = like

    def __call__(self, x):
        return self.like(x)


def main(niterations=300, nchains=64, host=False, like=None):
    from scipy.stats import uniform
    from pydream_amd.core import run_dream
    from pydream_amd.parameters import SampledParam
    like = make_likelihood() if like is None else like
    rng = np.random.default_rng(41)
    starts = [np.clip(TRUE + 0.2 * rng.uniform(-1, 1, NDIM), LOWER, LOWER + WIDTH) for _ in range(nchains)]
    sampled, log_ps = run_dream([SampledParam(uniform, loc=LOWER, scale=WIDTH)], HostTwin(like) if host else like, niterations=niterations,
                                nchains=nchains, multitry=5, start=starts, model_name="knockdown_device", verbose=False, save_history=False,
                                seed=42)
    S_, L_ = np.concatenate(sampled), np.concatenate(log_ps)
    best = S_[np.argmax(L_)]
    dense = np.linspace(0.25, 6.0, 47)
    rows, sim = posterior_predictive(sampled, like, burnin=niterations // 2, thin=max(1, niterations // 20), device=not host, t=dense)
    lo, hi = np.percentile(sim[..., 0], [5, 95], axis=0)            # [experiments, dense times]
    print("a knock-down, an inhibitor and three gels on %s (%d experiments per proposal, each with its own view of the point): %d chains x "
          "%d iterations; best log p %.3f at log10 [kf, kr, kcat, E_tot, eff, scale x 3] = %s (generated at %s); 5-95 %% band of the "
          "readout at t = %g from %d posterior rows, per experiment: %s"
          % ("the host twin" if host else "the device", len(EXPERIMENTS), nchains, niterations, L_.max(), np.round(best, 3), np.round(TRUE, 3),
             dense[-1], len(rows), ", ".join("%.2f..%.2f" % (a, b) for a, b in zip(lo[:, -1], hi[:, -1]))))
    return sampled, log_ps


if __name__ == "__main__":
    argv = [a for a in sys.argv[1:] if a != "--host"]
    main(*(int(a) for a in argv[:2]), host="--host" in sys.argv[1:])
