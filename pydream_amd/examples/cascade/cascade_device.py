"""A six-tier kinase cascade with double phosphorylation on the device, in the pattern of Huang & Ferrell's MAPK model (PNAS 93, 1996):
49 species, 72 mass-action reactions, 12 log10 rate constants -- more species than a lane group holds (32), so each proposal's ODE is
integrated by a whole 64-lane WAVE (lanes_per_point=64, csrc/dz_ode_group.h), one row of the iteration matrix per lane.

    tier i = 1..6:    X + K_i   <-> X:K_i   -> X + K_i-P          P_i + K_i-PP <-> P_i:K_i-PP -> P_i + K_i-P
                      X + K_i-P <-> X:K_i-P -> X + K_i-PP         P_i + K_i-P  <-> P_i:K_i-P  -> P_i + K_i

X, the enzyme of tier i, is the doubly phosphorylated kinase of tier i - 1 (K_i-1-PP) and for tier 1 the input enzyme E; P_i is the
tier's phosphatase.  Per tier: K, K-P, K-PP, P and the four enzyme-substrate complexes; with E that is 6 x 8 + 1 = 49 species, and each
of the four conversions is bind / unbind / catalyse: 6 x 12 = 72 reactions.  The twelve rate constants (bind, unbind, catalyse for each
of the four kinds of conversion) are shared by all tiers.  From E = 0.1, K_i = 1 (K_1 = 0.3), P_i = 0.1; K_i-PP of every tier observed
at 16 times in [1, 24] with sd 3 % + 0.01; log10 rate constants under a uniform prior one decade wide (+- 0.5) around the nominal ones.  The
data are simulated from the nominal constants.

    python -m pydream_amd.examples.cascade.cascade_device [niterations] [nchains] [--host]

--host: the same run with the likelihood's host twin as a plain Python callable (run_dream's host path), which gives the same bits.
"""
import sys

import numpy as np

from pydream_amd.likelihoods import MassActionODELogLike

TIERS = 6
LANES = 64
E = 0                                       # the input enzyme
K, KP, KPP, PASE, XK, XKP, PKPP, PKP = range(8)   # a tier's species, as offsets from tier_base(i)
N_SPECIES = 1 + 8 * TIERS
KINDS = ("K -> K-P", "K-P -> K-PP", "K-PP -> K-P", "K-P -> K")      # parameters 3 m, 3 m + 1, 3 m + 2: bind, unbind, catalyse


def tier_base(i):
    return 1 + 8 * i


def _conversion(enzyme, substrate, complex_, product, i):
    """enzyme + substrate <-> complex -> enzyme + product with parameters i, i + 1, i + 2"""
    return [({enzyme: 1, substrate: 1}, {complex_: 1}, i), ({complex_: 1}, {enzyme: 1, substrate: 1}, i + 1),
            ({complex_: 1}, {enzyme: 1, product: 1}, i + 2)]


def _reactions():
    rx = []
    for i in range(TIERS):
        b = tier_base(i)
        x = E if i == 0 else tier_base(i - 1) + KPP
        rx += _conversion(x, b + K, b + XK, b + KP, 0) + _conversion(x, b + KP, b + XKP, b + KPP, 3)
        rx += _conversion(b + PASE, b + KPP, b + PKPP, b + KP, 6) + _conversion(b + PASE, b + KP, b + PKP, b + K, 9)
    return rx


REACTIONS = _reactions()
Y0 = np.zeros(N_SPECIES)
Y0[E] = 0.1
for _i in range(TIERS):
    Y0[tier_base(_i) + K], Y0[tier_base(_i) + PASE] = (0.3 if _i == 0 else 1.0), 0.1
NOMINAL = np.log10([20.0, 3.0, 3.0, 20.0, 3.0, 3.0, 20.0, 3.0, 2.0, 20.0, 3.0, 2.0])
WIDTH = 0.5                                 # the prior box: NOMINAL +- WIDTH
TSPAN = np.linspace(1.0, 24.0, 16)
OBSERVABLES = np.zeros((TIERS, N_SPECIES))
OBSERVABLES[np.arange(TIERS), [tier_base(i) + KPP for i in range(TIERS)]] = 1.0


def simulated_data(rtol=1e-11, atol=1e-13):
    """K_i-PP at TSPAN for the nominal constants, [6, T], integrated tightly on the host."""
    tight = MassActionODELogLike(N_SPECIES, REACTIONS, Y0, TSPAN, OBSERVABLES, np.zeros((TIERS, len(TSPAN))), np.ones((TIERS, len(TSPAN))), rtol=rtol,
                                 atol=atol, max_steps=100000, lanes_per_point=LANES)
    return tight.simulate(NOMINAL)[0].T.copy()


def make_likelihood(data=None, sd=None, **kw):
    data = simulated_data() if data is None else np.asarray(data, dtype=float)
    sd = 0.03 * np.abs(data) + 0.01 if sd is None else np.broadcast_to(sd, data.shape)
    kw.setdefault("lanes_per_point", LANES)
    return MassActionODELogLike(N_SPECIES, REACTIONS, Y0, TSPAN, OBSERVABLES, data, sd, rate_scale="log10", **kw)


class HostTwin:
    """The likelihood as a plain Python callable: run_dream takes the host path"""
    def __init__(self, like):
        self.like = like

    def __call__(self, x):
        return self.like(x)


def main(niterations=100, nchains=64, host=False, like=None):
    from scipy.stats import uniform
    from pydream_amd.core import run_dream
    from pydream_amd.parameters import SampledParam
    like = make_likelihood() if like is None else like
    rng = np.random.default_rng(12)
    starts = [NOMINAL + 0.5 * WIDTH * rng.uniform(-1, 1, len(NOMINAL)) for _ in range(nchains)]
    sampled, log_ps = run_dream([SampledParam(uniform, loc=NOMINAL - WIDTH, scale=2 * WIDTH)], HostTwin(like) if host else like,
                                niterations=niterations, nchains=nchains, multitry=5, start=starts, model_name="cascade_device", verbose=False,
                                save_history=False, seed=13)
    S, L = np.concatenate(sampled), np.concatenate(log_ps)
    best = S[np.argmax(L)]
    print("cascade49 on %s (%d lanes per point): %d chains x %d iterations; best log p %.3f; |log10 k - nominal| at the best point: max %.2f"
          % ("the host twin" if host else "the device", LANES, nchains, niterations, L.max(), np.max(np.abs(best - NOMINAL))))
    return sampled, log_ps


if __name__ == "__main__":
    argv = [a for a in sys.argv[1:] if a != "--host"]
    main(*(int(a) for a in argv[:2]), host="--host" in sys.argv[1:])
