"""A two-substrate enzyme with an inhibitor on the device: 13 species, 20 mass-action reactions, 20 log10 rate constants -- more species
than one lane's registers hold (MassActionODELogLike's default shape stops at 8), so each proposal's ODE is integrated by a GROUP of 16
lanes (lanes_per_point=16, csrc/dz_ode_group.h), one row of the iteration matrix per lane.

    E + A <-> EA -> E + P        EA + A <-> EAA -> EA + P       EB + A <-> EBA -> EB + P
    E + B <-> EB -> E + Q        EA + B <-> EAB -> EA + Q       EB + B <-> EBB -> EB + Q        E + I <-> EI

The enzyme E turns the substrates A and B into P and Q, binds a second substrate molecule at a slower site, and is held back by the
inhibitor I.  From E = 0.05, A = 4, B = 2, I = 0.5; P, Q, A and B observed at 20 times in [0.5, 10] with sd 3 % + 0.01; log10 rate
constants under a uniform prior two decades wide around the nominal ones.  The data are simulated from the nominal constants.

    python -m pydream_amd.examples.enzyme.enzyme_device [niterations] [nchains]
"""
import sys

import numpy as np

from pydream_amd.likelihoods import MassActionODELogLike

SPECIES = ("E", "A", "B", "P", "Q", "EA", "EB", "EAA", "EAB", "EBA", "EBB", "I", "EI")
E, A, B, P, Q, EA, EB, EAA, EAB, EBA, EBB, I, EI = range(13)
LANES = 16


def _binding(a, b, c, i):
    """a + b <-> c with parameters i (forward) and i + 1 (backward)"""
    return [({a: 1, b: 1}, {c: 1}, i), ({c: 1}, {a: 1, b: 1}, i + 1)]


def _turnover(enzyme, substrate, complex_, product, i):
    """enzyme + substrate <-> complex -> enzyme + product with parameters i, i + 1, i + 2"""
    return _binding(enzyme, substrate, complex_, i) + [({complex_: 1}, {enzyme: 1, product: 1}, i + 2)]


REACTIONS = (_turnover(E, A, EA, P, 0) + _turnover(E, B, EB, Q, 3) + _turnover(EA, A, EAA, P, 6) + _turnover(EA, B, EAB, Q, 9)
             + _turnover(EB, A, EBA, P, 12) + _turnover(EB, B, EBB, Q, 15) + _binding(E, I, EI, 18))
Y0 = np.zeros(13)
Y0[[E, A, B, I]] = [0.05, 4.0, 2.0, 0.5]
NOMINAL = np.log10([100, 80, 1.3, 100, 70, 1.2, 10, 3, 2.3, 10, 8, 0.2, 10, 5, 1.0, 10, 40, 0.5, 50, 5.0])
TSPAN = np.linspace(0.5, 10.0, 20)
OBSERVABLES = np.zeros((4, 13))
OBSERVABLES[[0, 1, 2, 3], [P, Q, A, B]] = 1.0


def simulated_data(rtol=1e-12, atol=1e-14):
    """P, Q, A, B at TSPAN for the nominal constants, [4, T], integrated tightly on the host."""
    tight = MassActionODELogLike(13, REACTIONS, Y0, TSPAN, OBSERVABLES, np.zeros((4, len(TSPAN))), np.ones((4, len(TSPAN))), rtol=rtol, atol=atol,
                                 max_steps=100000, lanes_per_point=LANES)
    return tight.simulate(NOMINAL)[0].T.copy()


def make_likelihood(data=None, sd=None, **kw):
    data = simulated_data() if data is None else np.asarray(data, dtype=float)
    sd = 0.03 * np.abs(data) + 0.01 if sd is None else np.broadcast_to(sd, data.shape)
    kw.setdefault("lanes_per_point", LANES)
    return MassActionODELogLike(13, REACTIONS, Y0, TSPAN, OBSERVABLES, data, sd, rate_scale="log10", **kw)


def main(niterations=100, nchains=64):
    from scipy.stats import uniform
    from pydream_amd.core import run_dream
    from pydream_amd.parameters import SampledParam
    like = make_likelihood()
    lower = NOMINAL - 1
    sampled, log_ps = run_dream([SampledParam(uniform, loc=lower, scale=2)], like, niterations=niterations, nchains=nchains, multitry=5,
                                model_name="enzyme_device", verbose=False, save_history=False)
    S, L = np.concatenate(sampled), np.concatenate(log_ps)
    best = S[np.argmax(L)]
    print("enzyme13 on the device (%d lanes per point): %d chains x %d iterations; best log p %.3f; |log10 k - nominal| at the best point: max %.2f"
          % (LANES, nchains, niterations, L.max(), np.max(np.abs(best - NOMINAL))))
    return sampled, log_ps


if __name__ == "__main__":
    main(*(int(a) for a in sys.argv[1:3]))
