"""Networks of more than 8 species for the lane-group ODE solver's tests: the 13-species two-substrate enzyme of
pydream_amd/examples/enzyme and chains of S species with two bimolecular cross links.  All synthetic; data from scipy's Radau at the
nominal constants, sd = 0.03 |data| + 0.01."""
import numpy as np

from pydream_amd.examples.enzyme import enzyme_device as ENZ
from pydream_amd.likelihoods import MassActionODELogLike

from . import ode_networks as NW

CHAIN_T = np.linspace(0.0, 5.0, 11)
CHAIN_NOMINAL = np.log10(np.r_[np.linspace(0.5, 2.0, 8), np.linspace(0.1, 0.4, 8), 3.0, 1.5])


def chain_network(S):
    """i <-> i + 1 (forward parameter i % 8, backward 8 + i % 8), 0 + (S-1) -> 2 x (S/2) (16), S/4 + 3S/4 -> S/3 + 1 (17): (reactions, y0,
    observables: every (S/8)-th species, 8 of them)"""
    rx = [({i: 1}, {i + 1: 1}, i % 8) for i in range(S - 1)] + [({i + 1: 1}, {i: 1}, 8 + i % 8) for i in range(S - 1)]
    rx += [({0: 1, S - 1: 1}, {S // 2: 2}, 16), ({S // 4: 1, 3 * S // 4: 1}, {S // 3: 1, 1: 1}, 17)]
    y0 = np.zeros(S)
    y0[[0, S // 4, 3 * S // 4, S - 1]] = [1.0, 0.5, 0.2, 0.3]
    return rx, y0, np.eye(S)[:: max(1, S // 8)][:8]


def dense_network(S, R, lanes, seed=1, **kw):
    """R reactions a + b -> c and c -> a + b in turn over random species triples (20 log10 parameters): as many reactions per species as
    the limits allow, for the register budget and the bit-equality test.  Data 1, sd 1 at three times in [0, 1]."""
    rng = np.random.default_rng(seed)
    rx = []
    for j in range(R):
        a, b, c = (int(s) for s in rng.choice(S, 3, replace=False))
        rx.append(({a: 1, b: 1}, {c: 1}, j % 20) if j % 2 == 0 else ({c: 1}, {a: 1, b: 1}, j % 20))
    t = np.array([0.1, 0.4, 1.0])
    return MassActionODELogLike(S, rx, np.linspace(0.2, 1.0, S), t, np.eye(S)[:4], np.ones((4, 3)), np.ones((4, 3)), lanes_per_point=lanes, **kw)


def _with_radau_data(S, rx, y0, t, obs, nominal, **kw):
    data = (NW.radau(S, rx, y0, t, nominal) @ np.asarray(obs).T).T.copy()
    return MassActionODELogLike(S, rx, y0, t, obs, data, 0.03 * np.abs(data) + 0.01, **kw)


def chain(S, lanes, **kw):
    rx, y0, obs = chain_network(S)
    return _with_radau_data(S, rx, y0, CHAIN_T, obs, CHAIN_NOMINAL, lanes_per_point=lanes, **kw)


def enzyme13(lanes=16, **kw):
    return _with_radau_data(13, ENZ.REACTIONS, ENZ.Y0, ENZ.TSPAN, ENZ.OBSERVABLES, ENZ.NOMINAL, lanes_per_point=lanes, **kw)


def enzyme_radau_loglike(args):
    """(x, data, sd) -> (the Gaussian log likelihood of a scipy Radau solution of enzyme13 at x, the sum of its terms' magnitudes);
    a module-level function of one argument, for a process pool"""
    from scipy.stats import norm
    x, data, sd = args
    y = NW.radau(13, ENZ.REACTIONS, ENZ.Y0, ENZ.TSPAN, x, rtol=1e-10, atol=1e-14)
    terms = norm(loc=data, scale=sd).logpdf((y @ ENZ.OBSERVABLES.T).T)
    return float(np.sum(terms)), float(np.sum(np.abs(terms)))


# name -> (constructor(**kw), nominal, (S, reactions, y0, t) for NW.radau)
def _chain_case(S, lanes):
    rx, y0, _ = chain_network(S)
    return (lambda **kw: chain(S, lanes, **kw)), CHAIN_NOMINAL, (S, rx, y0, CHAIN_T)


CASES = {
    "enzyme13@16": (enzyme13, ENZ.NOMINAL, (13, ENZ.REACTIONS, ENZ.Y0, ENZ.TSPAN)),
    "chain16@16": _chain_case(16, 16),
    "chain17@32": _chain_case(17, 32),
    "chain32@32": _chain_case(32, 32),
    "chain8@16": _chain_case(8, 16),
}
# a step cap per output interval that starves about half of the +-1 decade box (the one-lane algorithm's host build: the issue's table)
STARVED_MAX_STEPS = {"enzyme13@16": 75, "chain16@16": 40, "chain17@32": 40, "chain32@32": 40, "chain8@16": 40}
