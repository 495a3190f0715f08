"""Networks of 33..64 species for the wave-per-point ODE solver's tests (MassActionODELogLike(lanes_per_point=64)): ode_wide_networks'
chains and dense networks at 64 lanes, the 49-species kinase cascade of pydream_amd/examples/cascade, and chain40 with conditions,
events and Monomials.  All synthetic; the chains' data come from scipy's Radau at the nominal constants (ode_wide_networks.chain), the
cascade's from the example's own tight host integration."""
import functools

import numpy as np

from pydream_amd.examples.cascade import cascade_device as CAS
from pydream_amd.likelihoods import MassActionODELogLike, Monomial

from . import ode_wide_networks as W

LANES = 64
STARVED_MAX_STEPS = 40      # per output interval: part of the +-1 decade box (chains) and of the cascade's +-0.5 box fails, part finishes
CHAIN_NOMINAL = W.CHAIN_NOMINAL
CASCADE_WIDTH = CAS.WIDTH
N_ITER, N_CHAINS = 6, 8     # the reduced size at which the cascade example's main() runs on the device and through the host twin


@functools.lru_cache(maxsize=None)
def _cascade_data():
    data = CAS.simulated_data()
    data.setflags(write=False)
    return data


def cascade(**kw):
    return CAS.make_likelihood(data=_cascade_data(), **kw)


@functools.lru_cache(maxsize=None)
def _chain_data(S):
    like = W.chain(S, LANES)
    like.data.setflags(write=False); like.sd.setflags(write=False)
    return like.data, like.sd


def chain(S, **kw):
    """ode_wide_networks.chain(S, 64), its Radau data computed once per S"""
    rx, y0, obs = W.chain_network(S)
    data, sd = _chain_data(S)
    return MassActionODELogLike(S, rx, y0, W.CHAIN_T, obs, data, sd, lanes_per_point=LANES, **kw)


def _chain_case(S):
    rx, y0, _ = W.chain_network(S)
    return (lambda **kw: chain(S, **kw)), CHAIN_NOMINAL, 1.0, (S, rx, y0, W.CHAIN_T)


# name -> (constructor(**kw), nominal, half width of the prior box, (S, reactions, y0, t) for ode_networks.radau)
CASES = {
    "chain33": _chain_case(33),
    "chain48": _chain_case(48),
    "chain64": _chain_case(64),
    "cascade49": (cascade, CAS.NOMINAL, CASCADE_WIDTH, (CAS.N_SPECIES, CAS.REACTIONS, CAS.Y0, CAS.TSPAN)),
}

CONDITION_SCALES = (0.5, 1.0, 2.0)
EVENTS = ((1.3, 0, 0.5, 0.0), (3.0, 10, 1.0, 0.25))        # between two output times; on one (t = 3.0)


def chain_conditions(S, C=3, events=False, monomials=False, **kw):
    """(the chain of S species under C conditions -- the start amounts scaled by CONDITION_SCALES --, single(c): the object of condition c
    alone).  events: condition 1 has the two EVENTS; monomials: a Monomial scale on observable 0 and one constraint (with condition 0)."""
    rx, y0, obs = W.chain_network(S)
    data, sd = _chain_data(S)
    shared = dict(lanes_per_point=LANES, **kw)
    if monomials:
        shared["scale"] = [Monomial({16: 1}, -np.log10(3.0))] + [1.0] * (len(obs) - 1)
    cons = [(Monomial({0: 1, 8: -1}), 5.0, 2.0)] if monomials else None
    conds = [dict(y0=s * y0, **(dict(events=list(EVENTS)) if events and c == 1 else {})) for c, s in enumerate(CONDITION_SCALES[:C])]
    multi = MassActionODELogLike(S, rx, None, W.CHAIN_T, obs, data, sd, conditions=conds, constraints=cons, **shared)

    def single(c):
        return MassActionODELogLike(S, rx, conds[c]["y0"], W.CHAIN_T, obs, data, sd, events=conds[c].get("events"),
                                    constraints=cons if c == 0 else None, **shared)
    return multi, single


def chain_with_events(S, n_events=3, **kw):
    rx, y0, obs = W.chain_network(S)
    data, sd = _chain_data(S)
    events = [(0.7, 0, 0.5, 0.0), (2.0, S - 1, 1.0, 0.3), (3.6, S // 2, 0.0, 0.1)][:n_events]
    return MassActionODELogLike(S, rx, y0, W.CHAIN_T, obs, data, sd, lanes_per_point=LANES, events=events, **kw)


def chain_with_monomials(S, **kw):
    """a Monomial rate (the backward constant of the first link as KD x forward), a Monomial start amount, a scale and a constraint"""
    rx, y0, obs = W.chain_network(S)
    data, sd = _chain_data(S)
    rx = list(rx)
    rx[S - 1] = (rx[S - 1][0], rx[S - 1][1], Monomial({0: 1, 8: 1}))
    start = list(y0)
    start[0] = Monomial({17: 1}, np.log10(1.0 / 1.5))
    return MassActionODELogLike(S, rx, start, W.CHAIN_T, obs, data, sd, lanes_per_point=LANES, scale=[Monomial({16: 1}, -np.log10(3.0))] + [1.0] * (len(obs) - 1),
                                constraints=[(Monomial({0: 1, 8: -1}), 5.0, 2.0)], **kw)
