"""The networks, noise models and point sets of the sampled-noise tests (likelihoods.Noise): seeded networks of the grammar
(tests/ode_grammar) for every build -- three species and eight species (more than 16 reactions: the long form) on one lane, 11 species
on 16 lanes, 17 on 32 and 33 on a wave --, each read through three observables that stay positive (species 0, the total of all species,
the total without species 0), and the coordinates of the noise models behind the network's own P parameters: x[P] and x[P + 1].
Shared by the CPU and the GPU test file."""
import numpy as np

from pydream_amd.likelihoods import Monomial, Noise

from . import ode_grammar as G
from .ode_networks import box_points

# the grammar's cases (tests/ode_grammar.CASES): name -> index
NETWORKS = dict(one3=2, long8=7, group16=12, group32=18, wave64=29)
SIGMA_NOMINAL = 0.3                         # sigma and rel at the centre of a box, on the natural scale
REL_NOMINAL = 0.2
WIDTH = 0.5                                 # the boxes' half width, the grammar tests' own


def network(name):
    return G.network(NETWORKS[name])


def observables(net):
    obs = np.ones((3, net.S))
    obs[0, 1:] = 0.0
    obs[2, 0] = 0.0
    return obs if net.S > 1 else obs[:2]


def cases(P):
    """name -> the three observables' noise models, sigma and rel as a parameter index, a float and a Monomial; both dists, both
    scales; observables with and without a Noise in one object.  P, P + 1: the two coordinates behind the network's own."""
    return dict(
        index_rel=[Noise(P, rel=Monomial({P + 1: 1}, -0.3)), None, Noise(0.4, dist="laplace")],
        monomial_log=[Noise(Monomial({P: 1, P + 1: -1}, -0.5), rel=0.1, dist="laplace"), Noise(P, scale="log"), None],
        all_three=[Noise(0.3, dist="laplace", scale="log"), Noise(P + 1, scale="log"), Noise(P, rel=P + 1, dist="laplace")])


def nominal(net):
    """The centre of the box: the network's own, then sigma and rel in the network's rate scale"""
    extra = np.array([SIGMA_NOMINAL, REL_NOMINAL])
    return np.r_[net.nominal(), extra if net.rate_scale == "linear" else np.log10(extra)]


def data_and_weights(net, seed, T=len(G.T_OUT)):
    """(data, sd): positive data around 1 with two entries not observed, weights between 0.5 and 2"""
    rng = np.random.default_rng(seed)
    O = len(observables(net))
    data = rng.uniform(0.5, 1.5, (O, T))
    data[0, 1] = data[O - 1, T - 1] = np.nan
    return data, rng.uniform(0.5, 2.0, (O, T))


def like(net, noise, seed=1, **kw):
    data, sd = data_and_weights(net, seed)
    kw.setdefault("data", data)
    kw.setdefault("sd", sd)
    return net.like(observables=observables(net), ndim=net.P + 2, noise=noise, **kw)


def dead_rows(net):
    """rows of (coordinate offset from P, value): noise coordinates at which a point may not be live -- not finite, and under "linear"
    0.0, -0.0 or negative (a bare sigma must be > 0, a bare rel >= 0; a Monomial reads any finite number)"""
    rows = [(0, np.nan), (0, np.inf), (0, -np.inf), (1, np.nan)]
    if net.rate_scale == "linear":
        rows += [(0, 0.0), (0, -0.0), (0, -0.25), (1, -0.125)]
    return rows


def points(net, n, seed, noise):
    """(X, dead): n points of the box nominal +- WIDTH with rows just outside it (box_points' `outside`), the first rows overwritten by
    dead_rows; dead: the rows whose noise coordinates are not live under the contract (csrc/dz_ode.h, NOISE), worked out here from the
    noise models themselves: a coordinate that one of them reads is not finite, or under "linear" a bare sigma is <= 0 or a bare rel
    is < 0.  (Under "log10" 10**x is > 0 for every finite x.)"""
    X = box_points(nominal(net), n, seed, width=WIDTH, outside=0.05)
    for i, (c, v) in enumerate(dead_rows(net)):
        X[i, net.P + c] = v
    dead = np.zeros(n, dtype=bool)
    for z in noise:
        for c, least in ((z and z.sigma, "> 0"), (z and z.rel, ">= 0")):
            if isinstance(c, Monomial):
                dead |= ~np.all(np.isfinite(X[:, list(c.indices)]), axis=1)
            elif isinstance(c, (int, np.integer)):
                dead |= ~np.isfinite(X[:, c])
                if net.rate_scale == "linear":
                    dead |= X[:, c] <= 0 if least == "> 0" else X[:, c] < 0
    return X, dead
