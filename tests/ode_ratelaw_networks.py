"""The networks of the rate-law tests (RateLaw, Hill): named ones -- Michaelis-Menten turnover, a Goodwin oscillator with n = 8, and
the same kinetics behind inert chains for the builds of 16, 32 and 64 lanes -- and a seeded grammar: tests/ode_reference.KINDS plus
    mm                a -> b            Vmax a / (Km + a)                       RateLaw(k, [Hill(a, K)], order={})
    mm_catalysed      a -> b            kcat e a / (Km + a)                     RateLaw(k, [Hill(a, K)], order={e: 1})
    hill_activation   0 -> b            k a^n / (K^n + a^n)                     RateLaw(k, [Hill(a, K, n)])
    hill_repression   0 -> b            k K^n / (K^n + a^n)                     RateLaw(k, [Hill(a, K, n, "repression")])
    order_and_factor  a -> b            k a K^n / (K^n + a^n)                   RateLaw(k, [Hill(a, K, n, "repression")]): a in both
    two_factors       a -> b            k a^n / (K1^n + a^n) K2^m / (K2^m + a^m)   two factors on one species, order={}
with n drawn from 1..4, K a parameter index (half), a float or a Monomial of two parameters.  S is the smallest that exercises each
shape: 2..8 for one lane, 9 and 13 for 16 lanes, 17 and 20 for 32, 33 for 64.  Shared by the CPU and the GPU test file."""
import numpy as np

from pydream_amd.likelihoods import Hill, MassActionODELogLike, Monomial, RateLaw

from . import ode_grammar as G
from . import ode_reference as REF

NEW_KINDS = ("mm", "mm_catalysed", "hill_activation", "hill_repression", "order_and_factor", "two_factors")
KINDS = REF.KINDS + NEW_KINDS
T_OUT = G.T_OUT

# (lanes_per_point, S, R, seed, rate_scale): one lane on both sides of the 16 reactions where the generated source changes form
CASES = [(1, 2, 4, 511, "log10"), (1, 4, 9, 502, "linear"), (1, 6, 16, 503, "log10"), (1, 8, 20, 504, "linear"), (1, 5, 24, 505, "log10"),
         (16, 9, 14, 601, "linear"), (16, 13, 20, 602, "log10"), (16, 9, 22, 603, "log10"),
         (32, 17, 20, 701, "log10"), (32, 20, 26, 702, "linear"), (32, 17, 30, 703, "linear"),
         (64, 33, 36, 801, "linear"), (64, 33, 44, 802, "log10"), (64, 33, 40, 803, "log10")]


def _draw_K(rng, P):
    u = rng.uniform()
    if u < 0.5:
        return int(rng.integers(P))
    if u < 0.75 or P < 2:
        return float(rng.uniform(0.3, 1.5))
    i, j = (int(v) for v in rng.choice(P, 2, replace=False))
    return Monomial({i: 1, j: -1}, float(np.log10(rng.uniform(0.5, 1.5))))


def random_network(rng, S, R, P):
    """(reactions, kinds): half of the reactions from the new kinds, half from the mass-action grammar"""
    reactions, drawn = [], []
    for _ in range(R):
        if rng.uniform() < 0.5:
            rx, kind = REF.random_network(rng, S, 1, P)
            reactions += rx
            drawn += kind
            continue
        kind = NEW_KINDS[int(rng.integers(len(NEW_KINDS)))]
        a, b, e = (int(s) for s in (rng.choice(S, 3, replace=False) if S >= 3 else rng.integers(0, S, 3)))
        if S == 2:
            b = 1 - a
        rate = int(rng.integers(P)) if rng.uniform() < 0.7 else float(rng.uniform(0.2, 1.5))
        n, m = int(rng.integers(1, 5)), int(rng.integers(1, 5))
        K, K2 = _draw_K(rng, P), _draw_K(rng, P)
        reactions.append({"mm": ({a: 1}, {b: 1}, RateLaw(rate, [Hill(a, K)], order={})),
                          "mm_catalysed": ({a: 1}, {b: 1}, RateLaw(rate, [Hill(a, K)], order={e: 1})),
                          "hill_activation": ({}, {b: 1}, RateLaw(rate, [Hill(a, K, n)])),
                          "hill_repression": ({}, {b: 1}, RateLaw(rate, [Hill(a, K, n, "repression")])),
                          "order_and_factor": ({a: 1}, {b: 1}, RateLaw(rate, [Hill(a, K, n, "repression")])),
                          "two_factors": ({a: 1}, {b: 1}, RateLaw(rate, [Hill(a, K, n), Hill(a, K2, m, "repression")], order={}))}[kind])
        drawn.append(kind)
    return reactions, drawn


class Network(G.Network):
    """One seeded network of the rate-law grammar; tests/ode_grammar.Network's points, nominal, like and states"""

    def __init__(self, lanes, S, R, seed, rate_scale):
        rng = np.random.default_rng(seed)
        self.lanes, self.S, self.R, self.seed, self.rate_scale = lanes, S, R, seed, rate_scale
        self.P = max(2, min(6, R // 2))
        self.reactions, self.kinds = random_network(rng, S, R, self.P)
        self.y0 = np.where(rng.uniform(size=S) < 0.2, 0.0, rng.uniform(0.2, 1.2, S))
        self.y0[0] = max(self.y0[0], 0.5)
        self.k_nominal = rng.uniform(0.3, 1.5, self.P)
        self.name = "rl-S%dR%d@%d" % (S, R, lanes)


def network(i, bump=0):
    lanes, S, R, seed, scale = CASES[i]
    return Network(lanes, S, R, seed + 1000 * bump, scale)


def hill_factors(net):
    return [f for _, _, rate in net.reactions if isinstance(rate, RateLaw) for f in rate.factors]


def coverage_gaps(networks):
    """What the set lacks: three networks per build, every new kind, both one-lane forms, K as an index, a float and a Monomial, both
    rate scales."""
    gaps = [(lanes, "three networks") for lanes in G.BUILDS if sum(n.lanes == lanes for n in networks) < 3]
    gaps += [k for k in NEW_KINDS if not any(k in n.kinds for n in networks)]
    gaps += [form for form, has in (("short form", any(n.lanes == 1 and n.R <= 16 for n in networks)), ("long form", any(n.lanes == 1 and n.R > 16 for n in networks))) if not has]
    gaps += [t.__name__ for t in (int, float, Monomial) if not any(isinstance(f.K, t) for n in networks for f in hill_factors(n))]
    gaps += [s for s in ("linear", "log10") if s not in {n.rate_scale for n in networks}]
    return gaps


# ---------------------------------------------------------------------------------------------------- named networks
# mm2: S -> P at Vmax S / (Km + S) (x[0], x[1]), 0 -> S (0.3), P -> 0 (0.4): the smallest, two species
MM2 = dict(S=2, reactions=[({0: 1}, {1: 1}, RateLaw(0, [Hill(0, 1)], order={})), ({}, {0: 1}, 0.3), ({1: 1}, {}, 0.4)], y0=[2.0, 0.0],
           nominal=np.log10([1.5, 0.6]), t=np.linspace(0.5, 6.0, 12), obs=np.eye(2), lanes=1)
# mm_enzyme: E + S, kcat E S / (Km + S) with the enzyme a species of its own (order={E: 1}) that is made and degraded
MM_ENZYME = dict(S=3, reactions=[({1: 1}, {2: 1}, RateLaw(0, [Hill(1, 1)], order={0: 1})), ({}, {0: 1}, 0.2), ({0: 1}, {}, 2), ({2: 1}, {}, 0.3)],
                 y0=[0.5, 3.0, 0.0], nominal=np.log10([2.0, 0.8, 0.4]), t=np.linspace(0.5, 6.0, 12), obs=np.eye(3)[1:], lanes=1)
# goodwin8: X -| ... a Goodwin oscillator's loop with n = 8 (the largest exponent), K = x[1]: 0 -> X repressed by Z, X -> X + Y, Y -> Y + Z
GOODWIN8 = dict(S=3, reactions=[({}, {0: 1}, RateLaw(0, [Hill(2, 1, 8, "repression")])), ({0: 1}, {}, 0.5), ({0: 1}, {0: 1, 1: 1}, 2), ({1: 1}, {}, 0.4),
                                ({1: 1}, {1: 1, 2: 1}, 1.0), ({2: 1}, {}, 0.6)],
                y0=[0.1, 0.2, 0.5], nominal=np.log10([2.0, 1.0, 0.8]), t=np.linspace(0.5, 8.0, 16), obs=np.eye(3), lanes=1)
# activated: 0 -> B at k A^2 / (K^2 + A^2), K a Monomial x[1] - x[2] (a ratio of two sampled constants), A decaying: composition with a Monomial K
ACTIVATED = dict(S=2, reactions=[({}, {1: 1}, RateLaw(0, [Hill(0, Monomial({1: 1, 2: -1}), 2)])), ({0: 1}, {}, 0.3), ({1: 1}, {}, 0.5)], y0=[2.0, 0.0],
                 nominal=np.log10([1.2, 1.6, 2.0]), t=np.linspace(0.5, 6.0, 12), obs=np.eye(2), lanes=1)
NAMED = dict(mm2=MM2, mm_enzyme=MM_ENZYME, goodwin8=GOODWIN8, activated=ACTIVATED)


def padded(spec, S, lanes):
    """The named network in front of an inert conversion chain S0 -> S0 + 1 -> ... -> S - 1 (0.5 each, fed by the last own species at 0.1):
    the same kinetics for the builds of 16, 32 and 64 lanes"""
    S0 = spec["S"]
    chain = [({S0 - 1: 1}, {S0: 1}, 0.1)] + [({s: 1}, {s + 1: 1}, 0.5) for s in range(S0, S - 1)]
    obs = np.zeros((len(spec["obs"]) + 1, S))
    obs[:-1, :S0] = spec["obs"]
    obs[-1, S - 1] = 1.0
    return dict(spec, S=S, reactions=list(spec["reactions"]) + chain, y0=list(spec["y0"]) + [0.0] * (S - S0), obs=obs, lanes=lanes)


def build(spec, rate_scale="log10", data=None, sd=None, y0="own", **kw):
    """The likelihood of a named network; data None: ones (the tests that compare states or bits do not need a fit)"""
    obs, t = np.atleast_2d(spec["obs"]), spec["t"]
    kw.setdefault("lanes_per_point", spec["lanes"])
    return MassActionODELogLike(spec["S"], spec["reactions"], spec["y0"] if isinstance(y0, str) else y0, t, obs,
                                np.ones((len(obs), len(t))) if data is None else data, 1.0 if sd is None else sd, rate_scale=rate_scale, **kw)
