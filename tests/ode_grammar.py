"""The seeded networks of the ODE grammar tests (tests/ode_reference.random_network) for the four builds of MassActionODELogLike (one
lane, 16, 32 and 64 lanes per point), a second family of tame networks for steps so large that the LU's pivots leave the diagonal, and
a hand-built network whose iteration matrix has tied pivot candidates.  Shared by the CPU and the GPU test file."""
import numpy as np

from pydream_amd.likelihoods import MassActionODELogLike

from . import ode_reference as REF

# (lanes_per_point, S, R, seed, rate_scale): the one-lane build S = 1..8 (R on both sides of the 16 reactions where its generated source
# changes form), 16 lanes S = 1..16, 32 lanes S = 1 and 17..32, 64 lanes S = 33..64
CASES = [(1, 1, 3, 101, "linear"), (1, 2, 5, 102, "log10"), (1, 3, 8, 103, "linear"), (1, 4, 12, 104, "log10"),
         (1, 5, 16, 105, "linear"), (1, 6, 24, 106, "log10"), (1, 7, 31, 107, "linear"), (1, 8, 40, 108, "log10"),
         (16, 1, 2, 211, "log10"), (16, 4, 9, 202, "linear"), (16, 6, 14, 203, "log10"), (16, 9, 18, 204, "linear"),
         (16, 11, 22, 205, "log10"), (16, 13, 30, 206, "linear"), (16, 16, 40, 207, "log10"), (16, 16, 25, 208, "linear"),
         (32, 1, 1, 311, "linear"), (32, 5, 10, 302, "log10"), (32, 17, 20, 303, "linear"), (32, 20, 26, 304, "log10"),
         (32, 23, 30, 305, "linear"), (32, 26, 34, 306, "log10"), (32, 29, 40, 307, "linear"), (32, 32, 36, 308, "log10"),
         (1, 8, 5, 109, "linear"), (1, 6, 3, 110, "log10"), (16, 16, 9, 209, "linear"), (16, 12, 7, 210, "log10"),      # fewer reactions than
         (32, 32, 20, 309, "linear"),                                                                                    # species: invariants
         # the 64-lane wave per point, S = 33..64 (appended: the indices above are used elsewhere); the last two have fewer reactions than species
         (64, 33, 70, 401, "linear"), (64, 40, 80, 402, "log10"), (64, 48, 90, 403, "linear"), (64, 56, 100, 404, "log10"),
         (64, 63, 110, 405, "linear"), (64, 64, 120, 406, "log10"), (64, 64, 40, 407, "linear"), (64, 36, 20, 408, "log10")]
BUILDS = (1, 16, 32, 64)
T_OUT = np.array([0.25, 0.5, 1.0, 2.0])
OBS_LIMIT = {1: 8, 16: 16, 32: 16, 64: 16}


class Network:
    """One seeded network: reactions, kinds, y0 (a fifth of the species start empty), P parameters and their nominal values in the
    case's rate scale (rate constants 0.3 .. 1.5)."""

    def __init__(self, lanes, S, R, seed, rate_scale, kinds=REF.KINDS):
        rng = np.random.default_rng(seed)
        self.lanes, self.S, self.R, self.seed, self.rate_scale = lanes, S, R, seed, rate_scale
        self.P = max(1, min(6, R // 2))
        self.reactions, self.kinds = REF.random_network(rng, S, R, self.P, kinds)
        self.y0 = np.where(rng.uniform(size=S) < 0.2, 0.0, rng.uniform(0.2, 1.2, S))
        self.y0[0] = max(self.y0[0], 0.5)
        self.k_nominal = rng.uniform(0.3, 1.5, self.P)
        self.name = "S%dR%d@%d" % (S, R, lanes)

    def nominal(self, rate_scale=None):
        return self.k_nominal if (rate_scale or self.rate_scale) == "linear" else np.log10(self.k_nominal)

    def points(self, n, rate_scale=None, seed=0):
        """n parameter points within half a decade of the nominal rate constants, in the rate scale's coordinates"""
        logk = np.log10(self.k_nominal) + np.random.default_rng(self.seed * 7 + seed).uniform(-0.5, 0.5, (n, self.P))
        return 10.0 ** logk if (rate_scale or self.rate_scale) == "linear" else logk

    def like(self, observables=None, t=T_OUT, rate_scale=None, lanes=None, reactions=None, y0=None, data=None, sd=1.0, **kw):
        obs = np.eye(self.S)[:OBS_LIMIT[lanes or self.lanes]] if observables is None else np.atleast_2d(observables)
        data = np.ones((len(obs), len(t))) if data is None else data
        kw.setdefault("ndim", self.P)
        return MassActionODELogLike(self.S, self.reactions if reactions is None else reactions, self.y0 if y0 is None else y0, t, obs, data, sd,
                                    rate_scale=rate_scale or self.rate_scale, lanes_per_point=lanes or self.lanes, **kw)

    def states(self, X, t=T_OUT, **kw):
        """simulate() of every species, [n, T, S]: identity observables in blocks of as many rows as the build accepts"""
        lim = OBS_LIMIT[kw.get("lanes") or self.lanes]
        return np.concatenate([self.like(observables=np.eye(self.S)[i:i + lim], t=t, **kw).simulate(X) for i in range(0, self.S, lim)], axis=2)


def network(i, bump=0):
    lanes, S, R, seed, scale = CASES[i]
    return Network(lanes, S, R, seed + 1000 * bump, scale)


def coverage_gaps(networks):
    """What the set lacks, per build: a reaction kind (counted where S >= 4, so that no kind degenerates), a fixed rate, a rate scale."""
    gaps = []
    for lanes in BUILDS:
        nets = [n for n in networks if n.lanes == lanes]
        kinds = {k for n in nets if n.S >= 4 for k in n.kinds}
        gaps += [(lanes, k) for k in REF.KINDS if k not in kinds]
        if not any(isinstance(r[2], float) for n in nets for r in n.reactions):
            gaps.append((lanes, "fixed rate"))
        gaps += [(lanes, s) for s in ("linear", "log10") if s not in {n.rate_scale for n in nets}]
    return gaps


assert len(CASES) >= 32 and sum(c[0] == 64 for c in CASES) >= 8 and not coverage_gaps([network(i) for i in range(len(CASES))]), coverage_gaps([network(i) for i in range(len(CASES))])

# A + B -> 2A + C + D (k1 = 6), A -> B (k2 = 6), C -> 0, D -> 0 (2.0 each); A + B is conserved, so the system is bounded, and it starts
# near its steady state B = k2 / k1 = 1, A = 0.5, C = D = 1.5 (eigenvalue -k1 A = -3).  Column A of W = I / (h gamma) - J holds
# 4/h - k1 B + k2, k1 B - k2, -k1 B, -k1 B: near B = 1 and for h > 2/3 the rows of C and D tie for the pivot, ahead of the diagonal.
TIED_REACTIONS = [({0: 1, 1: 1}, {0: 2, 2: 1, 3: 1}, 0), ({0: 1}, {1: 1}, 1), ({2: 1}, {}, 2.0), ({3: 1}, {}, 2.0)]
TIED_Y0 = np.array([0.45, 1.05, 1.2, 1.2])
TIED_X = np.array([6.0, 6.0])                                                 # rate_scale "linear"
TIED_T = np.array([5.0, 50.0, 500.0])                                        # (long intervals: the step grows to the interval's length)


# For the wave per point (33..64 species) the same four species sit at indices 32..35, behind an inert conversion chain 0 -> 1 -> ... -> 31
# (0.5 each) that starts empty and shares nothing with them: the chain's columns keep their diagonal pivots (4/h + 0.5 against 0.5) and
# leave the last four rows untouched, so column 32 is column A above and its tie is broken among lanes 34 and 35.
TIED_PAD = 32


def tied_network(lanes):
    """(S, reactions, y0, the indices of A, B, C, D) of the tied network as the build of `lanes` lanes gets it"""
    if lanes != 64:
        return 4, TIED_REACTIONS, TIED_Y0, np.arange(4)
    moved = [({s + TIED_PAD: c for s, c in reac.items()}, {s + TIED_PAD: c for s, c in prod.items()}, rate) for reac, prod, rate in TIED_REACTIONS]
    chain = [({s: 1}, {s + 1: 1}, 0.5) for s in range(TIED_PAD - 1)]
    return TIED_PAD + 4, moved + chain, np.concatenate([np.zeros(TIED_PAD), TIED_Y0]), np.arange(TIED_PAD, TIED_PAD + 4)


def tied(lanes, t=TIED_T, **kw):
    """The likelihood of A, B, C, D against ones: the same function of x in every build"""
    S, reactions, y0, abcd = tied_network(lanes)
    return MassActionODELogLike(S, reactions, y0, t, np.eye(S)[abcd], np.ones((4, len(t))), 1.0, rate_scale="linear", lanes_per_point=lanes, **kw)


# ---------------------------------------------------------------------------------------------------- large steps
# Networks of sources, degradations, conversions and catalysts only, integrated with steps of h = t1 / n = 4 .. 16: such a network stays
# tame under Rodas4 steps far beyond its time scales (a catalyst's own row of f is identically 0, so along the solution the system is
# close to linear), and 1 / (h gamma) = 1 .. 1/4 no longer dominates the Jacobian's entries of order 1, so the LU's pivots leave the
# diagonal.  With the full grammar (autocatalysis, third order) steps of this size go negative and blow up.
# (lanes_per_point, S, R, seed, t1, n); rate_scale "linear".  What the family has to provide is asserted on the reference's own
# matrices in tests/test_ode_grammar_cpu.py -- a bounded solution, W of condition <= 1e3, pivots off the diagonal in every quarter of
# the columns and in both halves of a wave --; the seeds were searched with the float64 restatement alone so that it holds.
LARGE_STEP_KINDS = ("source", "degradation", "conversion", "catalyst")
LARGE_STEP_CASES = [(1, 6, 12, 89, 64.0, 4), (1, 8, 16, 48, 32.0, 4), (16, 16, 32, 48, 16.0, 4), (16, 12, 24, 20, 16.0, 4),
                    (32, 32, 64, 12, 16.0, 4), (32, 24, 40, 8, 16.0, 4), (64, 64, 80, 17, 16.0, 4), (64, 40, 60, 3, 32.0, 4)]
assert all(sum(c[0] == lanes for c in LARGE_STEP_CASES) >= 2 for lanes in BUILDS) and any(c[0] == 64 and c[1] >= 60 for c in LARGE_STEP_CASES)
assert all(c[1] <= 8 for c in LARGE_STEP_CASES if c[0] == 1) and all(4 <= c[4] / c[5] <= 16 for c in LARGE_STEP_CASES)


def large_step_network(j):
    lanes, S, R, seed, _, _ = LARGE_STEP_CASES[j]
    net = Network(lanes, S, R, seed, "linear", kinds=LARGE_STEP_KINDS)
    net.name = "large-" + net.name
    return net
