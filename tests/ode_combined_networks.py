"""Seeded networks that hold the features of MassActionODELogLike TOGETHER -- conditions, Monomials, events, equilibrate, RateLaw/Hill,
Noise and Input in one object --, for the four builds (one lane, 16, 32 and 64 lanes per point).  Shared by test_ode_combined_cpu.py and
test_ode_combined_gpu.py.  All synthetic.  The construction is chosen so that the REFERENCE alone is well behaved:

  * the base network is ode_reference.random_network over the tame kinds of ode_grammar.LARGE_STEP_KINDS (source, degradation,
    conversion, catalyst) plus a plain degradation for every species at 0.3 or more: bounded, with a resting state, so equilibrate is
    meaningful -- and no mode slower than about 1 / horizon, which the phase's steady-state test needs: it bounds the DRIFT over the
    horizon, so a state that passes it lies within drift / rate of the resting state, a tolerance only where rate * horizon is of
    order 1 (csrc/dz_ode.h; tests/test_ode_inputs_cpu.py says the same of chain17).  Every species also has a plain source (0.05 ..
    0.3): without one the catalysts of a seed can close a loop of species that only produce one another, whose extinction is a
    resting state on an invariant face that the experiment's stimulus makes unstable.  The reference itself shows it (seeds 512 and
    551 without the sources): after Radau's equilibration such species stand at 1e-22, below its own atol, and then grow fourfold
    during the experiment -- the trajectory is whatever residue the equilibration leaves, amplified, and no solver's answer is
    determined to a tolerance.  No rate law is put on these degradations and sources;
  * "ratelaw": a seeded choice of four of the other reactions gets a RateLaw -- a repression with K a parameter index, an activation with K a Monomial
    (of the first input species where there are inputs), two factors in one reaction (a float K, and the first reaction's (K, n) pair
    again: one slot read by two reactions), a Michaelis-Menten form with order={} --, n in 1..4.  Hill factors lie in [0, 1];
  * "inputs": one (S < 8) or two input species come last, each the catalyst of a production; the gains are a parameter index and a
    Monomial.  The first input's table differs between the conditions (1, 2 and 5 working knots, T0, T1, T2 below);
  * three conditions that differ in the table, the events, equilibrate (inherited True, False, a mapping) and y0 (condition 1 knocks
    out, with 0.0, the species whose y0 is a Monomial);
  * a Monomial stands as a y0 entry, a scale entry, a constraint, a rate, a Hill K and a gain;
  * "noise": the observables cycle through Noise(index, rel=index), Noise(Monomial, dist="laplace", scale="log") -- on weighted totals
    of the base species, which stay positive -- and None; a tenth of the data is NaN and the last observable is the first input species
    itself with NaN data.

Every parameter index has one job (P_* below), so that a coordinate can be made non-finite for one reader alone.  The data of a case
are the host build's own observables at the nominal point times a seeded 5 % log-normal factor: numbers, not a reference."""
import numpy as np

from pydream_amd.likelihoods import Hill, Input, MassActionODELogLike, Monomial, Noise, RateLaw

from . import ode_grammar as G
from . import ode_reference as REF

FEATURES = ("conditions", "monomials", "events", "equilibrate", "ratelaw", "noise", "inputs")
SHARED_ROW = ("ratelaw", "inputs", "noise")         # the three features whose values share a point's LDS row
P_RATES = 4                                         # coordinates 0..3: the base network's rate constants (and the rate Monomial, the constraint)
P_K, P_GAIN, P_Y0, P_SCALE, P_SIGMA, P_REL = 4, 5, 6, 7, 8, 9      # read only by: Hill Ks, gains, the y0 Monomial, the scale Monomial, Noises (two)
NDIM = 10
OMIT = object()                                     # a keyword's value for Case.like / Case.single: do not pass the keyword
T0 = 0.0
T_OUT = 0.5 * np.arange(1, 13)                      # 0.5, 1.0, ..., 6.0
# the first input's tables, one per condition: 1 (a ramp: the knot at t0 installs its slope after the phase), 2 and 5 working knots.  The last begins before t0 and ends after t[-1], has knots
# BETWEEN two outputs (0.75, 4.2), ON an output (3.0) and a falling segment that ends at 0 (at 5.0) followed by a flat one
TABLES = (((-1.0, 8.0), (0.4, 1.3)), ((0.0, 3.0, 8.0), (0.0, 1.2, 0.3)), ((-1.0, 0.75, 3.0, 4.2, 5.0, 8.0), (0.2, 0.2, 1.5, 1.5, 0.0, 0.0)))
RAMP = ((0.0, 2.2, 8.0), (0.0, 0.6, 0.6))           # the second input's table in every condition
EQUILIBRATE = (None, False, dict(max_steps=4000, horizon=3.0))      # per condition; None inherits the constructor's True
OBS_LIMIT = G.OBS_LIMIT
SPECIES_LIMIT = {1: 8, 16: 16, 32: 32, 64: 64}

# (lanes, S, seed, features left out, rate_scale, observables at the limit)
CASES = ([(1, 5, 501, (), "log10", False), (1, 8, 502, (), "linear", False), (16, 9, 511, (), "log10", False), (16, 16, 512, (), "linear", False),
          (32, 17, 521, (), "log10", False), (32, 32, 522, (), "linear", False), (64, 33, 531, (), "log10", False), (64, 64, 532, (), "linear", False)]
         + [(lanes, S, 540 + 10 * j + i, (drop,), ("log10", "linear")[(i + j) % 2], False)
            for j, (lanes, S) in enumerate([(1, 5), (16, 9), (32, 17), (64, 33)]) for i, drop in enumerate(SHARED_ROW)]
         + [(16, 9, 581, (), "log10", True), (32, 17, 582, (), "linear", True), (64, 33, 583, (), "log10", True)])
FULL = [i for i, c in enumerate(CASES) if not c[3] and not c[5]]


def _wrap(rate, factors, order=None):
    return RateLaw(rate, factors, order)


class Case:
    """One seeded network and everything the reference needs as plain records: S, reactions (RateLaw, Hill and Monomial objects, read as
    records), y0[c] (numbers and Monomials), inputs[c] (Input objects), events[c], equilibrate[c] (bool), observables, scale,
    constraints, noise, t, t0, rate_scale, nominal.  like() and single(c) build the objects under test."""

    def __init__(self, lanes, S, seed, without=(), rate_scale="log10", obs_limit=False):
        rng = np.random.default_rng(seed)
        self.lanes, self.S, self.seed, self.rate_scale, self.obs_limit = lanes, S, seed, rate_scale, obs_limit
        self.features = tuple(f for f in FEATURES if f not in without)
        self.name = "S%d@%d%s%s" % (S, lanes, "".join("-" + f for f in without), "+O" if obs_limit else "")
        n_in = 0 if "inputs" in without else 2 if S >= 8 else 1
        Sb = self.Sb = S - n_in
        rx, self.kinds = REF.random_network(rng, Sb, Sb + Sb // 2, P_RATES, G.LARGE_STEP_KINDS)
        rx += [({s: 1}, {}, float(rng.uniform(0.3, 1.0))) for s in range(Sb)]
        rx += [({}, {s: 1}, float(rng.uniform(0.05, 0.3))) for s in range(Sb)]
        rx[-2 * Sb] = (rx[-2 * Sb][0], rx[-2 * Sb][1], Monomial({0: 0.25, 1: -0.25}, -0.1))         # a Monomial as a rate: species 0's degradation, 0.3 .. 2.1 in the box
        perm = [int(s) for s in rng.permutation(Sb)]
        m, e1, e2, h = self.special = perm[:4]
        U = self.U = list(range(Sb, S))
        if U:
            rx.append(({U[0]: 1}, {U[0]: 1, perm[1]: 1}, 2))
            if n_in == 2:
                rx.append(({U[1]: 1}, {U[1]: 1, perm[2]: 1}, 0.5))
        if "ratelaw" not in without:
            # (never one of the Sb plain degradations and Sb plain sources: every species keeps an unhindered decay and supply, module's head)
            order = [int(r) for r in rng.permutation(len(rx)) if not Sb + Sb // 2 <= r < 3 * Sb + Sb // 2]
            consumed = lambda r: [s for s, n in rx[r][0].items() if n > rx[r][1].get(s, 0)]      # noqa: E731
            mm = next(r for r in order if len(consumed(r)) == 1)
            a, b, c = [r for r in order if r != mm][:3]
            nA, nB, nC = (int(n) for n in rng.integers(1, 5, 3))
            wrap = lambda r, *args: rx.__setitem__(r, (rx[r][0], rx[r][1], _wrap(rx[r][2], *args)))      # noqa: E731
            wrap(a, [Hill(h, P_K, nA, "repression")])
            wrap(b, [Hill(U[0] if U else perm[0], Monomial({P_K: 0.5}, -0.2), nB)])
            wrap(c, [Hill(perm[1], 0.7, nC), Hill(perm[2], P_K, nA, "repression")])
            wrap(mm, [Hill(consumed(mm)[0], 0.6, 1)], {})
            self.ratelaws = dict(repression=a, monomial_K=b, two_factors=c, michaelis_menten=mm)
        self.reactions = rx
        y0 = [0.0 if rng.uniform() < 0.2 else float(rng.uniform(0.2, 1.2)) for _ in range(Sb)] + [0.0] * n_in
        y0[m] = Monomial({P_Y0: 0.5}, -0.3)
        knocked = list(y0)
        knocked[m] = 0.0
        self.y0 = [y0, knocked, y0]
        gains = [P_GAIN, Monomial({P_GAIN: 0.5}, 0.1)]
        self.inputs = [[Input(U[0], *TABLES[c], gain=gains[0])] + [Input(s, *RAMP, gain=gains[1]) for s in U[1:]] for c in range(3)] if U else [[], [], []]
        # a bolus, a wash-out and a dilution: at t0, between outputs (1.25), on the output 3.0 that is also a knot of the first input's
        # tables 1 and 2, two at one time (the order matters: (y + 0.6) / 2), and on the knot 4.2 between outputs
        own = [(0.0, e1, 1.0, 0.8), (3.0, e2, 0.5, 0.0)]
        self.events = [[], own, [(0.0, e1, 1.0, 0.5), (1.25, e2, 0.0, 0.0), (3.0, e1, 1.0, 0.6), (3.0, e1, 0.5, 0.0), (4.2, e2, 1.0, 0.3)]]
        self.own_events = own
        self.equilibrate = [True, False, True]
        # the observables: single species and weighted totals of the base species; the last one the first input itself
        total = lambda w: [w] * Sb + [0.0] * n_in      # noqa: E731
        e = np.eye(S)
        if obs_limit:
            O = OBS_LIMIT[lanes]
            obs = [total(1.0 + 0.1 * q) if q % 2 else list(e[perm[(q // 2) % Sb]]) for q in range(O)]
        else:
            obs = [list(e[m]), total(1.0), list(e[e1]), list(e[e2] + e[h])] + ([[0.0] * S] if U else [])
        if U:
            obs[-1] = list(e[U[0]])
        self.observables = np.array(obs)
        O = len(obs)
        rel, log = Noise(P_SIGMA, rel=P_REL), Noise(Monomial({P_SIGMA: 0.5}, -0.3), dist="laplace", scale="log")
        if "noise" in without:
            self.noise = None
        elif obs_limit:                             # a Noise on every observable: the largest block at the end of the row
            self.noise = [log if q % 2 else Noise(0.5, rel=P_REL, dist="laplace") if q % 4 == 2 else rel for q in range(O)]
        else:
            self.noise = [(rel, log, None)[q % 3] for q in range(O)]
        self.scale = [Monomial({P_SCALE: 0.5})] + [1.0] * (O - 1)
        self.constraints = [(Monomial({0: 1, 1: -1}), 1.0, 2.0)]
        self.t, self.t0 = T_OUT, T0
        k = rng.uniform(0.8, 1.5, NDIM)
        self.nominal = k if rate_scale == "linear" else np.log10(k)
        self._data = None

    # ---- what the case provides, from the records alone
    def event_placements(self):
        """which of the placements the issue names occur: "t0", "between outputs", "output and knot", "two at one time" """
        out = set()
        for c, events in enumerate(self.events):
            knots = {tau for u in self.inputs[c] for tau in u.times}
            times = [ev[0] for ev in events]
            for tau in times:
                out |= {"t0"} if tau == self.t0 else set()
                out |= {"between outputs"} if tau > self.t0 and tau not in self.t else set()
                out |= {"output and knot"} if tau in self.t and tau in knots else set()
            out |= {"two at one time"} if len(set(times)) < len(times) else set()
        return out

    # ---- the objects under test
    def points(self, n, seed, width=0.5, outside=0.0):
        """n points of nominal +- width in the case's own coordinates.  Under "linear" the nominal constants are 0.8 .. 1.5, so the box
        0.3 .. 2.0 lies inside the +-0.5-decade box and every sampled constant stays > 0, also `outside` = 0.05 beyond it."""
        rng = np.random.default_rng(self.seed * 7 + seed)
        return self.nominal - width - outside + 2 * (width + outside) * rng.uniform(size=(n, NDIM))

    def _kw(self, kw):
        """the keywords every object of the case gets, then the caller's; a value of OMIT: that keyword is not passed at all"""
        shared = dict(rate_scale=self.rate_scale, t0=self.t0, lanes_per_point=self.lanes, ndim=NDIM, scale=self.scale, noise=self.noise)
        return {key: v for key, v in dict(shared, **kw).items() if v is not OMIT}

    def data(self):
        """[(data, sd)] per condition (the module's head)"""
        if self._data is None:
            ones = np.ones((len(self.observables), len(self.t)))
            sim = self.like(data=[(np.full_like(ones, np.nan), ones)] * 3).simulate(self.nominal)[0]     # (nothing observed: trajectories only)
            assert np.all(np.isfinite(sim)), self.name
            rng, out = np.random.default_rng(self.seed + 1), []
            for c in range(3):
                d = sim[c].T * np.exp(0.05 * rng.standard_normal(sim[c].T.shape))
                for q, z in enumerate(self.noise or [None] * len(d)):
                    assert z is None or z.scale != "log" or q == len(d) - 1 and self.U or np.all(d[q] > 0), (self.name, c, q)
                sd = 0.05 * np.abs(d) + 0.02
                d[rng.uniform(size=d.shape) < 0.1] = np.nan
                if self.U:
                    d[-1] = np.nan
                out.append((d, sd))
            self._data = out
        return self._data

    def like(self, data=None, plain_species=False, **kw):
        """the three conditions in one object.  The constructor carries condition 0's table, the events `own_events` and equilibrate=True;
        condition 0 gives events=[], condition 1 its table, its knocked-out y0 and equilibrate=False, condition 2 its table, its events
        and a mapping.  plain_species: no condition carries tables and `inputs` is the caller's (OMIT, [] or None): the input species
        are plain species that stay at 0."""
        data = self.data() if data is None else data
        conds = [dict(data=data[0][0], sd=data[0][1], events=[]),
                 dict(data=data[1][0], sd=data[1][1], y0=self.y0[1], equilibrate=False),
                 dict(data=data[2][0], sd=data[2][1], events=self.events[2], equilibrate=EQUILIBRATE[2])]
        if self.U and not plain_species:
            conds[1]["inputs"], conds[2]["inputs"] = self.inputs[1], self.inputs[2]
            kw.setdefault("inputs", self.inputs[0])
        kw.setdefault("events", self.own_events)
        kw.setdefault("equilibrate", True)
        return MassActionODELogLike(self.S, self.reactions, self.y0[0], self.t, self.observables, None, None, conditions=conds,
                                    constraints=self.constraints, **self._kw(kw))

    def single(self, c, plain_species=False, **kw):
        """condition c alone as a single experiment; the constraints on condition 0 only"""
        d, sd = self.data()[c]
        if self.U and not plain_species:
            kw.setdefault("inputs", self.inputs[c])
        kw.setdefault("events", self.events[c])
        kw.setdefault("equilibrate", (True, False, EQUILIBRATE[2])[c])
        return MassActionODELogLike(self.S, self.reactions, self.y0[c], self.t, self.observables, d, sd,
                                    constraints=self.constraints if c == 0 else None, **self._kw(kw))

    def dead_rows(self):
        """[(why, row)]: the nominal point with one coordinate spoilt for ONE reader -- a gain, a Noise, a Hill K, the y0 Monomial, the
        scale Monomial --, and under "linear" a sampled sigma, K and gain that is <= 0.  Only the readers the case has."""
        spoil = [("y0 Monomial", P_Y0, np.nan), ("scale Monomial", P_SCALE, np.inf)]
        lin = self.rate_scale == "linear"
        if "inputs" in self.features:
            spoil += [("gain", P_GAIN, np.nan)] + [("gain <= 0", P_GAIN, 0.0)] * lin
        if "noise" in self.features:
            spoil += [("Noise", P_REL, np.nan), ("Noise", P_SIGMA, -np.inf if lin else np.inf)] + [("sigma <= 0", P_SIGMA, -0.5)] * lin
        if "ratelaw" in self.features:
            spoil += [("Hill K", P_K, np.nan)] + [("K <= 0", P_K, 0.0)] * lin
        rows = []
        for why, i, v in spoil:
            x = self.nominal.copy()
            x[i] = v
            rows.append((why, x))
        return rows


_cache = {}


def case(i):
    if i not in _cache:
        _cache[i] = Case(*CASES[i])
    return _cache[i]


def combined(lanes, S, seed, features=FEATURES, rate_scale="log10", obs_limit=False):
    """(the likelihood object, the case with the records the reference needs)"""
    c = Case(lanes, S, seed, tuple(f for f in FEATURES if f not in features), rate_scale, obs_limit)
    return c.like(), c


# the GPU file's launches: a full block plus a ragged one in every build (x 3 conditions: 393 items at one lane, 201 groups of 16, 111
# groups of 32, 27 waves; 5 points at S = 64)
GPU_POINTS = {1: 131, 16: 67, 32: 37, 64: 9}
# {lanes: (max_steps, the constructor's equilibrate max_steps)} at which the small full case of the build fails a mix over
# starved_points(lanes): some points in every condition, some in a few, some in none; for some the PHASE of condition 0 fails, for others
# only an experiment.  Chosen on the host build and asserted there (test_ode_combined_cpu.py).  The phase's budget is part of it because
# max_steps alone gives no such mix: condition 0 (one knot, no events) needs the fewest steps per segment and fails only at limits at
# which condition 2 fails at every point.
STARVED = {1: (20, 140), 16: (30, 165), 32: (36, 165), 64: (20, 130)}


def starved_case(lanes):
    return case(next(i for i in FULL if CASES[i][0] == lanes))


def gpu_points(lanes, c=None):
    c = c or starved_case(lanes)
    return c.points(5 if c.S == 64 else GPU_POINTS[lanes], 5, outside=0.05)


def starved_points(lanes):
    """the launch of the starved runs: a box of +-1 decade (the small full cases are "log10"), where the points differ enough in
    stiffness for a mix of failures"""
    return starved_case(lanes).points(GPU_POINTS[lanes], 6, width=1.0)


def coverage_gaps(cases):
    """What the set lacks: per build a pair of features never together, a rate scale, a size (the smallest that holds the construction
    and the limit) for the full cases, a two-of-three case, a case at the observable limit with a Noise everywhere (group builds); over
    the whole set a dist, a noise scale, an event placement, a kind of gain, of K."""
    gaps = []
    for lanes in G.BUILDS:
        own = [c for c in cases if c.lanes == lanes]
        gaps += [(lanes, a, b) for a in FEATURES for b in FEATURES if a < b and not any(a in c.features and b in c.features for c in own)]
        gaps += [(lanes, s) for s in ("linear", "log10") if s not in {c.rate_scale for c in own}]
        full = [c for c in own if set(c.features) == set(FEATURES) and not c.obs_limit]
        gaps += [(lanes, "full at the limit")] * (not any(c.S == SPECIES_LIMIT[lanes] for c in full))
        gaps += [(lanes, "full, small")] * (not any(c.S < SPECIES_LIMIT[lanes] for c in full))
        gaps += [(lanes, "without " + f) for f in SHARED_ROW if not any(set(FEATURES) - set(c.features) == {f} for c in own)]
        if lanes != 1:
            gaps += [(lanes, "observable limit")] * (not any(c.obs_limit and len(c.observables) == OBS_LIMIT[lanes] and all(z is not None for z in c.noise) for c in own))
        gaps += [(lanes, p) for p in ("t0", "between outputs", "output and knot", "two at one time") if not any(p in c.event_placements() for c in own)]
    noises = [z for c in cases for z in c.noise or [] if z is not None]
    gaps += [d for d in ("normal", "laplace") if d not in {z.dist for z in noises}] + [s for s in ("lin", "log") if s not in {z.scale for z in noises}]
    gaps += ["a None beside Noises"] * (not any(c.noise and None in c.noise for c in cases))
    gains = {type(u.gain) for c in cases for u in c.inputs[0]}
    gaps += ["gain kinds"] * (not {int, Monomial} <= gains)
    Ks = {type(f.K) for c in cases for r in c.reactions if isinstance(r[2], RateLaw) for f in r[2].factors}
    gaps += ["K kinds"] * (not {int, float, Monomial} <= Ks)
    gaps += ["a Hill factor of an input species"] * (not any(f.species in c.U for c in cases for r in c.reactions if isinstance(r[2], RateLaw) for f in r[2].factors))
    return gaps


assert 18 <= len(CASES) <= 24 and not coverage_gaps([case(i) for i in range(len(CASES))]), coverage_gaps([case(i) for i in range(len(CASES))])
