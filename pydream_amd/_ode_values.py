"""The limits of pydream_amd.likelihoods.MassActionODELogLike, the predicates its checks are made of, and the immutable values a network
is written with: Monomial, Hill, RateLaw, Noise, Input, Normalize."""
import numpy as np

ODE_LIMITS = dict(species=8, reactions=64, observables=8, times=4096)
ODE_GROUP_LIMITS = dict(species=32, reactions=128, observables=16, times=4096, lanes=(16, 32), conditions=64)      # lanes_per_point=16 | 32: species <= lanes
ODE_WAVE_LIMITS = dict(species=64, reactions=256, observables=16, times=4096, lanes=(64,), conditions=64)            # lanes_per_point=64: 33..64 species
ODE_MAX_CONSTRAINTS = 16    # constraints=[(Monomial, loc, sd), ...]
ODE_MAX_EVENTS = 16         # events=[(time, species, factor, amount), ...] per experiment
ODE_EQUILIBRATE_MAX_STEPS = 2000    # equilibrate=...: the attempted steps of the phase before the experiment, unless its "max_steps" says otherwise
ODE_SETTLE_MAX_STEPS = 2000         # settle=...: the attempted steps of the phase ahead of a steady output (t[-1] = inf), unless its "max_steps" says otherwise
ODE_MAX_CONDITIONS = 64     # conditions=[...], either shape: the engine's DZ_MAX_LIKELIHOOD_ITEMS (ODE_LIMITS: the one-lane shape's own four limits)
ODE_MAX_HILL_EXPONENT = 8   # Hill(species, K, n): n = 1..8, powers as repeated products
ODE_MAX_RATE_FACTORS = 4    # RateLaw(rate, factors): at most 4 Hill factors per reaction
ODE_MAX_INPUTS = 4          # inputs=[Input, ...]: piecewise-linear time courses, each on a species of its own
ODE_MAX_INPUT_KNOTS = 128   # the working knots of one experiment, over all its inputs together (csrc/dz_ode.h: MAX_INPUT_KNOTS)
ODE_MAX_VIEW_COORDINATES = 128      # conditions=[dict(params=...)]: P, one more than the largest index the network reads (csrc/dz_ode.h: VIEWS)
_INT = (int, np.integer)
_REAL = (int, np.integer, float, np.floating)


def _is_int(v, lo=None, hi=None):
    """v is an integer and no bool, with lo <= v and v <= hi where they are given."""
    return not isinstance(v, bool) and isinstance(v, _INT) and (lo is None or v >= lo) and (hi is None or v <= hi)


def _is_real(v):
    """v is a finite real number and no bool."""
    return not isinstance(v, bool) and isinstance(v, _REAL) and bool(np.isfinite(v))


class Monomial:
    """10**(log10_factor + sum_i exponents[i] * x[i]): a product of powers of the sampled constants 10**x[i] times a fixed factor, for
    MassActionODELogLike -- a reaction's rate constant (kr = KD kf: Monomial({i: 1}, log10(kf)); a rate closed by a thermodynamic cycle,
    k4 = k1 k2 / k3: Monomial({0: 1, 1: 1, 2: -1})), a sampled start amount, an observable's scale factor, or the argument of a Gaussian
    constraint.  exponents: a non-empty mapping from parameter index to a finite, non-zero float; log10_factor: finite.  An immutable
    value: `exponents` is the tuple of (index, exponent) pairs in ascending index, the order in which the device and the host build add
    them (csrc/dz_ode.h)."""
    __slots__ = ("exponents", "log10_factor")

    def __init__(self, exponents, log10_factor=0.0):
        if not hasattr(exponents, "items") or len(exponents) == 0:
            raise ValueError("MassActionODELogLike: a Monomial's exponents must be a non-empty mapping {parameter index: exponent}")
        pairs = []
        for i, e in exponents.items():
            if not _is_int(i, 0):
                raise ValueError("MassActionODELogLike: a Monomial's parameter index must be a non-negative integer (got %r)" % (i,))
            if not _is_real(e) or e == 0:
                raise ValueError("MassActionODELogLike: a Monomial's exponent must be a finite, non-zero number (got %r for index %d)" % (e, i))
            pairs.append((int(i), float(e)))
        if not _is_real(log10_factor):
            raise ValueError("MassActionODELogLike: a Monomial's log10_factor must be finite (got %r)" % (log10_factor,))
        object.__setattr__(self, "exponents", tuple(sorted(pairs)))
        object.__setattr__(self, "log10_factor", float(log10_factor))

    def __setattr__(self, name, value):
        raise AttributeError("a Monomial is immutable")

    __delattr__ = __setattr__

    @property
    def indices(self):
        return tuple(i for i, _ in self.exponents)

    def value(self, x):
        """10.0**(log10_factor + sum e_i x[i]) in numpy (the solvers' own arithmetic: csrc/dz_ode.h), for the rows of x"""
        x = np.asarray(x, dtype=float)
        s = self.log10_factor
        for i, e in self.exponents:
            s = s + e * x[..., i]
        return 10.0 ** s

    def __eq__(self, other):
        return isinstance(other, Monomial) and self.exponents == other.exponents and self.log10_factor == other.log10_factor

    def __hash__(self):
        return hash((self.exponents, self.log10_factor))

    def __reduce__(self):
        return Monomial, (dict(self.exponents), self.log10_factor)

    def __repr__(self):
        return "Monomial(%r, %r)" % (dict(self.exponents), self.log10_factor)


def _checked_constant(v, what, wrong_type=None):
    """A rate constant or a Hill constant as the generators take it: a parameter index (int), a float or a Monomial.  wrong_type: the
    caller's own words for a value that is none of them."""
    if isinstance(v, Monomial):
        return v
    if _is_int(v):
        if v < 0:
            raise ValueError("MassActionODELogLike: %s: parameter index %d is negative" % (what, v))
        return int(v)
    if isinstance(v, (float, np.floating)):
        return float(v)
    raise ValueError("MassActionODELogLike: " + (wrong_type or "%s is a parameter index (int), a fixed constant (float) or a Monomial (got %r)" % (what, v)))


class Hill:
    """A saturating factor of one species in a RateLaw: y^n / (K^n + y^n) for kind "activation", K^n / (K^n + y^n) for "repression".
    species: the species' index; K: a parameter index (10**x[i] under rate_scale "log10", x[i] under "linear"), a finite float > 0 or a
    Monomial; n: an integer 1..8 (ODE_MAX_HILL_EXPONENT; powers are repeated products).  An immutable value."""
    __slots__ = ("species", "K", "n", "kind")

    def __init__(self, species, K, n=1, kind="activation"):
        if not _is_int(species, 0):
            raise ValueError("MassActionODELogLike: a Hill factor's species must be a non-negative integer (got %r)" % (species,))
        K = _checked_constant(K, "a Hill factor's K")
        if isinstance(K, float) and not (np.isfinite(K) and K > 0):
            raise ValueError("MassActionODELogLike: a Hill factor's fixed K must be finite and > 0 (got %r)" % (K,))
        if not _is_int(n, 1, ODE_MAX_HILL_EXPONENT):
            raise ValueError("MassActionODELogLike: a Hill factor's n must be an integer 1..%d (got %r)" % (ODE_MAX_HILL_EXPONENT, n))
        if kind not in ("activation", "repression"):
            raise ValueError('MassActionODELogLike: a Hill factor\'s kind must be "activation" or "repression" (got %r)' % (kind,))
        for name, v in zip(self.__slots__, (int(species), K, int(n), kind)):
            object.__setattr__(self, name, v)

    def __setattr__(self, name, value):
        raise AttributeError("a Hill factor is immutable")

    def __delattr__(self, name):
        raise AttributeError("a Hill factor is immutable")

    def _key(self):
        return (self.species, type(self.K).__name__, self.K, self.n, self.kind)

    def __eq__(self, other):
        return isinstance(other, Hill) and self._key() == other._key()

    def __hash__(self):
        return hash(self._key())

    def __reduce__(self):
        return Hill, (self.species, self.K, self.n, self.kind)

    def __repr__(self):
        return "Hill(%r, %r, %r, %r)" % (self.species, self.K, self.n, self.kind)


class RateLaw:
    """A reaction's rate beyond mass action, where its third element stands: v = k * prod_s y_s^order_s * prod_m h_m(y).
    rate: what the third element may be without it (a parameter index, a float, a Monomial); factors: at most 4 (ODE_MAX_RATE_FACTORS)
    Hill objects, multiplied in the order given; order: None -- the kinetic orders are the reactants' coefficients -- or a mapping
    {species: non-negative integer} that replaces them (kinetics apart from stoichiometry; {}: no mass-action factor).  An immutable
    value: `factors` is a tuple, `order` None or the tuple of (species, order) pairs in ascending species, zeros dropped."""
    __slots__ = ("rate", "factors", "order")

    def __init__(self, rate, factors=(), order=None):
        if isinstance(rate, RateLaw):
            raise ValueError("MassActionODELogLike: a RateLaw's rate is a parameter index, a float or a Monomial, not another RateLaw")
        rate = _checked_constant(rate, "a RateLaw's rate")
        if isinstance(rate, float) and not np.isfinite(rate):
            raise ValueError("MassActionODELogLike: a RateLaw's fixed rate constant must be finite (got %r)" % (rate,))
        try:
            factors = tuple(factors)
        except TypeError:
            factors = (factors,)
        if not all(isinstance(f, Hill) for f in factors):
            raise ValueError("MassActionODELogLike: a RateLaw's factors must be Hill objects (got %r)" % (factors,))
        if len(factors) > ODE_MAX_RATE_FACTORS:
            raise ValueError("MassActionODELogLike: a RateLaw has at most %d factors (got %d)" % (ODE_MAX_RATE_FACTORS, len(factors)))
        if order is not None:
            if not hasattr(order, "items"):
                raise ValueError("MassActionODELogLike: a RateLaw's order must be None or a mapping {species: order} (got %r)" % (order,))
            pairs = []
            for s, c in order.items():
                if not _is_int(s, 0):
                    raise ValueError("MassActionODELogLike: a RateLaw's order names species %r (a non-negative integer)" % (s,))
                if not _is_int(c, 0):
                    raise ValueError("MassActionODELogLike: a RateLaw's kinetic orders must be non-negative integers (got %r for species %d)" % (c, s))
                if c:
                    pairs.append((int(s), int(c)))
            order = tuple(sorted(pairs))
        for name, v in zip(self.__slots__, (rate, factors, order)):
            object.__setattr__(self, name, v)

    def __setattr__(self, name, value):
        raise AttributeError("a RateLaw is immutable")

    def __delattr__(self, name):
        raise AttributeError("a RateLaw is immutable")

    def _key(self):
        return (type(self.rate).__name__, self.rate, self.factors, self.order)

    def __eq__(self, other):
        return isinstance(other, RateLaw) and self._key() == other._key()

    def __hash__(self):
        return hash(self._key())

    def __reduce__(self):
        return RateLaw, (self.rate, self.factors, None if self.order is None else dict(self.order))

    def __repr__(self):
        return "RateLaw(%r, %r, %r)" % (self.rate, list(self.factors), None if self.order is None else dict(self.order))


class Noise:
    """An observable's measurement noise as a sampled quantity, for MassActionODELogLike(noise=[...]): the residual of observable q at an
    output time is scaled by s = sigma (with rel: sigma + rel * |m|, m the simulated observable) times the entry's fixed weight, and
    the term -log s is part of the likelihood.  sigma, rel: a parameter index (10**x[i] under rate_scale "log10", x[i] under "linear"),
    a finite float (sigma > 0, rel >= 0) or a Monomial; rel None: no proportional part.  dist: "normal" or "laplace" residuals; scale:
    "lin", or "log" -- the residual is ln m - ln data (rel is then refused: a proportional part on the log scale is the log scale
    itself).  An immutable value."""
    __slots__ = ("sigma", "rel", "dist", "scale")

    def __init__(self, sigma, rel=None, dist="normal", scale="lin"):
        sigma = _checked_constant(sigma, "a Noise's sigma")
        if isinstance(sigma, float) and not (np.isfinite(sigma) and sigma > 0):
            raise ValueError("MassActionODELogLike: a Noise's fixed sigma must be finite and > 0 (got %r)" % (sigma,))
        if rel is not None:
            rel = _checked_constant(rel, "a Noise's rel")
            if isinstance(rel, float) and not (np.isfinite(rel) and rel >= 0):
                raise ValueError("MassActionODELogLike: a Noise's fixed rel must be finite and >= 0 (got %r)" % (rel,))
        if dist not in ("normal", "laplace"):
            raise ValueError('MassActionODELogLike: a Noise\'s dist must be "normal" or "laplace" (got %r)' % (dist,))
        if scale not in ("lin", "log"):
            raise ValueError('MassActionODELogLike: a Noise\'s scale must be "lin" or "log" (got %r)' % (scale,))
        if rel is not None and scale == "log":
            raise ValueError('MassActionODELogLike: a Noise with scale "log" takes no rel: a proportional part on the log scale is the log scale itself')
        for name, v in zip(self.__slots__, (sigma, rel, dist, scale)):
            object.__setattr__(self, name, v)

    def __setattr__(self, name, value):
        raise AttributeError("a Noise is immutable")

    def __delattr__(self, name):
        raise AttributeError("a Noise is immutable")

    def _key(self):
        return (type(self.sigma).__name__, self.sigma, type(self.rel).__name__, self.rel, self.dist, self.scale)

    def __eq__(self, other):
        return isinstance(other, Noise) and self._key() == other._key()

    def __hash__(self):
        return hash(self._key())

    def __reduce__(self):
        return Noise, (self.sigma, self.rel, self.dist, self.scale)

    def __repr__(self):
        return "Noise(%r, %r, %r, %r)" % (self.sigma, self.rel, self.dist, self.scale)


class Input:
    """A measured or prescribed time course that drives the network, for MassActionODELogLike(inputs=[...]): the amount of `species` is
    gain * u(t), u the piecewise-linear curve through (times[k], values[k]).  species: the species' index -- nothing may produce or
    consume it; times: at least 2, finite and strictly increasing; values: one per time, finite and >= 0; gain: None, a finite float
    > 0, a parameter index (10**x[i] under rate_scale "log10", x[i] under "linear") or a Monomial: a sampled amplitude.  An immutable
    value: `times` and `values` are tuples of floats."""
    __slots__ = ("species", "times", "values", "gain")

    def __init__(self, species, times, values, gain=None):
        if not _is_int(species, 0):
            raise ValueError("MassActionODELogLike: an Input's species must be a non-negative integer (got %r)" % (species,))
        try:
            times, values = [float(v) for v in np.asarray(times, dtype=float).reshape(-1)], [float(v) for v in np.asarray(values, dtype=float).reshape(-1)]
        except (TypeError, ValueError):
            raise ValueError("MassActionODELogLike: an Input's times and values must be sequences of numbers")
        if len(times) < 2 or not np.all(np.isfinite(times)) or np.any(np.diff(times) <= 0):
            raise ValueError("MassActionODELogLike: an Input's times must be at least 2 finite, strictly increasing numbers (got %r)" % (times,))
        if len(values) != len(times) or not np.all(np.isfinite(values)) or np.any(np.asarray(values) < 0):
            raise ValueError("MassActionODELogLike: an Input's values must be finite and >= 0, one per time (got %r for %d times)" % (values, len(times)))
        if gain is not None:
            gain = _checked_constant(gain, "an Input's gain")
            if isinstance(gain, float) and not (np.isfinite(gain) and gain > 0):
                raise ValueError("MassActionODELogLike: an Input's fixed gain must be finite and > 0 (got %r)" % (gain,))
        for name, v in zip(self.__slots__, (int(species), tuple(times), tuple(values), gain)):
            object.__setattr__(self, name, v)

    def __setattr__(self, name, value):
        raise AttributeError("an Input is immutable")

    def __delattr__(self, name):
        raise AttributeError("an Input is immutable")

    def interp(self, t):
        """u(t) in numpy, without the gain (a time outside the table: the nearest end's value)"""
        return np.interp(t, self.times, self.values)

    def working_knots(self, t0, t_end):
        """The knots the solver applies between t0 and t_end (csrc/dz_ode.h, INPUTS), as (time, value, slope) in ascending time: one at
        t0 -- the table's value there, v_k + (t0 - tau_k) * s_k in the segment that holds t0, or the table value itself where t0 is a
        table time -- with that segment's slope, then the table's knots strictly inside (t0, t_end), each with its value and the slope
        of the segment that follows.  The table must cover [t0, t_end]."""
        tau, v = self.times, self.values
        slope = [(v[k + 1] - v[k]) / (tau[k + 1] - tau[k]) for k in range(len(tau) - 1)]
        k = max(j for j in range(len(tau) - 1) if tau[j] <= t0) if t0 < tau[-1] else len(tau) - 2
        first = v[k] if t0 == tau[k] else v[k + 1] if t0 == tau[k + 1] else v[k] + (t0 - tau[k]) * slope[k]
        out = [(float(t0), first, slope[k] if t0 < tau[-1] else 0.0)]
        return out + [(tau[j], v[j], slope[j]) for j in range(1, len(tau) - 1) if t0 < tau[j] < t_end]

    def _key(self):
        return (self.species, self.times, self.values, type(self.gain).__name__, self.gain)

    def __eq__(self, other):
        return isinstance(other, Input) and self._key() == other._key()

    def __hash__(self):
        return hash(self._key())

    def __reduce__(self):
        return Input, (self.species, self.times, self.values, self.gain)

    def __repr__(self):
        return "Input(%r, %r, %r, %r)" % (self.species, list(self.times), list(self.values), self.gain)


class Normalize:
    """A readout known only relative to its own time course, for MassActionODELogLike(normalize=[...]): with m_j the observable after
    `scale` at output row j of one experiment, the likelihood compares m'_j with the data.  kind "max": m' = m / max_j m (a fraction of
    the trajectory's own maximum); "ref" with t= one of the object's output times (np.inf: the steady row): m' = m / m(t) (fold change
    over a chosen point); "minmax": m' = (m - min_j m) / (max_j m - min_j m).  The extrema run over every output row, observed or not.
    t is given exactly for "ref" and not otherwise.  An immutable value."""
    __slots__ = ("kind", "t")

    def __init__(self, kind, t=None):
        if kind not in ("max", "ref", "minmax"):
            raise ValueError('MassActionODELogLike: a Normalize\'s kind must be "max", "ref" or "minmax" (got %r)' % (kind,))
        if kind == "ref":
            if isinstance(t, bool) or not isinstance(t, _REAL) or np.isnan(t) or t == -np.inf:
                raise ValueError('MassActionODELogLike: a Normalize of kind "ref" needs t=, one of the output times (np.inf: the steady row; got %r)' % (t,))
            t = float(t)
        elif t is not None:
            raise ValueError('MassActionODELogLike: a Normalize of kind %r takes no t (got %r): only "ref" names a row' % (kind, t))
        object.__setattr__(self, "kind", kind)
        object.__setattr__(self, "t", t)

    def __setattr__(self, name, value):
        raise AttributeError("a Normalize is immutable")

    def __delattr__(self, name):
        raise AttributeError("a Normalize is immutable")

    def _key(self):
        return (self.kind, self.t)

    def __eq__(self, other):
        return isinstance(other, Normalize) and self._key() == other._key()

    def __hash__(self):
        return hash(self._key())

    def __reduce__(self):
        return Normalize, (self.kind, self.t)

    def __repr__(self):
        return "Normalize(%r, %r)" % (self.kind, self.t)
