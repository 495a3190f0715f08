"""Parameter priors -- the interface of pydream/parameters.py (SampledParam, FlatParam): ``dsize``, ``interval``,
``random``, ``prior``.

Additionally each parameter can describe itself to the device (``device_prior``) so that
``scipy.stats.norm`` / ``scipy.stats.uniform`` / flat priors are evaluated inside the HIP kernels
(``dz_set_prior``).  ``device_prior_ext`` does the same for eleven more families -- laplace, cauchy, t, lognorm,
gamma (and expon), beta, halfnorm, halfcauchy, truncnorm, loguniform / reciprocal, invgamma -- which a kernel of the
multi-kernel path adds beside a device likelihood (``dz_set_prior_ext``; the arithmetic: csrc/dz_prior_ext.h).
Any other distribution, and every prior beside a Python-callable likelihood, is evaluated on the host through ``.prior``.
"""
import numpy as np

# scipy's name -> (kind of dz_set_prior_ext, number of shape parameters)
_EXT_KINDS = {"norm": (1, 0), "uniform": (2, 0), "laplace": (3, 0), "cauchy": (4, 0), "t": (5, 1), "lognorm": (6, 1), "gamma": (7, 1), "expon": (7, 0),
              "beta": (8, 2), "halfnorm": (9, 0), "halfcauchy": (10, 0), "truncnorm": (11, 2), "loguniform": (12, 2), "reciprocal": (12, 2), "invgamma": (13, 1)}


class SampledParam():
    """A prior given by a frozen SciPy distribution (interface of pydream/parameters.py:6-47).

    ``SampledParam(scipy.stats.norm, loc=..., scale=...)``: the first argument is the SciPy continuous distribution
    class, everything after it is handed to that class.  The dimension of the parameter (``dsize``) is the size of
    one draw from the distribution."""

    def __init__(self, scipy_distribution, *args, **kwargs):
        self.dist = scipy_distribution(*args, **kwargs)
        self.dsize = np.size(self.random())

    def interval(self, alpha=1):
        """Central interval holding a fraction ``alpha`` of the prior mass; ``alpha = 1`` gives the support, which is
        what Dream uses as hard boundaries (parameters.py:23-26, Dream.py:86-105)."""
        return self.dist.interval(alpha)

    def random(self, reseed=False):
        """One draw from the prior.  ``reseed=True`` draws from a freshly seeded generator instead of numpy's
        global one (parameters.py:28-35: forked workers would otherwise all produce the same start)."""
        state = np.random.RandomState() if reseed else None
        return self.dist.rvs(random_state=state)

    def prior(self, q0):
        """Log prior density of the point ``q0``: the log pdf summed over the parameter's dimensions
        (parameters.py:37-47)."""
        return np.sum(self.dist.logpdf(q0))

    def device_prior(self):
        """(kind[d], a[d], b[d]) for dz_set_prior, or None if this distribution has no device form.
        kind 1 = norm(loc=a, scale=b), kind 2 = uniform(loc=a, scale=b)."""
        name = getattr(getattr(self.dist, "dist", None), "name", None)
        if name not in ("norm", "uniform"):
            return None
        try:
            shapes, loc, scale = self.dist.dist._parse_args(*self.dist.args, **self.dist.kwds)
        except Exception:
            return None
        loc = np.broadcast_to(np.asarray(loc, dtype=float), (self.dsize,)).copy()
        scale = np.broadcast_to(np.asarray(scale, dtype=float), (self.dsize,)).copy()
        kind = np.full(self.dsize, 1 if name == "norm" else 2, dtype=np.int32)
        return kind, loc, scale

    def device_prior_ext(self):
        """(kind[d], a[d], b[d], s1[d], s2[d]) for dz_set_prior_ext -- scipy's loc, scale and shapes broadcast over the parameter's
        dimensions --, or None if this distribution has no device form or its arguments cannot be parsed."""
        name = getattr(getattr(self.dist, "dist", None), "name", None)
        if name not in _EXT_KINDS:
            return None
        kind, nshapes = _EXT_KINDS[name]
        try:
            shapes, loc, scale = self.dist.dist._parse_args(*self.dist.args, **self.dist.kwds)
            if len(shapes) != nshapes:
                return None
            cols = [np.broadcast_to(np.asarray(v, dtype=float), (self.dsize,)).copy() for v in (loc, scale) + tuple(shapes)]
        except Exception:
            return None
        while len(cols) < 4:
            cols.append(np.ones(self.dsize) if name == "expon" and len(cols) == 2 else np.zeros(self.dsize))      # (expon: gamma with k = 1)
        return (np.full(self.dsize, kind, dtype=np.int32),) + tuple(cols)


class FlatParam(SampledParam):
    """An improper flat prior: log density 0 everywhere, unbounded support (interface of
    pydream/parameters.py:49-70).  ``test_value`` is any representative value; only its size is used."""

    def __init__(self, test_value):
        self.dsize = np.size(test_value)

    def prior(self, q0):
        return 0

    def interval(self, alpha=1):
        """(-inf, +inf) in every dimension, whatever ``alpha``."""
        return [[-np.inf] * self.dsize, [np.inf] * self.dsize]

    def device_prior(self):
        return np.zeros(self.dsize, dtype=np.int32), np.zeros(self.dsize), np.ones(self.dsize)

    def device_prior_ext(self):
        return np.zeros(self.dsize, dtype=np.int32), np.zeros(self.dsize), np.ones(self.dsize), np.zeros(self.dsize), np.zeros(self.dsize)
