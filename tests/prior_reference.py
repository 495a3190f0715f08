"""The eleven extended prior families (dz_set_prior_ext, kinds 3..13) and the three old kinds as plain formulas at 40 digits, the error bounds a
binary64 evaluation of them must keep, and the seeded inputs tests/test_prior_ext_cpu.py (the host twin) and tests/test_prior_ext_gpu.py (the
kernel) are held to.  numpy and mpmath only: nothing here knows the engine, its header or scipy.

THE FORMULAS, from the distributions' definitions.  x, loc = a, scale = b and the shapes are binary64 numbers taken exactly; z = (x - a) / b.

    laplace       pdf exp(-|z|) / (2 b)
    cauchy        pdf 1 / (pi b (1 + z^2))
    t, nu         pdf Gamma((nu + 1) / 2) / (sqrt(nu pi) Gamma(nu / 2) b) (1 + z^2 / nu)^(-(nu + 1) / 2)
    lognorm, s    pdf exp(-(log z)^2 / (2 s^2)) / (s z sqrt(2 pi) b), z > 0
    gamma, k      pdf z^(k - 1) exp(-z) / (Gamma(k) b), z >= 0      (z = 0: +inf for k < 1, 1 / b for k = 1, 0 for k > 1)
    beta, al, be  pdf z^(al - 1) (1 - z)^(be - 1) Gamma(al + be) / (Gamma(al) Gamma(be) b), 0 <= z <= 1   (the ends as gamma's)
    halfnorm      pdf sqrt(2 / pi) exp(-z^2 / 2) / b, z >= 0
    halfcauchy    pdf 2 / (pi b (1 + z^2)), z >= 0
    truncnorm     pdf exp(-z^2 / 2) / (sqrt(2 pi) (Phi(hi) - Phi(lo)) b), lo <= z <= hi   (Phi from erfc at 40 digits: no cancellation matters there)
    loguniform    pdf 1 / (z log(hi / lo) b), lo <= z <= hi
    invgamma, k   pdf z^(-k - 1) exp(-1 / z) / (Gamma(k) b), z > 0
    flat 0;  norm exp(-z^2 / 2) / (sqrt(2 pi) b);  uniform 1 / b on [a, a + b]
    Outside the support the log density is -inf.  A point's prior is the sum over its dimensions.

THE BOUNDS, u = 2^-53, first order in u (n u < 1e-13 for every count here).  They are not measured: every value the evaluation forms carries a
running bound on its absolute error through the standard model fl(a op b) = (a op b)(1 + e), |e| <= u (class B below: a sum adds the operands'
bounds and u |result|; a product |a| eb + |b| ea + u |result|; a quotient likewise; a logarithm passes ea / |a| on and adds its own error).
The evaluation whose roundings are counted is the one the interface states (include/dreamzs.h; DESIGN.md section 7, "Extended priors"): z = (x - a) rb with
rb = fl(1 / b); the core left to right; one final addition of c; c made in binary64 from log, lgamma and erfc, and it includes -log b.
    dz::dlog is within 2 ulp (tests/test_contract_primitives.py): 4 u |value|.
    The host's log is within 1 ulp (glibc's documented bound for x86-64): 2 u |value|.
    Two quantities cannot be derived from the project and were measured against mpmath over the ranges the shapes of these inputs reach,
    on glibc 2.35: lgamma on [0.2, 65] (40 000 seeded arguments and the shapes' own) is off by at most 1.98 ulp, erfc on [-6, 6] (40 000 seeded
    arguments and the truncations' own) by at most 2.84 ulp.  Twice the worst observed is allowed: LGAMMA_ULP = 4, ERFC_ULP = 6.
    A point's sum of d terms in any order adds at most (d - 1) u sum |term|.
Near an end of the support the bound grows with the conditioning of the logarithm there (the relative error 3 u of z becomes 3 u z / (1 - z) in
log(1 - z)): that is the evaluation's true error, not slack.

THE INPUTS (cases()): per family, shapes on both sides of the special cases -- k and alpha, beta in {0.5, 1, 2.5}, nu in {1, 4.5, 60}, truncations
(-1, 2), (3, 6), (-inf, 0.5) --, scales 1e-3, 1 and 1e3 (and the dyadic 2^-10, 2^10), and per parameter set points well inside the support (seeded),
within 1e-12 b of each finite end on both sides, exactly on each finite end, and outside.  A point exactly on an end other than z = 0 is made with a
dyadic loc and scale, so that the end is a binary64 number and z is exact; at z = 0 (x = a) it is exact for every scale."""
import mpmath
import numpy as np

mp = mpmath.mp
mp.dps = 40
MPF = mpmath.mpf
U = MPF(2) ** -53
DLOG_ULP, LOG_ULP, LGAMMA_ULP, ERFC_ULP = 2, 1, 4, 6
INF = float("inf")
NAMES = {0: "flat", 1: "norm", 2: "uniform", 3: "laplace", 4: "cauchy", 5: "t", 6: "lognorm", 7: "gamma", 8: "beta", 9: "halfnorm", 10: "halfcauchy",
         11: "truncnorm", 12: "loguniform", 13: "invgamma"}


# ------------------------------------------------------------------------------------------------------------------ the formulas
def _mass(lo, hi):
    r = mpmath.sqrt(MPF(2))
    return (mpmath.erfc(MPF(lo) / r) - mpmath.erfc(MPF(hi) / r)) / 2


def logpdf(kind, x, a, b, s1=0.0, s2=0.0):
    """the log density at x (mpmath number, or +-inf as an mpf)"""
    if kind == 0:
        return MPF(0)
    x, a, b = MPF(float(x)), MPF(float(a)), MPF(float(b))
    z = (x - a) / b
    lb = mpmath.log(b)
    ninf, pinf = MPF("-inf"), MPF("inf")
    pi = mpmath.pi
    if kind == 1:
        return -z * z / 2 - mpmath.log(2 * pi) / 2 - lb
    if kind == 2:
        return -lb if 0 <= z <= 1 else ninf
    if kind == 3:
        return -abs(z) - mpmath.log(2) - lb
    if kind == 4:
        return -mpmath.log(pi * (1 + z * z)) - lb
    if kind == 5:
        nu = MPF(float(s1))
        return mpmath.loggamma((nu + 1) / 2) - mpmath.loggamma(nu / 2) - mpmath.log(nu * pi) / 2 - (nu + 1) / 2 * mpmath.log(1 + z * z / nu) - lb
    if kind == 6:
        s = MPF(float(s1))
        return -mpmath.log(z) ** 2 / (2 * s * s) - mpmath.log(s * z * mpmath.sqrt(2 * pi)) - lb if z > 0 else ninf
    if kind == 7:
        k = MPF(float(s1))
        if z < 0:
            return ninf
        if z == 0:
            return pinf if k < 1 else (-lb if k == 1 else ninf)
        return (k - 1) * mpmath.log(z) - z - mpmath.loggamma(k) - lb
    if kind == 8:
        al, be = MPF(float(s1)), MPF(float(s2))
        if z < 0 or z > 1:
            return ninf
        c = mpmath.loggamma(al + be) - mpmath.loggamma(al) - mpmath.loggamma(be) - lb
        if z == 0 and al != 1:
            return pinf if al < 1 else ninf
        if z == 1 and be != 1:
            return pinf if be < 1 else ninf
        t1 = (al - 1) * mpmath.log(z) if al != 1 else 0
        t2 = (be - 1) * mpmath.log(1 - z) if be != 1 else 0
        return t1 + t2 + c
    if kind == 9:
        return mpmath.log(2 / pi) / 2 - z * z / 2 - lb if z >= 0 else ninf
    if kind == 10:
        return mpmath.log(2 / pi) - mpmath.log(1 + z * z) - lb if z >= 0 else ninf
    if kind == 11:
        return -z * z / 2 - mpmath.log(2 * pi) / 2 - mpmath.log(_mass(s1, s2)) - lb if MPF(s1) <= z <= MPF(s2) else ninf
    if kind == 12:
        lo, hi = MPF(float(s1)), MPF(float(s2))
        return -mpmath.log(z) - mpmath.log(mpmath.log(hi / lo)) - lb if lo <= z <= hi else ninf
    if kind == 13:
        k = MPF(float(s1))
        return -(k + 1) * mpmath.log(z) - 1 / z - mpmath.loggamma(k) - lb if z > 0 else ninf
    raise ValueError(kind)


# ------------------------------------------------------------------------------------------------------------------ the bounds
class B:
    """a value at 40 digits and a bound on the absolute error of its binary64 counterpart"""

    def __init__(self, v, e=0):
        self.v, self.e = MPF(v), MPF(e)

    @staticmethod
    def of(x):
        return x if isinstance(x, B) else B(x)

    def __add__(self, o):
        o = B.of(o); r = self.v + o.v
        return B(r, self.e + o.e + U * abs(r))

    def __sub__(self, o):
        o = B.of(o); r = self.v - o.v
        return B(r, self.e + o.e + U * abs(r))

    def __mul__(self, o):
        o = B.of(o); r = self.v * o.v
        return B(r, abs(self.v) * o.e + abs(o.v) * self.e + U * abs(r))

    def __truediv__(self, o):
        o = B.of(o); r = self.v / o.v
        return B(r, self.e / abs(o.v) + abs(r) * o.e / abs(o.v) + U * abs(r))

    def __neg__(self):
        return B(-self.v, self.e)

    def half(self):          # exact
        return B(self.v / 2, self.e / 2)

    def fn(self, f, df, ulps):
        """f of this value by a routine that is within `ulps` ulp (an ulp is at most 2 u |value|); df: |f'| there"""
        r = f(self.v)
        return B(r, self.e * df + 2 * ulps * U * abs(r))

    def log(self, ulps):
        return self.fn(mpmath.log, 1 / abs(self.v), ulps)


def rounded(x):
    """a real constant as the binary64 number nearest to it"""
    return B(x, U * abs(MPF(x)))


def _lgamma(x):
    return B.of(x).fn(mpmath.loggamma, abs(mpmath.digamma(B.of(x).v)), LGAMMA_ULP)


def _erfc_half(x):      # 0.5 erfc(x r), r = fl(1 / sqrt 2)
    t = B.of(x) * rounded(1 / mpmath.sqrt(2))
    return t.fn(mpmath.erfc, 2 / mpmath.sqrt(mpmath.pi) * mpmath.exp(-t.v * t.v), ERFC_ULP).half()


def const_bound(kind, b, s1, s2):
    """the bound on |c - exact|, c = c0 - log b as the host makes it"""
    b, s1, s2 = MPF(float(b)), MPF(float(s1)), MPF(float(s2))
    pi = rounded(mpmath.pi)
    lb = B(b).log(LOG_ULP)
    if kind in (1, 2):
        return B(b).log(DLOG_ULP).e
    if kind == 3:
        c0 = -B(2).log(LOG_ULP)
    elif kind == 4:
        c0 = -pi.log(LOG_ULP)
    elif kind == 5:
        c0 = _lgamma((B(s1) + 1).half()) - _lgamma(B(s1).half()) - (B(s1) * pi).log(LOG_ULP).half()
    elif kind == 6:
        c0 = -B(s1).log(LOG_ULP) - (B(2) * pi).log(LOG_ULP).half()
    elif kind == 7 or kind == 13:
        c0 = -_lgamma(s1)
    elif kind == 8:
        c0 = _lgamma(B(s1) + B(s2)) - _lgamma(s1) - _lgamma(s2)
    elif kind == 9:
        c0 = (B(2) / pi).log(LOG_ULP).half()
    elif kind == 10:
        c0 = (B(2) / pi).log(LOG_ULP)
    elif kind == 11:
        lo, hi = float(s1), float(s2)
        zero = B(0)
        if lo > 0 and hi > 0:
            m = _erfc_half(lo) - (_erfc_half(hi) if hi != INF else zero)
        elif lo < 0 and hi < 0:
            m = _erfc_half(-hi) - (_erfc_half(-lo) if lo != -INF else zero)
        else:
            m = B(1) - (_erfc_half(-lo) if lo != -INF else zero) - (_erfc_half(hi) if hi != INF else zero)
        c0 = -(B(2) * pi).log(LOG_ULP).half() - m.log(LOG_ULP)
    elif kind == 12:
        c0 = -(B(s2) / B(s1)).log(LOG_ULP).log(LOG_ULP)
    else:
        raise ValueError(kind)
    return (c0 - lb).e


def term_bound(kind, x, a, b, s1=0.0, s2=0.0, ref=None):
    """the bound on |term - ref| for a finite ref (0 where the term is decided without arithmetic)"""
    if kind == 0:
        return MPF(0)
    ec = const_bound(kind, b, s1, s2)
    if kind == 2:
        return ec
    z = (B(float(x)) - B(float(a))) * (B(1) / B(float(b)))
    if kind == 1:
        return ((-(z * z)).half() - rounded(mpmath.log(2 * mpmath.pi) / 2) - B(mpmath.log(MPF(float(b))), ec)).e
    s1b, s2b = B(float(s1)) if np.isfinite(s1) else None, B(float(s2)) if np.isfinite(s2) else None
    if kind == 3:
        core = -z
    elif kind in (4, 10):
        core = -(B(1) + z * z).log(DLOG_ULP)
    elif kind == 5:
        core = -((s1b + 1).half() * (B(1) + (z * z) * (B(1) / s1b)).log(DLOG_ULP))
    elif kind == 6:
        w = z.log(DLOG_ULP)
        core = -(w * w) * (B(1) / (B(2) * (s1b * s1b))) - w
    elif kind == 7:
        core = -z if s1 == 1 else (s1b - 1) * z.log(DLOG_ULP) - z
    elif kind == 8:
        if z.v == 0 or z.v == 1:      # (both coefficients' terms absent or exactly 0 there)
            core = B(0)
        else:
            t1 = (s1b - 1) * z.log(DLOG_ULP) if s1 != 1 else None
            t2 = (s2b - 1) * (B(1) - z).log(DLOG_ULP) if s2 != 1 else None
            core = t1 + t2 if (t1 is not None and t2 is not None) else (t1 if t1 is not None else (t2 if t2 is not None else B(0)))
    elif kind in (9, 11):
        core = (-(z * z)).half()
    elif kind == 12:
        core = -z.log(DLOG_ULP)
    elif kind == 13:
        core = -((s1b + 1) * z.log(DLOG_ULP)) - B(1) / z
    else:
        raise ValueError(kind)
    c = B((MPF(ref) if ref is not None else logpdf(kind, x, a, b, s1, s2)) - core.v, ec)
    return (core + c).e


def point(kind, a, b, s1, s2, x):
    """-> (ref, bound) of one point's prior as mpmath numbers: the sum of the terms; the bound 0 where ref is not finite"""
    terms = [logpdf(int(kind[j]), x[j], a[j], b[j], s1[j], s2[j]) for j in range(len(kind))]
    ref = mpmath.fsum(terms)
    if not mpmath.isfinite(ref):
        return ref, MPF(0)
    bound = mpmath.fsum(term_bound(int(kind[j]), x[j], a[j], b[j], s1[j], s2[j], terms[j]) for j in range(len(kind)))
    return ref, bound + (len(kind) - 1) * U * mpmath.fsum(abs(t) for t in terms)


def points(kind, a, b, s1, s2, X):
    out = [point(kind, a, b, s1, s2, row) for row in np.atleast_2d(X)]
    return [r for r, _ in out], [e for _, e in out]


def agrees(got, ref, bound):
    """is the binary64 number `got` what the reference allows: the same infinity, or within the bound"""
    if not mpmath.isfinite(ref):
        return float(ref) == got
    return bool(np.isfinite(got)) and abs(MPF(float(got)) - ref) <= bound


# ------------------------------------------------------------------------------------------------------------------ the inputs
SHAPES = {3: [(0.0, 0.0)], 4: [(0.0, 0.0)], 5: [(1.0, 0.0), (4.5, 0.0), (60.0, 0.0)], 6: [(0.25, 0.0), (1.5, 0.0)], 7: [(0.5, 0.0), (1.0, 0.0), (2.5, 0.0)],
          8: [(al, be) for al in (0.5, 1.0, 2.5) for be in (0.5, 1.0, 2.5)], 9: [(0.0, 0.0)], 10: [(0.0, 0.0)],
          11: [(-1.0, 2.0), (3.0, 6.0), (-INF, 0.5)], 12: [(0.5, 8.0), (1e-3, 1e2)], 13: [(0.5, 0.0), (2.5, 0.0)], 1: [(0.0, 0.0)], 2: [(0.0, 0.0)]}
LOCSCALE = [(0.0, 1.0), (-1.7, 1e-3), (0.3, 1e3), (0.75, 2.0 ** -10), (-3.0, 2.0 ** 10)]


def z_support(kind, s1, s2):
    if kind in (2, 8):
        return 0.0, 1.0
    if kind in (6, 7, 9, 10, 13):
        return 0.0, INF
    if kind in (11, 12):
        return s1, s2
    return -INF, INF


def cases(seed=20240611, inside=6):
    """[(kind, a, b, s1, s2, x[m])]: every family, every shape, every (loc, scale); x as the module docstring describes"""
    rng = np.random.default_rng(seed)
    out = []
    for kind in sorted(SHAPES):
        for s1, s2 in SHAPES[kind]:
            for a, b in LOCSCALE:
                lo, hi = z_support(kind, s1, s2)
                dyadic = b in (1.0, 2.0 ** -10, 2.0 ** 10)
                if lo == -INF and hi == INF:
                    zs = list(rng.normal(0.0, 2.0, inside)) + [0.0, 37.5, -1e3]
                elif hi == INF:
                    zs = list(lo + rng.gamma(2.0, 1.5, inside)) + [lo + 1e-12, lo - 1e-12, lo - 2.5, lo + 40.0]
                    zs += [lo] if (lo == 0.0 or dyadic) else []
                elif lo == -INF:
                    zs = list(hi - rng.gamma(2.0, 1.5, inside)) + [hi - 1e-12, hi + 1e-12, hi + 2.5] + ([hi] if dyadic else [])
                else:
                    zs = list(rng.uniform(lo + 0.05 * (hi - lo), hi - 0.05 * (hi - lo), inside))
                    zs += [lo + 1e-12 * max(1.0, abs(lo)), lo - 1e-12 * max(1.0, abs(lo)), hi - 1e-12 * abs(hi), hi + 1e-12 * abs(hi), lo - 0.5 * (hi - lo), hi + 0.5 * (hi - lo)]
                    zs += [lo] if (lo == 0.0 or dyadic) else []
                    zs += [hi] if dyadic else []
                x = np.array([a + b * z for z in zs])
                out.append((kind, a, b, s1, s2, x))
    return out


def mixed_point_set(d, n, seed, flat_every=0, first=0):
    """(kind, a, b, s1, s2, X[n, d]) for the kernel's shapes: the q-th non-flat dimension takes kind 1 + (q + first) % 13 (every kind once per 13;
    flat_every = 2: a flat dimension after every other one), shapes and scales cycling through SHAPES / LOCSCALE, the rows drawn well inside every
    support except that row i of every third dimension sits outside (i % 7 == 3) or exactly on a lower end at z = 0 (i % 7 == 5) -- there only where
    the log density is finite at that end, or d == 1: in a sum of several dimensions +inf beside -inf would make the reference itself NaN."""
    rng = np.random.default_rng(seed)
    kind, a, b, s1, s2 = np.zeros(d, np.int32), np.zeros(d), np.ones(d), np.zeros(d), np.zeros(d)
    X = np.zeros((n, d))
    q = 0
    for j in range(d):
        if flat_every and j % flat_every == 1:
            X[:, j] = rng.normal(0, 3, n)
            continue
        k = 1 + (q + first) % 13
        sh = SHAPES[k][(q // 13) % len(SHAPES[k])]
        a[j], b[j] = LOCSCALE[(q // 3) % len(LOCSCALE)]
        kind[j], s1[j], s2[j] = k, sh[0], sh[1]
        lo, hi = z_support(k, sh[0], sh[1])
        if lo == -INF and hi == INF:
            z = rng.normal(0, 1.5, n)
        elif hi == INF:
            z = lo + rng.gamma(2.0, 1.0, n) + 0.01
        elif lo == -INF:
            z = hi - rng.gamma(2.0, 1.0, n) - 0.01
        else:
            z = rng.uniform(lo + 0.05 * (hi - lo), hi - 0.05 * (hi - lo), n)
        if q % 3 == 0 and lo != -INF:
            for i in range(n):
                if i % 7 == 3:
                    z[i] = lo - 0.75
                elif i % 7 == 5 and lo == 0.0 and (d == 1 or k in (2, 9, 10) or (k in (7, 8) and sh[0] == 1.0)):
                    z[i] = 0.0
        X[:, j] = a[j] + b[j] * z
        q += 1
    return kind, a, b, s1, s2, X
