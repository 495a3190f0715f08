"""tests/density_reference.py held to mpmath, the CPU oracle held to tests/density_reference.py, and the proof that the comparison can
see a wrong element: every mutation of the formulas a slipped index would amount to moves the reference by at least 100 bounds on the
inputs, and at every shape, tests/test_density_reference_gpu.py runs on the device.

Worst error-to-bound ratios of the oracle (d = 1 .. 1024, every family): MVN 0.39, mixture 0.14, prior 0.10 -- printed by
test_oracle_likelihoods_keep_the_bounds and test_oracle_priors_keep_the_bounds; recorded with the device's in
tests/test_density_reference_gpu.py's docstring and in DESIGN.md."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import density_reference as R

ORACLE_D = (1, 2, 15, 16, 17, 100, 113, 128, 129, 200, 256, 257, 333, 1000, 1024)


# ----------------------------------------------------------------------------------------------------------------- the reference against mpmath
def _mpf(mp, v):
    """a longdouble (or float) as an mpf, exactly"""
    v = np.longdouble(v)
    hi = float(v)
    if not np.isfinite(hi):
        return mp.mpf(hi)
    return mp.mpf(hi) + mp.mpf(float(v - np.longdouble(hi)))


def _mp_mvn(mp, x, mu, M, logF, tri):
    d = len(x)
    y = [mp.mpf(float(x[j])) - mp.mpf(float(mu[j])) for j in range(d)]
    z = [mp.fsum(mp.mpf(float(M[r, c])) * y[c] for c in range(r if tri else 0, d)) for r in range(d)]
    Q = mp.fsum(zr * zr for zr in z) if tri else mp.fsum(y[r] * z[r] for r in range(d))
    return mp.mpf(float(logF)) - Q / 2


def _mp_mixture(mp, x, mus, F):
    lh = [mp.mpf(float(F[j])) - mp.fsum((mp.mpf(float(x[i])) - mp.mpf(float(mus[j, i]))) ** 2 for i in range(len(x))) / 2 for j in range(len(F))]
    m = max(lh)
    return mp.log(mp.fsum(mp.exp(v - m) for v in lh)) + m


def _mp_prior(mp, x, kind, a, b):
    s = mp.mpf(0)
    for j in range(len(x)):
        xj, aj, bj = mp.mpf(float(x[j])), mp.mpf(float(a[j])), mp.mpf(float(b[j]))
        if kind[j] == 1:
            s += -((xj - aj) / bj) ** 2 / 2 - mp.log(2 * mp.pi) / 2 - mp.log(bj)
        elif kind[j] == 2:
            if not (aj <= xj <= aj + bj):
                return mp.mpf("-inf")
            s += -mp.log(bj)
    return s


def _agree(mp, ref, bound, want, what):
    for i in range(len(ref)):
        if want[i] == mp.mpf("-inf"):
            assert np.isneginf(ref[i]), (what, i)
            continue
        err = abs(_mpf(mp, ref[i]) - want[i])
        assert err * 100 <= _mpf(mp, bound[i]), "%s point %d: the longdouble reference is %s from mpmath, its bound is %s" % (what, i, mp.nstr(err, 5), bound[i])


@pytest.mark.parametrize("family", R.FAMILIES)
def test_mvn_reference_agrees_with_mpmath(family):
    """the longdouble formula against 50-digit mpmath: 100 times closer than the bound it serves, ~400 points per family"""
    import mpmath
    mp = mpmath.mp
    with mp.workdps(50):
        for d in (1, 2, 7, 17, 33):
            P, Uf = R.matrices(family, d)
            for zero in (True, False):
                mu = R.mean(d, zero)
                X = R.mvn_points(d, mu, n=20, key=1)
                for tri, M in ((False, P), (True, Uf)):
                    ref, bound = R.mvn(X, mu, M, R.log_f(d), tri)
                    want = [_mp_mvn(mp, X[i], mu, M, R.log_f(d), tri) for i in range(len(X))]
                    _agree(mp, ref, bound, want, "mvn %s d=%d tri=%d zero=%d" % (family, d, tri, zero))


def test_mixture_reference_agrees_with_mpmath():
    import mpmath
    mp = mpmath.mp
    with mp.workdps(50):
        for d in (1, 2, 10, 33):
            for J in R.MIX_J:
                for sep in R.MIX_SEP:
                    mus, F = R.mixtures(d, J, sep)
                    X, tags = R.mixture_points(d, mus, n=16, key=1)
                    ref, bound = R.mixture(X, mus, F)[:2]
                    want = [_mp_mixture(mp, X[i], mus, F) for i in range(len(X))]
                    _agree(mp, ref, bound, want, "mixture d=%d J=%d sep=%g" % (d, J, sep))


def test_prior_reference_agrees_with_mpmath():
    import mpmath
    mp = mpmath.mp
    seen_inf = 0
    with mp.workdps(50):
        assert abs(_mpf(mp, R.HALF_LOG_2PI) - mp.log(2 * mp.pi) / 2) < mp.mpf(2) ** -63
        for d in (1, 2, 3, 17, 129):
            for pattern in R.PRIOR_PATTERNS:
                kind, a, b = R.priors(d, pattern)
                X, tags = R.prior_points(d, kind, a, b, n=24, key=1)
                ref, bound = R.prior(X, kind, a, b)
                want = [_mp_prior(mp, X[i], kind, a, b) for i in range(len(X))]
                _agree(mp, ref, bound, want, "prior d=%d %s" % (d, pattern))
                assert (np.isneginf(ref) == (tags == "out")).all()
                seen_inf += int(np.isneginf(ref).sum())
    assert seen_inf > 0


# ----------------------------------------------------------------------------------------------------------------- the oracle against the reference
def _oracle(d, N=3, **kw):
    return O.Engine(nchains=N, ndim=d, history_capacity=kw.pop("history_capacity", 8), **kw)


@pytest.mark.parametrize("d", ORACLE_D)
def test_oracle_likelihoods_keep_the_bounds(d):
    """orc_loglike, MVN dense and triangular (four matrix families, zero and non-zero mean, logF = -1.2345 d) and the mixture
    (J = 1, 2, 3, 32; centres 0.5 and 5 apart), against the longdouble formulas: every point within its bound"""
    worst = {"mvn": 0.0, "mixture": 0.0}
    e = _oracle(d)
    n = 48 if d <= 333 else 24
    for family in R.FAMILIES:
        P, Uf = R.matrices(family, d)
        for zero in (True, False):
            mu = R.mean(d, zero)
            X = R.mvn_points(d, mu, n=n)
            for tri, M in ((False, P), (True, Uf)):
                e.set_likelihood_mvn(mu, M, int(tri), R.log_f(d))
                got = np.array([e.loglike(x) for x in X])
                ref, bound = R.mvn(X, mu, M, R.log_f(d), tri)
                worst["mvn"] = max(worst["mvn"], R.check(got, ref, bound, "oracle mvn %s d=%d tri=%d zero-mean=%d" % (family, d, tri, zero)))
                assert got[R.SPECIAL[0]] == R.log_f(d)              # Q = 0 at the mean: the normalisation exactly
    for J in R.MIX_J:
        for sep in R.MIX_SEP:
            mus, F = R.mixtures(d, J, sep)
            X, tags = R.mixture_points(d, mus, n=32)
            e.set_likelihood_mixture(mus, F)
            got = np.array([e.loglike(x) for x in X])
            ref, bound = R.mixture(X, mus, F)[:2]
            worst["mixture"] = max(worst["mixture"], R.check(got, ref, bound, "oracle mixture d=%d J=%d sep=%g" % (d, J, sep)))
    print("oracle d=%d worst error / bound: mvn %.3f mixture %.3f" % (d, worst["mvn"], worst["mixture"]))


@pytest.mark.parametrize("d", ORACLE_D)
def test_oracle_priors_keep_the_bounds(d):
    """The oracle has no prior accessor: three generations without hard boundaries from states inside (and on the edges of) the supports, then
    get_state()'s log prior and log likelihood at the returned states against the reference (mixed kinds beside an MVN, all-uniform beside a
    mixture, all-flat)."""
    worst = 0.0
    N = 16
    for pattern in R.PRIOR_PATTERNS:
        kind, a, b = R.priors(d, pattern)
        X0, tags = R.prior_points(d, kind, a, b, n=N + 32)
        keep = np.nonzero(tags != "out")[0]
        X0, Z0 = X0[keep[:N]], X0[keep]
        assert {"lo", "hi"} <= set(tags[keep[:N]]) or not (kind == 2).any()
        e = O.Engine(nchains=N, ndim=d, multitry=3, hardboundaries=0, history_thin=1, history_capacity=len(Z0) + 8 * N, seed=d)
        e.set_prior(kind, a, b)
        e.set_history(Z0)
        if pattern == "uniform":
            mus, F = R.mixtures(d, 3, 5.0)
            e.set_likelihood_mixture(mus, F)
            like = lambda X: R.mixture(X, mus, F)[:2]
        else:
            P, Uf = R.matrices("a", d)
            mu = R.mean(d, False)
            e.set_likelihood_mvn(mu, Uf, 1, R.log_f(d))
            like = lambda X: R.mvn(X, mu, Uf, R.log_f(d), True)
        e.set_state(X0)
        e.step(3)
        X, lp, ll = e.get_state()
        ref, bound = R.prior(X, kind, a, b)
        worst = max(worst, R.check(lp, ref, bound, "oracle prior d=%d %s" % (d, pattern)))
        if pattern == "flat":
            assert not lp.any()
        ref, bound = like(X)
        R.check(ll, ref, bound, "oracle likelihood beside the prior d=%d %s" % (d, pattern))
        assert np.isfinite(lp).all()
    print("oracle d=%d worst prior error / bound: %.3f" % (d, worst))


# ----------------------------------------------------------------------------------------------------------------- resolving power
def _moved(ref, bound, other, mask=None):
    """how many bounds the mutated formula lies from the reference, the smallest over the points"""
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.abs(other - ref) / bound
    r = np.where(np.isnan(r), 0, r)
    return float(r[mask].min() if mask is not None else r.min())


@pytest.mark.parametrize("d,tri", R.mvn_shapes())
def test_a_wrong_matrix_element_moves_the_mvn_reference_by_100_bounds(d, tri):
    """At every (d, form) an MVN kernel is run at on the device, with the family (a) and (c) inputs: dropping the last dimension, reading the
    factor transposed, swapping the stored rows 15 and 16 (d > 16), zeroing the mean's last element -- each moves the reference by at least 100
    bounds on EVERY ordinary point (the mean itself and the +-0.0 point have no quadratic form to move)."""
    n = 40 if d <= 333 else 16
    for family in ("a", "c"):
        P, Uf = R.matrices(family, d)
        M = Uf if tri else P
        for zero in (True, False):
            mu = R.mean(d, zero)
            X = R.mvn_points(d, mu, n=n)
            g = R.generic(n)
            ref, bound = R.mvn(X, mu, M, R.log_f(d), tri)
            muts = {}
            if d > 1:
                muts["last dimension dropped"] = R.mvn(X[:, :-1], mu[:-1], M[:-1, :-1], R.log_f(d), tri)[0]
            else:
                muts["last dimension dropped"] = np.full(n, np.longdouble(R.log_f(d)))
            if tri and d > 1:
                muts["factor transposed"] = _tri_transposed(X, mu, M, R.log_f(d))
            if d > 16:
                Ms = M.copy(); Ms[[15, 16]] = Ms[[16, 15]]
                muts["rows 15 and 16 swapped"] = R.mvn(X, mu, Ms, R.log_f(d), tri)[0]
            if not zero:
                m2 = mu.copy(); m2[-1] = 0.0
                muts["mean's last element zeroed"] = R.mvn(X, m2, M, R.log_f(d), tri)[0]
            for name, other in muts.items():
                r = _moved(ref, bound, other, g)
                assert r >= R.RESOLVE, "family %s d=%d tri=%d zero-mean=%d: `%s' moves the reference by only %.3g bounds on some point" % (family, d, tri, zero, name, r)


def _tri_transposed(X, mu, Uf, logF):
    """logF - |U^T y|^2 / 2"""
    Y = R._ld(X) - R._ld(mu)[None, :]
    Z = R._mm(Y, R._ld(np.triu(Uf).T))
    return np.longdouble(logF) - np.sum(Z * Z, axis=1) / 2


@pytest.mark.parametrize("d", R.prior_shapes())
def test_a_dropped_component_or_a_wrong_scale_moves_the_reference_by_100_bounds(d):
    for J in R.MIX_J[1:]:
        for sep in R.MIX_SEP:
            mus, F = R.mixtures(d, J, sep)
            X, tags = R.mixture_points(d, mus, n=64)
            ref, bound = R.mixture(X, mus, F)[:2]
            other = R.mixture(X, mus[:-1], F[:-1])[0]
            r = _moved(ref, bound, other, tags == "last")
            assert r >= R.RESOLVE, "d=%d J=%d sep=%g: dropping the last component moves a point next to it by only %.3g bounds" % (d, J, sep, r)
            other = R.mixture(X[:, :-1], mus[:, :-1], F)[0] if d > 1 else None
            if other is not None:
                r = _moved(ref, bound, other, tags == "near")
                assert r >= R.RESOLVE, "d=%d J=%d sep=%g: dropping the last dimension moves a point by only %.3g bounds" % (d, J, sep, r)
    kind, a, b = R.priors(d, "mixed")
    X, tags = R.prior_points(d, kind, a, b, n=64)
    ref, bound = R.prior(X, kind, a, b)
    other = R.prior(X, kind, a, b, swap_scale=True)[0]
    fin = np.isfinite(ref)
    r = _moved(ref[fin], bound[fin], other[fin])
    assert r >= R.RESOLVE, "d=%d: b for 1 / b and no log b in the normal prior moves some point by only %.3g bounds" % (d, r)
    if d > 1 and kind[-1] != 0:
        other = R.prior(X[:, :-1], kind[:-1], a[:-1], b[:-1])[0]
        fin2 = fin & np.isfinite(other)
        assert _moved(ref[fin2], bound[fin2], other[fin2]) >= R.RESOLVE


# ----------------------------------------------------------------------------------------------------------------- coverage of the inputs
def test_the_inputs_reach_the_edges_they_are_meant_to():
    d = 17
    kind, a, b = R.priors(d, "mixed")
    X, tags = R.prior_points(d, kind, a, b, n=64)
    uni = kind == 2
    assert set(kind) == {0, 1, 2} and not (b == 1.0).any()
    assert (X[tags == "lo"][:, uni] == a[uni]).all() and (tags == "lo").any()                     # both ends of the support occur ...
    assert (X[tags == "hi"][:, uni] == (a + b)[uni]).all() and (tags == "hi").any()
    ref = R.prior(X, kind, a, b)[0]
    assert np.isfinite(ref[(tags == "lo") | (tags == "hi")]).all()                                 # ... and belong to it
    out = X[tags == "out"]
    assert len(out) >= 2 and np.isneginf(ref[tags == "out"]).all()
    assert ((out > a + b) | (out < a))[:, uni].sum(axis=1).tolist() == [1] * len(out)             # one dimension, one ulp
    assert (out[:, uni] > (a + b)[uni]).any() and (out[:, uni] < a[uni]).any()
    for J in R.MIX_J[1:]:
        for sep in R.MIX_SEP:
            mus, F = R.mixtures(d, J, sep)
            X, tags = R.mixture_points(d, mus, n=64)
            ref, bound, lh, S = R.mixture(X, mus, F)
            assert (S[tags == "centre"].min(axis=1) == 0).all() and (tags == "centre").any()      # S = 0
            top = np.sort(lh[tags == "tie"], axis=1)
            assert (top[:, -1] == top[:, -2]).all() and (tags == "tie").any()                     # an exact tie of the two largest terms
            far = lh[tags == "far"]
            gap = np.sort(far, axis=1)
            assert (gap[:, -2] - gap[:, -1] < -746).all() and (tags == "far").any()               # every other term underflows (exp(-745.2) = 0 in binary64)
    for dd in (1, 17, 100):
        mu = R.mean(dd, False)
        X = R.mvn_points(dd, mu, n=16)
        P, Uf = R.matrices("a", dd)
        assert R.mvn(X, mu, P, R.log_f(dd), False)[0][R.SPECIAL[0]] == np.longdouble(R.log_f(dd))        # Q = 0
        z = X[R.SPECIAL[1]]
        assert (z == 0).all() and (np.signbit(z).any() or dd < 2) and not np.signbit(z).all()
        assert (mu != 0).all() and (dd == 1 or not np.allclose(mu, mu[::-1]))
    # every chunk count 1..8 of the prior / mixture kernels and every row-tile count 1..16 of the persistent kernels is reached by a listed dimension
    assert {R.chunks_of(dd) for dd in R.PRIOR_D} >= {1, 2, 3, 4, 8} and {R.nch_of(dd) for dd in R.PRIOR_D} == {1, 2, 4, 8}
    allmvn = {dd for dd, _ in R.mvn_shapes()}
    assert {R.row_tiles_of(dd) for dd in allmvn if dd <= 256} == set(range(1, 17)), sorted({R.row_tiles_of(dd) for dd in allmvn if dd <= 256})
    assert {R.chunks_of(dd) for dd in allmvn | set(R.PRIOR_D)} >= {1, 2, 3, 4, 8}
