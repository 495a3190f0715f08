"""Sampled noise models (likelihoods.Noise, MassActionODELogLike(noise=...)) without a GPU: the host build against an independent
reference in mpmath on every shape, the edges of the contract (csrc/dz_ode.h, NOISE), the cross-checks against the paths that
existed before, construction, pickling and the cache, and the cross-compilation for gfx950."""
import pickle

import numpy as np
import pytest

from pydream_amd.examples.robertson import robertson_device as ROB
from pydream_amd.likelihoods import MassActionODELogLike, Monomial, Noise

from . import ode_noise_networks as NN
from . import ode_noise_reference as NR
from .ode_support import notes

HOST_NETWORKS = ("one3", "long8", "group16", "wave64")


# ---------------------------------------------------------------------------------------------------- the host build against the reference
@pytest.mark.parametrize("case", ["index_rel", "monomial_log", "all_three"])
@pytest.mark.parametrize("name", HOST_NETWORKS)
def test_the_host_build_agrees_with_the_reference(name, case):
    """|host - reference| <= (32 + N) 2^-52 A on every live point whose integration succeeds.  Largest ratio of the error to that bound
    seen over the twelve cases: 0.121 (long8 and group16, all_three)."""
    net = NN.network(name)
    noise = NN.cases(net.P)[case]
    like = NN.like(net, noise)
    assert (like.lanes_per_point, len(like.reactions) > 16) == dict(one3=(1, False), long8=(1, True), group16=(16, True), wave64=(64, True))[name]
    assert like.d == net.P + 2 and "NOISE = true;" in like.source()
    X, dead = NN.points(net, 40, 11, noise)
    host = like.batch(X)
    assert np.all(host[dead] == -np.inf)
    ref, A, N = NR.loglike(like, X[~dead])
    ok = np.isfinite(ref)
    assert np.mean(ok) > 0.5 and np.array_equal(np.isfinite(host[~dead]), ok)
    assert np.all(N[ok] == np.sum(np.isfinite(like.data)))
    ratio = np.abs(host[~dead][ok] - ref[ok]) / NR.tolerance(A[ok], N[ok])
    print("%s %s: %d points, largest ratio %.3g" % (name, case, ok.sum(), ratio.max()))
    assert np.all(ratio <= 1.0)


# ---------------------------------------------------------------------------------------------------- edges
T_ZERO = np.array([0.0, 1.0, 2.0])


def _robertson(noise, data, sd=None, rate_scale="log10", **kw):
    return MassActionODELogLike(3, ROB.REACTIONS, ROB.Y0, T_ZERO, [[0, 0, 1]], np.asarray(data, dtype=float)[None, :], sd, rate_scale=rate_scale,
                                noise=noise, **kw)


def test_a_log_scale_observable_that_is_zero_counts_only_where_it_is_observed():
    x = np.r_[ROB.NOMINAL, -1.0]                                                  # C is exactly 0 at t = t0 = 0
    unobserved = _robertson([Noise(3, scale="log")], [np.nan, 0.2, 0.3])
    assert unobserved.simulate(x)[0, 0, 0] == 0.0 and np.isfinite(unobserved(x))
    ref, A, N = NR.loglike(unobserved, x[None, :])
    assert N[0] == 2 and abs(unobserved(x) - ref[0]) <= NR.tolerance(A[0], 2)
    observed = _robertson([Noise(3, scale="log")], [0.1, 0.2, 0.3])
    assert observed(x) == -np.inf
    assert np.isfinite(_robertson([Noise(3)], [0.1, 0.2, 0.3])(x))                # (on the linear scale a reading of 0 is a reading)


@pytest.mark.parametrize("rate_scale", ["log10", "linear"])
def test_points_whose_noise_is_not_live_are_minus_infinity(rate_scale):
    nominal = np.r_[ROB.NOMINAL, -1.0, -1.0] if rate_scale == "log10" else np.r_[10.0 ** ROB.NOMINAL, 0.1, 0.1]
    like = _robertson([Noise(3, rel=4)], [np.nan, 0.2, 0.3], rate_scale=rate_scale)
    assert np.isfinite(like(nominal))
    rows = [(3, np.nan), (3, np.inf), (3, -np.inf), (4, np.nan), (4, np.inf)]
    rows += [(3, 0.0), (3, -0.0), (3, -0.5), (4, -0.5), (4, -1e-300)] if rate_scale == "linear" else []
    X = np.tile(nominal, (len(rows), 1))
    for i, (c, v) in enumerate(rows):
        X[i, c] = v
    assert np.all(like.batch(X) == -np.inf)
    if rate_scale == "linear":                                                    # rel = 0 is allowed, sigma = 0 is not
        zero_rel = nominal.copy()
        zero_rel[4] = 0.0
        assert np.isfinite(like(zero_rel))
    else:                                                                         # 10**-745 = 0: a rel of 0 from a finite coordinate
        no_rel = nominal.copy()
        no_rel[4] = -745.0
        assert like.noise_values(no_rel)[0, 0, 1] == 0.0 and np.isfinite(like(no_rel))


# ---------------------------------------------------------------------------------------------------- cross-checks
def test_a_noise_of_one_agrees_with_the_fixed_sd_object():
    net = NN.network("one3")
    data, w = NN.data_and_weights(net, 3)
    fixed = net.like(observables=NN.observables(net), data=data, sd=w)
    sampled = net.like(observables=NN.observables(net), data=data, sd=w, noise=[Noise(1.0)] * 3)
    X = net.points(16)
    a, b = fixed.batch(X), sampled.batch(X)
    ref, A, N = NR.loglike(sampled, X)
    assert np.all(np.isfinite(a)) and np.all(np.abs(a - b) <= NR.tolerance(A, N)) and np.all(np.abs(b - ref) <= NR.tolerance(A, N))
    assert np.any(a != b)                                                         # (not to the bit: the log term moves from C into the sum)


def test_conditions_columns_equal_single_condition_objects():
    net = NN.network("group16")
    noise = NN.cases(net.P)["monomial_log"]
    conds = [dict(zip(("data", "sd"), NN.data_and_weights(net, s)), y0=net.y0 * f) for s, f in ((5, 1.0), (6, 0.5), (7, 2.0))]
    like = NN.like(net, noise, conditions=conds)
    X, dead = NN.points(net, 12, 13, noise)
    terms = like.batch_conditions(X)
    assert np.all(terms[dead] == -np.inf) and np.mean(np.isfinite(terms[~dead])) > 0.5
    for c, cond in enumerate(conds):
        single = NN.like(net, noise, data=cond["data"], sd=cond["sd"], y0=cond["y0"])
        assert terms[:, c].tobytes() == single.batch(X).tobytes()
    total = terms[:, 0]
    for c in range(1, len(conds)):
        total = total + terms[:, c]
    assert total.tobytes() == like.batch(X).tobytes()
    ref, A, N = NR.loglike(like, X[~dead])
    ok = np.isfinite(ref)
    assert np.all(np.abs(like.batch(X)[~dead][ok] - ref[ok]) <= NR.tolerance(A[ok], N[ok]))


def _ulps(a, b):
    return np.abs(a - b) / np.spacing(np.abs(b))


@pytest.mark.parametrize("name", ["one3", "long8", "group16"])
def test_noise_values_are_the_constants(name):
    net = NN.network(name)
    P = net.P
    mono = Monomial({P: 1, P + 1: -1}, -0.5)
    like = NN.like(net, [Noise(P, rel=mono), None, Noise(0.4, rel=P + 1)])
    X, _ = NN.points(net, 32, 17, [])
    X = X[np.all(np.isfinite(X), axis=1)]
    ab = like.noise_values(X)
    assert ab.shape == (len(X), 3, 2) and np.all(np.isnan(ab[:, 1])) and np.all(ab[:, 2, 0] == 0.4)
    own = (lambda i: 10.0 ** X[:, i]) if like.log10 else (lambda i: X[:, i])
    assert np.all(_ulps(ab[:, 0, 0], own(P)) <= 4) and np.all(_ulps(ab[:, 2, 1], own(P + 1)) <= 4)
    assert np.all(_ulps(ab[:, 0, 1], mono.value(X)) <= 4)
    assert np.all(NN.like(net, [Noise(P), None, None]).noise_values(X)[:, 0, 1] == 0.0)        # b is 0 without rel
    assert np.all(np.isnan(NN.like(net, None).noise_values(X)))


# ---------------------------------------------------------------------------------------------------- construction, pickle and cache
def test_construction_errors():
    for args, kw, text in [((-1,), {}, "negative"), (("a",), {}, "a Noise's sigma is"), ((0.0,), {}, "fixed sigma"), ((-1.0,), {}, "fixed sigma"),
                           ((np.inf,), {}, "fixed sigma"), ((1.0,), dict(rel=-0.5), "fixed rel"), ((1.0,), dict(rel=np.nan), "fixed rel"),
                           ((1.0,), dict(rel="b"), "a Noise's rel is"), ((1.0,), dict(dist="student"), "dist"), ((1.0,), dict(scale="log10"), "scale"),
                           ((1.0,), dict(rel=0.1, scale="log"), "takes no rel")]:
        with pytest.raises(ValueError, match=text):
            Noise(*args, **kw)
    z = Noise(3, rel=Monomial({4: 1}), dist="laplace")
    assert z == Noise(3, Monomial({4: 1}), "laplace", "lin") and hash(z) == hash(Noise(3, Monomial({4: 1}), "laplace"))
    assert z != Noise(3.0, Monomial({4: 1}), "laplace") and Noise(1) != Noise(1.0) and Noise(1.0, rel=0.0) != Noise(1.0)
    assert "Noise(3, Monomial({4: 1.0}, 0.0), 'laplace', 'lin')" == repr(z)
    with pytest.raises(AttributeError):
        z.sigma = 1
    with pytest.raises(AttributeError):
        del z.rel
    data = [0.1, 0.2, 0.3]
    for noise, text in [([Noise(3), None], "O = 1 entries"), ([], "O = 1 entries"), (Noise(3), "sequence of O entries"), ([0.1], "sequence of O entries"),
                        (3, "sequence of O entries")]:
        with pytest.raises(ValueError, match=text):
            _robertson(noise, data, sd=1.0)
    with pytest.raises(ValueError, match='must be > 0 where observed: its Noise has scale "log"'):
        _robertson([Noise(3, scale="log")], [0.0, 0.2, 0.3])
    with pytest.raises(ValueError, match='must be > 0 where observed: its Noise has scale "log"'):
        _robertson([Noise(3, scale="log")], [0.1, -0.2, 0.3])
    with pytest.raises(ValueError, match='condition 1: data of observable 0 must be > 0'):
        _robertson([Noise(3, scale="log")], data, conditions=[{}, dict(data=[[0.1, 0.2, -0.3]])])
    with pytest.raises(ValueError, match="y0, data and sd may be None"):           # sd=None needs a Noise on every observable
        MassActionODELogLike(3, ROB.REACTIONS, ROB.Y0, T_ZERO, np.eye(3)[1:], np.ones((2, 3)), None, noise=[Noise(3), None])
    with pytest.raises(ValueError, match="parameter index 4 is not < ndim = 4"):
        _robertson([Noise(3, rel=4)], data, ndim=4)
    assert _robertson([Noise(3, rel=Monomial({6: 1}))], data).d == 7 and _robertson([Noise(0.1)], data).d == 3
    assert np.all(_robertson([Noise(3)], data).sd == 1.0)                         # sd=None: a weight of 1


def test_pickle_and_objects_from_before_the_keyword():
    x = np.r_[ROB.NOMINAL, -1.0, -1.5]
    like = _robertson([Noise(3, rel=4, dist="laplace")], [np.nan, 0.2, 0.3], sd=0.5)
    copy = pickle.loads(pickle.dumps(like))
    assert copy.noise == like.noise and copy.source() == like.source() and copy(x) == like(x)
    assert pickle.loads(pickle.dumps(Noise(3, Monomial({4: -1}), "laplace"))) == Noise(3, Monomial({4: -1}), "laplace")
    plain = _robertson(None, [np.nan, 0.2, 0.3], sd=0.5)
    state = plain.__getstate__()
    del state["noise"]                                                            # an object pickled before Noise existed
    old = MassActionODELogLike.__new__(MassActionODELogLike)
    old.__dict__.update(state)
    assert old.noise is None and old.source() == plain.source() and old(x) == plain(x) and np.all(np.isnan(old.noise_values(x)))


def test_no_noise_generates_what_it_always_did():
    data = [np.nan, 0.2, 0.3]
    a, b = _robertson(None, data, sd=0.5), _robertson([None], data, sd=0.5)
    assert b.noise is None and a.source() == b.source() and a.data_block().tobytes() == b.data_block().tobytes()
    assert "NOISE" not in a.source() and "NOISE = true;" in _robertson([Noise(3)], data).source()


# ---------------------------------------------------------------------------------------------------- the cross-compilation for gfx950
@pytest.fixture(scope="module")
def code_objects():
    """name -> (notes with a Noise on every observable, notes of the same network with noise=None)"""
    out = {}
    for name in NN.NETWORKS:
        net = NN.network(name)
        out[name] = tuple(notes(NN.like(net, noise).code_object()) for noise in (NN.cases(net.P)["all_three"], None))
    return out


def test_every_shape_compiles_for_gfx950_with_a_noise_on_every_observable(code_objects):
    for name, (noisy, plain) in code_objects.items():
        print("%-8s with noise %s, without %s" % (name, noisy, plain))
        assert noisy["vgpr"] > 0
    for name in ("one3", "group16"):                                              # the noise values cost no scratch
        noisy, plain = code_objects[name]
        assert noisy["scratch"] <= plain["scratch"]
    O2 = 2 * 3                                                                    # the 2 O values in the point's row of LDS: 256 / L rows
    for name, rows in (("group16", 16), ("group32", 8), ("wave64", 4)):
        noisy, plain = code_objects[name]
        assert noisy["lds"] == plain["lds"] + rows * O2 * 8
