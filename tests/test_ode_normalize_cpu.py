"""NORMALISED READOUTS, MassActionODELogLike(normalize=[...]), on the host build (csrc/dz_ode.h's head): the term against an independent
longdouble evaluation from the un-normalised twin's trajectories, within the first-order rounding bound of the expanded form; the
normalised trajectories against scipy's Radau, within the twin's own error times the quotient's condition; and the exact properties
-- powers of two in `scale`, "max" against "ref" on a monotone readout, a condition's term against the object of that condition alone
(views included), a trajectory that is identically zero, with_outputs, the untouched object behind normalize=None, pickling and the
refusals."""
import pickle

import numpy as np
import pytest

from pydream_amd.likelihoods import MassActionODELogLike, Monomial, Noise, Normalize

from . import ode_networks as NW
from . import ode_normalize_networks as NN
from . import ode_normalize_reference as NR

INF = np.inf
X = NN.mm_points()


# ---------------------------------------------------------------- 1. against an independent evaluation
@pytest.mark.parametrize("steady", [False, True])
@pytest.mark.parametrize("noisy", [False, True])
@pytest.mark.parametrize("kind", NN.KINDS)
def test_the_term_equals_the_direct_longdouble_sum_within_the_rounding_bound(kind, noisy, steady):
    """the three kinds, with and without Noise(sigma), one NaN entry throughout; steady: t = [..., inf] and the product's "ref" at the
    steady row.  Measured on the host build, worst |term - reference| / bound over the 259 points: at most 0.02 in all twelve cases."""
    norm = NN.mm_normalize(kind, steady)
    like, twin = NN.mm(norm, steady=steady, noisy=noisy), NN.mm_twin(norm, steady=steady, noisy=noisy)
    pts = NN.with_sigma(X) if noisy else X
    got, sim = like.batch(pts), twin.simulate(pts)
    assert np.all(np.isfinite(got)) and np.all(np.isfinite(sim)) and np.isnan(like.data).sum() == 1
    sigma = like.noise_values(pts)[:, 0, 0] if noisy else None
    value, bound = NR.terms(sim, norm, like.t, like.data, like.sd, sigma)
    ratio = np.abs(got.astype(np.longdouble) - value) / bound
    print("%s noisy=%s steady=%s: worst |term - reference| / bound = %.3g" % (kind, noisy, steady, float(np.max(ratio))))
    assert np.all(ratio <= 1.0)


# ---------------------------------------------------------------- 2. against Radau
def test_normalised_trajectories_against_radau_within_the_twins_error_times_the_condition():
    """Per point and observable, with E = max_j |m_j - r_j| the twin's own error against Radau (r): for "max" and "ref"
    |m / g - r / g_r| = |(m - r) g_r + r (g_r - g)| / (g g_r) <= (E / g) (1 + |r'|), since a maximum and a row are 1-Lipschitz in the
    trajectory; for "minmax" numerator and range move by 2 E each: (2 E / g) (1 + |r'|).  1 + max |r'| is the quotient's condition
    number max |m| / g (plus one) from the reference.  Four ulp of |m'| for the division itself."""
    worst = {}
    refs = np.array([NW.radau(4, NW.MM_REACTIONS, NW.MM_Y0, NW.MM_T, x)[:, [1, 3]] for x in X])      # [n, T, O], once for the three kinds
    m = NN.mm_twin(None).simulate(X)
    E = np.max(np.abs(m - refs), axis=1)                                  # [n, O]
    for kind in NN.KINDS:
        norm = NN.mm_normalize(kind)
        sim = NN.mm(norm).simulate(X)
        for q, z in enumerate(norm):
            r = NN.normalized(refs[:, :, q], z, NW.MM_T)
            mq = m[:, :, q]                 # (g from the twin's trajectory: existing code)
            g = np.max(mq, axis=1) if kind == "max" else np.ptp(mq, axis=1) if kind == "minmax" else mq[:, int(np.flatnonzero(NW.MM_T == z.t)[0])]
            tol = (2.0 if kind == "minmax" else 1.0) * E[:, q] / g * (1.0 + np.max(np.abs(r), axis=1)) + 4 * 2.0 ** -52 * np.max(np.abs(r), axis=1)
            err = np.max(np.abs(sim[:, :, q] - r), axis=1)
            worst[kind, q] = float(np.max(err / tol))
            assert np.all(err <= tol), (kind, q, worst[kind, q])
    print("worst normalised error / (twin's error x condition): " + ", ".join("%s[%d] %.3f" % (k, q, v) for (k, q), v in worst.items()))
    print("twin's own worst error against Radau: %.3g" % float(np.max(E)))


# ---------------------------------------------------------------- 3. exact properties
@pytest.mark.parametrize("kind", NN.KINDS)
def test_powers_of_two_in_scale_give_the_bits_of_no_scale(kind):
    norm = NN.mm_normalize(kind)
    plain, scaled = NN.mm(norm), NN.mm(norm, scale=[4.0, 0.25])
    assert "scale" in scaled.source() and plain.batch(X).tobytes() == scaled.batch(X).tobytes()
    assert plain.simulate(X).tobytes() == scaled.simulate(X).tobytes()


def test_max_on_the_monotone_product_equals_ref_at_the_last_time():
    a = NN.mm([None, Normalize("max")], data_like=[None, Normalize("max")])
    b = NN.mm([None, Normalize("ref", 10.0)], data_like=[None, Normalize("max")])
    assert a.source() != b.source() and a.batch(X).tobytes() == b.batch(X).tobytes() and a.simulate(X).tobytes() == b.simulate(X).tobytes()
    # (the substrate, not normalised, keeps the twin's bits)
    assert a.simulate(X)[:, :, 0].tobytes() == NN.mm_twin(None).simulate(X)[:, :, 0].tobytes()


@pytest.mark.parametrize("kind", NN.KINDS)
def test_a_conditions_term_equals_the_object_of_that_condition_alone(kind):
    norm = NN.mm_normalize(kind)
    multi, one = NN.mm_conditions(norm, y0s=NN.MM_CONDITION_Y0[:2])
    terms, sim = multi.batch_conditions(X), multi.simulate(X)
    for c in range(2):
        assert terms[:, c].tobytes() == one(c).batch(X).tobytes() and np.ascontiguousarray(sim[:, c]).tobytes() == one(c).simulate(X).tobytes()
    assert multi.batch(X).tobytes() == (terms[:, 0] + terms[:, 1]).tobytes() and np.all(np.isfinite(terms))


def test_a_viewed_conditions_term_equals_the_single_object_at_the_viewed_row():
    """condition 1 reads the catalytic rate at a fixed value, with Noise(sigma) on the product: the record sits in front of the pairs"""
    norm, noise = NN.mm_normalize("minmax"), [None, Noise(NN.MM_SIGMA)]
    multi, one = NN.mm_conditions(norm, y0s=NN.MM_CONDITION_Y0[:2], params={1: {2: 0.3}}, noise=noise)
    pts = NN.with_sigma(X)
    assert "VIEW = 4" in multi.source() and "VIEW" not in one(1).source()
    terms, sim = multi.batch_conditions(pts), multi.simulate(pts)
    for c in range(2):
        rows = np.ascontiguousarray(multi.viewed(pts, c))
        assert terms[:, c].tobytes() == one(c).batch(rows).tobytes() and np.ascontiguousarray(sim[:, c]).tobytes() == one(c).simulate(rows).tobytes()
    assert np.all(np.isfinite(terms)) and not np.array_equal(terms[:, 1], one(1).batch(pts))


def test_a_trajectory_that_is_identically_zero_fails_its_condition_alone():
    """without enzyme the product stays 0: g = 0, the item is -inf and its slice NaN; the other conditions of the point stay finite"""
    multi, one = NN.mm_conditions(NN.mm_normalize("max"))
    terms, sim = multi.batch_conditions(X), multi.simulate(X)
    assert np.all(terms[:, 2] == -INF) and np.all(np.isnan(sim[:, 2])) and np.all(np.isfinite(terms[:, :2])) and np.all(np.isfinite(sim[:, :2]))
    assert np.all(multi.batch(X) == -INF) and np.all(one(2).batch(X) == -INF)
    # (the un-normalised twin integrates that condition: the failure is the normaliser's)
    twin, _ = NN.mm_conditions(None)
    assert np.all(twin.simulate(X)[:, 2, :, 1] == 0.0) and np.all(np.isfinite(twin.batch_conditions(X)[:, 2]))


@pytest.mark.parametrize("kind", NN.KINDS)
def test_with_outputs_on_the_objects_own_times_simulates_the_same_bytes(kind):
    like = NN.mm(NN.mm_normalize(kind))
    again = like.with_outputs(like.t)
    assert again.normalize == like.normalize and again.simulate(X[:40]).tobytes() == like.simulate(X[:40]).tobytes()
    dense = like.with_outputs(np.linspace(0.5, 10.0, 77))
    assert np.all(np.isfinite(dense.simulate(X[:5])))
    if kind == "ref":
        with pytest.raises(ValueError, match="reference time"):
            like.with_outputs(np.linspace(0.25, 9.75, 20))
    else:                                   # (the maximum over a denser grid is another number: at least as large)
        assert np.all(np.nanmax(dense.simulate(X[:5])[:, :, 1], axis=1) == 1.0)


def test_all_nones_is_the_object_it_always_was():
    plain, nones = NW.michaelis_menten(), NW.michaelis_menten(normalize=[None, None])
    assert nones.normalize is None and plain.source() == nones.source() and plain.data_block().tobytes() == nones.data_block().tobytes()
    assert plain._unit() == nones._unit() and "NORMALIZE" not in plain.source()
    like = NN.mm(NN.mm_normalize("max"))
    assert "NORMALIZE = 2" in like.source() and len(like.data_block()) == len(NN.mm_twin(None).data_block()) + 14
    # (only what a kind needs: 2 sums + 1 value, 3 sums + 2 values)
    assert "NORM_ACC = 6" in like.source() and "NORM_ACC = 10" in NN.mm(NN.mm_normalize("minmax")).source()
    old = MassActionODELogLike.__new__(MassActionODELogLike)               # (an object pickled before the keyword existed)
    old.__dict__.update({k: v for k, v in plain.__dict__.items() if k != "normalize"})
    assert old.normalize is None and old.source() == plain.source() and old.data_block().tobytes() == plain.data_block().tobytes()


def test_the_record_sits_behind_the_knots_and_in_front_of_the_pairs():
    norm = NN.mm_normalize("ref")
    multi, _ = NN.mm_conditions(norm, y0s=NN.MM_CONDITION_Y0[:2], params={1: {2: 0.3}})
    blk = multi.condition_block(1)
    P = 3
    rec = blk[-2 * P - 14:-2 * P]
    assert rec[0] == 2.0 and rec[1] == 0.0 and rec[7] == 2.0 and rec[8] == len(NW.MM_T) - 1 and rec[5] == 19 and rec[12] == 20
    assert blk[-2 * P:].tolist() == [0.0, 0.0, 1.0, 0.0, -1.0, 0.3]


def test_pickling_and_the_value_class():
    like = NN.mm(NN.mm_normalize("ref"), noisy=True)
    again = pickle.loads(pickle.dumps(like))
    pts = NN.with_sigma(X[:30])
    assert again.normalize == like.normalize and again.batch(pts).tobytes() == like.batch(pts).tobytes()
    z = Normalize("ref", INF)
    assert pickle.loads(pickle.dumps(z)) == z and repr(z) == "Normalize('ref', inf)" and z != Normalize("ref", 1.0) and hash(z) == hash(Normalize("ref", INF))
    assert Normalize("max") == Normalize("max") and Normalize("max") != Normalize("minmax") and repr(Normalize("max")) == "Normalize('max', None)"
    with pytest.raises(AttributeError):
        z.kind = "max"
    from pydream_amd import likelihoods
    assert likelihoods.Normalize is Normalize


@pytest.mark.parametrize("bad", [dict(kind="mean"), dict(kind="ref"), dict(kind="ref", t=np.nan), dict(kind="max", t=1.0), dict(kind="ref", t=True)])
def test_a_normalize_that_is_no_value_is_refused(bad):
    with pytest.raises(ValueError, match="Normalize"):
        Normalize(**bad)


@pytest.mark.parametrize("noise,word", [(Noise(3, rel=0.1), "rel"), (Noise(3, dist="laplace"), "laplace"), (Noise(3, scale="log"), "log")])
def test_a_noise_that_is_no_quadratic_form_is_refused_on_a_normalised_observable(noise, word):
    with pytest.raises(ValueError, match="normalised.*Noise\\(sigma\\)") as err:
        NW.michaelis_menten(normalize=[None, Normalize("max")], noise=[None, noise])
    assert word in str(err.value)
    NW.michaelis_menten(normalize=[Normalize("max"), None], noise=[None, Noise(3, rel=0.1)])        # (on another observable: fine)


def test_the_other_refusals():
    with pytest.raises(ValueError, match="O = 2 entries"):
        NW.michaelis_menten(normalize=[Normalize("max")])
    with pytest.raises(ValueError, match="O = 2 entries"):
        NW.michaelis_menten(normalize=Normalize("max"))
    with pytest.raises(ValueError, match="O = 2 entries"):
        NW.michaelis_menten(normalize=["max", None])
    with pytest.raises(ValueError, match="reference time 0.75 is not one of the output times"):
        NW.michaelis_menten(normalize=[Normalize("ref", 0.75), None])
    with pytest.raises(ValueError, match="reference time inf"):
        NW.michaelis_menten(normalize=[Normalize("ref", INF), None])
    with pytest.raises(ValueError, match='must be a mapping with the keys'):
        MassActionODELogLike(4, NW.MM_REACTIONS, None, NW.MM_T, NN.MM_OBS, None, None,
                             conditions=[dict(NN.mm_experiment(None), normalize=[Normalize("max"), None])])


def test_noise_terms_holds_nothing_for_a_normalised_observable():
    like = NN.mm([None, Normalize("max")], data_like=[None, Normalize("max")], noise=[Noise(3), Noise(3)])
    body = like.source().split("noise_terms")[1].split("norm_init")[0]
    assert "o[0]" in body and "o[1]" not in body and "nz[2]" in like.source().split("norm_finish")[1]
    mono = NN.mm([Normalize("max"), None], data_like=[Normalize("max"), None], scale=[Monomial({3: 1.0}), 1.0])
    pts = NN.with_sigma(X[:50], 0.0, 1.0)
    # (a sampled scale factor cancels in the quotient up to rounding: what the keyword is for)
    np.testing.assert_allclose(mono.simulate(pts)[:, :, 0], NN.mm([Normalize("max"), None], data_like=[Normalize("max"), None]).simulate(pts)[:, :, 0], rtol=1e-14)
