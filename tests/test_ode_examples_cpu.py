"""The shipped ODE examples that combine features -- washout (events, a Monomial scale, 4 conditions), binding_cycle (Monomial rates, a
Monomial start, a scale, a constraint, 9 conditions), dose_response (6 conditions, data made by the solver itself) -- and the combination
no other test builds, events together with Monomials (ode_monomial_networks' *_events specs), without a GPU: the host build's value
against a likelihood made of scipy alone (ode_monomial_networks.reference_loglike: Radau restarted at every event, norm.logpdf), every
condition's term against the single-experiment object bit for bit, and the cross-compilation for gfx950 without scratch.

The bound is that of test_ode_monomials_cpu.test_the_value_agrees_with_an_independent_radau_likelihood, |value - reference| <= 1e-6
sum |terms|; the references of all points are computed once per model, in a process pool."""
import functools
import multiprocessing
import os
from concurrent.futures import ProcessPoolExecutor

import numpy as np
import pytest

from pydream_amd.examples.binding_cycle import binding_cycle_device as BC
from pydream_amd.examples.dose_response import dose_response_device as DR
from pydream_amd.examples.washout import washout_device as WO
from pydream_amd.likelihoods import Monomial

from . import ode_condition_networks as CN
from . import ode_monomial_networks as MN
from . import ode_networks as NW
from .ode_support import notes

BOUND = 1e-6


def _pool():
    return ProcessPoolExecutor(max(1, min(8, len(os.sched_getaffinity(0)))), mp_context=multiprocessing.get_context("fork"))


def _reference(args):
    return MN.reference_loglike(*args)


def example_spec(name):
    """(spec, data, sd) of a shipped example in ode_monomial_networks' form, from the example module's own constants (never from the
    generated code); the data are the example's (scipy's Radau for washout and binding_cycle, the solver under test for dose_response)"""
    if name == "washout":
        like = WO.make_likelihood()
        spec = dict(S=3, reactions=WO.REACTIONS, y0=[WO.start_amounts(dose) for dose in WO.DOSES], t=WO.TSPAN, obs=WO.OBSERVABLES,
                    scale=[Monomial({WO.SCALE: 1})], constraints=[], events=[list(WO.WASHOUT)] * len(WO.DOSES), nominal=WO.NOMINAL)
    elif name == "binding_cycle":
        like = BC.make_likelihood()
        spec = dict(S=7, reactions=BC.REACTIONS, y0=[BC.start_amounts(a, b) for a, b in BC.DOSES], t=BC.TSPAN, obs=BC.OBSERVABLES,
                    scale=[Monomial({BC.SCALE: 1})], constraints=[BC.CYCLE], nominal=BC.NOMINAL)
    else:
        like = DR.make_likelihood()
        spec = dict(S=6, reactions=DR.REACTIONS, y0=[DR.start_amounts(s) for s in DR.DOSES], t=DR.TSPAN, obs=DR.OBSERVABLES, scale=None,
                    constraints=[], nominal=DR.NOMINAL)
    data, sd = np.stack([c["data"] for c in like.conditions]), np.stack([c["sd"] for c in like.conditions])
    return like, spec, data, sd


@functools.lru_cache(maxsize=None)
def references(name, n, seed, width):
    """(points, [(reference value, sum |terms|)]) of a model at n box points around its nominal values: once, shared, not to be written to"""
    spec, data, sd = example_spec(name)[1:] if name in ("washout", "binding_cycle", "dose_response") else MN.spec_and_data(name)
    X = NW.box_points(spec["nominal"], n, seed, width=width)
    with _pool() as ex:
        refs = list(ex.map(_reference, [(spec, data, sd, x) for x in X]))
    X.setflags(write=False)
    return X, refs


def _assert_within_bound(name, got, refs):
    assert np.all(np.isfinite(got))
    worst = 0.0
    for value, (total, magnitude) in zip(got, refs):
        worst = max(worst, abs(value - total) / magnitude)
        assert abs(value - total) <= BOUND * magnitude, (name, value, total, magnitude)
    print("%s: largest |value - reference| / sum |terms| = %.3g, largest |value| %.3g" % (name, worst, np.max(np.abs(got))))


def _assert_terms_are_the_single_experiments(like, single, X):
    """column c of batch_conditions == the single-experiment object of condition c (the constraints with condition 0), bit for bit, and
    batch their sum from left to right"""
    terms = like.batch_conditions(X)
    for c in range(len(like.conditions)):
        assert terms[:, c].tobytes() == single(c).batch(X).tobytes(), c
    assert like.batch(X).tobytes() == CN.left_to_right(terms).tobytes()


# ---------------------------------------------------------------------------------------------------- the shipped examples
@pytest.mark.parametrize("name,width", [("washout", 0.5), ("binding_cycle", 0.3), ("dose_response", 0.5)])
def test_a_shipped_example_agrees_with_an_independent_radau_likelihood(name, width):
    like, spec, data, sd = example_spec(name)
    X, refs = references(name, 10, 41, width)
    _assert_within_bound(name, like.batch(X), refs)
    assert len(like.conditions) == len(spec["y0"]) == {"washout": 4, "binding_cycle": 9, "dose_response": 6}[name]
    assert ("EVENTS = 1" in like.source()) == (name == "washout") and ("MONOMIALS" in like.source()) == (name != "dose_response")


@pytest.mark.parametrize("name", ["washout", "binding_cycle"])
def test_a_shipped_examples_terms_are_its_single_experiments(name):
    from pydream_amd.likelihoods import MassActionODELogLike
    like, spec, data, sd = example_spec(name)

    def single(c):
        return MassActionODELogLike(spec["S"], spec["reactions"], spec["y0"][c], spec["t"], spec["obs"], data[c], sd[c], scale=spec["scale"],
                                    constraints=spec["constraints"] if c == 0 and spec["constraints"] else None,
                                    events=list(spec["events"][c]) if spec.get("events") else None)
    _assert_terms_are_the_single_experiments(like, single, NW.box_points(spec["nominal"], 40, 42, width=0.5, outside=0.05))


def test_dose_response_data_are_radaus():
    """dose_response.simulated_data comes from the solver under test at rtol 1e-12: against Radau (rtol 1e-12, atol 1e-14) within ten
    tolerances of 1e-9 -- the criterion of test_host_build_is_accurate_against_radau_and_error_shrinks_with_tolerance at the tightest
    tolerance that test verifies; the data are made at a tighter one"""
    _, spec, data, _ = example_spec("dose_response")
    for c in range(len(DR.DOSES)):
        ref = MN.radau_observed(spec, c, DR.NOMINAL)
        err = float(np.max(np.abs(data[c] - ref) / (1e-9 * np.abs(ref) + 1e-9)))
        print("dose %g: %.3g tolerances of 1e-9" % (DR.DOSES[c], err))
        assert err < 10


# ---------------------------------------------------------------------------------------------------- events with Monomials
@pytest.mark.parametrize("lanes", [1, 16])
def test_events_with_monomials_agree_with_an_independent_radau_likelihood(lanes):
    """mm_kd with an event at t0 on the species whose start is a Monomial, one on an output time (whose reading is the NaN datum), one
    between two outputs and a condition without events (a padded block), in both shapes at rtol = atol = 1e-9"""
    like, single = MN.build("mm_kd_events", lanes_per_point=lanes, rtol=1e-9, atol=1e-9)
    spec, data, _ = MN.spec_and_data("mm_kd_events")
    assert like.lanes_per_point == lanes and "EVENTS = 2" in like.source() and "MONOMIALS" in like.source()
    assert [len(c["events"]) for c in like.conditions] == [2, 1, 0]
    j = int(np.flatnonzero(spec["t"] == spec["events"][1][0][0])[0])
    assert np.isnan(data[1, 0, j]) and np.isnan(data).sum() == 1 and spec["events"][0][0][:2] == (0.0, 0) and isinstance(spec["y0"][0][0], Monomial)
    X, refs = references("mm_kd_events", 10, 43, 1.0)
    _assert_within_bound("mm_kd_events @%d" % lanes, like.batch(X), refs)
    _assert_terms_are_the_single_experiments(like, lambda c: single(c, constraints=c == 0, rtol=1e-9, atol=1e-9, lanes_per_point=lanes),
                                             NW.box_points(spec["nominal"], 40, 44, width=1.0, outside=0.05))


@pytest.mark.parametrize("name", ["enzyme13_m_events", "chain17_m_events"])
def test_group_networks_with_events_and_monomials_equal_their_single_experiments(name):
    like, single = MN.build(name)
    spec = MN.spec_and_data(name)[0]
    assert like.lanes_per_point == spec["lanes"] and "EVENTS" in like.source() and "MONOMIALS" in like.source()
    _assert_terms_are_the_single_experiments(like, lambda c: single(c, constraints=c == 0), NW.box_points(spec["nominal"], 12, 45, width=0.5))


# ---------------------------------------------------------------------------------------------------- the device build
@pytest.mark.parametrize("model", ["mm_kd_events", "enzyme13_m_events", "chain17_m_events", "washout", "binding_cycle"])
def test_the_combinations_cross_compile_for_gfx950_without_scratch(model):
    if model in ("washout", "binding_cycle"):
        like, plain = example_spec(model)[0], None
    else:
        like, plain = MN.build(model)[0], MN.build(model[:-len("_events")])[0]
    a = notes(like.code_object())
    print("%s: %d VGPRs, %d AGPRs, scratch %d" % (model, a["vgpr"], a["agpr"], a["scratch"]))
    assert a["scratch"] == 0
    if plain is not None:
        assert "EVENTS" not in plain.source() and a["scratch"] <= notes(plain.code_object())["scratch"]
