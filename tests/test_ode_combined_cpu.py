"""The features of MassActionODELogLike TOGETHER, without a GPU: on the seeded networks of tests/ode_combined_networks.py -- conditions,
Monomials, events, equilibrate, RateLaw/Hill, Noise and Input in one object, in the four builds -- the host build's trajectories are
held to scipy's Radau restarted at every knot and event (tests/ode_combined_reference.py), its likelihood to the definition in 40-digit
mpmath, dead coordinates kill the whole point whoever reads them, the docstring's bit identities hold (a condition is its single
experiment, batch is the left-to-right sum, with_outputs of the own times, a feature removed is the object without the keyword), and the
likelihood and prediction units cross-compile for gfx950 with exactly the LDS row the header describes."""
import multiprocessing
import os
from concurrent.futures import ProcessPoolExecutor

import numpy as np
import pytest

from pydream_amd.likelihoods import _hill_slots

from . import ode_combined_networks as CB
from . import ode_combined_reference as CR
from . import ode_condition_networks as CN
from . import ode_noise_reference as NR
from .ode_support import max_rel_err, notes

ALL = list(range(len(CB.CASES)))
IDS = [CB.case(i).name for i in ALL]
FULL_IDS = [CB.case(i).name for i in CB.FULL]


def _trajectory_points(c):
    """3 points of the nominal +-0.5 box (2 at S >= 60, where a reference trajectory takes minutes)"""
    return c.points(2 if c.S >= 60 else 3, 1)


@pytest.fixture(scope="module")
def references(request):
    """{case index: [the reference's observables [C, T, O] per point]} for the cases whose trajectory test is selected in this run: their
    Radau runs in one process pool, the long ones first"""
    wanted = sorted({item.callspec.params["i"] for item in request.session.items
                     if getattr(item, "originalname", "") == "test_host_build_of_the_combination_is_accurate_against_radau" and hasattr(item, "callspec")})
    jobs = sorted(((i, j, x) for i in wanted for j, x in enumerate(_trajectory_points(CB.case(i)))), key=lambda job: -CB.case(job[0]).S)
    with ProcessPoolExecutor(max(1, min(8, len(os.sched_getaffinity(0)))), mp_context=multiprocessing.get_context("fork")) as ex:
        done = list(ex.map(CR.observed, [(CB.case(i), x) for i, _, x in jobs]))
    out = {i: [None] * len(_trajectory_points(CB.case(i))) for i in wanted}
    for (i, j, _), ref in zip(jobs, done):
        out[i][j] = ref
    return out


# ---------------------------------------------------------------------------------------------------- accuracy
@pytest.mark.parametrize("i", ALL, ids=IDS)
def test_host_build_of_the_combination_is_accurate_against_radau(i, references):
    """max |sim - ref| / (rtol |ref| + rtol) < 10 at rtol = atol = 1e-6 and 1e-9, the bound and the tolerances of test_ode_events_cpu,
    test_ode_inputs_cpu and test_ode_equilibrate_cpu.  The ratio of every case is printed; EXPERIMENTS.md keeps what was measured."""
    c = CB.case(i)
    X = _trajectory_points(c)
    errs = []
    for rtol in (1e-6, 1e-9):
        like = c.like(rtol=rtol, atol=rtol, max_steps=20000, equilibrate=dict(max_steps=20000))
        assert like.lanes_per_point == c.lanes and len(like.conditions) == 3
        errs.append(max_rel_err(like, references[i], X, rtol))
    print("%s: max |sim - ref| / (rtol |ref| + rtol) at rtol 1e-6, 1e-9: %.3g %.3g" % (c.name, errs[0], errs[1]))
    assert all(e < 10 for e in errs)


@pytest.mark.parametrize("i", ALL, ids=IDS)
def test_likelihood_of_the_combination_is_the_definition_and_dead_coordinates_kill_the_point(i):
    """|host - reference| <= ode_noise_reference.tolerance(A, N) for every condition's term and for the sum, on 24 points of the box and
    a margin outside it; the same rows are finite on both sides.  The dead rows (Case.dead_rows: a coordinate spoilt for one reader
    alone) are -inf from batch and in every column of batch_conditions.  The largest ratio of every case is printed; EXPERIMENTS.md keeps
    what was measured."""
    c = CB.case(i)
    like = c.like()
    dead = c.dead_rows()
    X = np.vstack([c.points(24, 2, outside=0.05)] + [x for _, x in dead])
    n = len(X) - len(dead)
    host, terms, sims = like.batch(X), like.batch_conditions(X), like.simulate(X)
    for (why, _), value, row in zip(dead, host[n:], terms[n:]):
        assert value == -np.inf and np.all(row == -np.inf), (c.name, why, value, row)
    assert np.all(np.isnan(sims[n:]))
    ref_terms, ref_total, A, N = CR.loglike(like, c, X[:n], sims[:n])
    live = np.isfinite(ref_total)
    assert live.sum() >= n // 2 and np.array_equal(live, np.isfinite(host[:n])) and np.array_equal(np.isfinite(terms[:n]).all(axis=1), live)
    worst = 0.0
    for c_ in range(3):
        worst = max(worst, float(np.max(np.abs(terms[:n][live, c_] - ref_terms[live, c_]) / NR.tolerance(A[live, c_], N[live, c_]))))
    worst_total = float(np.max(np.abs(host[:n][live] - ref_total[live]) / NR.tolerance(A[live].sum(axis=1), N[live].sum(axis=1))))
    print("%s: |host - reference| / tolerance: terms %.3g, sum %.3g (%d of %d rows live)" % (c.name, worst, worst_total, live.sum(), n))
    assert worst <= 1.0 and worst_total <= 1.0


# ---------------------------------------------------------------------------------------------------- the docstring's identities
@pytest.mark.parametrize("i", CB.FULL, ids=FULL_IDS)
def test_a_condition_of_the_combination_is_its_single_experiment_and_batch_is_the_sum(i):
    """batch_conditions(X)[:, c] and simulate(X)[:, c] have the bits of the single-experiment object of condition c (the constraints on
    condition 0 only), dead rows included -- but for one row: condition 1 knocks out the species whose y0 is a Monomial, so its
    single-experiment object has no such Monomial and does not read that coordinate, while in the object of all conditions the spoilt
    coordinate kills the point in every condition."""
    c = CB.case(i)
    like = c.like()
    dead = c.dead_rows()
    X = np.vstack([c.points(12, 3, outside=0.05)] + [x for _, x in dead])
    own = {k: np.array([True] * 12 + [not (k == 1 and why == "y0 Monomial") for why, _ in dead]) for k in range(3)}
    terms, sims = like.batch_conditions(X), like.simulate(X)
    assert np.any(np.isfinite(terms)) and [len(like._input_knots(e["inputs"])) for e in like._experiments()] == [1 + len(c.U[1:]) * 2, 2 + len(c.U[1:]) * 2, 5 + len(c.U[1:]) * 2]
    for k in range(3):
        one = c.single(k)
        assert (one.constraints != ()) == (k == 0)
        assert terms[own[k], k].tobytes() == one.batch(X)[own[k]].tobytes(), (c.name, k)
        assert np.ascontiguousarray(sims[own[k], k]).tobytes() == one.simulate(X)[own[k]].tobytes(), (c.name, k)
        assert np.all(terms[~own[k], k] == -np.inf) and np.all(np.isfinite(one.batch(X)[~own[k]]))
    assert like.batch(X).tobytes() == CN.left_to_right(terms).tobytes()
    again = like.with_outputs(like.t)
    assert again.simulate(X).tobytes() == sims.tobytes()


@pytest.mark.parametrize("i", CB.FULL, ids=FULL_IDS)
def test_a_feature_removed_from_the_combination_is_the_object_without_the_keyword(i):
    """noise=[None] * O, inputs=[] and events=[] against the keyword not passed (and None): the same source, data block, cache key of the
    code object and bits"""
    c = CB.case(i)
    X = c.points(8, 4)
    O = len(c.observables)

    def same(a, b):
        assert a.source() == b.source() and a.data_block().tobytes() == b.data_block().tobytes() and a._unit() == b._unit()
        value = a.batch(X)
        assert value.tobytes() == b.batch(X).tobytes() and a.simulate(X).tobytes() == b.simulate(X).tobytes() and np.any(np.isfinite(value))

    without = c.like(noise=CB.OMIT)
    assert "NOISE" not in without.source() and "NOISE" in c.like().source()
    same(c.like(noise=[None] * O), without)
    plain = c.like(plain_species=True, inputs=CB.OMIT)
    assert "INPUTS" not in plain.source() and "INPUTS" in c.like().source()
    same(c.like(plain_species=True, inputs=[]), plain)
    same(c.like(plain_species=True, inputs=None), plain)
    quiet = c.single(0, events=CB.OMIT)
    assert "EVENTS" not in quiet.source() and "EVENTS" in c.single(2).source()
    same(c.single(0, events=[]), quiet)
    same(c.single(0, events=None), quiet)


# ---------------------------------------------------------------------------------------------------- failures
@pytest.mark.parametrize("lanes", [1, 16, 32, 64])
def test_starved_step_limits_fail_a_mix_of_conditions_and_phases(lanes):
    """The limits the GPU file runs (CB.STARVED), chosen here on the host build: some points of the GPU test's batch fail in every
    condition, some in a few, some in none; the PHASE of condition 0 fails for some points (steady_state is NaN) while for others every
    phase passes and an experiment fails.  At the default limits nothing fails."""
    c, X = CB.starved_case(lanes), CB.starved_points(lanes)
    max_steps, phase_steps = CB.STARVED[lanes]
    assert np.all(np.isfinite(c.like().batch_conditions(X)))
    like = c.like(max_steps=max_steps, equilibrate=dict(max_steps=phase_steps))
    failed = like.batch_conditions(X) == -np.inf
    count = failed.sum(axis=1)
    phase_failed = np.isnan(like.steady_state(X)[:, 0]).any(axis=1)
    print("%s at max_steps %d and a phase of %d: points failing in no / some / all conditions: %d / %d / %d; in the phase of condition 0: %d, in an experiment alone: %d"
          % (c.name, max_steps, phase_steps, np.sum(count == 0), np.sum((count > 0) & (count < 3)), np.sum(count == 3), phase_failed.sum(),
             np.sum(failed.any(axis=1) & ~phase_failed)))
    assert np.any(count == 3) and np.any((count > 0) & (count < 3)) and np.any(count == 0)
    assert np.all(failed[phase_failed, 0]) and phase_failed.any() and np.any(failed.any(axis=1) & ~phase_failed)


# ---------------------------------------------------------------------------------------------------- the device build
def budget_line(c, like):
    """(the record of one full case, the two notes): registers, scratch and static LDS of its likelihood and prediction units for gfx950"""
    a, b = notes(like.code_object()), notes(like.predict_code_object())
    return ("%-10s R %3d SLOTS %d I %d O %2d | likelihood: %3d VGPRs %3d AGPRs scratch %4d LDS %5d | prediction: %3d VGPRs %3d AGPRs scratch %4d LDS %5d"
            % (c.name, len(like.reactions), len(_hill_slots(like.reactions)), len(like.inputs), len(like.observables), a["vgpr"], a["agpr"], a["scratch"],
               a["lds"], b["vgpr"], b["agpr"], b["scratch"], b["lds"])), a, b


@pytest.mark.parametrize("i", CB.FULL, ids=FULL_IDS)
def test_the_combination_cross_compiles_for_gfx950_with_the_lds_row_of_the_header(i):
    """A point's row (csrc/dz_ode_group.h): R + 1 rate constants, SLOTS Hill slots, I gains, I drives, the wave's S state doubles (64 lanes
    only), 2 O noise values; 256 / L rows to a block; nothing at one lane.  Registers and scratch are printed, not asserted
    (profiles/ode_combined_budget.txt is a copy of the lines this test printed when the cases were made; the test does not write
    into the tree)."""
    c = CB.case(i)
    like = c.like()
    line, a, b = budget_line(c, like)
    print(line)
    L, R, slots, I, O = c.lanes, len(like.reactions), len(_hill_slots(like.reactions)), len(like.inputs), len(like.observables)
    assert slots == 4 and I == len(c.U) and like.noise is not None
    want = 0 if L == 1 else (256 // L) * 8 * (R + slots + 2 * I + 1 + (c.S if L == 64 else 0) + 2 * O)
    assert a["lds"] == want and b["lds"] == want
