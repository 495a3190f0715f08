"""MassActionODELogLike(inputs=...) without a GPU: the host builds of the one-lane shape, the lane groups and the wave with
piecewise-linear input time courses are accurate against scipy's Radau restarted at every knot and against a closed form, carry the input
itself to rounding, follow the semantics of csrc/dz_ode.h bit for bit (clipped tables, a gain of exactly 1, conditions with different knot
counts, with_outputs, the order at one time, equilibration under the basal input), leave an object without inputs exactly as it was,
check their arguments, and cross-compile for gfx950 without more scratch than the emulation by a fixed zero-order source."""
import multiprocessing
import os
import pickle
from concurrent.futures import ProcessPoolExecutor

import numpy as np
import pytest

from pydream_amd import likelihoods as LK
from pydream_amd.likelihoods import Input, MassActionODELogLike, Monomial

from . import ode_condition_networks as CN
from . import ode_input_networks as IN
from . import ode_networks as NW
from . import ode_reference as R
from .ode_support import max_rel_err, notes

EPS = np.finfo(float).eps
# The input species' own trajectory against g * interp(t), in units of eps * max|g v| (test_the_input_species_follows_its_table): the
# worst value measured on the host builds, and the bound the tests assert, 8 times that
INPUT_DEVIATION_MEASURED = 8.3
INPUT_DEVIATION_BOUND = 8 * INPUT_DEVIATION_MEASURED


def _pool():
    return ProcessPoolExecutor(max(1, min(8, len(os.sched_getaffinity(0)))), mp_context=multiprocessing.get_context("fork"))


def _same_bits(a, b, X):
    """batch, the step counts and simulate of two objects agree bit for bit"""
    (la, sa), (lb, sb) = a.batch(X, return_steps=True), b.batch(X, return_steps=True)
    assert la.tobytes() == lb.tobytes() and np.array_equal(sa, sb)
    assert a.simulate(X).tobytes() == b.simulate(X).tobytes()
    return la


def _input_deviation(like, inputs, X):
    """the worst |U - g interp| / (eps max|g v|) over the points, the output times and the inputs (the inputs are the last observables)"""
    sim, worst = like.simulate(X), 0.0
    assert np.all(np.isfinite(sim))
    for x, s in zip(X, sim):
        for i, (u, g) in enumerate(zip(inputs, IN.gains(inputs, x))):
            q = s.shape[1] - len(inputs) + i
            worst = max(worst, float(np.max(np.abs(s[:, q] - IN.input_curve(u, g, like.t))) / (EPS * g * max(u.values))))
    return worst


# ---------------------------------------------------------------------------------------------------- accuracy
def test_the_closed_form_and_piecewise_radau_agree_on_drive2():
    """before any build is looked at: the two references, which share nothing, agree to well inside one tolerance (1e-9 relative)"""
    n = IN.network("drive2")
    for x in NW.box_points(n["nominal"], 6, 1, width=1.0):
        ref = IN.radau_observed((n["S"], n["rx"], n["y0"], n["t"], n["inputs"], (), 0.0, n["obs"], x))
        exact = IN.drive2_closed_form(x, n["t"], n["inputs"][0])
        assert np.max(np.abs(ref[:, 0] - exact) / (np.abs(exact) + 1.0)) < 1e-10
        assert np.max(np.abs(ref[:, 1] - IN.input_curve(n["inputs"][0], 10.0 ** x[2], n["t"]))) < 1e-10


@pytest.mark.parametrize("name,n_points,seed", [("drive2", 40, 11), ("mm", 30, 12), ("enzyme13", 16, 14), ("chain17", 16, 15), ("chain40", 8, 16)])
def test_host_build_with_inputs_is_accurate_against_the_references(name, n_points, seed):
    """max_rel_err < 10, the bound of test_ode_events_cpu, against piecewise Radau on every network and against the closed form on drive2"""
    n = IN.network(name)
    X = NW.box_points(n["nominal"], n_points, seed, width=1.0)
    with _pool() as ex:
        refs = list(ex.map(IN.radau_observed, [(n["S"], n["rx"], n["y0"], n["t"], n["inputs"], (), 0.0, n["obs"], x) for x in X], chunksize=2))
    errs = []
    for rtol in (1e-6, 1e-9):
        like = IN.single(name, rtol=rtol, atol=rtol, max_steps=20000)
        assert like.lanes_per_point == n["lanes"] and "INPUTS = %d" % len(n["inputs"]) in like.source()
        errs.append(max_rel_err(like, refs, X, rtol))
        if name == "drive2":
            exact = [np.c_[IN.drive2_closed_form(x, n["t"], n["inputs"][0]), IN.input_curve(n["inputs"][0], 10.0 ** x[2], n["t"])] for x in X]
            errs.append(max_rel_err(like, exact, X, rtol))
    print(name, errs)
    assert all(e < 10 for e in errs)


@pytest.mark.parametrize("name", ["drive2", "mm", "enzyme13", "chain17", "chain40"])
def test_the_input_species_follows_its_table(name):
    """The input species, declared as an observable, against g * interp(t) in units of eps * max|g v|.  Measured on the host builds at
    rtol 1e-8 over 12 box points: drive2 7.36, mm 8.30, enzyme13 6.70, chain17 4.94, chain40 7.43 (a one-segment emulation by a fixed
    source measured 2.3 against its own straight line; here the reference's g is numpy's 10**x, an ulp or two from the solver's dexp,
    and a segment of many steps adds a rounding of the increment per step until the next knot sets the value again); the bound asserted
    is 8 times the worst of them, INPUT_DEVIATION_BOUND = 66.4."""
    n = IN.network(name)
    like = IN.single(name, rtol=1e-8, atol=1e-8, max_steps=20000)
    worst = _input_deviation(like, n["inputs"], NW.box_points(n["nominal"], 12, 2, width=1.0))
    print("input deviation of %s: %.2f eps max|g v|" % (name, worst))
    assert worst <= INPUT_DEVIATION_BOUND


# ---------------------------------------------------------------------------------------------------- semantics, bit for bit
@pytest.mark.parametrize("name", ["mm", "chain17"])
def test_a_table_past_the_span_equals_the_table_clipped_by_hand(name):
    """the working knots are the same, so the data block and every bit are"""
    n = IN.network(name)
    u = n["inputs"][0]
    t0, t_end = 0.0, float(n["t"][-1])
    inner = [(tau, v) for tau, v in zip(u.times, u.values) if t0 < tau < t_end]
    clipped = Input(u.species, [t0] + [tau for tau, _ in inner] + [t_end], [float(u.interp(t0))] + [v for _, v in inner] + [float(u.interp(t_end))], gain=u.gain)
    a = IN.single(name)
    b = IN.single(name, inputs=[clipped], data=a.data)
    assert clipped.times != u.times and a.data_block().tobytes() == b.data_block().tobytes()
    assert np.all(np.isfinite(_same_bits(a, b, NW.box_points(n["nominal"], 20, 3, width=1.0))))


@pytest.mark.parametrize("name", ["mm", "enzyme13"])
def test_a_gain_of_exactly_one_equals_no_gain(name):
    n = IN.network(name)
    u = n["inputs"][0]
    gained = IN.single(name, inputs=[Input(u.species, u.times, u.values, gain=Monomial({u.gain: 1}))])
    plain = IN.single(name, inputs=[Input(u.species, u.times, u.values)], data=gained.data, ndim=len(n["nominal"]))
    X = NW.box_points(n["nominal"], 20, 4, width=1.0)
    X[:, u.gain] = 0.0
    assert gained.source() != plain.source()
    assert np.all(np.isfinite(_same_bits(gained, plain, X)))


def test_conditions_with_different_knot_counts_equal_their_single_experiments():
    """1, 2 and 5 working knots, the last condition also with three events: the blocks of the first two are padded"""
    multi, one = IN.mm_conditions()
    X = NW.box_points(IN.network("mm")["nominal"], 40, 8, width=1.0, outside=0.05)
    assert "INPUTS = 1" in multi.source() and "EVENTS = 3" in multi.source()
    assert [len(multi._input_knots(e["inputs"])) for e in multi._experiments()] == [1, 2, 5]
    blk = multi.data_block()
    assert blk[0] == 3 and len(blk) == 2 + 3 * blk[1] and blk[1] == len(one(2).data_block())
    terms, sims = multi.batch_conditions(X), multi.simulate(X)
    steps = np.zeros(len(X), dtype=np.int64)
    for c in range(3):
        lc, sc = one(c).batch(X, return_steps=True)
        assert terms[:, c].tobytes() == lc.tobytes() and np.all(np.isfinite(lc[np.all(np.abs(X - IN.network("mm")["nominal"]) <= 1.0, axis=1)]))
        assert sims[:, c].tobytes() == one(c).simulate(X).tobytes()
        steps += sc
    total, all_steps = multi.batch(X, return_steps=True)
    assert total.tobytes() == CN.left_to_right(terms).tobytes() and np.array_equal(all_steps, steps)


def test_a_condition_inherits_the_constructors_inputs_unless_it_gives_its_own():
    n = IN.network("mm")
    own = n["inputs"]
    other = [Input(own[0].species, (0.0, 10.0), (1.0, 0.0), gain=own[0].gain)]
    data = np.ones((len(n["obs"]), len(n["t"])))
    multi = MassActionODELogLike(n["S"], n["rx"], n["y0"], n["t"], n["obs"], data, data, inputs=own,
                                 conditions=[dict(), dict(inputs=None), dict(inputs=other)])
    assert [e["inputs"] for e in multi._experiments()] == [tuple(own), tuple(own), tuple(other)]
    X = NW.box_points(n["nominal"], 10, 9, width=1.0)
    terms = multi.batch_conditions(X)
    single = lambda inputs: MassActionODELogLike(n["S"], n["rx"], n["y0"], n["t"], n["obs"], data, data, inputs=inputs)      # noqa: E731
    assert terms[:, 0].tobytes() == terms[:, 1].tobytes() == single(own).batch(X).tobytes()
    assert terms[:, 2].tobytes() == single(other).batch(X).tobytes() != terms[:, 0].tobytes()


@pytest.mark.parametrize("name", ["drive2", "mm x 3", "chain17"])
def test_with_outputs_of_the_own_times_simulates_to_the_same_bits(name):
    like = IN.mm_conditions()[0] if name == "mm x 3" else IN.single(name)
    X = NW.box_points(IN.network(name.split()[0])["nominal"], 10, 5, width=1.0)
    again = like.with_outputs(like.t)
    assert again.inputs == like.inputs and again.simulate(X).tobytes() == like.simulate(X).tobytes()
    dense = like.with_outputs(np.linspace(like.t0, like.t[-1], 57))
    assert np.all(np.isfinite(dense.simulate(X)))
    with pytest.raises(ValueError, match=r"input 0: its table must cover t0 = .* \.\. t\[-1\] = 20.0"):
        like.with_outputs([1.0, 20.0])
    with pytest.raises(ValueError, match="input 0: its table must cover t0 = -5.0"):
        like.with_outputs(like.t, t0=-5.0)


def test_a_collinear_extra_knot_changes_nothing_beyond_the_tolerance():
    n = IN.network("mm")
    u = n["inputs"][0]
    tau = 1.9                               # inside the rising segment 0.75 .. 3.0, between two outputs
    times, values = sorted(u.times + (tau,)), None
    values = [float(u.interp(t)) for t in times]
    X = NW.box_points(n["nominal"], 20, 6, width=1.0)
    with _pool() as ex:
        refs = list(ex.map(IN.radau_observed, [(n["S"], n["rx"], n["y0"], n["t"], n["inputs"], (), 0.0, n["obs"], x) for x in X], chunksize=2))
    rtol = 1e-8
    plain = IN.single("mm", rtol=rtol, atol=rtol, max_steps=20000)
    extra_input = [Input(u.species, times, values, gain=u.gain)]
    extra = IN.single("mm", inputs=extra_input, data=plain.data, rtol=rtol, atol=rtol, max_steps=20000)
    assert len(extra._input_knots(extra.inputs)) == len(plain._input_knots(plain.inputs)) + 1
    assert extra.simulate(X).tobytes() != plain.simulate(X).tobytes()
    assert max_rel_err(extra, refs, X, rtol) < 10 and max_rel_err(plain, refs, X, rtol) < 10
    assert _input_deviation(extra, extra_input, X) <= INPUT_DEVIATION_BOUND


def test_a_knot_an_event_and_an_output_at_one_time_follow_the_stated_order():
    """At 3.0 drive2 has an output, a knot of its input and (here) an event on A.  The output is taken first: up to and including it the
    trajectory is that of the object without the event, bit for bit.  Then the knot, then the event: the run equals, after 3.0, the same
    network started AT 3.0 from the state before the event with the event at its t0 (events at t0 are applied to the start, after the
    knots at t0) -- to the tolerance, since the controller's history differs --, and the input is on its table throughout."""
    n = IN.network("drive2")
    u = n["inputs"][0]
    X = NW.box_points(n["nominal"], 12, 7, width=1.0)
    j = int(np.flatnonzero(n["t"] == 3.0)[0])
    rtol = 1e-9
    kw = dict(rtol=rtol, atol=rtol, max_steps=20000)
    plain = IN.single("drive2", **kw)
    event = (3.0, 1, 0.5, 0.25)
    with_event = IN.single("drive2", events=[event], data=plain.data, **kw)
    a, b = with_event.simulate(X), plain.simulate(X)
    assert a[:, :j + 1].tobytes() == b[:, :j + 1].tobytes() and np.all(a[:, j + 1, 0] != b[:, j + 1, 0])
    assert _input_deviation(with_event, n["inputs"], X) <= INPUT_DEVIATION_BOUND
    with _pool() as ex:
        refs = list(ex.map(IN.radau_observed, [(n["S"], n["rx"], n["y0"], n["t"], n["inputs"], (event,), 0.0, n["obs"], x) for x in X]))
    assert max_rel_err(with_event, refs, X, rtol) < 10
    # the event acts on the state the output showed: A just after 3.0 is 0.5 A(3.0) + 0.25, from which the closed form continues
    for x, s in zip(X, a):
        k_in, k_d, g = 10.0 ** x
        after = 0.5 * s[j, 0] + 0.25
        dt = n["t"][j + 1] - 3.0
        ua, ub = g * u.interp(3.0), g * (u.interp(n["t"][j + 1]) - u.interp(3.0)) / dt
        E = -np.expm1(-k_d * dt) / k_d
        want = after * np.exp(-k_d * dt) + k_in * (ua * E + ub * (dt - E) / k_d)
        assert abs(s[j + 1, 0] - want) < 10 * (rtol * abs(want) + rtol)
    with pytest.raises(ValueError, match="input 0: event 0 targets the input species 0"):
        IN.single("drive2", events=[(3.0, 0, 0.5, 0.25)], data=plain.data)


def test_equilibration_holds_the_input_at_its_basal_value():
    """drive2 and chain17 + input with equilibrate=True: steady_state is the resting state under g u(t0) with every drive 0.
    (1) The input's entry is g u(t0), and the state passes the steady-state test of csrc/dz_ode.h restated in numpy on the reaction
    list, in which nothing feeds the input: drift2 * horizon^2 <= 1.
    (2) The object WITHOUT the phase started from that state (the input's entry 0: the table sets it) gives the same bits.
    (3) drive2 has one mode, faster than the horizon: there the resting state is k_in g u0 / k_d, and a long run under the constant
    basal input -- t0 = -200 with the table flat until 0 -- goes on as the equilibrated run does, within the accuracy test's 10
    tolerances (measured: 0.4).  (chain17's slowest modes are slower than its horizon of 5: a state that passes the test may still be
    far from the limit of the long run, so that comparison says nothing there.)"""
    for name, n_points in (("drive2", 12), ("chain17", 6)):
        n = IN.network(name)
        u = n["inputs"][0]
        X = NW.box_points(n["nominal"], n_points, 8, width=0.5)
        rtol = 1e-9
        kw = dict(rtol=rtol, atol=rtol, max_steps=20000)
        eq = IN.single(name, equilibrate=dict(max_steps=20000), **kw)
        assert "EQUILIBRATE" in eq.source()
        ss, sim = eq.steady_state(X), eq.simulate(X)
        assert np.all(np.isfinite(ss)) and np.all(np.isfinite(sim))
        g = np.array([IN.gains([u], x)[0] for x in X])
        np.testing.assert_allclose(ss[:, u.species], g * u.values[0], rtol=8 * EPS)      # (g: numpy's 10**x here, dexp there)
        horizon = float(n["t"][-1])
        for i, x in enumerate(X):
            f = np.array(R._rhs_and_jacobian(n["S"], n["rx"], R.rate_constants(n["rx"], x, "log10"), ss[i], 0.0)[0])
            assert np.mean((f / (rtol + rtol * np.abs(ss[i]))) ** 2) * horizon ** 2 <= 1.0 + 1e-3
            y0 = ss[i].copy()
            y0[u.species] = 0.0
            started = MassActionODELogLike(n["S"], n["rx"], y0, n["t"], n["obs"], eq.data, eq.sd, inputs=n["inputs"], lanes_per_point=n["lanes"], **kw)
            assert started.simulate(x).tobytes() == sim[i:i + 1].tobytes()
        if name == "drive2":
            k_in, k_d = 10.0 ** X[:, 0], 10.0 ** X[:, 1]
            np.testing.assert_allclose(ss[:, 1], k_in * g * u.values[0] / k_d, rtol=1e-6)
            long_table = Input(u.species, (-1000.0,) + u.times[1:], u.values, gain=u.gain)
            long_run = IN.single(name, inputs=[long_table], t0=-200.0, data=eq.data, **kw).simulate(X)
            err = float(np.max(np.abs(long_run - sim) / (rtol * np.abs(sim) + rtol)))
            print("%s: equilibrated against the long basal run: %.3g tolerances" % (name, err))
            assert err < 10


# ---------------------------------------------------------------------------------------------------- nothing changes without inputs
@pytest.mark.parametrize("shape", ["one lane", "group", "conditions"])
def test_no_inputs_is_the_object_it_always_was(shape):
    from . import ode_wide_networks as W
    if shape == "one lane":
        make = lambda **kw: NW.michaelis_menten(**kw)                   # noqa: E731
    elif shape == "group":
        make = lambda **kw: W.dense_network(13, 30, 16, **kw)            # noqa: E731
    else:
        make = lambda **kw: CN.mm(**kw)[0]                               # noqa: E731
    plain = make()
    for inputs in (None, [], ()):
        like = make(inputs=inputs)
        assert like.source() == plain.source() and like.data_block().tobytes() == plain.data_block().tobytes()
        assert "INPUTS" not in like.source() and like.inputs is None and like._unit() == plain._unit()
        assert "inputs" not in like._experiments()[0]


def test_an_object_pickled_before_the_keyword_existed_still_loads_and_evaluates():
    X = NW.box_points(NW.MM_NOMINAL, 10, 10, width=1.0)
    for like in (NW.michaelis_menten(), CN.mm()[0]):
        want = like.batch(X)
        state = like.__getstate__()
        del state["inputs"]                                             # what such an object lacks
        old = MassActionODELogLike.__new__(MassActionODELogLike)
        old.__dict__.update(state)
        loaded = pickle.loads(pickle.dumps(old))
        assert "inputs" not in loaded.__dict__ and loaded.inputs is None
        assert loaded.source() == like.source() and loaded.data_block().tobytes() == like.data_block().tobytes()
        assert loaded.batch(X).tobytes() == want.tobytes()
    n = IN.network("mm")
    Xi = NW.box_points(n["nominal"], 10, 10, width=1.0)
    with_inputs = pickle.loads(pickle.dumps(IN.single("mm")))
    assert with_inputs.inputs == tuple(n["inputs"]) and with_inputs.batch(Xi).tobytes() == IN.single("mm").batch(Xi).tobytes()


# ---------------------------------------------------------------------------------------------------- validation
def test_inputs_are_checked_at_construction():
    assert LK.ODE_MAX_INPUTS == 4 and LK.ODE_MAX_INPUT_KNOTS == 128
    for args, message in [((0, [0.0], [1.0]), "times must be at least 2"), ((0, [0.0, 0.0], [1.0, 1.0]), "strictly increasing"),
                          ((0, [0.0, np.inf], [1.0, 1.0]), "times must be"), ((0, [0.0, 1.0], [1.0]), "values must be finite and >= 0, one per time"),
                          ((0, [0.0, 1.0], [1.0, -0.1]), "values must be finite and >= 0"), ((0, [0.0, 1.0], [1.0, np.nan]), "values must be finite"),
                          ((-1, [0.0, 1.0], [1.0, 1.0]), "species must be a non-negative integer"), ((True, [0.0, 1.0], [1.0, 1.0]), "species must be")]:
        with pytest.raises(ValueError, match="MassActionODELogLike: an Input's .*" + message):
            Input(*args)
    for gain, message in [(0.0, "fixed gain must be finite and > 0"), (-2.0, "fixed gain"), (np.inf, "fixed gain"), (-1, "parameter index -1 is negative"),
                          ("k", "an Input's gain is a parameter index")]:
        with pytest.raises(ValueError, match="MassActionODELogLike: .*" + message):
            Input(0, [0.0, 1.0], [1.0, 1.0], gain=gain)
    with pytest.raises(AttributeError):
        Input(0, [0.0, 1.0], [1.0, 1.0]).species = 1
    # the working knots: one at t0 with the value there, then the knots strictly inside the span; those at or after t[-1] are dropped
    u = Input(0, [-1.0, 1.0, 2.0, 10.0, 11.0], [0.0, 2.0, 2.0, 0.0, 5.0])
    assert u.working_knots(0.0, 10.0) == [(0.0, 1.0, 1.0), (1.0, 2.0, 0.0), (2.0, 2.0, -0.25)]
    assert u.working_knots(1.0, 2.0) == [(1.0, 2.0, 0.0)] and u.working_knots(1.5, 12.0)[0] == (1.5, 2.0, 0.0)

    n = IN.network("mm")
    S, rx, t, obs, U = n["S"], n["rx"], n["t"], n["obs"], n["inputs"][0].species
    data = np.ones((len(obs), len(t)))
    make = lambda inputs, rx=rx, y0=n["y0"], **kw: MassActionODELogLike(S, rx, y0, t, obs, data, data, inputs=inputs, **kw)      # noqa: E731
    table = ([0.0, 10.0], [1.0, 0.0])
    assert make([Input(U, *table)]).d == 4 and make([Input(U, *table, gain=7)]).d == 8
    assert make([Input(U, *table, gain=Monomial({9: 1}))]).d == 10
    y0_bad = n["y0"].copy(); y0_bad[U] = 0.5
    y0_mono = list(n["y0"]); y0_mono[U] = Monomial({0: 1})
    bad = [([Input(S, *table)], {}, "input 0 names species 5"),
           ([Input(U, *table), Input(U, *table)], {}, "input 1: species 4 already carries an input"),
           ([Input(1, *table)], {}, "input 0: reaction 0 produces or consumes species 1"),
           ([Input(U, *table)], dict(rx=rx + [({U: 1}, {}, 0.1)]), "input 0: reaction 4 produces or consumes species 4"),
           ([Input(U, *table)], dict(rx=rx + [({}, {U: 1}, 0.1)]), "input 0: reaction 4 produces or consumes species 4"),
           ([Input(U, *table)], dict(events=[(1.0, U, 1.0, 1.0)]), "input 0: event 0 targets the input species 4"),
           ([Input(U, *table)], dict(y0=y0_bad), r"input 0: y0\[4\] must be 0"),
           ([Input(U, *table)], dict(y0=y0_mono), r"input 0: y0\[4\] is a Monomial"),
           ([Input(U, [0.5, 10.0], [1.0, 1.0])], {}, "input 0: its table must cover t0 = 0.0 .. t.-1. = 10.0"),
           ([Input(U, [0.0, 9.5], [1.0, 1.0])], {}, "input 0: its table must cover"),
           ([Input(U, *table, gain=5)], dict(ndim=5), "parameter index 5 is not < ndim = 5"),
           ([Input(U, np.linspace(0.0, 10.0, 130), np.ones(130))], {}, r"at most 128 working knots per experiment .* \(got 129\)"),
           ([(U, *table)], {}, "inputs must be a sequence of Input objects"),
           ([Input(U, *table)] * 5, {}, r"at most 4 inputs are supported \(got 5\)")]
    for inputs, kw, message in bad:
        with pytest.raises(ValueError, match="MassActionODELogLike: " + message):
            make(inputs, **kw)
    assert len(make([Input(U, np.linspace(0.0, 10.0, 129), np.ones(129))])._input_knots(make([Input(U, np.linspace(0.0, 10.0, 129), np.ones(129))]).inputs)) == 128
    # a reaction may read the input as a catalyst, a kinetic order or a Hill factor's species
    reads = rx + [({U: 2, 0: 1}, {U: 2}, 0.1), ({}, {3: 1}, LK.RateLaw(0.2, [LK.Hill(U, 0.5, 2)])), ({1: 1}, {}, LK.RateLaw(0.1, order={U: 1, 1: 1}))]
    assert np.isfinite(make([Input(U, *table)], rx=reads)(n["nominal"]))
    # a condition's inputs: the same species, order and gains; its own tables; the message names the condition
    conds = lambda inputs, **kw: [dict(), dict(inputs=inputs, **kw)]      # noqa: E731
    own = [Input(U, *table, gain=4)]
    assert make(own, conditions=conds([Input(U, [0.0, 5.0, 10.0], [0.0, 1.0, 1.0], gain=4)])).conditions[1]["inputs"][0].times == (0.0, 5.0, 10.0)
    for inputs, kw, message in [([Input(U, *table)], {}, "condition 1: inputs must name the constructor's input species"),
                                ([Input(U, *table, gain=4.0)], {}, "condition 1: inputs must name"), ([], {}, "condition 1: inputs must name"),
                                ([Input(U, [1.0, 10.0], [1.0, 1.0], gain=4)], {}, "condition 1: input 0: its table must cover"),
                                (None, dict(events=[(2.0, U, 0.0, 0.0)]), "condition 1: input 0: event 0 targets the input species"),
                                (None, dict(y0=y0_bad), r"condition 1: input 0: y0\[4\] must be 0")]:
        with pytest.raises(ValueError, match="MassActionODELogLike: " + message):
            make(own, conditions=conds(inputs, **kw))
    with pytest.raises(ValueError, match="condition 1: inputs must name the constructor's input species"):
        make(None, conditions=conds(own))


def test_a_gain_that_is_not_finite_or_not_positive_rejects_the_point():
    n = IN.network("mm")
    u = n["inputs"][0]
    lin = IN.single("mm", rate_scale="linear", data=IN.single("mm").data)
    X = np.tile(10.0 ** n["nominal"], (5, 1))
    X[1:, u.gain] = [0.0, -1.0, np.inf, np.nan]
    assert np.isfinite(lin.batch(X)[0]) and np.all(lin.batch(X)[1:] == -np.inf)
    log = IN.single("mm")
    Y = np.tile(n["nominal"], (4, 1))
    Y[1:, u.gain] = [np.inf, -np.inf, np.nan]
    assert np.isfinite(log.batch(Y)[0]) and np.all(log.batch(Y)[1:] == -np.inf)
    for name in ("enzyme13", "chain40"):                                   # the group form's gain(): the same rule
        m = IN.network(name)
        Z = np.tile(m["nominal"], (3, 1))
        Z[1:, m["inputs"][0].gain] = [np.nan, -np.inf]
        got = IN.single(name).batch(Z)
        assert np.isfinite(got[0]) and np.all(got[1:] == -np.inf)


def test_fixed_steps_ignores_inputs():
    """as it ignores events: every drive 0, the input species at its y0 entry 0 -- the network underneath alone"""
    n = IN.network("mm")
    like = IN.single("mm")
    y = like.fixed_steps(n["nominal"], 2.0, 50)
    bare = NW.michaelis_menten().fixed_steps(NW.MM_NOMINAL, 2.0, 50)
    assert y[4] == 0.0 and np.allclose(y[:4], bare, rtol=1e-12, atol=1e-15)


# ---------------------------------------------------------------------------------------------------- failures
def test_a_starved_step_limit_fails_a_mix_of_conditions():
    """max_steps counts a segment's attempted steps; at IN.MM_STARVED_MAX_STEPS some points of the GPU test's batch fail in all three
    conditions, some in a few and some in none, and at 500 none fails."""
    X = NW.box_points(IN.network("mm")["nominal"], 131, 21, width=1.0)
    assert np.all(np.isfinite(IN.mm_conditions()[0].batch_conditions(X)))
    count = np.sum(IN.mm_conditions(max_steps=IN.MM_STARVED_MAX_STEPS)[0].batch_conditions(X) == -np.inf, axis=1)
    print("conditions failed per point at max_steps %d:" % IN.MM_STARVED_MAX_STEPS, np.bincount(count, minlength=4))
    assert np.any(count == 3) and np.any((count > 0) & (count < 3)) and np.any(count == 0)


# ---------------------------------------------------------------------------------------------------- the device build
@pytest.mark.parametrize("model", ["drive2", "mm x 3", "enzyme13@16 x 3", "chain40@64"])
def test_inputs_cross_compile_for_gfx950_without_more_scratch_than_the_emulation(model):
    """against what the code before inputs could build: the input species a plain species fed by a fixed zero-order source"""
    three = [dict(), dict(), dict()]
    if model == "drive2":
        with_inputs, emulated = IN.single("drive2"), IN.emulation("drive2")
    elif model == "mm x 3":
        with_inputs, emulated = IN.mm_conditions()[0], IN.emulation("mm", conditions=three, events=list(IN.MM_EVENTS))
    elif model == "enzyme13@16 x 3":
        with_inputs, emulated = IN.enzyme13_conditions()[0], IN.emulation("enzyme13", conditions=three)
    else:
        with_inputs, emulated = IN.single("chain40"), IN.emulation("chain40")
    assert "INPUTS" in with_inputs.source() and "INPUTS" not in emulated.source()
    a, b = notes(with_inputs.code_object()), notes(emulated.code_object())
    print("%s: with inputs %d VGPRs, %d AGPRs, scratch %d, LDS %d; emulated %d VGPRs, %d AGPRs, scratch %d, LDS %d"
          % (model, a["vgpr"], a["agpr"], a["scratch"], a["lds"], b["vgpr"], b["agpr"], b["scratch"], b["lds"]))
    assert a["scratch"] <= b["scratch"]
