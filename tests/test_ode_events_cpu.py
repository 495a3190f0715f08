"""MassActionODELogLike(events=...) without a GPU: the host build with dosing and wash-out events is accurate against scipy's Radau
restarted at every event, follows the semantics of csrc/dz_ode.h bit for bit (events at t0, on an output time, at one time, at the last
time), keeps conditions independent of each other's padding, leaves an object without events exactly as it was, checks its arguments,
and cross-compiles for gfx950 without more scratch than the same network without events."""
import multiprocessing
import os
import pickle
from concurrent.futures import ProcessPoolExecutor

import numpy as np
import pytest

from pydream_amd import likelihoods as LK
from pydream_amd.likelihoods import MassActionODELogLike

from . import ode_condition_networks as CN
from . import ode_event_networks as EN
from . import ode_networks as NW
from . import ode_reference as R
from . import ode_wide_networks as W
from .ode_support import max_rel_err, notes


def _pool():
    return ProcessPoolExecutor(max(1, min(8, len(os.sched_getaffinity(0)))), mp_context=multiprocessing.get_context("fork"))


def _same_bits(a, b, X):
    """batch, the step counts and simulate of two objects agree bit for bit"""
    (la, sa), (lb, sb) = a.batch(X, return_steps=True), b.batch(X, return_steps=True)
    assert la.tobytes() == lb.tobytes() and np.array_equal(sa, sb)
    assert a.simulate(X).tobytes() == b.simulate(X).tobytes()
    return la


# ---------------------------------------------------------------------------------------------------- accuracy
@pytest.mark.parametrize("name,n,seed", [("mm", 40, 12), ("chain8", 30, 13), ("enzyme13", 24, 14), ("chain17", 24, 15)])
def test_host_build_with_events_is_accurate_against_piecewise_radau(name, n, seed):
    """The measure and thresholds of test_host_build_is_accurate_against_radau_and_error_shrinks_with_tolerance; the events lie before the
    first output time, exactly on output times and strictly between them (ode_event_networks)."""
    S, rx, y0, t, obs, nominal, _, lanes = EN._network(name)
    events = EN.EVENTS[name]
    X = NW.box_points(nominal, n, seed, width=1.0)
    with _pool() as ex:
        refs = list(ex.map(EN.radau_observed, [(S, rx, y0, t, events, 0.0, obs, x) for x in X], chunksize=2))
    errs = []
    for rtol in (1e-6, 1e-9):
        like = EN.single(name, rtol=rtol, atol=rtol, max_steps=20000)
        assert like.lanes_per_point == lanes and "EVENTS = %d" % len(events) in like.source()
        errs.append(max_rel_err(like, refs, X, rtol))
    print(name, errs)
    assert errs[0] < 10 and errs[1] < 10
    abs_errs = [e * r for e, r in zip(errs, (1e-6, 1e-9))]
    assert abs_errs[1] < 1e-2 * abs_errs[0]


# ---------------------------------------------------------------------------------------------------- semantics, bit for bit
@pytest.mark.parametrize("name,event", [("mm", (0.0, 1, 1.0, 1.0)), ("chain8", (0.0, 2, 0.0, 0.25)), ("chain8", (0.0, 1, 0.5, 0.125))])
def test_an_event_at_t0_is_a_changed_start(name, event):
    """Exactly representable numbers: the object whose y0 was changed by hand gives the same bits (chain8 has an output at t0: it shows
    the changed start)."""
    S, rx, y0, t, obs, nominal, _, _ = EN._network(name)
    with_event = EN.single(name, events=[event])
    by_hand = np.array(y0, dtype=float)
    by_hand[event[1]] = event[2] * by_hand[event[1]] + event[3]
    changed = MassActionODELogLike(S, rx, by_hand, t, obs, with_event.data, with_event.sd)
    assert "EVENTS" in with_event.source() and "EVENTS" not in changed.source()
    like = _same_bits(with_event, changed, NW.box_points(nominal, 30, 3, width=1.0))
    assert np.all(np.isfinite(like))


def test_an_output_at_an_event_time_shows_the_state_before_the_event():
    """The product P of MM washed out at the output time 3.0: up to and including that output the trajectory is the undisturbed one, bit
    for bit; the next output shows the effect."""
    X = NW.box_points(NW.MM_NOMINAL, 30, 4, width=1.0)
    j = int(np.flatnonzero(NW.MM_T == 3.0)[0])
    washed, plain = EN.single("mm", events=[(3.0, 3, 0.0, 0.0)]).simulate(X), EN.single("mm", events=None).simulate(X)
    assert np.all(np.isfinite(washed)) and washed[:, :j + 1].tobytes() == plain[:, :j + 1].tobytes()
    assert np.all(washed[:, j + 1, 1] < washed[:, j, 1]) and np.all(plain[:, j + 1, 1] >= plain[:, j, 1])
    assert np.all(washed[:, j + 1:, 1] < plain[:, j + 1:, 1])


def test_events_at_one_time_apply_in_the_order_given():
    """wash out, then add 2: the amount is 2; add 2, then wash out: it is 0"""
    X = NW.box_points(NW.MM_NOMINAL, 20, 5, width=1.0)
    tau, s = 4.2, 1
    first, second = (tau, s, 0.0, 0.0), (tau, s, 1.0, 2.0)
    a = EN.single("mm", events=[first, second])
    data = dict(data=a.data, sd=a.sd)
    args = (4, NW.MM_REACTIONS, NW.MM_Y0, NW.MM_T, CN.MM_OBSERVABLES)
    b = MassActionODELogLike(*args, events=[second, first], **data)
    assert a.events == (first, second) and b.events == (second, first)
    assert a.simulate(X).tobytes() != b.simulate(X).tobytes()
    _same_bits(a, MassActionODELogLike(*args, events=[(tau, s, 0.0, 2.0)], **data), X)
    _same_bits(b, MassActionODELogLike(*args, events=[(tau, s, 0.0, 0.0)], **data), X)
    # sorted by time, stably: a later event given first moves behind, the two at tau keep their order
    c = MassActionODELogLike(*args, events=[(6.0, 0, 0.5, 0.0), second, first, (1.0, 3, 0.0, 0.0)], **data)
    assert c.events == ((1.0, 3, 0.0, 0.0), second, first, (6.0, 0, 0.5, 0.0))


@pytest.mark.parametrize("name", ["mm", "chain8"])
def test_an_event_at_the_last_output_time_changes_nothing(name):
    S, rx, y0, t, obs, nominal, _, _ = EN._network(name)
    plain = EN.single(name, events=None)
    late = MassActionODELogLike(S, rx, y0, t, obs, plain.data, plain.sd, events=[(float(t[-1]), 1, 0.0, 0.0), (float(t[-1]), 0, 1.0, 5.0)])
    assert "EVENTS = 2" in late.source()
    _same_bits(late, plain, NW.box_points(nominal, 30, 6, width=1.0))


def _equilibrated(args):
    S, rx, y0, x = args
    return np.maximum(R.radau(S, rx, R.rate_constants(rx, x, "log10"), y0, [0.0], t0=-1000.0)[0], 0.0)


def test_a_bolus_after_a_long_pre_equilibration_agrees_with_a_start_from_the_equilibrated_state():
    """MM with its enzyme, free substrate and complex left alone from t0 = -1000, then a bolus of substrate at 0, against the object started
    at 0 from Radau's state at 0 plus the bolus: the accuracy test's measure between the two, and each against piecewise Radau."""
    X = NW.box_points(NW.MM_NOMINAL, 20, 7, width=1.0)
    bolus = (0.0, 1, 1.0, 2.0)
    obs = np.asarray(CN.MM_OBSERVABLES, dtype=float)
    with _pool() as ex:
        starts = list(ex.map(_equilibrated, [(4, NW.MM_REACTIONS, NW.MM_Y0, x) for x in X]))
        refs = list(ex.map(EN.radau_observed, [(4, NW.MM_REACTIONS, NW.MM_Y0, NW.MM_T, (bolus,), -1000.0, obs, x) for x in X]))
    errs = []
    for rtol in (1e-6, 1e-9):
        kw = dict(rtol=rtol, atol=rtol, max_steps=20000)
        long_run = EN.single("mm", events=[bolus], t0=-1000.0, **kw)
        sim = long_run.simulate(X)
        assert np.all(np.isfinite(sim))
        between = 0.0
        for i, x in enumerate(X):
            y0 = starts[i].copy()
            y0[1] = y0[1] + 2.0
            short = MassActionODELogLike(4, NW.MM_REACTIONS, y0, NW.MM_T, obs, long_run.data, long_run.sd, **kw).simulate(x)[0]
            between = max(between, float(np.max(np.abs(sim[i] - short) / (rtol * np.abs(short) + rtol))))
        errs.append((between, max_rel_err(long_run, refs, X, rtol)))
    print("pre-equilibration: (against the equilibrated start, against piecewise Radau) at rtol 1e-6, 1e-9:", errs)
    assert all(e < 10 for pair in errs for e in pair)
    assert errs[1][1] * 1e-9 < 1e-2 * errs[0][1] * 1e-6


# ---------------------------------------------------------------------------------------------------- conditions
def test_conditions_with_different_event_counts_equal_their_single_experiments():
    """0, 1 and 3 events: the generated network has EVENTS = 3 and the blocks of the first two conditions are padded, the single-experiment
    objects have EVENTS absent, 1 and 3 -- the same bits."""
    multi, one = EN.mm_conditions()
    X = NW.box_points(NW.MM_NOMINAL, 60, 8, width=1.0, outside=0.05)
    assert "EVENTS = 3" in multi.source() and "EVENTS" not in one(0).source() and "EVENTS = 1" in one(1).source()
    blk = multi.data_block()
    assert blk[0] == 3 and len(blk) == 2 + 3 * blk[1] and blk[1] == len(one(2).data_block()) == len(one(0).data_block()) + 1 + 4 * 3
    terms = multi.batch_conditions(X)
    steps = np.zeros(len(X), dtype=np.int64)
    for c in range(3):
        lc, sc = one(c).batch(X, return_steps=True)
        assert terms[:, c].tobytes() == lc.tobytes() and np.all(np.isfinite(lc))
        assert multi.simulate(X)[:, c].tobytes() == one(c).simulate(X).tobytes()
        steps += sc
    total, all_steps = multi.batch(X, return_steps=True)
    assert total.tobytes() == CN.left_to_right(terms).tobytes() and np.array_equal(all_steps, steps)


def test_a_condition_inherits_the_constructors_events_unless_it_gives_its_own():
    _, one = EN.mm_conditions()
    d = [one(c) for c in range(3)]
    cond = lambda c, **kw: dict(y0=d[c].y0, data=d[c].data, sd=d[c].sd, **kw)          # noqa: E731
    args = (4, NW.MM_REACTIONS, None, NW.MM_T, CN.MM_OBSERVABLES, None, None)
    multi = MassActionODELogLike(*args, conditions=[cond(0, events=[]), cond(1, events=None), cond(2)], events=list(EN.MM_EVENTS))
    assert [c["events"] for c in multi.conditions] == [(), EN.MM_EVENTS, EN.MM_EVENTS]
    X = NW.box_points(NW.MM_NOMINAL, 20, 9, width=1.0)
    terms = multi.batch_conditions(X)
    single = lambda c, ev: MassActionODELogLike(*args[:2], d[c].y0, *args[3:5], d[c].data, d[c].sd, events=ev)      # noqa: E731
    assert terms[:, 0].tobytes() == single(0, None).batch(X).tobytes()
    assert terms[:, 1].tobytes() == single(1, EN.MM_EVENTS).batch(X).tobytes()
    assert terms[:, 2].tobytes() == single(2, EN.MM_EVENTS).batch(X).tobytes() == d[2].batch(X).tobytes()
    # every condition overrides to none: an object without events
    none = MassActionODELogLike(*args, conditions=[cond(c, events=[]) for c in range(3)], events=list(EN.MM_EVENTS))
    assert "EVENTS" not in none.source() and none.events == EN.MM_EVENTS


# ---------------------------------------------------------------------------------------------------- nothing changes without events
@pytest.mark.parametrize("shape", ["one lane", "group", "conditions", "group conditions"])
def test_no_events_is_the_object_it_always_was(shape):
    if shape == "one lane":
        make = lambda **kw: NW.michaelis_menten(**kw)                   # noqa: E731
    elif shape == "group":
        make = lambda **kw: W.dense_network(13, 30, 16, **kw)            # noqa: E731
    elif shape == "conditions":
        make = lambda **kw: CN.mm(**kw)[0]                               # noqa: E731
    else:
        def make(**kw):
            like = W.dense_network(13, 30, 16)
            return MassActionODELogLike(13, like.reactions, None, like.t, like.observables, like.data, like.sd, lanes_per_point=16,
                                        conditions=[dict(y0=like.y0), dict(y0=2 * like.y0)], **kw)
    plain = make()
    for events in (None, [], ()):
        like = make(events=events)
        assert like.source() == plain.source() and like.data_block().tobytes() == plain.data_block().tobytes()
        assert "EVENTS" not in like.source() and like.events is None and like._unit() == plain._unit()
    with_events = make(events=[(0.3, 0, 1.0, 1.0)])
    assert "EVENTS = 1" in with_events.source() and len(with_events.data_block()) > len(plain.data_block())


def test_an_object_pickled_before_the_keyword_existed_still_loads_and_evaluates():
    X = NW.box_points(NW.MM_NOMINAL, 10, 10, width=1.0)
    for like in (NW.michaelis_menten(), CN.mm()[0]):
        want = like.batch(X)
        state = like.__getstate__()
        del state["events"]                                             # what such an object lacks
        if state["conditions"] is not None:
            state["conditions"] = [{k: v for k, v in cond.items() if k != "events"} for cond in state["conditions"]]
        old = MassActionODELogLike.__new__(MassActionODELogLike)
        old.__dict__.update(state)
        loaded = pickle.loads(pickle.dumps(old))
        assert "events" not in loaded.__dict__ and loaded.events is None
        assert loaded.source() == like.source() and loaded.data_block().tobytes() == like.data_block().tobytes()
        assert loaded.batch(X).tobytes() == want.tobytes()
    with_events = pickle.loads(pickle.dumps(EN.single("mm")))
    assert with_events.events == EN.MM_EVENTS and with_events.batch(X).tobytes() == EN.single("mm").batch(X).tobytes()


# ---------------------------------------------------------------------------------------------------- validation
def test_events_are_checked_at_construction():
    data = np.ones((2, len(NW.MM_T)))
    args = (4, NW.MM_REACTIONS, NW.MM_Y0, NW.MM_T, CN.MM_OBSERVABLES, data, data)
    make = lambda events, **kw: MassActionODELogLike(*args, events=events, **kw)         # noqa: E731
    assert LK.ODE_MAX_EVENTS == 16
    ok = make([(0.0, 0, 0.0, 0.0), (10.0, 3, 2.5, 0.0), (np.float64(1.0), np.int64(2), 1, 3)])       # t0 and t[-1] themselves; numpy scalars, ints
    assert ok.events == ((0.0, 0, 0.0, 0.0), (1.0, 2, 1.0, 3.0), (10.0, 3, 2.5, 0.0))
    assert make([(-1.0, 0, 1.0, 1.0)], t0=-1.0).events == ((-1.0, 0, 1.0, 1.0),)
    bad = [([(np.nan, 0, 1.0, 1.0)], "event 0: the time"), ([(np.inf, 0, 1.0, 1.0)], "event 0: the time"),
           ([(1.0, 0, 1.0, 1.0), (-0.5, 0, 1.0, 1.0)], "event 1: the time"), ([(10.5, 0, 1.0, 1.0)], "event 0: the time"),
           ([("now", 0, 1.0, 1.0)], "event 0: the time"), ([(True, 0, 1.0, 1.0)], "event 0: the time"),
           ([(1.0, 4, 1.0, 1.0)], "event 0 names species 4"), ([(1.0, -1, 1.0, 1.0)], "event 0 names species -1"),
           ([(1.0, 1.0, 1.0, 1.0)], "event 0 names species 1.0"), ([(1.0, True, 1.0, 1.0)], "event 0 names species True"),
           ([(1.0, 0, -0.5, 1.0)], "event 0: factor and amount must be finite and >= 0"), ([(1.0, 0, np.nan, 1.0)], "event 0: factor and amount must be finite"),
           ([(1.0, 0, 1.0, -1e-9)], "event 0: factor and amount must be finite and >= 0"), ([(1.0, 0, 1.0, np.inf)], "event 0: factor and amount must be finite"),
           ([(1.0, 0, 1.0, LK.Monomial({0: 1}))], "event 0: factor and amount are numbers; a Monomial .a sampled dose. is not supported"),
           ([(1.0, 0, 1.0)], "event 0 must be .time, species, factor, amount."), ([1.0], "event 0 must be .time, species, factor, amount."),
           (3.0, "events must be a sequence")]
    for events, message in bad:
        with pytest.raises(ValueError, match="MassActionODELogLike: " + message):
            make(events)
    sixteen = [(0.5 * i, i % 4, 1.0, 0.1) for i in range(16)]
    assert len(make(sixteen).events) == 16 and "EVENTS = 16" in make(sixteen).source()
    with pytest.raises(ValueError, match=r"MassActionODELogLike: at most 16 events per experiment are supported \(got 17\)"):
        make(sixteen + [(9.0, 0, 1.0, 0.1)])
    # a condition's events: the same rules, and the message names the condition
    conds = lambda events: [dict(y0=NW.MM_Y0), dict(y0=NW.MM_Y0, events=events)]         # noqa: E731
    multi = lambda events, **kw: MassActionODELogLike(*args, conditions=conds(events), **kw)      # noqa: E731
    assert multi(sixteen).conditions[1]["events"] == tuple(sixteen) and multi(sixteen).conditions[0]["events"] == ()
    for events, message in bad + [(sixteen + [(9.0, 0, 1.0, 0.1)], r"at most 16 events per experiment are supported \(got 17\)")]:
        with pytest.raises(ValueError, match="MassActionODELogLike: condition 1: " + message):
            multi(events)
    with pytest.raises(ValueError, match="condition 0 must be a mapping with the keys"):
        MassActionODELogLike(*args, conditions=[dict(y0=NW.MM_Y0, event=[])])
    with pytest.raises(ValueError, match="MassActionODELogLike: event 0: the time"):                # the constructor's own: no condition named
        MassActionODELogLike(*args, conditions=conds([]), events=[(11.0, 0, 1.0, 1.0)])


# ---------------------------------------------------------------------------------------------------- the device build
@pytest.mark.parametrize("model", ["mm", "enzyme13@16", "mm x 3"])
def test_events_cross_compile_for_gfx950_without_more_scratch(model):
    if model == "mm":
        with_events, without = EN.single("mm"), EN.single("mm", events=None)
    elif model == "enzyme13@16":
        with_events, without = EN.single("enzyme13"), EN.single("enzyme13", events=None)
    else:
        with_events, without = EN.mm_conditions()[0], CN.mm()[0]
    assert "EVENTS = 3" in with_events.source() and "EVENTS" not in without.source()
    a, b = notes(with_events.code_object()), notes(without.code_object())
    print("%s: with events %d VGPRs, %d AGPRs, scratch %d; without %d VGPRs, %d AGPRs, scratch %d"
          % (model, a["vgpr"], a["agpr"], a["scratch"], b["vgpr"], b["agpr"], b["scratch"]))
    assert a["scratch"] <= b["scratch"]


# ---------------------------------------------------------------------------------------------------- failures
def test_a_small_step_limit_fails_some_points_in_a_segment_after_an_event():
    """max_steps counts a SEGMENT's attempted steps.  MM from a small dose (0.5) with a bolus of 8 at the output time 3.0 and
    max_steps 60 (EN.MM_STARVED_MAX_STEPS): the restart after the bolus needs more steps than the run up to it.  A point has failed after
    the event if the same object cut off at 3.0 (no event left in it) is finite and the whole is not."""
    ms = EN.MM_STARVED_MAX_STEPS
    y0, events = [0.5, 0.5, 0.0, 0.0], [(3.0, 1, 1.0, 8.0)]
    X = NW.box_points(NW.MM_NOMINAL, 200, 5, width=1.0)
    whole = EN.single("mm", events=events, y0=y0, max_steps=ms)
    j = int(np.flatnonzero(NW.MM_T == 3.0)[0]) + 1
    cut = MassActionODELogLike(4, NW.MM_REACTIONS, y0, NW.MM_T[:j], CN.MM_OBSERVABLES, whole.data[:, :j], whole.sd[:, :j], max_steps=ms)
    failed, failed_before = whole.batch(X) == -np.inf, cut.batch(X) == -np.inf
    print("max_steps %d: %d of %d points fail, %d of them before the event, %d after it; at the default limit %d fail"
          % (ms, failed.sum(), len(X), failed_before.sum(), np.sum(failed & ~failed_before), np.sum(EN.single("mm", events=events, y0=y0).batch(X) == -np.inf)))
    assert np.all(failed[failed_before])
    assert np.any(failed & ~failed_before) and np.any(~failed)
    sim = whole.simulate(X)
    assert np.all(np.isnan(sim[failed])) and np.all(np.isfinite(sim[~failed]))
    # ... and under conditions with 0, 1 and 3 events: points that fail in all, in some and in no condition (the GPU test's case)
    multi, _ = EN.mm_conditions(max_steps=ms)
    count = np.sum(multi.batch_conditions(NW.box_points(NW.MM_NOMINAL, 131, 21, width=1.0, outside=0.05)) == -np.inf, axis=1)
    assert np.any(count == 3) and np.any((count > 0) & (count < 3)) and np.any(count == 0)
