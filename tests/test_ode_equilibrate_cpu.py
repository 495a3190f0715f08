"""MassActionODELogLike(equilibrate=...) without a GPU: the keyword is checked and an object without the phase is byte for byte the
object it was on the commit before the keyword existed; the host build's resting state satisfies the steady-state test restated in
numpy and keeps the conserved totals; the hand-over to the experiment is exact (the object started by hand from steady_state gives the
same bits); trajectories agree with scipy's Radau run to its own steady state and restarted at t0; the Brusselator converges below its
Hopf point and fails after exactly max_steps attempts above it; conditions equilibrate independently; a starved phase fails some points
and not others; the example's closed-form check passes."""
import hashlib
import multiprocessing
import os
import pickle
from concurrent.futures import ProcessPoolExecutor

import numpy as np
import pytest

from pydream_amd import likelihoods as LK
from pydream_amd.likelihoods import MassActionODELogLike

from . import ode_condition_networks as CN
from . import ode_equilibrate_networks as EQ
from . import ode_event_networks as EV
from . import ode_networks as NW
from . import ode_reference as R
from . import ode_wave_networks as WV
from . import ode_wide_networks as W
from .ode_support import max_rel_err

# sha256 of source() on the commit before the keyword existed
PARENT_SOURCE_SHA256 = {
    "robertson": "c4fd92120c3b297f5ca95cc5badd01f82fb4e13702022f116b6aa3a583f6be0e",
    "mm": "6d00d6a6fca814cf3e78bbb94833510faea553e0a15e8c10a298484cf7625ceb",
    "chain8": "7c21c344e8c175a67e16fed278d7b683bdd838ae0231a090733fec458e45c951",
    "enzyme13@16": "0aa13e4724688b1327784e38675d9c71e37520f6bfef3fb95eef62929af3b1f6",
    "chain17@32": "213a3d0d37e097dc2e6d76aa47213ef57033529e4421fa2e4b47f1a050f9883c",
    "chain33@64": "b15bcf8e83a5d25d6d5fc0c7bc5afe213a3c340f97fd38a0e20db957675d1157",
    "mm x 3 with events": "5707f117e451ef7e7bf1cbd646718daab5d9bd5fa4350b5c0a1f16c88f87210f",
}
UNCHANGED = {
    "robertson": NW.robertson, "mm": NW.michaelis_menten, "chain8": NW.chain8, "enzyme13@16": lambda **kw: W.enzyme13(16, **kw),
    "chain17@32": lambda **kw: W.chain(17, 32, **kw), "chain33@64": lambda **kw: WV.chain(33, **kw),
    "mm x 3 with events": lambda **kw: EV.mm_conditions(**kw)[0],
}


def _sha(like):
    return hashlib.sha256(like.source().encode()).hexdigest()


def _drift(S, reactions, k, y, horizon, rtol, atol, ulps=0.0):
    """mean((f(y) horizon / (atol + rtol |y|))**2) in numpy: the steady-state test, written independently of the generated code.
    ulps: every |f_s| taken smaller by that many ulp of sum_j |N_sj| v_j, the magnitude of the terms that cancel in it."""
    N, nu = R.stoichiometry(S, reactions)
    v = k * np.prod(np.asarray(y, dtype=float)[None, :] ** nu, axis=1)
    f = np.maximum(np.abs(N @ v) - ulps * np.finfo(float).eps * (np.abs(N) @ np.abs(v)), 0.0)
    return float(np.mean((f * horizon / (atol + rtol * np.abs(y))) ** 2))


# ---------------------------------------------------------------------------------------------------- the keyword
def test_the_keyword_is_checked_at_construction():
    data = np.ones((2, len(NW.MM_T)))
    args = (4, NW.MM_REACTIONS, NW.MM_Y0, NW.MM_T, CN.MM_OBSERVABLES, data, data)
    make = lambda eq, **kw: MassActionODELogLike(*args, equilibrate=eq, **kw)                 # noqa: E731
    assert LK.ODE_EQUILIBRATE_MAX_STEPS == 2000
    assert make(None).equilibrate is None and make(False).equilibrate is None
    full = make(True, rtol=1e-6, atol=1e-9).equilibrate
    assert full == dict(rtol=1e-6, atol=1e-9, horizon=10.0, max_step=1e7, max_steps=2000) and make({}).equilibrate["horizon"] == 10.0
    assert make(True, t0=-2.0).equilibrate["horizon"] == 12.0
    given = make(dict(rtol=1e-5, atol=np.float64(1e-7), horizon=3, max_step=np.float64(50.0), max_steps=np.int64(7))).equilibrate
    assert given == dict(rtol=1e-5, atol=1e-7, horizon=3.0, max_step=50.0, max_steps=7)
    assert make(dict(horizon=4.0)).equilibrate["max_step"] == 4e6
    bad = [(1, "equilibrate must be None, False, True or a mapping"), ("yes", "equilibrate must be None, False, True or a mapping"),
           (1.0, "equilibrate must be None, False, True or a mapping"), ([("rtol", 1e-6)], "equilibrate must be None, False, True or a mapping"),
           (dict(tol=1e-6), "equilibrate must be None, False, True or a mapping"), (dict(rtol=0.0), "equilibrate: rtol must be finite and > 0"),
           (dict(rtol=np.nan), "equilibrate: rtol must be finite and > 0"), (dict(atol=-1e-9), "equilibrate: atol must be finite and > 0"),
           (dict(atol=True), "equilibrate: atol must be finite and > 0"), (dict(horizon=0.0), "equilibrate: horizon must be finite and > 0"),
           (dict(horizon=np.inf), "equilibrate: horizon must be finite and > 0"), (dict(horizon="long"), "equilibrate: horizon must be finite and > 0"),
           (dict(max_step=0.0), "equilibrate: max_step must be finite and > 0"), (dict(max_step=np.inf), "equilibrate: max_step must be finite and > 0"),
           (dict(max_steps=0), "equilibrate: max_steps must be an integer >= 1"), (dict(max_steps=10.0), "equilibrate: max_steps must be an integer >= 1"),
           (dict(max_steps=True), "equilibrate: max_steps must be an integer >= 1")]
    for eq, message in bad:
        with pytest.raises(ValueError, match="MassActionODELogLike: " + message):
            make(eq)
    # a condition's own: the same rules, and the message names the condition; a missing key or None inherits, False switches it off
    multi = lambda eq, **kw: MassActionODELogLike(*args, conditions=[dict(), dict(equilibrate=eq)], **kw)       # noqa: E731
    for eq, message in bad:
        with pytest.raises(ValueError, match="MassActionODELogLike: condition 1: " + message):
            multi(eq)
    m = MassActionODELogLike(*args, equilibrate=dict(max_steps=9), conditions=[dict(), dict(equilibrate=None), dict(equilibrate=False), dict(equilibrate=True)])
    assert [c.get("equilibrate", {}).get("max_steps") if c.get("equilibrate") else None for c in m.conditions] == [9, 9, None, 2000]
    assert "EQUILIBRATE = true" in m.source() and "EQUILIBRATE" not in multi(False).source()


@pytest.mark.parametrize("name", sorted(UNCHANGED))
def test_an_object_without_the_phase_is_the_object_it_always_was(name):
    """None, False, every condition off and the object built without the keyword: one source -- the parent commit's, by its sha256 --
    and one data block; so is an object unpickled from before the keyword existed."""
    make = UNCHANGED[name]
    plain = make()
    assert _sha(plain) == PARENT_SOURCE_SHA256[name] and "EQUILIBRATE" not in plain.source()
    variants = [make(equilibrate=None), make(equilibrate=False)]
    if plain.conditions is not None:
        off = [dict(cond, equilibrate=False) for cond in plain.conditions]
        variants.append(MassActionODELogLike(plain.n_species, plain.reactions, None, plain.t, plain.observables, None, None, conditions=off,
                                             equilibrate=None))
        variants.append(MassActionODELogLike(plain.n_species, plain.reactions, None, plain.t, plain.observables, None, None,
                                             conditions=[dict(cond, equilibrate=None) for cond in off], equilibrate=False))
    state = plain.__getstate__()
    state.pop("equilibrate")                                              # what an object from before the keyword lacks
    old = MassActionODELogLike.__new__(MassActionODELogLike)
    old.__dict__.update(state)
    loaded = pickle.loads(pickle.dumps(old))
    assert "equilibrate" not in loaded.__dict__ and loaded.equilibrate is None
    for like in variants + [loaded]:
        assert like.source() == plain.source() and like.data_block().tobytes() == plain.data_block().tobytes()
        assert like._unit() == plain._unit()                             # (the kernel cache's key: one entry)
    on = make(equilibrate=True)
    assert "EQUILIBRATE = true" in on.source() and len(on.data_block()) == len(plain.data_block()) + 6 * (len(plain.conditions or [0]))
    assert on.source().replace("    static constexpr bool EQUILIBRATE = true;\n", "") == plain.source()


def test_the_block_ends_with_the_six_doubles_of_the_phase():
    like = EQ.single("mm", equilibrate=dict(rtol=1e-5, atol=1e-7, horizon=3.0, max_step=50.0, max_steps=7), events=[EQ.BOLUS["mm"]])
    plain = EQ.plain_from(like, like.y0)
    assert like.data_block()[:-6].tobytes() == plain.data_block().tobytes()
    assert list(like.data_block()[-6:]) == [1.0, 1e-5, 1e-7, 3.0, 50.0, 7.0]
    multi, _ = EQ.conditions("mm")
    blk = multi.data_block()
    stride = int(blk[1])
    assert len(blk) == 2 + 3 * stride
    ends = blk[2:].reshape(3, stride)[:, -6:]
    assert list(ends[0]) == [0.0] * 6 and list(ends[1]) == list(ends[2]) == [1.0, multi.rtol, multi.atol, 10.0, 1e7, 2000.0]


# ---------------------------------------------------------------------------------------------------- the criterion and the conserved totals
@pytest.mark.parametrize("name,n,seed", [("mm", 60, 31), ("chain8", 40, 32), ("enzyme13", 30, 33), ("chain17", 30, 34)])
def test_the_resting_state_passes_the_test_restated_in_numpy_and_keeps_conserved_totals(name, n, seed):
    from scipy.linalg import null_space
    S, rx, y0, t, _, nominal, _, lanes = EQ.network(name)
    like = EQ.single(name)
    assert like.lanes_per_point == lanes
    eq = like.equilibrate
    X = NW.box_points(nominal, n, seed, width=1.0)
    y, attempts = like.steady_state(X, return_steps=True)
    assert y.shape == (n, S) and np.all(np.isfinite(y)) and np.all(attempts <= eq["max_steps"])
    args = [(S, rx, R.rate_constants(rx, x, "log10"), ys, eq["horizon"], eq["rtol"], eq["atol"]) for x, ys in zip(X, y)]
    drift = [_drift(*a) for a in args]
    print("%s: numpy's drift2 horizon^2 at the resting state, max over %d points: %.9f; attempted steps median %d, max %d"
          % (name, n, max(drift), np.median(attempts), attempts.max()))
    # The solver's own value passed <= 1.  numpy's differs in 10**x against dexp (2 ulp of a rate constant), in the order of the products
    # and of the sum (an ulp per operation, at most 4 factors and R terms): f_s, a difference of terms that cancel at rest, may be off by
    # that many ulp of the terms' magnitude, and the mean of squares by a few ulp of itself.
    ulps = 8 + len(rx)
    assert max(_drift(*a, ulps=ulps) for a in args) <= 1.0 + 64 * np.finfo(float).eps
    Wl = null_space(R.stoichiometry(S, rx)[0].astype(float).T).T            # rows: a basis of the conserved totals, W N = 0
    assert len(Wl) >= 1
    scale = np.abs(Wl) @ (like.atol + like.rtol * np.maximum(np.abs(y), np.abs(np.asarray(y0, dtype=float)))).T
    moved = np.abs(Wl @ (y - np.asarray(y0, dtype=float)).T)
    print("%s: %d conserved totals, largest change in units of |W| (atol + rtol |y|): %.3g" % (name, len(Wl), np.max(moved / scale)))
    assert np.all(moved <= scale)


# ---------------------------------------------------------------------------------------------------- the hand-over
@pytest.mark.parametrize("name,n", [("mm", 12), ("chain8", 8), ("enzyme13", 6), ("chain17", 4)])
@pytest.mark.parametrize("bolus", [False, True])
def test_the_hand_over_to_the_experiment_is_exact(name, n, bolus):
    """batch of the equilibrating object against the plain object started by hand from steady_state(x): the same bits, and the step
    counts differ by the phase's steps.  With a bolus at t0 the event is applied to the resting state."""
    nominal = EQ.network(name)[5]
    like = EQ.single(name, events=[EQ.BOLUS[name]] if bolus else ())
    X = NW.box_points(nominal, n, 35, width=1.0)
    y, attempts = like.steady_state(X, return_steps=True)
    value, steps = like.batch(X, return_steps=True)
    sim = like.simulate(X)
    assert np.all(np.isfinite(value)) and np.all(attempts > 0)
    for i, x in enumerate(X):
        plain = EQ.plain_from(like, y[i])
        assert "EQUILIBRATE" not in plain.source() and plain.source() == EQ.plain_from(like, y[0]).source()
        v, st = plain.batch(x[None], return_steps=True)
        assert v.tobytes() == value[i:i + 1].tobytes() and st[0] + attempts[i] == steps[i]
        assert plain.simulate(x[None]).tobytes() == sim[i:i + 1].tobytes()


# ---------------------------------------------------------------------------------------------------- an independent solver
def _radau_rest(S, rx, k, y0, horizon, rtol, atol):
    """Radau's state after a time long enough that it passes numpy's steady-state test"""
    span = 10.0 * horizon
    for _ in range(8):
        y = R.radau(S, rx, k, y0, [span])[0]
        if _drift(S, rx, k, y, horizon, rtol, atol) <= 1.0:
            return y
        span *= 10.0
    raise AssertionError("Radau did not come to rest")


def _radau_reference(args):
    """(S, reactions, y0, t, observables, bolus, horizon, tol, x) -> the observables [T, O]: Radau from y0 to rest (the test at a tenth
    of the tightest tolerance under test), the bolus, Radau on from t0; one argument, for a process pool"""
    S, rx, y0, t, obs, bolus, horizon, tol, x = args
    k = R.rate_constants(rx, x, "log10")
    rest = _radau_rest(S, rx, k, y0, horizon, 0.1 * tol, 0.1 * tol)
    return EV.piecewise_radau(S, rx, k, rest, t, [bolus]) @ np.asarray(obs, dtype=float).T


@pytest.mark.parametrize("name,n,seed", [("mm", 8, 41), ("chain8", 8, 42)])
def test_trajectories_agree_with_radau_run_to_rest_and_restarted_at_t0(name, n, seed):
    """Networks without a slow mode.  The measure and the bound of test_ode_events_cpu's Radau comparisons."""
    S, rx, y0, t, obs, nominal, _, _ = EQ.network(name)
    bolus = EQ.BOLUS[name]
    X = NW.box_points(nominal, n, seed, width=1.0)
    horizon = float(t[-1])
    with ProcessPoolExecutor(max(1, min(8, len(os.sched_getaffinity(0)))), mp_context=multiprocessing.get_context("fork")) as ex:
        refs = list(ex.map(_radau_reference, [(S, rx, y0, t, obs, bolus, horizon, 1e-9, x) for x in X]))
    errs = []
    for rtol in (1e-6, 1e-9):
        like = EQ.single(name, events=[bolus], rtol=rtol, atol=rtol, max_steps=20000, equilibrate=dict(max_steps=20000))
        assert like.equilibrate["horizon"] == horizon and like.equilibrate["rtol"] == rtol
        errs.append(max_rel_err(like, refs, X, rtol))
    print("%s equilibrated, then a bolus at t0, against Radau: max |sim - ref| / (rtol |ref| + rtol) at rtol 1e-6, 1e-9: %s" % (name, errs))
    assert errs[0] < 10 and errs[1] < 10


# ---------------------------------------------------------------------------------------------------- success and failure: the Brusselator
@pytest.mark.parametrize("y0", [(0.0, 0.0), (1.0, 1.0), (2.0, 0.5)])
def test_the_brusselator_comes_to_rest_below_the_hopf_point_and_fails_on_the_limit_cycle(y0):
    like = EQ.brusselator(list(y0))
    assert like.equilibrate["max_steps"] == 2000 and like.equilibrate["horizon"] == 10.0
    x = np.array([[1.0, 1.5, 1.0, 1.0], [1.0, 3.0, 1.0, 1.0]])
    y, attempts = like.steady_state(x, return_steps=True)
    value = like.batch(x)
    print("Brusselator from %s: B = 1.5 at rest %s after %d attempts; B = 3: %d attempts" % (y0, y[0], attempts[0], attempts[1]))
    # at rest: f = 0 to (atol + rtol |y|) sqrt(2) / horizon, and the Jacobian at (1, 1.5) has no small eigenvalue
    np.testing.assert_allclose(y[0], [1.0, 1.5], rtol=0, atol=1e-7)
    assert 0 < attempts[0] < 2000 and np.isfinite(value[0])
    assert np.all(np.isnan(y[1])) and attempts[1] == 2000 and value[1] == -np.inf and np.all(np.isnan(like.simulate(x)[1]))
    few = EQ.brusselator(list(y0), max_steps=17)
    assert few.steady_state(x, return_steps=True)[1].tolist() == [17, 17] and np.all(few.batch(x) == -np.inf)


# ---------------------------------------------------------------------------------------------------- conditions
@pytest.mark.parametrize("name,n", [("mm", 30), ("chain8", 12), ("enzyme13", 8)])
def test_conditions_equilibrate_on_their_own(name, n):
    """phase off / on / on with a bolus at t0: column c of batch_conditions is the single-condition object's value, bit for bit, and the
    sum runs from left to right; steady_state gives y0 where the phase is off and one state for the two conditions that have it."""
    S, _, y0, _, _, nominal, _, _ = EQ.network(name)
    multi, one = EQ.conditions(name)
    assert "EQUILIBRATE = true" in multi.source() and "EVENTS = 1" in multi.source()
    assert "EQUILIBRATE" not in one(0).source() and "EVENTS" not in one(1).source()
    X = NW.box_points(nominal, n, 36, width=1.0)
    terms = multi.batch_conditions(X)
    total, steps = multi.batch(X, return_steps=True)
    assert np.all(np.isfinite(terms)) and total.tobytes() == CN.left_to_right(terms).tobytes()
    all_steps = 0
    for c in range(3):
        v, st = one(c).batch(X, return_steps=True)
        assert v.tobytes() == terms[:, c].tobytes()
        assert one(c).simulate(X).tobytes() == np.ascontiguousarray(multi.simulate(X)[:, c]).tobytes()
        all_steps = all_steps + st
    assert np.array_equal(all_steps, steps)
    y, attempts = multi.steady_state(X, return_steps=True)
    assert y.shape == (n, 3, S) and np.all(y[:, 0] == np.asarray(y0, dtype=float)) and np.all(attempts[:, 0] == 0)
    assert y[:, 1].tobytes() == y[:, 2].tobytes() == one(1).steady_state(X).tobytes() and np.all(attempts[:, 1] > 0)
    assert one(0).steady_state(X).tobytes() == np.ascontiguousarray(y[:, 0]).tobytes()


def test_an_output_at_t0_shows_the_resting_state_after_the_bolus():
    """chain8 has an output at t0 = 0 and observes every species: the first row of simulate is steady_state with the bolus added"""
    multi, _ = EQ.conditions("chain8")
    X = NW.box_points(NW.CHAIN_NOMINAL, 10, 37, width=1.0)
    assert multi.t[0] == multi.t0
    y, sim = multi.steady_state(X), multi.simulate(X)
    _, s, factor, amount = EQ.BOLUS["chain8"]
    after = y[:, 2].copy()
    after[:, s] = factor * after[:, s] + amount
    assert sim[:, 0, 0].tobytes() == np.ascontiguousarray(y[:, 0]).tobytes()
    assert sim[:, 1, 0].tobytes() == np.ascontiguousarray(y[:, 1]).tobytes() and sim[:, 2, 0].tobytes() == after.tobytes()
    assert np.all(sim[:, 2, 0, s] > sim[:, 1, 0, s])


# ---------------------------------------------------------------------------------------------------- a starved phase
def test_a_starved_phase_fails_some_points_and_not_others():
    """The phase's own budget (EQ.MM_STARVED_EQUILIBRATE_STEPS attempted steps), the experiment's left at its default: the points that
    fail are those that need more attempts at the default budget, exactly."""
    n = EQ.MM_STARVED_EQUILIBRATE_STEPS
    X = NW.box_points(NW.MM_NOMINAL, 200, 5, width=1.0)
    starved, full = EQ.single("mm", equilibrate=dict(max_steps=n)), EQ.single("mm")
    need = full.steady_state(X, return_steps=True)[1]
    y, attempts = starved.steady_state(X, return_steps=True)
    failed = starved.batch(X) == -np.inf
    print("a phase of %d attempted steps: %d of %d points fail; at the default budget they need %d..%d attempts (median %d) and %d fail"
          % (n, failed.sum(), len(X), need.min(), need.max(), np.median(need), np.sum(full.batch(X) == -np.inf)))
    assert np.any(failed) and np.any(~failed) and not np.any(full.batch(X) == -np.inf)
    assert np.array_equal(failed, need > n) and np.all(attempts[failed] == n) and np.array_equal(attempts[~failed], need[~failed])
    assert np.all(np.isnan(y[failed])) and np.all(np.isfinite(y[~failed])) and np.all(np.isnan(starved.simulate(X)[failed]))
    # ... and under the three conditions with the experiment starved as well (ode_event_networks' limit): points that fail in all, in
    # some and in no condition -- the GPU test's case
    multi, _ = EQ.conditions("mm", equilibrate=dict(max_steps=n), max_steps=EV.MM_STARVED_MAX_STEPS)
    count = np.sum(multi.batch_conditions(NW.box_points(NW.MM_NOMINAL, 131, 21, width=1.0, outside=0.05)) == -np.inf, axis=1)
    assert np.any(count == 3) and np.any((count > 0) & (count < 3)) and np.any(count == 0)


# ---------------------------------------------------------------------------------------------------- the example
def test_the_examples_resting_receptor_is_ksyn_over_kdeg():
    from pydream_amd.examples.preequilibration import preequilibration_device as PE
    like = PE.make_likelihood()
    assert len(like.conditions) == len(PE.DOSES) and all(c["equilibrate"] for c in like.conditions) and "EQUILIBRATE = true" in like.source()
    X = PE.NOMINAL - 1 + 2 * np.random.default_rng(3).uniform(size=(100, len(PE.NOMINAL)))
    worst = PE.check_resting_state(like, np.vstack([PE.NOMINAL, X]))
    print("the example's resting receptor against k_syn / k_deg: %.4f of the steady-state test's bound" % worst)
    assert np.all(np.isfinite(like.batch(X))) and like(PE.NOMINAL) > np.max(like.batch(X))
    y = like.steady_state(PE.NOMINAL)
    np.testing.assert_allclose(y[0, :, PE.R], PE.resting_receptor(PE.NOMINAL), rtol=1e-6)
