"""A steady output, MassActionODELogLike(t=[..., inf], settle=...), without a GPU: the keyword and the times are checked; an object
whose t is finite is byte for byte the object it was on the commit before; the phase applied to the state at t_last gives the bits of the
equilibration phase of a second object started from that state (the hand-over identity); the settled state passes the steady-state test
restated in numpy and keeps the conserved totals; it lies within the test's own bound of an independent steady state (mpmath Newton on
the reference's right-hand side, closed forms); the steady row agrees with scipy's Radau at a late time; the order at t_last (output,
knots, events, then the phase with the inputs held); the Brusselator; a starved phase; every feature together in the four builds; the
kernels' registers; the example's closed form."""
import hashlib
import pickle

import numpy as np
import pytest

from pydream_amd import _ode_values
from pydream_amd import likelihoods as LK
from pydream_amd.likelihoods import Input, MassActionODELogLike

from . import ode_condition_networks as CN
from . import ode_equilibrate_networks as EQ
from . import ode_networks as NW
from . import ode_reference as R
from . import ode_settle_networks as SN
from . import test_ode_equilibrate_cpu as TEQ
from .ode_support import max_rel_err, notes

INF = np.inf
EPS = np.finfo(float).eps

# sha256 of data_block() of the networks of test_ode_equilibrate_cpu.PARENT_SOURCE_SHA256 on the commit before t could end in inf, with
# every entry unobserved (with_outputs(t): data NaN, sd 1) -- the block's layout and every number in it that does not come from scipy,
# whose Radau made the objects' own data and need not round alike on every machine; the objects' own blocks are compared with a
# restatement of that layout around their data
PARENT_BLOCK_SHA256 = {
    "chain17@32": "93dc3f8fb12c3f7ec91de3737b7388520f9b949a28e7a8467742a09c2fb9e150",
    "chain33@64": "f54936212925a1174b48bd9151cbde917a59473a58c8ec845d8dde352d2ff509",
    "chain8": "e9cc3e6cc8f7e56ade6b77182b178b3f38ce0465fa4e818fde5088330df7fab8",
    "enzyme13@16": "05990c240a85386328dfc0016acfa881364306e3673261424c2df10d3e9b6629",
    "mm": "88ee7f9a28f6ef65e795d894e27006bd295dac3ada7c339c88b6b7f1a49746d5",
    "mm x 3 with events": "7870d25a3918986b92ff5cfc8476ce9e4807582fa612509eca71b22b59456a03",
    "robertson": "df841d84ac00a8b0c32afceb049595c2993bcadc962a82a0766175ec6e52cdd3",
}


def _mm_args(t):
    data = np.ones((2, len(t)))
    return (4, NW.MM_REACTIONS, NW.MM_Y0, t, CN.MM_OBSERVABLES, data, data)


# ---------------------------------------------------------------------------------------------------- 1. the keyword and the times
def test_the_keyword_and_the_times_are_checked_at_construction():
    t = np.r_[NW.MM_T, INF]
    make = lambda st, t=t, **kw: MassActionODELogLike(*_mm_args(t), settle=st, **kw)      # noqa: E731
    assert LK.ODE_SETTLE_MAX_STEPS == 2000 and LK.ODE_SETTLE_MAX_STEPS is _ode_values.ODE_SETTLE_MAX_STEPS
    full = make(None, rtol=1e-6, atol=1e-9)
    assert full.t_last == 10.0 and full.settle == dict(rtol=1e-6, atol=1e-9, horizon=10.0, max_step=1e7, max_steps=2000) == make(True, rtol=1e-6, atol=1e-9).settle
    assert make(None, t0=-2.0).settle["horizon"] == 12.0 and make({}).settle["horizon"] == 10.0
    given = make(dict(rtol=1e-5, atol=np.float64(1e-7), horizon=3, max_step=np.float64(50.0), max_steps=np.int64(7))).settle
    assert given == dict(rtol=1e-5, atol=1e-7, horizon=3.0, max_step=50.0, max_steps=7)
    assert "SETTLE = true" in full.source() and "SETTLE" not in MassActionODELogLike(*_mm_args(NW.MM_T)).source()
    # the times: one inf, and it is the last
    for bad in ([0.5, INF, 1.0], [0.5, INF, INF], [INF, 0.5], [0.5, -INF], [0.5, np.nan], [-INF]):
        with pytest.raises(ValueError, match="output times must be finite, sorted and >= t0"):
            MassActionODELogLike(*_mm_args(np.array(bad)))
    # settle without an inf, settle=False with one: each refusal says which case it is
    for st in (True, {}, dict(horizon=2.0)):
        with pytest.raises(ValueError, match="settle is given but t does not end in inf"):
            make(st, t=NW.MM_T)
    assert make(None, t=NW.MM_T).settle is None and make(False, t=NW.MM_T).settle is None
    with pytest.raises(ValueError, match="settle=False but t ends in inf"):
        make(False)
    # t = [inf] alone: T = 1, and the horizon has no default
    for st in (None, True, {}, dict(max_steps=10)):
        with pytest.raises(ValueError, match='settle: "horizon" is required'):
            make(st, t=[INF])
    with pytest.raises(ValueError, match='settle: "horizon" is required'):
        make(None, t=[2.0, INF], t0=2.0)
    alone = make(dict(horizon=4.0), t=[INF])
    assert alone.t_last == 0.0 and alone.settle["horizon"] == 4.0 and alone.settle["max_step"] == 4e6 and len(alone.t) == 1
    bad = [(1, "settle must be None, True or a mapping"), ("yes", "settle must be None, True or a mapping"), (dict(tol=1e-6), "settle must be None, True or a mapping"),
           (dict(rtol=0.0), "settle: rtol must be finite and > 0"), (dict(atol=-1e-9), "settle: atol must be finite and > 0"),
           (dict(horizon=INF), "settle: horizon must be finite and > 0"), (dict(horizon=0.0), "settle: horizon must be finite and > 0"),
           (dict(max_step=0.0), "settle: max_step must be finite and > 0"), (dict(max_steps=0), "settle: max_steps must be an integer >= 1"),
           (dict(max_steps=2.5), "settle: max_steps must be an integer >= 1")]
    for st, message in bad:
        with pytest.raises(ValueError, match="MassActionODELogLike: " + message):
            make(st)
        with pytest.raises(ValueError, match="MassActionODELogLike: condition 1: " + message):
            MassActionODELogLike(*_mm_args(t), conditions=[dict(), dict(settle=st)])
    # events lie in [t0, t_last]; input tables cover [t0, t_last] (and need not reach further)
    assert make(None, events=[(10.0, 1, 1.0, 1.0)]).events == ((10.0, 1, 1.0, 1.0),)
    with pytest.raises(ValueError, match=r"event 0: the time must be finite and lie in t0 = 0.0 <= time <= t\[-1\] = 10.0"):
        make(None, events=[(10.5, 1, 1.0, 1.0)])
    with pytest.raises(ValueError, match="event 0: the time must be finite"):
        make(None, events=[(INF, 1, 1.0, 1.0)])
    rx5 = list(NW.MM_REACTIONS) + [({4: 1}, {4: 1, 0: 1}, 0.3)]
    five = lambda table: MassActionODELogLike(5, rx5, list(NW.MM_Y0) + [0.0], t, np.eye(5)[:2], np.ones((2, len(t))), 1.0,      # noqa: E731
                                              inputs=[Input(4, *table)])
    assert five(((0.0, 10.0), (0.0, 1.0))).inputs[0].times[-1] == 10.0
    with pytest.raises(ValueError, match="its table must cover t0 = 0.0 .. t"):
        five(((0.0, 9.0), (0.0, 1.0)))


def test_a_condition_inherits_the_constructors_settle_and_may_carry_its_own():
    t = np.r_[NW.MM_T, INF]
    m = MassActionODELogLike(*_mm_args(t), settle=dict(max_steps=9), conditions=[dict(), dict(settle=None), dict(settle=True), dict(settle=dict(horizon=2.0))])
    assert [c["settle"]["max_steps"] for c in m.conditions] == [9, 9, 2000, 2000] and [c["settle"]["horizon"] for c in m.conditions] == [10.0, 10.0, 10.0, 2.0]
    with pytest.raises(ValueError, match="condition 1: settle=False but t ends in inf"):
        MassActionODELogLike(*_mm_args(t), conditions=[dict(), dict(settle=False)])
    with pytest.raises(ValueError, match="condition 1: settle is given but t does not end in inf"):
        MassActionODELogLike(*_mm_args(NW.MM_T), conditions=[dict(), dict(settle=True)])
    # every experiment's block carries the phase's six doubles, its own
    blk = m.data_block()
    stride = int(blk[1])
    six = blk[2:].reshape(4, stride)[:, -6:]
    assert [list(r) for r in six] == [[1.0, m.rtol, m.atol, 10.0, 1e7, 9.0]] * 2 + [[1.0, m.rtol, m.atol, 10.0, 1e7, 2000.0], [1.0, m.rtol, m.atol, 2.0, 2e6, 2000.0]]
    assert np.all(blk[2:].reshape(4, stride)[:, 6 + 4 + len(t) - 1] == INF)


def test_an_object_with_a_steady_output_pickles_round_and_keeps_it_through_with_outputs():
    multi, _ = SN.mm_conditions(settle=dict(horizon=7.0))
    again = pickle.loads(pickle.dumps(multi))
    assert again.source() == multi.source() and again.data_block().tobytes() == multi.data_block().tobytes() and again.settle == multi.settle
    X = NW.box_points(NW.MM_NOMINAL, 5, 3, width=1.0)
    assert again.batch(X).tobytes() == multi.batch(X).tobytes()
    # with_outputs: the phase's settings carry over; a finite grid drops the phase; with the object's own t the same bits
    same = multi.with_outputs(multi.t)
    assert same.settle == multi.settle and same.simulate(X).tobytes() == multi.simulate(X).tobytes()
    dense = multi.with_outputs(np.r_[np.linspace(0.0, 10.0, 21), INF])
    assert dense.settle["horizon"] == 7.0 and "SETTLE = true" in dense.source()
    assert dense.simulate(X)[:, :, -1].tobytes() == multi.simulate(X)[:, :, -1].tobytes()
    finite = multi.with_outputs(np.linspace(0.0, 10.0, 21))
    assert finite.settle is None and "SETTLE" not in finite.source() and all("settle" not in c for c in finite.conditions)
    # an object from before the keyword existed
    state = NW.michaelis_menten().__getstate__()
    state.pop("settle")
    old = MassActionODELogLike.__new__(MassActionODELogLike)
    old.__dict__.update(state)
    loaded = pickle.loads(pickle.dumps(old))
    assert loaded.settle is None and loaded.source() == NW.michaelis_menten().source()
    assert loaded.data_block().tobytes() == NW.michaelis_menten().data_block().tobytes()
    with pytest.raises(ValueError, match="settled_state needs an object with a steady output"):
        loaded.settled_state(X)


# ---------------------------------------------------------------------------------------------------- 2. unchanged objects
def _parent_block(like, e):
    """One experiment's block as the commit before laid it out (csrc/dz_ode.h's head), for an object without noise, equilibration, inputs
    and views: header, y0, t, data and sd time-major, then with events their count and Emax records."""
    seen = np.isfinite(e["data"])
    C = float(np.sum(-np.log(e["sd"][seen]) - 0.5 * np.log(2 * np.pi)))
    blk = [[C, like.rtol, like.atol, float(like.max_steps), like.t0, float(len(like.t))], e["y0"], like.t,
           np.where(seen, e["data"], 0.0).T.reshape(-1), np.where(seen, e["sd"], INF).T.reshape(-1)]
    emax = max(len(x["events"]) for x in like._experiments())
    if emax:
        rec = np.zeros((emax, 4))
        rec[:len(e["events"])] = np.asarray(e["events"], dtype=float).reshape(-1, 4)
        blk += [[float(len(e["events"]))], rec.reshape(-1)]
    return np.concatenate(blk)


@pytest.mark.parametrize("name", sorted(TEQ.UNCHANGED))
def test_an_object_whose_t_is_finite_is_the_object_it_always_was(name):
    """(passes on the parent commit by design)"""
    make = TEQ.UNCHANGED[name]
    plain = make()
    assert hashlib.sha256(plain.source().encode()).hexdigest() == TEQ.PARENT_SOURCE_SHA256[name] and "SETTLE" not in plain.source()
    unobserved = plain.with_outputs(plain.t)
    assert hashlib.sha256(unobserved.data_block().tobytes()).hexdigest() == PARENT_BLOCK_SHA256[name]
    blocks = [_parent_block(plain, e) for e in plain._experiments()]
    head = [[float(len(blocks)), float(len(blocks[0]))]] if plain.conditions is not None else []
    assert plain.data_block().tobytes() == np.concatenate(head + blocks).tobytes()
    if name != "robertson":                                     # (the example's make_likelihood has no such keyword)
        assert make(settle=None).source() == plain.source() and make(settle=None).data_block().tobytes() == plain.data_block().tobytes()
        assert make(settle=None)._unit() == plain._unit()


def test_where_the_six_doubles_sit_in_the_block():
    """behind the equilibration's six, in front of the knots' count and records; tt[T-1] = +inf; the knots end with the held ones"""
    a = SN.input_held(True)
    S, T, O = 5, len(a.t), 5
    blk = a.data_block()
    base = 6 + S + T + 2 * T * O
    assert blk[6 + S + T - 1] == INF and list(blk[base:base + 6]) == [1.0, a.rtol, a.atol, 5.0, 5e6, 4000.0]
    K = int(blk[base + 6])
    knots = blk[base + 7:].reshape(-1, 4)
    # (t0, u(t0), first slope), the table's knot strictly inside (t0, t_last), then the held one: the value at t_last, slope 0
    assert K == 3 and len(blk) == base + 7 + 4 * K
    np.testing.assert_array_equal(knots, [[0.0, 0.0, 0.1, 0.225], [4.0, 0.0, 1.0, (0.8 - 1.0) / 2.0], [6.0, 0.0, 0.8, 0.0]])
    b = MassActionODELogLike(a.n_species, a.reactions, a.y0, a.t, a.observables, a.data, a.sd, inputs=a.inputs, settle=a.settle, equilibrate=dict(horizon=2.0),
                             events=[(1.5, 1, 1.0, 0.5)])
    blk = b.data_block()
    ev = base + 1 + 4
    assert list(blk[base:ev]) == [1.0, 1.5, 1.0, 1.0, 0.5] and blk[ev] == 1.0 and blk[ev + 3] == 2.0 and list(blk[ev + 6:ev + 12]) == [1.0, b.rtol, b.atol, 5.0, 5e6, 4000.0]
    assert blk[ev + 12] == 3.0 and len(blk) == ev + 13 + 12


# ---------------------------------------------------------------------------------------------------- 3. the hand-over identity
def _state_at_t_last(like, X):
    """The full state at t_last from objects with t = [.., t_last]: with identity observables where the shape's observable limit holds
    S of them, else from two objects that observe the first and the last 16 species (the observables do not enter the integration)."""
    S = like.n_species
    if S <= 16 or like.lanes_per_point == 1:
        return SN.finite_twin(like, np.eye(S)).simulate(X)[:, -1]
    lo, hi = SN.finite_twin(like, np.eye(S)[:16]).simulate(X)[:, -1], SN.finite_twin(like, np.eye(S)[S - 16:]).simulate(X)[:, -1]
    assert lo[:, S - 16:].tobytes() == hi[:, :32 - S].tobytes()
    return np.concatenate([lo, hi[:, 32 - S:]], axis=1)


@pytest.mark.parametrize("name,n", [("mm", 12), ("enzyme13", 6), ("chain17", 4)])
def test_the_phase_is_the_equilibration_of_a_second_object_started_from_the_state_at_t_last(name, n):
    S, _, _, _, obs, nominal, _, lanes = SN.network(name)
    obs = np.eye(S) if S <= 16 else obs
    like = SN.single(name, obs)
    X = NW.box_points(nominal, n, 35, width=1.0)
    y_last = _state_at_t_last(like, X)
    settled, attempts = like.settled_state(X, return_attempts=True)
    sim = like.simulate(X)
    value, steps = like.batch(X, return_steps=True)
    finite_steps = SN.finite_twin(like).batch(X, return_steps=True)[1]
    assert np.all(np.isfinite(value)) and np.any(attempts > 0)
    if S <= 16:
        assert sim[:, -2].tobytes() == y_last.tobytes()           # (identity observables: row T-2 is the state handed to the phase)
    for i, x in enumerate(X):
        twin = SN.equilibrating_from(like, y_last[i], obs)
        assert twin.equilibrate == like.settle and "SETTLE" not in twin.source()
        y2, a2 = twin.steady_state(x[None], return_steps=True)
        assert y2.tobytes() == settled[i:i + 1].tobytes() and a2[0] == attempts[i]
        assert twin.simulate(x[None])[0, 0].tobytes() == sim[i, -1].tobytes()
        assert finite_steps[i] + twin.batch(x[None], return_steps=True)[1][0] == steps[i]


# ---------------------------------------------------------------------------------------------------- 4. the test itself
@pytest.mark.parametrize("name,n,seed", [("mm", 60, 31), ("chain8", 40, 32), ("enzyme13", 30, 33), ("chain17", 30, 34)])
def test_the_settled_state_passes_the_test_restated_in_numpy_and_keeps_conserved_totals(name, n, seed):
    from scipy.linalg import null_space
    S, rx, y0, _, _, nominal, _, lanes = SN.network(name)
    like = SN.single(name)
    st = like.settle
    X = NW.box_points(nominal, n, seed, width=1.0)
    y, attempts = like.settled_state(X, return_attempts=True)
    steps = like.batch(X, return_steps=True)[1]
    assert y.shape == (n, S) and np.all(np.isfinite(y)) and np.all(attempts <= st["max_steps"])
    args = [(S, rx, R.rate_constants(rx, x, "log10"), ys, st["horizon"], st["rtol"], st["atol"]) for x, ys in zip(X, y)]
    print("%s: numpy's drift2 horizon^2 at the settled state, max over %d points: %.9f; attempted steps median %d, max %d"
          % (name, n, max(SN.drift(*a) for a in args), np.median(attempts), attempts.max()))
    ulps = 8 + len(rx)                                          # (test_ode_equilibrate_cpu's allowance, for the same reasons)
    assert max(SN.drift(*a, ulps=ulps) for a in args) <= 1.0 + 64 * EPS
    Wl = null_space(R.stoichiometry(S, rx)[0].astype(float).T).T            # rows: a basis of the conserved totals, W N = 0
    assert len(Wl) >= 1
    y0 = np.asarray(y0, dtype=float)
    total = np.abs(Wl) @ np.maximum(np.abs(y), np.abs(y0)).T                # [totals, n]
    moved = np.abs(Wl @ (y - y0).T)
    print("%s: %d conserved totals over %d..%d accepted steps, largest change in units of nsteps S eps total: %.3g"
          % (name, len(Wl), steps.min(), steps.max(), np.max(moved / (steps * S * EPS * total))))
    assert np.all(moved <= steps * S * EPS * total)


# ---------------------------------------------------------------------------------------------------- 5. an independent steady state
def _accuracy(like, rx, X, rate_scale="log10"):
    """max over the points of |y - y*|_2 / bound, bound = ||(J|_V)^-1|| sqrt(S) max_s(atol_ss + rtol_ss |y_s|) / horizon"""
    S, st = like.n_species, like.settle
    y = like.settled_state(X)
    assert np.all(np.isfinite(y))
    worst = 0.0
    for x, ys in zip(X, y):
        k = R.rate_constants(rx, x, rate_scale)
        star, inv = SN.newton_steady_state(S, rx, k, ys)
        bound = inv * np.sqrt(S) * np.max(st["atol"] + st["rtol"] * np.abs(ys)) / st["horizon"]
        worst = max(worst, float(np.linalg.norm(ys - star)) / bound)
    return worst, y


@pytest.mark.parametrize("name", ["cycle", "receptor", "enzyme13", "chain64"])
def test_the_settled_state_lies_within_the_tests_bound_of_an_independent_steady_state(name):
    """y* by mpmath Newton on the reference's right-hand side and Jacobian, restricted to the stoichiometric subspace, from the solver's
    state.  A state that passes the test has |f|_2 <= sqrt(S) max_s(atol_ss + rtol_ss |y_s|) / horizon, so to first order |y - y*|_2 <=
    ||(J|_V)^-1|| times that; twice the bound is asserted (the second-order term, rounding).  Measured error / bound, the worst point
    of each network: cycle 0.55, receptor 0.78, enzyme13@16 0.21, chain64@64 0.030."""
    if name == "cycle":
        like, rx, nominal, n = SN.cycle(), SN.CYCLE_REACTIONS, SN.CYCLE_NOMINAL, 12
    elif name == "receptor":
        like, rx, nominal, n = SN.receptor(), SN.RECEPTOR_REACTIONS, SN.RECEPTOR_NOMINAL, 12
    else:
        like = SN.single(name)
        rx, nominal, n = like.reactions, SN.network(name)[5], 4 if name == "enzyme13" else 2
    X = NW.box_points(nominal, n, 51, width=0.5)
    ratio, y = _accuracy(like, rx, X)
    print("%s: |settled - Newton's steady state| / bound, the worst of %d points: %.3g" % (name, n, ratio))
    assert ratio <= 2.0
    if name == "cycle":                                         # ... and the closed form, to the same bound's size
        closed = SN.cycle_closed_form(X)
        k1, k2 = 10.0 ** X[:, 0], 10.0 ** X[:, 1]
        bound = np.sqrt(3) * (like.settle["atol"] + like.settle["rtol"] * np.max(np.abs(y), axis=1)) / like.settle["horizon"] / (k1 * 1.5 + k2)
        assert np.all(np.abs(y[:, 1] - closed[:, 1]) <= 2 * bound) and np.all(y[:, 2] == 1.5)
    if name == "receptor":
        ksyn, kdeg, kon, koff, kint = (10.0 ** X).T
        Q = kon / (koff + kint)
        np.testing.assert_allclose(y[:, 0], ksyn / (kdeg + kint * Q * y[:, 1]), rtol=1e-6)
        np.testing.assert_allclose(y[:, 2], Q * y[:, 0] * y[:, 1], rtol=1e-6)
        np.testing.assert_allclose(y[:, 1] + y[:, 2], 1.0, rtol=1e-12)


# ---------------------------------------------------------------------------------------------------- 6. a late output
@pytest.mark.parametrize("name,n,seed", [("mm", 8, 41), ("chain8", 8, 42)])
def test_the_steady_row_agrees_with_radau_at_a_late_time(name, n, seed):
    """t_big: the first power of ten at which Radau's state passes numpy's drift test (the object's horizon and tolerances) at every
    point.  The measure and the bound of test_ode_equilibrate_cpu's Radau comparison, on the steady row."""
    S, rx, y0, t, obs, nominal, _, _ = SN.network(name)
    X = NW.box_points(nominal, n, seed, width=1.0)
    ks = [R.rate_constants(rx, x, "log10") for x in X]
    errs = []
    for rtol in (1e-6, 1e-9):
        like = SN.single(name, rtol=rtol, atol=rtol, max_steps=20000, settle=dict(max_steps=20000))
        assert like.settle["horizon"] == float(t[-1]) and like.settle["rtol"] == rtol
        t_big, ys = SN.first_t_big(S, rx, ks, y0, like.settle["horizon"], rtol, rtol)
        refs = [y[None] @ obs.T for y in ys]
        steady = like.with_outputs([INF])
        errs.append(max_rel_err(steady, refs, X, rtol))
        print("%s at rtol %g: t_big = %g" % (name, rtol, t_big))
    print("%s, the steady row against Radau at t_big: max |sim - ref| / (rtol |ref| + rtol) at rtol 1e-6, 1e-9: %s" % (name, errs))
    assert errs[0] < 10 and errs[1] < 10


# ---------------------------------------------------------------------------------------------------- 7. the order at t_last
def test_an_event_at_t_last_changes_the_steady_row_and_not_the_row_before():
    S, rx, y0, t, obs, nominal, _, _ = SN.network("mm", identity=True)
    t_last = float(t[-1])
    X = NW.box_points(nominal, 10, 36, width=1.0)
    plain = SN.single("mm", obs)
    late = SN.single("mm", obs, events=[(t_last, 3, 0.0, 0.0), (t_last, 1, 1.0, 1.0)])
    a, b = plain.simulate(X), late.simulate(X)
    assert np.all(np.isfinite(a)) and np.all(np.isfinite(b))
    assert a[:, :-1].tobytes() == b[:, :-1].tobytes()                                   # measured, then intervened
    # product washed out, substrate added: the steady state holds one unit of product (all substrate converted) instead of the lot
    assert np.all(np.abs(b[:, -1, 3] - (a[:, -2, 1] + a[:, -2, 2] + 1.0)) < 1e-5) and np.all(np.abs(a[:, -1, 3] - 2.0) < 1e-5)
    # the phase starts from the state after the events, in the order given: the hand-over identity on that state
    after = a[:, -2].copy()
    after[:, 3] = 0.0 * after[:, 3] + 0.0
    after[:, 1] = 1.0 * after[:, 1] + 1.0
    for i, x in enumerate(X[:4]):
        twin = SN.equilibrating_from(late, after[i])
        assert twin.steady_state(x[None]).tobytes() == late.settled_state(x[None]).tobytes()
    # in the finite object the same events have no effect at all
    assert SN.finite_twin(late).batch(X).tobytes() == SN.finite_twin(plain).batch(X).tobytes()


def test_inputs_are_held_at_their_value_at_t_last_with_drive_zero():
    """a knot ON t_last sets the held value; the table's slope after t_last does not matter: the bits of the object whose table is
    constant after t_last; and the input's own steady row is the knot's value exactly"""
    ramp, flat = SN.input_held(True), SN.input_held(False)
    X = NW.box_points(NW.MM_NOMINAL, 10, 37, width=1.0)
    a, b = ramp.simulate(X), flat.simulate(X)
    assert np.all(np.isfinite(a)) and a.tobytes() == b.tobytes() and ramp.batch(X).tobytes() == flat.batch(X).tobytes()
    # the output at t_last is taken BEFORE the knot there (the integrated ramp, to rounding); the steady row sees the knot's value exactly
    assert np.all(a[:, -1, 4] == 0.8) and np.all(np.abs(a[:, -2, 4] - 0.8) < 1e-12) and np.all(np.abs(a[:, 0, 4] - 0.325) < 1e-12)
    # drive 0: the enzyme settles at production / degradation under the held input, 0.3 * 0.8 / 0.4 (all substrate gone, no complex)
    y = ramp.settled_state(X)
    assert np.all(np.abs(y[:, 0] - 0.6) < 1e-5) and np.all(np.abs(y[:, 2]) < 1e-5)
    # t_last between two table knots: the held value is the table's value there
    rx, table = ramp.reactions, ((0.0, 4.0, 9.0), (0.1, 1.0, 0.2))
    mid = MassActionODELogLike(5, rx, ramp.y0, ramp.t, np.eye(5), ramp.data, ramp.sd, inputs=[Input(4, *table)], settle=ramp.settle)
    held = 1.0 + (6.0 - 4.0) * ((0.2 - 1.0) / 5.0)
    assert np.all(mid.simulate(X)[:, -1, 4] == held) and abs(held - 0.68) < 1e-12


# ---------------------------------------------------------------------------------------------------- 8. failure
@pytest.mark.parametrize("y0", [(0.0, 0.0), (2.0, 0.5)])
def test_the_brusselator_settles_below_the_hopf_point_and_fails_on_the_limit_cycle(y0):
    t = np.r_[EQ.BRUSSELATOR_T, INF]
    make = lambda **st: MassActionODELogLike(2, EQ.BRUSSELATOR_REACTIONS, list(y0), t, np.eye(2), np.ones((2, len(t))), 1.0,      # noqa: E731
                                             rate_scale="linear", settle=dict(horizon=10.0, **st))
    like = make()
    x = np.array([[1.0, 1.5, 1.0, 1.0], [1.0, 3.0, 1.0, 1.0]])
    y, attempts = like.settled_state(x, return_attempts=True)
    value, sim = like.batch(x), like.simulate(x)
    print("Brusselator from %s: B = 1.5 settles at %s after %d attempts; B = 3: %d attempts" % (y0, y[0], attempts[0], attempts[1]))
    np.testing.assert_allclose(y[0], [1.0, 1.5], rtol=0, atol=1e-7)
    assert 0 <= attempts[0] < 2000 and np.isfinite(value[0]) and np.all(np.isfinite(sim[0])) and np.array_equal(sim[0, -1], y[0])
    assert np.all(np.isnan(y[1])) and attempts[1] == 2000 and value[1] == -INF and np.all(np.isnan(sim[1]))
    few = make(max_steps=17)
    assert few.settled_state(x, return_attempts=True)[1][1] == 17 and few.batch(x)[1] == -INF


@pytest.mark.parametrize("name", ["mm", SN.WAVE])
def test_a_starved_phase_fails_a_quarter_and_settles_a_quarter(name):
    n = SN.STARVED_SETTLE_STEPS[name]
    X = SN.starved_points(name)
    starved, full = SN.starved(name), SN.single(name)
    need = full.settled_state(X, return_attempts=True)[1]
    y, attempts = starved.settled_state(X, return_attempts=True)
    value = starved.batch(X)
    failed = value == -INF
    print("%s, a phase of %d attempted steps: %d of %d points fail; at the default budget they need %d..%d attempts (median %d)"
          % (name, n, failed.sum(), len(X), need.min(), need.max(), np.median(need)))
    assert len(X) == 259 and failed.sum() >= 65 and (~failed).sum() >= 65 and not np.any(full.batch(X) == -INF)
    assert np.array_equal(failed, need > n) and np.all(attempts[failed] == n) and np.array_equal(attempts[~failed], need[~failed])
    sim = starved.simulate(X)
    assert np.all(np.isnan(y[failed])) and np.all(np.isfinite(y[~failed])) and np.all(np.isnan(sim[failed])) and np.all(np.isfinite(sim[~failed]))
    assert y[~failed].tobytes() == full.settled_state(X)[~failed].tobytes()


def test_fixed_steps_ignores_the_phase_as_it_ignores_events():
    """to a finite t1 the bits of the object without the steady row, whatever is due at t_last; to t1 = inf (the steady row's time) NaN"""
    like, (multi, _) = SN.single("mm"), SN.mm_conditions()
    x = NW.MM_NOMINAL
    plain = SN.finite_twin(like).fixed_steps(x, 10.0, 50)
    assert np.all(np.isfinite(plain)) and like.fixed_steps(x, 10.0, 50).tobytes() == plain.tobytes()
    assert multi.fixed_steps(x, 10.0, 50, condition=2).tobytes() == plain.tobytes()          # (condition 2: events at t_last)
    assert like.fixed_steps(x, 10.0, 50, embedded=True).tobytes() == SN.finite_twin(like).fixed_steps(x, 10.0, 50, embedded=True).tobytes()
    for obj, kw in ((like, {}), (multi, dict(condition=2))):
        assert np.all(np.isnan(obj.fixed_steps(x, INF, 10, **kw))) and obj.fixed_steps(x, INF, 10, **kw).shape == (4,)


# ---------------------------------------------------------------------------------------------------- 9. everything together
@pytest.mark.parametrize("lanes", [1, 16, 32, 64])
def test_every_feature_together_with_the_steady_row(lanes):
    """conditions, a Monomial y0, events, equilibrate, Hill rate laws, sampled noise, inputs, a condition's "params" and the steady row
    in one object: every condition's term, simulate slice and settled state are the single-condition object's at the viewed row"""
    case = SN.steady_case(lanes)
    like = case.steady_like()
    src = like.source()
    for member in ("SETTLE = true", "EQUILIBRATE = true", "EVENTS = ", "VIEW = ", "NOISE = true", "INPUTS = ", "MONOMIALS = true", "SLOTS = "):
        assert member in src, member
    X = case.points(5 if lanes == 64 else 12, 5)
    terms, sim = like.batch_conditions(X), like.simulate(X)
    settled = like.settled_state(X)
    total, steps = like.batch(X, return_steps=True)
    assert np.all(np.isfinite(terms)) and total.tobytes() == CN.left_to_right(terms).tobytes() and sim.shape[2] == len(case.t)
    all_steps = 0
    for c in range(3):
        one, Xc = case.steady_single(c), np.ascontiguousarray(case.viewed(X, c))
        v, st = one.batch(Xc, return_steps=True)
        assert v.tobytes() == np.ascontiguousarray(terms[:, c]).tobytes()
        assert one.simulate(Xc).tobytes() == np.ascontiguousarray(sim[:, c]).tobytes()
        assert one.settled_state(Xc).tobytes() == np.ascontiguousarray(settled[:, c]).tobytes()
        all_steps = all_steps + st
    assert np.array_equal(all_steps, steps)
    # the steady row differs from the last finite one, and moves with the condition
    assert np.all(np.abs(sim[:, :, -1, 1] - sim[:, :, -2, 1]) > 1e-6)
    # with_outputs([.., inf]) on the object's own times: the same bits in every row (another grid clips other steps, so its rows agree
    # to the tolerance and not to the bit, as for every with_outputs)
    again = like.with_outputs(case.t)
    assert again.simulate(X).tobytes() == sim.tobytes() and [c["settle"] for c in again.conditions] == [c["settle"] for c in like.conditions]
    coarse = like.with_outputs(np.r_[case.t[1:-1:2], INF]).simulate(X)
    np.testing.assert_allclose(coarse, sim[:, :, np.r_[1:len(case.t) - 1:2, len(case.t) - 1]], rtol=1e-4, atol=1e-6)


# ---------------------------------------------------------------------------------------------------- 10. registers
REGISTER_CASES = {"mm": "mm", "enzyme13@16": "enzyme13", "chain17@32": "chain17", "chain33@64": SN.WAVE}


@pytest.mark.parametrize("label", sorted(REGISTER_CASES))
def test_the_kernels_with_the_phase_keep_their_scratch(label):
    """cross-compiled for gfx950: VGPRs, scratch and LDS with the phase beside the same network without it; scratch stays 0 wherever it
    is 0 without the phase"""
    name = REGISTER_CASES[label]
    like = SN.single(name)
    with_phase, without = notes(like.code_object()), notes(SN.finite_twin(like).code_object())
    print("%-12s with the phase: vgpr %d agpr %d scratch %d lds %d; without: vgpr %d agpr %d scratch %d lds %d"
          % (label, with_phase["vgpr"], with_phase["agpr"], with_phase["scratch"], with_phase["lds"], without["vgpr"], without["agpr"], without["scratch"],
             without["lds"]))
    if without["scratch"] == 0:
        assert with_phase["scratch"] == 0
    assert with_phase["lds"] == without["lds"]


def test_the_examples_steady_states_are_the_closed_form():
    from pydream_amd.examples.steady_dose import steady_dose_device as SD
    like = SD.make_likelihood()
    assert "SETTLE = true" in like.source() and len(like.conditions) == len(SD.DOSES) and np.isinf(like.t[-1])
    X = SD.NOMINAL - 1 + 2 * np.random.default_rng(3).uniform(size=(100, len(SD.NOMINAL)))
    worst = SD.check_closed_form(like, np.vstack([SD.NOMINAL, X]))
    print("the example's steady states against Xtot k1 E / (k1 E + k2): %.4f of the steady-state test's bound" % worst)
    assert worst <= 2.0 and np.all(np.isfinite(like.batch(X))) and like(SD.NOMINAL) > np.max(like.batch(X))
