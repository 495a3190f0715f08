"""Saturating rate laws (likelihoods.RateLaw, likelihoods.Hill) in the four host builds of MassActionODELogLike, against references that
share no code with them (tests/ode_ratelaw_reference.py): the reference's own Jacobian against mpmath.diff, fixed Rodas4 steps against the
40-digit restatement at the tolerance its float64 restatement sizes, the adaptive path against scipy's Radau, the linear invariants,
composition with conditions, events, equilibration and a Monomial K, the edges of the liveness rule, that nothing existing moved
(sources, data blocks and the kernels' registers, scratch and LDS are the parent commit's), the new kernels' resources and the example.

Faults seeded in a scratch copy of the generators (never committed), and what caught them.  (A) the factor n dropped from a Hill
derivative (_hill_slope's numerator without `n.0 *`): the fixed-step test fails on all 14 grammar networks and on goodwin8 and activated
(the two named networks with n > 1), deviation 1e9 .. 6e11 tolerances; the adaptive test fails on the same 16 (9 .. 46 tolerances
from Radau at 1e-6 and 300 .. 1500 at 1e-9, where it should gain three digits); the invariant test fails on all 14 because the step
budget of the default settings runs out (states not finite); the event and the Monomial-K compositions and the example fail too.
(B) the sign of the repression derivative flipped: fixed steps fail on all 14 grammar networks and on goodwin8, 1e10 .. 8e11
tolerances; the adaptive test on the same 15 (8 .. 91 and 260 .. 2900 tolerances); invariants on 13 (not finite); the event
composition and the example.  mm2, mm_enzyme and activated, which have no repression, pass.  (C) the product-rule term dropped for a
species that is in `order` and in a factor (_rate_slope keeping only the mass-action term there): fixed steps fail on the 13 grammar
networks that drew an order_and_factor reaction, 4e9 .. 3e11 tolerances, the adaptive test on the same 13 (4 .. 32 and 130 .. 1000
tolerances), invariants on 12 of them (not finite); rl-S6R16@1, which drew none, and the named networks pass.  The tolerance of the
fixed-step test is about 1e-14 throughout, the faulty deviations 6e-5 .. 5e-3.
"""
import hashlib
import pickle

import numpy as np
import pytest

from pydream_amd.likelihoods import (ODE_GROUP_LIMITS, ODE_LIMITS, ODE_MAX_HILL_EXPONENT, ODE_MAX_RATE_FACTORS, ODE_WAVE_LIMITS, Hill,
                                     MassActionODELogLike, Monomial, RateLaw)

from . import ode_ratelaw_networks as RN
from . import ode_ratelaw_reference as RR
from . import ode_reference as REF
from .ode_support import notes

EPS = np.finfo(float).eps
INDEX = list(range(len(RN.CASES)))
IDS = [RN.network(i).name for i in INDEX]
N_POINTS = 2
_REPLACED, _NETS, _RADAU = set(), {}, {}


def resolved(i):
    """Case i's network, with Radau's states [point, T, S] at its box points; the next seed takes its place only if Radau fails on it."""
    if i not in _NETS:
        for bump in (0, 1):
            net = RN.network(i, bump)
            try:
                _RADAU[i] = np.array([RR.radau(net.S, RR.resolve(net.reactions, x, net.rate_scale), net.y0, RN.T_OUT) for x in net.points(N_POINTS)])
            except AssertionError:
                _REPLACED.add(i)
                continue
            _NETS[i] = net
            break
    return _NETS[i], _RADAU[i]


def _named(name):
    spec = RN.NAMED[name]
    return spec, spec["nominal"]


# ---------------------------------------------------------------------------------------------------- the reference itself
@pytest.mark.parametrize("i", INDEX, ids=IDS)
def test_the_references_jacobian_is_the_derivative_of_its_right_hand_side(i):
    """mpmath.diff at 30 digits: every column up to 8 species, six columns of species that a Hill factor reads in the larger networks"""
    net = RN.network(i)
    res = RR.resolve(net.reactions, net.nominal(), net.rate_scale)
    columns = None if net.S <= 8 else sorted({f.species for f in RN.hill_factors(net)})[:6]
    err = RR.jacobian_error(net.S, res, net.y0 + 0.1, columns=columns)
    assert err < 1e-20, err


@pytest.mark.parametrize("name", sorted(RN.NAMED))
def test_the_references_jacobian_on_the_named_networks(name):
    spec, x = _named(name)
    assert RR.jacobian_error(spec["S"], RR.resolve(spec["reactions"], x, "log10"), np.asarray(spec["y0"]) + 0.1) < 1e-20


def test_the_grammar_covers_what_it_is_meant_to():
    nets = [RN.network(i) for i in INDEX]
    assert not RN.coverage_gaps(nets), RN.coverage_gaps(nets)
    assert all(1 <= f.n <= 4 for n in nets for f in RN.hill_factors(n)) and {f.n for n in nets for f in RN.hill_factors(n)} == {1, 2, 3, 4}
    assert any(f.n == 8 for f in RN.GOODWIN8["reactions"][0][2].factors)
    assert sorted({c[1] for c in RN.CASES if c[0] == 16}) == [9, 13] and sorted({c[1] for c in RN.CASES if c[0] == 32}) == [17, 20]
    assert {c[1] for c in RN.CASES if c[0] == 64} == {33} and all(2 <= c[1] <= 8 for c in RN.CASES if c[0] == 1)


# ---------------------------------------------------------------------------------------------------- 1. fixed steps
def _check_fixed_steps(like, S, reactions, x, y0, label):
    res = RR.resolve(reactions, x, "linear")
    worst = 0.0
    for n in (4, 16):
        for embedded in (False, True):
            ref, scale, tol = RR.fixed_step_reference(S, res, y0, 0.0, 1.0, n, embedded)
            assert all(np.isfinite(float(v)) for v in ref) and float(scale) <= 1e3 * np.max(y0)      # (the input is tame: on the reference)
            dev = RR.deviation(like.fixed_steps(x, 1.0, n, embedded), ref, scale)
            worst = max(worst, dev / tol)
            assert dev <= tol, (label, n, embedded, dev, tol)
    return worst


@pytest.mark.parametrize("i", INDEX, ids=IDS)
def test_fixed_steps_equal_the_mp_restatement_to_rounding(i):
    net, _ = resolved(i)
    x = net.nominal("linear")
    worst = _check_fixed_steps(net.like(rate_scale="linear"), net.S, net.reactions, x, net.y0, net.name)
    print("%s: largest deviation / tolerance %.3f" % (net.name, worst))


@pytest.mark.parametrize("name", sorted(RN.NAMED))
def test_fixed_steps_of_the_named_networks(name):
    spec, x = _named(name)
    x = 10.0 ** x
    worst = _check_fixed_steps(RN.build(spec, rate_scale="linear"), spec["S"], spec["reactions"], x, np.asarray(spec["y0"], dtype=float), name)
    print("%s: largest deviation / tolerance %.3f" % (name, worst))


# ---------------------------------------------------------------------------------------------------- 2. the adaptive path
def _radau_errors(states_at, refs):
    errs = []
    for rtol in (1e-6, 1e-9):
        sim = states_at(rtol)
        assert np.all(np.isfinite(sim))
        errs.append(float(np.max(np.abs(sim - refs) / (rtol * np.abs(refs) + rtol))))
    assert errs[0] < 10 and errs[1] < 10, errs
    assert errs[1] * 1e-9 < 1e-2 * errs[0] * 1e-6, errs
    return errs


@pytest.mark.parametrize("i", INDEX, ids=IDS)
def test_adaptive_path_is_within_ten_tolerances_of_radau(i):
    net, refs = resolved(i)
    assert np.max(np.abs(refs - net.y0)) > 1e-3                               # (the reference moves: there is something to integrate)
    X = net.points(N_POINTS)
    errs = _radau_errors(lambda rtol: net.states(X, rtol=rtol, atol=rtol, max_steps=20000), refs)
    print("%s: Radau error in tolerances at 1e-6, 1e-9: %.3f %.3f" % (net.name, errs[0], errs[1]))


@pytest.mark.parametrize("name", sorted(RN.NAMED))
def test_adaptive_path_of_the_named_networks(name):
    spec, x = _named(name)
    X = np.array([x, x + 0.2])
    obs = spec["obs"]
    refs = np.array([RR.radau(spec["S"], RR.resolve(spec["reactions"], p, "log10"), spec["y0"], spec["t"]) @ np.asarray(obs).T for p in X])
    assert np.max(np.abs(refs - refs[:, :1])) > 1e-3
    errs = _radau_errors(lambda rtol: RN.build(spec, rtol=rtol, atol=rtol, max_steps=20000).simulate(X), refs)
    print("%s: Radau error in tolerances at 1e-6, 1e-9: %.3f %.3f" % (name, errs[0], errs[1]))


def test_at_most_two_networks_were_replaced_and_the_grammar_is_still_covered():
    nets = [resolved(i)[0] for i in INDEX]
    assert len(_REPLACED) <= 2, _REPLACED
    assert not RN.coverage_gaps(nets), RN.coverage_gaps(nets)


# ---------------------------------------------------------------------------------------------------- 3. invariants
@pytest.mark.parametrize("i", INDEX, ids=IDS)
def test_linear_invariants_hold_to_rounding_at_the_default_tolerance(i):
    from scipy.linalg import null_space
    net, _ = resolved(i)
    N, _ = REF.stoichiometry(net.S, net.reactions)
    Cn = null_space(N.T.astype(float))
    y = net.states(net.points(N_POINTS))
    assert np.all(np.isfinite(y))
    worst = 0.0
    for c in Cn.T:
        drift = np.max(np.abs((y - net.y0) @ c))
        bound = 1e3 * EPS * np.sum(np.abs(c)) * max(np.max(np.abs(y)), np.max(net.y0))
        worst = max(worst, drift / bound)
        assert drift <= bound, (net.name, drift, bound)
    print("%s: %d invariants, largest drift / bound %.4f" % (net.name, Cn.shape[1], worst))


# ---------------------------------------------------------------------------------------------------- 4. composition
COMPOSED = {"conditions": (RN.padded(RN.MM_ENZYME, 9, 16), dict()), "event": (RN.GOODWIN8, dict()), "equilibrate": (RN.MM_ENZYME, dict()),
            "monomial_K": (RN.ACTIVATED, dict())}
CONDITION_Y0 = [[0.5, 3.0, 0.0], [0.2, 5.0, 0.0], [1.0, 1.0, 0.5]]
EVENTS = [(0.0, 2, 1.0, 0.5), (2.2, 0, 0.5, 0.0), (4.0, 2, 0.0, 0.0)]          # at t0, between two outputs, and on an output time (t[7] = 4.0)


def test_composition_with_conditions():
    spec = COMPOSED["conditions"][0]
    x = spec["nominal"]
    X = np.array([x, x - 0.15])
    starts = [y + [0.0] * (spec["S"] - 3) for y in CONDITION_Y0]
    refs = np.array([[RR.radau(spec["S"], RR.resolve(spec["reactions"], p, "log10"), y0, spec["t"]) @ spec["obs"].T for y0 in starts] for p in X])
    rng = np.random.default_rng(3)
    data = refs[0] * (1 + 0.05 * rng.normal(size=refs[0].shape))                  # [C, T, O]
    conds = [dict(y0=y0, data=data[c].T, sd=0.05 * np.abs(data[c].T) + 0.01) for c, y0 in enumerate(starts)]
    made = lambda rtol: RN.build(spec, y0=None, data=None, sd=None, conditions=conds, rtol=rtol, atol=rtol, max_steps=20000)      # noqa: E731
    _radau_errors(lambda rtol: made(rtol).simulate(X), refs)
    like = made(1e-9)
    terms, total = like.batch_conditions(X), like.batch(X)
    assert np.all(np.isfinite(terms))
    summed = terms[:, 0].copy()
    for c in range(1, terms.shape[1]):
        summed = summed + terms[:, c]
    assert summed.tobytes() == total.tobytes()
    for c, cond in enumerate(conds):                                               # a condition alone gives its term's bits
        alone = RN.build(spec, y0=cond["y0"], data=cond["data"], sd=cond["sd"], rtol=1e-9, atol=1e-9, max_steps=20000)
        assert alone.batch(X).tobytes() == terms[:, c].tobytes()


def test_composition_with_an_event():
    spec = COMPOSED["event"][0]
    assert spec["t"][7] == 4.0
    x = spec["nominal"]
    X = np.array([x, x + 0.1])
    refs = np.array([RR.piecewise_radau(spec["S"], RR.resolve(spec["reactions"], p, "log10"), spec["y0"], spec["t"], EVENTS) for p in X])
    plain = RR.radau(spec["S"], RR.resolve(spec["reactions"], x, "log10"), spec["y0"], spec["t"])
    assert np.max(np.abs(plain - refs[0])) > 0.05                                  # (the events change the course)
    _radau_errors(lambda rtol: RN.build(spec, events=EVENTS, rtol=rtol, atol=rtol, max_steps=20000).simulate(X), refs)


def test_composition_with_equilibration():
    spec = COMPOSED["equilibrate"][0]
    x = spec["nominal"]
    X = np.array([x, x + 0.1])
    y0 = [0.0, 0.0, 0.0]                                                           # the enzyme's level 0.2 / k_deg is set by the point; no substrate at rest
    bolus = [(0.0, 1, 1.0, 3.0)]
    rest = np.array([RR.steady_state(spec["S"], RR.resolve(spec["reactions"], p, "log10"), y0) for p in X])
    assert np.allclose(rest[:, 0], 0.2 / 10.0 ** X[:, 2], rtol=1e-9) and np.all(np.abs(rest[:, 1:]) < 1e-12)
    refs = np.array([RR.piecewise_radau(spec["S"], RR.resolve(spec["reactions"], p, "log10"), r, spec["t"], bolus) @ spec["obs"].T for p, r in zip(X, rest)])
    made = lambda rtol: RN.build(spec, y0=y0, events=bolus, rtol=rtol, atol=rtol, max_steps=20000,      # noqa: E731
                                 equilibrate=dict(rtol=rtol * 1e-2, atol=rtol * 1e-2, max_steps=20000))
    _radau_errors(lambda rtol: made(rtol).simulate(X), refs)
    ss = made(1e-9).steady_state(X)
    assert np.all(np.abs(ss - rest) <= 1e-6 * (np.abs(rest) + 1))


def test_composition_with_a_monomial_K():
    spec = COMPOSED["monomial_K"][0]
    x = spec["nominal"]
    X = np.array([x, x + np.array([0.0, 0.3, -0.2])])
    refs = np.array([RR.radau(spec["S"], RR.resolve(spec["reactions"], p, "log10"), spec["y0"], spec["t"]) for p in X])
    assert np.max(np.abs(refs[0] - refs[1])) > 1e-2                                # (K moves with the second and the third coordinate)
    for scale in ("log10", "linear"):                                              # (a Monomial's value does not depend on rate_scale: x[0] does)
        Xs = X.copy()
        if scale == "linear":
            Xs[:, 0] = 10.0 ** X[:, 0]
        _radau_errors(lambda rtol: RN.build(spec, rate_scale=scale, rtol=rtol, atol=rtol, max_steps=20000).simulate(Xs), refs)
    assert RN.build(spec).d == 3


# ---------------------------------------------------------------------------------------------------- 5. edges
LANE_SPECS = {1: RN.MM2, 16: RN.padded(RN.MM2, 9, 16), 32: RN.padded(RN.MM2, 17, 32), 64: RN.padded(RN.MM2, 33, 64)}


@pytest.mark.parametrize("lanes", sorted(LANE_SPECS))
def test_edge_a_sampled_K_that_is_not_positive_or_not_finite_rejects_the_point(lanes):
    spec = LANE_SPECS[lanes]
    like = RN.build(spec, rate_scale="linear")
    good = 10.0 ** spec["nominal"]
    for bad in (0.0, -0.0, -0.6, -1e-300, np.inf, -np.inf, np.nan):
        X = np.array([good, [good[0], bad], good * 1.1])
        out = like.batch(X)
        assert out[1] == -np.inf and np.isfinite(out[0]) and np.isfinite(out[2]), (bad, out)
    for bad in (np.inf, -np.inf, np.nan):                                          # a coordinate that is not finite, in either scale
        assert RN.build(spec).batch(np.array([[spec["nominal"][0], bad]]))[0] == -np.inf
        assert like.batch(np.array([[bad, good[1]]]))[0] == -np.inf
    over = RN.build(dict(spec, reactions=[({0: 1}, {1: 1}, RateLaw(0, [Hill(0, 1, 8)], order={}))] + list(spec["reactions"][1:])), rate_scale="linear")
    assert over.batch(np.array([[good[0], 1e39]]))[0] == -np.inf                 # K finite, K^8 not
    assert over.batch(np.array([[good[0], 1e-50]]))[0] == -np.inf                # K > 0, K^8 = 0
    assert np.isfinite(over.batch(np.array([[good[0], 2.0]]))[0])


@pytest.mark.parametrize("lanes", sorted(LANE_SPECS))
def test_edge_an_empty_hill_species(lanes):
    """y0 = 0 on the Hill species and nothing that makes it: activation contributes 0, repression contributes k"""
    S = LANE_SPECS[lanes]["S"]
    t = np.array([0.5, 1.0, 2.0])
    pad = [({s: 1}, {s + 1: 1}, 0.5) for s in range(2, S - 1)]
    y0 = [0.0, 0.0] + [0.3] * (S - 2)
    obs = np.eye(S)[:2]
    for kind, slope in (("activation", 0.0), ("repression", 0.7)):
        for n in (1, 2, 8):
            rx = [({}, {1: 1}, RateLaw(0.7, [Hill(0, 0, n, kind)]))] + pad
            like = MassActionODELogLike(S, rx, y0, t, obs, np.ones((2, 3)), 1.0, lanes_per_point=lanes, ndim=1)
            sim = like.simulate(np.array([[0.3]]))[0]
            assert np.isfinite(like(np.array([0.3])))
            assert np.all(sim[:, 0] == 0.0) and np.all(np.abs(sim[:, 1] - slope * t) <= 1e-6), (kind, n, sim)


@pytest.mark.parametrize("lanes", sorted(LANE_SPECS))
def test_edge_a_rate_law_with_nothing_in_it_is_the_plain_reaction(lanes):
    spec = LANE_SPECS[lanes]
    plain = [({0: 1}, {1: 1}, 0), ({0: 2, 1: 1}, {0: 3}, Monomial({0: 1, 1: -1})), ({1: 1}, {}, 0.4)] + list(spec["reactions"][3:])
    wrapped = [(reac, prod, RateLaw(rate)) for reac, prod, rate in plain]
    a, b = RN.build(dict(spec, reactions=plain)), RN.build(dict(spec, reactions=wrapped))
    X = np.array([spec["nominal"], spec["nominal"] + 0.3, spec["nominal"] - 0.4])
    assert a.source() == b.source() and a.data_block().tobytes() == b.data_block().tobytes()
    assert a.batch(X).tobytes() == b.batch(X).tobytes() and np.all(np.isfinite(a.batch(X)))
    explicit = [(reac, prod, RateLaw(rate, order=dict(reac))) for reac, prod, rate in plain]      # the same orders, written out: the same bits
    assert RN.build(dict(spec, reactions=explicit)).batch(X).tobytes() == a.batch(X).tobytes()


def test_edge_validation_errors():
    mk = lambda rate, S=3, **kw: MassActionODELogLike(S, [({0: 1}, {1: 1}, rate)], [1.0] * S, [1.0], np.eye(S)[:1], [[1.0]], 1.0, **kw)      # noqa: E731
    with pytest.raises(ValueError, match="species"):
        mk(RateLaw(0, [Hill(3, 1)]))
    with pytest.raises(ValueError, match="species"):
        mk(RateLaw(0, order={5: 1}))
    with pytest.raises(ValueError, match="species"):
        Hill(-1, 0)
    for n in (0, 9, 2.0, True, -1):
        with pytest.raises(ValueError, match="1..%d" % ODE_MAX_HILL_EXPONENT):
            Hill(0, 1, n)
    with pytest.raises(ValueError, match="kind"):
        Hill(0, 1, 2, "inhibition")
    for K in (0.0, -1.0, np.inf, np.nan):
        with pytest.raises(ValueError, match="finite and > 0"):
            Hill(0, K)
    for K in (-1, True, "k", None):
        with pytest.raises(ValueError):
            Hill(0, K)
    with pytest.raises(ValueError, match="at most %d" % ODE_MAX_RATE_FACTORS):
        RateLaw(0, [Hill(0, 1)] * 5)
    assert len(RateLaw(0, [Hill(0, 1)] * 4).factors) == 4
    for order in ({0: -1}, {0: 1.5}, {-1: 1}, {0: True}, [0, 1], {"a": 1}):
        with pytest.raises(ValueError, match="order"):
            RateLaw(0, order=order)
    with pytest.raises(ValueError, match="RateLaw"):
        RateLaw(RateLaw(0))
    with pytest.raises(ValueError):
        RateLaw(np.inf)
    with pytest.raises(ValueError, match="Hill"):
        RateLaw(0, [1.0])
    with pytest.raises(ValueError, match="ndim"):
        mk(RateLaw(0, [Hill(0, 7)]), ndim=3)
    assert mk(RateLaw(0, [Hill(0, Monomial({4: 1, 2: -1}))])).d == 5 and mk(RateLaw(1, [Hill(0, 6)])).d == 7


@pytest.mark.parametrize("lanes, lim", [(1, ODE_LIMITS), (16, ODE_GROUP_LIMITS), (64, ODE_WAVE_LIMITS)])
def test_edge_reactions_plus_slots_stay_within_the_reaction_limit(lanes, lim):
    S = {1: 2, 16: 9, 64: 33}[lanes]
    R = lim["reactions"]
    base = [({0: 1}, {1: 1}, 0.1)] * (R - 2)
    mk = lambda rx: MassActionODELogLike(S, rx, [1.0] * S, [1.0], np.eye(S)[:1], [[1.0]], 1.0, lanes_per_point=lanes)      # noqa: E731
    one = ({0: 1}, {1: 1}, RateLaw(0, [Hill(0, 1, 2)]))
    mk(base + [one])                                                                # R - 1 reactions and one slot
    mk(base[1:] + [one, ({1: 1}, {0: 1}, RateLaw(0, [Hill(1, 1, 2)]))])            # the same (K, n): still one slot
    with pytest.raises(ValueError, match="within %d" % R):
        mk(base + [one, ({1: 1}, {0: 1}, 0.2)])
    with pytest.raises(ValueError, match="within %d" % R):
        mk(base[1:] + [one, ({1: 1}, {0: 1}, RateLaw(0, [Hill(1, 1, 3)]))])        # another n: two slots


def test_the_value_classes_are_immutable_hashable_comparable_and_picklable():
    h = Hill(2, Monomial({0: 1}), 3, "repression")
    law = RateLaw(1, [h, Hill(0, 0.5)], order={3: 2, 1: 0})
    assert law.order == ((3, 2),) and law.factors == (h, Hill(0, 0.5)) and h == Hill(np.int64(2), Monomial({0: 1}), 3, "repression")
    assert pickle.loads(pickle.dumps(law)) == law and hash(pickle.loads(pickle.dumps(law))) == hash(law) and eval(repr(law)) == law
    assert Hill(0, 1) != Hill(0, 1.0) and RateLaw(1) != RateLaw(1.0) and RateLaw(0, order={}) != RateLaw(0) and len({law, RateLaw(1, [h, Hill(0, 0.5)], {3: 2})}) == 1
    for obj, name in ((h, "n"), (law, "rate")):
        with pytest.raises(AttributeError):
            setattr(obj, name, 1)
        with pytest.raises(AttributeError):
            delattr(obj, name)


# ---------------------------------------------------------------------------------------------------- 6. nothing existing moved
# source() and data_block() hashes and the cross-compiled kernels' notes, all computed on the parent commit
PARENT = {
    "robertson": ("c4fd92120c3b297f5ca95cc5badd01f82fb4e13702022f116b6aa3a583f6be0e", "046f08c55d3e336c2f5686487331a79146aefda78d89ae8aa539dfd0b8aa7330",
                  dict(vgpr=155, agpr=0, scratch=0, lds=0)),
    "enzyme13_16": ("0aa13e4724688b1327784e38675d9c71e37520f6bfef3fb95eef62929af3b1f6", "349c13663e539a491a505d150a53decf18f2baeddacf4ba08e56635dfa74f00b",
                    dict(vgpr=218, agpr=0, scratch=0, lds=2688)),
    "cascade_64": ("b0efab83cb0fbb70af3ee21f2ed93593cf30af172456910e963acce3f020bdb1", "c68d83a94ba64e86cd396cad14a8d5149d5a530df0d68aba13f7a25756eac0de",
                   dict(vgpr=412, agpr=156, scratch=0, lds=3904)),
    "mm_kd": ("871983a15ec53e4bfeb7f19703da14d1799159e9f5157902115f10116fb93b8f", "e4bf50e507ec5f638a57145e469ff7897da5f905e6b67d85c51a1890e1aec937",
              dict(vgpr=209, agpr=0, scratch=0, lds=0)),
    "washout": ("27fbd69a46047c26e6b7ca0c5d6591cfafffe88dda8618e9e3bb1694794f82b6", "f5c47c63ec9a9c525463f3729488eeda10f0062d44644748d666bb1f58603644",
                dict(vgpr=175, agpr=0, scratch=0, lds=0)),
    "preequilibration": ("1c8cb9fc9cee2cdf7c4acf51b0470aca7f69921edcd1ef71242c31cdccde26fe", "e87b71db6ec9afbce8fe4ae85e086c1e7fb748128f62c5de910f4484eac6a840",
                         dict(vgpr=205, agpr=0, scratch=0, lds=0)),
}


def _existing(name):
    if name == "robertson":
        from .ode_networks import robertson
        return robertson()
    if name == "enzyme13_16":
        from .ode_wide_networks import enzyme13
        return enzyme13(16)
    if name == "cascade_64":
        from .ode_wave_networks import cascade
        return cascade()
    if name == "mm_kd":
        from .ode_monomial_networks import build
        return build("mm_kd")[0]
    if name == "washout":
        from pydream_amd.examples.washout import washout_device
        return washout_device.make_likelihood()
    from pydream_amd.examples.preequilibration import preequilibration_device
    return preequilibration_device.make_likelihood()


@pytest.mark.parametrize("name", sorted(PARENT))
def test_nothing_existing_moved(name):
    like = _existing(name)
    source, data, parent_notes = PARENT[name]
    assert hashlib.sha256(like.source().encode()).hexdigest() == source
    assert hashlib.sha256(like.data_block().tobytes()).hexdigest() == data
    assert "SLOTS" not in like.source()
    assert notes(like.code_object()) == parent_notes


# ---------------------------------------------------------------------------------------------------- 7. the new kernels' resources
def _lds_row(like):
    """dz_ode_group.h's group_lds_row times the points of a block, in bytes"""
    lanes = like.lanes_per_point
    slots = int(like.source().split("SLOTS = ")[1].split(";")[0])
    return 8 * (256 // lanes) * (len(like.reactions) + slots + 1 + (like.n_species if lanes == 64 else 0))


@pytest.mark.parametrize("name", sorted(RN.NAMED))
def test_the_named_one_lane_kernels_use_no_scratch_and_no_lds(name):
    got = notes(RN.build(RN.NAMED[name]).code_object())
    print(name, got)
    assert got["scratch"] == 0 and got["lds"] == 0


@pytest.mark.parametrize("lanes", (16, 32, 64))
def test_the_group_kernels_lds_is_the_row_formula_with_the_slots(lanes):
    like = RN.build(LANE_SPECS[lanes])
    got = notes(like.code_object())
    print(lanes, got)
    assert got["lds"] == _lds_row(like) and got["scratch"] == 0
    i = next(i for i in INDEX if RN.CASES[i][0] == lanes)
    like = RN.network(i).like()
    got = notes(like.code_object())
    print(RN.network(i).name, got)
    assert got["lds"] == _lds_row(like)


# ---------------------------------------------------------------------------------------------------- 8. the example
def test_the_repressilator_example():
    from scipy.stats import norm

    from pydream_amd.examples.repressilator import repressilator_device as REP
    data = REP.simulated_data()
    assert data.shape == (3, len(REP.TSPAN)) and np.all(np.isfinite(data)) and np.min(np.ptp(data, axis=1)) > 1.0      # finite, and it moves
    like = REP.make_likelihood(data)
    X = np.array([REP.TRUE, REP.TRUE + 0.1, REP.TRUE - np.array([0.2, 0.0, 0.1, -0.1])])
    twin = REP.HostTwin(like)
    assert np.array([twin(x) for x in X]).tobytes() == like.batch(X).tobytes() and np.all(np.isfinite(like.batch(X)))
    assert like.d == 4 and like.source().count("SLOTS = 1;") == 1 and like.lanes_per_point == 1
    sd = 0.05 * np.abs(data) + 0.05
    tight = REP.make_likelihood(data, rtol=1e-10, atol=1e-10, max_steps=20000)
    assert np.max(np.abs(tight.simulate(REP.TRUE)[0].T - data)) < 1e-6           # the data are the model's at the true point ...
    ref = float(np.sum(norm(data, sd).logpdf(tight.simulate(REP.TRUE)[0].T)))
    assert abs(tight(REP.TRUE) - ref) <= 1e-9 * abs(ref) and like(REP.TRUE) > like(X[1]) and like(REP.TRUE) > like(X[2])      # ... where the likelihood peaks
    again = pickle.loads(pickle.dumps(like))
    assert again.reactions == like.reactions and again.source() == like.source() and again.batch(X).tobytes() == like.batch(X).tobytes()
