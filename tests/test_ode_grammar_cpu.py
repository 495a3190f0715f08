"""The four host builds of MassActionODELogLike (one lane, 16, 32 and 64 lanes per point) on a grammar of seeded random networks, against
references that share no code with them (tests/ode_reference.py): fixed Rodas4 steps against a 40-digit restatement at a tolerance
sized by a float64 restatement, the adaptive path against scipy's Radau, the linear invariants of the stoichiometric matrix, edge
inputs, relabelled species and reordered reactions, large steps whose pivots leave the diagonal, and a network whose pivot candidates tie.

The grammar's fixed steps (t1 = 1, n = 4 and 16) never pivot: 1 / (h gamma) is 16 or 64 against Jacobian entries of order 1, W is
diagonally dominant, and REF.pivot_rows on the float64 restatement's W finds no column off the diagonal in any step of any of the 37
cases, at n = 4 or at n = 16.  There the arg-max, piv, pos and the solves' b[piv[k]] are the same as no pivoting at all.  The large-step family
(tests/ode_grammar.LARGE_STEP_CASES) and the tied network are where a permutation is checked to rounding; fixed n = 16 runs on every
64-lane case (the slowest, S = 63, takes about 40 s, most of it the mp restatement).

Permutation faults seeded in a scratch copy (never committed), and what they did: the host twin's forward solve reading b[k] for
b[piv[k]] (csrc/dz_ode_group.h, HostGroup::lu_solve: the builds of 16, 32 and 64 lanes) together with the one-lane lu_solve leaving b
unpermuted (csrc/dz_ode.h).  All 29 fixed-step cases the grammar had before pass with both faults, at the ratios they show without
(0.013 .. 0.051); so do the eight 64-lane cases.  All eight large-step cases fail: the state after four steps is not finite in seven and
7e12 tolerances off in large-S16R32@16; after two steps the deviation is 1e13 .. 1e88 tolerances in every case, after the first step
6e15 (large-S6R12@1), 2e21 (large-S12R24@16) and 9e16 (large-S64R80@64) where the first W already pivots, and 0.02 .. 0.09 where it
does not.  The tied network fails in every build (not finite).  On the inputs of tests/test_ode_grammar_gpu.py the faults change the
host value's bits at 2002 of 2051 (one lane), 1004 of 1027 (16 and 32 lanes) and 250 of 259 (64 lanes) tied points, and at 1027 of
1027, 515 of 515, 512 of 515 and 131 of 131 large-step points: what the device comparison resolves there.

Faults seeded while these were written, and what caught them: the multiplicity factor (2.0 *, 3.0 *) dropped from the generated Jacobian
of the one-lane generator fails the fixed-step test on all 10 one-lane networks, dropped from the group generator on all 18 group
networks (deviation 1e-6 .. 1e-4 where the tolerance is about 1e-14); a product coefficient 2 turned into 1 in the group generator's
coefficient() fails the fixed-step test on 16 group networks and the invariant test on two.  The host twin breaking pivot ties towards
the highest row passes everything here (either pivot is valid) and changes the likelihood's bits at 71 of the 1027 points of
tests/test_ode_grammar_gpu.py's tied-pivot case, which is what that test compares with the device."""
import numpy as np
import pytest

from . import ode_grammar as G
from . import ode_reference as REF

EPS = np.finfo(float).eps
INDEX = list(range(len(G.CASES)))
IDS = [G.network(i).name for i in INDEX]
N_POINTS = 3
_REPLACED, _NETS, _RADAU = set(), {}, {}
_WORST = {lanes: dict(fixed=0.0, radau=0.0) for lanes in G.BUILDS}             # per build, for the summary the last grammar test prints


def resolved(i):
    """Case i's network, with Radau's states [point, T, S] at its box points; the next seed takes its place only if Radau fails on it."""
    if i not in _NETS:
        for bump in (0, 1):
            net = G.network(i, bump)
            X = net.points(N_POINTS)
            try:
                _RADAU[i] = np.array([REF.radau(net.S, net.reactions, REF.rate_constants(net.reactions, x, net.rate_scale), net.y0, G.T_OUT) for x in X])
            except AssertionError:
                _REPLACED.add(i)
                continue
            _NETS[i] = net
            break
    return _NETS[i], _RADAU[i]


def _check_fixed_steps(builds, S, reactions, x, y0, t1, label, ns=(4, 16), on_matrix=None):
    """fixed_steps(x, t1, n, embedded) of every build against the mp restatement, n = 4 and 16, both solutions; the largest ratio of
    deviation to tolerance.  on_matrix(step, W): sees the reference's iteration matrices, the order-4 run's first."""
    k = REF.rate_constants(reactions, x, "linear")
    worst = 0.0
    for n in ns:
        for embedded in (False, True):
            ref, scale, tol = REF.fixed_step_reference(S, reactions, k, y0, 0.0, t1, n, embedded, on_matrix=on_matrix)
            assert all(np.isfinite(float(v)) for v in ref) and float(scale) <= 1e3 * np.max(y0)      # (the input is tame: on the reference)
            for like in builds:
                dev = REF.deviation(like.fixed_steps(x, t1, n, embedded), ref, scale)
                worst = max(worst, dev / tol)
                assert dev <= tol, (label, like.lanes_per_point, n, embedded, dev, tol)
    return worst


@pytest.mark.parametrize("i", INDEX, ids=IDS)
def test_fixed_steps_equal_the_mp_restatement_to_rounding(i):
    net, _ = resolved(i)
    x = net.nominal("linear")
    worst = _check_fixed_steps([net.like(rate_scale="linear")], net.S, net.reactions, x, net.y0, 1.0, net.name)
    print("%s: largest deviation / tolerance %.3f" % (net.name, worst))
    _WORST[net.lanes]["fixed"] = max(_WORST[net.lanes]["fixed"], worst)


@pytest.mark.parametrize("i", INDEX, ids=IDS)
def test_adaptive_path_is_within_ten_tolerances_of_radau(i):
    """The project's criterion: every output within 10 requested tolerances of Radau at 1e-12, at rtol = atol = 1e-6 and 1e-9, and
    the absolute error at 1e-9 below 1e-2 of that at 1e-6."""
    net, refs = resolved(i)
    assert np.max(np.abs(refs - net.y0)) > 1e-3                               # (the reference moves: there is something to integrate)
    X = net.points(N_POINTS)
    errs = []
    for rtol in (1e-6, 1e-9):
        sim = net.states(X, rtol=rtol, atol=rtol, max_steps=20000)
        assert np.all(np.isfinite(sim))
        errs.append(float(np.max(np.abs(sim - refs) / (rtol * np.abs(refs) + rtol))))
    print("%s: Radau error in tolerances at 1e-6, 1e-9: %.3f %.3f" % (net.name, errs[0], errs[1]))
    _WORST[net.lanes]["radau"] = max(_WORST[net.lanes]["radau"], *errs)
    assert errs[0] < 10 and errs[1] < 10
    assert errs[1] * 1e-9 < 1e-2 * errs[0] * 1e-6


@pytest.mark.parametrize("i", INDEX, ids=IDS)
def test_linear_invariants_hold_to_rounding_at_the_default_tolerance(i):
    """c . (y(t) - y0) for every left null vector c of the stoichiometric matrix: a Rosenbrock step keeps it to rounding, whatever
    the tolerance."""
    from scipy.linalg import null_space
    net, _ = resolved(i)
    N, _ = REF.stoichiometry(net.S, net.reactions)
    Cn = null_space(N.T.astype(float))
    X = net.points(N_POINTS)
    y = net.states(X)
    assert np.all(np.isfinite(y))
    worst = 0.0
    for c in Cn.T:
        drift = np.max(np.abs((y - net.y0) @ c))
        bound = 1e3 * EPS * np.sum(np.abs(c)) * max(np.max(np.abs(y)), np.max(net.y0))
        worst = max(worst, drift / bound)
        assert drift <= bound, (net.name, drift, bound)
    print("%s: %d invariants, largest drift / bound %.4f" % (net.name, Cn.shape[1], worst))


def test_at_most_two_networks_were_replaced_and_the_grammar_is_still_covered():
    from scipy.linalg import null_space
    nets = [resolved(i)[0] for i in INDEX]
    assert len(_REPLACED) <= 2, _REPLACED
    assert not G.coverage_gaps(nets), G.coverage_gaps(nets)
    for lanes in G.BUILDS:                                                     # and every build meets invariants that more than one species shares
        shared = sum(int(np.sum(np.sum(np.abs(null_space(REF.stoichiometry(n.S, n.reactions)[0].T.astype(float))) > 1e-9, axis=0) > 1))
                     for n in nets if n.lanes == lanes)
        print("%d lanes: %d invariants over more than one species" % (lanes, shared))
        assert shared >= 3
        print("%d lanes: largest fixed-step deviation / tolerance %.3f, largest Radau error %.3f tolerances (of the tests that ran before)"
              % (lanes, _WORST[lanes]["fixed"], _WORST[lanes]["radau"]))


# ---------------------------------------------------------------------------------------------------- edges
EDGE = {1: 4, 16: 11, 32: 19, 64: 29}          # the case each build's edge tests use (S = 5 with one lane, 9 with 16 lanes, 20 with 32, 33 with 64)


def _close(sim, ref, rtol, factor=10):
    return np.all(np.abs(sim - ref) <= factor * (rtol * np.abs(ref) + rtol))


def _edge(lanes):
    net = resolved(EDGE[lanes])[0]
    return net, net.points(4, seed=3)


@pytest.mark.parametrize("lanes", sorted(EDGE))
def test_edge_t0_and_repeated_output_times(lanes):
    net, X = _edge(lanes)
    kw = dict(rtol=1e-9, atol=1e-9, max_steps=20000)
    for t0, t in ((3.0, np.array([3.0, 3.5, 4.5])), (0.0, np.array([0.5, 0.5, 1.0, 1.0, 1.0])), (1.0, np.array([1.0, 1.0, 2.0]))):
        sim = net.states(X, t=t, t0=t0, **kw)
        ref = np.array([REF.radau(net.S, net.reactions, REF.rate_constants(net.reactions, x, net.rate_scale), net.y0, t, t0=t0) for x in X])
        assert _close(sim, ref, 1e-9), (t0, t)
        for a, b in zip(np.flatnonzero(np.diff(t) == 0), np.flatnonzero(np.diff(t) == 0) + 1):
            assert np.array_equal(sim[:, a], sim[:, b])
        if t[0] == t0:
            assert np.array_equal(sim[:, 0], np.tile(net.y0, (len(X), 1)))


@pytest.mark.parametrize("lanes", sorted(EDGE))
def test_edge_a_single_output_time_equal_to_t0_is_the_likelihood_of_y0_and_takes_no_step(lanes):
    from scipy.stats import norm
    net, X = _edge(lanes)
    rng = np.random.default_rng(1)
    obs = rng.normal(size=(3, net.S))
    data, sd = rng.normal(size=(3, 1)), rng.uniform(0.5, 2.0, (3, 1))
    for t0 in (0.0, 3.0):
        like = net.like(observables=obs, t=np.array([t0]), t0=t0, data=data, sd=sd)
        L, steps = like.batch(X, return_steps=True)
        ref = float(np.sum(norm(loc=data[:, 0], scale=sd[:, 0]).logpdf(obs @ net.y0)))
        assert np.all(steps == 0)
        assert np.all(np.abs(L - ref) <= 1e-12 * np.sum(np.abs(norm(loc=data[:, 0], scale=sd[:, 0]).logpdf(obs @ net.y0)))), (L, ref)


@pytest.mark.parametrize("lanes", sorted(EDGE))
def test_edge_nan_data_and_negative_non_integer_observable_weights(lanes):
    """Observables with weights like -0.73 against Radau; the likelihood against scipy.stats.norm over the observed entries."""
    from scipy.stats import norm
    net, X = _edge(lanes)
    rng = np.random.default_rng(2)
    obs = rng.normal(size=(4, net.S))
    assert np.any(obs < 0) and not np.any(obs == np.round(obs))
    Y = np.array([REF.radau(net.S, net.reactions, REF.rate_constants(net.reactions, x, net.rate_scale), net.y0, G.T_OUT) for x in X])
    ref = Y @ obs.T
    data = ref[0].T + 0.1 * rng.normal(size=(4, len(G.T_OUT)))
    data[1, 2] = data[3, 0] = data[0, 3] = np.nan
    sd = rng.uniform(0.05, 0.2, data.shape)
    sd[1, 2] = np.nan                                                          # (not read where nothing is observed)
    like = net.like(observables=obs, data=data, sd=sd, rtol=1e-9, atol=1e-9, max_steps=20000)
    sim = like.simulate(X)
    assert np.all(np.abs(sim - ref) <= 10 * 1e-9 * ((np.abs(Y) + 1) @ np.abs(obs).T))      # every species within 10 tolerances, weighted
    seen = np.isfinite(data)
    for x, s in zip(X, sim):
        terms = norm(loc=data[seen], scale=sd[seen]).logpdf(s.T[seen])
        assert np.isfinite(like(x)) and abs(like(x) - np.sum(terms)) <= 1e-12 * np.sum(np.abs(terms))


@pytest.mark.parametrize("lanes", sorted(EDGE))
def test_edge_ndim_above_the_highest_parameter_index_and_wider_rows(lanes):
    net, X = _edge(lanes)
    kw = dict(rtol=1e-9, atol=1e-9, max_steps=20000)
    wide = np.concatenate([X, np.full((len(X), 5), np.nan)], axis=1)          # (columns the model must not read)
    like = net.like(ndim=net.P + 2, **kw)
    assert like.d == net.P + 2
    ref = np.array([REF.radau(net.S, net.reactions, REF.rate_constants(net.reactions, x, net.rate_scale), net.y0, G.T_OUT) for x in X])
    sim = like.simulate(wide)
    assert _close(sim, ref[:, :, :sim.shape[2]], 1e-9)
    assert like.batch(wide).tobytes() == net.like(**kw).batch(X).tobytes()
    with pytest.raises(ValueError, match="coordinates"):
        like.batch(X)


@pytest.mark.parametrize("lanes", sorted(EDGE))
def test_edge_a_log10_parameter_of_minus_400_switches_its_reactions_off(lanes):
    """10**-400 is 0: finite, and the network without the reactions that parameter drives."""
    net, X = _edge(lanes)
    X = np.log10(net.points(4, rate_scale="linear", seed=3))
    used = sorted({r[2] for r in net.reactions if isinstance(r[2], int)})
    p = used[0]
    rest = [r for r in net.reactions if r[2] != p]
    assert 0 < len(rest) < len(net.reactions)
    X[:, p] = -400.0
    kw = dict(rate_scale="log10", rtol=1e-9, atol=1e-9, max_steps=20000)
    assert np.all(np.isfinite(net.like(**kw).batch(X)))
    sim = net.states(X, **kw)
    ref = np.array([REF.radau(net.S, rest, REF.rate_constants(rest, x, "log10"), net.y0, G.T_OUT) for x in X])
    assert _close(sim, ref, 1e-9)


# ---------------------------------------------------------------------------------------------------- metamorphic
RELABELLED = [3, 7, 11, 14, 18, 23, 31, 35]                                    # (the last two: 64 lanes, S = 48 and 64)


@pytest.mark.parametrize("i", RELABELLED, ids=[IDS[i] for i in RELABELLED])
def test_relabelled_species_and_reordered_reactions_give_the_same_states(i):
    """new species perm[s] is old species s: rows move between lanes and the pivot sequence changes; then the reactions in another order"""
    net, _ = resolved(i)
    rng = np.random.default_rng(net.seed + 5)
    X = net.points(N_POINTS)
    kw = dict(rtol=1e-9, atol=1e-9, max_steps=20000)
    base = net.states(X, **kw)
    perm = rng.permutation(net.S)
    relabelled = [({int(perm[s]): c for s, c in reac.items()}, {int(perm[s]): c for s, c in prod.items()}, rate) for reac, prod, rate in net.reactions]
    y0 = np.zeros(net.S)
    y0[perm] = net.y0
    moved = net.states(X, reactions=relabelled, y0=y0, **kw)
    assert _close(moved[:, :, perm], base, 1e-9)
    order = rng.permutation(net.R)
    shuffled = net.states(X, reactions=[net.reactions[j] for j in order], **kw)
    assert _close(shuffled, base, 1e-9)
    if net.S > 1 and net.R > 1:
        assert not np.array_equal(perm, np.arange(net.S)) and not np.array_equal(order, np.arange(net.R))


# ---------------------------------------------------------------------------------------------------- large steps
LARGE = list(range(len(G.LARGE_STEP_CASES)))
_PIVOTS, _LARGE_WORST = {}, {}           # per large-step case: the reference's pivot rows of every step; deviation / tolerance
# The tolerance is sized by ONE float64 ordering of the operations (numpy's).  Where W is badly conditioned that sample says little: on
# a one-lane network of this family with cond(W) = 2e6 (seed 5, S = 8, h = 16) numpy's own deviation from mp went from 2e-14 to 6e-12
# when nothing but the species' labels changed, a spread of 300 where the formula allows 64.  So a large-step input has cond(W) <= 1e3
# in every step: then cond * eps = 2e-13 bounds what any backward-stable ordering may lose, and the 16 eps floor times 64 is of that size.
MAX_CONDITION = 1e3


def _pivots(j):
    """The pivot rows (REF.pivot_rows) of every step's W in the mp integration of large-step case j: from the reference alone"""
    if j not in _PIVOTS:
        net, (_, _, _, _, t1, n) = G.large_step_network(j), G.LARGE_STEP_CASES[j]
        found = []
        REF.rodas4_fixed_mp(net.S, net.reactions, REF.rate_constants(net.reactions, net.nominal(), "linear"), net.y0, 0.0, t1, n,
                            on_matrix=lambda step, W: found.append(REF.pivot_rows(W)))
        _PIVOTS[j] = found
    return _PIVOTS[j]


def _off_diagonal(piv):
    """[(column, row)] of the pivots that left the diagonal"""
    return [(int(c), int(piv[c])) for c in np.flatnonzero(piv != np.arange(len(piv)))]


@pytest.mark.parametrize("j", LARGE, ids=[G.large_step_network(j).name for j in LARGE])
def test_large_steps_whose_pivots_leave_the_diagonal_equal_the_mp_restatement_to_rounding(j):
    """h = 4 .. 16 on a network that stays tame there: in at least one step three or more columns pivot off the diagonal (a condition on
    the reference's matrices), and both solutions are the mp restatement's to the tolerance its float64 restatement sizes -- a
    permutation that is wrong anywhere (the arg-max, the packed piv bytes, pos, the solves' b[piv[k]], the wave's broadcast of the
    pivot lane) is an error of the order of the solution."""
    net, (_, _, _, _, t1, n) = G.large_step_network(j), G.LARGE_STEP_CASES[j]
    found, cond = [], []

    def on_matrix(step, W):
        cond.append(float(np.linalg.cond(np.array([[float(v) for v in row] for row in W]))))
        assert cond[-1] <= MAX_CONDITION, (net.name, step, cond[-1])           # (on the reference, before any build is looked at)
        if len(found) < n:
            found.append(REF.pivot_rows(W))
    worst = _check_fixed_steps([net.like()], net.S, net.reactions, net.nominal(), net.y0, t1, net.name, ns=(n,), on_matrix=on_matrix)
    _PIVOTS[j], _LARGE_WORST[j] = found, worst
    counts = [len(_off_diagonal(p)) for p in found]
    print("%s, h = %g: off-diagonal pivot columns per step %s, largest condition of W %.0f, largest deviation / tolerance %.3f"
          % (net.name, t1 / n, counts, max(cond), worst))
    assert len(found) == n and len(cond) == 2 * n and max(counts) >= 3


@pytest.mark.parametrize("lanes", G.BUILDS)
def test_large_step_cases_pivot_off_the_diagonal_in_every_quarter_of_the_columns(lanes):
    """Over a build's large-step cases a column of each quarter of 0..S-1 pivots off the diagonal, so every int of packed piv bytes
    carries one that is not its own index; with 64 lanes also a pivot with column and row both >= 32, and one with column and row on
    opposite sides of 32 (the wave's halves).  All from the reference's matrices."""
    quarters, high, across, counts = set(), False, False, {}
    for j in [j for j in LARGE if G.LARGE_STEP_CASES[j][0] == lanes]:
        S = G.LARGE_STEP_CASES[j][1]
        off = [cr for piv in _pivots(j) for cr in _off_diagonal(piv)]
        counts[G.large_step_network(j).name] = [len(_off_diagonal(piv)) for piv in _pivots(j)]
        quarters |= {4 * c // S for c, _ in off}
        high |= any(c >= 32 and r >= 32 for c, r in off)
        across |= any((c >= 32) != (r >= 32) for c, r in off)
    ran = [_LARGE_WORST[j] for j in LARGE if G.LARGE_STEP_CASES[j][0] == lanes and j in _LARGE_WORST]
    print("%d lanes, large steps: off-diagonal pivot columns per step %s; largest deviation / tolerance %s (of the tests that ran before)"
          % (lanes, counts, "%.3f" % max(ran) if ran else "-"))
    assert quarters == {0, 1, 2, 3}, quarters
    if lanes == 64:
        assert high and across


# ---------------------------------------------------------------------------------------------------- tied pivots
def test_tied_pivot_candidates_in_all_four_builds():
    """The 4-species network for one lane and groups of 16 and 32; for the wave its copy behind an inert chain (tests/ode_grammar.py),
    where the tied rows are 34 and 35 and the column is 32"""
    for builds in ((1, 16, 32), (64,)):
        S, reactions, y0, abcd = G.tied_network(builds[0])
        ties = []

        def on_matrix(step, W):
            for q in abcd:
                mag = [abs(W[s][q]) for s in abcd]
                top = [int(abcd[s]) for s in range(4) if mag[s] == max(mag)]
                if len(top) >= 2 and q not in top:
                    ties.append((step, int(q), top))
        REF.rodas4_fixed_mp(S, reactions, REF.rate_constants(reactions, G.TIED_X, "linear"), y0, 0.0, 4.0, 4, on_matrix=on_matrix)
        print("tied pivot candidates (step, column, rows):", ties)
        assert ties                                                            # (a condition on the reference's matrices, not on the code under test)
        worst = _check_fixed_steps([G.tied(lanes) for lanes in builds], S, reactions, G.TIED_X, y0, 4.0, "tied")
        print("tied @%s: largest deviation / tolerance %.3f" % (builds, worst))
