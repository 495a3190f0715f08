"""The sampler's decisions on NaN, +inf and -inf log densities, on the CPU: tests/nonfinite_rule.py's plain twin of Dream.py:279-334 and
metrop_select over the table of value classes, (1) under the three conventions for the maximum of :320 / :902 -- which must not matter --
(2) against the oracle, one generation of an engine whose chains are the table's rows: the host callback returns the row's values for the
proposal and the reference set (in call order: the oracle steps its chains one after the other under a host likelihood), set_state gives
the current state's; try_idx and moved of the trace must be the twin's sel and accept.  A value v reaches the oracle as prior 0, like v --
NaN as prior -inf, like +inf, whose sum is the NaN (a NaN returned by the callback itself is mapped to -inf on the way in).
(3) The poisoned samplers of tests/test_nonfinite_gpu.py part B, run by the oracle alone: each configuration holds chain-generations that
start from +inf, from -inf and from NaN, and accepts neither everything nor nothing.

Seen to fail with a perturbed twin (and, the other way round, with the same change made in a copy of the oracle): nan_to_num(+inf) -> +inf
turns (2) red at k = 1, 3 and 5, snooker on and off; accepting without the isfinite test turns (2) red at k = 1 without snooker (the
ratio +inf of nan_to_num(+inf) - nan_to_num(-inf)); a selection that defaults to try 0 instead of k-1 turns (2) red at k = 3 and 5.
"""
import math

import numpy as np
import pytest

from tests import nonfinite_rule as R


# --------------------------------------------------------------------------------------------------------------- 1. the table itself
def test_table_sizes_and_coverage():
    assert R.table(1).n == 81 * 10 * 4 and R.table(2).n == 9 ** 4 and R.table(3).n == 5 ** 6
    for k in (2, 3) + R.SEEDED_K:
        t = R.table(k)
        assert abs(int(t.snk.sum()) * 2 - t.n) <= 1                            # half the rows are snooker rows, with finite terms
        assert np.isfinite(t.slp).all() and np.isfinite(t.slr).all()
        assert set(t.u_sel) == set(R.U) and set(t.u_acc) == set(R.U)
    for k in R.SEEDED_K:
        t = R.table(k)
        assert t.n == 4096
        cl, cb = R.classes(t.lp), R.classes(t.B)
        inside, between = np.zeros((9, 9), bool), np.zeros((9, 9), bool)
        for i in range(k):
            for j in range(k):
                between[cl[:, i], cb[:, j]] = True
                if i < j:
                    inside[cl[:, i], cl[:, j]] = True
        assert inside.all() and between.all()                                  # every ordered pair of classes, in lp and between lp and B


@pytest.mark.parametrize("k", (1, 2, 3) + R.SEEDED_K)
def test_the_max_convention_is_immaterial(k):
    """fmax (skips NaN), np.amax (propagates it) and the oracle's loop (keeps it in slot 0 only) give the same sel, accept and bits of
    ratio: a NaN term makes its own weight NaN, and with it both sums, whatever was subtracted"""
    t = R.table(k)
    ref = t.decide_all("propagate")
    for conv in ("skip", "first"):
        got = t.decide_all(conv)
        np.testing.assert_array_equal(got[0], ref[0])
        np.testing.assert_array_equal(R.bits(got[1]), R.bits(ref[1]))
        np.testing.assert_array_equal(got[2], ref[2])
    assert 0 < ref[2].sum() < t.n and not np.isnan(ref[1]).any()
    if k > 1:
        assert len(set(ref[0])) == k                                           # every try is selected somewhere
        for v in (R.DBL_MAX, -R.DBL_MAX, 0.0):                                 # log(SA / SB) = +inf, -inf and NaN all occur, and a plain ratio
            assert (ref[1] == v).sum() >= 10, v
        assert (np.abs(ref[1]) < 1e300).sum() - (ref[1] == 0.0).sum() >= 100


# --------------------------------------------------------------------------------------------------------------- 2. the oracle
def _split(v):
    """value -> (prior, like) whose sum at T = 1 is v, bits included, and survives the NaN -> -inf mapping of each term"""
    return (-math.inf, math.inf) if v != v else (0.0, v)


def oracle_generation(k, lp, B, snooker, d=4, seed=11):
    """one generation of an oracle engine with a chain per row (one crossover value, CR = 1: an accepted proposal differs from the state in every
    dimension, so moved is accept -- but for a
    snooker step whose two archive rows or whose axis coincide, which proposes the state itself) -> (trace, expected sel, expected moved, callback calls) -- the twin fed with the engine's
    own u_sel, u_acc and, on snooker rows, its own snooker terms (debug_propose replays the proposal points)"""
    from oracle import oracle as O
    n = len(lp)
    rng = np.random.default_rng(seed)
    Z0 = rng.uniform(-5.0, 15.0, (2 * n + 10 * d, d))
    e = O.Engine(nchains=n, ndim=d, multitry=k, ncr=1, history_thin=1, hardboundaries=0, history_capacity=len(Z0) + 2 * n, trace_capacity=1,
                 seed=seed, snooker=1.0 if snooker else 0.0, p_gamma_unity=0.2)
    e.set_gamma_table(np.array([[2.38 / np.sqrt(2.0 * np.arange(1, d + 1))]]))
    st = dict(chain=0, calls=0)

    def cb(Xp, m, dd, pp, lk, user):               # call order: per chain the proposal set (again in every redraw round), then the reference set
        c = st["chain"]
        st["calls"] += 1
        if k > 1 and m == k - 1:
            vals = B[c, :k - 1]; st["chain"] = c + 1
        else:
            vals = lp[c]
            if k == 1:
                st["chain"] = c + 1
        for i in range(m):
            pp[i], lk[i] = _split(float(vals[i]))
        return 0
    cfn = O.LOGP_CB(cb)
    e._keep.append(cfn)
    e._chk(e.L.orc_set_likelihood_host(e.h, cfn, None))
    e.set_history(Z0)
    cur = [_split(float(v)) for v in B[:, k - 1]]
    e.set_state(Z0[:n], np.array([p for p, _ in cur]), np.array([l for _, l in cur]))
    e.step(1)
    assert st["chain"] == n
    tr = e.get_trace(0, 1)
    e.set_history(Z0)                              # (the generation appended its states: debug_propose replays from the archive the step saw)
    s_ctrl = O.stream_id(O.K_CTRL)
    sel, moved = np.zeros(n, int), np.zeros(n, bool)
    for c in range(n):
        w = O.philox(seed, 2, s_ctrl, c, 0)
        u_sel, u_acc = O.u53(w[0], w[1]), O.u53(w[2], w[3])
        slp, slr, cur_snk, pts = [0.0] * k, [0.0] * k, 0.0, None
        anyfinite = k == 1 or bool(np.isfinite(lp[c]).any())
        if snooker and anyfinite:                                              # (after the redraw rounds of a row without a finite try the step is a rejection)
            cr = int(tr["cr_idx"][0, c])
            pts, s0, _, zidx = e_propose(e, c, 0, Z0[c], cr)
            slp = s0.tolist()
            if k == 1:
                v = Z0[c] - Z0[zidx[0, 0]]
                nc = math.sqrt(O.wave_dot(v, v))
                cur_snk = O.log(nc) * (d - 1) if nc != 0.0 else 0.0
            else:
                s = R.select(k, lp[c].tolist(), u_sel)
                slr = e_propose(e, c, 1, pts[s], cr)[1].tolist() + [0.0]
        s, _, acc = R.decide(k, lp[c].tolist(), B[c].tolist(), snooker, slp, slr, cur_snk, float(B[c, k - 1]), u_sel, u_acc)
        differs = pts is None or bool((pts[s] != Z0[c]).any())                 # (a snooker step along a zero vector proposes the state itself)
        sel[c], moved[c] = s, acc and anyfinite and differs                    # DESIGN.md deviation D1: no finite try after the redraw rounds -> reject
    e.close()
    return tr, sel, moved, st["calls"]


def e_propose(e, c, phase, base, cr):
    return e.debug_propose(c, 0, phase, base, 1, cr)


@pytest.mark.parametrize("snooker", [False, True])
@pytest.mark.parametrize("k", [1, 3, 5])
def test_the_oracle_agrees_with_the_twin(k, snooker):
    t = R.table(k)
    if k == 1:                                                                 # V x V, four chains each (their u_acc are the engine's own)
        rows = np.repeat(np.arange(81), 4)
    else:
        rows = np.arange(t.n)
    lp, B = t.lp[rows], t.B[rows]
    tr, sel, moved, calls = oracle_generation(k, lp, B, snooker)
    np.testing.assert_array_equal(tr["try_idx"][0], sel)
    np.testing.assert_array_equal(tr["moved"][0].astype(bool), moved)
    np.testing.assert_array_equal(tr["snooker"][0].astype(bool), np.full(len(rows), snooker))
    assert 0 < moved.sum() < len(rows)
    if k > 1:
        nofin = int((~np.isfinite(lp).any(axis=1)).sum())
        assert nofin > 0 and calls == 2 * len(rows) + 64 * nofin               # the rows without a finite try went through every redraw round


# --------------------------------------------------------------------------------------------------------------- 3. the poisoned samplers
def _conditions(run, nan_needed=True):
    s = R.starts(run)
    assert np.isposinf(s).sum() >= 20, "chain-generations starting from +inf: %d" % np.isposinf(s).sum()
    assert np.isneginf(s).sum() >= 20, "chain-generations starting from -inf: %d" % np.isneginf(s).sum()
    if nan_needed:
        assert np.isnan(s).sum() >= 5, "chain-generations starting from NaN: %d" % np.isnan(s).sum()
    rate = run["trace"]["moved"].mean()
    assert 0.02 < rate < 0.98, rate


@pytest.mark.parametrize("lk,k,prior,snk", R.MODULE_CASES)
def test_the_oracle_meets_the_poison_in_every_user_kernel_configuration(lk, k, prior, snk):
    """what tests/test_nonfinite_gpu.py compares the HIP engine with: the twin's unmapped NaN, +inf and -inf seed a third of the chains, the
    bands keep supplying them"""
    _conditions(R.oracle_run(R.module_case(lk, k, prior, snk)))


@pytest.mark.parametrize("name", sorted(R.FUNCTION_CASES))
def test_the_oracle_meets_the_poison_with_the_device_function(name):
    _conditions(R.oracle_run(R.FUNCTION_CASES[name]))


@pytest.mark.parametrize("name", sorted(R.BUILTIN_CASES))
def test_the_oracle_meets_the_poison_in_the_built_in_configurations(name):
    """the built-in densities are never +inf or NaN themselves: those come from the start states (set_state stores what it is given), -inf
    also from proposals made with the archive's huge rows"""
    run = R.oracle_run(R.BUILTIN_CASES[name][0])
    _conditions(run)
    assert (np.abs(run["Z"][:20]) >= 1e200).sum() == len(R.HUGE_ROWS)          # (the seed rows that hold them)
