"""The arithmetic of the persistent kernel's serial phases, on the CPU.

1. dz::row_prefix_ordered<K> (csrc/dz_device.h) as a numpy model -- K - 1 shifted copies of the row (a source outside the row of 16 lanes
   reads +0.0) added to +0.0 in the order K-1, .., 1, then the row itself -- against the sequential left-to-right sum of the reduction
   contract (S = 0.0; S = S + w_0; ...), bit for bit, K = 1..16, in every lane i < K; and that a lane's bits do not depend on K.
2. The selection's "first i < K with u < cum_i, else K - 1" as one compare mask, cut to K lanes with bit K - 1 set, and a find-first-set,
   against the loop it replaces; all-false and NaN rows included.
3. That the two targets of tests/test_mega_serial_gpu.py (tests/serial_cases.py) drive the oracle alone through the special paths: from the
   oracle's own proposals (debug_propose), densities (loglike), orc_exp and orc_log, generation 0 is rebuilt the way chain_step does it.
   STEEP: selection weights below dexp's lower cut-off (exact 0), SA / SB = 0 with dlog(0) = -inf and SA / SB = +inf.  FLAT: all tries
   tie to the last bit.  dexp's UPPER cut-off cannot be reached by any sampler run: every argument the engines hand to it is a
   difference from a maximum, never above 0 (chain_step: lp - mx, A - m2, B - m2; the mixture density: lh - mx).  Its value, like that
   of every other special argument, is checked on the device function itself in tests/test_mega_serial_gpu.py."""
import numpy as np
import pytest

from tests import helpers as H
from tests import serial_cases as S


@pytest.mark.parametrize("K", range(1, 17))
def test_row_prefix_model_is_the_sequential_sum(K):
    rows = S.prefix_rows()
    for half in (rows[:, :16], rows[:, 16:]):
        want = S.sequential_prefix(half)
        got = S.row_prefix_model(half, K)
        np.testing.assert_array_equal(S.bits(got[:, :K]), S.bits(want[:, :K]))


def test_row_prefix_inputs_cover_the_edges():
    rows = S.prefix_rows()
    seq = S.sequential_prefix(rows[:, :16])
    assert (S.bits(rows) == S.bits(-0.0)).any() and (S.bits(rows) == 0).any()
    assert ((rows != 0) & (np.abs(rows) < 2.2250738585072014e-308)).any()                  # subnormal terms
    fin = np.where(np.isfinite(rows) & (rows != 0), np.abs(rows), 1.0)
    assert (np.log2(fin.max(axis=1)) - np.log2(fin.min(axis=1)) > 1000).any()              # terms 2^1000 apart in one row
    assert np.isinf(rows).any() and np.isnan(rows).any() and np.isnan(seq).any()
    assert (S.bits(seq[:, 0]) == 0)[S.bits(rows[:, 0]) == S.bits(-0.0)].all()              # +0.0 + -0.0 = +0.0 in lane 0
    # the order matters in these rows: the reversed sum has other bits
    rev = S.sequential_prefix(rows[:, 15::-1])[:, 15]
    assert (S.bits(rev) != S.bits(seq[:, 15])).sum() >= 8


def test_row_prefix_lane_does_not_depend_on_K():
    rows = S.prefix_rows()[:, :16]
    full = S.row_prefix_model(rows, 16)
    for K in range(1, 16):
        np.testing.assert_array_equal(S.bits(S.row_prefix_model(rows, K)[:, :K]), S.bits(full[:, :K]))


@pytest.mark.parametrize("K", range(1, 17))
def test_first_hit_ballot_is_the_loop(K):
    rng = np.random.default_rng(100 + K)
    n = 0
    for trial in range(400):
        pr = rng.uniform(0, 1, 16)
        pr[:K] /= pr[:K].sum()
        kind = trial % 8
        if kind == 1:
            pr[rng.integers(0, K)] = np.nan                      # NaN from there on: compares false
        elif kind == 2:
            pr[:] = np.nan
        elif kind == 3:
            pr[:K] = 0.0                                         # all false
        elif kind == 4:
            pr[:K] = 1.0 / K                                     # the FLAT target's weights
        cum = S.sequential_prefix(pr)
        for u in (rng.uniform(0, 1), 0.0, np.nextafter(1.0, 0.0), cum[rng.integers(0, K)], 2.0):
            assert S.first_hit_ballot(u, cum, K) == S.first_hit_loop(u, cum, K)
            n += 1
    assert n == 2000
    nan = np.full(16, np.nan)
    assert S.first_hit_ballot(0.5, nan, K) == S.first_hit_loop(0.5, nan, K) == K - 1
    ones_beyond = np.concatenate([np.zeros(K), np.ones(16 - K)])                            # hits only in lanes >= K: not seen
    assert S.first_hit_ballot(0.5, ones_beyond, K) == S.first_hit_loop(0.5, ones_beyond, K) == K - 1


# ------------------------------------------------------------------------------------------------------------------ the targets, on the oracle
N, D, K_TRIES = 48, 100, 5
DBL_MAX = 1.7976931348623157e308


def rebuild_generation0(O, target, snooker, seed=811):
    """chain_step's selection and ratio for generation 0 of every chain, from the oracle's parts -> dict of per-chain arrays"""
    Z0 = H.seed_history(10 * D, D, seed)
    X0 = H.seed_history(N, D, seed + 1)

    def engine():
        e = O.Engine(nchains=N, ndim=D, multitry=K_TRIES, history_thin=10, history_lag=0, snooker=snooker, schedule=2, seed=seed,
                     history_capacity=len(Z0) + 2 * N, trace_capacity=1)
        e.set_history(Z0)
        e.set_state(X0)
        S.set_target(e, D, "tri", target)
        return e
    stepped, fresh = engine(), engine()
    stepped.step(1)
    tr = stepped.get_trace(0, 1)
    out = dict(exp_args=[], q=[], lp=[], ratio=[], moved=tr["moved"][0].astype(bool), snk=tr["snooker"][0].astype(bool))
    for c in range(N):
        snk, cr, sel = bool(tr["snooker"][0][c]), int(tr["cr_idx"][0][c]), int(tr["try_idx"][0][c])
        pts, slp = fresh.debug_propose(c, 0, 0, X0[c], snk, cr)[:2]
        lp = np.array([0.0 + 1.0 * fresh.loglike(p) for p in pts])
        args = list(lp - lp.max())
        refs, slr = fresh.debug_propose(c, 0, 1, pts[sel], snk, cr)[:2]
        B = np.array([fresh.loglike(r) for r in refs] + [fresh.loglike(X0[c])])
        A = lp.copy()
        if snk:
            slr = np.concatenate([slr, [0.0]])
            A = lp + slp
            B = (B + slr) + slp
        m2 = max(A.max(), B.max())
        args += list(A - m2) + list(B - m2)
        SA = SB = 0.0
        for a in A:
            SA = SA + O.exp(a - m2)
        for b in B:
            SB = SB + O.exp(b - m2)
        with np.errstate(all="ignore"):
            q = np.float64(SA) / np.float64(SB)
        lg = O.log(q)
        ratio = 0.0 if lg != lg else DBL_MAX if lg == np.inf else -DBL_MAX if lg == -np.inf else lg
        if ratio == -DBL_MAX:                                    # the rebuilt decision is the run's: log(u) < -DBL_MAX never holds
            assert not tr["moved"][0][c]
        if ratio == DBL_MAX:                                     # ... and log(u) < DBL_MAX always: the selected try is the new state
            np.testing.assert_array_equal(tr["X"][0][c], pts[sel])
        out["exp_args"].append(args); out["q"].append(q); out["lp"].append(lp); out["ratio"].append(ratio)
    return {k: np.array(v) for k, v in out.items()}


@pytest.fixture(scope="module")
def O():
    from oracle import oracle
    oracle.build()
    return oracle


@pytest.mark.parametrize("snooker", [0.1, 1.0])
def test_steep_target_takes_the_lower_cutoff_and_log_of_zero(O, snooker):
    r = rebuild_generation0(O, "steep", snooker)
    a = r["exp_args"]
    assert (a <= 0).all()                                        # (why the upper cut-off is out of reach)
    below = a < -745.2
    assert below[:, :K_TRIES].any(axis=1).all()                  # every chain's selection holds a weight that is an exact 0
    assert all(O.exp(x) == 0.0 for x in a[below][:50])
    assert (r["q"] == 0.0).sum() >= 5                            # dlog(0) = -inf -> -DBL_MAX: a certain reject
    assert O.log(0.0) == -np.inf
    assert (r["q"] == np.inf).sum() >= 1                         # dlog(+inf) -> +DBL_MAX: a certain accept
    assert r["snk"].all() if snooker == 1.0 else (0 < r["snk"].sum() < N)


@pytest.mark.parametrize("snooker", [0.1, 1.0])
def test_flat_target_ties_every_try(O, snooker):
    r = rebuild_generation0(O, "flat", snooker)
    assert (S.bits(r["lp"]) == S.bits(1.0)).all()                # every try of every chain: log density 1 to the last bit
    assert (r["exp_args"][:, :K_TRIES] == 0.0).all()
    if snooker != 1.0:
        plain = ~r["snk"]
        assert plain.any() and (r["q"][plain] == 1.0).all() and (r["ratio"][plain] == 0.0).all()
        assert r["moved"][plain].all()                           # log(u) < 0: accepted
