"""The persistent kernel's instantiation with the try count compiled in (k_generations<.., KC = 5, PLAIN>; dz_megakernel.h, chosen in
run_mega_segment for multitry 5 outside the crossover burn-in at 16 chains per block) against the instantiation that reads the try count
at run time (DZ_MEGA_KC=0) and against the oracle: trace states, log p, the decision columns, the archive and the chains' final log prior /
log likelihood, bit for bit.

Every case: multitry 5, flat prior, history thin 10, snooker 0.5 (both move types occur in every block of 16 chains).  History lag 0 runs 25
generations.  History lag 3 runs 45: set_history starts the count of appends at 0 and mega_segment (dz_engine.hip) lets a launch hold a second
append only once history_lag of them are made, so with appends behind generations 0, 10 and 20 the launches are 0, 1..10, 11..20 whatever
DZ_MEGA_SEGS says, and 25 generations end (21..24) before any launch holds two.  The next one, 21..40, does: the append of generation 30 in the
middle of the launch -- the archive length the later generations draw from grows inside the kernel -- and that of 40 at its end, which is the
schedule the headline runs at.  Each case checks the number of launches, and the lag-3 cases run a third time with DZ_MEGA_SEGS=1.
Population: 3073 chains -- the smallest mega_block_plan (dz_mega_select.h) gives 16-chain blocks on the MI355X's 256 CUs: up to 3072 chains 256 blocks
of 12 chains are one round at 0.82 of a 16-chain block's time; 3073 chains are two rounds of 12 (1.64), two of 8 (1.34), or ONE round of 193
blocks of 16 (1.0), the last of which holds a single chain -- so the blocks' inactive-chain path runs as well."""
import numpy as np
import pytest

from tests import helpers as H

pytestmark = pytest.mark.gpu

N = 3073
THIN = 10
# generations, stepped in two pieces: the first ends with a launch that ends with an append (what it ran as is asked there, not only behind the
# appendless tail), and, history lag 3, holds another one in its middle
PIECES = {0: (21, 4), 3: (41, 4)}
# launches of the persistent kernel: lag 0: 0, 1..10, 11..20 | 21..24;  lag 3, two appends per launch: 0, 1..10, 11..20, 21..40 | 41..44;  one: 21..30 and 31..40
LAUNCHES = {(0, None): 4, (3, 2): 5, (3, 1): 6}


@pytest.fixture(scope="module")
def G():
    from pydream_amd import _capi
    return _capi


@pytest.fixture(scope="module")
def O():
    from oracle import oracle
    return oracle


def run(Cls, d, k, kind, lag, trace, seed, want=None):
    """-> engine, outputs;  want = (variant, tries, launches): a GPU run, which checks after each piece what its last launch ran as"""
    GENS = sum(PIECES[lag])
    Z0 = H.seed_history(max(10 * d, 64), d, seed)
    X0 = H.seed_history(N, d, seed + 1)
    e = Cls(nchains=N, ndim=d, multitry=k, history_thin=THIN, history_lag=lag, snooker=0.5, schedule=2, seed=seed,
            history_capacity=len(Z0) + N * (GENS // THIN + 2), trace_capacity=GENS if trace else 0)
    e.set_history(Z0)
    e.set_state(X0)
    P = H.mvn_precision(d)
    if kind == "tri":
        e.set_likelihood_mvn(np.zeros(d), H.tri_factor(P), 1, 0.0)
    else:
        e.set_likelihood_mvn(np.zeros(d), P, 0, 0.0)
    if want:
        e.profile_enable(True); e.profile_reset()
    for m in PIECES[lag]:
        e.step(m)
        if want:
            assert e.last_kernel_variant() == want[0]
            assert e.last_kernel_tries() == want[1]
    if want:
        assert e.profile_get("generations")[1] == want[2]
        e.profile_enable(False)
    out = dict(history=e.get_history())
    out["X"], out["lprior"], out["llike"] = e.get_state()
    if trace:
        out.update({"trace_" + key: v for key, v in e.get_trace(0, GENS).items()})
    return e, out


def assert_identical(a, b, what):
    assert sorted(a) == sorted(b)
    for key in sorted(a):
        np.testing.assert_array_equal(a[key], b[key], err_msg="%s: %s" % (what, key))


def three_way(G, O, monkeypatch, d, k, kind, lag, trace, want_kc, xl="xlds"):
    segs = 2 if lag else None
    if lag:
        monkeypatch.setenv("DZ_MEGA_SEGS", "2")              # two history appends per launch, once three appends are made
    else:
        monkeypatch.delenv("DZ_MEGA_SEGS", raising=False)    # history lag 0: a launch ends with its append
    seed = 7100 + 13 * d + lag
    # chain states in LDS wherever they fit next to the matrix and the point tiles: the packed triangle leaves room at every d <= 112, the dense
    # 100 x 102 square does not (mega_layout: 170192 bytes with them, 157264 without, of 160 KiB), the dense 7 x 8 one does
    variant = "k_generations<%d,%s,%s,16,1,lean>" % ((d + 15) // 16, kind, xl)
    monkeypatch.delenv("DZ_MEGA_KC", raising=False)
    _, new = run(G.Engine, d, k, kind, lag, trace, seed, (variant, want_kc, LAUNCHES[lag, segs]))
    monkeypatch.setenv("DZ_MEGA_KC", "0")
    _, gen = run(G.Engine, d, k, kind, lag, trace, seed, (variant, 0, LAUNCHES[lag, segs]))
    monkeypatch.delenv("DZ_MEGA_KC", raising=False)
    assert_identical(new, gen, "default against DZ_MEGA_KC=0")
    if lag:      # the same generations with one append per launch: one launch more, the same numbers
        monkeypatch.setenv("DZ_MEGA_SEGS", "1")
        _, one = run(G.Engine, d, k, kind, lag, trace, seed, (variant, want_kc, LAUNCHES[lag, 1]))
        monkeypatch.setenv("DZ_MEGA_SEGS", "2")
        assert_identical(new, one, "two appends per launch against one")
    _, ora = run(O.Engine, d, k, kind, lag, trace, seed)
    assert_identical(new, ora, "default against the oracle")
    if trace:
        snk = new["trace_snooker"].mean()
        assert 0.4 < snk < 0.6, snk
        assert 0.02 < new["trace_moved"].mean() < 0.98
    assert len(new["history"]) == max(10 * d, 64) + N * (sum(PIECES[lag]) // THIN + 1)          # every append was made


# d = 7: one row tile; 97: odd, the point rows' pad column; 100: the headline; 112: the last row tile full
@pytest.mark.parametrize("lag", [0, 3])
@pytest.mark.parametrize("d", [7, 97, 100, 112])
def test_compiled_in_try_count_triangular_factor(G, O, monkeypatch, d, lag):
    three_way(G, O, monkeypatch, d, 5, "tri", lag, True, 5)


# the dense matrix: d = 100 leaves no room for the chain states in LDS (<.., dense, xhbm, .., 5, true>), d = 7 does (<.., dense, xlds, .., 5, true>)
@pytest.mark.parametrize("lag", [0, 3])
@pytest.mark.parametrize("d,xl", [(100, "xhbm"), (7, "xlds")])
def test_compiled_in_try_count_dense_matrix(G, O, monkeypatch, d, xl, lag):
    three_way(G, O, monkeypatch, d, 5, "dense", lag, True, 5, xl)


def test_compiled_in_try_count_without_a_trace_buffer(G, O, monkeypatch):
    three_way(G, O, monkeypatch, 100, 5, "tri", 3, False, 5)


def test_four_tries_still_run_the_generic_instantiation(G, O, monkeypatch):
    three_way(G, O, monkeypatch, 100, 4, "tri", 3, True, 0)
