"""The output cursors of the persistent kernel's <.., KC = 5, PLAIN> instantiations (dz_megakernel.h: the addresses of a chain's trace row, history-append
row, state row and scalar trace columns are built once per launch, kept in LDS and stepped by a launch constant) against the instantiation that rebuilds
every address from the kernel arguments (DZ_MEGA_KC=0), the oracle and the multi-kernel path (DZ_MEGA=0): trace states, log p, the five decision columns,
the archive and the chains' final state / log prior / log likelihood, bit for bit.

The run shape is tests/test_mega_kc_gpu.py's (its constants and its comparison are imported, the file is not touched): 3073 chains -- 193 blocks of 16,
the last with one chain and fifteen inactive ones, whose cursors must never be stored through --, multitry 5, thin 10, snooker 0.5, stepped in two uneven
pieces, so that
  * the second `step` starts with trace_slot0 > 0 (21 or 41) in the middle of a thin-cycle;
  * history lag 3, two appends per launch: the launch of generations 21..40 makes the append of generation 30 in its middle (the append cursor moves on by
    N rows inside the kernel) and that of 40 at its end; with DZ_MEGA_SEGS=1 the same generations take one launch more.
d = 97 and 100 both run the row length 112 (NRT = 7): d odd -- lane 48 owns dimension 96 alone -- and lanes 50..55 store only padding zeros.
Further cases: trace_reset() between the two pieces (the trace cursor restarts at slot 0 while the generation count runs on), no trace buffer at all
(trace_capacity = 0: no trace store may happen), and the dense matrix with the chains' states in LDS (d = 7) and in HBM (d = 100: the state row is read
and written through its cursor every generation)."""
import numpy as np
import pytest

from tests import helpers as H
from tests import test_mega_kc_gpu as KC

pytestmark = pytest.mark.gpu

N, THIN, PIECES, LAUNCHES = KC.N, KC.THIN, KC.PIECES, KC.LAUNCHES
TRACE_KEYS = ("X", "logp", "moved", "try_idx", "cr_idx", "snooker")


@pytest.fixture(scope="module")
def G():
    from pydream_amd import _capi
    return _capi


@pytest.fixture(scope="module")
def O():
    from oracle import oracle
    return oracle


def run(Cls, d, kind, lag, trace, seed, want=None, reset=False):
    """-> outputs;  want = (variant, tries, launches or None): a GPU run, which checks after each piece what its last launch ran as.
    reset: trace_reset() between the pieces; the pieces' traces come back joined, as a run without the reset leaves them"""
    pieces = PIECES[lag]
    GENS = sum(pieces)
    Z0 = H.seed_history(max(10 * d, 64), d, seed)
    X0 = H.seed_history(N, d, seed + 1)
    e = Cls(nchains=N, ndim=d, multitry=5, history_thin=THIN, history_lag=lag, snooker=0.5, schedule=2, seed=seed,
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
    parts = []
    for i, m in enumerate(pieces):
        e.step(m)
        if want:
            assert e.last_kernel_variant() == want[0]
            assert e.last_kernel_tries() == want[1]
        if reset and trace:
            parts.append(e.get_trace(0, m))
            if i + 1 < len(pieces):
                e.trace_reset()
    if want:
        if want[2] is not None:
            assert e.profile_get("generations")[1] == want[2]
        e.profile_enable(False)
    out = dict(history=e.get_history())
    out["X"], out["lprior"], out["llike"] = e.get_state()
    if trace:
        tr = {key: np.concatenate([p[key] for p in parts]) for key in TRACE_KEYS} if reset else e.get_trace(0, GENS)
        out.update({"trace_" + key: tr[key] for key in TRACE_KEYS})
    return out


CHECKED = {}      # (d, kind, lag, trace) -> the default run's outputs, once they have been compared four ways (computed once, never changed)


def setup_env(monkeypatch, lag):
    for name in ("DZ_MEGA", "DZ_MEGA_KC", "DZ_MEGA_SEGS"):
        monkeypatch.delenv(name, raising=False)
    if lag:
        monkeypatch.setenv("DZ_MEGA_SEGS", "2")              # two history appends per launch, once three appends are made


def four_way(G, O, monkeypatch, d, kind, lag, trace, xl="xlds"):
    if (d, kind, lag, trace) in CHECKED:
        return CHECKED[d, kind, lag, trace]
    segs = 2 if lag else None
    setup_env(monkeypatch, lag)
    seed = 7300 + 13 * d + lag
    variant = "k_generations<%d,%s,%s,16,1,lean>" % ((d + 15) // 16, kind, xl)
    new = run(G.Engine, d, kind, lag, trace, seed, (variant, 5, LAUNCHES[lag, segs]))
    monkeypatch.setenv("DZ_MEGA_KC", "0")
    gen = run(G.Engine, d, kind, lag, trace, seed, (variant, 0, LAUNCHES[lag, segs]))
    monkeypatch.delenv("DZ_MEGA_KC")
    KC.assert_identical(new, gen, "cursors against DZ_MEGA_KC=0")
    if lag:      # the same generations with one append per launch: one launch more, the same numbers
        monkeypatch.setenv("DZ_MEGA_SEGS", "1")
        one = run(G.Engine, d, kind, lag, trace, seed, (variant, 5, LAUNCHES[lag, 1]))
        monkeypatch.setenv("DZ_MEGA_SEGS", "2")
        KC.assert_identical(new, one, "two appends per launch against one")
    monkeypatch.setenv("DZ_MEGA", "0")
    mk = run(G.Engine, d, kind, lag, trace, seed, ("multi-kernel path", 0, None))
    monkeypatch.delenv("DZ_MEGA")
    KC.assert_identical(new, mk, "cursors against the multi-kernel path")
    ora = run(O.Engine, d, kind, lag, trace, seed)
    KC.assert_identical(new, ora, "cursors against the oracle")
    if trace:
        assert 0.4 < new["trace_snooker"].mean() < 0.6
        assert 0.02 < new["trace_moved"].mean() < 0.98
    assert len(new["history"]) == max(10 * d, 64) + N * (sum(PIECES[lag]) // THIN + 1)          # every append was made, each where it belongs
    for v in new.values():
        v.setflags(write=False)
    CHECKED[d, kind, lag, trace] = new
    return new


# ld = 112 both: d = 97 odd (a lane with only its first dimension live), 100 the headline
@pytest.mark.parametrize("lag", [0, 3])
@pytest.mark.parametrize("d", [97, 100])
def test_cursors_triangular_factor(G, O, monkeypatch, d, lag):
    four_way(G, O, monkeypatch, d, "tri", lag, True)


@pytest.mark.parametrize("lag", [0, 3])
def test_cursors_restart_after_trace_reset(G, O, monkeypatch, lag):
    # the trace cursor restarts at slot 0 in the second piece while the generation count, the archive and the append cursor run on
    d = 97
    new = four_way(G, O, monkeypatch, d, "tri", lag, True)
    setup_env(monkeypatch, lag)
    rst = run(G.Engine, d, "tri", lag, True, 7300 + 13 * d + lag, ("k_generations<7,tri,xlds,16,1,lean>", 5, LAUNCHES[lag, 2 if lag else None]), reset=True)
    KC.assert_identical(new, rst, "trace_reset() between the pieces against none")


def test_cursors_without_a_trace_buffer(G, O, monkeypatch):
    four_way(G, O, monkeypatch, 100, "tri", 3, False)


# the dense matrix: d = 100 leaves no room for the chain states in LDS (the state row's cursor is used every generation), d = 7 does
@pytest.mark.parametrize("lag", [0, 3])
@pytest.mark.parametrize("d,xl", [(100, "xhbm"), (7, "xlds")])
def test_cursors_dense_matrix(G, O, monkeypatch, d, xl, lag):
    four_way(G, O, monkeypatch, d, "dense", lag, True, xl)
