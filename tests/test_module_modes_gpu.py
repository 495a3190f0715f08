"""The fourth likelihood kind (LK_MODULE: dz_set_likelihood_module, dz_set_likelihood_items) in the engine's modes, each at the smallest shape
that can still go wrong: chain-group streams, the items scratch array across growth, sharded engines, parallel tempering, chain-by-chain
stepping, history_lag inside the persistent kernel, lane groups at ragged point counts.  The kernels are tests/module_kernels.py's; the ORACLE
runs their numpy twins through its host callback, and everything is compared bit for bit: the trace (snooker, cr_idx, try_idx, moved, X, logp),
the archive and the crossover state (probabilities, jump sums, update counts).

Every test here has been seen to fail with a perturbed TWIN and an untouched engine: the butterfly's offsets in reverse order (1, 2, .., L/2)
turns the group16, group32 and function tests red, a point's items added right to left the items tests, a sum over descending j the thread
tests.  (Swapping only the offsets 32 and 16 does not reach `function` at d <= 20: lanes 32..63 hold zeros there.)"""
import numpy as np
import pytest

from tests import fuzz_parity as F
from tests import module_kernels as MK

pytestmark = pytest.mark.gpu

KEYS = ("snooker", "cr_idx", "try_idx", "moved", "X", "logp")


def config(**kw):
    """a fuzz_parity configuration (what F.build takes) with crossover adaptation on, so that the crossover state is part of the comparison"""
    c = dict(d=10, N=192, k=3, depairs=1, ngamma=1, ncr=3, adapt_cr=1, adapt_g=0, burnin=9, n=24, lk="items", items=1, finite=1, prior="flat",
             thin=5, lag=0, snooker=0.1, pgu=0.2, lamb=0.05, zeta=1e-12, zero_mean=0, J=2, extra_rows=7, seed=20251, pt=0, world=1, s1=0,
             adapt_lag=0)
    c.update(kw)
    return c


def run(Cls, c, steps=None):
    """-> dict(trace, Z, cr, state, variants, redraws[, swaps]) of one engine over c["n"] generations in the step calls `steps`"""
    MK.code_object(c["lk"])
    e = F.build(Cls, c, {})
    hip = not Cls.__module__.startswith("oracle")
    variants = []
    for m in steps or (c["n"] // 2, c["n"] - c["n"] // 2):
        e.step(m)
        if hip:
            variants.append(e.last_kernel_variant())
    out = dict(trace=e.get_trace(0, c["n"]), Z=e.get_history(), cr=e.get_cr_state(), state=e.get_state(), variants=variants,
               redraws=e.redraw_rounds() if hip else None)
    if c["pt"]:
        out["swaps"] = e.get_swaps(0, c["n"])
    e.close()
    return out


def assert_same(a, b):
    for key in KEYS:
        np.testing.assert_array_equal(a["trace"][key], b["trace"][key], err_msg=key)
    np.testing.assert_array_equal(a["Z"], b["Z"])
    for u, v in zip(a["cr"], b["cr"]):
        np.testing.assert_array_equal(u, v)
    for u, v in zip(a["state"], b["state"]):
        np.testing.assert_array_equal(u, v)


_REFERENCE = {}      # the oracle's runs, by configuration
_PLAIN = {}          # the HIP engine's runs without DZ_STREAMS, by variant


def oracle_run(c, **kw):
    """the oracle's run of c with the twin, computed once per configuration"""
    from oracle import oracle as O
    key = repr(sorted(c.items())) + repr(sorted(kw.items()))
    if key not in _REFERENCE:
        _REFERENCE[key] = run(O.Engine, c, **kw)
    return _REFERENCE[key]


def hip_run(c, **kw):
    from pydream_amd import _capi as G
    return run(G.Engine, c, **kw)


# ---------------------------------------------------------------------------------------------------- 1. chain-group streams with items
@pytest.mark.parametrize("streams", ["2", "3"])
@pytest.mark.parametrize("finite", [1, 0])
def test_items_on_chain_group_streams(streams, finite, monkeypatch):
    """DZ_STREAMS 2 and 3 at 192 chains (the engine drops to one stream below 64 chains per stream) with three items per point: every
    stream's launches write their items into their own slice of d_items and k_sum_items reads that slice.  The non-finite variant under the
    open uniform prior runs redraw rounds through the kernel (shared buffers: those generations go down one stream).  Equal to the oracle and
    to the run without DZ_STREAMS.
    What keeps the lanes: dz_create clamps DZ_STREAMS to one stream when nchains_local < 64 x streams, and N = 192 = 64 x 3 is the smallest
    count that keeps three; one_generation uses them for a full generation whose proposal sets cannot all be impossible (the finite
    variant under the flat prior: redo_possible() is false).  The engine reports no lane count, so the test cannot observe one: if the
    threshold moves, N moves with it."""
    c = config(lk="items", items=3, finite=finite, prior="flat" if finite else "uniform_open", N=192, d=10, k=3, n=24)
    monkeypatch.delenv("DZ_STREAMS", raising=False)
    if finite not in _PLAIN:
        _PLAIN[finite] = hip_run(c)
    plain = _PLAIN[finite]
    monkeypatch.setenv("DZ_STREAMS", streams)
    got = hip_run(c)
    assert_same(got, oracle_run(c))
    assert_same(got, plain)
    assert got["variants"] == ["multi-kernel path"] * 2
    assert 0.02 < got["trace"]["moved"].mean() < 0.95
    if not finite:
        assert got["redraws"] > 0 and plain["redraws"] > 0


# ---------------------------------------------------------------------------------------------------- 2. the items scratch across growth
@pytest.mark.parametrize("streams", [None, "2"])
def test_items_scratch_survives_growth(streams, monkeypatch):
    """tests/test_gpu_parity.py test_eval_logp_scratch_buffers_survive_growth for d_items: dz_eval_logp with 40, 700, 90 and 1500 points
    (the array grows, is kept, grows), generations (whose launches take their slices of it), 1800 points (it is released and allocated
    again between two step calls), generations again.  128 chains = 64 x 2: the smallest count at which DZ_STREAMS=2 keeps two streams
    (dz_create), each with its slice of the array; the finite variant under the flat prior, so the generations use both."""
    from oracle import oracle as O
    from pydream_amd import _capi as G
    if streams is None:
        monkeypatch.delenv("DZ_STREAMS", raising=False)
    else:
        monkeypatch.setenv("DZ_STREAMS", streams)
    c = config(lk="items", items=3, N=128, d=10, k=3, n=8, thin=2)
    MK.code_object("items")
    e, o = F.build(G.Engine, c, {}), F.build(O.Engine, c, {})
    twin = MK.twin("items", c["d"], np.inf, 3)
    P = np.random.default_rng(8).uniform(-5.0, 15.0, (1800, c["d"]))
    for n in (40, 700, 90, 1500):
        np.testing.assert_array_equal(e.eval_logp(P[:n])[1], twin(P[:n])[1])
    e.step(4); o.step(4)
    np.testing.assert_array_equal(e.eval_logp(P)[1], twin(P)[1])
    e.step(4); o.step(4)
    a, b = e.get_trace(0, 8), o.get_trace(0, 8)
    for key in KEYS:
        np.testing.assert_array_equal(a[key], b[key], err_msg=key)
    np.testing.assert_array_equal(e.get_history(), o.get_history())
    for u, v in zip(e.get_cr_state(), o.get_cr_state()):
        np.testing.assert_array_equal(u, v)
    assert a["moved"].any()


# ---------------------------------------------------------------------------------------------------- 3. sharded
@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("shape", ["items", "group16", "function"])
def test_sharded_engines_with_a_module_likelihood(shape, world):
    """96 chains over 2 and 3 engines (threads of this process, rows through the host transport): the ranks' columns side by side equal the
    one oracle's run; archive and adaptation state are replicated (asserted in F.run_sharded).  `function` is carried by the persistent
    kernel on every rank."""
    from pydream_amd import _capi as G
    c = config(lk=shape, items=3 if shape == "items" else 1, N=96, d=10, k=3, n=24, world=world)
    MK.code_object(shape)
    variants = []
    tr, Z, cr, _, state = F.run_sharded(G, c, variants)
    want = oracle_run(dict(c, world=1))
    assert_same(dict(trace=tr, Z=Z, cr=cr, state=state), want)
    assert variants == (["k_generations_user"] * 2 if shape == "function" else ["multi-kernel path"] * 2), variants
    assert 0.02 < tr["moved"].mean() < 0.95


# ---------------------------------------------------------------------------------------------------- 4. tempering and S1
@pytest.mark.parametrize("shape", ["thread", "function"])
def test_parallel_tempering_with_a_module_likelihood(shape):
    """8 chains on the reference's temperature ladder, a swap attempt after every generation: the swap log equals the oracle's and holds
    accepted swaps"""
    c = config(lk=shape, N=8, d=6, k=3, n=30, pt=1, thin=1, extra_rows=0)
    got, want = hip_run(c), oracle_run(c)
    np.testing.assert_array_equal(got["swaps"], want["swaps"])
    assert got["swaps"][:, 2].sum() >= 1
    assert_same(got, want)
    assert got["variants"][-1] == ("k_generations_user" if shape == "function" else "multi-kernel path")


@pytest.mark.parametrize("shape", ["thread", "function"])
def test_chain_by_chain_stepping_with_a_module_likelihood(shape):
    """schedule S1 (Dream.astep chain by chain) through dz_step_range at 5 chains against the oracle's S1"""
    from oracle import oracle as O
    from pydream_amd import _capi as G
    c = config(lk=shape, N=5, d=6, k=3, n=20, s1=1, thin=1, extra_rows=0)
    MK.code_object(shape)
    e, o = F.build(G.Engine, c, {}), F.build(O.Engine, c, {})
    x0, rows0 = e.get_state()[0].copy(), len(e.get_history())
    for _ in range(c["n"]):
        for ch in range(c["N"]):
            e.step_range(ch, 1)
    o.step(c["n"])
    np.testing.assert_array_equal(e.get_history(), o.get_history())
    for u, v in zip(tuple(e.get_cr_state()) + tuple(e.get_state()), tuple(o.get_cr_state()) + tuple(o.get_state())):
        np.testing.assert_array_equal(u, v)
    assert len(e.get_history()) == rows0 + c["N"] * c["n"] and not np.array_equal(e.get_state()[0], x0)


# ---------------------------------------------------------------------------------------------------- 5. history_lag inside k_generations_user
def test_history_lag_inside_the_persistent_user_kernel():
    """`function` at 256 chains, history_lag 2, history_thin 2: behind the burn-in a launch of k_generations_user holds up to three
    appends (history_lag + 1), the generations behind each sampling the rows of those before"""
    c = config(lk="function", N=256, d=20, k=3, n=40, lag=2, thin=2, burnin=6)
    got = hip_run(c, steps=(13, 27))
    assert_same(got, oracle_run(c, steps=(13, 27)))
    assert got["variants"] == ["k_generations_user"] * 2, got["variants"]
    assert 0.02 < got["trace"]["moved"].mean() < 0.95


# ---------------------------------------------------------------------------------------------------- 6. lane groups at ragged counts
@pytest.mark.parametrize("shape", ["group16", "group32"])
def test_lane_groups_at_ragged_point_counts(shape):
    """dz_eval_logp at 1, 15, 17 and 259 points: the last block's groups beyond the last point run too and must neither write nor disturb
    the butterfly of their neighbours; d below, at and above the group's width"""
    from pydream_amd import _capi as G
    MK.code_object(shape)
    for d in (1, 16, 17, 33):
        e = G.Engine(nchains=3, ndim=d, history_capacity=8)
        MK.apply(e, shape, d, cut=11.0)
        X = np.random.default_rng(d).uniform(-5.0, 15.0, (259, d))
        twin = MK.twin(shape, d, 11.0)
        for n in (1, 15, 17, 259):
            got = e.eval_logp(X[:n])
            np.testing.assert_array_equal(got[1], twin(X[:n])[1], err_msg="d=%d n=%d" % (d, n))
            assert not got[0].any()
        assert np.isneginf(got[1]).any() and np.isfinite(got[1]).any()
        e.close()
