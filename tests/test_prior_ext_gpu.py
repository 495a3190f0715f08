"""The extended device priors on the GPU: k_prior_ext beside every producer of the likelihood column (dz_eval_logp), whole trajectories against the oracle
on the host twin's bits, and run_dream with an ODE likelihood that never leaves the device.

What holds the kernel's values: its prior column equals the host twin (dz_prior_ext_host, the same header's functions in the same order) bit for bit on
EVERY row, and lies inside tests/prior_reference.py's derived bound on the first nine rows of every point set (the n = 1 and n = 9 sets are prefixes of
the n = 260 set; the 40-digit reference of 260 x 130 terms would take half a minute, and the twin itself is held to the bound on every input of
prior_reference.cases() in tests/test_prior_ext_cpu.py)."""
import numpy as np
import pytest
import scipy.stats as st

from oracle import oracle as O
from pydream_amd import _capi
from tests import prior_ext_cases as PC
from tests import prior_reference as REF

pytestmark = pytest.mark.gpu

NS = (1, 9, 260)          # one point; a partial block of 4-wave blocks; more than one block, the last one partial
# d: one dimension (gamma, k = 0.5: both infinities); every kind 1..13 once; flat dimensions interleaved; two 128-chunks, the last lane pair half empty
SHAPES = {1: dict(first=6), 13: dict(), 26: dict(flat_every=2), 130: dict()}
_SETS = {}


def point_set(d):
    """(prior tuple, X[260, d], ref[9], bound[9]), made once per d"""
    if d not in _SETS:
        kind, a, b, s1, s2, X = REF.mixed_point_set(d, max(NS), seed=900 + d, **SHAPES[d])
        ref, bound = REF.points(kind, a, b, s1, s2, X[:9])
        _SETS[d] = ((kind, a, b, s1, s2), X, ref, bound)
    return _SETS[d]


def check_prior_column(pr, prior, X, ref, bound, what):
    twin = _capi.prior_ext_host(*prior, X)
    twin = np.where(np.isnan(twin), -np.inf, twin)          # (the kernel's nan_to_ninf)
    np.testing.assert_array_equal(pr, twin, err_msg=what)
    assert (np.signbit(pr) == np.signbit(twin))[pr != 0].all()
    for i in range(min(9, len(X))):
        assert REF.agrees(pr[i], ref[i], bound[i]), (what, i, pr[i], float(ref[i]), float(bound[i]))


def producers(d):
    """name -> a function that gives an engine its likelihood"""
    rng = np.random.default_rng(40 + d)
    U = np.triu(rng.normal(0, 0.3, (d, d))) + np.diag(1.0 + rng.uniform(0, 1, d))
    mu = rng.normal(0, 1, d)
    mus = rng.normal(0, 2, (3, d))
    F = rng.normal(-1, 0.5, 3)
    w = 0.5 + rng.uniform(0, 1, d)

    def host(X):
        return np.zeros(len(X)), -0.5 * np.sum(w * X * X, axis=1)

    return {"mvn": lambda e: e.set_likelihood_mvn(mu, U, 1, -0.25), "mixture": lambda e: e.set_likelihood_mixture(mus, F), "host": lambda e: e.set_likelihood_host(host)}


@pytest.mark.parametrize("d", sorted(SHAPES))
@pytest.mark.parametrize("name", ["mvn", "mixture", "host"])
def test_the_prior_column_beside_the_built_in_producers(name, d):
    """dz_eval_logp with set_prior_ext beside the triangular MVN (d = 130: the tiled kernel and k_q_finish), the mixture and a host callback: the prior
    column as the module docstring says; the likelihood column is what the same call returns with flat priors, bit for bit"""
    prior, X, ref, bound = point_set(d)
    apply = producers(d)[name]
    ext, flat = _capi.Engine(nchains=4, ndim=d, history_capacity=8), _capi.Engine(nchains=4, ndim=d, history_capacity=8)
    ext.set_prior_ext(*prior)
    apply(ext); apply(flat)
    for n in NS:
        pr, lk = ext.eval_logp(X[:n])
        pr0, lk0 = flat.eval_logp(X[:n])
        assert not pr0.any()
        assert lk.tobytes() == lk0.tobytes(), (name, d, n)
        check_prior_column(pr, prior, X[:n], ref, bound, "%s d=%d n=%d" % (name, d, n))
    assert np.isneginf(pr).any() and np.isfinite(pr).any() and (d != 1 or np.isposinf(pr).any())      # (of the n = 260 set)
    ext.close(); flat.close()


def test_every_kind_up_to_2_is_set_prior_itself():
    """dz_set_prior_ext with no kind above 2 calls dz_set_prior: the built-in kernels evaluate the prior (the persistent kernel stays eligible)"""
    d, N = 10, 64
    rng = np.random.default_rng(3)
    kind = np.array([0, 1, 2, 1, 2, 0, 1, 2, 1, 1], np.int32)
    a, b = rng.normal(0, 1, d), rng.uniform(0.5, 3, d)
    X = a + b * rng.uniform(-0.2, 1.2, (33, d))
    Z0 = a + b * rng.uniform(0.1, 0.9, (200, d))
    out = []
    for how in ("ext", "plain"):
        e = _capi.Engine(nchains=N, ndim=d, multitry=3, history_capacity=len(Z0) + N * 8, trace_capacity=20, seed=5)
        e.set_prior_ext(kind, a, b, np.zeros(d), np.zeros(d)) if how == "ext" else e.set_prior(kind, a, b)
        e.set_bounds(np.where(kind == 2, a, -np.inf), np.where(kind == 2, a + b, np.inf))
        e.set_likelihood_mvn(np.zeros(d), np.eye(d), 1, 0.0)
        e.set_history(Z0); e.set_state(Z0[:N])
        pr, lk = e.eval_logp(X)
        e.step(20)
        out.append((pr, lk, e.get_trace(0, 20), e.last_kernel_variant()))
        e.close()
    assert out[0][3] == out[1][3]
    assert out[0][0].tobytes() == out[1][0].tobytes() and out[0][1].tobytes() == out[1][1].tobytes()
    for key in ("X", "logp", "moved", "try_idx"):
        np.testing.assert_array_equal(out[0][2][key], out[1][2][key])


@pytest.fixture(scope="module")
def ode_models():
    from pydream_amd.examples.dose_response import dose_response_device as DOSE
    from pydream_amd.examples.noise import noise_device as NOISE
    return {"plain": (NOISE.make_likelihood(), NOISE.TRUE), "conditions": (DOSE.make_likelihood(), DOSE.NOMINAL)}


@pytest.mark.parametrize("which", ["plain", "conditions"])
def test_the_prior_column_beside_an_ode_module(ode_models, which):
    """a MassActionODELogLike module without conditions (the Robertson fit with sampled noise, d = 5) and with conditions (the dose series: six items per
    point, k_sum_items in front of k_prior_ext): the prior column as above around points near the nominal one -- the kinds 3..13 cycle over the
    dimensions, some rows outside a support --, the likelihood column that of flat priors"""
    like, centre = ode_models[which]
    d = len(centre)
    rng = np.random.default_rng(17)
    X = centre + 0.05 * rng.uniform(-1, 1, (max(NS), d))
    kind = (3 + (np.arange(d) * 3) % 11).astype(np.int32)
    shapes = [REF.SHAPES[int(k)][-1] for k in kind]
    s1, s2 = np.array([s[0] for s in shapes]), np.array([s[1] for s in shapes])
    lo = np.array([REF.z_support(int(k), *s)[0] for k, s in zip(kind, shapes)])
    b = np.full(d, 0.5)
    a = np.where(np.isfinite(lo), centre - 0.5 * b * (np.where(np.isfinite(lo), lo, 0.0) + 1.0), centre)      # z near lo + 1 (bounded below) or 0
    jb = int(np.flatnonzero(lo == 0.0)[0])
    a[jb] = centre[jb] + 0.02                                                                                  # the first dimension bounded at z = 0: some rows outside
    prior = (kind, a, b, s1, s2)
    ref, bound = REF.points(kind, a, b, s1, s2, X[:9])
    ext, flat = _capi.Engine(nchains=4, ndim=d, history_capacity=8), _capi.Engine(nchains=4, ndim=d, history_capacity=8)
    ext.set_prior_ext(*prior)
    like._dz_apply(ext); like._dz_apply(flat)
    for n in NS:
        pr, lk = ext.eval_logp(X[:n])
        pr0, lk0 = flat.eval_logp(X[:n])
        assert not pr0.any() and np.isfinite(lk0).all()
        assert lk.tobytes() == lk0.tobytes(), (which, n)
        check_prior_column(pr, prior, X[:n], ref, bound, "ode %s n=%d" % (which, n))
    assert np.isfinite(pr).any()
    ext.close(); flat.close()


# ------------------------------------------------------------------------------------------------------------------ trajectories
def run(Cls, k, hard, apply):
    e = PC.make(Cls, k, hard, likelihood=apply)
    e.step(PC.GENS)
    hip = Cls is _capi.Engine
    out = dict(trace=e.get_trace(0, PC.GENS), Z=e.get_history(), cr=e.get_cr_state(), state=e.get_state(),
               variant=e.last_kernel_variant() if hip else None, redraws=e.redraw_rounds() if hip else None)
    e.close()
    return out


def assert_same(a, b):
    for key in ("snooker", "cr_idx", "try_idx", "moved", "X", "logp"):
        np.testing.assert_array_equal(a["trace"][key], b["trace"][key], err_msg=key)
    np.testing.assert_array_equal(a["Z"], b["Z"])
    for u, v in zip(a["cr"] + a["state"], b["cr"] + b["state"]):
        np.testing.assert_array_equal(u, v)


@pytest.mark.parametrize("hard", [1, 0])
@pytest.mark.parametrize("k", [3, 1])
def test_trajectories_equal_the_oracle_on_the_twins_bits(k, hard):
    """8 chains, d = 6, the kinds 3, 6, 7 (k = 1), 9, 11 and 1 mixed (tests/prior_ext_cases.py), 60 generations through a crossover burn-in: engine and
    oracle both run a host callback for the likelihood; the engine adds the device prior, the oracle's callback fills its prior column from
    prior_ext_host.  States, log densities, decisions, the archive and the crossover state are equal bit for bit, on the multi-kernel path.
    Multitry 3 without hard boundaries is the configuration whose archive reaches 4 scales beyond the supports: the oracle alone draws whole proposal
    sets again in 10 % .. 60 % of its chain steps (checked on the CPU: tests/test_prior_ext_cpu.py), so the engine must report redraw rounds."""
    sizes = []
    o = run(O.Engine, k, hard, lambda e: e.set_likelihood_host(PC.oracle_callback(sizes=sizes)))

    def device_prior(e):
        e.set_prior_ext(*PC.PRIOR)
        e.set_likelihood_host(PC.engine_callback())
    g = run(_capi.Engine, k, hard, device_prior)
    assert g["variant"] == "multi-kernel path"
    assert_same(g, o)
    assert np.isfinite(g["trace"]["logp"]).all() and g["trace"]["moved"].any()
    if k == 3 and not hard:
        assert 0.10 <= PC.redrawn_fraction(sizes[PC.N:], k) <= 0.60
        assert g["redraws"] > 0


@pytest.mark.parametrize("hard", [1, 0])
@pytest.mark.parametrize("k", [3, 1])
def test_trajectories_with_the_device_mvn_beside_the_device_prior(k, hard):
    """the same once more with the device MVN on the engine's side (no host callback at all) and the oracle's own MVN log likelihood inside the oracle's
    callback: the same bits as long as the two likelihood kinds follow the same schedule in the oracle, which they do -- a redraw is decided from the
    log densities alone"""
    rng = np.random.default_rng(8)
    U = np.triu(rng.normal(0, 0.2, (PC.D, PC.D))) + np.diag(np.sqrt(PC.WEIGHT))
    mvn = O.Engine(nchains=1, ndim=PC.D, history_capacity=8)
    mvn.set_likelihood_mvn(PC.CENTRE, U, 1, 0.5)
    like = lambda X: np.array([mvn.loglike(x) for x in X])
    o = run(O.Engine, k, hard, lambda e: e.set_likelihood_host(PC.oracle_callback(like=like)))

    def device(e):
        e.set_prior_ext(*PC.PRIOR)
        e.set_likelihood_mvn(PC.CENTRE, U, 1, 0.5)
    g = run(_capi.Engine, k, hard, device)
    assert g["variant"] == "multi-kernel path"
    assert_same(g, o)
    if k == 3 and not hard:
        assert g["redraws"] > 0


# ------------------------------------------------------------------------------------------------------------------ run_dream
def robertson_run(monkeypatch, sigma_prior):
    from pydream_amd import core
    from pydream_amd.examples.priors import priors_device as EX
    from pydream_amd.likelihoods import MassActionODELogLike, Noise
    from pydream_amd.examples.noise import noise_device as NOISE
    from pydream_amd.examples.robertson import robertson_device as ROB
    from pydream_amd.parameters import SampledParam
    like = MassActionODELogLike(3, ROB.REACTIONS, ROB.Y0, NOISE.TSPAN, [[0, 0, 1]], NOISE.simulated_data()[None, :], None, rate_scale="linear", noise=[Noise(3)])
    true = np.r_[10.0 ** ROB.NOMINAL, 0.006]
    params = [SampledParam(st.norm, loc=true[0], scale=0.1 * true[0]), SampledParam(st.lognorm, 0.5, scale=true[1:3]), sigma_prior]
    calls = dict(call=0, batch=0)
    batch, call = type(like).batch, type(like).__call__
    monkeypatch.setattr(type(like), "batch", lambda self, *a, **kw: (calls.__setitem__("batch", calls["batch"] + 1), batch(self, *a, **kw))[1])
    monkeypatch.setattr(type(like), "__call__", lambda self, *a, **kw: (calls.__setitem__("call", calls["call"] + 1), call(self, *a, **kw))[1])
    rng = np.random.default_rng(4)
    starts = [true * np.exp(0.05 * rng.uniform(-1, 1, 4)) for _ in range(8)]
    sampled, log_ps = core.run_dream(params, like, niterations=30, nchains=8, multitry=3, start=starts, model_name="prior_ext_test", verbose=False,
                                     save_history=False, seed=9)
    entered = dict(calls)
    monkeypatch.undo()
    return like, params, np.concatenate(sampled), np.concatenate(log_ps).reshape(-1), entered, core.last_kernel_variant


def test_run_dream_keeps_an_ode_likelihood_on_the_device_under_extended_priors(monkeypatch):
    """Robertson, rate_scale "linear", sampled sigma; priors [norm, lognorm, halfnorm]; 8 chains x 30 iterations.  The likelihood object's host
    __call__ and batch are never entered, and every returned log p is prior_ext_host(row) + like.batch(row) of its sample to the bit (the ODE host
    build gives the device's bits; the engine adds prior + 1.0 * like, the same one addition)."""
    from pydream_amd.model import Model
    from pydream_amd.parameters import SampledParam
    like, params, S, L, entered, variant = robertson_run(monkeypatch, SampledParam(st.halfnorm, scale=0.02))
    assert entered == dict(call=0, batch=0), entered
    assert variant == "multi-kernel path"
    ext = Model(like, params).device_prior_ext()
    want = _capi.prior_ext_host(*ext, S) + like.batch(S)
    assert np.isfinite(L).all() and len(np.unique(L)) > 8
    assert L.tobytes() == want.tobytes(), np.abs(L - want).max()


def test_run_dream_with_a_family_that_has_no_device_form_takes_the_host_path_as_before(monkeypatch):
    from pydream_amd.parameters import SampledParam
    like, params, S, L, entered, variant = robertson_run(monkeypatch, SampledParam(st.weibull_min, 1.5, scale=0.02))
    assert entered["call"] + entered["batch"] > 0
    assert np.isfinite(L).all()
