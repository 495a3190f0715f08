"""MassActionODELogLike(lanes_per_point=16 | 32) on the MI355X: the lane-group solver gives its host twin's bits (also where failed and
finished points share a wave), run_dream with it equals the oracle driven by the host twin, what the sampler consumed agrees with an
independent scipy Radau likelihood, and the engine launches any user kernel with 16 or 32 lanes per point."""
import os

import numpy as np
import pytest
from scipy.stats import uniform

from pydream_amd import _capi
from pydream_amd.core import run_dream
from pydream_amd.parameters import SampledParam

from . import ode_networks as NW
from . import ode_wide_networks as W
from .ode_support import device_equals_host, device_logp, run_dream_equals_oracle

pytestmark = pytest.mark.gpu

N_POINTS = 4099           # not a multiple of the 16 (or 8) points of a block: the last block has groups without a point


@pytest.mark.parametrize("starved", [False, True])
@pytest.mark.parametrize("name", list(W.CASES))
def test_device_equals_host_twin_bit_for_bit(name, starved):
    make, nom, _ = W.CASES[name]
    like = make(max_steps=W.STARVED_MAX_STEPS[name]) if starved else make()
    X = NW.box_points(nom, N_POINTS, 21, width=1.0, outside=0.05 / len(nom))      # a few points outside the prior's support
    host = device_equals_host(like, X, nom)
    failed = host == -np.inf
    print("%s: %d of %d points -inf" % (name, failed.sum(), len(X)))
    outside = np.any((X < nom - 1.0) | (X > nom + 1.0), axis=1)
    assert outside.any()
    if starved:                                                         # failed and finished points inside one wave
        per_wave = 64 // like.lanes_per_point
        waves = failed[:len(X) // per_wave * per_wave].reshape(-1, per_wave)
        assert np.any(waves.any(axis=1) & ~waves.all(axis=1))
    else:
        assert np.all(np.isfinite(host[~outside]))


@pytest.mark.parametrize("S,R,lanes", [(32, 128, 32), (16, 128, 16)])
def test_device_equals_host_twin_on_a_network_at_the_reaction_limit(S, R, lanes):
    """128 bimolecular reactions: the longest generated sums the class accepts, same bits on both sides."""
    like = W.dense_network(S, R, lanes)
    X = NW.box_points(np.zeros(20), 1027, 4, width=1.0)
    pr, lk = device_logp(like, X, np.full(20, -1.0), 2.0)
    host, steps = like.batch(X, return_steps=True)
    print("dense S=%d R=%d: %d of %d points -inf, median %d steps" % (S, R, np.sum(host == -np.inf), len(X), np.median(steps)))
    assert lk.tobytes() == host.tobytes()
    assert np.mean(np.isfinite(host)) > 0.9


@pytest.mark.parametrize("multitry,hard,max_steps", [(False, True, 500), (3, False, 75)])
def test_run_dream_on_the_device_equals_the_oracle(tmp_path, multitry, hard, max_steps):
    """enzyme13 with 16 lanes per point against run_dream's own sequence on the oracle with the host twin as the Python likelihood; with
    max_steps 75 half of the prior box fails, so whole proposal sets are impossible and drawn again."""
    os.chdir(tmp_path)
    N, G = 8, 40
    like = W.enzyme13(max_steps=max_steps)
    nom = W.ENZ.NOMINAL
    params = [SampledParam(uniform, loc=nom - 1.0, scale=2)]
    rng = np.random.default_rng(78)
    Z0 = nom - 1.0 + 2 * rng.uniform(0, 1, (60, len(nom)))
    np.save("enz_seed.npy", Z0)
    if max_steps < 500:
        assert np.mean(like.batch(Z0) == -np.inf) > 0.2
    starts = [nom + 0.1 * rng.uniform(-1, 1, len(nom)) for _ in range(N)]
    kw = dict(multitry=multitry, gamma_levels=4, adapt_gamma=True, history_thin=1, hardboundaries=hard, history_file="enz_seed.npy")
    run_dream_equals_oracle(like, params, starts, 56, N, G, **kw)


def test_the_trace_agrees_with_an_independent_radau_likelihood(tmp_path):
    """200 (x, log p) pairs the device run produced: log p = uniform prior + the Gaussian log likelihood of a scipy Radau solution."""
    import multiprocessing
    from concurrent.futures import ProcessPoolExecutor
    os.chdir(tmp_path)
    like = W.enzyme13()
    nom = W.ENZ.NOMINAL
    params = [SampledParam(uniform, loc=nom - 1.0, scale=2)]
    N, G = 64, 40
    rng = np.random.default_rng(5)
    np.save("seed.npy", NW.box_points(nom, 300, 6, width=1.0))
    starts = [nom + 0.5 * rng.uniform(-1, 1, len(nom)) for _ in range(N)]
    sampled, log_ps = run_dream(params, like, nchains=N, niterations=G, verbose=False, start=starts, save_history=False, seed=9, multitry=5,
                                history_file="seed.npy")
    S, L = np.concatenate(sampled), np.concatenate(log_ps).reshape(-1)
    pick = np.random.default_rng(1).choice(len(S), 200, replace=False)
    prior = float(np.sum(uniform(loc=nom - 1.0, scale=2).logpdf(nom)))
    with ProcessPoolExecutor(max(1, min(8, len(os.sched_getaffinity(0)))), mp_context=multiprocessing.get_context("spawn")) as ex:
        refs = list(ex.map(W.enzyme_radau_loglike, [(S[i], like.data, like.sd) for i in pick], chunksize=5))
    for i, (total, magnitude) in zip(pick, refs):
        ref = prior + total
        assert abs(L[i] - ref) <= 1e-6 * (abs(prior) + magnitude), (S[i], L[i], ref)      # (relative to the sum's terms: log p itself can be near 0)


@pytest.mark.parametrize("lanes", [16, 32])
def test_a_user_kernel_with_a_lane_group_per_point(lanes):
    """DeviceKernelLogLike(lanes_per_point=16 | 32): point i on lanes [i * L, (i + 1) * L) of the grid, 256 / L points per block; the
    groups past the last point are predicated, not returned, in front of the group's butterfly."""
    from pydream_amd.likelihoods import DeviceKernelLogLike
    src = r'''
    #define L %d
    extern "C" __global__ void sq_dist(const double* X, long long n, int d, int ld, double* like, const void* data)
    {
        const long long i = (blockIdx.x * 256ll + threadIdx.x) / L;
        const int lane = threadIdx.x %% L;
        const bool valid = i < n;
        const double* x = X + (valid ? i : n - 1) * ld;
        const double* c = (const double*)data;
        double acc = 0.0;
        for (int j = lane; j < d; j += L) { const double t = x[j] - c[j]; acc = acc + t * t; }
        for (int o = L / 2; o > 0; o >>= 1) acc = acc + __shfl_xor(acc, o, L);
        if (valid && lane == 0) like[i] = -0.5 * acc;
    }''' % lanes
    d = 150
    c = np.linspace(-1, 1, d)
    like = DeviceKernelLogLike("sq_dist", d, source=src, data=c, lanes_per_point=lanes)
    X = np.random.default_rng(0).normal(size=(37, d))                  # 37: neither a multiple of 16 nor of 8

    def twin(x):          # the same order of additions: lane l adds j = l, l + L, ...; then the xor butterfly L/2 .. 1
        part = np.zeros(lanes)
        for j in range(d):
            t = x[j] - c[j]; part[j % lanes] = part[j % lanes] + t * t
        o = lanes // 2
        while o:
            part = part + part[np.arange(lanes) ^ o]
            o //= 2
        return -0.5 * part[0]
    e = _capi.Engine(nchains=3, ndim=d, history_capacity=8)
    like._dz_apply(e)
    np.testing.assert_array_equal(e.eval_logp(X)[1], np.array([twin(x) for x in X]))
    np.testing.assert_array_equal(np.array([like(x) for x in X[:3]]), np.array([twin(x) for x in X[:3]]))
    with pytest.raises(_capi.DreamZSError, match="lanes_per_point"):
        e.set_likelihood_module(like.code_object(), "sq_dist", 8)
