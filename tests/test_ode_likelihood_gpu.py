"""MassActionODELogLike on the MI355X: the gfx950 solver gives the host build's bits, run_dream with it equals the oracle driven by the
host build, and what the sampler consumed agrees with an independent scipy Radau likelihood."""
import os

import numpy as np
import pytest
from scipy.stats import uniform

from pydream_amd.core import run_dream
from pydream_amd.parameters import SampledParam

from . import ode_networks as NW
from .ode_support import device_equals_host, run_dream_equals_oracle

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("net", ["robertson", "mm", "chain8"])
def test_device_equals_host_build_bit_for_bit(net):
    if net == "robertson":
        like, nom, n, w = NW.robertson(), NW.ROB.NOMINAL, 20480, 3.0
    elif net == "mm":
        like, nom, n, w = NW.michaelis_menten(), NW.MM_NOMINAL, 2048, 1.0
    else:
        like, nom, n, w = NW.chain8(), NW.CHAIN_NOMINAL, 1024, 1.0
    X = NW.box_points(nom, n, 21, width=w, outside=0.05 * w)           # a few points outside the prior's support
    host = device_equals_host(like, X, nom, w)
    outside = np.any((X < nom - w) | (X > nom + w), axis=1)
    assert outside.any() and np.all(np.isfinite(host[~outside]))


@pytest.mark.parametrize("multitry,hard,max_steps", [(False, True, 500), (3, False, 30)])
def test_run_dream_on_the_device_equals_the_oracle(tmp_path, multitry, hard, max_steps):
    """The example's call with the device likelihood against run_dream's own sequence on the oracle with the host build as the Python
    likelihood; with max_steps 30 a third of the prior box fails, so whole proposal sets are impossible and drawn again."""
    os.chdir(tmp_path)
    N, G = 5, 50
    like = NW.robertson(max_steps=max_steps)
    lower = NW.ROB_LOWER
    params = [SampledParam(uniform, loc=lower, scale=6)]
    rng = np.random.default_rng(78)
    Z0 = lower + 6 * rng.uniform(0, 1, (40, 3))
    np.save("rob_seed.npy", Z0)
    if max_steps < 500:
        assert np.mean(like.batch(Z0) == -np.inf) > 0.2
    starts = [NW.ROB.NOMINAL + 0.3 * rng.uniform(-1, 1, 3) for _ in range(N)]
    kw = dict(multitry=multitry, gamma_levels=4, adapt_gamma=True, history_thin=1, hardboundaries=hard, history_file="rob_seed.npy")
    run_dream_equals_oracle(like, params, starts, 56, N, G, **kw)


def test_the_trace_agrees_with_an_independent_radau_likelihood(tmp_path):
    """200 (x, log p) pairs the device run produced: log p = uniform prior + the Gaussian log likelihood of a scipy Radau solution."""
    from scipy.stats import norm
    os.chdir(tmp_path)
    like = NW.robertson()
    lower = NW.ROB_LOWER
    params = [SampledParam(uniform, loc=lower, scale=6)]
    N, G = 64, 40
    rng = np.random.default_rng(5)
    np.save("seed.npy", NW.box_points(NW.ROB.NOMINAL, 300, 6))
    starts = [NW.ROB.NOMINAL + 0.5 * rng.uniform(-1, 1, 3) for _ in range(N)]
    sampled, log_ps = run_dream(params, like, nchains=N, niterations=G, verbose=False, start=starts, save_history=False, seed=9, multitry=5,
                                history_file="seed.npy")
    S, L = np.concatenate(sampled), np.concatenate(log_ps).reshape(-1)
    pick = np.random.default_rng(1).choice(len(S), 200, replace=False)
    prior = float(np.sum(uniform(loc=lower, scale=6).logpdf(NW.ROB.NOMINAL)))
    for i in pick:
        c = NW.radau(3, NW.ROB.REACTIONS, NW.ROB.Y0, NW.ROB.TSPAN, S[i], rtol=1e-10, atol=1e-14)[:, 2]
        terms = norm(loc=like.data[0], scale=like.sd[0]).logpdf(c)
        ref = prior + float(np.sum(terms))
        assert abs(L[i] - ref) <= 1e-6 * (abs(prior) + float(np.sum(np.abs(terms)))), (S[i], L[i], ref)      # (relative to the sum's terms: log p itself can be near 0)
