"""Sampled noise models (likelihoods.Noise) on the MI355X: the device gives the host build's bits in every shape -- one lane in the
short and the long form, 16 lanes with conditions (the item kernel), 32 lanes, a wave per point --, on point sets that hold rows outside
the prior box and rows whose noise coordinates are not live, and with a step budget that some points exhaust; run_dream on the device
with a sampled sigma equals its own sequence on the oracle, and the example with unknown noise runs end to end."""
import os
from unittest import mock

import numpy as np
import pytest
from scipy.stats import uniform

from pydream_amd.likelihoods import Monomial, Noise
from pydream_amd.parameters import SampledParam

from . import ode_noise_networks as NN
from .ode_support import device_equals_host, device_logp, oracle_run_dream, run_dream_equals_oracle

pytestmark = pytest.mark.gpu


def _device_equals_host(like, net, X):
    """ode_support.device_equals_host on the rows of X under the prior box of the point sets; the rows with a NaN coordinate apart, with
    the likelihood alone (that helper's test of the prior puts every row inside the box or outside it, and a NaN is neither): the
    device's bytes are the host build's and say -inf.  Returns the host build's values."""
    nan = np.any(np.isnan(X), axis=1)
    host = np.zeros(len(X))
    host[~nan] = device_equals_host(like, X[~nan], NN.nominal(net), width=NN.WIDTH)
    _, lk = device_logp(like, X[nan], NN.nominal(net) - NN.WIDTH, 2 * NN.WIDTH)
    host[nan] = like.batch(X[nan])
    assert np.sum(nan) >= 1 and lk.tobytes() == host[nan].tobytes() and np.all(lk == -np.inf)
    return host


def _equal(like, net, noise, n, seed):
    """The device's bytes are the host build's on n points; the rows whose noise is not live are -inf on both sides, and of the others
    more than half are finite.  Returns (X, dead, host)."""
    X, dead = NN.points(net, n, seed, noise)
    host = _device_equals_host(like, net, X)
    assert np.sum(dead) >= 4 and np.all(host[dead] == -np.inf)
    assert np.mean(np.isfinite(host[~dead])) > 0.5
    return X, dead, host


def test_one_lane_short_form_equals_the_host_build():
    net = NN.network("one3")
    noise = [Noise(net.P, rel=Monomial({net.P + 1: 1}, -0.3)), None, Noise(net.P + 1, dist="laplace")]      # normal, lin, sigma index plus rel Monomial
    like = NN.like(net, noise)
    assert like.lanes_per_point == 1 and len(like.reactions) <= 16 and like.rate_scale == "linear" and "NOISE = true;" in like.source()
    X, dead, _ = _equal(like, net, noise, 1027, 41)
    short = NN.like(net, noise, max_steps=12, rtol=1e-6, atol=1e-8)               # a budget that about half of the live points exhaust
    host = _device_equals_host(short, net, X)
    print("max_steps = 12: %d of %d live points fail" % (np.sum(host[~dead] == -np.inf), np.sum(~dead)))
    assert np.any(host[~dead] == -np.inf) and np.any(np.isfinite(host))


def test_one_lane_long_form_equals_the_host_build():
    net = NN.network("long8")
    noise = [Noise(net.P, dist="laplace"), Noise(0.4, rel=net.P + 1, dist="laplace"), None]
    like = NN.like(net, noise)
    assert like.lanes_per_point == 1 and len(like.reactions) > 16 and like.rate_scale == "log10"
    _equal(like, net, noise, 515, 42)


def test_16_lanes_with_conditions_equal_the_host_build():
    net = NN.network("group16")
    noise = [Noise(net.P, scale="log"), Noise(Monomial({net.P: 1, net.P + 1: -1}, -0.5), dist="laplace", scale="log"), Noise(net.P + 1, rel=0.1)]
    conds = [dict(zip(("data", "sd"), NN.data_and_weights(net, s)), y0=net.y0 * f) for s, f in ((5, 1.0), (6, 0.5), (7, 2.0))]
    like = NN.like(net, noise, conditions=conds)
    assert like.lanes_per_point == 16 and "DZODE_GROUP_ITEM_ENTRIES" in like.source() and "dzode::dlog(m)" in like.source()
    _equal(like, net, noise, 259, 43)


def test_32_lanes_equal_the_host_build():
    net = NN.network("group32")
    noise = NN.cases(net.P)["all_three"]
    like = NN.like(net, noise)
    assert like.lanes_per_point == 32 and like.n_species == 17 and like.rate_scale == "linear"
    _equal(like, net, noise, 131, 44)


def test_a_wave_per_point_equals_the_host_build():
    net = NN.network("wave64")
    noise = [Noise(net.P, rel=net.P + 1), None]                                   # one observable with a Noise, one without
    obs = NN.observables(net)[:2]
    data, sd = NN.data_and_weights(net, 9)
    like = net.like(observables=obs, ndim=net.P + 2, noise=noise, data=data[:2], sd=sd[:2])
    assert like.lanes_per_point == 64 and like.n_species == 33
    _equal(like, net, noise, 67, 45)


def _sigma_fit():
    """The three-species network's own simulation at its nominal point as data, read with a sampled sigma"""
    net = NN.network("one3")
    noise = [Noise(net.P), Noise(net.P, dist="laplace", scale="log"), None]
    nom = NN.nominal(net)[:net.P + 1]
    obs = NN.observables(net)
    sim = net.like(observables=obs).simulate(nom[:net.P])[0].T
    data = sim * (1.0 + 0.1 * np.random.default_rng(3).standard_normal(sim.shape))
    return net.like(observables=obs, ndim=net.P + 1, noise=noise, data=data, sd=np.where(np.arange(3)[:, None] == 2, 0.1, 1.0) * np.ones_like(data)), nom


@pytest.mark.parametrize("multitry", [3, False])
def test_run_dream_with_a_sampled_sigma_equals_the_oracle(tmp_path, multitry):
    os.chdir(tmp_path)
    N, G = 8, 40
    like, nom = _sigma_fit()
    lower = nom - 0.25                                                            # ("linear": sigma in 0.05 .. 0.55)
    params = [SampledParam(uniform, loc=lower, scale=0.5)]
    rng = np.random.default_rng(82)
    np.save("sigma_seed.npy", lower + 0.5 * rng.uniform(0, 1, (60, len(nom))))
    box = lower + 0.5 * rng.uniform(0, 1, (200, len(nom)))
    starts = list(box[np.isfinite(like.batch(box))][:N])
    assert len(starts) == N
    run_dream_equals_oracle(like, params, starts, 59, N, G, multitry=multitry, gamma_levels=4, adapt_gamma=True, history_thin=1, hardboundaries=False,
                            history_file="sigma_seed.npy")


def test_the_noise_example_on_the_device_equals_the_oracle(tmp_path, capsys):
    from pydream_amd.examples.noise import noise_device as ND
    os.chdir(tmp_path)
    N, G = 8, 40
    like = ND.make_likelihood()
    sampled, log_ps = ND.main(G, N, like=like)
    assert "unknown noise on the device" in capsys.readouterr().out
    rng = np.random.default_rng(31)                                                 # main's own starts, prior and settings
    starts = [ND.TRUE + 0.25 * ND.WIDTH * rng.uniform(-1, 1, len(ND.TRUE)) for _ in range(N)]
    params = [SampledParam(uniform, loc=ND.TRUE - ND.WIDTH, scale=2 * ND.WIDTH)]
    with mock.patch.dict(os.environ, DREAMZS_HOST_WORKERS="1"):
        o_s, o_l = oracle_run_dream(params, lambda x: like(x), N, G, starts, 32, multitry=5, model_name="noise_device")
    assert np.all(np.isfinite(np.array(log_ps))) and len(np.unique(np.concatenate(sampled)[:, 0])) > N
    np.testing.assert_array_equal(np.array(sampled), np.array(o_s))
    np.testing.assert_array_equal(np.array(log_ps), np.array(o_l))
