"""Saturating rate laws (likelihoods.RateLaw, likelihoods.Hill) on the MI355X: the device gives the host build's bits in every shape --
one lane in the short and the long form, under both rate scales, with a box that crosses K = 0 and with a step budget that some points
exhaust; 16 lanes with conditions (the item kernel); 32 lanes; a wave per point --, run_dream on the device equals its own sequence on
the oracle, and the repressilator example runs end to end."""
import os
from unittest import mock

import numpy as np
import pytest
from scipy.stats import uniform

from pydream_amd.parameters import SampledParam

from . import ode_ratelaw_networks as RN
from . import ode_ratelaw_reference as RR
from .ode_networks import box_points
from .ode_support import device_equals_host, oracle_run_dream, run_dream_equals_oracle

pytestmark = pytest.mark.gpu


def _grammar(i, n, seed):
    net = RN.network(i)
    assert net.rate_scale == "log10"
    X = box_points(net.nominal(), n, seed, width=0.5, outside=0.05)
    return net, X


def test_one_lane_short_form_log10_equals_the_host_build():
    spec = RN.GOODWIN8                                                              # n = 8
    like = RN.build(spec)
    assert like.lanes_per_point == 1 and len(like.reactions) <= 16 and "SLOTS = 1;" in like.source()
    X = box_points(spec["nominal"], 1027, 31, width=1.0, outside=0.1)
    host = device_equals_host(like, X, spec["nominal"], width=1.0)
    assert np.mean(np.isfinite(host)) > 0.9
    short = RN.build(spec, max_steps=12)                                            # a budget some points exhaust
    host = device_equals_host(short, X, spec["nominal"], width=1.0)
    print("max_steps = 12: %d of %d points fail" % (np.sum(host == -np.inf), len(host)))
    assert np.any(host == -np.inf) and np.any(np.isfinite(host))


def test_one_lane_short_form_linear_with_a_box_across_K_equal_to_zero():
    spec = RN.MM2
    like = RN.build(spec, rate_scale="linear")
    nominal = 10.0 ** spec["nominal"]                                               # [Vmax, Km] = [1.5, 0.6]: Km in [-0.4, 1.6]
    X = box_points(nominal, 1027, 32, width=1.0, outside=0.1)
    X[:3, 1] = [0.0, -0.0, np.inf]
    host = device_equals_host(like, X, nominal, width=1.0)
    assert np.all(host[X[:, 1] <= 0] == -np.inf) and np.sum(X[:, 1] <= 0) > 100 and host[2] == -np.inf      # liveness, as the host has it
    assert np.mean(np.isfinite(host[X[:, 1] > 0.05])) > 0.9


def test_one_lane_long_form_equals_the_host_build():
    net, X = _grammar(4, 515, 33)
    like = net.like()
    assert like.lanes_per_point == 1 and len(like.reactions) > 16 and "SLOTS" in like.source()
    host = device_equals_host(like, X, net.nominal(), width=0.5)
    assert np.mean(np.isfinite(host)) > 0.5


def test_16_lanes_with_conditions_equal_the_host_build():
    spec = RN.padded(RN.MM_ENZYME, 9, 16)
    starts = [[0.5, 3.0, 0.0] + [0.0] * 6, [0.2, 5.0, 0.0] + [0.0] * 6, [1.0, 1.0, 0.5] + [0.0] * 6]
    ones = np.ones((len(spec["obs"]), len(spec["t"])))
    like = RN.build(spec, y0=None, conditions=[dict(y0=y0, data=ones * (c + 1), sd=ones) for c, y0 in enumerate(starts)])
    assert like.lanes_per_point == 16 and "DZODE_GROUP_ITEM_ENTRIES" in like.source() and "SLOTS = 1;" in like.source()
    X = box_points(spec["nominal"], 259, 34, width=1.0, outside=0.1)
    host = device_equals_host(like, X, spec["nominal"], width=1.0)
    assert np.mean(np.isfinite(host)) > 0.9


def test_32_lanes_equal_the_host_build():
    net, X = _grammar(8, 131, 35)
    like = net.like()
    assert like.lanes_per_point == 32 and like.n_species == 17 and "SLOTS" in like.source()
    host = device_equals_host(like, X, net.nominal(), width=0.5)
    assert np.mean(np.isfinite(host)) > 0.5


def test_a_wave_per_point_equals_the_host_build():
    net, X = _grammar(12, 67, 36)
    like = net.like()
    assert like.lanes_per_point == 64 and like.n_species == 33 and "SLOTS" in like.source()
    host = device_equals_host(like, X, net.nominal(), width=0.5)
    assert np.mean(np.isfinite(host)) > 0.5


def _mm2_fit():
    spec = RN.MM2
    y = RR.radau(spec["S"], RR.resolve(spec["reactions"], spec["nominal"], "log10"), spec["y0"], spec["t"])
    data = (y @ np.asarray(spec["obs"]).T).T
    return RN.build(spec, data=data, sd=0.05 * np.abs(data) + 0.01), spec["nominal"]


@pytest.mark.parametrize("multitry", [3, False])
def test_run_dream_on_the_device_equals_the_oracle(tmp_path, multitry):
    os.chdir(tmp_path)
    N, G = 8, 40
    like, nom = _mm2_fit()
    params = [SampledParam(uniform, loc=nom - 1.0, scale=2)]
    rng = np.random.default_rng(81)
    np.save("mm2_seed.npy", nom - 1.0 + 2 * rng.uniform(0, 1, (60, len(nom))))
    box = nom - 1.0 + 2 * rng.uniform(0, 1, (200, len(nom)))
    starts = list(box[np.isfinite(like.batch(box))][:N])
    assert len(starts) == N
    run_dream_equals_oracle(like, params, starts, 58, N, G, multitry=multitry, gamma_levels=4, adapt_gamma=True, history_thin=1, hardboundaries=False,
                            history_file="mm2_seed.npy")


def test_the_repressilator_example_on_the_device_equals_the_oracle(tmp_path, capsys):
    from pydream_amd.examples.repressilator import repressilator_device as REP
    os.chdir(tmp_path)
    N, G = 8, 40
    like = REP.make_likelihood()
    sampled, log_ps = REP.main(G, N, like=like)
    assert "repressilator on the device" in capsys.readouterr().out
    rng = np.random.default_rng(21)                                                 # main's own starts, prior and settings
    starts = [REP.TRUE + 0.5 * REP.WIDTH * rng.uniform(-1, 1, len(REP.TRUE)) for _ in range(N)]
    params = [SampledParam(uniform, loc=REP.TRUE - REP.WIDTH, scale=2 * REP.WIDTH)]
    with mock.patch.dict(os.environ, DREAMZS_HOST_WORKERS="1"):
        o_s, o_l = oracle_run_dream(params, lambda x: like(x), N, G, starts, 22, multitry=5, model_name="repressilator_device")
    assert np.all(np.isfinite(np.array(log_ps))) and len(np.unique(np.concatenate(sampled)[:, 0])) > N
    np.testing.assert_array_equal(np.array(sampled), np.array(o_s))
    np.testing.assert_array_equal(np.array(log_ps), np.array(o_l))
