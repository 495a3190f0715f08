"""The shipped example of normalised readouts on the MI355X: the device gives the host build's bits on prior draws, main() on the device
equals main(host=True) sample for sample -- posterior-predictive bands included --, and a short run_dream equals the oracle driven by the
host build."""
import os

import numpy as np
import pytest
from scipy.stats import uniform

from pydream_amd.examples.normalized import normalized_device as ND
from pydream_amd.parameters import SampledParam

from .ode_support import device_equals_host, run_dream_equals_oracle
from .test_ode_normalize_example_cpu import data

pytestmark = pytest.mark.gpu


def test_the_example_on_the_device_equals_the_host_build():
    """259 draws of the prior box and a little beyond"""
    like = ND.make_likelihood(data=data())
    X = ND.NOMINAL - 1.05 + 2.1 * np.random.default_rng(52).uniform(size=(259, 7))
    host = device_equals_host(like, X, ND.NOMINAL, ND.WIDTH)
    assert np.isfinite(host).sum() > 200


def test_run_dream_with_the_example_on_the_device_equals_the_oracle(tmp_path):
    """8 chains, 40 generations, multitry 3"""
    os.chdir(tmp_path)
    N, G = 8, 40
    like = ND.make_likelihood(data=data())
    params = [SampledParam(uniform, loc=ND.NOMINAL - ND.WIDTH, scale=2 * ND.WIDTH)]
    rng = np.random.default_rng(83)
    np.save("normalized_seed.npy", ND.NOMINAL + ND.WIDTH * rng.uniform(-1, 1, (70, 7)))
    starts = [ND.NOMINAL + 0.25 * rng.uniform(-1, 1, 7) for _ in range(N)]
    run_dream_equals_oracle(like, params, starts, 59, N, G, multitry=3, history_thin=1, hardboundaries=False, history_file="normalized_seed.npy")


def test_main_on_the_device_equals_its_host_likelihood_run(tmp_path, capsys):
    """64 chains, 60 iterations, multitry 5, a fixed seed: main() on the device gives, sample for sample, what main(host=True) gives"""
    os.chdir(tmp_path)
    like = ND.make_likelihood(data=data())
    sampled, log_ps, bands = ND.main(60, 64, like=like)
    assert "on the device" in capsys.readouterr().out
    h_sampled, h_log_ps, h_bands = ND.main(60, 64, host=True, like=like)
    assert np.all(np.isfinite(np.array(log_ps))) and len(np.unique(np.concatenate(sampled)[:, 0])) > 64
    np.testing.assert_array_equal(np.array(sampled), np.array(h_sampled))
    np.testing.assert_array_equal(np.array(log_ps), np.array(h_log_ps))
    assert bands.tobytes() == h_bands.tobytes() and np.all(np.isfinite(bands))
