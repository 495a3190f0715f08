"""The shipped knock-down example on the MI355X: the device gives the host build's bits on prior draws in both shapes it offers, and a
short run_dream equals the oracle driven by the host build."""
import os

import numpy as np
import pytest
from scipy.stats import uniform

from pydream_amd.examples.knockdown import knockdown_device as KD
from pydream_amd.parameters import SampledParam

from .ode_support import device_equals_host, run_dream_equals_oracle
from .test_ode_view_example_cpu import data

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("lanes", [1, 16])
def test_the_example_on_the_device_equals_the_host_build(lanes):
    """64 prior draws x 6 experiments"""
    like = KD.make_likelihood(data=data(), lanes_per_point=lanes)
    X = KD.LOWER + KD.WIDTH * np.random.default_rng(52).uniform(size=(64, KD.NDIM))
    from pydream_amd import _capi
    eng = _capi.Engine(nchains=3, ndim=KD.NDIM, history_capacity=8)
    eng.set_prior(np.full(KD.NDIM, 2, dtype=np.int32), KD.LOWER, KD.WIDTH)
    like._dz_apply(eng)
    pr, lk = eng.eval_logp(X)
    eng.close()
    host = like.batch(X)
    assert lk.tobytes() == host.tobytes() and np.all(np.isfinite(pr)) and np.isfinite(host).sum() > 32


def test_run_dream_with_the_example_on_the_device_equals_the_oracle(tmp_path):
    """8 chains, 40 generations, multitry 3, no hard boundaries"""
    os.chdir(tmp_path)
    N, G = 8, 40
    like = KD.make_likelihood(data=data())
    params = [SampledParam(uniform, loc=KD.LOWER, scale=KD.WIDTH)]
    rng = np.random.default_rng(83)
    np.save("knockdown_seed.npy", KD.LOWER + KD.WIDTH * rng.uniform(0, 1, (60, KD.NDIM)))
    box = KD.LOWER + KD.WIDTH * rng.uniform(0, 1, (200, KD.NDIM))
    starts = list(box[np.isfinite(like.batch(box))][:N])
    assert len(starts) == N
    kw = dict(multitry=3, history_thin=1, hardboundaries=False, history_file="knockdown_seed.npy")
    run_dream_equals_oracle(like, params, starts, 59, N, G, **kw)
