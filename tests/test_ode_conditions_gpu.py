"""MassActionODELogLike(conditions=[...]) on the MI355X: a launch over points x conditions items plus the engine's sum gives the host
build's bits (one lane and a lane group per item, also where some conditions of a point fail), the engine adds the items of any user
kernel from left to right, and run_dream with a multi-condition likelihood equals the oracle driven by the host build."""
import os

import numpy as np
import pytest
from scipy.stats import uniform

from pydream_amd import _capi
from pydream_amd.likelihoods import DeviceKernelLogLike
from pydream_amd.parameters import SampledParam

from . import ode_condition_networks as CN
from . import ode_networks as NW
from . import ode_wide_networks as W
from .ode_support import device_equals_host, run_dream_equals_oracle

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("doses,max_steps", [(CN.MM_DOSES, 500), (CN.MM_DOSES_5, 500), (CN.MM_DOSES, 60)])
def test_device_equals_host_build_one_lane_per_item(doses, max_steps):
    """1027 points x 3 conditions = 3081 items (12 blocks and 9 items of a 13th), x 5 = 5135; with max_steps 60 there are points that
    fail in every condition, in some, in none."""
    multi, _ = CN.mm(doses, max_steps=max_steps)
    X = NW.box_points(NW.MM_NOMINAL, 1027, 21, width=1.0, outside=0.05)
    host = device_equals_host(multi, X, NW.MM_NOMINAL)
    failed = multi.batch_conditions(X) == -np.inf
    count = failed.sum(axis=1)
    print("MM x %d at max_steps %d: points failing in all / some / no conditions: %d / %d / %d"
          % (len(doses), max_steps, np.sum(count == len(doses)), np.sum((count > 0) & (count < len(doses))), np.sum(count == 0)))
    if max_steps == 60:
        assert np.any(count == 3) and np.any((count > 0) & (count < 3)) and np.any(count == 0)
    else:
        assert np.all(np.isfinite(host))


@pytest.mark.parametrize("name", ["enzyme13@16 x 3", "chain17@32 x 2"])
def test_device_equals_host_twin_a_lane_group_per_item(name):
    """enzyme13: 259 points x 3 = 777 items, 16 to a block: the last block has groups without an item; chain17: 131 x 2 = 262, 8 to a block."""
    if name.startswith("enzyme"):
        (multi, _), nom, n = CN.enzyme13(), W.ENZ.NOMINAL, 259
    else:
        (multi, _), nom, n = CN.chain(17, 32, (1.0, 2.0)), W.CHAIN_NOMINAL, 131
    X = NW.box_points(nom, n, 21, width=1.0)
    host = device_equals_host(multi, X, nom)
    assert np.all(np.isfinite(host))


ITEM_KERNEL = r'''
extern "C" __global__ void item_terms(const double* X, long long n, int d, int ld, double* like, const void* data)
{
    const long long w = blockIdx.x * 256ll + threadIdx.x;
    if (w >= n) return;
    const double* c = (const double*)data;              // [0..3): a weight per item, [3]: the items the launch must have, [4]: C
    const long long C = (long long)c[4], i = w / C, t = w - i * C;
    const double* x = X + i * ld;
    double v = x[0] * c[t] + x[1];
    if (x[2] > 1.0 && t == 1) v = -__builtin_huge_val();
    if (n != (long long)c[3]) v = __builtin_nan("");
    like[w] = v;
}'''


def test_the_engine_adds_the_items_of_a_user_kernel_from_left_to_right():
    n, d, C = 37, 3, 3
    X = np.random.default_rng(0).normal(size=(n, d))
    weight = np.array([1.0, 3.0, -7.0])
    terms = X[:, :1] * weight[None, :] + X[:, 1:2]                      # (contraction is off in the kernel: numpy's rounding)
    terms[X[:, 2] > 1.0, 1] = -np.inf
    want = (terms[:, 0] + terms[:, 1]) + terms[:, 2]
    assert 0 < np.sum(want == -np.inf) < n and np.any(want != terms[:, 0] + (terms[:, 1] + terms[:, 2]))
    like = DeviceKernelLogLike("item_terms", d, source=ITEM_KERNEL, data=np.r_[weight, n * C, C], items_per_point=C)
    e = _capi.Engine(nchains=3, ndim=d, history_capacity=8)
    like._dz_apply(e)
    got = e.eval_logp(X)[1]
    assert got.tobytes() == want.tobytes()
    for bad in (0, -1, 65):
        with pytest.raises(_capi.DreamZSError, match=r"items_per_point must be 1\.\.64"):
            e.set_likelihood_module(like.code_object(), "item_terms", 1, like.data, items_per_point=bad)
    # a set_likelihood_module call without the keyword is back at one item per point: n items = n points, every point its term 0
    e.set_likelihood_module(like.code_object(), "item_terms", 1, np.r_[weight, n, 1.0])
    assert e.eval_logp(X)[1].tobytes() == terms[:, 0].tobytes()
    e.set_likelihood_module(like.code_object(), "item_terms", 1, np.r_[weight, n * 2, 2.0], items_per_point=2)
    assert e.eval_logp(X)[1].tobytes() == (terms[:, 0] + terms[:, 1]).tobytes()


def test_a_user_kernel_with_items_called_on_the_host_side():
    """DeviceKernelLogLike.__call__ without a host twin evaluates one point on the device: 1 point x 3 items."""
    d, C = 3, 3
    weight = np.array([1.0, 2.0, 3.0])
    like = DeviceKernelLogLike("item_terms", d, source=ITEM_KERNEL, data=np.r_[weight, C, C], items_per_point=C)
    x = np.array([0.25, -0.5, 0.0])
    assert like(x) == ((x[0] * 1.0 + x[1]) + (x[0] * 2.0 + x[1])) + (x[0] * 3.0 + x[1])


@pytest.mark.parametrize("multitry,hard,max_steps", [(False, True, 500), (3, False, 60)])
def test_run_dream_on_the_device_equals_the_oracle(tmp_path, multitry, hard, max_steps):
    """MM under three doses against run_dream's own sequence on the oracle with the host build as the Python likelihood; with max_steps 60
    most of the prior box fails in at least one condition, so whole proposal sets are impossible and drawn again."""
    os.chdir(tmp_path)
    N, G = 8, 40
    multi, _ = CN.mm(max_steps=max_steps)
    nom = NW.MM_NOMINAL
    params = [SampledParam(uniform, loc=nom - 1.0, scale=2)]
    rng = np.random.default_rng(78)
    Z0 = nom - 1.0 + 2 * rng.uniform(0, 1, (60, len(nom)))
    np.save("mm_seed.npy", Z0)
    if max_steps < 500:
        assert np.mean(multi.batch(Z0) == -np.inf) > 0.2
    box = nom - 1.0 + 2 * rng.uniform(0, 1, (200, len(nom)))          # (at 60 steps the nominal point itself fails: start where no condition does)
    starts = list(box[np.isfinite(multi.batch(box))][:N])
    assert len(starts) == N
    kw = dict(multitry=multitry, gamma_levels=4, adapt_gamma=True, history_thin=1, hardboundaries=hard, history_file="mm_seed.npy")
    run_dream_equals_oracle(multi, params, starts, 56, N, G, **kw)
