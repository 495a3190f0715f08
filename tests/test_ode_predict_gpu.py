"""MassActionODELogLike.device() on the MI355X: simulate, batch_conditions and batch of the device evaluator give the bytes of the host
methods of the same names -- in every entry shape (a lane or a lane group per point or per item; 16, 32 and 64 lanes), with every
feature on the prediction path, where items fail (NaN slices, the neighbours untouched), across buffer reuse and chunk boundaries, and
end to end through posterior_predictive; and dz_set_output_module / dz_eval_outputs launch any user kernel with their signature.
Every comparison is on bytes (same())."""
import os

import numpy as np
import pytest
from scipy.stats import uniform

from pydream_amd import _capi
from pydream_amd.core import run_dream
from pydream_amd.likelihoods import compile_device_kernel, posterior_predictive
from pydream_amd.parameters import SampledParam

from . import ode_condition_networks as CN
from . import ode_networks as NW
from . import ode_noise_networks as NZ
from . import ode_pinned_corpus as PC
from . import ode_ratelaw_networks as RN
from . import ode_wave_networks as WN
from . import ode_wide_networks as W

pytestmark = pytest.mark.gpu

C5_SCALES = (1.0, 0.5, 2.0, 0.25, 4.0)


def same(dev, host):
    assert dev.shape == host.shape and dev.dtype == host.dtype
    assert np.array_equal(dev, host, equal_nan=True)
    fin = np.isfinite(host)
    assert dev[fin].tobytes() == host[fin].tobytes()


def device_equals_host(like, X, **kw):
    """simulate (and the terms beside it), batch_conditions where there are conditions, and batch of the device evaluator against the
    host methods; returns the host's (sim, terms)."""
    sim, total = like.simulate(X), like.batch(X)
    terms = like.batch_conditions(X) if like.conditions is not None else None
    with like.device(**kw) as ev:
        dsim, dterms = ev.simulate(X, return_terms=True)
        same(dsim, sim)
        if terms is not None:
            same(ev.batch_conditions(X), terms)
            same(dterms, terms)
            same(CN.left_to_right(dterms), total)
        else:
            same(dterms, total)
        same(ev.batch(X), total)
    return sim, (terms if terms is not None else total)


SHAPES = {
    "robertson@1 n=1": (NW.robertson, NW.ROB.NOMINAL, 3.0, 1),
    "robertson@1 n=257": (NW.robertson, NW.ROB.NOMINAL, 3.0, 257),                       # a second block, a ragged tail
    "chain8@1 x 5 n=52": (lambda: CN.chain(8, 1, C5_SCALES)[0], NW.CHAIN_NOMINAL, 1.0, 52),      # 260 items
    "enzyme13@16 n=1": (W.enzyme13, W.ENZ.NOMINAL, 1.0, 1),
    "enzyme13@16 n=17": (W.enzyme13, W.ENZ.NOMINAL, 1.0, 17),                            # one group in the second block, 15 padding groups
    "enzyme13@16 x 3 n=6": (lambda: CN.enzyme13()[0], W.ENZ.NOMINAL, 1.0, 6),           # 18 items
    "chain32@32 n=9": (lambda: W.chain(32, 32), W.CHAIN_NOMINAL, 1.0, 9),
    "cascade49@64 n=5": (WN.cascade, WN.CAS.NOMINAL, WN.CASCADE_WIDTH, 5),              # four items per block, three padding waves
}


@pytest.mark.parametrize("name", list(SHAPES))
def test_every_entry_shape_gives_the_host_methods_bytes(name):
    make, nominal, width, n = SHAPES[name]
    like = make()
    sim, terms = device_equals_host(like, NW.box_points(nominal, n, 31, width=width))
    print("%s: %d of %d items -inf" % (name, np.sum(terms == -np.inf), terms.size))
    assert np.any(np.isfinite(sim))


@pytest.mark.parametrize("shape", ["one-lane-short", "16-lanes"])
def test_every_feature_at_once_on_the_prediction_path(shape):
    """conditions, a Monomial rate, scale and constraint, events, equilibration and a Hill factor together (ode_pinned_corpus.everything_on)"""
    net = RN.network(PC.SHAPES[shape])
    like = PC.everything_on(net)
    sim, terms = device_equals_host(like, NW.box_points(net.nominal(), 7, 8, width=0.5))
    assert np.any(np.isfinite(sim)) and np.any(np.isfinite(terms))


def test_sampled_noise_on_the_log_scale_on_the_prediction_path():
    net = NZ.network("one3")
    noise = NZ.cases(net.P)["all_three"]
    like = NZ.like(net, noise)
    X = NW.box_points(NZ.nominal(net), 7, 5, width=NZ.WIDTH)
    X[1, net.P] = np.nan                            # sigma not finite: the point is not live
    X[4, net.P + 1] = np.inf
    sim, terms = device_equals_host(like, X)
    failed = terms == -np.inf
    assert failed[1] and failed[4] and not failed.all()
    assert np.all(np.isnan(sim[failed])) and np.all(np.isfinite(sim[~failed]))


FAILED = {
    "robertson@1": (NW.robertson, NW.ROB.NOMINAL, 0.5),
    "enzyme13@16": (W.enzyme13, W.ENZ.NOMINAL, 0.25),
    "cascade49@64": (WN.cascade, WN.CAS.NOMINAL, 0.1),
}


@pytest.mark.parametrize("name", list(FAILED))
def test_a_row_with_a_nan_coordinate_leaves_nan_and_its_neighbours_stand(name):
    make, nominal, width = FAILED[name]
    like = make()
    X = NW.box_points(nominal, 5, 2, width=width)
    X[2, 0] = np.nan
    sim, terms = device_equals_host(like, X)
    assert terms[2] == -np.inf and np.all(np.isnan(sim[2]))
    assert np.all(np.isfinite(terms[[0, 1, 3, 4]])) and np.all(np.isfinite(sim[[0, 1, 3, 4]]))
    with like.device() as ev:                      # ... also after a call that filled the buffer with finite numbers: nothing relies on its content
        ev.simulate(X[[0, 1, 3, 4, 0]])
        same(ev.simulate(X), sim)


def test_integrations_that_run_out_of_steps_leave_nan():
    """enzyme13@16 with max_steps 75 on nine points of the prior box: the host build finds rows that fail in the middle of the run (the
    entries written before the failure are overwritten) and rows that finish."""
    like = W.enzyme13(max_steps=75)
    X = NW.box_points(W.ENZ.NOMINAL, 9, 2, width=1.0)
    failed = like.batch(X) == -np.inf
    assert failed.any() and not failed.all()
    sim, _ = device_equals_host(like, X)
    assert np.all(np.isnan(sim[failed])) and np.all(np.isfinite(sim[~failed]))


def test_a_failed_condition_between_two_that_finish():
    like = CN.chain(8, 1, C5_SCALES, max_steps=30)[0]
    X = NW.box_points(NW.CHAIN_NOMINAL, 9, 3, width=1.0)
    failed = like.batch_conditions(X) == -np.inf
    between = failed[:, 1:-1] & ~failed[:, :-2] & ~failed[:, 2:]
    assert between.any()
    sim, _ = device_equals_host(like, X)
    assert np.all(np.isnan(sim[failed])) and np.all(np.isfinite(sim[~failed]))


def test_one_evaluator_over_a_large_a_small_and_a_large_batch():
    like = CN.chain(8, 1, C5_SCALES)[0]
    X = NW.box_points(NW.CHAIN_NOMINAL, 40, 9, width=1.0)
    with like.device() as ev:
        got = [ev.simulate(x, return_terms=True) for x in (X, X[37:], X)] + [ev.batch(x) for x in (X, X[37:], X)]
    fresh = []
    for x in (X, X[37:], X):
        with like.device() as ev:
            fresh.append(ev.simulate(x, return_terms=True))
    for (s, t), (fs, ft), x in zip(got[:3], fresh, (X, X[37:], X)):
        same(s, fs); same(t, ft)
        same(s, like.simulate(x)); same(t, like.batch_conditions(x))
    for b, x in zip(got[3:], (X, X[37:], X)):
        same(b, like.batch(x))


def test_chunks_are_whole_points():
    """A chunk never ends in the middle of a point's conditions, by construction: points per chunk = max(1, chunk_items // C).  30 items of
    the C = 5 network with chunk_items=7 are six launches of one point, with chunk_items=12 three of two, with 4 still one point each."""
    like = CN.chain(8, 1, C5_SCALES)[0]
    X = NW.box_points(NW.CHAIN_NOMINAL, 6, 12, width=1.0)
    with like.device() as ev:
        whole = ev.simulate(X, return_terms=True)
        assert ev.points_per_chunk() >= 6
    same(whole[0], like.simulate(X))
    for chunk_items, points in ((7, 1), (12, 2), (4, 1)):
        with like.device(chunk_items=chunk_items) as ev:
            assert ev.points_per_chunk() == points
            s, t = ev.simulate(X, return_terms=True)
            same(s, whole[0]); same(t, whole[1])
            same(ev.batch(X), like.batch(X))
    with like.device(max_bytes=8 * 5 * 11 * 8 * 2 + 8) as ev:      # (room for two points' C * T * O doubles and a bit)
        assert ev.points_per_chunk() == 2
        same(ev.simulate(X), whole[0])


def test_posterior_predictive_end_to_end(tmp_path):
    os.chdir(tmp_path)
    like = NW.robertson()
    rng = np.random.default_rng(3)
    np.save("seed.npy", NW.box_points(NW.ROB.NOMINAL, 60, 6))
    starts = [NW.ROB.NOMINAL + 0.3 * rng.uniform(-1, 1, 3) for _ in range(8)]
    sampled, _ = run_dream([SampledParam(uniform, loc=NW.ROB_LOWER, scale=6)], like, nchains=8, niterations=40, verbose=False, start=starts,
                           save_history=False, seed=17, history_file="seed.npy")
    rows, sim = posterior_predictive(sampled, like, burnin=20, thin=5)
    hrows, hsim = posterior_predictive(sampled, like, burnin=20, thin=5, device=False)
    assert rows.shape == (8 * 4, 3) and rows.tobytes() == hrows.tobytes()
    same(sim, hsim)
    assert np.all(np.isfinite(hsim))
    t = np.linspace(0.0, float(like.t[-1]), 25)
    rows_t, sim_t = posterior_predictive(sampled, like, burnin=20, thin=5, t=t)
    same(sim_t, posterior_predictive(sampled, like, burnin=20, thin=5, device=False, t=t)[1])
    assert sim_t.shape == (32, 25, len(like.observables)) and rows_t.tobytes() == rows.tobytes()


USER_KERNEL = r'''
extern "C" __global__ __launch_bounds__(256)
void ramp(const double* X, long long n, int d, int ld, double* like, const void* data, double* out, long long out_ld)
{
    const long long w = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= n) return;
    for (int m = 0; m < 5; ++m) out[w * out_ld + m] = X[w * ld] * m;
    like[w] = (double)w;
}'''


def test_the_output_module_launches_any_kernel_with_its_signature():
    path = compile_device_kernel(USER_KERNEL)
    d, n = 3, 300
    X = np.random.default_rng(1).normal(size=(n, d))
    e = _capi.Engine(nchains=3, ndim=d, history_capacity=8)
    try:
        with pytest.raises(_capi.DreamZSError, match="dz_set_output_module first"):
            e.eval_outputs(X)
        e.set_output_module(path, "ramp", 1, 1, 5)
        terms, out = e.eval_outputs(X)
        np.testing.assert_array_equal(terms, np.arange(n, dtype=float)[:, None])
        np.testing.assert_array_equal(out[:, 0], X[:, :1] * np.arange(5.0))
        terms3, out3 = e.eval_outputs(X[:3])                       # (a smaller call after a larger one)
        np.testing.assert_array_equal(out3, out[:3]); np.testing.assert_array_equal(terms3, terms[:3])
        with pytest.raises(_capi.DreamZSError, match="hipModuleGetFunction\\(no_such_kernel\\)"):
            e.set_output_module(path, "no_such_kernel", 1, 1, 5)
        with pytest.raises(_capi.DreamZSError, match="lanes_per_point must be 1"):
            e.set_output_module(path, "ramp", 8, 1, 5)
        with pytest.raises(_capi.DreamZSError, match="doubles_per_item must be >= 1"):
            e.set_output_module(path, "ramp", 1, 1, 0)
        with pytest.raises(_capi.DreamZSError, match="items_per_point must be 1..64"):
            e.set_output_module(path, "ramp", 1, 65, 5)
        np.testing.assert_array_equal(e.eval_outputs(X)[1], out)    # the refused calls left the module as it was
    finally:
        e.close()
