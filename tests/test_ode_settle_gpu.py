"""A steady output, MassActionODELogLike(t=[..., inf], settle=...), on the MI355X: the kernels with the phase at the experiment's end
give the host build's bits -- values, simulate rows and per-condition terms, no tolerance -- in the one-lane shape (items of three
conditions, through the likelihood kernel and the item prediction kernel), a lane group of 16 and of 32 and a wave per point; also where
a starved phase fails some points of a wave and a block and not others; with every other feature in the same object in all four builds;
run_dream on the shipped example equals its host-likelihood run; posterior_predictive with and without the device.  The smallest shapes
that hold a full block, a part-filled block and an idle tail."""
import os

import numpy as np
import pytest

from pydream_amd.likelihoods import posterior_predictive

from . import ode_networks as NW
from . import ode_settle_networks as SN
from .ode_support import device_equals_host

pytestmark = pytest.mark.gpu
INF = np.inf


def _predictions_equal_host(like, X):
    """simulate and the terms through the prediction kernel: the host build's bytes, NaN positions included"""
    with like.device() as ev:
        sim, terms = ev.simulate(X, return_terms=True)
        assert ev.batch(X).tobytes() == like.batch(X).tobytes()
    assert sim.tobytes() == like.simulate(X).tobytes()
    host_terms = like.batch_conditions(X) if like.conditions is not None else like.batch(X)
    assert terms.tobytes() == host_terms.tobytes()
    return sim, terms


def test_one_lane_items_with_the_steady_row_equal_the_host_build():
    """MM x 3 conditions (plain, a double dose, events AT t_last), 259 points = 777 items: three full blocks and nine lanes of a fourth;
    through dz_eval_logp and through the item prediction kernel"""
    multi, _ = SN.mm_conditions()
    assert multi.lanes_per_point == 1 and "SETTLE = true" in multi.source() and len(multi.conditions) == 3
    X = NW.box_points(NW.MM_NOMINAL, 259, 21, width=1.0, outside=0.05)
    host = device_equals_host(multi, X, NW.MM_NOMINAL)
    assert np.all(np.isfinite(host))
    sim, _ = _predictions_equal_host(multi, X)
    assert np.all(np.isfinite(sim)) and sim.shape == (259, 3, len(multi.t), 4)


@pytest.mark.parametrize("name,lanes,n", [("enzyme13", 16, 131), ("chain17", 32, 131), (SN.WAVE, 64, 259)])
def test_a_group_and_a_wave_with_the_steady_row_equal_the_host_twin(name, lanes, n):
    """enzyme13 at 16 lanes: 131 points, 16 to a block; chain17 at 32 lanes: 131 points, 8 to a block; chain33 at 64 lanes: 259 points,
    four waves to a block, the last block with three"""
    like = SN.single(name)
    nominal = SN.network(name)[5]
    assert like.lanes_per_point == lanes and like.conditions is None and "SETTLE = true" in like.source()
    X = NW.box_points(nominal, n, 22, width=1.0, outside=0.05)
    host = device_equals_host(like, X, nominal)
    assert np.all(np.isfinite(host))
    _predictions_equal_host(like, X[:2 * 256 // lanes + 3])


@pytest.mark.parametrize("name,lanes", [("mm", 1), (SN.WAVE, 64)])
def test_a_starved_phase_on_the_device_fails_the_points_the_host_build_fails(name, lanes):
    """test_ode_settle_cpu's starved case: failing and finishing points share waves and blocks; the -inf / NaN positions and all finite
    bits are the host build's"""
    like = SN.starved(name)
    nominal = SN.network(name)[5]
    X = SN.starved_points(name)
    assert like.lanes_per_point == lanes and len(X) == 259
    host = device_equals_host(like, X, nominal)
    failed = host == -INF
    print("%s starved at %d attempts on the device: %d of %d points fail" % (name, SN.STARVED_SETTLE_STEPS[name], failed.sum(), len(X)))
    assert failed.sum() >= 65 and (~failed).sum() >= 65
    sim, terms = _predictions_equal_host(like, X)
    assert np.all(np.isnan(sim[failed])) and np.all(np.isfinite(sim[~failed])) and np.array_equal(terms == -INF, failed)


@pytest.mark.parametrize("lanes", [1, 16, 32, 64])
def test_every_feature_together_with_the_steady_row_equals_the_host_build(lanes):
    """test_ode_settle_cpu's combined network: 67 points x its three conditions"""
    case = SN.steady_case(lanes)
    like = case.steady_like()
    X = case.points(67, 5, outside=0.05)
    from pydream_amd import _capi
    eng = _capi.Engine(nchains=3, ndim=X.shape[1], history_capacity=8)
    like._dz_apply(eng)
    lk = eng.eval_logp(X)[1]
    eng.close()
    host = like.batch(X)
    assert lk.tobytes() == host.tobytes() and np.isfinite(host).sum() > 33
    _predictions_equal_host(like, X[:5 if lanes == 64 else 19])


def test_run_dream_on_the_example_equals_its_host_likelihood_run(tmp_path, capsys):
    """64 chains, 60 iterations, multitry 5, a fixed seed: main() on the device gives, sample for sample, what main(host=True) gives"""
    from pydream_amd.examples.steady_dose import steady_dose_device as SD
    os.chdir(tmp_path)
    like = SD.make_likelihood()
    sampled, log_ps, bands = SD.main(60, 64, like=like)
    assert "on the device" in capsys.readouterr().out
    h_sampled, h_log_ps, h_bands = SD.main(60, 64, host=True, like=like)
    assert np.all(np.isfinite(np.array(log_ps))) and len(np.unique(np.concatenate(sampled)[:, 0])) > 64
    np.testing.assert_array_equal(np.array(sampled), np.array(h_sampled))
    np.testing.assert_array_equal(np.array(log_ps), np.array(h_log_ps))
    assert bands.tobytes() == h_bands.tobytes()


def test_posterior_predictive_with_the_steady_row_on_sixteen_rows():
    from pydream_amd.examples.steady_dose import steady_dose_device as SD
    like = SD.make_likelihood()
    rng = np.random.default_rng(7)
    chains = [SD.NOMINAL + 0.3 * rng.uniform(-1, 1, (8, 3)) for _ in range(2)]
    rows, sim = posterior_predictive(chains, like, device=True)
    h_rows, h_sim = posterior_predictive(chains, like, device=False)
    assert len(rows) == 16 and rows.tobytes() == h_rows.tobytes() and sim.tobytes() == h_sim.tobytes() and np.all(np.isfinite(sim))
    assert sim.shape == (16, len(SD.DOSES), len(SD.TSPAN), 1)
    t = np.r_[np.linspace(0.0, 2.0, 9), INF]
    dense, h_dense = posterior_predictive(chains, like, device=True, t=t)[1], posterior_predictive(chains, like, device=False, t=t)[1]
    assert dense.tobytes() == h_dense.tobytes() and dense.shape == (16, len(SD.DOSES), len(t), 1) and np.all(np.isfinite(dense))
