"""NORMALISED READOUTS, MassActionODELogLike(normalize=[...]), on the MI355X: the kernels with the running sums and the finish behind the
last row give the host build's bits -- values, normalised simulate rows and per-condition terms, no tolerance -- in the one-lane shape
(items of three conditions, through the likelihood kernel and the item prediction kernel), a lane group of 16 and of 32 and a wave per
point; the condition whose product is identically zero is -inf with a NaN slice exactly where the host build says; with every other
feature in the same object in all four builds.  The smallest shapes that hold a full block, a part-filled block and an idle tail."""
import numpy as np
import pytest

from . import ode_equilibrate_networks as EQ
from . import ode_networks as NW
from . import ode_normalize_networks as NN
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


@pytest.mark.parametrize("kind", NN.KINDS)
def test_one_lane_items_with_normalised_readouts_equal_the_host_build(kind):
    """MM x 3 conditions, 259 points = 777 items: three full blocks and nine lanes of a fourth.  The third condition has no enzyme, so
    its product is identically zero: every point's sum is -inf, that item's slice NaN and the other two items finite."""
    multi, _ = NN.mm_conditions(NN.mm_normalize(kind))
    assert multi.lanes_per_point == 1 and "NORMALIZE = 2" in multi.source() and len(multi.conditions) == 3
    X = NN.mm_points()
    host = device_equals_host(multi, X, NW.MM_NOMINAL)
    assert np.all(host == -INF)
    sim, terms = _predictions_equal_host(multi, X)
    assert np.all(np.isfinite(terms[:, :2])) and np.all(terms[:, 2] == -INF) and np.all(np.isfinite(sim[:, :2])) and np.all(np.isnan(sim[:, 2]))
    # (and the two conditions that integrate, alone: finite sums through the likelihood kernel)
    two, _ = NN.mm_conditions(NN.mm_normalize(kind), y0s=NN.MM_CONDITION_Y0[:2])
    assert np.all(np.isfinite(device_equals_host(two, X, NW.MM_NOMINAL)))


def test_one_lane_single_experiment_with_noise_and_the_steady_row():
    """Noise(sigma) on both normalised readouts, the product's reference at the steady row: 259 points, a block and three lanes"""
    like = NN.mm(NN.mm_normalize("ref", steady=True), steady=True, noisy=True)
    X = NN.with_sigma(NN.mm_points())
    nominal = np.r_[NW.MM_NOMINAL, NN.MM_LOG_SIGMA]
    host = device_equals_host(like, X, nominal)
    assert np.all(np.isfinite(host))
    sim, _ = _predictions_equal_host(like, X)
    assert np.all(sim[:, -1, 1] == 1.0)


@pytest.mark.parametrize("name,lanes,n", [("enzyme13", 16, 131), ("chain17", 32, 131), (EQ.smallest_wave_chain(), 64, 259)])
def test_a_group_and_a_wave_with_normalised_readouts_equal_the_host_twin(name, lanes, n):
    """enzyme13 at 16 lanes: 131 points, 16 to a block; chain17 at 32 lanes: 131 points, 8 to a block; the smallest wave chain at 64
    lanes: 259 points, four waves to a block, the last block with three.  The observables cycle through the three kinds and None,
    every second normalised one with a Noise."""
    like, nominal = NN.group(name)
    assert like.lanes_per_point == lanes and like.conditions is None and "NORMALIZE" in like.source() and "NOISE" in like.source()
    X = NW.box_points(nominal, n, 22, width=1.0, outside=0.05)
    host = device_equals_host(like, X, nominal)
    assert np.isfinite(host).sum() > n // 2
    _predictions_equal_host(like, X[:2 * 256 // lanes + 3])


@pytest.mark.parametrize("lanes", [1, 16, 32, 64])
def test_every_feature_together_with_normalised_readouts_equals_the_host_build(lanes):
    """ode_settle_networks' combined network -- conditions, Monomials, events, equilibrate, rate laws, noise, inputs, a view, the steady
    row -- with three normalised observables: 67 points x its three conditions"""
    case, like = NN.combined(lanes)
    assert "NORMALIZE = 3" in like.source() and "VIEW" in like.source() and "SETTLE" in like.source() and "INPUTS" in like.source()
    X = case.points(67, 5, outside=0.05)
    from pydream_amd import _capi
    eng = _capi.Engine(nchains=3, ndim=X.shape[1], history_capacity=8)
    like._dz_apply(eng)
    lk = eng.eval_logp(X)[1]
    eng.close()
    host = like.batch(X)
    assert lk.tobytes() == host.tobytes() and np.isfinite(host).sum() > 33
    _predictions_equal_host(like, X[:5 if lanes == 64 else 19])
