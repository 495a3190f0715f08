"""MassActionODELogLike on the MI355X over the grammar networks of tests/ode_grammar.py (whose host builds tests/test_ode_grammar_cpu.py
holds against independent references): the device likelihood is the host build's, bit for bit, for the one-lane build (also in its long
form and at its limit of 64 reactions) and for groups of 16 and 32 lanes, on a network whose pivot candidates tie, for a single point,
and where failed and finished points share a wave."""
import numpy as np
import pytest

from . import ode_grammar as G
from . import ode_networks as NW
from . import ode_wide_networks as W
from .test_ode_likelihood_gpu import _device_logp

pytestmark = pytest.mark.gpu

SUBSET = [0, 3, 5, 7, 24, 2, 8, 11, 14, 26, 16, 18, 23]      # one lane: S = 1, 4, 6, 8, 8, 3; 16 lanes: S = 1, 9, 16, 16; 32 lanes: S = 1, 17, 32
N_POINTS = {1: 2051, 16: 1027, 32: 1027}                     # (a block holds 256, 16, 8 points: the last block is not full)
STARVED = (14, 35)                                           # S16R40@16 with max_steps 35: the host build fails 0.4 of the box


def _same_bits(like, X):
    lower = X.min(axis=0) - 1.0
    pr, lk = _device_logp(like, X, lower, float(np.max(X.max(axis=0) - lower)) + 1.0)
    host = like.batch(X)
    assert np.all(np.isfinite(pr))
    assert lk.tobytes() == host.tobytes(), (np.flatnonzero(lk != host)[:8], len(X))
    one = _device_logp(like, X[:1], lower, float(np.max(X.max(axis=0) - lower)) + 1.0)[1]
    assert one.shape == (1,) and one.tobytes() == host[:1].tobytes()
    return host


@pytest.mark.parametrize("i", SUBSET, ids=[G.network(i).name for i in SUBSET])
def test_device_equals_host_build_on_the_grammar_networks(i):
    net = G.network(i)
    rng = np.random.default_rng(i)
    obs = rng.normal(size=(3, net.S))                                         # weights of either sign; one datum not observed
    data = rng.normal(size=(3, len(G.T_OUT)))
    data[1, 2] = np.nan
    host = _same_bits(net.like(observables=obs, data=data, sd=0.5), net.points(N_POINTS[net.lanes]))
    print("%s: %d of %d points -inf" % (net.name, np.sum(host == -np.inf), len(host)))
    assert np.all(np.isfinite(host))


@pytest.mark.parametrize("lanes", [1, 16, 32])
def test_device_equals_host_build_where_pivot_candidates_tie(lanes):
    """Output times of 5, 50 and 500: the step grows until 4/h is below k1 B, where the rows of C and D tie for column A's pivot
    (tests/ode_grammar.py); a side that broke the tie the other way would round differently."""
    X = G.TIED_X * 10.0 ** np.random.default_rng(6).uniform(-0.3, 0.3, (N_POINTS[lanes], 2))
    host, steps = G.tied(lanes).batch(X, return_steps=True)
    _same_bits(G.tied(lanes), X)
    print("tied @%d: median %d steps to t = 500" % (lanes, np.median(steps)))
    assert np.all(np.isfinite(host)) and np.median(steps) < 200               # (few steps over a long time: large ones)


@pytest.mark.parametrize("R", [32, 64])
def test_device_equals_host_build_on_dense_one_lane_networks_up_to_the_reaction_limit(R):
    like = W.dense_network(8, R, 1)
    host = _same_bits(like, NW.box_points(np.zeros(20), 2051, 4, width=1.0))
    print("dense S=8 R=%d @1: %d of %d points -inf" % (R, np.sum(host == -np.inf), len(host)))
    assert np.mean(np.isfinite(host)) > 0.9


def test_failed_and_finished_points_share_a_wave_on_a_grammar_network():
    i, max_steps = STARVED
    net = G.network(i)
    host = _same_bits(net.like(max_steps=max_steps), net.points(N_POINTS[net.lanes]))
    failed = host == -np.inf
    per_wave = 64 // net.lanes
    waves = failed[:len(failed) // per_wave * per_wave].reshape(-1, per_wave)
    print("%s at max_steps %d: %.3f of the points -inf" % (net.name, max_steps, failed.mean()))
    assert np.any(waves.any(axis=1) & ~waves.all(axis=1))
