"""MassActionODELogLike on the MI355X over the grammar networks of tests/ode_grammar.py (whose host builds tests/test_ode_grammar_cpu.py
holds against independent references): the device likelihood is the host build's, bit for bit, for the one-lane build (also in its long
form and at its limit of 64 reactions), for groups of 16 and 32 lanes and for the 64-lane wave per point, on a network whose pivot
candidates tie, on networks whose large steps pivot off the diagonal, for a single point, and where failed and finished points share a
wave or, with a wave per point, a block.

What the bit comparison resolves on the tied and the large-step inputs: with a permutation fault seeded in the host builds (the
forward solve reading b[k] for b[piv[k]]; tests/test_ode_grammar_cpu.py's head) the host value's bits change at 2002 of 2051, 1004 of
1027, 1004 of 1027 and 250 of 259 tied points (1, 16, 32, 64 lanes) and at 1027 of 1027, 515 of 515, 512 of 515 and 131 of 131
large-step points, so a device whose permutation bookkeeping differed from the host's anywhere would not pass them."""
import numpy as np
import pytest

from . import ode_grammar as G
from . import ode_networks as NW
from . import ode_wide_networks as W
from .ode_support import device_logp

pytestmark = pytest.mark.gpu

SUBSET = [0, 3, 5, 7, 24, 2, 8, 11, 14, 26, 16, 18, 23,      # one lane: S = 1, 4, 6, 8, 8, 3; 16 lanes: S = 1, 9, 16, 16; 32 lanes: S = 1, 17, 32
          29, 33, 35]                                        # 64 lanes: S = 33, 63, 64 (the last with fewer reactions than species)
N_POINTS = {1: 2051, 16: 1027, 32: 1027, 64: 259}            # (a block holds 256, 16, 8, 4 points: the last block is not full)
N_POINTS_WIDE = 131                                          # S >= 60: 259 points took 7 .. 8 s, most of it the host build; 32 blocks and one with an idle wave
STARVED = (14, 35)                                           # S16R40@16 with max_steps 35: the host build fails 0.4 of the box
STARVED_WAVE = (31, 25)                                      # S48R90@64 with max_steps 25: the host build fails 0.57 of the box
LARGE_STEP = {1: (0, 1027), 16: (2, 515), 32: (4, 515), 64: (6, N_POINTS_WIDE)}      # build: (index into G.LARGE_STEP_CASES, points)


def _same_bits(like, X):
    lower = X.min(axis=0) - 1.0
    pr, lk = device_logp(like, X, lower, float(np.max(X.max(axis=0) - lower)) + 1.0)
    host = like.batch(X)
    assert np.all(np.isfinite(pr))
    assert lk.tobytes() == host.tobytes(), (np.flatnonzero(lk != host)[:8], len(X))
    one = device_logp(like, X[:1], lower, float(np.max(X.max(axis=0) - lower)) + 1.0)[1]
    assert one.shape == (1,) and one.tobytes() == host[:1].tobytes()
    return host


@pytest.mark.parametrize("i", SUBSET, ids=[G.network(i).name for i in SUBSET])
def test_device_equals_host_build_on_the_grammar_networks(i):
    net = G.network(i)
    rng = np.random.default_rng(i)
    obs = rng.normal(size=(3, net.S))                                         # weights of either sign; one datum not observed
    data = rng.normal(size=(3, len(G.T_OUT)))
    data[1, 2] = np.nan
    host = _same_bits(net.like(observables=obs, data=data, sd=0.5), net.points(N_POINTS[net.lanes] if net.S < 60 else N_POINTS_WIDE))
    print("%s: %d of %d points -inf" % (net.name, np.sum(host == -np.inf), len(host)))
    assert np.all(np.isfinite(host))


@pytest.mark.parametrize("lanes", [1, 16, 32, 64])
def test_device_equals_host_build_where_pivot_candidates_tie(lanes):
    """Output times of 5, 50 and 500: the step grows until 4/h is below k1 B, where the rows of C and D tie for column A's pivot
    (tests/ode_grammar.py); a side that broke the tie the other way would round differently.  With 64 lanes the four species are
    rows 32..35 behind an inert chain: the tie is broken among the wave's high lanes."""
    X = G.TIED_X * 10.0 ** np.random.default_rng(6).uniform(-0.3, 0.3, (N_POINTS[lanes], 2))
    host, steps = G.tied(lanes).batch(X, return_steps=True)
    _same_bits(G.tied(lanes), X)
    print("tied @%d: median %d steps to t = 500" % (lanes, np.median(steps)))
    assert np.all(np.isfinite(host)) and np.median(steps) < 200               # (few steps over a long time: large ones)


@pytest.mark.parametrize("lanes", [1, 16, 32, 64])
def test_device_equals_host_build_where_large_steps_pivot_off_the_diagonal(lanes):
    """A network of the large-step family (tests/ode_grammar.py: sources, degradations, conversions, catalysts) out to t = 500 at
    rtol = atol = 1e-5: the steps average more than 4 time units (fewer than 125 of them, asserted; about 40 .. 70 on the host build),
    the sizes at which the CPU file shows from the reference's matrices that many columns pivot off the diagonal.  The device's
    permutation bookkeeping has to be the host build's, whose fixed steps are held to the mp restatement on the same network."""
    j, n = LARGE_STEP[lanes]
    net = G.large_step_network(j)
    like = net.like(t=G.TIED_T, rtol=1e-5, atol=1e-5)
    X = net.points(n)
    host, steps = like.batch(X, return_steps=True)
    _same_bits(like, X)
    print("%s: median %d steps to t = 500" % (net.name, np.median(steps)))
    assert np.all(np.isfinite(host)) and np.max(steps) < 125                  # (a mean step above 4 at every point)


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


def test_failed_and_finished_points_share_a_block_on_a_64_lane_grammar_network():
    """A wave holds one point, a block four: the mix is within a block of four waves"""
    i, max_steps = STARVED_WAVE
    net = G.network(i)
    host = _same_bits(net.like(max_steps=max_steps), net.points(N_POINTS[64]))
    failed = host == -np.inf
    blocks = failed[:len(failed) // 4 * 4].reshape(-1, 4)
    print("%s at max_steps %d: %.3f of the points -inf" % (net.name, max_steps, failed.mean()))
    assert 0.2 < failed.mean() < 0.8 and np.any(blocks.any(axis=1) & ~blocks.all(axis=1))
