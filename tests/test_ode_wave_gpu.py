"""MassActionODELogLike(lanes_per_point=64) on the MI355X: the wave-per-point solver gives its host twin's bits -- in blocks with idle
waves, where failed and finished points share a block, at the reaction limit, and through the item kernel with events, a Monomial scale
and a constraint --, and run_dream with the 49-species cascade equals the oracle driven by the host twin."""
import functools
import os

import numpy as np
import pytest
from scipy.stats import uniform

from pydream_amd.parameters import SampledParam

from . import ode_networks as NW
from . import ode_wave_networks as WN
from . import ode_wide_networks as W
from .ode_support import device_logp, run_dream_equals_oracle

pytestmark = pytest.mark.gpu

N_POINTS = 259            # 4 * 64 + 3: the last block has one wave without a point


@functools.lru_cache(maxsize=None)
def _host(name, starved):
    """(the object, the points, the host twin's values): once per case, shared by the point counts, not to be written to"""
    make, nom, width, _ = WN.CASES[name]
    like = make(max_steps=WN.STARVED_MAX_STEPS) if starved else make()
    X = NW.box_points(nom, N_POINTS, 21, width=width, outside=0.05 / len(nom))      # a few points outside the prior's support
    host = like.batch(X)
    X.setflags(write=False); host.setflags(write=False)
    return like, X, host


@pytest.mark.parametrize("n", [1, 5, N_POINTS])
@pytest.mark.parametrize("starved", [False, True])
@pytest.mark.parametrize("name", ["chain33", "chain64", "cascade49"])
def test_device_equals_host_twin_bit_for_bit(name, starved, n):
    """n = 1 and n = 5: a block with three idle waves; 259: 64 full blocks and one with an idle wave"""
    like, X, host = _host(name, starved)
    nom, width = WN.CASES[name][1:3]
    pr, lk = device_logp(like, X[:n], nom - width, 2 * width)
    failed = host == -np.inf
    print("%s: %d of %d points -inf" % (name, failed[:n].sum(), n))
    assert lk.tobytes() == host[:n].tobytes()
    outside = np.any((X[:n] < nom - width) | (X[:n] > nom + width), axis=1)
    assert np.all(pr[outside] == -np.inf) and np.all(np.isfinite(pr[~outside]))
    if n == N_POINTS:
        assert outside.any()
        if starved:                                                     # failed and finished points inside one block of four waves
            blocks = failed[:n // 4 * 4].reshape(-1, 4)
            assert np.any(blocks.any(axis=1) & ~blocks.all(axis=1))
        else:
            assert np.all(np.isfinite(lk[~outside]))


def test_device_equals_host_twin_on_a_network_at_the_reaction_limit():
    """64 species, 256 bimolecular reactions: the longest generated sums the class accepts, same bits on both sides"""
    like = W.dense_network(64, 256, 64)
    X = NW.box_points(np.zeros(20), 67, 4, width=1.0)
    pr, lk = device_logp(like, X, np.full(20, -1.0), 2.0)
    host, steps = like.batch(X, return_steps=True)
    print("dense S=64 R=256: %d of %d points -inf, median %d steps" % (np.sum(host == -np.inf), len(X), np.median(steps)))
    assert lk.tobytes() == host.tobytes()
    assert np.mean(np.isfinite(host)) > 0.9


def test_everything_through_the_item_kernel_equals_the_host_build():
    """chain40 x 3 conditions, condition 1 with two events, a Monomial scale and one constraint: 67 points = 201 items, four to a block --
    the last block has three waves without an item, and the waves of a block hold different conditions"""
    like, _ = WN.chain_conditions(40, 3, events=True, monomials=True)
    assert "DZODE_GROUP_ITEM_ENTRIES(Net, 64)" in like.source() and "EVENTS = 2" in like.source() and "MONOMIALS" in like.source()
    assert [len(c["events"]) for c in like.conditions] == [0, 2, 0] and len(like.constraints) == 1
    nom = WN.CHAIN_NOMINAL
    X = NW.box_points(nom, 67, 25, width=1.0, outside=0.05 / len(nom))
    pr, lk = device_logp(like, X, nom - 1.0, 2.0)
    host = like.batch(X)
    assert lk.tobytes() == host.tobytes()
    assert np.isfinite(host).sum() > len(X) // 2


@pytest.mark.parametrize("multitry,hard,max_steps", [(False, True, 500), (3, False, 80)])
def test_run_dream_on_the_device_equals_the_oracle(tmp_path, multitry, hard, max_steps):
    """cascade49 with a wave per point against run_dream's own sequence on the oracle with the host twin as the Python likelihood; with
    max_steps 80 part of the prior box fails (0.4 of the seed archive; the starts near the nominal constants finish), so whole proposal
    sets can be impossible and are drawn again."""
    os.chdir(tmp_path)
    N, G = 8, 20
    like = WN.cascade(max_steps=max_steps)
    nom, width = WN.CAS.NOMINAL, WN.CASCADE_WIDTH
    params = [SampledParam(uniform, loc=nom - width, scale=2 * width)]
    rng = np.random.default_rng(78)
    Z0 = nom - width + 2 * width * rng.uniform(0, 1, (40, len(nom)))
    np.save("cascade_seed.npy", Z0)
    seed_like = like.batch(Z0)
    if max_steps < 500:
        assert np.mean(seed_like == -np.inf) > 0.2 and np.any(np.isfinite(seed_like))
    starts = [nom + 0.05 * rng.uniform(-1, 1, len(nom)) for _ in range(N)]
    assert np.all(np.isfinite(like.batch(np.array(starts))))
    kw = dict(multitry=multitry, gamma_levels=4, adapt_gamma=True, history_thin=1, hardboundaries=hard, history_file="cascade_seed.npy")
    run_dream_equals_oracle(like, params, starts, 56, N, G, **kw)
