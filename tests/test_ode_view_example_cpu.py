"""The shipped knock-down example (pydream_amd/examples/knockdown: a sampled knock-down efficiency, a known inhibitor factor on a formal
index and a sampled scale per gel, all through the conditions' "params") without a GPU: it builds in both shapes it offers, the
generating point scores above a perturbed one, every experiment's term is the single experiment's at the viewed row, and both shapes
cross-compile for gfx950 without scratch."""
import functools

import numpy as np
import pytest

from pydream_amd.examples.knockdown import knockdown_device as KD
from pydream_amd.likelihoods import MassActionODELogLike

from . import ode_condition_networks as CN
from . import ode_networks as NW
from . import ode_view_networks as VN
from .ode_support import notes


@functools.lru_cache(maxsize=None)
def data():
    out = KD.simulated_data()
    out.setflags(write=False)
    return out


@pytest.mark.parametrize("lanes", [1, 16])
def test_the_example_builds_in_both_shapes(lanes):
    like = KD.make_likelihood(data=data(), lanes_per_point=lanes)
    assert like.lanes_per_point == lanes and len(like.conditions) == len(KD.EXPERIMENTS) == 6
    assert like.d == KD.NDIM == 8 and like._view_size() == KD.FACTOR + 1 == 9 and "VIEW = 9" in like.source()
    assert np.isfinite(like(KD.TRUE))


def test_the_generating_point_scores_above_a_perturbed_one():
    like = KD.make_likelihood(data=data())
    best = like(KD.TRUE)
    for i in range(KD.NDIM):
        x = KD.TRUE.copy()
        x[i] += 0.3 if i != KD.EFF else -0.3
        assert like(x) < best - 5, i


@pytest.mark.parametrize("lanes", [1, 16])
def test_every_experiment_is_the_single_experiment_at_its_viewed_row(lanes):
    like = KD.make_likelihood(data=data(), lanes_per_point=lanes)
    maps = [KD.params_of(*exp) for exp in KD.EXPERIMENTS]
    X = NW.box_points(KD.LOWER + 0.5 * KD.WIDTH, 16, 51, width=0.4)
    terms = like.batch_conditions(X)
    for c, cond in enumerate(like.conditions):
        one = MassActionODELogLike(4, KD.REACTIONS, KD.Y0, KD.TSPAN, KD.OBSERVABLES, cond["data"], cond["sd"], scale=like.scale, lanes_per_point=lanes)
        assert terms[:, c].tobytes() == one.batch(VN.viewed(maps, c, X, 9)).tobytes(), c
    assert like.batch(X).tobytes() == CN.left_to_right(terms).tobytes() and np.all(np.isfinite(terms))


@pytest.mark.parametrize("lanes", [1, 16])
def test_the_example_cross_compiles_for_gfx950_without_scratch(lanes):
    a = notes(KD.make_likelihood(data=data(), lanes_per_point=lanes).code_object())
    print("knockdown @%d: %d VGPRs, %d AGPRs, scratch %d, LDS %d" % (lanes, a["vgpr"], a["agpr"], a["scratch"], a["lds"]))
    assert a["scratch"] == 0
