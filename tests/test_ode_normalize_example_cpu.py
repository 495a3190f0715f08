"""The shipped example of normalised readouts (pydream_amd/examples/normalized: a two-step cascade whose reporters are fractions of their
own maximum, with unknown noise) without a GPU: it builds, the generating point scores above perturbed ones, its simulate is the
un-normalised twin's trajectory over its maximum, and it cross-compiles for gfx950 without scratch."""
import functools

import numpy as np

from pydream_amd.examples.normalized import normalized_device as ND
from pydream_amd.likelihoods import MassActionODELogLike

from .ode_support import notes


@functools.lru_cache(maxsize=None)
def data():
    out = ND.simulated_data()
    out.setflags(write=False)
    return out


def test_the_example_builds_and_scores_the_generating_point_above_perturbed_ones():
    like = ND.make_likelihood(data=data())
    assert like.d == 7 and "NORMALIZE = 2" in like.source() and "NOISE = true" in like.source()
    assert np.isfinite(data()).sum() == 2 * len(ND.OBSERVED) and np.all(np.isnan(np.delete(data(), ND.OBSERVED, axis=1)))
    best = like(ND.NOMINAL)
    assert np.isfinite(best)
    for i in range(5):                      # (the five rate constants: half a decade off costs more than the noise explains)
        for step in (-0.5, 0.5):
            x = ND.NOMINAL.copy()
            x[i] += step
            assert like(x) < best - 3, (i, step)


def test_simulate_is_the_twins_trajectory_over_its_maximum_unobserved_rows_included():
    like = ND.make_likelihood(data=data())
    twin = MassActionODELogLike(5, ND.REACTIONS, ND.Y0, ND.TSPAN, ND.OBSERVABLES, np.full((2, len(ND.TSPAN)), np.nan), 1.0)
    X = ND.NOMINAL + 0.5 * np.random.default_rng(3).uniform(-1, 1, (16, 7))
    m, sim = twin.simulate(X), like.simulate(X)
    assert sim.tobytes() == (m / np.max(m, axis=1, keepdims=True)).tobytes() and np.all(np.max(sim, axis=1) == 1.0)
    peak = np.argmax(m, axis=1)
    assert np.any(~np.isin(peak, ND.OBSERVED))          # (some maxima lie on rows that carry no data)


def test_the_example_cross_compiles_for_gfx950_without_scratch():
    a = notes(ND.make_likelihood(data=data()).code_object())
    print("normalized example: %d VGPRs, %d AGPRs, scratch %d" % (a["vgpr"], a["agpr"], a["scratch"]))
    assert a["scratch"] == 0
