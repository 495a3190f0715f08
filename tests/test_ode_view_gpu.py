"""MassActionODELogLike(conditions=[dict(params=...)]) on the MI355X (csrc/dz_ode.h, VIEWS): the item kernels of the four shapes gather
each item's view and give the host build's bits -- with a partly filled last block or groups without an item, and where some items of a
point fail --, the prediction kernels likewise, liveness is per item on the device too, and run_dream with a view equals the oracle
driven by the host build."""
import os

import numpy as np
import pytest
from scipy.stats import uniform

from pydream_amd.parameters import SampledParam

from . import ode_view_networks as VN
from .ode_support import device_equals_host, run_dream_equals_oracle

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("max_steps", [500, VN.STARVED_MAX_STEPS])
def test_device_equals_host_build_one_lane_per_item(max_steps):
    """1027 points x 3 conditions = 3081 items: 12 blocks and 9 items of a 13th; at max_steps 60 there are points that fail in every
    condition, in some, in none"""
    multi, _, _ = VN.basic("mm", max_steps=max_steps)
    X = VN.points("mm", 1027, 21, outside=0.05)
    failed = (multi.batch_conditions(X) == -np.inf).sum(axis=1)
    print("mm with views at max_steps %d: points failing in all / some / no conditions: %d / %d / %d"
          % (max_steps, np.sum(failed == 3), np.sum((failed > 0) & (failed < 3)), np.sum(failed == 0)))
    if max_steps == VN.STARVED_MAX_STEPS:
        assert np.any(failed == 3) and np.any((failed > 0) & (failed < 3)) and np.any(failed == 0)
    host = device_equals_host(multi, X, VN.nominal_of("mm"))
    if max_steps == 500:
        assert np.all(np.isfinite(host))


@pytest.mark.parametrize("name,n", [("enzyme13", 259), ("chain17", 131), (VN.WAVE, 67)])
def test_device_equals_host_twin_a_lane_group_or_a_wave_per_item(name, n):
    """enzyme13: 259 x 3 = 777 items, 16 to a block; chain17: 131 x 2 = 262, 8 to a block; the wave chain: 67 x 3 = 201, 4 to a block:
    the last block has groups without an item, which gather the last item's view"""
    multi, _, _ = VN.basic(name)
    host = device_equals_host(multi, VN.points(name, n, 21), VN.nominal_of(name))
    assert np.all(np.isfinite(host))


@pytest.mark.parametrize("lanes", [1, 16])
def test_the_prediction_kernels_follow_the_view(lanes):
    """every kind of reader remapped, 64 points x 3 items in chunks of 7 points"""
    multi, _, _, _ = VN.readers(lanes)
    X = VN.reader_points(lanes, 64, 32)
    with multi.device(chunk_items=21) as ev:
        assert ev.points_per_chunk() == 7
        terms = ev.batch_conditions(X)
        sim, again = ev.simulate(X, return_terms=True)
        total = ev.batch(X)
    assert terms.tobytes() == multi.batch_conditions(X).tobytes() == again.tobytes()
    assert sim.tobytes() == multi.simulate(X).tobytes() and total.tobytes() == multi.batch(X).tobytes()
    assert np.isfinite(terms).mean() > 0.9


@pytest.mark.parametrize("name", ["mm", "enzyme13"])
@pytest.mark.parametrize("bad", [np.nan, np.inf])
def test_liveness_is_per_item_on_the_device(name, bad):
    """condition 1 replaces the moved rate's index and reads the extra coordinate in its place; the others read the coordinate itself"""
    multi, _, maps = VN.basic(name)
    moved = next(i for i, t in maps[1].items() if isinstance(t, int))
    X = VN.points(name, 37, 34)
    Y = X.copy()
    Y[:, moved] = bad
    with multi.device() as ev:
        clean, terms, total = ev.batch_conditions(X), ev.batch_conditions(Y), ev.batch(Y)
    assert terms.tobytes() == multi.batch_conditions(Y).tobytes() and total.tobytes() == multi.batch(Y).tobytes()
    assert np.all(terms[:, 0] == -np.inf) and np.all(terms[:, 2] == -np.inf) and np.all(np.isfinite(terms[:, 1]))
    assert terms[:, 1].tobytes() == clean[:, 1].tobytes() and np.all(total == -np.inf)


@pytest.mark.parametrize("multitry", [False, 3])
def test_run_dream_with_a_view_on_the_device_equals_the_oracle(tmp_path, multitry):
    """mm on three gels -- a sampled scale per condition and a fixed-factor knock-down -- against run_dream's own sequence on the oracle
    with the host build as the Python likelihood: 8 chains, 40 generations"""
    os.chdir(tmp_path)
    N, G = 8, 40
    multi, _ = VN.mm_gels()
    nom = VN.GEL_NOMINAL
    assert multi.d == len(nom) == 6 and multi._view_size() == 7
    params = [SampledParam(uniform, loc=nom - 1.0, scale=2)]
    rng = np.random.default_rng(82)
    np.save("gels_seed.npy", nom - 1.0 + 2 * rng.uniform(0, 1, (60, len(nom))))
    box = nom - 1.0 + 2 * rng.uniform(0, 1, (200, len(nom)))
    starts = list(box[np.isfinite(multi.batch(box))][:N])
    assert len(starts) == N
    kw = dict(multitry=multitry, gamma_levels=4, adapt_gamma=True, history_thin=1, hardboundaries=not multitry, history_file="gels_seed.npy")
    run_dream_equals_oracle(multi, params, starts, 58, N, G, **kw)
