"""MassActionODELogLike(lanes_per_point=64) without a GPU: the wave-per-point solver cross-compiles for gfx950 without scratch up to 64
species and 256 reactions (also the item kernel, events and Monomials), the limits are checked at construction, its host twin is as
accurate against scipy's Radau as the lane group's, failures are -inf exactly where the step cap was hit, and the terms of a
multi-condition object are its single experiments."""
import multiprocessing
import os
import pickle
import subprocess
from concurrent.futures import ProcessPoolExecutor

import numpy as np
import pytest

from pydream_amd import likelihoods as LK
from pydream_amd.likelihoods import MassActionODELogLike

from . import ode_condition_networks as CN
from . import ode_networks as NW
from . import ode_wave_networks as WN
from . import ode_wide_networks as W
from .ode_support import READELF, max_rel_err, notes

COMPILE_CASES = {
    "chain33": (lambda: WN.chain(33), False),
    "chain48": (lambda: WN.chain(48), False),
    "chain64": (lambda: WN.chain(64), False),
    "cascade49": (WN.cascade, False),
    "dense64x128": (lambda: W.dense_network(64, 128, 64), False),
    "dense64x256": (lambda: W.dense_network(64, 256, 64), False),
    "chain64x2conditions": (lambda: WN.chain_conditions(64, 2)[0], True),
    "chain40+3events": (lambda: WN.chain_with_events(40, 3), False),
    "chain40+monomials": (lambda: WN.chain_with_monomials(40), False),
}


@pytest.mark.parametrize("name", list(COMPILE_CASES))
def test_wave_solver_cross_compiles_for_gfx950_without_scratch(name, tmp_path, monkeypatch):
    monkeypatch.setenv("DREAMZS_KERNEL_CACHE", str(tmp_path))
    make, items = COMPILE_CASES[name]
    like = make()
    assert like.lanes_per_point == 64
    assert ("DZODE_GROUP_ITEM_ENTRIES(Net, 64)" if items else "DZODE_GROUP_ENTRIES(Net, 64)") in like.source()
    assert ("EVENTS = 3" in like.source()) == (name == "chain40+3events") and ("MONOMIALS" in like.source()) == (name == "chain40+monomials")
    path = like.code_object()
    assert open(path, "rb").read(4) == b"\x7fELF"
    syms = subprocess.run([READELF, "-s", path], capture_output=True, text=True).stdout
    assert ("dz_ode_group_item_batch.kd" if items else "dz_ode_group_batch.kd") in syms
    n = notes(path)
    print("%s: S=%d R=%d: %d VGPRs (%d of them AGPRs), static LDS %d B, scratch %d"
          % (name, like.n_species, len(like.reactions), n["vgpr"], n["agpr"], n["lds"], n["scratch"]))
    assert n["scratch"] == 0
    assert n["lds"] == 4 * (len(like.reactions) + 1 + like.n_species) * 8     # four waves: the rate constants (a padded row) and the state


def _kw(S, **over):
    rx, y0, obs = W.chain_network(S)
    kw = dict(n_species=S, reactions=rx, y0=y0, t=W.CHAIN_T, observables=obs, data=np.ones((8, 11)), sd=np.ones((8, 11)), lanes_per_point=64)
    kw.update(over)
    return kw


def test_construction_limits_of_the_wave_shape_and_pickle():
    one = [({0: 1}, {1: 1}, 0)]
    assert LK.ODE_WAVE_LIMITS == dict(species=64, reactions=256, observables=16, times=4096, lanes=(64,), conditions=64)
    assert LK.ODE_GROUP_LIMITS == dict(species=32, reactions=128, observables=16, times=4096, lanes=(16, 32), conditions=64)
    assert LK.ODE_LIMITS == dict(species=8, reactions=64, observables=8, times=4096)
    for S in (33, 64):
        like = MassActionODELogLike(**_kw(S))
        assert like.lanes_per_point == 64 and "DZODE_GROUP_ENTRIES(Net, 64)" in like.source()
    with pytest.raises(ValueError, match=r"n_species must be 1\.\.64"):
        MassActionODELogLike(**_kw(33, n_species=65, y0=np.zeros(65), observables=np.ones((1, 65)), data=np.ones((1, 11)), sd=np.ones((1, 11))))
    with pytest.raises(ValueError, match=r"lanes_per_point=64 is for networks of 33\.\.64 species; use 16 or 32"):
        MassActionODELogLike(**_kw(32))
    with pytest.raises(ValueError, match="lanes_per_point"):
        MassActionODELogLike(**_kw(13))
    with pytest.raises(ValueError, match=r"lanes_per_point must be 1, 16, 32 or 64"):
        MassActionODELogLike(**_kw(33, lanes_per_point=48))
    MassActionODELogLike(**_kw(64, reactions=one * 256))
    with pytest.raises(ValueError, match=r"1\.\.256 reactions"):
        MassActionODELogLike(**_kw(64, reactions=one * 257))
    with pytest.raises(ValueError, match=r"1\.\.128 reactions"):
        MassActionODELogLike(**_kw(32, reactions=one * 129, lanes_per_point=32))
    with pytest.raises(ValueError, match=r"O = 1\.\.16"):
        MassActionODELogLike(**_kw(40, observables=np.ones((17, 40)), data=np.ones((17, 11)), sd=np.ones((17, 11))))
    like = WN.chain(33)
    X = NW.box_points(WN.CHAIN_NOMINAL, 6, 8, width=1.0)
    back = pickle.loads(pickle.dumps(like))
    assert back._host is None and back.lanes_per_point == 64 and back.batch(X).tobytes() == like.batch(X).tobytes()


@pytest.mark.parametrize("name", ["chain64", "cascade49"])
def test_host_twin_is_accurate_against_radau_and_error_shrinks_with_tolerance(name):
    """test_ode_group_cpu's criterion and thresholds (those it applies to chain32 @ 32): every output within 10 requested tolerances of
    Radau at rtol 1e-12 over the prior box, at 1e-6 and at 1e-9, and the absolute error at 1e-9 below 1e-2 of that at 1e-6."""
    make, nominal, width, (S, rx, y0, t) = WN.CASES[name]
    X = NW.box_points(nominal, 12, 13, width=width)
    obs = make().observables
    with ProcessPoolExecutor(max(1, min(8, len(os.sched_getaffinity(0)))), mp_context=multiprocessing.get_context("fork")) as ex:
        refs = [y @ obs.T for y in ex.map(NW.radau, *zip(*[(S, rx, y0, t, x) for x in X]), chunksize=2)]
    errs = []
    for rtol in (1e-6, 1e-9):
        errs.append(max_rel_err(make(rtol=rtol, atol=rtol, max_steps=20000), refs, X, rtol))
    print(name, errs)
    assert errs[0] < 10 and errs[1] < 10
    abs_errs = [e * r for e, r in zip(errs, (1e-6, 1e-9))]
    assert abs_errs[1] < 1e-2 * abs_errs[0]


@pytest.mark.parametrize("S", [33, 48, 64])
def test_prior_box_never_fails_at_default_settings_and_a_starved_step_cap_is_minus_infinity(S):
    """259 points of the +-1 decade box: none fails at the defaults; with max_steps 40 per output interval some fail and some do not, and
    -inf stands exactly where an interval ran into the cap (the steps that passed the finiteness test reach 40 in some interval only
    then: a point that finishes under the cap takes the same steps as at the default settings)."""
    X = NW.box_points(WN.CHAIN_NOMINAL, 259, 21, width=1.0)
    L, steps = WN.chain(S).batch(X, return_steps=True)
    assert np.all(np.isfinite(L)), X[~np.isfinite(L)]
    Ls, ss = WN.chain(S, max_steps=WN.STARVED_MAX_STEPS).batch(X, return_steps=True)
    failed = Ls == -np.inf
    print("chain%d: steps per point: median %d, max %d; %d of 259 -inf at max_steps %d" % (S, np.median(steps), steps.max(), failed.sum(), WN.STARVED_MAX_STEPS))
    assert 0 < failed.sum() < len(X)
    assert Ls[~failed].tobytes() == L[~failed].tobytes() and np.array_equal(ss[~failed], steps[~failed])
    assert np.all(ss[failed] < steps[failed])                               # stopped at the cap, short of the steps the point needs
    bad = WN.CHAIN_NOMINAL.copy()
    for v in (np.nan, np.inf, -np.inf, 400.0):
        bad[3] = v
        assert WN.chain(S)(bad) == -np.inf


def test_the_cascades_prior_box_never_fails_at_default_settings():
    """the example's own box, +-0.5 decades around its nominal constants"""
    X = NW.box_points(WN.CAS.NOMINAL, 67, 21, width=WN.CASCADE_WIDTH)
    L, steps = WN.cascade().batch(X, return_steps=True)
    print("cascade49: steps per point: median %d, max %d" % (np.median(steps), steps.max()))
    assert np.all(np.isfinite(L)), X[~np.isfinite(L)]
    assert len(WN.CAS.REACTIONS) == 72 and WN.CAS.N_SPECIES == 49 and len(WN.CAS.NOMINAL) == 12


def test_the_terms_of_three_conditions_are_the_single_experiments():
    multi, single = WN.chain_conditions(40, 3)
    X = NW.box_points(WN.CHAIN_NOMINAL, 24, 22, width=1.0)
    terms = multi.batch_conditions(X)
    assert terms.shape == (24, 3) and np.all(np.isfinite(terms))
    for c in range(3):
        assert terms[:, c].tobytes() == single(c).batch(X).tobytes(), c
    assert multi.batch(X).tobytes() == ((terms[:, 0] + terms[:, 1]) + terms[:, 2]).tobytes() == CN.left_to_right(terms).tobytes()
