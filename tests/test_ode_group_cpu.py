"""MassActionODELogLike(lanes_per_point=16 | 32) without a GPU: the lane-group solver cross-compiles for gfx950 without scratch, its
host twin is as accurate against scipy's Radau as the one-lane build and has the Rosenbrock pair's orders, failures are -inf, the new
limits are checked at construction, and the default keyword still generates the one-lane source byte for byte."""
import hashlib
import os
import pickle
import subprocess

import numpy as np
import pytest

from pydream_amd import likelihoods as LK
from pydream_amd.likelihoods import MassActionODELogLike

from . import ode_networks as NW
from . import ode_wide_networks as W
from .ode_support import READELF, max_rel_err, notes

NAMES = list(W.CASES)


@pytest.mark.parametrize("name", NAMES)
def test_group_solver_cross_compiles_for_gfx950_without_scratch(name, tmp_path, monkeypatch):
    monkeypatch.setenv("DREAMZS_KERNEL_CACHE", str(tmp_path))
    like = W.CASES[name][0]()
    path = like.code_object()
    assert open(path, "rb").read(4) == b"\x7fELF" and like.code_object() == path
    syms = subprocess.run([READELF, "-s", path], capture_output=True, text=True).stdout
    assert "dz_ode_group_batch.kd" in syms
    n = notes(path)
    print("%s: S=%d R=%d: %d VGPRs (%d of them AGPRs), static LDS %d B, scratch %d"
          % (name, like.n_species, len(like.reactions), n["vgpr"], n["agpr"], n["lds"], n["scratch"]))
    assert n["scratch"] == 0
    assert n["lds"] == (256 // like.lanes_per_point) * (len(like.reactions) + 1) * 8      # the rate constants, a padded row per point


@pytest.mark.parametrize("S,R,lanes", [(32, 128, 32), (32, 64, 32), (24, 128, 32), (16, 128, 16)])
def test_networks_at_the_reaction_limit_compile_without_scratch(S, R, lanes, tmp_path, monkeypatch):
    """Every species in about 3 R / S bimolecular reactions, up to the 128 reactions the class accepts: scratch 0.  The generated sums
    are fenced every four terms, so what a lane holds at once hardly depends on R (measured: 32 species at 32 / 64 / 128 reactions
    374 / 401 / 407 registers)."""
    monkeypatch.setenv("DREAMZS_KERNEL_CACHE", str(tmp_path))
    n = notes(W.dense_network(S, R, lanes).code_object())
    print("dense S=%d R=%d @%d: %d VGPRs (%d of them AGPRs), static LDS %d B, scratch %d" % (S, R, lanes, n["vgpr"], n["agpr"], n["lds"], n["scratch"]))
    assert n["scratch"] == 0


@pytest.mark.parametrize("S,R,lanes", [(8, 64, 1), (8, 32, 1)])
def test_one_lane_networks_at_the_reaction_limit_compile_without_scratch(S, R, lanes, tmp_path, monkeypatch):
    """The one-lane build at its limits, 8 species and up to 64 reactions, on the same recipe (20 parameters): scratch 0.  Above 16
    reactions its generated source builds every sum up reaction by reaction behind fences and keeps one rate constant per parameter
    (_ode_source._ode_long_source); written like the short form these two took 512 registers and 796 / 84 bytes of scratch."""
    monkeypatch.setenv("DREAMZS_KERNEL_CACHE", str(tmp_path))
    like = W.dense_network(S, R, lanes)
    assert "DZODE_FENCE" in like.source() and "dz_ode_group" not in like.source()
    n = notes(like.code_object())
    print("dense S=%d R=%d @%d: %d VGPRs (%d of them AGPRs), scratch %d" % (S, R, lanes, n["vgpr"], n["agpr"], n["scratch"]))
    assert n["scratch"] == 0


@pytest.mark.parametrize("name", NAMES)
def test_host_twin_is_accurate_against_radau_and_error_shrinks_with_tolerance(name):
    """The one-lane build's criterion, unchanged: every output within 10 requested tolerances of Radau at rtol 1e-12 over a +-1 decade
    box, at 1e-6 and at 1e-9, and the absolute error at 1e-9 below 1e-2 of that at 1e-6."""
    make, nominal, (S, rx, y0, t) = W.CASES[name]
    X = NW.box_points(nominal, 30 if S == 13 else 20, 13, width=1.0)
    obs = make().observables
    import multiprocessing
    from concurrent.futures import ProcessPoolExecutor
    with ProcessPoolExecutor(max(1, min(8, len(os.sched_getaffinity(0)))), mp_context=multiprocessing.get_context("fork")) as ex:
        refs = [y @ obs.T for y in ex.map(NW.radau, *zip(*[(S, rx, y0, t, x) for x in X]), chunksize=2)]
    errs = []
    for rtol in (1e-6, 1e-9):
        like = make(rtol=rtol, atol=rtol, max_steps=20000)
        errs.append(max_rel_err(like, refs, X, rtol))
    print(name, errs)
    assert errs[0] < 10 and errs[1] < 10
    abs_errs = [e * r for e, r in zip(errs, (1e-6, 1e-9))]
    assert abs_errs[1] < 1e-2 * abs_errs[0]


@pytest.mark.parametrize("lanes", [16, 32])
def test_rosenbrock_pair_has_orders_four_and_three_through_the_group_path(lanes):
    """Fixed steps h and h/2 on a smooth non-stiff network: error ratios 2^(4 +- 0.3) for the solution, 2^(3 +- 0.3) for the embedded one."""
    rx = [({0: 1}, {1: 1}, 0.7), ({1: 1}, {0: 1}, 0.3), ({1: 1, 2: 1}, {3: 1}, 1.1), ({3: 1}, {2: 1}, 0.4)]
    y0 = [1.0, 0.2, 0.8, 0.0]
    m = MassActionODELogLike(4, rx, y0, [2.0], [[1, 0, 0, 0]], [[1.0]], [[1.0]], ndim=0, lanes_per_point=lanes)
    ref = NW.radau(4, [(a, b, i) for i, (a, b, _) in enumerate(rx)], y0, [2.0], np.log10([0.7, 0.3, 1.1, 0.4]), rtol=1e-13, atol=1e-15)[-1]
    for embedded, p in ((False, 4), (True, 3)):
        e = np.array([np.max(np.abs(m.fixed_steps([], 2.0, n, embedded) - ref)) for n in (10, 20, 40)])
        rates = np.log2(e[:-1] / e[1:])
        print("embedded" if embedded else "solution", e, rates)
        assert np.all(np.abs(rates - p) < 0.3), (embedded, rates)


@pytest.mark.parametrize("name", NAMES)
def test_prior_box_never_fails_at_default_settings_and_a_starved_step_cap_is_minus_infinity(name):
    """2 000 points of the +-1 decade box: none fails at the defaults; with max_steps 75 (enzyme13) / 40 (chains) per output interval a
    share in [0.1, 0.9] is -inf.  The one-lane algorithm's host build fails 0.73 / 0.31 of enzyme13 at 70 / 80 and 0.61, 0.48, 0.25 of
    chain8, chain16, chain32 at 40; the group path, measured: enzyme13@16 0.5385, chain16@16 0.4795, chain17@32 0.475, chain32@32
    0.25, chain8@16 0.6045."""
    make, nominal, _ = W.CASES[name]
    X = NW.box_points(nominal, 2000, 5, width=1.0)
    L, steps = make().batch(X, return_steps=True)
    assert np.all(np.isfinite(L)), X[~np.isfinite(L)]
    few = make(max_steps=W.STARVED_MAX_STEPS[name])
    share = float(np.mean(few.batch(X) == -np.inf))
    print("%s: steps per point: median %d, max %d; -inf share at max_steps %d: %.4f" % (name, np.median(steps), steps.max(), W.STARVED_MAX_STEPS[name], share))
    assert 0.1 <= share <= 0.9
    bad = nominal.copy()
    for v in (np.nan, np.inf, -np.inf, 400.0):
        bad[3] = v
        assert make()(bad) == -np.inf


def _enzyme_kw(**over):
    from pydream_amd.examples.enzyme import enzyme_device as ENZ
    kw = dict(n_species=13, reactions=ENZ.REACTIONS, y0=ENZ.Y0, t=ENZ.TSPAN, observables=ENZ.OBSERVABLES, data=np.ones((4, 20)), sd=np.ones((4, 20)),
              lanes_per_point=16)
    kw.update(over)
    return kw


# sha256 of source() on the commit before the lanes_per_point keyword existed; the long one-lane form and the two group sources: on the
# commit before the three generators shared their scaffolding
PARENT_SOURCE_SHA256 = {"robertson": "c4fd92120c3b297f5ca95cc5badd01f82fb4e13702022f116b6aa3a583f6be0e",
                        "chain8": "7c21c344e8c175a67e16fed278d7b683bdd838ae0231a090733fec458e45c951",
                        "dense8x64@1": "13626834e185b0af64b9033f11ca543aaa69a2bb9f8d179186fda84ef67665f5",
                        "enzyme13@16": "0aa13e4724688b1327784e38675d9c71e37520f6bfef3fb95eef62929af3b1f6",
                        "chain32@32": "21746d67757913646ba884447bf66fb3a2f51064cd1323f94c2fcc26e9f3e804"}


def test_construction_checks_defaults_unchanged_and_pickle():
    one = [({0: 1}, {1: 1}, 0)]
    for over, msg in [(dict(n_species=17, y0=np.zeros(17), observables=np.ones((1, 17))), r"n_species must be 1\.\.16"),
                      (dict(n_species=33, y0=np.zeros(33), observables=np.ones((1, 33)), lanes_per_point=32), r"n_species must be 1\.\.32"),
                      (dict(lanes_per_point=8), "lanes_per_point"),
                      (dict(lanes_per_point=64), "lanes_per_point"),
                      (dict(lanes_per_point=0), "lanes_per_point"),
                      (dict(reactions=one * 129), r"1\.\.128 reactions"),
                      (dict(observables=np.ones((17, 13)), data=np.ones((17, 20)), sd=np.ones((17, 20))), r"O = 1\.\.16"),
                      (dict(lanes_per_point=1), r"n_species must be 1\.\.8")]:
        with pytest.raises(ValueError, match=msg):
            MassActionODELogLike(**_enzyme_kw(**over))
    MassActionODELogLike(**_enzyme_kw(reactions=one * 128))
    MassActionODELogLike(**_enzyme_kw(observables=np.ones((16, 13)), data=np.ones((16, 20)), sd=np.ones((16, 20))))
    MassActionODELogLike(**_enzyme_kw(n_species=32, y0=np.zeros(32), observables=np.ones((1, 32)), data=np.ones((1, 20)), sd=np.ones((1, 20)),
                                      lanes_per_point=32))
    assert LK.ODE_LIMITS == dict(species=8, reactions=64, observables=8, times=4096)
    assert LK.ODE_GROUP_LIMITS["reactions"] == 128 and LK.ODE_GROUP_LIMITS["observables"] == 16
    for make in (NW.robertson, NW.chain8):                                  # the default keyword: the one-lane source, byte for byte
        like = make()
        assert like.lanes_per_point == 1 and "dz_ode_group" not in like.source()
        assert hashlib.sha256(like.source().encode()).hexdigest() == PARENT_SOURCE_SHA256[make.__name__]
    for name, like in (("dense8x64@1", W.dense_network(8, 64, 1)), ("enzyme13@16", W.enzyme13()), ("chain32@32", W.chain(32, 32))):
        assert hashlib.sha256(like.source().encode()).hexdigest() == PARENT_SOURCE_SHA256[name], name
    like = W.enzyme13()
    assert like.lanes_per_point == 16 and "DZODE_GROUP_ENTRIES(Net, 16)" in like.source()
    assert "DZODE_GROUP_ENTRIES(Net, 32)" in W.enzyme13(lanes=32).source()
    X = NW.box_points(W.ENZ.NOMINAL, 6, 8, width=1.0)
    back = pickle.loads(pickle.dumps(like))
    assert back._host is None and back.lanes_per_point == 16 and back.batch(X).tobytes() == like.batch(X).tobytes()
    sim = like.simulate(X)
    assert sim.shape == (6, 20, 4)
    from scipy.stats import norm
    for x, s in zip(X, sim):
        ref = float(np.sum(norm(loc=like.data, scale=like.sd).logpdf(s.T)))
        assert abs(like(x) - ref) <= 1e-9 * abs(ref)
    wide = W.enzyme13(lanes=32)                                             # idle lanes change the summation tree's padding, not the method
    np.testing.assert_allclose(wide.batch(X), like.batch(X), rtol=1e-5)


def test_group_and_one_lane_builds_agree_to_the_tolerance_on_a_network_both_run():
    rx, y0, obs = W.chain_network(8)
    grp = W.chain(8, 16, rtol=1e-9, atol=1e-9)
    one = MassActionODELogLike(8, rx, y0, W.CHAIN_T, obs, grp.data, grp.sd, rtol=1e-9, atol=1e-9)
    X = NW.box_points(W.CHAIN_NOMINAL, 50, 3, width=1.0)
    a, b = grp.simulate(X), one.simulate(X)
    assert np.max(np.abs(a - b)) < 1e-7


# name -> (constructor(**kw), nominal, half width of the box, a max_steps that starves part of the box, whether fixed_steps goes in)
HOST_CASES = {
    "robertson": (NW.robertson, NW.ROB.NOMINAL, 3.0, 40, False),
    "chain8": (NW.chain8, NW.CHAIN_NOMINAL, 1.0, 40, True),
    "chain8@16": (lambda **kw: W.chain(8, 16, **kw), W.CHAIN_NOMINAL, 1.0, 40, True),
    "enzyme13@16": (W.enzyme13, W.ENZ.NOMINAL, 1.0, 75, False),
    "chain32@32": (lambda **kw: W.chain(32, 32, **kw), W.CHAIN_NOMINAL, 1.0, 40, False),
}
PARENT_HOST_SHA256 = {"robertson": "43c3380897edf22280ddfbd126007403115176acb4c01c336411825e6dbb9989",
                      "chain8": "e980ecfea219174727f302d18ad2e759a79a2b6665b7e2e5ea41be1713594bc9",
                      "chain8@16": "83a6094adeff4063d4b5999e54f29b6355a5a155b11e545e1a1d0426101f45c3",
                      "enzyme13@16": "fc43c0735d58eee514f22772ac1011b7cb636912cd54dc082bf682cc5908c94e",
                      "chain32@32": "00bf1a20cf3dc90bf581dd020cf15c916f0415bf99cc894e95be07343a0c265a"}


def _six_decimals(like):
    """The networks' data come from scipy's Radau, whose last bits may depend on the LAPACK build: pinned to six decimals, so that what
    the digest sees is this project's arithmetic alone."""
    like.data, like.sd = np.round(like.data, 6), np.round(like.sd, 6)
    return like


@pytest.mark.parametrize("name", list(HOST_CASES))
def test_host_results_have_the_bits_of_the_commit_before_the_shared_stepping_loop(name):
    """sha256 over batch (values and step counts) on 200 box points, simulate on the first 20, batch again under a step cap that starves
    part of the box (the max_steps exit; -inf and the steps taken until then) and, for one network per shape, fixed_steps of both
    orders.  PARENT_HOST_SHA256 was recorded by running exactly this code on the parent commit, where the one-lane loop, the lane
    group's loop and the host twin's loop were three copies.  The host build uses + - * / and correctly rounded fma with contraction off,
    so the digests do not depend on the compiler; the GPU tests require device bytes == host bytes, so this pins the device too."""
    make, nominal, width, starved, fixed = HOST_CASES[name]
    X = NW.box_points(nominal, 200, 17, width=width)
    like = _six_decimals(make())
    L, steps = like.batch(X, return_steps=True)
    h = hashlib.sha256(L.tobytes() + steps.tobytes() + like.simulate(X[:20]).tobytes())
    Ls, ss = _six_decimals(make(max_steps=starved)).batch(X, return_steps=True)
    h.update(Ls.tobytes() + ss.tobytes())
    if fixed:
        for embedded in (False, True):
            h.update(like.fixed_steps(X[0], 2.0, 10, embedded).tobytes())
    print(name, "finite", int(np.isfinite(L).sum()), "finite when starved", int(np.isfinite(Ls).sum()), "steps", int(steps.sum()), h.hexdigest())
    assert 0 < np.isfinite(Ls).sum() < len(X)
    assert h.hexdigest() == PARENT_HOST_SHA256[name]
