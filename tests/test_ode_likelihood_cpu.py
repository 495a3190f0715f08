"""MassActionODELogLike without a GPU: the generated solver cross-compiles for gfx950 without scratch on the networks here (the one-lane
limit of 64 reactions: tests/test_ode_group_cpu.py; the measured boundary beyond it: DESIGN.md), the host build of the same source
is accurate against scipy's Radau and has the Rosenbrock pair's orders, limits are checked at construction, and the kernel cache refuses
a fallback directory that others could write to."""
import os
import pickle
import stat
import subprocess

import numpy as np
import pytest

from oracle import oracle as O
from pydream_amd import likelihoods as LK
from pydream_amd.likelihoods import MassActionODELogLike

from . import ode_networks as NW
from .ode_support import READELF, max_rel_err, notes


@pytest.mark.parametrize("make", [NW.robertson, NW.chain8])
def test_generated_solver_cross_compiles_for_gfx950_without_scratch(make, tmp_path, monkeypatch):
    monkeypatch.setenv("DREAMZS_KERNEL_CACHE", str(tmp_path))
    like = make()
    path = like.code_object()
    assert open(path, "rb").read(4) == b"\x7fELF" and like.code_object() == path
    syms = subprocess.run([READELF, "-s", path], capture_output=True, text=True).stdout
    assert "dz_ode_batch.kd" in syms
    n = notes(path)
    print("S=%d: %d VGPRs, %d AGPRs, scratch %d" % (like.n_species, n["vgpr"], n["agpr"], n["scratch"]))
    assert n["scratch"] == 0
    assert MassActionODELogLike(**_robertson_kw(), path=path).code_object() == path          # a code object built beforehand


def _robertson_kw(**over):
    kw = dict(n_species=3, reactions=NW.ROB.REACTIONS, y0=NW.ROB.Y0, t=NW.ROB.TSPAN, observables=[[0, 0, 1]],
              data=np.ones((1, 50)), sd=np.ones((1, 50)))
    kw.update(over)
    return kw


@pytest.mark.parametrize("net", ["robertson", "mm", "chain8"])
def test_host_build_is_accurate_against_radau_and_error_shrinks_with_tolerance(net):
    """Every output within a small multiple of the requested tolerance of Radau at rtol 1e-12; the error falls with the tolerance."""
    if net == "robertson":
        S, rx, y0, t, make, X = 3, NW.ROB.REACTIONS, NW.ROB.Y0, NW.ROB.TSPAN, NW.robertson, NW.box_points(NW.ROB.NOMINAL, 300, 11)
    elif net == "mm":
        S, rx, y0, t, make, X = 4, NW.MM_REACTIONS, NW.MM_Y0, NW.MM_T, NW.michaelis_menten, NW.box_points(NW.MM_NOMINAL, 60, 12, width=1.0)
    else:
        S, rx, y0, t, make, X = 8, NW.CHAIN_REACTIONS, NW.CHAIN_Y0, NW.CHAIN_T, NW.chain8, NW.box_points(NW.CHAIN_NOMINAL, 40, 13, width=1.0)
    obs = make().observables
    import multiprocessing
    from concurrent.futures import ProcessPoolExecutor
    with ProcessPoolExecutor(max(1, min(8, len(os.sched_getaffinity(0)))), mp_context=multiprocessing.get_context("fork")) as ex:
        refs = [y @ obs.T for y in ex.map(NW.radau, *zip(*[(S, rx, y0, t, x) for x in X]), chunksize=4)]
    errs = []
    for rtol in (1e-6, 1e-9):
        like = make(rtol=rtol, atol=rtol, max_steps=20000)
        errs.append(max_rel_err(like, refs, X, rtol))
    print(net, errs)
    assert errs[0] < 10 and errs[1] < 10
    abs_errs = [e * r for e, r in zip(errs, (1e-6, 1e-9))]
    assert abs_errs[1] < 1e-2 * abs_errs[0]


def test_rosenbrock_pair_has_orders_four_and_three():
    """Fixed steps h and h/2 on a smooth non-stiff network: the error ratios are 2^(4 +- 0.3) for the solution and 2^(3 +- 0.3) for the
    embedded one (a mistyped tableau coefficient breaks one of the two)."""
    rx = [({0: 1}, {1: 1}, 0.7), ({1: 1}, {0: 1}, 0.3), ({1: 1, 2: 1}, {3: 1}, 1.1), ({3: 1}, {2: 1}, 0.4)]
    y0 = [1.0, 0.2, 0.8, 0.0]
    m = MassActionODELogLike(4, rx, y0, [2.0], [[1, 0, 0, 0]], [[1.0]], [[1.0]], ndim=0)
    ref = NW.radau(4, [(a, b, i) for i, (a, b, _) in enumerate(rx)], y0, [2.0], np.log10([0.7, 0.3, 1.1, 0.4]), rtol=1e-13, atol=1e-15)[-1]
    for embedded, p in ((False, 4), (True, 3)):
        e = np.array([np.max(np.abs(m.fixed_steps([], 2.0, n, embedded) - ref)) for n in (10, 20, 40)])
        rates = np.log2(e[:-1] / e[1:])
        print("embedded" if embedded else "solution", e, rates)
        assert np.all(np.abs(rates - p) < 0.3), (embedded, rates)


def test_prior_box_failures_and_bad_parameters():
    like = NW.robertson()
    X = NW.box_points(NW.ROB.NOMINAL, 2000, 5)
    L, steps = like.batch(X, return_steps=True)
    assert np.all(np.isfinite(L)), X[~np.isfinite(L)]                      # no point of the prior box fails at default settings
    print("steps per point: median %d, max %d" % (np.median(steps), steps.max()))
    few = NW.robertson(max_steps=20)
    assert np.mean(few.batch(X) == -np.inf) > 0.3                           # too few steps per interval: -inf
    for bad in ([np.nan, 7.0, 4.0], [-1.0, np.inf, 4.0], [-1.0, 7.0, -np.inf], [400.0, 7.0, 4.0]):
        assert like(np.array(bad)) == -np.inf


def test_exp_log_restatement_equals_the_oracle_bit_for_bit():
    L = NW.robertson().host_library()
    rng = np.random.default_rng(3)
    xe = np.concatenate([rng.uniform(-745, 710, 5000), rng.uniform(-5, 5, 4990), [0.0, -0.0, 709.78, -745.1, 1e-300, np.inf, -np.inf, 800, -800, 2.302585092994046]])
    xl = np.concatenate([np.exp(rng.uniform(-700, 700, 5000)), rng.uniform(0.5, 2.0, 4990), [5e-324, 1e-310, 1.0, 2.0, 0.0, np.inf, 1e308, 0.7071067811865476, 1.4142135623730951, 3.0]])
    for f, g, xs in ((L.dzode_exp, O.exp, xe), (L.dzode_log, O.log, xl)):
        a = np.array([f(float(x)) for x in xs])
        b = np.array([g(float(x)) for x in xs])
        assert a.tobytes() == b.tobytes()


def test_construction_checks_and_api():
    for over, msg in [(dict(n_species=9, y0=np.zeros(9), observables=np.ones((1, 9))), "n_species"),
                      (dict(reactions=[({0: 1}, {1: 1}, 0)] * 65), "reactions"),
                      (dict(observables=np.ones((9, 3)), data=np.ones((9, 50)), sd=np.ones((9, 50))), "observables"),
                      (dict(t=np.linspace(0, 1, 4097), data=np.ones((1, 4097)), sd=np.ones((1, 4097))), "output times"),
                      (dict(t=np.linspace(40, 0)), "sorted"),
                      (dict(t=np.linspace(-1, 40)), "sorted"),
                      (dict(reactions=[({0: 1.5}, {1: 1}, 0)]), "non-negative integers"),
                      (dict(reactions=[({0: -1}, {1: 1}, 0)]), "non-negative integers"),
                      (dict(reactions=[({3: 1}, {1: 1}, 0)]), "species"),
                      (dict(reactions=[({0: 1}, {1: 1}, 3)], ndim=3), "ndim"),
                      (dict(reactions=[({0: 1}, {1: 1}, "k")]), "rate"),
                      (dict(y0=[1.0, -1.0, 0.0]), "y0"),
                      (dict(sd=np.zeros((1, 50))), "sd"),
                      (dict(data=np.ones((1, 49))), "data"),
                      (dict(rate_scale="ln"), "rate_scale")]:
        with pytest.raises(ValueError, match=msg):
            MassActionODELogLike(**_robertson_kw(**over))
    like = NW.robertson()
    X = NW.box_points(NW.ROB.NOMINAL, 20, 8)
    sim = like.simulate(X)
    assert sim.shape == (20, 50, 1)
    from scipy.stats import norm
    for x, s in zip(X, sim):
        ref = float(np.sum(norm(loc=like.data, scale=like.sd).logpdf(s.T)))
        assert abs(like(x) - ref) <= 1e-9 * abs(ref)
    mm = NW.michaelis_menten()                                              # NaN data: that entry does not count
    s = mm.simulate(NW.MM_NOMINAL)[0].T
    seen = np.isfinite(mm.data)
    assert abs(mm(NW.MM_NOMINAL) - np.sum(norm(loc=mm.data[seen], scale=mm.sd[seen]).logpdf(s[seen]))) < 1e-9
    back = pickle.loads(pickle.dumps(like))
    assert back._host is None and back(X[0]) == like(X[0])
    fixed = MassActionODELogLike(**_robertson_kw(reactions=[({0: 1}, {1: 1}, 0.04), ({1: 2}, {1: 1, 2: 1}, 0), ({1: 1, 2: 1}, {0: 1, 2: 1}, 1)]))
    assert fixed.d == 2 and np.isfinite(fixed(NW.ROB.NOMINAL[1:]))
    lin = MassActionODELogLike(**_robertson_kw(rate_scale="linear"))
    assert np.isfinite(lin(10.0 ** NW.ROB.NOMINAL))


def test_kernel_cache_refuses_a_fallback_directory_others_can_write(tmp_path, monkeypatch):
    import tempfile
    monkeypatch.delenv("DREAMZS_KERNEL_CACHE", raising=False)
    (tmp_path / "file").write_text("")
    monkeypatch.setenv("HOME", str(tmp_path / "file" / "home"))             # ~/.cache cannot be created
    monkeypatch.setattr(tempfile, "tempdir", str(tmp_path))
    monkeypatch.setattr(LK._kernel_cache, "_FALLBACK_DIR", [])
    fallback = tmp_path / ("dreamzs_kernels_%d" % os.getuid())
    d = LK.kernel_cache_dir()
    assert d == str(fallback) and stat.S_IMODE(os.stat(d).st_mode) == 0o700
    os.chmod(d, 0o777)                                                      # world-writable: refused
    d2 = LK.kernel_cache_dir()
    assert d2 != str(fallback) and LK._kernel_cache._private_dir(d2) and os.path.dirname(d2) == str(tmp_path)
    os.chmod(d, 0o700)
    real = os.getuid()
    monkeypatch.setattr(os, "getuid", lambda: real + 1)                     # a directory of another user: refused
    os.mkdir(tmp_path / ("dreamzs_kernels_%d" % (real + 1)), 0o700)
    d3 = LK.kernel_cache_dir()
    assert d3 != str(tmp_path / ("dreamzs_kernels_%d" % (real + 1)))
    monkeypatch.setattr(os, "getuid", lambda: real)
    monkeypatch.setenv("DREAMZS_KERNEL_CACHE", str(tmp_path / "explicit"))  # an explicit cache is used as given
    assert LK.kernel_cache_dir() == str(tmp_path / "explicit")
