"""MassActionODELogLike(conditions=[...]) without a GPU: every condition's term has the bytes of the single-condition object, the point's
value those of the left-to-right sum (also under a step cap that fails some conditions of a point and not others), on the one-lane and
the lane-group path; the sum agrees with an independent scipy Radau likelihood; construction checks, fallbacks, pickling and shapes; and
the item kernels cross-compile for gfx950 without scratch."""
import pickle
import subprocess

import numpy as np
import pytest

from pydream_amd import likelihoods as LK
from pydream_amd.likelihoods import MassActionODELogLike

from . import ode_condition_networks as CN
from . import ode_networks as NW
from . import ode_reference as REF
from . import ode_wide_networks as W
from .ode_support import READELF, notes


def _check_terms_and_sum(multi, single, X, **kw):
    """batch_conditions' columns against the single-condition objects, batch against their left-to-right sum; returns [n, C] failed flags"""
    C = len(multi.conditions)
    terms = multi.batch_conditions(X)
    assert terms.shape == (len(X), C)
    alone = np.stack([single(c, **kw).batch(X) for c in range(C)], axis=1)
    for c in range(C):
        assert terms[:, c].tobytes() == alone[:, c].tobytes(), c
    total, steps = multi.batch(X, return_steps=True)
    assert total.tobytes() == CN.left_to_right(alone).tobytes()
    assert np.array_equal(steps, sum(single(c, **kw).batch(X, return_steps=True)[1] for c in range(C)))
    assert np.array_equal(total == -np.inf, np.any(alone == -np.inf, axis=1))
    return alone == -np.inf


@pytest.fixture(scope="module")
def mm_points():
    return NW.box_points(NW.MM_NOMINAL, 1027, 21, width=1.0, outside=0.05)


def test_each_condition_has_the_single_experiments_bytes_and_the_point_their_sum(mm_points):
    multi, single = CN.mm()
    failed = _check_terms_and_sum(multi, single, mm_points)
    assert not failed.any()


def test_a_step_cap_that_fails_some_conditions_of_a_point(mm_points):
    """max_steps=60: of the 1027 points 124 fail in all three conditions, 575 in some, 328 in none (the single-condition host build)."""
    multi, single = CN.mm(max_steps=60)
    failed = _check_terms_and_sum(multi, single, mm_points).sum(axis=1)
    groups = (int(np.sum(failed == 3)), int(np.sum((failed > 0) & (failed < 3))), int(np.sum(failed == 0)))
    print("fail in all / some / no conditions:", groups)
    assert min(groups) > 0


@pytest.mark.parametrize("max_steps", [500, 75])
def test_the_lane_group_path(max_steps):
    """enzyme13 with 16 lanes per point, the substrate A at 0.5, 1 and 2 times its amount; 75 steps per interval starve about half."""
    multi, single = CN.enzyme13(max_steps=max_steps)
    X = NW.box_points(W.ENZ.NOMINAL, 259, 21, width=1.0)
    failed = _check_terms_and_sum(multi, single, X)
    print("enzyme13 x 3 at max_steps %d: -inf terms per condition %s" % (max_steps, failed.sum(axis=0)))
    assert failed.any() == (max_steps < 500)


def test_the_sum_agrees_with_an_independent_radau_likelihood():
    """20 box points: |sum - reference| <= 1e-6 of the magnitude of the sum's terms (the bound of the existing Radau tests), the
    reference being scipy's Radau on tests/ode_reference.py's right-hand side from every condition's start."""
    from scipy.stats import norm
    multi, _ = CN.mm()
    X = NW.box_points(NW.MM_NOMINAL, 20, 13, width=1.0)
    got = multi.batch(X)
    obs = np.asarray(CN.MM_OBSERVABLES, dtype=float)
    for x, value in zip(X, got):
        total = magnitude = 0.0
        for cond in multi.conditions:
            y = REF.radau(4, NW.MM_REACTIONS, REF.rate_constants(NW.MM_REACTIONS, x, "log10"), cond["y0"], NW.MM_T, rtol=1e-10, atol=1e-14)
            seen = np.isfinite(cond["data"])
            terms = norm(loc=cond["data"][seen], scale=cond["sd"][seen]).logpdf((y @ obs.T).T[seen])
            total, magnitude = total + float(np.sum(terms)), magnitude + float(np.sum(np.abs(terms)))
        print("%.9g %.9g %.3g" % (value, total, abs(value - total) / magnitude))
        assert abs(value - total) <= 1e-6 * magnitude, (x, value, total)


def _mm_kw(**over):
    data = np.ones((2, 20))
    kw = dict(n_species=4, reactions=NW.MM_REACTIONS, y0=NW.MM_Y0, t=NW.MM_T, observables=CN.MM_OBSERVABLES, data=data, sd=0.1)
    kw.update(over)
    return kw


def test_fallbacks_and_top_level_none():
    data2 = np.full((2, 20), 2.0)
    like = MassActionODELogLike(**_mm_kw(conditions=[{}, {"y0": [0.5, 8.0, 0, 0]}, {"data": data2}, {"sd": 0.3}, {"y0": [1, 1, 1, 1], "data": data2, "sd": 0.2}]))
    want = [(NW.MM_Y0, 1.0, 0.1), ([0.5, 8.0, 0, 0], 1.0, 0.1), (NW.MM_Y0, 2.0, 0.1), (NW.MM_Y0, 1.0, 0.3), ([1, 1, 1, 1], 2.0, 0.2)]
    assert len(like.conditions) == 5
    for cond, (y0, d, s) in zip(like.conditions, want):
        assert np.array_equal(cond["y0"], np.asarray(y0, dtype=float))
        assert np.array_equal(cond["data"], np.full((2, 20), d)) and np.array_equal(cond["sd"], np.full((2, 20), s))
    x = NW.MM_NOMINAL
    for c, (y0, d, s) in enumerate(want):
        alone = MassActionODELogLike(**_mm_kw(y0=y0, data=np.full((2, 20), d), sd=s))
        assert like.batch_conditions(x)[0, c] == alone(x)
        assert np.array_equal(like.fixed_steps(x, 1.0, 8, condition=c), alone.fixed_steps(x, 1.0, 8))
    every = [dict(y0=NW.MM_Y0, data=data2, sd=0.2)] * 2
    none = MassActionODELogLike(**_mm_kw(y0=None, data=None, sd=None, conditions=every))
    assert none.y0 is None and none.data is None and none.sd is None and np.isfinite(none(x))
    with pytest.raises(ValueError, match="condition 1 has no sd"):
        MassActionODELogLike(**_mm_kw(sd=None, conditions=[{"sd": 0.1}, {}]))
    with pytest.raises(ValueError, match="condition 0 has no y0"):
        MassActionODELogLike(**_mm_kw(y0=None, conditions=[{}]))
    with pytest.raises(ValueError, match="only when every one of the conditions"):
        MassActionODELogLike(**_mm_kw(y0=None))
    with pytest.raises(ValueError, match="batch_conditions needs"):
        MassActionODELogLike(**_mm_kw()).batch_conditions(x)


def test_validation_errors_name_the_condition_and_the_limit_is_enforced():
    bad_data = np.ones((2, 20)); bad_data[1, 4] = np.inf
    for cond, msg in [({"y0": [0.5, -1.0, 0, 0]}, "condition 2: y0 must hold 4 finite, non-negative"),
                      ({"y0": [0.5, 1.0, 0]}, "condition 2: y0 must hold 4"),
                      ({"y0": [0.5, np.nan, 0, 0]}, "condition 2: y0 must hold 4"),
                      ({"data": np.ones((2, 19))}, "condition 2: data and sd must be O x T = 2 x 20"),
                      ({"sd": np.ones((3, 20))}, "condition 2: data and sd must be O x T = 2 x 20"),
                      ({"data": bad_data}, "condition 2: data must be finite or NaN"),
                      ({"sd": 0.0}, "condition 2: data must be finite or NaN .* sd finite and > 0"),
                      ({"sd": -np.ones((2, 20))}, "condition 2: data must be finite or NaN"),
                      ({"dose": 1.0}, "condition 2 must be a mapping with the keys"),
                      ([1.0, 2.0], "condition 2 must be a mapping")]:
        with pytest.raises(ValueError, match=msg):
            MassActionODELogLike(**_mm_kw(conditions=[{}, {}, cond]))
    unobserved = np.ones((2, 20)); unobserved[0, 5] = np.nan
    sd = np.ones((2, 20)); sd[0, 5] = -1.0                  # (sd is only looked at where the data are observed)
    MassActionODELogLike(**_mm_kw(conditions=[{"data": unobserved, "sd": sd}]))
    limit = LK.ODE_MAX_CONDITIONS
    assert limit >= 64 and LK.ODE_GROUP_LIMITS["conditions"] == limit
    for lanes in (1, 16):
        MassActionODELogLike(**_mm_kw(conditions=[{}] * limit, lanes_per_point=lanes))
        for n in (0, limit + 1):
            with pytest.raises(ValueError, match=r"1\.\.%d conditions are supported \(got %d\)" % (limit, n)):
                MassActionODELogLike(**_mm_kw(conditions=[{}] * n, lanes_per_point=lanes))


def test_pickle_call_simulate_and_the_data_block(mm_points):
    multi, single = CN.mm()
    X = mm_points[:6]
    back = pickle.loads(pickle.dumps(multi))
    assert back._host is None and len(back.conditions) == 3 and back.batch(X).tobytes() == multi.batch(X).tobytes()
    assert multi(X[0]) == multi.batch(X)[0] and isinstance(multi(X[0]), float)
    sim = multi.simulate(X)
    assert sim.shape == (6, 3, 20, 2)
    for c in range(3):
        assert sim[:, c].tobytes() == single(c).simulate(X).tobytes()
    few, few_single = CN.mm(max_steps=60)
    sim, terms = few.simulate(mm_points[:200]), few.batch_conditions(mm_points[:200])
    assert np.array_equal(np.isnan(sim).all(axis=(2, 3)), terms == -np.inf) and np.array_equal(np.isnan(sim).any(axis=(2, 3)), terms == -np.inf)
    blk = multi.data_block()
    stride = len(single(0).data_block())
    assert blk[0] == 3 and blk[1] == stride and len(blk) == 2 + 3 * stride
    for c in range(3):
        assert blk[2 + c * stride: 2 + (c + 1) * stride].tobytes() == single(c).data_block().tobytes()
        assert multi.condition_block(c).tobytes() == single(c).data_block().tobytes()
    assert "DZODE_ITEM_ENTRIES(Net)" in multi.source() and multi.source().replace("DZODE_ITEM_ENTRIES", "DZODE_ENTRIES") == single(0).source()
    grp, grp_single = CN.enzyme13()
    assert grp.source().replace("DZODE_GROUP_ITEM_ENTRIES", "DZODE_GROUP_ENTRIES") == grp_single(0).source()


def test_without_conditions_source_and_data_block_are_what_they_were():
    """conditions=None is the object built without the keyword: source, data block, values (tests/test_ode_group_cpu.py and
    tests/test_ode_grammar_cpu.py pin those against the commits before)."""
    for lanes, kw in ((1, _mm_kw()), (16, _mm_kw(lanes_per_point=16))):
        a, b = MassActionODELogLike(**kw), MassActionODELogLike(conditions=None, **kw)
        assert a.conditions is None and b.conditions is None
        assert a.source() == b.source() and a.data_block().tobytes() == b.data_block().tobytes()
        assert ("DZODE_ENTRIES(Net)" if lanes == 1 else "DZODE_GROUP_ENTRIES(Net, 16)") in a.source() and "ITEM" not in a.source()
        assert len(a.data_block()) == 6 + 4 + 20 + 2 * 40
    old = MassActionODELogLike(**_mm_kw())
    del old.__dict__["conditions"]                         # an object pickled before the keyword existed
    assert pickle.loads(pickle.dumps(old)).data_block().tobytes() == MassActionODELogLike(**_mm_kw()).data_block().tobytes()


CROSS = {"mm x 3": (lambda: CN.mm(), "dz_ode_item_batch"),
         "chain8 x 5": (lambda: CN.chain(8, 1, (1.0, 0.5, 2.0, 0.25, 4.0)), "dz_ode_item_batch"),
         "enzyme13@16 x 3": (lambda: CN.enzyme13(), "dz_ode_group_item_batch"),
         "chain32@32 x 2": (lambda: CN.chain(32, 32, (1.0, 2.0)), "dz_ode_group_item_batch")}


@pytest.mark.parametrize("name", list(CROSS))
def test_item_kernels_cross_compile_for_gfx950_without_scratch(name, tmp_path, monkeypatch):
    monkeypatch.setenv("DREAMZS_KERNEL_CACHE", str(tmp_path))
    make, kernel = CROSS[name]
    multi, single = make()
    path = multi.code_object()
    assert open(path, "rb").read(4) == b"\x7fELF" and multi.code_object() == path
    syms = subprocess.run([READELF, "-s", path], capture_output=True, text=True).stdout
    assert kernel + ".kd" in syms and kernel.replace("_item", "") + ".kd" not in syms
    n, one = notes(path), notes(single(0).code_object())
    print("%s: %d VGPRs (%d of them AGPRs), static LDS %d B, scratch %d; the single-condition build: %d VGPRs (%d AGPRs), scratch %d"
          % (name, n["vgpr"], n["agpr"], n["lds"], n["scratch"], one["vgpr"], one["agpr"], one["scratch"]))
    assert n["scratch"] == 0
    assert n["lds"] == one["lds"]
