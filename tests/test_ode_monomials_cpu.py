"""likelihoods.Monomial in MassActionODELogLike without a GPU: a monomial of one parameter is the bare index to the byte; rate constants,
start amounts, scales and constraints as monomials agree with a likelihood made of scipy's Radau and norm.logpdf alone; where the
constraints' term goes (condition 0, and nowhere else); failures are -inf; construction, ndim and pickling; the source of a network
without monomials is what it was on the commit before, and the four new networks cross-compile for gfx950 without scratch."""
import hashlib
import pickle
import subprocess

import numpy as np
import pytest

from pydream_amd import likelihoods as LK
from pydream_amd.likelihoods import MassActionODELogLike, Monomial

from . import ode_condition_networks as CN
from . import ode_monomial_networks as MN
from . import ode_networks as NW
from . import ode_wide_networks as W
from .ode_support import READELF, notes


# ---------------------------------------------------------------------------------------------------- the value object
def test_monomial_is_an_immutable_value():
    m = Monomial({3: 1, 1: -0.5}, 0.25)
    assert m.exponents == ((1, -0.5), (3, 1.0)) and m.log10_factor == 0.25 and m.indices == (1, 3)
    assert m == Monomial({1: -0.5, 3: 1.0}, 0.25) and hash(m) == hash(Monomial({1: -0.5, 3: 1.0}, 0.25)) and len({m, Monomial({1: -0.5, 3: 1}, 0.25)}) == 1
    assert m != Monomial({1: -0.5, 3: 1}) and m != Monomial({1: -0.5}, 0.25) and m != 3 and Monomial({0: 1}).log10_factor == 0.0
    back = pickle.loads(pickle.dumps(m))
    assert back == m and hash(back) == hash(m) and "Monomial" in repr(m)
    with pytest.raises(AttributeError):
        m.log10_factor = 1.0
    with pytest.raises(AttributeError):
        m.other = 1.0
    x = np.array([0.0, 0.4, 0.0, -0.3])
    assert abs(m.value(x) - 10.0 ** (0.25 - 0.5 * 0.4 - 0.3)) < 1e-15
    for bad in ({}, None, [1, 2], {0: 0.0}, {0: np.nan}, {0: np.inf}, {-1: 1.0}, {0.5: 1.0}, {True: 1.0}, {0: True}, {0: "1"}):
        with pytest.raises(ValueError, match="MassActionODELogLike: a Monomial's"):
            Monomial(bad)
    for bad in (np.nan, np.inf, "0", None, True):
        with pytest.raises(ValueError, match="MassActionODELogLike: a Monomial's log10_factor must be finite"):
            Monomial({0: 1}, bad)


# ---------------------------------------------------------------------------------------------------- 1. Monomial({i: 1}) is the bare index i
def _with_unit_monomials(like):
    rx = [(a, b, Monomial({r: 1}) if isinstance(r, int) else r) for a, b, r in like.reactions]
    return MassActionODELogLike(like.n_species, rx, like.y0, like.t, like.observables, like.data, like.sd, lanes_per_point=like.lanes_per_point,
                                max_steps=like.max_steps)


@pytest.mark.parametrize("name", ["mm", "chain8", "enzyme13@16"])
def test_a_monomial_of_one_parameter_gives_the_bare_index_s_bytes(name):
    make, nom, width = {"mm": (NW.michaelis_menten, NW.MM_NOMINAL, 3.0), "chain8": (NW.chain8, NW.CHAIN_NOMINAL, 3.0),
                        "enzyme13@16": (W.enzyme13, W.ENZ.NOMINAL, 1.0)}[name]
    bare = make()
    mono = _with_unit_monomials(bare)
    assert "MONOMIALS" in mono.source() and "MONOMIALS" not in bare.source() and mono.d == bare.d
    X = NW.box_points(nom, 200, 5, width=width)
    (lb, sb), (lm, sm) = bare.batch(X, return_steps=True), mono.batch(X, return_steps=True)
    print(name, "finite", int(np.isfinite(lb).sum()), "of 200; steps", int(sb.sum()))
    assert np.isfinite(lb).sum() > 100
    assert lm.tobytes() == lb.tobytes() and sm.tobytes() == sb.tobytes()
    assert mono.simulate(X).tobytes() == bare.simulate(X).tobytes()


# ---------------------------------------------------------------------------------------------------- 2. an independent reference
@pytest.mark.parametrize("name,n", [("mm_kd", 20), ("enzyme13_m", 10)])
def test_the_value_agrees_with_an_independent_radau_likelihood(name, n):
    """|value - reference| <= 1e-6 sum |terms| (the bound of the existing Radau tests); the reference: tests/ode_reference.radau at rtol
    1e-10, rate constants, starts and scales as numpy's 10.0**(c + sum e x), norm.logpdf for data and constraints."""
    like, _ = MN.build(name)
    spec, data, sd = MN.spec_and_data(name)
    X = NW.box_points(spec["nominal"], n, 13, width=1.0)
    got = like.batch(X)
    assert np.all(np.isfinite(got))
    for x, value in zip(X, got):
        total, magnitude = MN.reference_loglike(spec, data, sd, x)
        print("%.9g %.9g %.3g" % (value, total, abs(value - total) / magnitude))
        assert abs(value - total) <= 1e-6 * magnitude, (x, value, total)


# ---------------------------------------------------------------------------------------------------- 3. where the terms go
@pytest.fixture(scope="module")
def mm_kd_points():
    return NW.box_points(MN.nominal("mm_kd"), 300, 21, width=1.0, outside=0.05)


def _check_terms(name, X, **kw):
    multi, single = MN.build(name, **kw)
    C = len(multi.conditions)
    terms = multi.batch_conditions(X)
    assert terms.shape == (len(X), C)
    with_g = single(0).batch(X)
    plain = np.stack([single(c, constraints=False).batch(X) for c in range(C)], axis=1)
    assert terms[:, 0].tobytes() == with_g.tobytes()
    for c in range(1, C):
        assert terms[:, c].tobytes() == plain[:, c].tobytes(), c
    total, steps = multi.batch(X, return_steps=True)
    assert total.tobytes() == CN.left_to_right(terms).tobytes()
    assert np.array_equal(steps, sum(single(c).batch(X, return_steps=True)[1] for c in range(C)))
    g = multi.constraint_terms(X)
    assert np.all(np.isfinite(g)) and (plain[:, 0] + g).tobytes() == terms[:, 0].tobytes()
    assert g.tobytes() == single(0).constraint_terms(X).tobytes() and not np.any(single(1, constraints=False).constraint_terms(X))
    spec = MN.spec_and_data(name)[0]
    for x, gx in zip(X[:50], g):                     # g = G0 + acc as specified, in numpy (10.0**s for dexp: a few ulp of the monomial)
        G0, acc, size = sum(-np.log(s) - 0.5 * np.log(2 * np.pi) for _, _, s in spec["constraints"]), 0.0, 0.0
        for m, loc, s in spec["constraints"]:
            r = (MN.mono_value(m, x) - loc) / s
            acc, size = acc - 0.5 * r * r, size + abs(r) * MN.mono_value(m, x) / s
        assert abs(gx - (G0 + acc)) <= 1e-13 * (abs(G0) + abs(acc) + size)
    return multi, terms == -np.inf


def test_constraints_go_to_condition_0_and_the_sum_is_left_to_right(mm_kd_points):
    multi, failed = _check_terms("mm_kd", mm_kd_points)
    assert not failed.any()
    sim = multi.simulate(mm_kd_points[:40])
    assert sim.shape == (40, 3, 20, 2) and np.all(sim[:, 2, :, 1] == 0.0) and np.all(sim[:, :2, :, 1] > 0.0)      # no enzyme: no product
    spec, _, _ = MN.spec_and_data("mm_kd")
    x = spec["nominal"]                                   # simulate returns what is compared with the data: scale * observable
    want = np.stack([MN.radau_observed(spec, c, x).T for c in range(3)])
    assert np.max(np.abs(multi.simulate(x)[0] - want)) < 1e-5


@pytest.mark.parametrize("name", ["mm_kd", "mm_kd_doses"])
def test_constraints_where_a_step_cap_fails_some_conditions(name, mm_kd_points):
    """max_steps=60.  mm_kd's last condition has no enzyme: nothing happens and it never runs out of steps, so no point fails in all
    three; mm_kd_doses (the enzyme in all three) has points of every kind."""
    _, failed = _check_terms(name, mm_kd_points, max_steps=60)
    count = failed.sum(axis=1)
    print("fail in all / some / no conditions:", int(np.sum(count == 3)), int(np.sum((count > 0) & (count < 3))), int(np.sum(count == 0)))
    assert np.any((count > 0) & (count < 3)) and np.any(count == 0)
    assert np.any(count == 3) if name == "mm_kd_doses" else not failed[:, 2].any()


def test_the_lane_group_path():
    X = NW.box_points(MN.nominal("enzyme13_m"), 40, 21, width=1.0)
    _, failed = _check_terms("enzyme13_m", X)
    assert not failed.any()


def test_a_scale_of_plain_ones_changes_no_byte():
    X = NW.box_points(NW.MM_NOMINAL, 50, 3)
    a = NW.michaelis_menten()
    b = NW.michaelis_menten(scale=[1.0, 1.0])
    assert b.scale == [1.0, 1.0] and a.source() == b.source() and a.batch(X).tobytes() == b.batch(X).tobytes()
    assert a.simulate(X).tobytes() == b.simulate(X).tobytes() and not np.any(a.constraint_terms(X))
    c = NW.michaelis_menten(scale=[1.0, 2.0])             # a plain factor scales the simulation exactly
    sa, sc = a.simulate(X), c.simulate(X)
    assert np.array_equal(sc[..., 0], sa[..., 0], equal_nan=True) and np.array_equal(sc[..., 1], 2.0 * sa[..., 1], equal_nan=True)


# ---------------------------------------------------------------------------------------------------- 4. failures are -inf, never NaN
def _mm(**kw):
    data = np.ones((2, 20))
    args = dict(n_species=4, reactions=NW.MM_REACTIONS, y0=NW.MM_Y0, t=NW.MM_T, observables=CN.MM_OBSERVABLES, data=data, sd=0.1)
    args.update(kw)
    return MassActionODELogLike(**args)


@pytest.mark.parametrize("where", ["y0", "scale", "constraint", "rate"])
def test_a_coordinate_or_a_monomial_that_is_not_finite(where):
    m = Monomial({3: 1})
    like = {"y0": lambda: _mm(y0=[m, 2.0, 0.0, 0.0]), "scale": lambda: _mm(scale=[1.0, m]), "constraint": lambda: _mm(constraints=[(m, 1.0, 1.0)]),
            "rate": lambda: _mm(reactions=NW.MM_REACTIONS[:2] + [({2: 1}, {0: 1, 3: 1}, Monomial({2: 1, 3: 1}))])}[where]()
    assert like.d == 4
    conds = {"y0": lambda: _mm(y0=None, conditions=[dict(y0=[m, 2.0, 0.0, 0.0]), dict(y0=[m, 1.0, 0.0, 0.0])]),
             "scale": lambda: _mm(scale=[1.0, m], conditions=[{}, {}]), "constraint": lambda: _mm(constraints=[(m, 1.0, 1.0)], conditions=[{}, {}]),
             "rate": lambda: _mm(reactions=like.reactions, conditions=[{}, {}])}[where]()
    x = np.r_[NW.MM_NOMINAL, 0.0]
    X = np.stack([x] * 6)
    X[1:, 3] = [np.nan, np.inf, -np.inf, 400.0, -400.0]       # (the last: an underflow to 0 is a value like any other)
    for obj in (like, conds):
        v, g = obj.batch(X), obj.constraint_terms(X)
        print(where, v, g)
        assert not np.any(np.isnan(v)) and not np.any(np.isnan(g))
        assert np.isfinite(v[0]) and np.all(v[1:5] == -np.inf) and np.all(g[1:5] == -np.inf) and np.isfinite(g[0])
        assert v[5] != np.inf and (np.isfinite(v[5]) or where == "constraint" or where == "y0")
        assert np.all(np.isnan(obj.simulate(X)[1:5])) and not np.any(np.isnan(obj.simulate(X)[0]))
    terms = conds.batch_conditions(X)
    assert not np.any(np.isnan(terms)) and np.all(terms[1:5] == -np.inf)
    assert np.all(np.isnan(like.fixed_steps(X[1], 1.0, 4))) and np.all(np.isfinite(like.fixed_steps(X[0], 1.0, 4)))


def test_a_starved_integration_with_constraints_is_minus_infinity():
    X = NW.box_points(MN.nominal("mm_kd"), 30, 2, width=1.0)
    multi, single = MN.build("mm_kd", max_steps=3)
    for obj in (multi, single(0), MN.build("dense8_m", max_steps=1)[0]):
        Y = X if obj.d == 5 else NW.box_points(MN.nominal("dense8_m"), 30, 2, width=1.0)
        v = obj.batch(Y)
        assert np.all(v == -np.inf) and np.all(np.isfinite(obj.constraint_terms(Y)))
    assert np.all(multi.batch_conditions(X) == -np.inf)


# ---------------------------------------------------------------------------------------------------- 5. construction and pickling
def test_construction_errors_and_ndim():
    m, other = Monomial({3: 1}), Monomial({3: 1}, 0.5)
    ok = _mm(y0=[m, 2.0, 0.0, 0.0], scale=[1.0, Monomial({6: 2})], constraints=[(Monomial({1: 1, 5: -1}), 1.0, 0.1)])
    assert ok.d == 7 and ok.y0_monomials == {0: m} and np.isnan(ok.y0[0]) and ok.y0[1] == 2.0
    assert _mm(reactions=NW.MM_REACTIONS[:2] + [({2: 1}, {0: 1, 3: 1}, Monomial({9: 1, 2: 1}))]).d == 10
    assert _mm(scale=[1.0, m], ndim=8).d == 8
    for kw, msg in [(dict(scale=[1.0, m], ndim=3), "parameter index 3 is not < ndim = 3"),
                    (dict(constraints=[(Monomial({7: 1}), 1.0, 1.0)], ndim=7), "parameter index 7 is not < ndim = 7"),
                    (dict(y0=[m, 2.0, 0.0]), "y0 must hold 4"), (dict(y0=[m, -2.0, 0.0, 0.0]), "y0 must hold 4"), (dict(y0=[m, np.nan, 0.0, 0.0]), "y0 must hold 4"),
                    (dict(scale=[1.0]), "scale must hold O = 2"), (dict(scale=[1.0, np.inf]), "scale must hold O = 2"), (dict(scale=[1.0, "a"]), "scale must hold O = 2"),
                    (dict(scale=[1.0, 1.0, 1.0]), "scale must hold O = 2"),
                    (dict(constraints=[(1.0, 1.0, 1.0)]), r"constraint 0 must be \(Monomial, loc, sd\)"), (dict(constraints=[(m, 1.0)]), "constraint 0 must be"),
                    (dict(constraints=[(m, 1.0, 1.0), m]), "constraint 1 must be"),
                    (dict(constraints=[(m, 1.0, 0.0)]), "constraint 0: loc must be finite and sd finite and > 0"), (dict(constraints=[(m, 1.0, -1.0)]), "constraint 0: loc"),
                    (dict(constraints=[(m, np.nan, 1.0)]), "constraint 0: loc"), (dict(constraints=[(m, 1.0, np.inf)]), "constraint 0: loc"),
                    (dict(constraints=[(m, 1.0, 1.0)] * 17), r"at most 16 constraints are supported \(got 17\)"),
                    (dict(reactions=NW.MM_REACTIONS[:2] + [({2: 1}, {0: 1, 3: 1}, "k")]), "reaction 2: the rate is a parameter index"),
                    (dict(y0=[m, 2.0, 0.0, 0.0], conditions=[{}, dict(y0=[other, 1.0, 0.0, 0.0])]), r"condition 1: y0\[0\] is .* one Monomial per species"),
                    (dict(y0=None, conditions=[dict(y0=[m, 1.0, 0.0, 0.0]), dict(y0=[0.0, 1.0, 0.0, 0.0]), dict(y0=[other, 1.0, 0.0, 0.0])]),
                     r"condition 2: y0\[0\] is")]:
        with pytest.raises(ValueError, match="MassActionODELogLike: .*" + msg):
            _mm(**kw)
    assert LK.ODE_MAX_CONSTRAINTS == 16 and len(_mm(constraints=[(m, 1.0, 1.0)] * 16).constraints) == 16
    two = _mm(y0=None, conditions=[dict(y0=[m, 1.0, 0.0, 0.0]), dict(y0=[0.0, 1.0, Monomial({4: 1}), 0.0]), dict(y0=[m, 2.0, Monomial({4: 1}), 0.0])])
    assert two.d == 5 and two.y0_monomials == {0: m, 2: Monomial({4: 1})}
    assert [np.flatnonzero(np.isnan(c["y0"])).tolist() for c in two.conditions] == [[0], [2], [0, 2]]


def test_the_meaning_does_not_depend_on_rate_scale():
    x = np.r_[NW.MM_NOMINAL, -0.3, 0.2]
    kw = dict(y0=[Monomial({3: 1}), 2.0, 0.0, 0.0], scale=[1.0, Monomial({4: 1})], constraints=[(Monomial({3: 1, 4: 1}), 1.0, 0.5)])
    log = _mm(**kw)
    lin = _mm(rate_scale="linear", **kw)
    fixed = _mm(reactions=[(a, b, float(10.0 ** x[r])) for a, b, r in NW.MM_REACTIONS], ndim=5, **kw)
    assert np.isfinite(log(x)) and abs(log(x) - fixed(x)) <= 1e-9 * abs(log(x))
    assert lin(np.r_[10.0 ** NW.MM_NOMINAL, -0.3, 0.2]) == fixed(x) and lin.constraint_terms(x).tobytes() == log.constraint_terms(x).tobytes()


def test_pickle_round_trip():
    X = NW.box_points(MN.nominal("mm_kd"), 6, 4, width=1.0)
    for name in ("mm_kd", "dense8_m"):
        like, _ = MN.build(name)
        Y = X if like.d == 5 else NW.box_points(MN.nominal(name), 6, 4, width=1.0)
        back = pickle.loads(pickle.dumps(like))
        assert back._host is None and back.source() == like.source() and back.data_block().tobytes() == like.data_block().tobytes()
        assert back.batch(Y).tobytes() == like.batch(Y).tobytes() and back.constraint_terms(Y).tobytes() == like.constraint_terms(Y).tobytes()
        assert back.constraints == like.constraints and back.scale == like.scale and back.y0_monomials == like.y0_monomials
    old = NW.michaelis_menten()
    for key in ("scale", "constraints", "y0_monomials"):  # an object pickled before the keywords existed
        del old.__dict__[key]
    back = pickle.loads(pickle.dumps(old))
    assert back.source() == NW.michaelis_menten().source() and back.batch(NW.MM_NOMINAL).tobytes() == NW.michaelis_menten().batch(NW.MM_NOMINAL).tobytes()


# ---------------------------------------------------------------------------------------------------- 6. unchanged source, cross-compiled kernels
# sha256 of source() on the commit before Monomial existed, from these same constructors
PARENT_SOURCE_SHA256 = {
    "robertson": "c4fd92120c3b297f5ca95cc5badd01f82fb4e13702022f116b6aa3a583f6be0e",
    "mm": "6d00d6a6fca814cf3e78bbb94833510faea553e0a15e8c10a298484cf7625ceb",
    "chain8": "7c21c344e8c175a67e16fed278d7b683bdd838ae0231a090733fec458e45c951",
    "enzyme13@16": "0aa13e4724688b1327784e38675d9c71e37520f6bfef3fb95eef62929af3b1f6",
    "chain32@32": "21746d67757913646ba884447bf66fb3a2f51064cd1323f94c2fcc26e9f3e804",
    "mm x 3": "2b2dad4e814f035f72ab52019a62c04c99461636d7ec7165e30b3b37559edfad",
    "enzyme13@16 x 3": "d14b4d145307bbd558381313b8e909fe78c0d9a7e71357b1c39dd40bfa5c5061",
}


def test_a_network_without_monomials_generates_the_source_it_always_did():
    made = {"robertson": NW.robertson(), "mm": NW.michaelis_menten(), "chain8": NW.chain8(), "enzyme13@16": W.enzyme13(), "chain32@32": W.chain(32, 32),
            "mm x 3": CN.mm()[0], "enzyme13@16 x 3": CN.enzyme13()[0]}
    for name, like in made.items():
        assert hashlib.sha256(like.source().encode()).hexdigest() == PARENT_SOURCE_SHA256[name], name
        assert "MONOMIALS" not in like.source()
    mm = NW.michaelis_menten(scale=None, constraints=None)
    assert hashlib.sha256(mm.source().encode()).hexdigest() == PARENT_SOURCE_SHA256["mm"] and mm.constraints == () and mm.y0_monomials == {}


def _dense8_plain():
    return W.dense_network(8, 24, 1)


# name -> (the monomial-free counterpart, the kernel)
CROSS = {"mm_kd": (lambda: CN.mm()[0], "dz_ode"), "enzyme13_m": (lambda: CN.enzyme13()[0], "dz_ode_group"),
         "chain17_m": (lambda: CN.chain(17, 32, (1.0, 2.0))[0], "dz_ode_group"), "dense8_m": (_dense8_plain, "dz_ode")}


@pytest.mark.parametrize("name", list(CROSS))
def test_kernels_cross_compile_for_gfx950_without_scratch(name, tmp_path, monkeypatch):
    """Both entries of every network: the items kernel (or, for dense8_m, the only one) and the single-experiment kernel of condition 0."""
    monkeypatch.setenv("DREAMZS_KERNEL_CACHE", str(tmp_path))
    like, single = MN.build(name)
    plain, stem = CROSS[name]
    builds = [(like, stem + ("_item_batch" if like.conditions else "_batch"))] + ([(single(0), stem + "_batch")] if like.conditions else [])
    counterpart = notes(plain().code_object())
    for obj, kernel in builds:
        path = obj.code_object()
        assert open(path, "rb").read(4) == b"\x7fELF" and obj.code_object() == path
        syms = subprocess.run([READELF, "-s", path], capture_output=True, text=True).stdout
        assert kernel + ".kd" in syms
        n = notes(path)
        print("%s %s: %d VGPRs (%d of them AGPRs), static LDS %d B, scratch %d; without monomials (%s): %d VGPRs (%d AGPRs), scratch %d"
              % (name, kernel, n["vgpr"], n["agpr"], n["lds"], n["scratch"], "the items kernel" if plain().conditions else "single",
                 counterpart["vgpr"], counterpart["agpr"], counterpart["scratch"]))
        assert n["scratch"] == 0
