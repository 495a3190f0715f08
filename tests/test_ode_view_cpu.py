"""MassActionODELogLike(conditions=[dict(params={i: target}), ...]), a view of the point per condition, without a GPU (csrc/dz_ode.h,
VIEWS): item c of the object has the bits of the object of condition c alone, made without "params", at the row V_c x -- in the four
shapes and for every kind of reader --; identities, non-finite coordinates, ndim, the validation errors, the rest of the surface, and
the host build's generated source in a stand-alone program under the address and undefined-behaviour sanitizers.

V_c X is computed here from the declared mappings by numpy indexing (ode_view_networks.viewed), not by the class, except in the test of
MassActionODELogLike.viewed itself."""
import os
import pickle
import subprocess

import numpy as np
import pytest

from pydream_amd.likelihoods import (ODE_MAX_VIEW_COORDINATES, MassActionODELogLike, Monomial, csrc_dir, posterior_predictive)

from . import ode_combined_networks as CB
from . import ode_condition_networks as CN
from . import ode_networks as NW
from . import ode_view_networks as VN

SHAPES = [("mm", 64), ("enzyme13", 64), ("chain17", 64), (VN.WAVE, 16)]


def _assert_items_are_the_single_objects(multi, single, maps, X, steady=False, noise=False):
    """terms, sum, simulate slices and steps (and resting states, noise values) of the object with views against single(c) at V_c X"""
    P, C = multi._view_size(), len(maps)
    terms, sim = multi.batch_conditions(X), multi.simulate(X)
    total, steps = multi.batch(X, return_steps=True)
    assert terms.shape == (len(X), C) and total.tobytes() == CN.left_to_right(terms).tobytes()
    want_steps = np.zeros(len(X), dtype=np.int64)
    for c in range(C):
        one, V = single(c), VN.viewed(maps, c, X, P)
        value, st = one.batch(V, return_steps=True)
        assert terms[:, c].tobytes() == value.tobytes(), c
        assert sim[:, c].tobytes() == one.simulate(V).tobytes(), c
        want_steps += st
        if steady:
            assert multi.steady_state(X)[:, c].tobytes() == one.steady_state(V).tobytes(), c
        if noise:
            assert multi.noise_values(X)[:, c].tobytes() == one.noise_values(V).tobytes(), c
    assert np.array_equal(steps, want_steps)
    return terms


def test_a_condition_may_carry_params():
    """(on the code before this key existed: the ValueError about a condition's keys)"""
    multi, _, maps = VN.basic("mm")
    assert [cond.get("params", {}) for cond in multi.conditions] == maps
    assert "VIEW = 5" in multi.source() and multi.d == 4


@pytest.mark.parametrize("name,n", SHAPES)
def test_host_items_equal_the_single_objects_at_the_viewed_rows(name, n):
    """each shape: a mapping to another coordinate, a fixed value and a formal index >= d"""
    multi, single, maps = VN.basic(name)
    targets = [t for m in maps for t in m.values()]
    assert any(isinstance(t, int) for t in targets) and any(isinstance(t, float) for t in targets)
    assert multi._view_size() - 1 >= multi.d and all(multi._view_size() - 1 in m for m in maps)        # the formal index
    terms = _assert_items_are_the_single_objects(multi, single, maps, VN.points(name, n, 31))
    assert np.all(np.isfinite(terms))


@pytest.mark.parametrize("lanes,n", [(1, 64), (16, 64), (32, 64), (64, 16)])
def test_every_kind_of_reader_goes_through_the_view(lanes, n):
    """a Monomial rate, a y0 Monomial, a Monomial scale, Noise sigma and rel, Hill Ks and input gains, each remapped in some condition;
    two conditions equilibrate, and their resting states follow the view"""
    multi, single, maps, case = VN.readers(lanes)
    assert set(case.features) == set(CB.FEATURES) and multi.d == VN.READER_D and multi._view_size() == CB.NDIM
    replaced = {i for m in maps for i, t in m.items() if t != i}
    assert replaced == {0, CB.P_K, CB.P_GAIN, CB.P_Y0, CB.P_SCALE, CB.P_SIGMA, CB.P_REL}
    X = VN.reader_points(lanes, n, 32)
    terms = _assert_items_are_the_single_objects(multi, single, maps, X, steady=True, noise=True)
    assert np.isfinite(terms).mean() > 0.9
    assert multi.noise_values(X).shape == (n, 3, len(case.observables), 2)
    assert VN.readers(lanes, view=False)[0].noise_values(X[:, :CB.NDIM]).shape == (n, len(case.observables), 2)
    # a resting state does depend on what the view replaces: the Hill K of condition 0 comes from coordinate 10
    Y = X.copy()
    Y[:, 10] += 0.3
    assert np.any(multi.steady_state(X)[:, 0] != multi.steady_state(Y)[:, 0])


@pytest.mark.parametrize("name,n", SHAPES)
def test_explicit_identities_give_the_bits_of_the_object_without_params(name, n):
    viewed, _, maps = VN.basic(name, identity=True)
    plain, _, _ = VN.basic(name, view=False, identity=True)
    assert "VIEW" in viewed.source() and "VIEW" not in plain.source() and viewed.d == plain.d
    X = VN.points(name, n, 33)[:, :plain.d]
    assert viewed.batch_conditions(X).tobytes() == plain.batch_conditions(X).tobytes()
    assert viewed.simulate(X).tobytes() == plain.simulate(X).tobytes()


def test_params_missing_none_or_empty_is_the_object_it_always_was():
    never, _ = CN.mm()
    for value in (None, {}):
        conds = [dict(cond, params=value) for cond in never.conditions]
        named = MassActionODELogLike(4, NW.MM_REACTIONS, None, NW.MM_T, CN.MM_OBSERVABLES, None, None, conditions=conds)
        assert named.source() == never.source() and named.data_block().tobytes() == never.data_block().tobytes()
        assert named._unit() == never._unit() and named.d == never.d
    mixed = MassActionODELogLike(4, NW.MM_REACTIONS, None, NW.MM_T, CN.MM_OBSERVABLES, None, None,
                                 conditions=[dict(never.conditions[0], params={1: 1})] + [dict(c) for c in never.conditions[1:]])
    block, P = mixed.data_block(), 3
    assert mixed.source() != never.source() and len(block) == len(never.data_block()) + 3 * 2 * P and block[1] == never.data_block()[1] + 2 * P
    stride = int(block[1])
    for c in range(3):                       # (every condition gets a table; without a mapping: the identity)
        assert block[2 + (c + 1) * stride - 2 * P:2 + (c + 1) * stride].tolist() == [0.0, 0.0, 1.0, 0.0, 2.0, 0.0]


def test_the_table_holds_the_pairs_of_the_contract():
    multi, _, maps = VN.basic("mm")
    block, stride, P = multi.data_block(), int(multi.data_block()[1]), 5
    tab = block[2 + 2 * stride - 2 * P:2 + 2 * stride].reshape(P, 2)          # condition 1: {4: -0.5, 0: 3}
    assert tab.tolist() == [[3.0, 0.0], [1.0, 0.0], [2.0, 0.0], [-1.0, 0.0], [-1.0, -0.5]]      # (index 3: nothing reads it)


@pytest.mark.parametrize("bad", [np.nan, np.inf])
def test_liveness_is_per_item(bad):
    """condition 1 replaces index 0 and reads coordinate 3 in its place; conditions 0 and 2 read coordinate 0"""
    multi, _, maps = VN.basic("mm")
    assert maps[1][0] == 3 and 0 not in maps[0] and 0 not in maps[2]
    X = VN.points("mm", 16, 34)
    Y = X.copy()
    Y[:, 0] = bad
    a, b = multi.batch_conditions(X), multi.batch_conditions(Y)
    assert np.all(b[:, 0] == -np.inf) and np.all(b[:, 2] == -np.inf) and np.all(np.isfinite(b[:, 1]))
    assert b[:, 1].tobytes() == a[:, 1].tobytes() and np.all(multi.batch(Y) == -np.inf)
    Y[:, 0] = -7.25                          # (anything else: condition 1's term does not move)
    assert multi.batch_conditions(Y)[:, 1].tobytes() == a[:, 1].tobytes()


def test_a_fixed_value_is_used_bit_for_bit():
    """v = 0.3 and its upper neighbour: a pair whose rate constants 10**v differ (dexp rounds many neighbours onto one constant, the
    mapping's own value among them; then nothing downstream can tell them apart)"""
    v = 0.3
    low, up = [[dict(m) for m in VN.mappings_of("mm")] for _ in range(2)]
    low[2][1], up[2][1] = v, float(np.nextafter(v, 1))
    X = VN.points("mm", 16, 35)
    (one, _, _), (two, _, _) = VN.basic("mm", maps=low), VN.basic("mm", maps=up)
    exp = one.host_library().dzode_exp
    assert exp(low[2][1] * 2.302585092994046) != exp(up[2][1] * 2.302585092994046)
    a, b = one.batch_conditions(X), two.batch_conditions(X)
    assert a[:, :2].tobytes() == b[:, :2].tobytes() and np.all(a[:, 2] != b[:, 2])


def test_ndim_covers_what_some_condition_reads_from_the_point():
    multi, _, maps = VN.basic("mm")
    assert multi._view_size() == 5 and multi.d == 4          # the formal index 4 is never read from the point; the target 3 is
    assert VN.basic("mm", ndim=4)[0].d == 4 and VN.basic("mm", ndim=6)[0].d == 6
    with pytest.raises(ValueError, match="parameter index 3 is not < ndim = 3"):
        VN.basic("mm", ndim=3)
    far = [dict(m) for m in maps]
    far[1][0] = 9                            # a target beyond the network's own indices
    assert VN.basic("mm", maps=far)[0].d == 10
    moved = [{4: 0.0, 2: 7}, {4: 0.0, 2: 7}, {4: 0.0, 2: 7}]      # index 2 is mapped away in every condition: the point needs 0, 1 and 7
    assert VN.basic("mm", maps=moved)[0].d == 8
    fixed = [{4: 0.0, 0: 0.5, 1: 0.5, 2: 0.5}] * 3                # nothing is read from the point at all
    like = VN.basic("mm", maps=fixed)[0]
    assert like.d == 0 and like._view_size() == 5
    assert like.batch(np.zeros((2, 1))).tobytes() == like.batch(np.full((2, 1), np.nan)).tobytes()
    readers = VN.readers(1)[0]
    assert readers._view_size() == 10 and readers.d == 15         # P < d


def test_viewed_restates_the_mappings():
    multi, _, maps = VN.basic("mm")
    X = VN.points("mm", 8, 36)
    V = multi.viewed(X)
    assert V.shape == (8, 3, 5)
    for c in range(3):
        want = VN.viewed(maps, c, X, 5)
        want[:, 3] = 0.0                     # (index 3: nothing reads it)
        assert V[:, c].tobytes() == want.tobytes() and multi.viewed(X, c).tobytes() == want.tobytes()
    with pytest.raises(ValueError, match="conditions"):
        NW.michaelis_menten().viewed(X)


@pytest.mark.parametrize("params,match", [
    ({3: 0}, "not a parameter index the network reads"),
    ({-1: 0}, "not a parameter index the network reads"),
    ({"k": 0}, "not a parameter index the network reads"),
    ({0: -1}, "an int >= 0"),
    ({0: np.nan}, "finite value"),
    ({0: np.inf}, "finite value"),
    ({0: "1"}, "an int >= 0"),
    ({0: Monomial({1: 1})}, "an int >= 0"),
    ({0: True}, "a bool is refused"),
    ({0: np.bool_(False)}, "a bool is refused"),
    ([0, 1], "must be a mapping"),
    (3, "must be a mapping"),
])
def test_params_are_validated(params, match):
    maps = VN.mappings_of("mm")
    maps[1] = params
    with pytest.raises(ValueError, match="MassActionODELogLike: condition 1: .*" + match):
        VN.basic("mm", maps=maps)


def test_numpy_integers_count_as_indices():
    maps = VN.mappings_of("mm")
    maps[1] = {np.int64(4): -0.5, np.int32(0): np.int64(3)}
    X = VN.points("mm", 4, 37)
    assert VN.basic("mm", maps=maps)[0].batch(X).tobytes() == VN.basic("mm")[0].batch(X).tobytes()


def test_the_view_has_a_limit():
    never, _ = CN.mm()

    def make(top):
        rx = list(NW.MM_REACTIONS)
        rx[2] = (rx[2][0], rx[2][1], Monomial({2: 1, top: 1}))
        return MassActionODELogLike(4, rx, None, NW.MM_T, CN.MM_OBSERVABLES, None, None, conditions=[dict(c, params={top: 0.0}) for c in never.conditions])
    assert make(ODE_MAX_VIEW_COORDINATES - 1)._view_size() == ODE_MAX_VIEW_COORDINATES == 128
    with pytest.raises(ValueError, match="at most 128 coordinates"):
        make(ODE_MAX_VIEW_COORDINATES)


def test_a_constraint_on_a_replaced_coordinate_is_refused_and_others_stay_on_condition_0():
    with pytest.raises(ValueError, match=r"constraint 1 reads parameter 0, which condition 1 replaces"):
        VN.basic("mm", constraints=[(Monomial({2: 1}), 0.0, 2.0), (Monomial({2: 1, 0: -1}), 0.0, 2.0)])
    cons = [(Monomial({2: 1}, 0.25), 1.0, 2.0)]
    multi, single, maps = VN.basic("mm", constraints=cons)
    X = VN.points("mm", 16, 38)
    terms, g = multi.batch_conditions(X), multi.constraint_terms(X)
    assert np.all(np.isfinite(g)) and np.all(g != 0)
    assert terms[:, 0].tobytes() == (single(0, constraints=None).batch(VN.viewed(maps, 0, X, 5)) + g).tobytes()
    for c in (1, 2):
        assert terms[:, c].tobytes() == single(c, constraints=None).batch(VN.viewed(maps, c, X, 5)).tobytes()
    same = [dict(maps[0]), {**maps[1], 2: 2}, dict(maps[2])]     # (an explicit identity replaces nothing)
    assert VN.basic("mm", constraints=cons, maps=same)[0].batch(X).tobytes() == multi.batch(X).tobytes()


def test_the_rest_of_the_surface_follows_the_view():
    multi, single, maps = VN.basic("mm")
    X = VN.points("mm", 16, 39)
    dense = np.linspace(0.25, 10.0, 27)
    sim = multi.with_outputs(dense).simulate(X)
    assert sim.shape == (16, 3, 27, 2)
    for c in range(3):
        V = VN.viewed(maps, c, X, 5)
        assert sim[:, c].tobytes() == single(c).with_outputs(dense).simulate(V).tobytes()
        for x, v in zip(X[:3], V[:3]):
            assert multi.fixed_steps(x, 2.0, 9, condition=c).tobytes() == single(c).fixed_steps(v, 2.0, 9).tobytes()
    assert np.any(multi.fixed_steps(X[0], 2.0, 9, condition=0) != multi.fixed_steps(X[0], 2.0, 9, condition=1))
    again = pickle.loads(pickle.dumps(multi))
    assert again.batch_conditions(X).tobytes() == multi.batch_conditions(X).tobytes() and again.source() == multi.source()
    rows, traj = posterior_predictive([X[:8], X[8:]], multi, burnin=2, thin=2, device=False)
    assert rows.tobytes() == np.concatenate([X[2:8:2], X[10::2]]).tobytes() and traj.tobytes() == multi.simulate(rows).tobytes()
    rows, traj = posterior_predictive([X[:8], X[8:]], multi, device=False, t=dense)
    assert traj.tobytes() == sim.tobytes()


# ---------------------------------------------------------------------------------------------------- the host build under sanitizers
MAIN = r'''
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
extern "C" void dzode_loglike(const double* X, long long n, int ld, const double* blk, double* like, int* nsteps);
static const double POINTS[] = {%s};
static const double BLOCK[] = {%s};
int main()
{
    const long long n = %d;
    const int d = %d;
    double* X = (double*)malloc(sizeof POINTS);             // exactly n * d doubles, and the exact block
    double* blk = (double*)malloc(sizeof BLOCK);
    double* like = (double*)malloc(n * sizeof(double));
    int* steps = (int*)malloc(n * sizeof(int));
    memcpy(X, POINTS, sizeof POINTS);
    memcpy(blk, BLOCK, sizeof BLOCK);
    if (sizeof POINTS != n * d * sizeof(double)) return 2;
    dzode_loglike(X, n, d, blk, like, steps);
    for (long long i = 0; i < n; ++i) printf("%%a\n", like[i]);
    free(X); free(blk); free(like); free(steps);
    return 0;
}
'''


def _host_compiler():
    return "/opt/rocm/llvm/bin/clang++" if os.path.exists("/opt/rocm/llvm/bin/clang++") else "g++"


def test_the_host_build_under_sanitizers_reads_nothing_beyond_the_point(tmp_path):
    """a P > d model (P = 5, d = 4: the formal index is never read from the point): the generated source and a small main, compiled
    with -fsanitize=address,undefined, on a heap row of exactly n * d doubles; a clean exit and the bytes of the normal host build.
    A stand-alone program: nothing is preloaded, nothing is loaded into python."""
    cc, flags = _host_compiler(), ["-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-fsanitize=address,undefined",
                                   "-fno-sanitize-recover=all", "-I" + csrc_dir()]
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    built = subprocess.run([cc] + flags + ["-o", str(tmp_path / "probe"), str(probe)], capture_output=True, text=True)
    if built.returncode != 0 or subprocess.run([str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.skip("no address / undefined-behaviour sanitizer runtime for %s here: %s" % (cc, built.stderr.strip()[-200:]))
    multi, _, _ = VN.basic("mm")
    assert multi._view_size() > multi.d == 4
    X = VN.points("mm", 12, 40, outside=0.05)
    X[3, 0], X[5, 3] = np.nan, np.inf
    hexes = lambda a: ", ".join("__builtin_nan(\"\")" if v != v else "__builtin_huge_val()" if v == np.inf else float(v).hex() for v in a.reshape(-1))      # noqa: E731
    src = tmp_path / "view_main.cpp"
    src.write_text(multi.source() + MAIN % (hexes(X), hexes(multi.data_block()), len(X), X.shape[1]))
    exe = tmp_path / "view_main"
    built = subprocess.run([cc] + flags + ["-o", str(exe), str(src), "-lm"], capture_output=True, text=True)
    assert built.returncode == 0, built.stderr[-2000:]
    ran = subprocess.run([str(exe)], capture_output=True, text=True)
    assert ran.returncode == 0 and not ran.stderr, ran.stderr[-2000:]
    got = np.array([float.fromhex(line) if "inf" not in line and "nan" not in line else float(line) for line in ran.stdout.split()])
    want = multi.batch(X)
    assert got.tobytes() == want.tobytes() and want[3] == -np.inf and np.isfinite(want).sum() >= 6
