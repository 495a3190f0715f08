"""The extended device priors (dz_set_prior_ext, pydream_amd/csrc/dz_prior_ext.h) without a GPU: the host twin dz_prior_ext_host -- the kernel's
functions in the kernel's order -- against tests/prior_reference.py (40 digits, bounds derived there), the reference against scipy, the parameters'
own description of themselves, the support / covered functions, and the two selections (dz_mega_select.h, dz_multi_select.h) with prior_ext set."""
import ctypes
import json
import os
import shutil
import subprocess

import mpmath
import numpy as np
import pytest
import scipy.stats as st

from pydream_amd import _capi
from pydream_amd.model import Model
from pydream_amd.parameters import FlatParam, SampledParam

from . import prior_reference as REF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pydream_amd", "csrc")
INF = float("inf")
SCIPY = {1: st.norm, 2: st.uniform, 3: st.laplace, 4: st.cauchy, 5: st.t, 6: st.lognorm, 7: st.gamma, 8: st.beta, 9: st.halfnorm, 10: st.halfcauchy,
         11: st.truncnorm, 12: st.loguniform, 13: st.invgamma}
NSHAPES = {1: 0, 2: 0, 3: 0, 4: 0, 5: 1, 6: 1, 7: 1, 8: 2, 9: 0, 10: 0, 11: 2, 12: 2, 13: 1}
INSIDE = 6      # prior_reference.cases: the first points of every case lie well inside the support


def frozen(kind, a, b, s1, s2):
    return SCIPY[kind](*((s1, s2)[:NSHAPES[kind]]), loc=a, scale=b)


def twin1(kind, a, b, s1, s2, x):
    one = lambda v: np.array([v], dtype=np.float64)
    return _capi.prior_ext_host(np.array([kind], np.int32), one(a), one(b), one(s1), one(s2), np.asarray(x, dtype=np.float64).reshape(-1, 1))


@pytest.fixture(scope="module")
def cases():
    return REF.cases()


def test_the_host_twin_stays_inside_the_derived_bounds_on_every_input(cases):
    """no value filtered: every point of every case; where the reference is +-inf the twin says the same"""
    bad, worst, ninf, pinf = [], 0.0, 0, 0
    for kind, a, b, s1, s2, x in cases:
        got = twin1(kind, a, b, s1, s2, x)
        for xi, g in zip(x, got):
            ref = REF.logpdf(kind, xi, a, b, s1, s2)
            if not mpmath.isfinite(ref):
                ninf += ref < 0; pinf += ref > 0
                if float(ref) != g:
                    bad.append((REF.NAMES[kind], a, b, s1, s2, xi, g, float(ref)))
                continue
            bound = REF.term_bound(kind, xi, a, b, s1, s2, ref)
            err = abs(mpmath.mpf(float(g)) - ref) if np.isfinite(g) else mpmath.inf
            worst = max(worst, float(err / bound) if bound > 0 else (0.0 if err == 0 else INF))
            if not err <= bound:
                bad.append((REF.NAMES[kind], a, b, s1, s2, xi, g, float(ref), float(err), float(bound)))
    print("largest |twin - ref| / bound: %.3f; -inf points %d, +inf points %d" % (worst, ninf, pinf))
    assert not bad, bad[:10]
    assert ninf > 300 and pinf >= 10          # the inputs do reach outside every bounded support and the infinite ends


def test_the_reference_equals_scipy_to_1e_12_relative(cases):
    """guards the table against a misread parametrisation: the points well inside every support to 1e-12 relative, and scipy's infinities where the
    reference has them"""
    bad = []
    for kind, a, b, s1, s2, x in cases:
        sp = frozen(kind, a, b, s1, s2).logpdf(x)
        for i, (xi, s) in enumerate(zip(x, sp)):
            ref = REF.logpdf(kind, xi, a, b, s1, s2)
            if not mpmath.isfinite(ref):
                ok = float(ref) == s
            elif i < INSIDE:
                ok = abs(mpmath.mpf(float(s)) - ref) <= mpmath.mpf("1e-12") * abs(ref)
            else:
                continue
            if not ok:
                bad.append((REF.NAMES[kind], a, b, s1, s2, xi, float(ref), s))
    assert not bad, bad[:10]


PARAMS = [
    ("laplace", lambda: SampledParam(st.laplace, loc=0.5, scale=2.0)),
    ("cauchy", lambda: SampledParam(st.cauchy, loc=[0.0, 1.0, -2.0], scale=[1.0, 0.25, 30.0])),
    ("t", lambda: SampledParam(st.t, [1.0, 4.5, 60.0], loc=[0.0, 1.0, 2.0], scale=0.5)),
    ("lognorm", lambda: SampledParam(st.lognorm, s=[0.25, 1.5], loc=0.1, scale=[1e-3, 1e3])),
    ("gamma", lambda: SampledParam(st.gamma, [0.5, 1.0, 2.5], scale=[2.0, 1.0, 0.5])),
    ("expon", lambda: SampledParam(st.expon, loc=[1.0, 0.0], scale=[3.0, 0.125])),
    ("beta", lambda: SampledParam(st.beta, [0.5, 1.0, 2.5], [2.5, 1.0, 0.5], loc=-1.0, scale=4.0)),
    ("halfnorm", lambda: SampledParam(st.halfnorm, scale=[0.2, 5.0])),
    ("halfcauchy", lambda: SampledParam(st.halfcauchy, loc=0.25, scale=0.1)),
    ("truncnorm", lambda: SampledParam(st.truncnorm, [-1.0, 3.0, -INF], [2.0, 6.0, 0.5], loc=[0.0, 1.0, 2.0], scale=[1.0, 2.0, 0.5])),
    ("loguniform", lambda: SampledParam(st.loguniform, [0.5, 1e-3], [8.0, 1e2])),
    ("reciprocal", lambda: SampledParam(st.reciprocal, 0.5, 8.0, scale=3.0)),
    ("invgamma", lambda: SampledParam(st.invgamma, [0.5, 2.5], scale=[1.0, 4.0])),
    ("norm", lambda: SampledParam(st.norm, loc=[1.0, -1.0], scale=[0.5, 2.0])),
    ("uniform", lambda: SampledParam(st.uniform, loc=-6.0, scale=[22.0, 3.0])),
]


@pytest.mark.parametrize("name,make", PARAMS, ids=[p[0] for p in PARAMS])
def test_a_parameter_describes_itself_and_the_twin_agrees_with_its_prior(name, make):
    """SampledParam(dist, ...).device_prior_ext() fed to the twin against param.prior(x): vector-valued parameters with array shapes, expon as gamma(1);
    the bound is the reference's for the same point"""
    np.random.seed(11)
    param = make()
    ext = param.device_prior_ext()
    assert ext is not None and all(len(v) == param.dsize for v in ext) and ext[0].dtype == np.int32
    if name == "expon":
        assert (ext[0] == 7).all() and (ext[3] == 1.0).all()
    for _ in range(8):
        x = np.atleast_1d(param.random())
        got = _capi.prior_ext_host(*ext, x[None, :])[0]
        ref, bound = REF.point(*ext, x)
        assert REF.agrees(got, ref, bound), (x, got, float(ref), float(bound))
        want = param.prior(x)
        assert abs(mpmath.mpf(float(want)) - ref) <= mpmath.mpf("1e-12") * abs(ref), (x, want, float(ref))      # (scipy's own rounding: not the twin's bound)


def test_flat_parameters_and_models_concatenate_and_unknown_families_say_none():
    model = Model(lambda q: 0.0, [SampledParam(st.norm, loc=0.0, scale=1.0), FlatParam(np.zeros(2)), SampledParam(st.gamma, 2.0, scale=[1.0, 3.0])])
    assert model.device_prior() is None                      # (as before: tests/test_api_cpu.py)
    kind, a, b, s1, s2 = model.device_prior_ext()
    assert kind.tolist() == [1, 0, 0, 7, 7] and b.tolist() == [1.0, 1.0, 1.0, 1.0, 3.0] and s1.tolist() == [0.0, 0.0, 0.0, 2.0, 2.0] and not s2.any() and not a.any()
    assert SampledParam(st.weibull_min, 1.5).device_prior_ext() is None
    assert Model(lambda q: 0.0, [SampledParam(st.norm), SampledParam(st.weibull_min, 1.5)]).device_prior_ext() is None
    assert SampledParam(st.gamma, 2.0).device_prior() is None and SampledParam(st.norm).device_prior_ext()[0].tolist() == [1]


def test_kinds_up_to_2_equal_the_numpy_restatement_bit_for_bit():
    """prior_of_point (dz_kernels.h) restated in numpy: per lane the two dimensions of each 128-chunk in ascending order, chunks ascending, the xor
    butterfly 32 .. 1; t1 = (-(z z) / 2 - 0.918...) - logb with z = (x - a) (1 / b), t2 = -logb inside [a, a + b] else -inf.  logb = dlog(b) enters
    as data: the scales are powers of two, 2^m, where dlog's polynomial part is exactly 0 and its value is fma(m, ln2_hi, fma(m, ln2_lo, 0)), restated here."""
    rng = np.random.default_rng(5)
    for d in (1, 13, 130, 300):
        kind = rng.integers(0, 3, d).astype(np.int32)
        a = rng.normal(0, 2, d)
        m = rng.integers(-10, 11, d)
        b = 2.0 ** m
        ef = m.astype(np.float64)
        inner = [float(mpmath.mpf(e) * mpmath.mpf(1.90821492927058770002e-10)) for e in ef]      # (an fma is one rounding of the exact result: 40 digits hold it)
        logb = np.array([float(mpmath.mpf(e) * mpmath.mpf(6.93147180369123816490e-01) + mpmath.mpf(i)) for e, i in zip(ef, inner)])
        X = a + b * rng.uniform(-0.5, 1.5, (9, d))
        X[3, 0] = np.nan
        z = (X - a) * (1.0 / b)
        with np.errstate(invalid="ignore"):
            t1 = (-(z * z) / 2.0 - 0.91893853320467274178) - logb
            t2 = np.where((X >= a) & (X <= a + b), -logb, -INF)
        T = np.where(kind == 1, t1, np.where(kind == 2, t2, 0.0))
        want = np.zeros(len(X))
        for i in range(len(X)):
            acc = np.zeros(64)
            for j in range(d):
                acc[(j % 128) // 2] = acc[(j % 128) // 2] + T[i, j]
            for off in (32, 16, 8, 4, 2, 1):
                acc = acc + acc[np.arange(64) ^ off]
            want[i] = acc[0]
        got = _capi.prior_ext_host(kind, a, b, np.zeros(d), np.zeros(d), X)
        nan = np.isnan(want)      # (row 3 where dimension 0 is normal; a NaN's sign and payload are not part of the contract: nan_to_ninf maps it)
        assert np.array_equal(np.isnan(got), nan) and got[~nan].tobytes() == want[~nan].tobytes(), (d, got, want)


def test_refusals_name_the_dimension():
    z = np.zeros(3)
    for kind, b, s1, s2, dim, word in [([1, 14, 0], [1, 1, 1], z, z, 1, "kind"), ([1, 3, 0], [1, 0.0, 1], z, z, 1, "scale"), ([0, 3, 4], [-1, 1, INF], z, z, 2, "scale"),
                                        ([1, 1, 5], [1, 1, 1], [0, 0, -1.0], z, 2, "t:"), ([1, 1, 8], [1, 1, 1], [0, 0, 1.0], [0, 0, 0.0], 2, "beta"),
                                        ([1, 1, 11], [1, 1, 1], [0, 0, 40.0], [0, 0, 41.0], 2, "mass"), ([1, 1, 11], [1, 1, 1], [0, 0, 2.0], [0, 0, 1.0], 2, "lo < hi"),
                                        ([1, 1, 12], [1, 1, 1], [0, 0, 0.0], [0, 0, 1.0], 2, "loguniform")]:
        with pytest.raises(_capi.DreamZSError) as exc:
            _capi.prior_ext_host(kind, z, np.asarray(b, float), np.asarray(s1, float), np.asarray(s2, float), np.zeros((1, 3)))
        assert "dimension %d" % dim in str(exc.value) and word in str(exc.value), str(exc.value)


def test_the_oracle_alone_redraws_in_the_stated_share_of_its_steps():
    """tests/prior_ext_cases.py, multitry 3 without hard boundaries: the oracle, on the twin's prior, draws whole proposal sets again in at least 10 % and
    at most 60 % of its chain steps -- the configuration in which tests/test_prior_ext_gpu.py expects the engine to report redraw rounds; with hard
    boundaries it still redraws (a reflected proposal may land on lognorm's open end) but far less"""
    from oracle import oracle as O
    from tests import prior_ext_cases as PC
    share = {}
    for hard in (0, 1):
        sizes = []
        e = PC.make(O.Engine, 3, hard, likelihood=lambda e: e.set_likelihood_host(PC.oracle_callback(sizes=sizes)))
        e.step(PC.GENS)
        tr = e.get_trace(0, PC.GENS)
        assert np.isfinite(tr["logp"]).all() and tr["moved"].mean() > 0.1
        share[hard] = PC.redrawn_fraction(sizes[PC.N:], 3)
        e.close()
    print("redrawn share of the oracle's steps: %.3f without hard boundaries, %.3f with" % (share[0], share[1]))
    assert 0.10 <= share[0] <= 0.60 and share[1] < share[0]


# ---------------------------------------------------------------------------------------------------- the header's host functions and the selections
SOURCE = r"""
#include "%(csrc)s/dz_prior_ext.h"
#include "%(csrc)s/dz_multi_select.h"
#include <string>
using namespace dz;
extern "C" void support_of(int kind, double a, double b, double s1, double s2, double* o)
{
    const PriorExtSupport S = support(kind, a, b, s1, s2);
    o[0] = S.lo; o[1] = S.hi; o[2] = S.lo_finite; o[3] = S.hi_finite;
}
extern "C" int covered_by(int kind, double a, double b, double s1, double s2, int hard, double mn, double mx) { return covered(kind, a, b, s1, s2, hard != 0, mn, mx); }
extern "C" int mega_family(const int* v, int ext)
{
    MegaShape s;
    s.d = v[0]; s.ld = v[1]; s.k = v[2]; s.depairs = v[3]; s.npt = v[4]; s.nslots = v[5]; s.ncr = v[6]; s.ngamma = v[7]; s.J = v[8];
    s.tri = v[9]; s.mtp = v[10]; s.hard = v[11]; s.have_prior = v[12]; s.nl = v[13]; s.N = v[14]; s.ncu = v[15]; s.lk = v[16]; s.lk_items = v[17];
    for (int i = 0; i < 4; ++i) s.gen_fn[i] = v[18 + i];
    s.redo_possible = v[22]; s.ad_multi = v[23]; s.ad_R1 = v[24]; s.ad_nbp = v[25]; s.adapt_lag = v[26]; s.adapt_fused = v[27]; s.adapt_groups = v[28];
    s.tempering = v[29]; s.world = v[30]; s.mega = v[31]; s.mega_d2 = v[32]; s.mega_kc = v[33]; s.mega_redo = v[34];
    s.prior_ext = ext != 0;
    return (int)mega_choose(s).family;
}
// the launches of one eval_logp call as a bit set of what follows the family's kernel, the family, and the k_prior_ext launch
extern "C" void logp_of(const int* v, int ext, int n, long long* o)
{
    MultiShape s;
    s.d = v[0]; s.ld = v[1]; s.k = v[2]; s.depairs = v[3]; s.nslots = v[4]; s.nch = v[5]; s.tri = v[6]; s.mtp_len = v[7]; s.mu_zero = v[8]; s.have_prior = v[9];
    s.nl = v[10]; s.N = v[11]; s.ncu = v[12]; s.nlanes = v[13]; s.lk = v[14]; s.lk_lanes = v[15]; s.lk_items = v[16]; s.redo_possible = v[17]; s.adapt = v[18];
    s.tempering = v[19]; s.world = v[20]; s.thin = v[21]; s.burnin = v[22]; s.history_lag = v[23]; s.adapt_lag = v[24]; s.adapt_groups = v[25]; s.trace = v[26];
    s.propose_split = v[27]; s.q_defer = v[28]; s.logp_gemm = v[29];
    s.prior_ext = ext != 0;
    const LogpPlan P = logp_plan(s, n, false);
    const long long r[] = {P.family, P.main.grid, P.main.block, (long long)P.main.lds, P.q_finish, P.sum_items, P.prior_only, P.prior_add, P.prior_ext, P.ext_fix_like,
                           P.ext.grid, P.ext.block, (long long)P.ext.lds, multi_max_threads(MK_PRIOR_EXT, s.nch)};
    for (int i = 0; i < 14; ++i) o[i] = r[i];
    MultiCarry c;
    const GenerationPlan G = generation_plan(s, MultiStep{0, s.nl, 1u, true, true, 0}, c);
    o[14] = G.qdefer;
}
"""


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    cxx = next((c for c in ("g++", "c++", "clang++", "/opt/rocm/lib/llvm/bin/clang++") if shutil.which(c)), None)
    assert cxx, "no host C++ compiler"
    tmp = tmp_path_factory.mktemp("prior_ext")
    src, so = str(tmp / "prior_ext.cpp"), str(tmp / "libprior_ext.so")
    with open(src, "w") as f:
        f.write(SOURCE % dict(csrc=CSRC))
    subprocess.check_call([cxx, "-O1", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", "-shared", "-fPIC", src, "-o", so])      # (no HIP header on the include path)
    L = ctypes.CDLL(so)
    D = ctypes.c_double
    L.support_of.argtypes = [ctypes.c_int, D, D, D, D, ctypes.POINTER(D)]
    L.covered_by.argtypes = [ctypes.c_int, D, D, D, D, ctypes.c_int, D, D]
    return L


# (kind, a, b, s1, s2) -> (lo, hi, lo_finite, hi_finite)
SUPPORTS = [((0, 0, 1, 0, 0), (-INF, INF, 1, 1)), ((1, 2, 3, 0, 0), (-INF, INF, 1, 1)), ((2, -6, 22, 0, 0), (-6, 16, 1, 1)), ((3, 1, 2, 0, 0), (-INF, INF, 1, 1)),
            ((4, 1, 2, 0, 0), (-INF, INF, 1, 1)), ((5, 1, 2, 4.5, 0), (-INF, INF, 1, 1)), ((6, 0.5, 2, 0.7, 0), (0.5, INF, 0, 1)), ((7, 1, 2, 0.5, 0), (1, INF, 0, 1)),
            ((7, 1, 2, 1.0, 0), (1, INF, 1, 1)), ((7, 1, 2, 2.5, 0), (1, INF, 0, 1)), ((8, -1, 4, 1.0, 1.0), (-1, 3, 1, 1)), ((8, -1, 4, 0.5, 1.0), (-1, 3, 0, 1)),
            ((8, -1, 4, 1.0, 2.5), (-1, 3, 1, 0)), ((9, 0.25, 2, 0, 0), (0.25, INF, 1, 1)), ((10, 0.25, 2, 0, 0), (0.25, INF, 1, 1)), ((11, 1, 2, -1, 2), (-1, 5, 1, 1)),
            ((11, 1, 2, -INF, 0.5), (-INF, 2, 1, 1)), ((12, 0, 2, 0.5, 8), (1, 16, 1, 1)), ((13, 0.5, 2, 2.5, 0), (0.5, INF, 0, 1))]
# (kind, a, b, s1, s2, hard, mins, maxs) -> covered
COVERED = [((1, 0, 1, 0, 0, 0, -INF, INF), 1), ((4, 0, 1, 0, 0, 0, -INF, INF), 1), ((5, 0, 1, 3, 0, 1, -1, 1), 1),
           ((2, -6, 22, 0, 0, 1, -6, 16), 1), ((2, -6, 22, 0, 0, 0, -6, 16), 0), ((2, -6, 22, 0, 0, 1, -7, 16), 0), ((2, -6, 22, 0, 0, 1, -6, 16.5), 0),
           ((9, 0.25, 2, 0, 0, 1, 0.25, INF), 1), ((9, 0.25, 2, 0, 0, 0, 0.25, INF), 0), ((9, 0.25, 2, 0, 0, 1, 0.0, INF), 0), ((10, 0, 1, 0, 0, 1, 0, 50), 1),
           ((11, 1, 2, -1, 2, 1, -1, 5), 1), ((11, 1, 2, -1, 2, 1, -1, 5.5), 0), ((11, 1, 2, -INF, 0.5, 1, -INF, 2), 1), ((11, 1, 2, -INF, 0.5, 1, -INF, 2.5), 0),
           ((12, 0, 2, 0.5, 8, 1, 1, 16), 1), ((12, 0, 2, 0.5, 8, 1, 0.5, 16), 0), ((7, 0, 1, 1.0, 0, 1, 0, INF), 1), ((7, 0, 1, 2.5, 0, 1, 0, INF), 0),
           ((7, 0, 1, 2.5, 0, 1, 0.125, INF), 1), ((7, 0, 1, 0.5, 0, 1, 0, INF), 0), ((8, -1, 4, 1, 1, 1, -1, 3), 1), ((8, -1, 4, 0.5, 1, 1, -1, 3), 0),
           ((8, -1, 4, 1, 2.5, 1, -1, 3), 0), ((8, -1, 4, 1, 2.5, 1, -1, 2.5), 1), ((6, 0, 1, 0.7, 0, 1, 0, INF), 0), ((6, 0, 1, 0.7, 0, 1, 0.5, 9), 1),
           ((13, 0, 1, 2.5, 0, 1, 0, INF), 0), ((13, 0, 1, 2.5, 0, 0, 1, 2), 0)]


def test_support_and_covered_over_a_table(lib):
    for args, want in SUPPORTS:
        o = (ctypes.c_double * 4)()
        lib.support_of(int(args[0]), *[float(v) for v in args[1:]], o)
        assert tuple(o) == tuple(float(v) for v in want), (args, tuple(o))
    for args, want in COVERED:
        got = lib.covered_by(int(args[0]), *[float(v) for v in args[1:5]], int(args[5]), float(args[6]), float(args[7]))
        assert got == want, (args, got)


def test_the_density_is_finite_wherever_covered_says_so():
    """what covered promises, asked of the twin: at both boundaries of every row of COVERED that is covered and bounded there, the term is finite"""
    for args, want in COVERED:
        if want and args[5]:
            for x in (args[6], args[7]):
                if np.isfinite(x):
                    assert np.isfinite(twin1(args[0], args[1], args[2], args[3], args[4], [x])[0]), (args, x)


def test_an_extended_prior_takes_every_recorded_shape_to_the_multi_kernel_path(lib):
    """mega_choose with prior_ext: MEGA_NONE for every shape of tests/mega_select_cases.py (as recorded in the golden file); without it some family runs
    (that the recorded selections themselves are reproduced unchanged is tests/test_mega_select_cpu.py's and tests/test_multi_select_cpu.py's)"""
    with open(os.path.join(ROOT, "tests", "golden", "mega_selection.json")) as f:
        entries = [e for e in json.load(f)["entries"] if "shape" in e]      # (the cases the engine refuses have none)
    some = 0
    for e in entries:
        v = (ctypes.c_int * 35)(*e["shape"][:35])
        assert lib.mega_family(v, 1) == 0, e["case"]
        some += lib.mega_family(v, 0) != 0
    assert some > len(entries) // 2


def test_the_logp_plan_gains_exactly_the_one_launch(lib):
    """for every recorded shape of the multi-kernel path and n = 1, 9, 260: the family's kernel, k_q_finish and k_sum_items as without the extended prior;
    k_prior_only / k_prior_add gone, k_prior_ext in their place with their geometry (a wave per point, four per block), mapping the likelihood's NaN
    exactly where k_prior_add would have; and no deferred row-tile sums (the kernels that finish those write a zero prior)"""
    with open(os.path.join(ROOT, "tests", "golden", "multi_selection.json")) as f:
        entries = [e for e in json.load(f)["entries"] if "shape" in e]      # (the cases the engine refuses have none)
    kinds = set()
    for e in entries:
        v = (ctypes.c_int * 30)(*e["shape"][:30])
        for n in (1, 9, 260):
            p0, p1 = (ctypes.c_longlong * 15)(), (ctypes.c_longlong * 15)()
            lib.logp_of(v, 0, n, p0)
            lib.logp_of(v, 1, n, p1)
            assert list(p1[:6]) == list(p0[:6]), e["case"]
            assert p0[8] == 0 and p1[6] == 0 and p1[7] == 0 and p1[8] == 1 and p1[9] == p0[7], e["case"]
            assert (p1[10], p1[11], p1[12]) == ((n + 3) // 4, 256, 0) and p1[13] == 256, e["case"]
            assert p1[14] == 0
            kinds.add(p0[0])
    assert len(kinds) >= 4
