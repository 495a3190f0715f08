"""Every device copy of the three built-in densities -- the multivariate normal (dense matrix / triangular factor), the identity-covariance
mixture and the per-dimension priors -- against tests/density_reference.py: the plain formulas in extended precision, under error bounds
derived from the rounding model (that file's docstring), on inputs no other test uses.  The oracle does not appear here: kernel == oracle is
what the rest of the suite pins, bit for bit; this file (with tests/test_density_reference_cpu.py for the oracle) pins both to the density.
Every value the device returns is compared, none is filtered; where the reference is -inf the device must say -inf.

Part A: dz_eval_logp's kernels, each reached by the dimensions and point counts eval_logp (dz_engine.hip) selects it for -- the rule is
restated at each test, and every call is checked to have been one timed `logp' evaluation.
Part B: the copies inside the persistent kernels (k_generations, _w4, _d2, _mix) and on the multi-kernel path: short runs whose every traced
log p is compared with prior(X) + likelihood(X) of the traced state, and get_state()'s two halves with each.

Worst error-to-bound ratios (1 = the bound; every test prints its own):
    CPU oracle, d = 1 .. 1024 (tests/test_density_reference_cpu.py)     MVN 0.39   mixture 0.14   prior 0.10
    MI355X, dz_eval_logp     k_logp_mvn_lds 0.39   k_logp_mvn_mfma<1|2> 0.25   k_logp_mvn_mfma_tiled 0.21   k_logp_mvn_gemm<1> 0.21, <2> 0.11, <4> 0.11
                             k_logp_mix 0.16, its prior 0.11   k_prior_only 0.11 (the MVN beside it 0.24)   k_prior_add 0.07
    MI355X, the sampler      (traced log p / get_state's log prior / log likelihood)
                             k_generations 0.22 / 0.11 / 0.18   k_generations_w4 0.16 / - / 0.10   k_generations_d2 0.01 / 0.01 / 0.01
                             k_generations_mix 0.09 / 0.09 / 0.07   multi-kernel path 0.01 / 0.01 / 0.01
(the sampler's states sit within a few standard deviations of the mean, where the magnitude A the bound is made of is far above the
quadratic form itself: the small ratios at d > 128 are those of sqrt(d)-like error growth against a bound that grows like d)"""
import ctypes
import re

import numpy as np
import pytest

from tests import density_reference as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def G():
    from pydream_amd import _capi
    return _capi


@pytest.fixture(scope="module")
def num_cu(G):
    """the device's compute-unit count, as dz_create reads it (hipDeviceProp_t::multiProcessorCount), from the HIP runtime the engine uses"""
    hip = ctypes.CDLL(G.hip_library())
    v = ctypes.c_int(0)
    assert hip.hipDeviceGetAttribute(ctypes.byref(v), 63, 0) == 0          # hipDeviceAttributeMultiprocessorCount
    assert 1 <= v.value <= 4096
    return v.value


def report(name, worst):
    print("worst error / bound  %-28s %.3f" % (name, worst))


_REF = {}


def mvn_case(family, d, zero, tri, ndist):
    """the distinct points of a case with their reference values and bounds, made once"""
    key = (family, d, zero, tri)
    if key not in _REF or len(_REF[key][0]) < ndist:
        P, Uf = R.matrices(family, d)
        M = Uf if tri else P
        mu = R.mean(d, zero)
        X = R.mvn_points(d, mu, n=ndist)
        ref, bound = R.mvn(X, mu, M, R.log_f(d), tri)
        _REF[key] = (X, ref, bound, mu, M)
    return _REF[key]


def eval_once(e, X):
    """one dz_eval_logp call that was one timed evaluation"""
    e.profile_reset()
    pr, lk = e.eval_logp(X)
    assert e.profile_get("logp")[1] == 1
    return pr, lk


def run_mvn(G, d, family, forms, ns, monkeypatch=None, gemm=None):
    worst = 0.0
    if gemm is not None:
        monkeypatch.setenv("DZ_LOGP_GEMM", gemm)
    e = G.Engine(nchains=4, ndim=d, history_capacity=8)
    e.profile_enable(True)
    ndist = min(R.NDISTINCT, max(ns))
    for tri in forms:
        for zero in (True, False):
            X, ref, bound, mu, M = mvn_case(family, d, zero, tri, ndist)
            e.set_likelihood_mvn(mu, M, int(tri), R.log_f(d))
            for n in ns:
                idx = R.spread(n, ndist)
                pr, lk = eval_once(e, X[idx])
                assert not pr.any()                                      # no prior set: exactly 0
                worst = max(worst, R.check(lk, ref[idx], bound[idx], "mvn family %s d=%d tri=%d zero-mean=%d n=%d" % (family, d, tri, zero, n)))
                if n > R.SPECIAL[0]:
                    assert lk[R.SPECIAL[0]] == R.log_f(d)                # Q = 0 at the mean
    e.close()
    return worst


def families_at(d, one_d):
    return ("a", "b", "c", "d") if d == one_d else ("a", "b", "c")


# ------------------------------------------------------------------------------------------------------------------ part A: dz_eval_logp
# eval_logp: nrt = ceil(d / 16) <= 8 and matrix (packed triangle, or the square) + mean + four wave tiles within 160 KB of LDS -> k_logp_mvn_lds<nrt, tri|dense>:
# both forms up to d = 112, the triangle alone at 113 .. 128.  A block has max(4, min(8, ceil(ceil(n / 16) / CUs))) waves: more than four from n > 16 * 4 * CUs.
@pytest.mark.parametrize("d", R.LDS_D_BOTH + R.LDS_D_TRI)
def test_k_logp_mvn_lds(G, d):
    forms = (False, True) if d in R.LDS_D_BOTH else (True,)
    ns = R.LDS_N + (R.LDS_BIG_N if d == 17 else ())
    worst = max(run_mvn(G, d, f, forms, ns) for f in families_at(d, 17))
    report("k_logp_mvn_lds d=%d" % d, worst)


# ... the dense square at 113 .. 128 does not fit: k_logp_mvn_mfma<1, nrt, dense>, and <2, ..> (two point tiles per wave) from 1025 point tiles on
@pytest.mark.parametrize("d", R.MFMA_D)
def test_k_logp_mvn_mfma(G, d):
    ns = R.MFMA_N + ((R.MFMA2_N,) if d == 113 else ())
    assert (R.MFMA2_N + 15) // 16 > 1024 and all((n + 15) // 16 <= 1024 for n in R.MFMA_N)
    worst = max(run_mvn(G, d, f, (False,), ns) for f in families_at(d, 113))
    report("k_logp_mvn_mfma d=%d" % d, worst)


# nrt > 8 (d > 128) and fewer than 512 points (or DZ_LOGP_GEMM=0): k_logp_mvn_mfma_tiled<2, 4> + k_q_finish
@pytest.mark.parametrize("d,family", [(d, f) for d in R.TILED_D for f in families_at(d, 129)])
def test_k_logp_mvn_mfma_tiled(G, d, family):
    assert all(n < 512 for n in R.TILED_N)
    report("k_logp_mvn_mfma_tiled d=%d family %s" % (d, family), run_mvn(G, d, family, (False, True), R.TILED_N))


@pytest.mark.parametrize("d", [d for d in R.TILED_D if d <= 257])
def test_k_logp_mvn_mfma_tiled_with_the_gemm_switched_off(G, d, monkeypatch):
    worst = max(run_mvn(G, d, f, (False, True), (600,), monkeypatch, "0") for f in ("a", "b", "c"))
    report("k_logp_mvn_mfma_tiled (DZ_LOGP_GEMM=0) d=%d" % d, worst)


def gemm_thresholds(d, num_cu):
    """the smallest n at which eval_logp picks 64 and 128 points per block: ceil(n / 64) nbn >= 5 CUs, ceil(n / 128) nbn >= 5 CUs, nbn = ceil(16 ceil(d / 16) / 64)"""
    nbn = (16 * ((d + 15) // 16) + 63) // 64
    need = (5 * num_cu + nbn - 1) // nbn                # blocks of points
    return 64 * (need - 1) + 1, 128 * (need - 1) + 1


# nrt > 8 and n >= 512: k_logp_mvn_gemm<1 | 2 | 4> (32 / 64 / 128 points per block, the largest that leaves five blocks per CU) + k_q_finish
@pytest.mark.parametrize("d,family", [(d, f) for d in R.GEMM_D for f in families_at(d, 129)])
def test_k_logp_mvn_gemm_32_points_per_block(G, d, family, num_cu):
    n2, n4 = gemm_thresholds(d, num_cu)
    assert all(512 <= n < n2 for n in R.GEMM_N)
    report("k_logp_mvn_gemm<1> d=%d family %s" % (d, family), run_mvn(G, d, family, (False, True), R.GEMM_N))


@pytest.mark.parametrize("family", ["a", "b", "c"])
@pytest.mark.parametrize("bm", [64, 128])
def test_k_logp_mvn_gemm_64_and_128_points_per_block(G, bm, family, num_cu):
    """d = 129, the first n that makes eval_logp choose the tile (from the device's own CU count) and one that does not fill the last block"""
    n2, n4 = gemm_thresholds(129, num_cu)
    assert 512 < n2 < n4 < (1 << 22)
    ns = (n2, n2 + 70) if bm == 64 else (n4, n4 + 130)
    assert ns[1] < n4 or bm == 128
    report("k_logp_mvn_gemm<%d> d=129 family %s n=%d, %d (%d CUs)" % (bm // 32, family, ns[0], ns[1], num_cu), run_mvn(G, 129, family, (False, True), ns))


# priors set beside an MVN: k_prior_only<NCH> after the likelihood kernel;  the mixture: k_logp_mix<NCH> makes both (NCH: 128-dimension chunks, 1 / 2 / 4 / 8)
@pytest.mark.parametrize("pattern", R.PRIOR_PATTERNS)
@pytest.mark.parametrize("d", R.PRIOR_D)
def test_k_prior_only_and_k_logp_mix(G, d, pattern):
    kind, a, b = R.priors(d, pattern)
    X, tags = R.prior_points(d, kind, a, b, n=67)
    pref, pbound = R.prior(X, kind, a, b)
    assert (np.isneginf(pref) == (tags == "out")).all() and ((tags == "out").any() or not (kind == 2).any())
    e = G.Engine(nchains=4, ndim=d, history_capacity=8)
    e.profile_enable(True)
    e.set_prior(kind, a, b)
    worst = {"k_prior_only": 0.0, "k_logp_mix prior": 0.0, "k_logp_mix": 0.0, "mvn beside": 0.0}
    P, Uf = R.matrices("a" if d <= 257 else "b", d)
    mu = R.mean(d, False)
    e.set_likelihood_mvn(mu, Uf, 1, R.log_f(d))
    pr, lk = eval_once(e, X)
    worst["k_prior_only"] = R.check(pr, pref, pbound, "k_prior_only d=%d %s" % (d, pattern))
    if pattern == "flat":
        assert not pr.any()
    ref, bound = R.mvn(X, mu, Uf, R.log_f(d), True)
    worst["mvn beside"] = R.check(lk, ref, bound, "mvn beside the priors d=%d" % d)
    for J in R.MIX_J:
        mus, F = R.mixtures(d, J, 5.0)
        e.set_likelihood_mixture(mus, F)
        pr, lk = eval_once(e, X)
        worst["k_logp_mix prior"] = max(worst["k_logp_mix prior"], R.check(pr, pref, pbound, "k_logp_mix's prior d=%d %s J=%d" % (d, pattern, J)))
        ref, bound = R.mixture(X, mus, F)[:2]
        worst["k_logp_mix"] = max(worst["k_logp_mix"], R.check(lk, ref, bound, "k_logp_mix d=%d %s J=%d" % (d, pattern, J)))
    e.close()
    for k, v in worst.items():
        report("%s d=%d %s" % (k, d, pattern), v)


@pytest.mark.parametrize("d", R.PRIOR_D)
def test_k_logp_mix_on_the_mixture_points(G, d):
    """no priors: centres 0.5 and 5 apart, points on a centre, on an exact tie, and where every other component underflows"""
    e = G.Engine(nchains=4, ndim=d, history_capacity=8)
    e.profile_enable(True)
    worst = 0.0
    for J in R.MIX_J:
        for sep in R.MIX_SEP:
            mus, F = R.mixtures(d, J, sep)
            X, tags = R.mixture_points(d, mus, n=67)
            e.set_likelihood_mixture(mus, F)
            pr, lk = eval_once(e, X)
            assert not pr.any()
            ref, bound = R.mixture(X, mus, F)[:2]
            worst = max(worst, R.check(lk, ref, bound, "k_logp_mix d=%d J=%d sep=%g" % (d, J, sep)))
    e.close()
    report("k_logp_mix d=%d" % d, worst)


FIRST_SRC = r"""
#include <hip/hip_runtime.h>
extern "C" __global__ __launch_bounds__(256) void first_coordinate(const double* X, long long n, int d, int ld, double* like, const void* data)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) like[i] = X[(size_t)i * ld];
}
"""


# a user's kernel as the likelihood: the engine zeroes prior[], runs the kernel, then k_prior_add<NCH> adds the built-in priors
@pytest.mark.parametrize("d", [4, 129])
def test_k_prior_add(G, d):
    from pydream_amd.likelihoods import compile_device_kernel
    obj = compile_device_kernel(FIRST_SRC)
    kind, a, b = R.priors(d, "mixed")
    X, tags = R.prior_points(d, kind, a, b, n=67)
    pref, pbound = R.prior(X, kind, a, b)
    e = G.Engine(nchains=4, ndim=d, history_capacity=8)
    e.profile_enable(True)
    e.set_prior(kind, a, b)
    e.set_likelihood_module(obj, "first_coordinate", 1, None, False)
    pr, lk = eval_once(e, X)
    worst = R.check(pr, pref, pbound, "k_prior_add d=%d" % d)
    np.testing.assert_array_equal(lk, X[:, 0])
    assert np.isneginf(pr).any()
    e.close()
    report("k_prior_add d=%d" % d, worst)


# ------------------------------------------------------------------------------------------------------------------ part B: the sampler's copies
GENS, THIN = 12, 5


def sampler_priors(d, which):
    """-> (kind, a, b, mins, maxs) or None.  'mixed': every kind, hard boundaries on the uniform dimensions' supports (no whole proposal set can be
    impossible: the instantiations with the full proposal code, not their redraw variants); 'uniform': all uniform, boundaries = supports (the
    constant-prior path); 'normal': all normal, no boundaries; 'flat': priors set, all flat"""
    if which is None:
        return None
    if which == "normal":
        kind, a, b = R.priors(d, "mixed")
        return np.ones(d, np.int32), a, b, None, None
    kind, a, b = R.priors(d, which)
    if which == "flat":
        return kind, a, b, None, None
    mins = np.where(kind == 2, a, -1.0e6)
    maxs = np.where(kind == 2, a + b, 1.0e6)
    return kind, a, b, mins, maxs


def starts(d, n, pri, centre, key):
    """n points inside every support: uniform dimensions uniformly, the others around `centre'"""
    rng = np.random.default_rng([991, d, n, key])
    X = centre[None, :] + rng.normal(size=(n, d))
    if pri is not None:
        kind, a, b = pri[:3]
        X = np.where(kind[None, :] == 2, a + b * rng.uniform(0.0, 1.0, (n, d)), X)
    return X


def sampler_run(G, N, d, like, pri=None, k=5, check_gens=None, variant=None, monkeypatch=None, env=None):
    """like: ("mvn", family, tri, zero) or ("mix", J, sep).  -> worst ratios {what: value} of the traced log p and of get_state()'s halves"""
    for name, val in (env or {}).items():
        monkeypatch.setenv(name, val)
    P = sampler_priors(d, pri)
    if like[0] == "mvn":
        _, family, tri, zero = like
        Pm, Uf = R.matrices(family, d)
        M, mu = (Uf if tri else Pm), R.mean(d, zero)
        centre = mu
        like_ref = lambda X: R.mvn(X, mu, M, R.log_f(d), tri)
    else:
        _, J, sep = like
        mus, F = R.mixtures(d, J, sep)
        centre = mus[0]
        like_ref = lambda X: R.mixture(X, mus, F)[:2]
    M0 = max(10 * d, 2 * N)
    Z0 = starts(d, M0, P, centre, 1)
    X0 = starts(d, N, P, centre, 2)
    if like[0] == "mix":
        X0[1::2] += (mus[-1] - mus[0])[None, :] * (P is None)         # (every other chain at the last centre, where no support forbids it)
    hard = P is not None and P[3] is not None
    e = G.Engine(nchains=N, ndim=d, multitry=k, history_thin=THIN, hardboundaries=1 if hard else 0, seed=1000 + d + N,
                 history_capacity=M0 + N * (GENS // THIN + 2), trace_capacity=GENS)
    if P is not None:
        e.set_prior(*P[:3])
        if hard:
            e.set_bounds(P[3], P[4])
    e.set_history(Z0)
    if like[0] == "mvn":
        e.set_likelihood_mvn(mu, M, int(tri), R.log_f(d))
    else:
        e.set_likelihood_mixture(mus, F)
    e.set_state(X0)
    e.step(GENS)
    got_variant = e.last_kernel_variant()
    tr = e.get_trace(0, GENS)
    Xs, lp, ll = e.get_state()
    e.close()
    if variant is not None:
        assert re.fullmatch(variant, got_variant), "ran as %s, expected %s" % (got_variant, variant)
    assert tr["moved"].any(), "no chain moved"
    np.testing.assert_array_equal(Xs, tr["X"][-1])

    def prior_ref(X):
        if P is None:
            z = np.zeros(len(X), np.longdouble)
            return z, z
        return R.prior(X, *P[:3])

    out = {}
    gens = list(range(GENS)) if check_gens is None else list(check_gens)
    pts = tr["X"][gens].reshape(-1, d)
    uniq, inv = np.unique(pts, axis=0, return_inverse=True)          # (a chain that stayed put repeats its state: one reference value per distinct state, every traced value compared)
    inv = inv.reshape(-1)
    (pr, pb), (lr, lb) = prior_ref(uniq), like_ref(uniq)
    out["trace"] = R.check(tr["logp"][gens].reshape(-1), (pr + lr)[inv], (pb + lb)[inv], "traced log p (%s)" % got_variant)
    (pr, pb), (lr, lb) = prior_ref(Xs), like_ref(Xs)
    out["lprior"] = R.check(lp, pr, pb, "get_state's log prior (%s)" % got_variant)
    out["llike"] = R.check(ll, lr, lb, "get_state's log likelihood (%s)" % got_variant)
    if P is None or pri == "flat":
        assert not lp.any()
    assert np.isfinite(tr["logp"]).all()
    print("%-50s N=%d d=%d %s priors=%s: worst error / bound  trace %.3f  prior %.3f  likelihood %.3f" % (got_variant, N, d, like, pri, out["trace"], out["lprior"], out["llike"]))
    return out


def form(tri):
    return "tri" if tri else "dense"


@pytest.mark.parametrize("tri", [1, 0])
def test_k_generations_headline_instantiations(G, tri):
    """4096 chains x 100-D x 5 tries, flat priors: 16 chains per block, the try count compiled in -- what bench.py times; generations 0 and 11"""
    sampler_run(G, 4096, 100, ("mvn", "a", tri, False), check_gens=(0, GENS - 1), variant=r"k_generations<7,%s,x(lds|hbm),16,1,lean>" % form(tri))


# 2304 chains: 12 per block on 256 CUs; 300 chains: 4 per block with 4 waves per chain -- without priors that is k_generations_w4
@pytest.mark.parametrize("pri,tri", [(None, 1), (None, 0), ("mixed", 1), ("mixed", 0), ("uniform", 1)])
@pytest.mark.parametrize("N", [2304, 300])
@pytest.mark.parametrize("d", R.GEN_D)
def test_k_generations(G, N, d, pri, tri):
    code = "lean" if pri is None else "full"
    fam = r"k_generations(_w4)?" if (N == 300 and pri is None) else "k_generations"
    sampler_run(G, N, d, ("mvn", "a", tri, False), pri=pri, variant=r"%s<%d,%s,x(lds|hbm),\d+,\d+,%s(,ahead)?>" % (fam, R.row_tiles_of(d), form(tri), code))


@pytest.mark.parametrize("d", R.GEN_D_MORE)
def test_k_generations_other_row_tile_counts(G, d):
    sampler_run(G, 2304, d, ("mvn", "a", 1, True), pri="mixed", variant=r"k_generations<%d,tri,xlds,\d+,\d+,full>" % R.row_tiles_of(d))


@pytest.mark.parametrize("tri", [1, 0])
@pytest.mark.parametrize("N", [1024, 260])
@pytest.mark.parametrize("d", R.W4_D)
def test_k_generations_w4(G, N, d, tri):
    sampler_run(G, N, d, ("mvn", "a", tri, False), variant=r"k_generations_w4<%d,%s,xlds,4,4,lean,ahead>" % (R.row_tiles_of(d), form(tri)))


# 128 < d <= 256 with the triangular factor (and d <= 128 where 16 chains' tiles do not fit beside the matrix): k_generations_d2, forced at these chain counts by DZ_MEGA_D2=2
@pytest.mark.parametrize("N", [80, 250])
@pytest.mark.parametrize("d", R.D2_D)
def test_k_generations_d2(G, N, d, monkeypatch):
    # (d <= 128: at five tries 16 chains still fit beside the packed triangle and the classic kernels run; eight tries do not)
    sampler_run(G, N, d, ("mvn", "a", 1, False), k=5 if d > 128 else 8, variant=r"k_generations_d2<%d,tri,xhbm,\d+,\d+,lean(,two-pass)?>" % R.row_tiles_of(d), monkeypatch=monkeypatch, env={"DZ_MEGA_D2": "2"})


@pytest.mark.parametrize("d", R.D2_D_MORE)
def test_k_generations_d2_other_row_tile_counts(G, d, monkeypatch):
    sampler_run(G, 80, d, ("mvn", "a", 1, True), variant=r"k_generations_d2<%d,tri,xhbm,\d+,\d+,lean(,two-pass)?>" % R.row_tiles_of(d), monkeypatch=monkeypatch, env={"DZ_MEGA_D2": "2"})


def test_k_generations_d2_nine_tries(G, monkeypatch):
    sampler_run(G, 250, 256, ("mvn", "a", 1, False), k=9, variant=r"k_generations_d2<16,tri,xhbm,\d+,\d+,lean,two-pass>", monkeypatch=monkeypatch, env={"DZ_MEGA_D2": "2"})


def test_k_generations_d2_normal_priors(G, monkeypatch):
    sampler_run(G, 250, 160, ("mvn", "a", 1, False), pri="normal", variant=r"k_generations_d2<10,tri,xhbm,\d+,\d+,full>", monkeypatch=monkeypatch, env={"DZ_MEGA_D2": "2"})


@pytest.mark.parametrize("pri", [None, "mixed"])
@pytest.mark.parametrize("J", [2, 3])
@pytest.mark.parametrize("d", R.MIX_D)
def test_k_generations_mix(G, d, J, pri):
    fields = ",".join(f for f in ("full" if pri else "", "wide" if d > 128 else "") if f)
    sampler_run(G, 256, d, ("mix", J, 5.0), pri=pri, variant="k_generations_mix" + ("<%s>" % fields if fields else ""))


def test_k_generations_mix_one_try(G):
    sampler_run(G, 256, 100, ("mix", 3, 0.5), k=1, variant="k_generations_mix")


# DZ_MEGA=0: k_propose makes the proposals' priors (prior_of_point), the likelihood kernels of part A run on the proposal sets, and at d > 128 the
# row-tile sums are added by the kernels that consume them (no k_q_finish launch)
@pytest.mark.parametrize("tri", [1, 0])
@pytest.mark.parametrize("d", R.MULTI_D)
def test_multi_kernel_path(G, d, tri, monkeypatch):
    sampler_run(G, 64, d, ("mvn", "a", tri, False), pri="mixed", variant="multi-kernel path", monkeypatch=monkeypatch, env={"DZ_MEGA": "0"})
