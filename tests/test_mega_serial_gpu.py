"""The persistent kernel's serial phases -- the multi-try selection and the multi-try ratio (dz::mt_select_vals<5>, dz::mt_log_ratio<5>: ordered
in-row prefix sums, one compare mask for the selection) with the branch-free dz::dexp / dz::dlog under them -- on the GPU, bit for bit.

Part A: the device functions themselves.  A test-side kernel (a wave per point, driven through dz_set_likelihood_module / dz_eval_logp the
way tests/test_nonfinite_gpu.py drives its own) evaluates dz::dexp and dz::dlog on tests/serial_cases.py's arguments -- every special case,
both sides of every threshold, signalling and payload NaNs, random bit patterns -- against the oracle's orc_exp / orc_log, all 64 bits;
and dz::row_prefix_ordered<K>, K = 1..16, on two rows of 16 lanes at once against the sequential left-to-right sum.  (The selection and
the ratio as wholes, K = 3, 5, 16, over the non-finite table: tests/test_nonfinite_gpu.py part A.)

Part B: k_generations<.., KC = 5> against the oracle, against the instantiation that reads the try count at run time (DZ_MEGA_KC=0: the
generic forms of the two functions, which keep their scalar sums) and against the multi-kernel path (DZ_MEGA=0): trace states, log p, the
five decision columns, the archive and the chains' final log prior / log likelihood.  Chain count, thin, pieces and launch counts are those
of tests/test_mega_kc_gpu.py.  d = 97, 100, 112 (the three row lengths of seven row tiles) x triangular / dense x history lag 0 / 3 x
snooker 0.1 / 1.0 (at 1.0 every chain adds the snooker log densities, whose dlog runs in every chain) x the two targets of
tests/serial_cases.py: STEEP (weights underflow to exact 0, SA / SB hits 0 and +inf) and FLAT (all tries tie to the last bit).  That the
oracle alone takes those paths with these inputs is asserted on the CPU, tests/test_serial_primitives_cpu.py."""
import re

import numpy as np
import pytest

from tests import helpers as H
from tests import serial_cases as S
from tests import test_mega_kc_gpu as KC

pytestmark = pytest.mark.gpu

# ------------------------------------------------------------------------------------------------------------------ part A: the device functions
# data block: [n, 0 | values]; a point X[i] = (index, what, K, lane):  what 0 / 1: high / low word of dexp(values[index]);  2 / 3: of dlog;
# 4 / 5: of lane `lane` (0..31) of row_prefix_ordered<K> over the 32 values from 32 * index on (lanes 32..63 hold +0.0)
PRIM_SRC = r"""
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstddef>
#include "dz_device.h"

template <int K>
__device__ double prefix_or_next(int k, double w) { if (k == K) return dz::row_prefix_ordered<K>(w); if constexpr (K < 16) return prefix_or_next<K + 1>(k, w); else return w; }

extern "C" __global__ __launch_bounds__(256) void serial_prim(const double* X, long long n, int d, int ld, double* like, const void* data)
{
    const long long i = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (i >= n) return;                                            // (the whole wave)
    const double* hd = (const double*)data;
    const long long nv = (long long)hd[0];
    const double* x = X + (size_t)i * ld;
    const long long idx = (long long)x[0];
    const int what = (int)x[1], K = (int)x[2], ln = (int)x[3];
    double out = -1.0;
    if (what >= 0 && what <= 3 && idx >= 0 && idx < nv) {
        const double v = hd[2 + idx];
        const double r = what < 2 ? dz::dexp(v) : dz::dlog(v);
        const unsigned long long b = (unsigned long long)__double_as_longlong(r);
        out = (what & 1) ? (double)(unsigned)(b & 0xffffffffull) : (double)(unsigned)(b >> 32);
    } else if ((what == 4 || what == 5) && idx >= 0 && 32 * idx + 32 <= nv && K >= 1 && K <= 16 && ln >= 0 && ln < 32) {
        const double w = lane < 32 ? hd[2 + 32 * idx + lane] : 0.0;
        const double c = prefix_or_next<1>(K, w);                  // (K is the same in the whole wave)
        const double r = dz::readlane_f64(c, __builtin_amdgcn_readfirstlane(ln));
        const unsigned long long b = (unsigned long long)__double_as_longlong(r);
        out = what == 5 ? (double)(unsigned)(b & 0xffffffffull) : (double)(unsigned)(b >> 32);
    }
    if (lane == 0) like[i] = out;
}
"""


def prim_engine(values):
    from pydream_amd import _capi as G
    from pydream_amd.likelihoods import compile_device_kernel, csrc_dir
    obj = compile_device_kernel(PRIM_SRC, extra_flags=("-I" + csrc_dir(), "-Wno-unused-value", "-Wno-unused-result"))
    e = G.Engine(nchains=3, ndim=4, history_capacity=8)
    e.set_likelihood_module(obj, "serial_prim", 64, np.concatenate([[float(len(values)), 0.0], values]), False)
    return e


def words(e, X, what_hi):
    X = X.copy()
    X[:, 1] = what_hi
    prior, hi = e.eval_logp(X)
    assert not prior.any()
    X[:, 1] = what_hi + 1
    lo = e.eval_logp(X)[1]
    assert (hi >= 0).all() and (lo >= 0).all()
    return (hi.astype(np.uint64) << np.uint64(32)) | lo.astype(np.uint64)


@pytest.fixture(scope="module")
def O():
    from oracle import oracle
    return oracle


def test_dexp_and_dlog_give_the_oracles_bits_for_every_kind_of_argument(O):
    v = S.elementary_inputs()
    e = prim_engine(v)
    X = np.zeros((len(v), 4)); X[:, 0] = np.arange(len(v))
    for what, fn, name in ((0, O.exp, "dexp"), (2, O.log, "dlog")):
        got = words(e, X, what)
        want = S.bits(np.array([fn(x) for x in v]))
        bad = np.nonzero(got != want)[0]
        assert len(bad) == 0, "%s: %d of %d arguments differ, first %r (%#018x): device %#018x, oracle %#018x" % (
            name, len(bad), len(v), v[bad[0]], S.bits(v)[bad[0]], got[bad[0]], want[bad[0]])
    # the inputs reach every case: both cut-offs and the two-step scaling of dexp; NaN, negative, zero, +inf, subnormal and m > sqrt 2 of dlog
    assert (v > 709.782712893384).any() and (v < -745.2).any() and ((v < -693.2) & (v >= -745.2)).any() and np.isnan(v).any()
    assert (v < 0).any() and (v == 0).any() and (v == np.inf).any() and ((v > 0) & (v < 2.2250738585072014e-308)).any()
    e.close()


def test_row_prefix_ordered_is_the_sequential_sum_in_both_rows():
    rows = S.prefix_rows()
    e = prim_engine(rows.ravel())
    want = np.concatenate([S.sequential_prefix(rows[:, :16]), S.sequential_prefix(rows[:, 16:])], axis=1)
    pts = [(r, 0, K, 16 * row + i) for r in range(len(rows)) for K in range(1, 17) for row in (0, 1) for i in range(K)]
    X = np.array(pts, dtype=float)
    got = words(e, X, 4)
    ref = S.bits(want)[X[:, 0].astype(int), X[:, 3].astype(int)]
    bad = np.nonzero(got != ref)[0]
    assert len(bad) == 0, "%d of %d lanes differ, first: row %d K %d lane %d: device %#018x, sequential sum %#018x" % (
        len(bad), len(X), X[bad[0], 0], X[bad[0], 2], X[bad[0], 3], got[bad[0]], ref[bad[0]])
    e.close()


# ------------------------------------------------------------------------------------------------------------------ part B: the sampler
N, THIN, PIECES, LAUNCHES = KC.N, KC.THIN, KC.PIECES, KC.LAUNCHES


def run(Cls, d, kind, lag, snooker, target, seed, want=None):
    """-> outputs;  want = (variant pattern, tries, launches or None): a GPU run, which checks after each piece what its last launch ran as"""
    GENS = sum(PIECES[lag])
    Z0 = H.seed_history(max(10 * d, 64), d, seed)
    X0 = H.seed_history(N, d, seed + 1)
    e = Cls(nchains=N, ndim=d, multitry=5, history_thin=THIN, history_lag=lag, snooker=snooker, schedule=2, seed=seed,
            history_capacity=len(Z0) + N * (GENS // THIN + 2), trace_capacity=GENS)
    e.set_history(Z0)
    e.set_state(X0)
    S.set_target(e, d, kind, target)
    if want:
        e.profile_enable(True); e.profile_reset()
    for m in PIECES[lag]:
        e.step(m)
        if want:
            assert re.fullmatch(want[0], e.last_kernel_variant()), e.last_kernel_variant()
            assert e.last_kernel_tries() == (want[1] if ",16,1," in e.last_kernel_variant() else 0)      # (the try count is compiled in at 16 chains per block only)
    if want:
        if want[2] is not None:
            assert e.profile_get("generations")[1] == want[2]
        e.profile_enable(False)
    out = dict(history=e.get_history())
    out["X"], out["lprior"], out["llike"] = e.get_state()
    out.update({"trace_" + key: v for key, v in e.get_trace(0, GENS).items()})
    e.close()
    return out


@pytest.mark.parametrize("target", ["steep", "flat"])
@pytest.mark.parametrize("snooker", [0.1, 1.0])
@pytest.mark.parametrize("lag", [0, 3])
@pytest.mark.parametrize("kind", ["tri", "dense"])
@pytest.mark.parametrize("d", [97, 100, 112])
def test_serial_phases_against_oracle_generic_instantiation_and_multi_kernel_path(O, monkeypatch, d, kind, lag, snooker, target):
    from pydream_amd import _capi as G
    for name in ("DZ_MEGA", "DZ_MEGA_KC", "DZ_MEGA_SEGS"):
        monkeypatch.delenv(name, raising=False)
    segs = 2 if lag else None
    if lag:
        monkeypatch.setenv("DZ_MEGA_SEGS", "2")              # two history appends per launch, once three appends are made
    seed = 7500 + 13 * d + lag
    # the packed triangle leaves room for 16 chains' states in LDS at every d <= 112; what the dense square leaves room for is mega_layout's
    # business (d = 100: 16 chains with their states in HBM; d = 112: blocks of 8 chains, which read the try count at run time)
    variant = r"k_generations<7,tri,xlds,16,1,lean>" if kind == "tri" else r"k_generations<7,dense,(xlds|xhbm),(16|8),1,lean>"
    new = run(G.Engine, d, kind, lag, snooker, target, seed, (variant, 5, LAUNCHES[lag, segs]))
    ora = run(O.Engine, d, kind, lag, snooker, target, seed)
    KC.assert_identical(new, ora, "compiled-in try count against the oracle")
    monkeypatch.setenv("DZ_MEGA_KC", "0")
    gen = run(G.Engine, d, kind, lag, snooker, target, seed, (variant, 0, LAUNCHES[lag, segs]))
    monkeypatch.delenv("DZ_MEGA_KC")
    KC.assert_identical(new, gen, "compiled-in try count against DZ_MEGA_KC=0")
    monkeypatch.setenv("DZ_MEGA", "0")
    mk = run(G.Engine, d, kind, lag, snooker, target, seed, ("multi-kernel path", 0, None))
    monkeypatch.delenv("DZ_MEGA")
    KC.assert_identical(new, mk, "compiled-in try count against the multi-kernel path")
    snk = new["trace_snooker"].mean()
    assert snk == 1.0 if snooker == 1.0 else 0.05 < snk < 0.15
    if target == "flat":         # every ratio is log 1 = 0 without the snooker terms: every such step is accepted
        plain = new["trace_snooker"] == 0
        assert not plain.any() or new["trace_moved"][plain].mean() > 0.99
    else:                        # a certain accept or a certain reject, both occur
        assert 0.0 < new["trace_moved"].mean() < 1.0
    assert len(new["history"]) == max(10 * d, 64) + N * (sum(PIECES[lag]) // THIN + 1)          # every append was made
