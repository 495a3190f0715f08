"""The sampler's decisions on NaN, +inf and -inf log densities, on the GPU.

Part A: the engine's own device functions -- dz::mt_select_vals and dz::mt_log_ratio in their three forms (run-time k; BIG, more than 16
tries with the reference terms from lane 32; the try count compiled in, K = 3, 5, 16) and the single-try expressions written with
dz::nan_to_num and dz::is_finite -- over every row of tests/nonfinite_rule.py's table, against its plain twin: sel, accept, the
"a finite try exists" flag and all 64 bits of ratio.  A test-side kernel (a wave per row) includes the engine's headers the way
DeviceFunctionLogLike's translation unit does, lays the lanes out as the callers do (tries in lanes 0..k-1, B terms at mt_boff(k) + i,
-inf elsewhere; the snooker terms added as in k_accept) and is driven through dz_set_likelihood_module / dz_eval_logp: X[i] = (row,
quantity, form), the table in the data block, like[i] a finite encoding of the answer (ratio as its two 32-bit words).

Part B: every copy of the rule inside a running sampler -- tests/module_kernels.py's poison variants (NaN, +inf, -inf in bands of
frac(x[0])) on the multi-kernel path and in k_generations_user, chains seeded through set_state with NaN, +inf and -inf log densities,
and the persistent built-in kernels poisoned through their initial state -- against the oracle, bit for bit (trace, archive, crossover
state, final state).  tests/test_nonfinite_rule_cpu.py checks on the oracle's runs alone that each configuration really holds
chain-generations starting from +inf, -inf and NaN.

Seen to fail with an untouched engine.  Part A, the TWIN perturbed: nan_to_num(+inf) -> +inf turns every k red (ratio bits and accept: each
table holds rows whose sums divide to inf, asserted on the CPU); accepting without the isfinite test the k = 1 rows (the only place a ratio
is not finite); a selection that defaults to try 0 instead of k-1 every k > 1.  Part B compares with the ORACLE, which
tests/test_nonfinite_rule_cpu.py pins to the twin, so there the same three changes were made in a copy of the oracle: nan_to_num turns red
every single-try case (multi-kernel path, k_generations_user, the k1 instantiations of k_generations, k_generations_d2 and
k_generations_mix), nearly all multi-try user-kernel cases, and k_generations' run-time-k, dense and REDO cases; the isfinite test the
single-try user-kernel cases and both k_generations_user cases; the selection default every multi-try user-kernel case.  What part B
cannot reach: the built-in densities are never +inf or NaN, so inside k_generations<KC>, k_generations_w4, k_generations_d2 and
k_generations_mix at several tries no selection weight is NaN and no weight sum divides to inf in these runs -- those copies are the device
functions of part A, which covers them row by row; the kernels' own part (operands, lanes, the single-try formulas, D1) is what part B adds.
Two tries exist in part A only: both engines refuse multitry = 2 (deviation D4).
"""
import numpy as np
import pytest

from tests import nonfinite_rule as R

pytestmark = pytest.mark.gpu

# ------------------------------------------------------------------------------------------------------------------ part A: the kernel
# data block: [nrows, k, stride, 0 | rows], a row = [snooker, u_sel, u_acc, cur_snk | lp[k] | B[k] | slp[k] | slr[k]]
# quantity: 0 sel, 1 accept, 2 / 3 the high / low word of ratio, 4 anyfinite;  form: 0 run-time k, 1 BIG, 2 compile-time K, 3 single try
RULE_SRC = r"""
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstddef>
#include "dz_device.h"
#define DZ_TEMPLATES_ONLY
#include "dz_kernels.h"
#undef DZ_TEMPLATES_ONLY

extern "C" __global__ __launch_bounds__(256) void nf_rule(const double* X, long long n, int d, int ld, double* like, const void* data)
{
    const long long i = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (i >= n) return;                                            // (the whole wave)
    const double* hd = (const double*)data;
    const long long nrows = (long long)hd[0];
    const int k = (int)hd[1], stride = (int)hd[2];
    const double* x = X + (size_t)i * ld;
    const long long row = (long long)x[0];
    const int what = (int)x[1], form = (int)x[2];
    const double ninf = -__builtin_huge_val();
    double out = -1.0;
    const bool known = form == 3 ? k == 1 : (k >= 2 && (form == 1 ? k <= 32 : form == 0 ? k <= 16 : form == 2 && (k == 3 || k == 5 || k == 16)));
    if (row >= 0 && row < nrows && known && stride == 4 + 4 * k) {
        const double* r = hd + 4 + (size_t)row * stride;
        const bool snk = r[0] != 0.0;
        const double u_sel = r[1], u_acc = r[2], cur = r[3];
        const double *lp = r + 4, *B = lp + k, *slp = B + k, *slr = slp + k;
        int sel = 0; bool fin = true; double ratio, lu;
        if (form == 3) {
            const double q_logp = lp[0], last_logp = B[0];
            if (snk) ratio = dz::nan_to_num((q_logp + slp[0]) - (last_logp + cur));
            else ratio = dz::nan_to_num(q_logp) - dz::nan_to_num(last_logp);
            lu = dz::dlog(u_acc);
        } else {
            const int boff = form == 1 ? dz::mt_boff(k) : 16;
            const double l = lane < k ? lp[lane] : ninf;
            double val = ninf;
            if (lane < k) { val = lp[lane]; if (snk) val = val + slp[lane]; }
            else if (lane >= boff && lane < boff + k) {
                const int t = lane - boff;
                val = B[t];
                if (snk) { const double sr = t < k - 1 ? slr[t] : 0.0; val = (val + sr) + slp[t]; }
            }
            if (form == 0) { sel = dz::mt_select_vals<false>(k, l, u_sel, lane, &fin); ratio = dz::mt_log_ratio<false>(k, val, u_acc, lane, &lu); }
            else if (form == 1) { sel = dz::mt_select_vals<true>(k, l, u_sel, lane, &fin); ratio = dz::mt_log_ratio<true>(k, val, u_acc, lane, &lu); }
            else if (k == 3) { sel = dz::mt_select_vals<3>(l, u_sel, lane, &fin); ratio = dz::mt_log_ratio<3>(val, u_acc, lane, &lu); }
            else if (k == 5) { sel = dz::mt_select_vals<5>(l, u_sel, lane, &fin); ratio = dz::mt_log_ratio<5>(val, u_acc, lane, &lu); }
            else { sel = dz::mt_select_vals<16>(l, u_sel, lane, &fin); ratio = dz::mt_log_ratio<16>(val, u_acc, lane, &lu); }
        }
        const bool accept = dz::is_finite(ratio) && (lu < ratio);
        const unsigned long long b = (unsigned long long)__double_as_longlong(ratio);
        out = what == 0 ? (double)sel : what == 1 ? (accept ? 1.0 : 0.0) : what == 2 ? (double)(unsigned)(b >> 32) : what == 3 ? (double)(unsigned)(b & 0xffffffffull)
            : what == 4 ? (fin ? 1.0 : 0.0) : -1.0;
    }
    if (lane == 0) like[i] = out;
}
"""

FORMS = {1: (3,), 2: (0, 1), 3: (0, 1, 2), 5: (0, 1, 2), 16: (0, 1, 2), 17: (1,), 24: (1,)}
FORM_NAMES = {0: "run-time k", 1: "BIG", 2: "compile-time K", 3: "single try"}


def rule_object():
    from pydream_amd.likelihoods import compile_device_kernel, csrc_dir
    return compile_device_kernel(RULE_SRC, extra_flags=("-I" + csrc_dir(), "-Wno-unused-value", "-Wno-unused-result"))


def rule_data(t):
    k = t.k
    rows = np.concatenate([t.snk[:, None].astype(float), t.u_sel[:, None], t.u_acc[:, None], t.cur[:, None], t.lp, t.B, t.slp, t.slr], axis=1)
    assert rows.shape == (t.n, 4 + 4 * k)
    return np.concatenate([[float(t.n), float(k), float(4 + 4 * k), 0.0], rows.ravel()])


@pytest.mark.parametrize("k", sorted(FORMS))
def test_device_functions_decide_like_the_twin(k):
    from pydream_amd import _capi as G
    t = R.table(k)
    sel, ratio, accept = t.decide_all("skip")
    rb = R.bits(ratio)
    want = {0: sel.astype(float), 1: accept.astype(float), 2: (rb >> np.uint64(32)).astype(float), 3: (rb & np.uint64(0xffffffff)).astype(float),
            4: np.ones(t.n) if k == 1 else np.isfinite(t.lp).any(axis=1).astype(float)}
    e = G.Engine(nchains=3, ndim=3, history_capacity=8)
    e.set_likelihood_module(rule_object(), "nf_rule", 64, rule_data(t), False)
    X = np.zeros((t.n, 3)); X[:, 0] = np.arange(t.n)
    for form in FORMS[k]:
        X[:, 2] = form
        for what in range(5):                                      # one launch per quantity
            X[:, 1] = what
            prior, like = e.eval_logp(X)
            assert not prior.any()
            bad = np.nonzero(like != want[what])[0]
            assert len(bad) == 0, "k=%d %s, quantity %d: %d rows differ, first row %d: lp %s B %s snooker %d: engine %r, twin %r" % (
                k, FORM_NAMES[form], what, len(bad), bad[0], t.lp[bad[0]], t.B[bad[0]], t.snk[bad[0]], like[bad[0]], want[what][bad[0]])
    X[:, 0] = t.n; X[:, 1] = 0                                     # (a row number past the table is answered, not read)
    assert (e.eval_logp(X[:5])[1] == -1.0).all()
    e.close()


# ------------------------------------------------------------------------------------------------------------------ part B: running samplers
def _hip_run(c):
    from pydream_amd import _capi as G
    from tests import module_kernels as MK
    if c["kind"] == "module":
        MK.code_object(c["lk"])
    return R.run_sampler(G.Engine, c)


@pytest.mark.parametrize("lk,k,prior,snk", R.MODULE_CASES)
def test_poisoned_user_kernels_on_the_multi_kernel_path(lk, k, prior, snk):
    """k_accept's copy of the rule (mt_select_vals<true> / mt_log_ratio<true>, BIG at 17 tries; the single-try formula and its snooker
    form), the redraw rounds' "no finite try" test, k_prior_add's NaN -> -inf -- with the user kernel returning NaN, +inf and -inf in bands
    and a third of the chains STARTING from such a state; under the open uniform prior -inf + +inf makes NaN log densities"""
    c = R.module_case(lk, k, prior, snk)
    got, want = _hip_run(c), R.oracle_run(c)
    R.assert_same(got, want)
    assert got["variants"] == ["multi-kernel path"] * 2, got["variants"]
    if k > 1 and prior == "uniform_open":
        assert got["redraws"] > 0                                  # (whole proposal sets without a finite try occurred: redraw rounds)


@pytest.mark.parametrize("name", sorted(R.FUNCTION_CASES))
def test_poisoned_device_function(name):
    """generations_wave_body's copy of the rule inside k_generations_user (a single try: no redraw rounds whatever the promise), and the
    function's batch kernel on the multi-kernel path at three tries"""
    c = R.FUNCTION_CASES[name]
    got, want = _hip_run(c), R.oracle_run(c)
    R.assert_same(got, want)
    assert got["variants"] == [name] * 2, got["variants"]


@pytest.mark.parametrize("name", sorted(R.BUILTIN_CASES))
def test_poisoned_states_in_the_persistent_kernels(name):
    """every persistent built-in kernel's copy: chains 0, 1, 2 of every nine start from NaN, +inf, -inf (set_state), four archive rows hold
    +-1e200 and +-1e308, so that DE differences and quadratic forms overflow to inf and NaN (then -inf) in some tries -- next to tries of
    other chains in the same MFMA tiles, which must not notice"""
    c, variant, tries = R.BUILTIN_CASES[name]
    got, want = _hip_run(c), R.oracle_run(c)
    assert all(variant in v if variant.startswith(",") else v.startswith(variant) for v in got["variants"]), got["variants"]
    assert got["tries"] == [tries] * 2, got["tries"]
    R.assert_same(got, want)
