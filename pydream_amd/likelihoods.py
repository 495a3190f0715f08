"""Built-in likelihoods that run on the device ("batched device callback").

Each object is an ordinary Python callable ``f(x[d]) -> float`` (so it also works with the
reference), and carries a descriptor that ``run_dream`` hands to ``dz_set_likelihood_*`` so the
evaluation happens inside the HIP kernels instead of on the host.
"""
import numpy as np

from . import _kernel_cache, _ode_source      # noqa: F401
from ._kernel_cache import _build_cached, _compiler_version, compile_device_kernel, csrc_dir, kernel_cache_dir      # noqa: F401
from ._ode_source import _LOG_2PI_HALF, _hill_slots, _indices_read, _rate, _rate_indices, _slot_indices
from ._ode_values import (ODE_EQUILIBRATE_MAX_STEPS, ODE_GROUP_LIMITS, ODE_LIMITS, ODE_MAX_CONDITIONS, ODE_MAX_CONSTRAINTS,      # noqa: F401
                          ODE_MAX_EVENTS, ODE_MAX_HILL_EXPONENT, ODE_MAX_INPUT_KNOTS, ODE_MAX_INPUTS, ODE_MAX_RATE_FACTORS, ODE_MAX_VIEW_COORDINATES,
                          ODE_SETTLE_MAX_STEPS, ODE_WAVE_LIMITS,
                          Hill, Input, Monomial, Noise, Normalize, RateLaw, _checked_constant, _is_int, _is_real)


class MVNormalLogLike:
    """log_F - 1/2 (x-mu)^T P (x-mu)  (pydream/examples/ndim_gaussian/dream_ex_ndim_gaussian.py:49-52).

    factorize=True hands the device the upper-triangular factor U of P = U^T U (half the work of the
    dense form; agrees with it to ~1e-12); factorize=False uses P itself."""

    def __init__(self, precision, mu=None, log_F=0.0, factorize=True):
        P = np.asarray(precision, dtype=float)
        self.d = P.shape[0]
        self.precision = P
        self.mu = np.zeros(self.d) if mu is None else np.asarray(mu, dtype=float)
        self.log_F = float(log_F)
        self.factorize = bool(factorize)
        self.U = np.linalg.cholesky((P + P.T) / 2.0).T if self.factorize else None

    def __call__(self, x):
        v = np.asarray(x, dtype=float) - self.mu
        return self.log_F - .5 * np.sum(v * np.dot(self.precision, v))

    def _dz_apply(self, engine):
        if self.factorize:
            engine.set_likelihood_mvn(self.mu, self.U, 1, self.log_F)
        else:
            engine.set_likelihood_mvn(self.mu, self.precision, 0, self.log_F)


class GaussianMixtureLogLike:
    """log sum_j exp(-1/2 |x - mu_j|^2 + log_F_j)  (pydream/examples/mixturemodel/mixturemodel.py:37-48)."""

    def __init__(self, mu, log_F):
        self.mu = np.atleast_2d(np.asarray(mu, dtype=float))
        self.log_F = np.asarray(log_F, dtype=float)
        self.d = self.mu.shape[1]

    @classmethod
    def from_weights(cls, mu, weights):
        mu = np.atleast_2d(np.asarray(mu, dtype=float))
        d = mu.shape[1]
        return cls(mu, np.log(np.asarray(weights, dtype=float)) - (d / 2.) * np.log(2 * np.pi))

    def __call__(self, x):
        log_lh = -.5 * np.sum((np.asarray(x, dtype=float) - self.mu) ** 2, axis=1) + self.log_F
        m = np.max(log_lh)
        return np.log(np.sum(np.exp(log_lh - m))) + m

    def _dz_apply(self, engine):
        engine.set_likelihood_mixture(self.mu, self.log_F)


KERNEL_SIGNATURE = 'extern "C" __global__ void NAME(const double* X, long long n, int d, int ld, double* like, const void* data)'



FUNCTION_SIGNATURE = '__device__ double NAME(const double* x, int d, const void* data, int lane)'

# The translation unit around a user's wave-level device function: the batch kernel the engine's multi-kernel path launches (one wave per
# point) and the persistent kernels -- csrc/dz_megakernel.h generations_wave_body, the kernel the built-in mixture runs in, with the user's
# function in the likelihood's place.  The names of the latter carry the layout generation of the structures they take (DZ_USER_ABI).
_FUNCTION_TU = r"""
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstddef>
#include "dz_device.h"
__device__ __forceinline__ double dz_wave_sum(double v) { return dz::wave_bfly(v); }      // the xor butterfly over the wave's 64 lanes: every lane gets the total
%(source)s
#define DZ_TEMPLATES_ONLY
#include "dz_kernels.h"
#undef DZ_TEMPLATES_ONLY
#include "dz_megakernel.h"
namespace dz {
struct UserLike {
    template <int NCH>
    DZ_DEV static void eval(const Params& p, const double* rows, int LDP, int n, int lane, double* lh, double* out)
    {
        for (int i = 0; i < n; ++i) {
            const double v = %(name)s(rows + (size_t)i * LDP, p.d, p.udata, lane);
            if (lane == 0) out[i] = nan_to_ninf(v);
        }
    }
};
}
#define DZ_USER_CAT2(a, b) a##b
#define DZ_USER_CAT(a, b) DZ_USER_CAT2(a, b)
extern "C" __global__ __launch_bounds__(1024) void DZ_USER_CAT(dz_user_generations_v, DZ_USER_ABI)(const dz::Params* __restrict__ pp, uint32_t g0, int ngen, uint32_t M0, int64_t trace_slot0,
                                                                                                     int64_t zappend, int seg0, dz::Publish pub)
{
    dz::generations_wave_body<false, false, dz::UserLike>(pp, g0, ngen, M0, trace_slot0, zappend, seg0, pub);
}
extern "C" __global__ __launch_bounds__(1024) void DZ_USER_CAT(dz_user_generations_full_v, DZ_USER_ABI)(const dz::Params* __restrict__ pp, uint32_t g0, int ngen, uint32_t M0, int64_t trace_slot0,
                                                                                                          int64_t zappend, int seg0, dz::Publish pub)
{
    dz::generations_wave_body<true, false, dz::UserLike>(pp, g0, ngen, M0, trace_slot0, zappend, seg0, pub);
}
// ... and for 128 < d <= 256 (a lane owns four dimensions of the chain's state)
extern "C" __global__ __launch_bounds__(1024) void DZ_USER_CAT(dz_user_generations_wide_v, DZ_USER_ABI)(const dz::Params* __restrict__ pp, uint32_t g0, int ngen, uint32_t M0, int64_t trace_slot0,
                                                                                                          int64_t zappend, int seg0, dz::Publish pub)
{
    dz::generations_wave_body<false, false, dz::UserLike, 2>(pp, g0, ngen, M0, trace_slot0, zappend, seg0, pub);
}
extern "C" __global__ __launch_bounds__(1024) void DZ_USER_CAT(dz_user_generations_wide_full_v, DZ_USER_ABI)(const dz::Params* __restrict__ pp, uint32_t g0, int ngen, uint32_t M0, int64_t trace_slot0,
                                                                                                               int64_t zappend, int seg0, dz::Publish pub)
{
    dz::generations_wave_body<true, false, dz::UserLike, 2>(pp, g0, ngen, M0, trace_slot0, zappend, seg0, pub);
}
extern "C" __global__ __launch_bounds__(256) void dz_user_batch(const double* X, long long n, int d, int ld, double* like, const void* data)
{
    const long long i = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (i >= n) return;
    const double v = %(name)s(X + (size_t)i * ld, d, data, lane);
    if (lane == 0) like[i] = v;
}
"""


class _UserKernelLogLike:
    """What the two likelihoods written by the user share: a call on the host goes to the Python twin `host` or, without one, evaluates
    the point on the device with an engine of the object's own, made on first use."""

    def __call__(self, x):
        if self.host is not None:
            return self.host(np.asarray(x, dtype=float))
        if self._eval_engine is None:
            from . import _capi
            self._eval_engine = _capi.Engine(nchains=3, ndim=self.d, history_capacity=8)
            self._dz_apply(self._eval_engine)
        return float(self._eval_engine.eval_logp(np.asarray(x, dtype=float).reshape(1, self.d))[1][0])

    def __getstate__(self):                      # (the evaluation engine is a device handle: not part of the object's value)
        st = dict(self.__dict__); st["_eval_engine"] = None
        return st


class DeviceFunctionLogLike(_UserKernelLogLike):
    """A user-written HIP DEVICE FUNCTION as the likelihood, evaluated by one wave per point -- and INSIDE the persistent generation kernel:

        SRC = '''
        __device__ double sphere(const double* x, int d, const void* data, int lane) {     // all 64 lanes call it; x: the point (d doubles)
            const double* c = (const double*)data;
            double acc = 0.0;
            for (int j = lane; j < d; j += 64) { const double t = x[j] - c[j]; acc += t * t; }
            return -0.5 * dz_wave_sum(acc);                                                // the same value in every lane
        }'''
        like = DeviceFunctionLogLike(SRC, "sphere", ndim=d, data=centre, always_finite=True)
        sampled, log_ps = run_dream(parameters, like, nchains=4096, multitry=5, ...)

    The function's signature is FUNCTION_SIGNATURE; x may point to LDS or global memory (d doubles; what follows them is not the
    function's to read); `dz_wave_sum(double)` (the xor butterfly over the wave's 64 lanes, every lane gets the total) and the helpers of
    csrc/dz_device.h (namespace dz) are in scope.  The source is compiled once (hipcc on first use, cached like compile_device_kernel's
    objects; the key includes the engine's own headers) into a code object with (a) a batch kernel for the engine's multi-kernel path and
    (b) the persistent kernels of csrc/dz_megakernel.h with this function in the place of the built-in mixture -- the same launches, the
    same bits as (a), at the persistent kernels' rate instead of the multi-kernel path's.  They run where the mixture's would: d <= 256,
    multitry 1 or 3..32 tries, and always_finite=True (a density that may be -inf for a whole proposal set needs the multi-kernel path's
    redraw rounds, Dream.py:281-289).  host: an optional Python twin f(x[d]) -> float for calls on the host (Model.total_logp)."""

    def __init__(self, source, name, ndim, data=None, always_finite=False, host=None, extra_flags=(), path=None):
        """path: a code object built beforehand from this source (`DeviceFunctionLogLike(...).code_object()` on a machine with hipcc and THIS
        version of the package: the persistent kernels' names carry the layout generation, a stale object just runs the multi-kernel path)"""
        if source is None and path is None:
            raise ValueError("give the device function's HIP source (or the path of a code object built from it)")
        self.name, self.d, self.source = name, int(ndim), source
        self.data = None if data is None else np.ascontiguousarray(data)
        self.always_finite, self.host, self.extra_flags = bool(always_finite), host, tuple(extra_flags)
        self.path = path
        self._eval_engine = None

    def code_object(self):
        if self.path is None:
            import glob
            import hashlib
            import os
            hdr = hashlib.sha256()
            for h in sorted(glob.glob(os.path.join(csrc_dir(), "*.h"))):       # (the object is only as current as the headers it was built against)
                with open(h, "rb") as fh:
                    hdr.update(fh.read())
            text = _FUNCTION_TU % dict(source=self.source, name=self.name) + "\n// headers " + hdr.hexdigest() + "\n"
            self.path = compile_device_kernel(text, extra_flags=("-I" + csrc_dir(), "-Wno-unused-value", "-Wno-unused-result") + self.extra_flags)
        return self.path

    def _dz_apply(self, engine):
        engine.set_likelihood_module(self.code_object(), "dz_user_batch", 64, self.data, self.always_finite)


class DeviceKernelLogLike(_UserKernelLogLike):
    """A user-written HIP kernel as the likelihood -- the batched device callback for ANY model (the reference accepts any callable,
    pydream/model.py:17-32; a Python callable runs through the host callback at ~40 k proposals/s, this runs where the built-in
    densities' kernels run).

        like = DeviceKernelLogLike(source=SRC, name="my_logp", ndim=d, data=np.array([...]))     # compiled with hipcc on first use
        like = DeviceKernelLogLike(path="model.hsaco", name="my_logp", ndim=d)                   # or a code object built beforehand
        sampled, log_ps = run_dream(parameters, like, nchains=4096, ...)

    The kernel's signature is KERNEL_SIGNATURE: point i is the row X + i * ld, like[i] receives its log likelihood (-inf allowed); `data`
    is the device copy of the `data` array.  lanes_per_point=1: one thread per point; 64: one wave per point (coalesced row reads, the
    kernel reduces over its lanes itself); 16 or 32: a group of that many lanes per point, point i on lanes [i * L, (i + 1) * L) of the
    grid, 256 / L points per block -- the groups of the last block whose point index is >= n run too, so the kernel predicates them
    instead of returning in front of a cross-lane operation.  always_finite=True promises the density is finite wherever the priors are (skips the
    per-generation "every try impossible?" check of Dream.py:281-289).  host: an optional Python twin f(x[d]) -> float used when the
    object is called on the host (Model.total_logp); without it a call evaluates the point on the device.

    items_per_point=C (1..64): a log-likelihood that is a sum of C independent terms (data sets, experimental conditions), one work ITEM
    per term.  The kernel is launched over n * C items: its `n` is the item count, item w is term w % C of point w // C -- the term is
    the fastest index -- so it reads the row X + (w / C) * ld and writes like[w]; lanes_per_point counts the lanes of an item.  The engine
    then adds each point's C terms in ascending order with plain additions, ((l_0 + l_1) + l_2) + ... (a -inf term: the point is -inf)."""

    items_per_point = 1     # (an object pickled before the keyword existed)

    def __init__(self, name, ndim, source=None, path=None, data=None, lanes_per_point=1, always_finite=False, host=None, extra_flags=(),
                 items_per_point=1):
        if (source is None) == (path is None):
            raise ValueError("give either the kernel's HIP source or the path of a gfx950 code object")
        self.name, self.d, self.source, self.path = name, int(ndim), source, path
        self.data = None if data is None else np.ascontiguousarray(data)
        self.lanes_per_point, self.always_finite, self.host, self.extra_flags = int(lanes_per_point), bool(always_finite), host, tuple(extra_flags)
        self.items_per_point = int(items_per_point)
        self._eval_engine = None

    def code_object(self):
        if self.path is None:
            self.path = compile_device_kernel(self.source, extra_flags=self.extra_flags)
        return self.path

    def _dz_apply(self, engine):
        engine.set_likelihood_module(self.code_object(), self.name, self.lanes_per_point, self.data, self.always_finite,
                                     items_per_point=self.items_per_point)


class MassActionODELogLike:
    """A mass-action reaction network with Gaussian data as the likelihood, integrated ON THE DEVICE by a stiff Rosenbrock solver (Rodas4,
    csrc/dz_ode.h), one lane per point -- robertson_nopysb/example_sample_robertson_nopysb_with_dream.py:43-95 written as

        like = MassActionODELogLike(
            n_species=3,
            reactions=[({0: 1}, {1: 1}, 0),               # A -> B          k = 10**theta[0]
                       ({1: 2}, {1: 1, 2: 1}, 1),         # 2B -> B + C     k = 10**theta[1]
                       ({1: 1, 2: 1}, {0: 1, 2: 1}, 2)],  # B + C -> A + C  k = 10**theta[2]
            y0=[1.0, 0.0, 0.0], t=np.linspace(0, 40),     # integration starts at t0 = 0 (an output at t0 is y0)
            observables=[[0, 0, 1]],                      # O x S linear combinations of species
            data=exp_data_ctot[None, :], sd=exp_data_sd_ctot[None, :], rate_scale="log10")

    A reaction is (reactants {species: coefficient}, products {species: coefficient}, rate), rate a parameter index (the rate constant is
    10**x[index] for rate_scale "log10", x[index] for "linear"), a float (the rate constant itself) or a Monomial (below).  Its rate is k prod y_s^nu_s (no
    combinatorial factor), dy/dt = N v with N = products - reactants.  The log-likelihood is sum norm(data, sd).logpdf(sim) over the
    finite data entries (NaN data: not observed), sim the observables at the output times t (data and sd are O x T).  rtol, atol: as
    odeint's defaults; max_steps: per output interval, as odeint's mxstep.  A failed integration (more than max_steps steps in an interval,
    a step that underflows, a state or rate that is not finite) is -inf.  Amounts are non-negative: y0 >= 0, and a step that takes a species
    below -(atol + rtol |y|) is rejected and retried smaller.

    The device build runs on the engine's multi-kernel path (dz_set_likelihood_module, one thread per point) with the redraw rounds on.
    A call on the host -- __call__, simulate, the host path of run_dream -- goes through the same generated source compiled for the host
    (ROCm's clang++, else g++), which gives the same bits.  path: a code object built beforehand (`.code_object()`).

    lanes_per_point=1 (the default) keeps a point's whole S x S iteration matrix in one lane's registers: up to 8 species, 64 reactions,
    8 observables.  Without scratch memory as measured at 8 species: up to 64 reactions over at most 32 distinct parameters, or 40
    reactions with a parameter each; more distinct parameters than that spill 90..280 bytes per lane (same values, slower; see
    DESIGN.md).  lanes_per_point=16 or 32 integrates a point with a GROUP of that many lanes, one matrix row per lane
    (csrc/dz_ode_group.h: pivoted LU, triangular solves and the error norm over the group's lanes): n_species <= lanes_per_point, up to
    128 reactions and 16 observables (ODE_GROUP_LIMITS).  The same stepping loop (dzode::integrate in csrc/dz_ode.h, on another shape of
    state), the same data block, the same host-build contract (the host twin of the group solver gives the device's bits); the two
    shapes round differently, so their values on a network both can run agree to the integration tolerance, not to the bit.

    lanes_per_point=64 gives a point a whole 64-lane WAVE, for networks of 33..64 species (a smaller network is refused: 16 or 32 lanes
    are its shape), with up to 256 reactions and 16 observables (ODE_WAVE_LIMITS).  The method, the pivot rule, the order of every sum
    and so the bits are the lane group's at L = 64 -- the host twin is the same plain loop --; what differs is where things live
    (csrc/dz_ode_group.h, "a wave per point"): a lane keeps its matrix row in registers, the state the right-hand side reads is in LDS
    (S doubles per wave), and pivot rows travel through scalar registers.  Four points to a block of 256 threads; conditions,
    Monomials and events work as below.

    conditions: the same network measured in several experiments (a dose series, knock-outs, wash-outs) -- a sequence of 1..64
    (ODE_MAX_CONDITIONS) mappings with the optional keys "y0", "data", "sd", "events", "equilibrate", "inputs", "params" (below: Condition-specific
    parameters); a missing key is the constructor's own argument,
    which (y0, data, sd) may be None when every condition gives its own.  Network, t, t0, observables, tolerances and max_steps are shared.  The log-likelihood of a
    point is ((l_0 + l_1) + l_2) + ..., l_c exactly what this class gives for condition c alone (-inf if any integration fails).  On the
    device a launch covers points x C ITEMS, item w = condition w % C of point w // C (kernel dz_ode_item_batch or
    dz_ode_group_item_batch, dz_set_likelihood_items), and the engine adds a point's items in that order; the host build loops the same
    way and gives the same bits.  simulate then returns [n, C, T, O], batch(return_steps=True) the steps of all conditions, and
    batch_conditions(X) the l_c, [n, C].

    events: interventions during an experiment -- a sequence of at most 16 (ODE_MAX_EVENTS) tuples (time, species, factor, amount): at
    `time` the amount of `species` becomes factor * y + amount (a product, then a sum: two roundings).  A bolus is (t, s, 1, dose), a
    wash-out (t, s, 0, 0), setting a value (t, s, 0, v), a dilution (t, s, 0.5, 0).  t0 <= time <= t[-1]; factor and amount are finite
    and >= 0.  Events are sorted by time (stably: events at one time apply in the order given).  A condition's "events" replaces the
    constructor's ([]: none; a missing key or None inherits them, as for y0, data and sd); the constructor's events=None and
    events=[] both mean none, and an object without any generates the source and the data
    block it always did.  Integration runs in segments between breakpoints -- t0, the event times, the output times -- and lands
    exactly on each; max_steps counts the attempted steps of a segment.  An output at an event's time is taken BEFORE the event
    (measure, then intervene), so an event at t[-1] has no effect; events at t0 are part of the start: applied to y0 before the
    start step, and seen by an output at t0.  After the events at a time the step controller restarts with the start step's formula
    from the new state (a start step that is not finite or not > 0: -inf); batch(return_steps=True) counts the accepted steps of all
    segments.  Both builds and both shapes follow this exactly (csrc/dz_ode.h) and give the same bits.  Not supported: an amount that
    is a Monomial (a sampled dose), events triggered by the state; fixed_steps ignores events.

    equilibrate: start the experiment from the RESTING STATE of the unstimulated system -- receptor turnover, basal phosphorylation,
    pre-formed complexes: a state that depends on the sampled rate constants -- instead of from amounts someone wrote down.  None or
    False: no such phase (an object without it in any experiment generates the source and the data block it always did); True: the
    defaults; or a mapping with the optional keys
      * rtol, atol: the tolerances of the steady-state test (default: the constructor's rtol and atol);
      * horizon: the length of time over which the state is to stand still (default max(t[-1] - t0, 1e-300); finite and > 0);
      * max_step: the largest step of the phase (default 1e6 * horizon; finite and > 0);
      * max_steps: the attempted steps of the phase (default 2000, ODE_EQUILIBRATE_MAX_STEPS; >= 1).
    A condition may carry its own "equilibrate": a missing key or None inherits the constructor's value, False switches the phase off
    for that condition, True and a mapping stand for themselves (defaults filled in, not the constructor's mapping).  The semantics
    (csrc/dz_ode.h's head), the same in both builds and every shape:
      * the phase starts from the experiment's y0 (Monomial entries as always).  The system is autonomous, so the phase keeps no
        clock: only the state and the step size exist;
      * the first step is start_step(y0, rtol, atol, horizon) -- not finite or not > 0: -inf --, the steps and the controller are the
        experiment's (error test, negativity rule, rejection rule, the same rtol and atol), but no step is clipped to a breakpoint, and
        after an accepted step h = min(h * factor, max_step);
      * before every attempted step, so also on y0 itself, the steady-state test: the state is steady when
        mean((f(y) / (atol_ss + rtol_ss |y|))**2) * horizon**2 <= 1 -- left alone for the length of the experiment it would move by
        less than the tolerance, in the RMS sense;
      * -inf when the state is not steady after max_steps attempted steps (a limit cycle, a mode too slow for the budget), a state is
        not finite, the iteration matrix is singular or a step is not > 0;
      * the state at which the test passed is the experiment's start; from there everything is as without the phase.  The events at t0
        are applied to it, so a condition's stimulus is a bolus (t0, s, 1, dose); the controller starts with the usual formula from
        that state; an output at t0 sees the equilibrated state after the events at t0.  batch(return_steps=True) includes the phase's
        steps.
    steady_state(X) returns the state handed to the experiment, before the events at t0 (host build).  Not supported: one
    equilibration shared between the conditions of a point -- every condition equilibrates on its own, also where two of them start
    from the same y0 --; a setting of the phase that is a Monomial; fixed_steps ignores equilibrate, as it ignores events.

    settle: a measurement AT STEADY STATE -- a dose-response point, a binding equilibrium, a blot "after the system has settled", PEtab's
    time = inf -- is an output time of +inf: t may end in exactly one np.inf (every other entry finite, sorted and >= t0; t = [inf]
    alone is a pure steady-state read-out with T = 1), and row T-1 of data and sd is that measurement (NaN: not observed, as
    everywhere).  t_last is the last finite output time, or t0 if there is none; wherever this text says t[-1] -- the events' and the
    input tables' span, equilibrate's default horizon, the start step's span -- such an object uses t_last.  The phase ahead of the
    steady row is set with settle=None | True | a mapping with equilibrate's keys, meanings and checks:
      * rtol, atol: the tolerances of the steady-state test (default: the constructor's rtol and atol);
      * horizon: the length of time over which the state is to stand still (default t_last - t0 when that is > 0; otherwise, so for
        t = [inf], the key is required: an experiment without a finite length has no honest default);
      * max_step (default 1e6 * horizon), max_steps (default 2000, ODE_SETTLE_MAX_STEPS; >= 1).
    None means True when t ends in inf.  A condition may carry its own "settle": a missing key or None inherits the constructor's, True
    and a mapping stand for themselves.  The phase cannot be switched off per condition, because t is shared: settle=False with a t
    that ends in inf is refused, and so is True or a mapping with a t that does not.  The contract (csrc/dz_ode.h's head, STEADY OUTPUT),
    the same in both builds and every shape:
      * the finite outputs run exactly as in the object without the steady row.  At t_last the order at one time holds: the output,
        then the knots that are due, then the events that are due in the order given -- an event at t_last, which has no effect in an
        object with a finite last output, is "measure, intervene, let it settle".  Inputs are then held at their value at t_last with
        every drive 0, as ahead of an equilibration;
      * the phase is equilibrate's loop from that state: start_step(y, rtol, atol, horizon) (not finite or not > 0: -inf), the
        steady-state test before every attempted step, so also on the state as it arrives, the experiment's step, error test,
        negativity and rejection rules, no step clipped, h = min(h * factor, max_step) after an accepted step; -inf when the state is
        not steady after max_steps attempts, a state is not finite, the matrix is singular or a step is not > 0.  The phase applied to a
        state y therefore gives the bits of the equilibration of a second object started from y0 = y with equilibrate set to the same
        five numbers;
      * at the state where the test passed the observables are taken and row T-1's terms added by the code of the finite rows (a
        Noise's, or the fixed-sd residual); a failure there is -inf.
    settled_state(X) returns that state, [n, S] or [n, C, S], NaN where the item failed (host build; return_attempts=True: also the
    phase's attempted steps), the twin of steady_state at the other end.  simulate, batch, batch_conditions, batch(return_steps=True) --
    which includes the phase's accepted steps --, noise_values, pickling, with_outputs (whose t may end in inf likewise; the phase's
    settings carry over; with the object's own t every row, the steady one included, has the same bits -- another grid clips other
    steps, so its rows and the state the phase starts from agree to the integration tolerance and not to the bit, as for every
    with_outputs), device(), posterior_predictive and the host path of run_dream treat row T-1 as any row.  Every experiment's
    block grows by the phase's six doubles and the generated network gains SETTLE = true; an object whose t is finite generates the
    source, the data block and the cache key it always did.  Not supported: more than one steady row per experiment; a steady state
    between two finite outputs (use two conditions); Newton polishing of the state (conservation laws make the Jacobian singular); a
    setting of the phase that is a Monomial; fixed_steps ignores the phase, as it ignores events, and gives NaN for t1 = inf.

    Products of parameters: a Monomial(exponents, log10_factor) = 10**(log10_factor + sum_i exponents[i] x[i]) may stand
      * as a reaction's rate (kr = KD kf with a fixed kf: Monomial({i: 1}, log10(kf)); a closed cycle: Monomial({0: 1, 1: 1, 2: -1}));
      * as an entry of y0, the constructor's or a condition's: a sampled total amount.  A species has the same Monomial wherever a y0
        gives it one; a condition may still give it a plain number (a knock-out at 0.0);
      * in scale=[...], O numbers or Monomials shared by all conditions: the residual is (scale_q o[q] - data) / sd, and simulate returns
        the scaled observables, what is compared with the data;
      * in constraints=[(Monomial, loc, sd), ...] (at most 16, ODE_MAX_CONSTRAINTS): g(x) = sum norm(loc, sd).logpdf(monomial) is added
        to the single experiment's value, l + g, and with conditions to the term of condition 0 (l_0 + g, what an object of condition 0
        alone with the same constraints returns; the other conditions' terms are those of objects without constraints).
        constraint_terms(X) returns g.
    Its value is computed the same way on the device and the host (csrc/dz_ode.h: the sum in ascending index, then dzode::dexp) and
    does not depend on rate_scale; Monomial({i: 1}) as a rate gives the bits of the bare index i under "log10".  A point at which a
    coordinate read by a monomial, or a monomial's value, is not finite is -inf.  ndim is inferred over every index read, bare or
    inside a monomial.  A model that uses none of this generates the source, and runs the kernels, it always did.

    Saturating rate laws: a RateLaw(rate, factors=(), order=None) may stand where a reaction's third element stands, for a rate that is
    not mass action: v = k * prod_s y_s^order_s * prod_m h_m(y), dy/dt = N v as before.  `rate` is what the third element may be
    without it; `order` None keeps the reactants' coefficients as kinetic orders, a mapping {species: non-negative integer} replaces
    them ({}: no mass-action factor); `factors` are up to 4 (ODE_MAX_RATE_FACTORS) Hill(species, K, n=1, kind="activation"):
    y^n / (K^n + y^n), or K^n / (K^n + y^n) for kind "repression", with K a parameter index (10**x[i] or x[i], by rate_scale), a
    finite float > 0 or a Monomial and n an integer 1..8 (ODE_MAX_HILL_EXPONENT; powers are repeated products):
        ({S: 1}, {P: 1}, RateLaw(iV, [Hill(S, iKm)], order={}))             # Michaelis-Menten: Vmax S / (Km + S)
        ({S: 1}, {P: 1}, RateLaw(ikcat, [Hill(S, iKm)], order={E: 1}))      # kcat E S / (Km + S)
        ({}, {M: 1}, RateLaw(ialpha, [Hill(Prot, iK, 2, "repression")]))    # repressed synthesis
    The contract (csrc/dz_ode.h's head, RATE LAWS), the same in both builds and every shape: each distinct (K, n) pair is evaluated
    once per point into a SLOT beside the rate constants, Kn = K * K * ... (n factors, left to right), and reactions plus slots stay
    within the shape's reaction limit (64 / 128 / 256); a point is -inf if a coordinate that a K reads or a K is not finite, or a Kn is
    not finite or not > 0 (under "linear" a sampled K <= 0 rejects the point); a factor is yn / (Kn + yn) or Kn / (Kn + yn) with yn the
    repeated product of y, its derivative +-(n Kn y^(n-1)) / ((Kn + yn) (Kn + yn)); v is the product of k, the mass-action factors in
    ascending species and the Hill factors in the order given, and a Jacobian column is the product rule's sum in that order (a
    species may be in `order` and in a factor, or in two factors).  Nothing is clamped; the Jacobian stays analytic.  ndim covers
    the indices every K reads.  A RateLaw with no factors and order=None is the plain reaction, source and bits; a model without a
    RateLaw generates the source and the data block it always did.  Conditions, Monomials, events, equilibration, fixed_steps,
    simulate and steady_state work with it unchanged.  Not supported: a non-integer or sampled Hill exponent, arbitrary rate
    expressions, rate laws in event amounts.

    Inputs: inputs=[Input(species, times, values, gain=None), ...], at most 4 (ODE_MAX_INPUTS), each on a species of its own: a
    measured or prescribed TIME COURSE that drives the network -- an upstream activity read off a blot, a perfusion protocol, a PK
    curve, a light schedule.  The amount of `species` is gain * u(t), u the piecewise-linear curve through (times[k], values[k])
    (times strictly increasing, at least 2; values finite and >= 0); gain is None, a finite float > 0, a parameter index (10**x[i]
    or x[i], by rate_scale) or a Monomial: a sampled amplitude.  Nothing produces or consumes an input species -- every reaction has
    net stoichiometry 0 on it; it may be a catalyst, a kinetic order or the species of a Hill factor --, no event targets it, its y0
    entry is 0 and not a Monomial (the value comes from the table), it counts towards the shape's species limit, and each table
    covers [t0, t[-1]].  A condition may carry its own "inputs": a missing key or None inherits the constructor's; its list names the
    same species in the same order with the same gains, only the tables differ.  The contract (csrc/dz_ode.h's head, INPUTS), the
    same in both builds and every shape:
      * the input is carried as one more species: its right-hand side is the current segment's slope, its Jacobian row is zero, its
        value is set exactly at every knot.  The system stays autonomous, and a Rosenbrock method integrates u' = const exactly up
        to rounding;
      * the WORKING KNOTS are made here, once (Input.working_knots): one at t0 -- the table's value there and the slope of the
        segment that holds t0 --, then the table's knots strictly inside (t0, t[-1]), each with its value and the slope that follows;
        at most 128 per experiment over all its inputs together (ODE_MAX_INPUT_KNOTS).  Each experiment's block grows at its end by
        their count and Kmax records (time, input, value, slope);
      * the gain g_i is evaluated once per point, when the rate constants are and with their arithmetic; a point is -inf if a
        coordinate that a gain reads is not finite or g_i is not finite or not > 0;
      * a due knot sets y[species] = g_i * v (one product; without a gain v itself, so Monomial({i: 1}) at x[i] = 0 gives the bits
        of no gain) and the drive to g_i * s; inputs at one time apply in ascending index;
      * knots are breakpoints beside t0, the event times and the output times: a step is clipped to land exactly on a knot, and the
        controller is NOT restarted there -- a clipped step leaves its size alone, as at an output time; max_steps counts per
        segment;
      * at one time: an output first (measure, then intervene), then the knots, then the events in the order given;
      * equilibrate runs with the input held at g_i * u(t0) and every drive 0, the resting state under the basal input; the knot at
        t0 then installs the first slope before the start step.
    ndim covers the indices a gain reads.  with_outputs(t, t0) carries the inputs over, recomputes the working knots and refuses a
    span the tables do not cover; simulate, batch, batch_conditions, steady_state, device(), posterior_predictive and the host path of
    run_dream work with inputs; fixed_steps ignores them, as it ignores events (every drive 0, the input species at 0).  inputs=None
    and inputs=[] are the object it always was: the same source, data block and cache key.  To see an input's own trajectory declare
    it as an observable with NaN data.  Not supported: inputs that are not piecewise linear, an input that reactions also consume,
    sampled knot times.

    Sampled noise: noise=[...], None or O entries, each None or a Noise(sigma, rel=None, dist="normal", scale="lin"), shared by all
    conditions like `scale`.  An observable whose entry is None keeps the fixed-sd term above exactly; for one with a Noise the spread
    of the readout is part of the point, and its sd (still O x T, the constructor's or a condition's; sd=None means 1 when every
    observable has a Noise) is a fixed WEIGHT w, the replicate's relative precision.  sigma and rel are a parameter index (10**x[i]
    under "log10", x[i] under "linear"), a finite float (sigma > 0, rel >= 0) or a Monomial; dist is "normal" or "laplace"; scale is
    "lin" or "log" (rel with "log" is refused: a proportional part on the log scale is the log scale itself; data of a "log" observable
    must be > 0 where observed).  The contract (csrc/dz_ode.h's head, NOISE), the same in both builds and every shape:
      * a_q = sigma_q and b_q = rel_q are evaluated once per point, when the rate constants are and with their arithmetic (one dexp,
        or the Monomial's sum), never per output time; noise_values(X) returns them, [n, O, 2] (NaN for an observable without a Noise,
        b = 0 without rel);
      * a point is -inf if a coordinate that a Noise reads is not finite, a_q is not finite or not > 0, or b_q is not finite or < 0:
        under "linear" a sampled sigma <= 0 rejects the point;
      * at an output time, with m the observable after `scale`, d the data and w the weight: "lin": s = a_q (with rel: a_q + b_q |m|),
        s = s * w, r = (m - d) / s; "log": s = a_q * w, r = (dlog(m) - ln d) / s with ln d computed on the host; "normal" adds
        -r r / 2 - dlog(s), "laplace" -|r| - dlog(s): the log-likelihood is sum norm(m, s).logpdf(d), or laplace(m, s), and on the log
        scale the same density at ln d around ln m, minus ln d;
      * an entry that is not observed (NaN data) adds exactly 0 whatever m is, also m <= 0 on the log scale; an observed entry at
        which m is not finite, m is not > 0 on the log scale, or s is not finite or not > 0 is a failed integration (-inf);
      * the block's constant holds, per observed entry, -log sd - log(2 pi) / 2 (no Noise), -log(2 pi) / 2 ("normal"), -log 2
        ("laplace") and on the log scale additionally -ln d; w is inside s.
    simulate still returns the scaled observables on the natural scale; ndim covers every index a Noise reads; noise=None and a list
    of Nones generate the source and the data block the object always had.  Not supported: Student-t residuals, a per-condition
    noise, a sampled offset on the log scale; fixed_steps has no likelihood and ignores noise.

    Normalised readouts: normalize=[...], None or O entries, each None or a Normalize(kind, t=None), shared by all conditions like
    `scale` and `noise` -- a western blot, a reporter trace or a FACS time course reported as a fraction of its own maximum, as fold
    change over a chosen point, or rescaled to [0, 1].  With m_j the observable after `scale` at output row j of one experiment (the
    single experiment, or one condition on its own): "max": m'_j = m_j / max_j m_j, the maximum over EVERY output row, observed or
    not (rows with NaN data sample the peak more densely); "ref" with t= one of the object's output times (np.inf: the steady row):
    m'_j = m_j / m(t); "minmax": m'_j = (m_j - lo) / (hi - lo) over every row.  The residual is (m' - d) / sd with `data` on the
    normalised scale; simulate, device().simulate and posterior_predictive return m'.  An observable without a Noise keeps its fixed
    sd; with Noise(sigma) the spread is sigma times the weight, as always.  The contract (csrc/dz_ode.h's head, NORMALISED READOUTS):
    the integration and the un-normalised m have the bits of the object without `normalize`; the rows feed running sums
    (A = sum p p, B = sum p e, p = m / sd, e = d / sd) and the term is formed once behind the last row as a quadratic form in 1 / g;
    a g that is not finite or not > 0 -- a trajectory that is identically zero -- is a failed integration (-inf, NaN in simulate);
    every experiment's block grows by seven doubles per normalised observable, behind the input knots and in front of a view's pairs.
    with_outputs(t) carries the setting over and normalises over the NEW grid: the maximum over a denser grid is a different (larger
    or equal) number, so dense curves of a "max" or "minmax" readout do not pass exactly through simulate's values; a "ref" whose
    time is not in the new t is refused.  normalize=None and a list of Nones are the object it always was: source, data block and
    cache key.  Not supported: Noise with rel, dist="laplace" or scale="log" on a normalised observable (refused: their residuals are
    no quadratic form, and the likelihood kernel stores no trajectory); a normaliser shared between conditions (the lanes of one gel
    across doses); a scale fitted to the data.

    Condition-specific parameters: a condition's "params" = {i: target} makes the experiments differ in the SYSTEM and not only in what
    is done to it -- a knock-down or a mutant that changes a rate constant, an inhibitor in the treated arms only, a sampled readout
    scale per gel, a noise level per assay, a cell line's own expression level (PEtab's condition table).  i is a parameter index the
    network reads -- bare as a rate or a Hill K, inside a Monomial, in scale, noise, a gain or a y0 Monomial --; an int target j (numpy
    ints count, a bool is refused) means: this condition reads x[j] wherever the network says x[i]; a finite float target v means: it
    reads the number v there -- the coordinate's value, not the constant: under "log10" a bare rate index then gives 10**v.  A missing
    key, None or {} is the identity, and an object in which no condition has a mapping is the object it always was: source, data
    block and code object.  Example: conds = [dict(y0=..., data=..., sd=..., params={5: 7, 9: 0.0}), ...].  The contract
    (csrc/dz_ode.h's head, VIEWS), the same in both builds and every shape, with x'_c = V_c(x) the row of P = 1 + the largest index
    the network reads entries that condition c sees (viewed(X, c) restates it in numpy):
      * x'[i] is a SELECT between x[j] and v, no arithmetic: the bits are one or the other, and a coordinate of the point that a
        condition does not read has no effect on its term, whatever it holds, NaN included;
      * item c's term l_c(x) has the bits of the object of condition c alone, made without "params", at the row x'_c; its simulate
        slice, steps, resting state and noise values likewise.  The sum stays ((l_0 + l_1) + l_2) + ...;
      * liveness is per item: a non-finite coordinate that condition 1 replaces and condition 0 reads makes l_0 = -inf and leaves l_1
        finite;
      * an index mapped away in EVERY condition is formal: it is never read from the point and may lie at or beyond ndim -- a factor
        that is 0.0 in control arms and -1.0 in inhibitor arms needs no sampled coordinate.  ndim is inferred as one more than the
        largest coordinate some condition actually reads, an unmapped index or a target; an explicit ndim must be at least that;
        P <= 128 (ODE_MAX_VIEW_COORDINATES);
      * constraints are statements about the point: one whose Monomial reads a coordinate that some condition replaces is refused,
        so they give the same value under every view; they stay on condition 0's term, and constraint_terms(X) evaluates them
        through condition 0's view;
      * with a view every experiment's block grows at its very end by 2 P doubles, the pairs (j_i, v_i), and the generated network
        gains VIEW = P; the host build then evaluates rate constants, slots, gains and noise values per condition.
    batch, batch_conditions, simulate, steady_state, fixed_steps(condition=c), with_outputs, pickling, device() and
    posterior_predictive follow the view per condition; noise_values(X) returns [n, C, O, 2] for an object with a view (each
    condition's own values, what a replicate of that condition is drawn with) and [n, O, 2] otherwise.  Not supported: targets that
    are Monomials or expressions (x[j] + c and sums are reached through a Monomial plus a fixed formal coordinate:
    pydream_amd/examples/knockdown), a constraint on a replaced coordinate, a view without conditions.

    Prediction: what follows a fit -- the trajectories of the posterior's rows against the data -- runs on the device too.
    device(device=0, max_bytes=256 << 20, chunk_items=None) returns an ODEDeviceEvaluator (a context manager; close() frees its small
    engine) with batch(X), batch_conditions(X) and simulate(X, return_terms=False): the host methods of the same names evaluated by the
    kernels, no prior added.  batch goes through the likelihood kernel the sampler runs (dz_eval_logp); simulate and batch_conditions
    through the PREDICTION kernels (csrc/dz_ode.h, PREDICTION: dz_ode_predict, dz_ode_item_predict, dz_ode_group_predict,
    dz_ode_group_item_predict), the same integration with the observables kept: predict_source() is source() behind the line
    "#define DZODE_PREDICT 1", a translation unit of its own that is compiled on first use and cached under its own key -- a model that
    never predicts never compiles it, and the likelihood's code object is what it was.  Results are the bits of the host methods in
    every shape and with every feature above: simulate gives the scaled observables on the natural scale, [n, T, O] or
    [n, C, T, O], and NaN throughout the slice of an item whose term is -inf; the terms are those of batch_conditions.  Rows are
    processed in chunks of whole points (at least one) so that the device's output buffer stays within max_bytes, or within
    chunk_items items.  Without a GPU device() raises DreamZSError: there is no fallback to the host build.
    with_outputs(t, t0=None) returns a sibling object for smooth curves between the measurement times: the same network, conditions,
    y0, events, equilibration, scale and noise, new output times, and every data entry NaN (not observed), so its batch is the
    block's constant (0, plus the constraints' term) wherever the integration succeeds; events must lie within the new [t0, t[-1]];
    with the object's own t it simulates to the same bits.  posterior_predictive(sampled_params, like, burnin, thin, device, t) in this
    module selects the rows of run_dream's chains and simulates them.  Noise replicates are drawn on the host from simulate's result
    and noise_values(rows).  Not supported on the device: trajectories of species that are not observables (declare an observable
    with NaN data), steady_state and fixed_steps; these remain host-only."""

    conditions = None       # (an object pickled before the keyword existed)
    events = None           # (likewise)
    equilibrate = None      # (likewise)
    settle = None           # (likewise: before the steady output existed)
    scale, constraints, y0_monomials = None, (), {}     # (likewise: before Monomial existed)
    noise = None            # (likewise: before Noise existed)
    inputs = None           # (likewise: before Input existed)
    normalize = None        # (likewise: before Normalize existed)

    def __init__(self, n_species, reactions, y0, t, observables, data, sd, rate_scale="log10", t0=0.0, rtol=1.49012e-8, atol=1.49012e-8,
                 max_steps=500, ndim=None, path=None, lanes_per_point=1, conditions=None, scale=None, constraints=None, events=None,
                 equilibrate=None, noise=None, inputs=None, settle=None, normalize=None):
        self.n_species, self.lanes_per_point, lim = self._checked_shape(n_species, lanes_per_point, len(reactions))
        noise = self._checked_noise(noise)      # None, or the entries (None | Noise); their number is tested below, once O is known
        if sd is None and noise is not None and all(z is not None for z in noise):
            sd = 1.0                            # (every observable has a Noise: sd is a weight, 1 unless the user says otherwise)
        if rate_scale not in ("log10", "linear"):
            raise ValueError('MassActionODELogLike: rate_scale must be "log10" or "linear"')
        self.rate_scale, self.log10 = rate_scale, rate_scale == "log10"
        self.reactions = self._checked_reactions(reactions, self.n_species, lim["reactions"])
        conditions = self._checked_condition_keys(conditions, dict(y0=y0, data=data, sd=sd))
        self.y0_monomials = {}                  # species -> the Monomial its start amount is, wherever a y0 says so (the same in all)
        self.y0 = y0 if y0 is None else self._checked_y0(y0, "")
        self.t, self.t0, self.observables = self._checked_times(t, t0, observables, self.n_species, lim)
        if noise is not None and len(noise) != len(self.observables):
            raise ValueError("MassActionODELogLike: noise must be None or hold O = %d entries, each None or a Noise (got %d)" % (len(self.observables), len(noise)))
        self.noise = noise if noise is not None and any(z is not None for z in noise) else None
        self.normalize = self._checked_normalize(normalize)     # None, or O entries None | Normalize with at least one Normalize
        self.data, self.sd = self._checked_data(data, sd, "") if data is not None and sd is not None else (data, sd)
        events = self._checked_events(events, "")
        if not (rtol > 0 and atol > 0 and np.isfinite(rtol) and np.isfinite(atol)) or int(max_steps) < 1:
            raise ValueError("MassActionODELogLike: rtol and atol must be > 0, max_steps >= 1")
        self.rtol, self.atol, self.max_steps = float(rtol), float(atol), int(max_steps)
        self.events = events or None            # None, or the checked (time, species, factor, amount) tuples sorted by time
        self.equilibrate = self._checked_equilibrate(equilibrate, "")       # None, or dict(rtol, atol, horizon, max_step, max_steps), every default filled in
        self.settle = self._checked_settle(settle, "")                      # likewise: None exactly when t is finite throughout
        # None, or a list of dict(y0, data, sd, events[, equilibrate]): checked, the fallbacks filled in -- every condition as the single
        # experiment: its own values, else the constructor's (checked above)
        self.conditions = conditions and [self._checked_condition(cond, "condition %d: " % c, events) for c, cond in enumerate(conditions)]
        self.scale, self.constraints = self._checked_scale(scale, len(self.observables)), self._checked_constraints(constraints)
        self.inputs = self._checked_inputs(inputs, "") or None      # None, or the checked Input objects
        self._check_input_species()
        if self.conditions is not None:         # (a condition's own tables: the same species, order and gains as the constructor's)
            for c, cond in enumerate(self.conditions):
                own = conditions[c].get("inputs")
                if own is not None:
                    cond["inputs"] = self._checked_inputs(own, "condition %d: " % c, like=self.inputs or ())
        if self.conditions is not None:         # (a condition's view of the point: csrc/dz_ode.h, VIEWS)
            for c, cond in enumerate(self.conditions):
                view = self._checked_params(conditions[c].get("params"), c)
                if view:
                    cond["params"] = view
        self.d = self._checked_ndim(ndim)
        self.path, self._host = path, None

    @staticmethod
    def _checked_shape(n_species, lanes_per_point, R):
        """(S, lanes, the limits of that shape) of a network of R reactions"""
        S = int(n_species)
        lanes = int(lanes_per_point)
        if lanes != 1 and lanes not in ODE_GROUP_LIMITS["lanes"] + ODE_WAVE_LIMITS["lanes"]:
            raise ValueError("MassActionODELogLike: lanes_per_point must be 1, 16, 32 or 64 (got %r)" % (lanes_per_point,))
        lim = ODE_LIMITS if lanes == 1 else ODE_WAVE_LIMITS if lanes in ODE_WAVE_LIMITS["lanes"] else dict(ODE_GROUP_LIMITS, species=lanes)
        if not 1 <= S <= lim["species"]:
            raise ValueError("MassActionODELogLike: n_species must be 1..%d (got %d)" % (lim["species"], S))
        if lim is ODE_WAVE_LIMITS and S <= ODE_GROUP_LIMITS["species"]:          # (half the wave would idle)
            raise ValueError("MassActionODELogLike: lanes_per_point=%d is for networks of %d..%d species; use 16 or 32 (got %d species)"
                             % (lanes, ODE_GROUP_LIMITS["species"] + 1, lim["species"], S))
        if not 1 <= R <= lim["reactions"]:
            raise ValueError("MassActionODELogLike: 1..%d reactions are supported (got %d)" % (lim["reactions"], R))
        return S, lanes, lim

    @staticmethod
    def _checked_reactions(reactions, S, limit):
        """The reactions as (reactants, products, rate): {species: coefficient > 0} with plain ints, the rate an int, a float, a Monomial
        or a RateLaw that says more than its rate."""
        rx = []
        for r, reaction in enumerate(reactions):
            if len(reaction) != 3:
                raise ValueError("MassActionODELogLike: reaction %d must be (reactants, products, rate)" % r)
            reac, prod, rate = reaction
            for side in (reac, prod):
                for s, c in dict(side).items():
                    if not _is_int(s, 0, S - 1):
                        raise ValueError("MassActionODELogLike: reaction %d names species %r (0..%d)" % (r, s, S - 1))
                    if not _is_int(c, 0):
                        raise ValueError("MassActionODELogLike: reaction %d: stoichiometric coefficients must be non-negative integers (got %r)" % (r, c))
            if isinstance(rate, RateLaw):
                for s in [s for s, _ in rate.order or ()] + [f.species for f in rate.factors]:
                    if not 0 <= s < S:
                        raise ValueError("MassActionODELogLike: reaction %d: its RateLaw names species %r (0..%d)" % (r, s, S - 1))
                if not rate.factors and rate.order is None:          # (nothing beyond its rate: the plain reaction, source and bits)
                    rate = rate.rate
            else:
                rate = _checked_constant(rate, "reaction %d" % r, "reaction %d: the rate is a parameter index (int), a fixed rate constant (float), "
                                                                    "a Monomial or a RateLaw" % r)
                if isinstance(rate, float) and not np.isfinite(rate):
                    raise ValueError("MassActionODELogLike: reaction %d: the fixed rate constant must be finite" % r)
            rx.append(({int(s): int(c) for s, c in dict(reac).items() if c}, {int(s): int(c) for s, c in dict(prod).items() if c}, rate))
        slots = _hill_slots(rx)
        if len(rx) + len(slots) > limit:
            raise ValueError("MassActionODELogLike: reactions plus distinct Hill (K, n) pairs must stay within %d (got %d + %d)" % (limit, len(rx), len(slots)))
        return rx

    @staticmethod
    def _checked_condition_keys(conditions, own):
        """None, or the conditions as a list of mappings with known keys -- every one of y0, data and sd given by the condition or by the
        constructor (own)."""
        if conditions is None:
            if any(v is None for v in own.values()):
                raise ValueError("MassActionODELogLike: y0, data and sd may be None only when every one of the conditions gives its own")
            return None
        conditions = list(conditions)
        if not 1 <= len(conditions) <= ODE_MAX_CONDITIONS:
            raise ValueError("MassActionODELogLike: 1..%d conditions are supported (got %d)" % (ODE_MAX_CONDITIONS, len(conditions)))
        for c, cond in enumerate(conditions):
            if not hasattr(cond, "keys") or set(cond.keys()) - {"y0", "data", "sd", "events", "equilibrate", "inputs", "params", "settle"}:
                raise ValueError('MassActionODELogLike: condition %d must be a mapping with the keys "y0", "data", "sd", "events", "equilibrate", "inputs", '
                                 '"params", "settle" (each optional)' % c)
            for key, top in own.items():
                if cond.get(key) is None and top is None:
                    raise ValueError("MassActionODELogLike: condition %d has no %s, and the constructor's %s is None" % (c, key, key))
        return conditions

    @staticmethod
    def _checked_times(t, t0, observables, S, lim):
        """(the output times, t0, the O x S observables)"""
        t = np.asarray(t, dtype=float).reshape(-1)
        if not 1 <= len(t) <= lim["times"]:
            raise ValueError("MassActionODELogLike: 1..%d output times are supported (got %d)" % (lim["times"], len(t)))
        fin = t[:-1] if t[-1] == np.inf else t      # (the last may be +inf: a steady output, csrc/dz_ode.h's STEADY OUTPUT)
        if not np.isfinite(t0) or not np.all(np.isfinite(fin)) or np.any(np.diff(fin) < 0) or t[0] < t0:
            raise ValueError("MassActionODELogLike: output times must be finite, sorted and >= t0 = %r; only the last may be inf, a steady "
                             "output (got %r)" % (t0, t.tolist()))
        obs = np.atleast_2d(np.asarray(observables, dtype=float))
        if obs.ndim != 2 or obs.shape[1] != S or not 1 <= len(obs) <= lim["observables"] or not np.all(np.isfinite(obs)):
            raise ValueError("MassActionODELogLike: observables must be an O x %d finite matrix with O = 1..%d" % (S, lim["observables"]))
        return t, float(t0), obs

    def _checked_condition(self, cond, who, events):
        """A condition as the single experiment: dict(y0, data, sd, events[, equilibrate]); events: the constructor's, checked."""
        y0 = self.y0 if cond.get("y0") is None else self._checked_y0(cond["y0"], who)
        data, sd = (self.data if cond.get("data") is None else cond["data"]), (self.sd if cond.get("sd") is None else cond["sd"])
        if cond.get("data") is not None or cond.get("sd") is not None or self.data is None or self.sd is None:
            data, sd = self._checked_data(data, sd, who)
        if cond.get("events") is not None:
            events = self._checked_events(cond["events"], who)
        eq = self.equilibrate if cond.get("equilibrate") is None else self._checked_equilibrate(cond["equilibrate"], who)
        st = self.settle if cond.get("settle") is None else self._checked_settle(cond["settle"], who)
        return dict(y0=y0, data=data, sd=sd, events=events, **({"equilibrate": eq} if eq else {}), **({"settle": st} if st else {}))

    @staticmethod
    def _checked_scale(scale, O):
        """None, or the O scale factors: floats and Monomials"""
        if scale is None:
            return None
        scale = list(scale) if hasattr(scale, "__len__") or hasattr(scale, "__iter__") else [scale]
        if len(scale) != O or not all(isinstance(f, Monomial) or _is_real(f) for f in scale):
            raise ValueError("MassActionODELogLike: scale must hold O = %d finite numbers or Monomials" % O)
        return [f if isinstance(f, Monomial) else float(f) for f in scale]

    @staticmethod
    def _checked_constraints(constraints):
        """The constraints as a tuple of (Monomial, loc, sd)"""
        cons = []
        for m, entry in enumerate(() if constraints is None else constraints):
            if not isinstance(entry, (tuple, list)) or len(entry) != 3 or not isinstance(entry[0], Monomial):
                raise ValueError("MassActionODELogLike: constraint %d must be (Monomial, loc, sd)" % m)
            try:
                loc, csd = float(entry[1]), float(entry[2])
            except (TypeError, ValueError):
                loc = csd = np.nan
            if not (_is_real(loc) and _is_real(csd) and csd > 0):
                raise ValueError("MassActionODELogLike: constraint %d: loc must be finite and sd finite and > 0" % m)
            cons.append((entry[0], loc, csd))
        if len(cons) > ODE_MAX_CONSTRAINTS:
            raise ValueError("MassActionODELogLike: at most %d constraints are supported (got %d)" % (ODE_MAX_CONSTRAINTS, len(cons)))
        return tuple(cons)

    @staticmethod
    def _checked_noise(noise):
        """None, or the noise models as a list of None | Noise"""
        if noise is None:
            return None
        try:
            entries = list(noise)
        except TypeError:
            entries = [noise]
        if isinstance(noise, Noise) or not all(z is None or isinstance(z, Noise) for z in entries):
            raise ValueError("MassActionODELogLike: noise must be None or a sequence of O entries, each None or a Noise (got %r)" % (noise,))
        return entries

    def _checked_normalize(self, normalize, t=None):
        """None, or the normalisations as a list of None | Normalize, at least one of them a Normalize (csrc/dz_ode.h, NORMALISED
        READOUTS); t: the output times a "ref" must name (default: the object's)."""
        if normalize is None:
            return None
        try:
            entries = list(normalize)
        except TypeError:
            entries = [normalize]
        O, t = len(self.observables), self.t if t is None else t
        if isinstance(normalize, Normalize) or len(entries) != O or not all(z is None or isinstance(z, Normalize) for z in entries):
            raise ValueError("MassActionODELogLike: normalize must be None or hold O = %d entries, each None or a Normalize (got %r)" % (O, normalize))
        for q, z in enumerate(entries):
            if z is None:
                continue
            if z.kind == "ref" and not np.any(t == z.t):
                raise ValueError('MassActionODELogLike: normalize[%d]: the reference time %r is not one of the output times %r' % (q, z.t, t.tolist()))
            nz = self.noise[q] if self.noise is not None else None
            if nz is not None and (nz.rel is not None or nz.dist != "normal" or nz.scale != "lin"):
                raise ValueError('MassActionODELogLike: observable %d is normalised, so its Noise must be Noise(sigma): normal residuals on the "lin" '
                                 'scale without rel (got %r).  Other residuals are no quadratic form in 1 / g, and the likelihood kernel stores '
                                 'no trajectory' % (q, nz))
        return entries if any(z is not None for z in entries) else None

    def _norm_records(self, data, sd):
        """One experiment's records of its normalised observables (csrc/dz_ode.h, NORMALISED READOUTS), seven doubles each in ascending
        q: kind (1 "max", 2 "ref", 3 "minmax"), the reference row (0 unless "ref"), D = sum e e, E = sum e iw, W = sum iw iw with
        iw = 1 / sd and e = d iw over the rows from left to right (an unobserved entry: d = 0, sd = inf, so exactly 0), the observed
        count n_q and L_q = sum ln sd over the observed entries.  data, sd: O x T."""
        seen = np.isfinite(data)
        rec = []
        for q, z in enumerate(self.normalize):
            if z is None:
                continue
            D = E = W = L = 0.0
            for j in range(data.shape[1]):
                iw = 1.0 / float(sd[q, j]) if seen[q, j] else 0.0
                e = (float(data[q, j]) if seen[q, j] else 0.0) * iw
                D, E, W = D + e * e, E + e * iw, W + iw * iw
                if seen[q, j]:
                    L = L + float(np.log(sd[q, j]))
            row = float(np.flatnonzero(self.t == z.t)[0]) if z.kind == "ref" else 0.0
            rec += [float(_ode_source._NORM_KINDS[z.kind]), row, D, E, W, float(np.sum(seen[q])), L]
        return rec

    def _indices(self):
        """The parameter indices the network reads -- a rate, a Hill K, a Monomial, a Noise or a gain --, ascending."""
        outside = list(self.y0_monomials.values()) + [f for f in self.scale or [] if isinstance(f, Monomial)] + [c[0] for c in self.constraints]
        outside += [c for z in self.noise or [] if z is not None for c in (z.sigma, z.rel) if c is not None and not isinstance(c, float)]
        outside += [u.gain for u in self.inputs or () if u.gain is not None and not isinstance(u.gain, float)]
        return sorted(set(_rate_indices(self.reactions) + _slot_indices(_hill_slots(self.reactions)) + _indices_read(outside)))

    def _checked_params(self, params, c):
        """Condition c's view as {index the network reads: int j (read x[j]) | float v (read the number v)}; {}: the identity."""
        if params is None:
            return {}
        if not hasattr(params, "items"):
            raise ValueError('MassActionODELogLike: condition %d: "params" must be a mapping {parameter index: parameter index (int) or value (float)} '
                             '(got %r)' % (c, params))
        read, view = self._indices(), {}
        for i, target in params.items():
            if not _is_int(i) or int(i) not in read:
                raise ValueError('MassActionODELogLike: condition %d: "params" names %r, which is not a parameter index the network reads (%s)'
                                 % (c, i, ", ".join(str(k) for k in read)))
            if _is_int(target, 0):
                view[int(i)] = int(target)
            elif isinstance(target, (float, np.floating)) and np.isfinite(target):
                view[int(i)] = float(target)
            else:
                raise ValueError('MassActionODELogLike: condition %d: "params"[%d] must be a parameter index (an int >= 0; a bool is refused) or a '
                                 'finite value (float) (got %r)' % (c, i, target))
        if view and read[-1] + 1 > ODE_MAX_VIEW_COORDINATES:
            raise ValueError('MassActionODELogLike: condition %d: "params" views at most %d coordinates (ODE_MAX_VIEW_COORDINATES); the largest '
                             'parameter index the network reads is %d' % (c, ODE_MAX_VIEW_COORDINATES, read[-1]))
        for m, (mono, _, _) in enumerate(self.constraints):        # (constraints are statements about the point: the same under every view)
            for i in mono.indices:
                if i in view and (isinstance(view[i], float) or view[i] != i):
                    raise ValueError('MassActionODELogLike: constraint %d reads parameter %d, which condition %d replaces through "params"; '
                                     'a constraint is a statement about the point, the same under every view' % (m, i, c))
        return view

    def _has_view(self):
        """Some condition carries a non-empty "params": the generated network's VIEW and the 2 P doubles at each block's end."""
        return self.conditions is not None and any(cond.get("params") for cond in self.conditions)

    def _view_size(self):
        """P: one more than the largest index the network reads."""
        read = self._indices()
        return read[-1] + 1 if read else 0

    def _view_table(self, params):
        """A condition's view as the block holds it (csrc/dz_ode.h, VIEWS): P pairs (j_i, v_i) -- j_i >= 0 selects x[j_i], j_i = -1 the number
        v_i; an index without an entry in `params` is itself, an index nothing reads (-1, 0)."""
        read = set(self._indices())
        tab = np.zeros((self._view_size(), 2))
        for i in range(len(tab)):
            target = params.get(i, i) if i in read else 0.0
            tab[i] = (-1.0, target) if isinstance(target, float) else (float(target), 0.0)
        return tab.reshape(-1)

    def viewed(self, X, c=None):
        """The rows of X as condition c reads them, x'_c = V_c(x): [n, P], or for c None [n, C, P] -- P one more than the largest index
        the network reads; an index nothing reads holds 0.  Plain numpy, a restatement of what the kernels gather."""
        if self.conditions is None:
            raise ValueError("MassActionODELogLike: viewed needs an object made with conditions=[...]")
        X = self._rows(X)
        if c is None:
            return np.stack([self.viewed(X, k) for k in range(len(self.conditions))], axis=1)
        tab = self._view_table(self.conditions[c].get("params") or {}).reshape(-1, 2)
        j = tab[:, 0].astype(int)
        return np.where(j >= 0, X[:, np.maximum(j, 0)], tab[:, 1])

    def _checked_ndim(self, ndim):
        """The number of coordinates of a point: ndim, or one more than the largest index that a rate, a Hill K, a Monomial or a Noise
        reads -- with views: that some condition reads from the point, an unmapped index or a target."""
        idx = self._indices()
        if self._has_view():
            idx = sorted({t for cond in self.conditions for t in (cond.get("params", {}).get(i, i) for i in idx) if not isinstance(t, float)})
        d = (max(idx) + 1 if idx else 0) if ndim is None else int(ndim)
        if idx and max(idx) >= d:
            raise ValueError("MassActionODELogLike: parameter index %d is not < ndim = %d" % (max(idx), d))
        return d

    def _checked_y0(self, y0, who):
        """The start amounts as S doubles, NaN where the entry is a Monomial (csrc/dz_ode.h: "take the network's monomial");
        self.y0_monomials: species -> Monomial, filled in here -- a species has the same one wherever a y0 gives it one."""
        S, monomials = self.n_species, self.y0_monomials
        entries = list(y0) if isinstance(y0, (list, tuple)) or (isinstance(y0, np.ndarray) and y0.dtype == object) else None
        given = {s: m for s, m in enumerate(entries or ()) if isinstance(m, Monomial)}
        if given:
            y0 = [0.0 if s in given else v for s, v in enumerate(entries)]
        try:
            y0 = np.array(y0, dtype=float).reshape(-1)
        except (TypeError, ValueError):
            y0 = np.zeros(0)
        if y0.shape != (S,) or not np.all(np.isfinite(y0)) or np.any(y0 < 0):
            raise ValueError("MassActionODELogLike: %sy0 must hold %d finite, non-negative amounts (numbers or Monomials)" % (who, S))
        for s, m in given.items():
            if monomials.setdefault(s, m) != m:
                raise ValueError("MassActionODELogLike: %sy0[%d] is %r, but another y0 gives this species %r: one Monomial per species"
                                 % (who, s, m, monomials[s]))
            y0[s] = np.nan
        return y0

    def _checked_inputs(self, inputs, who, like=None):
        """The inputs as a tuple of Input whose tables cover [t0, t[-1]] and whose working knots fit the experiment's limit.  like: the
        constructor's inputs, for a condition's own: the same species in the same order with the same gains, only the tables differ."""
        if inputs is None:
            return ()
        try:
            inputs = list(inputs)
        except TypeError:
            inputs = [inputs]
        if not all(isinstance(u, Input) for u in inputs):
            raise ValueError("MassActionODELogLike: %sinputs must be a sequence of Input objects (got %r)" % (who, inputs))
        if len(inputs) > ODE_MAX_INPUTS:
            raise ValueError("MassActionODELogLike: %sat most %d inputs are supported (got %d)" % (who, ODE_MAX_INPUTS, len(inputs)))
        t0, t_end = self.t0, self.t_last
        for i, u in enumerate(inputs):
            if not u.species < self.n_species:
                raise ValueError("MassActionODELogLike: %sinput %d names species %r (an int in 0..%d)" % (who, i, u.species, self.n_species - 1))
            if u.species in [v.species for v in inputs[:i]]:
                raise ValueError("MassActionODELogLike: %sinput %d: species %d already carries an input: one input per species" % (who, i, u.species))
            if not (u.times[0] <= t0 and u.times[-1] >= t_end):
                raise ValueError("MassActionODELogLike: %sinput %d: its table must cover t0 = %r .. t[-1] = %r (with a steady output: t_last; it covers %r .. %r)"
                                 % (who, i, t0, t_end, u.times[0], u.times[-1]))
        if like is not None and [(u.species, type(u.gain), u.gain) for u in inputs] != [(u.species, type(u.gain), u.gain) for u in like]:
            raise ValueError("MassActionODELogLike: %sinputs must name the constructor's input species in the same order with the same gains; "
                             "only the tables may differ" % who)
        knots = sum(len(u.working_knots(t0, t_end)) for u in inputs) + (len(inputs) if self._settles() else 0)
        if knots > ODE_MAX_INPUT_KNOTS:
            raise ValueError("MassActionODELogLike: %sat most %d working knots per experiment are supported, over all its inputs together (got %d)"
                             % (who, ODE_MAX_INPUT_KNOTS, knots))
        return tuple(inputs)

    def _check_input_species(self):
        """What an input species may not be: produced or consumed by a reaction, the target of an event, started from anything but 0."""
        for i, u in enumerate(self.inputs or ()):
            for r, (reac, prod, _) in enumerate(self.reactions):
                if reac.get(u.species, 0) != prod.get(u.species, 0):
                    raise ValueError("MassActionODELogLike: input %d: reaction %d produces or consumes species %d; an input species has net "
                                     "stoichiometry 0 in every reaction (a catalyst, a kinetic order, a Hill factor's species)" % (i, r, u.species))
            if u.species in self.y0_monomials:
                raise ValueError("MassActionODELogLike: input %d: y0[%d] is a Monomial; an input species starts from its table (y0 entry 0)" % (i, u.species))
            for c, e in enumerate(self._experiments()):
                who = "condition %d: " % c if self.conditions is not None else ""
                if e["y0"][u.species] != 0:
                    raise ValueError("MassActionODELogLike: %sinput %d: y0[%d] must be 0, the value comes from the table (got %r)"
                                     % (who, i, u.species, float(e["y0"][u.species])))
                for n, ev in enumerate(e["events"]):
                    if ev[1] == u.species:
                        raise ValueError("MassActionODELogLike: %sinput %d: event %d targets the input species %d" % (who, i, n, u.species))

    @property
    def t_last(self):
        """The end of the experiment's finite stretch: t[-1], or for an object with a steady output (t[-1] = inf) the last finite output
        time -- t0 if there is none."""
        t = self.t
        return float(t[-1]) if np.isfinite(t[-1]) else float(t[-2]) if len(t) > 1 else float(self.t0)

    def _settles(self):
        """t ends in inf: the generated network's SETTLE and the phase's six doubles in every experiment's block."""
        return bool(np.isinf(self.t[-1]))

    def _checked_equilibrate(self, eq, who):
        """None (no phase) or the phase's settings, every default filled in: dict(rtol, atol, horizon, max_step, max_steps)."""
        if eq is None or eq is False:
            return None
        return self._checked_phase(eq, who + "equilibrate", "None, False, True", max(self.t_last - self.t0, 1e-300), ODE_EQUILIBRATE_MAX_STEPS)

    def _checked_settle(self, st, who):
        """None (t is finite throughout) or the settings of the phase ahead of the steady output, as _checked_equilibrate gives them."""
        if not self._settles():
            if st is None or st is False:
                return None
            raise ValueError("MassActionODELogLike: %ssettle is given but t does not end in inf: the phase runs ahead of a steady output, "
                             "t = [..., inf] (got settle = %r)" % (who, st))
        if st is False:
            raise ValueError("MassActionODELogLike: %ssettle=False but t ends in inf: the output times are shared by all conditions, so the "
                             "phase ahead of the steady output cannot be switched off" % who)
        span = self.t_last - self.t0
        if span <= 0 and (st is None or st is True or (hasattr(st, "keys") and "horizon" not in st)):
            raise ValueError('MassActionODELogLike: %ssettle: "horizon" is required when no finite output time lies after t0 (t_last = t0): there is '
                             "no experiment whose length could say how long the state must stand still" % who)
        return self._checked_phase(st, who + "settle", "None, True", span, ODE_SETTLE_MAX_STEPS)

    def _checked_phase(self, eq, name, values, horizon, max_steps):
        """A steady-state phase's settings (equilibrate's or settle's; name: whose), every default filled in."""
        if eq is True or eq is None:
            eq = {}
        keys = ("rtol", "atol", "horizon", "max_step", "max_steps")
        if not hasattr(eq, "keys") or set(eq.keys()) - set(keys):
            raise ValueError('MassActionODELogLike: %s must be %s or a mapping with the keys "rtol", "atol", "horizon", '
                             '"max_step", "max_steps" (each optional; got %r)' % (name, values, eq))
        out = dict(rtol=eq.get("rtol", self.rtol), atol=eq.get("atol", self.atol), horizon=eq.get("horizon", horizon))
        for key in ("rtol", "atol", "horizon", "max_step"):
            if key == "max_step":
                out[key] = eq.get(key, 1e6 * out["horizon"])
            if not _is_real(out[key]) or not out[key] > 0:
                raise ValueError("MassActionODELogLike: %s: %s must be finite and > 0 (got %r)" % (name, key, out[key]))
            out[key] = float(out[key])
        n = eq.get("max_steps", max_steps)
        if not _is_int(n, 1):
            raise ValueError("MassActionODELogLike: %s: max_steps must be an integer >= 1 (got %r)" % (name, n))
        out["max_steps"] = int(n)
        return out

    def _checked_events(self, events, who):
        """The events as a tuple of (time, species, factor, amount), stably sorted by time (events at one time keep the order given)."""
        S, t0 = self.n_species, self.t0
        if events is None:
            return ()
        try:
            events = list(events)
        except TypeError:
            raise ValueError("MassActionODELogLike: %sevents must be a sequence of (time, species, factor, amount)" % who)
        if len(events) > ODE_MAX_EVENTS:
            raise ValueError("MassActionODELogLike: %sat most %d events per experiment are supported (got %d)" % (who, ODE_MAX_EVENTS, len(events)))
        out = []
        for e, event in enumerate(events):
            if not isinstance(event, (tuple, list)) or len(event) != 4:
                raise ValueError("MassActionODELogLike: %sevent %d must be (time, species, factor, amount)" % (who, e))
            time, species, factor, amount = event
            if not _is_real(time) or not t0 <= time <= self.t_last:     # (with a steady output: t_last, the last finite output time)
                raise ValueError("MassActionODELogLike: %sevent %d: the time must be finite and lie in t0 = %r <= time <= t[-1] = %r (got %r)"
                                 % (who, e, t0, self.t_last, time))
            if not _is_int(species, 0, S - 1):
                raise ValueError("MassActionODELogLike: %sevent %d names species %r (an int in 0..%d)" % (who, e, species, S - 1))
            if isinstance(factor, Monomial) or isinstance(amount, Monomial):
                raise ValueError("MassActionODELogLike: %sevent %d: factor and amount are numbers; a Monomial (a sampled dose) is not supported" % (who, e))
            if not _is_real(factor) or factor < 0 or not _is_real(amount) or amount < 0:
                raise ValueError("MassActionODELogLike: %sevent %d: factor and amount must be finite and >= 0 (got %r, %r)" % (who, e, factor, amount))
            out.append((float(time), int(species), float(factor), float(amount)))
        return tuple(sorted(out, key=lambda ev: ev[0]))

    def _checked_data(self, data, sd, who):
        O, T = len(self.observables), len(self.t)
        data, sd = np.asarray(data, dtype=float), np.asarray(sd, dtype=float)
        try:
            sd = np.broadcast_to(sd, data.shape) if data.shape == (O, T) else sd
        except ValueError:                      # (an sd that does not broadcast to O x T: the shape test below says so)
            pass
        if data.shape != (O, T) or sd.shape != (O, T):
            raise ValueError("MassActionODELogLike: %sdata and sd must be O x T = %d x %d" % (who, O, T))
        seen = np.isfinite(data)
        if np.any(np.isinf(data)) or not np.all(np.isfinite(sd[seen]) & (sd[seen] > 0)):
            raise ValueError("MassActionODELogLike: %sdata must be finite or NaN (not observed), and sd finite and > 0 where data is observed" % who)
        for q, z in enumerate(self.noise or []):
            if z is not None and z.scale == "log" and np.any(data[q][seen[q]] <= 0):
                raise ValueError('MassActionODELogLike: %sdata of observable %d must be > 0 where observed: its Noise has scale "log"' % (who, q))
        return data, np.array(sd)

    # ---- the data block (csrc/dz_ode.h) and the generated source
    def _experiments(self):
        """The object's experiments as a list of dict(y0, data, sd, events, equilibrate): the conditions, or the single experiment of the
        constructor's own values.  events () and equilibrate None where there are none (so for an object from before the keywords
        existed).  What tells the two kinds of object apart is `self.conditions is not None`: only then the data block has its
        [C, stride] header, the kernels are the item kernels and the host build's results have an axis of conditions."""
        own = [dict(y0=self.y0, data=self.data, sd=self.sd, events=self.events, equilibrate=self.equilibrate, settle=self.settle)]
        with_inputs = lambda e: dict(inputs=e.get("inputs") or self.inputs) if self.inputs else {}      # noqa: E731
        with_view = lambda e: dict(params=e.get("params") or {}) if self._has_view() else {}      # noqa: E731
        with_settle = lambda e: dict(settle=e.get("settle") or self.settle) if self._settles() else {}      # noqa: E731
        return [dict(y0=e["y0"], data=e["data"], sd=e["sd"], events=e.get("events") or (), equilibrate=e.get("equilibrate") or None, **with_inputs(e),
                     **with_view(e), **with_settle(e)) for e in (own if self.conditions is None else self.conditions)]

    def _input_knots(self, inputs):
        """One experiment's working knots as records (time, input, value, slope), sorted by time and at one time by input
        (csrc/dz_ode.h, INPUTS).  Ahead of a steady output (csrc/dz_ode.h, STEADY OUTPUT) every input is held: one more record per input
        behind all others, (t_last, i, u_i(t_last), 0)."""
        t0, t_end = self.t0, self.t_last
        knots = sorted((tau, float(i), v, s) for i, u in enumerate(inputs) for tau, v, s in u.working_knots(t0, t_end))
        if self._settles():
            knots += [(t_end, float(i), u.working_knots(t_end, t_end)[0][1], 0.0) for i, u in enumerate(inputs)]
        return knots

    def _max_input_knots(self):
        """Kmax: the largest count of working knots over the object's experiments (0: a network without inputs)."""
        return max(len(self._input_knots(e["inputs"])) for e in self._experiments()) if self.inputs else 0

    def _event_lists(self):
        """Every experiment's events."""
        return [e["events"] for e in self._experiments()]

    def _max_events(self):
        """Emax, the generated network's EVENTS: the largest event count over the object's experiments (0: a network without events)."""
        return max(len(ev) for ev in self._event_lists())

    def _equilibrate_list(self):
        """Every experiment's equilibration settings, None where it has none."""
        return [e["equilibrate"] for e in self._experiments()]

    def _equilibrates(self):
        """Some experiment of the object equilibrates: the generated network's EQUILIBRATE and the six doubles at each block's end."""
        return any(eq is not None for eq in self._equilibrate_list())

    def _experiment_block(self, y0, data, sd, events=(), equilibrate=None, inputs=(), params=None, settle=None):
        seen = np.isfinite(data)
        norm = self._norm_records(data, sd) if self.normalize else None
        if self.noise is None:
            C = float(np.sum(-np.log(sd[seen]) - _LOG_2PI_HALF))
        else:                                   # (csrc/dz_ode.h, NOISE: an entry's constant by its observable's model; "log": ln d in the data slot)
            const, data = np.zeros(data.shape), np.array(data)
            for q, z in enumerate(self.noise):
                with np.errstate(invalid="ignore", divide="ignore"):
                    if z is None:
                        const[q] = -np.log(sd[q]) - _LOG_2PI_HALF
                        continue
                    const[q] = -_LOG_2PI_HALF if z.dist == "normal" else -np.log(2.0)
                    if z.scale == "log":
                        data[q] = np.log(data[q])
                        const[q] = const[q] - data[q]
            C = float(np.sum(const[seen]))
        dat = np.where(seen, data, 0.0).T.reshape(-1)               # (time-major; unobserved: data 0, sd inf -> adds exactly 0)
        sd = np.where(seen, sd, np.inf).T.reshape(-1)
        blk = [[C, self.rtol, self.atol, float(self.max_steps), self.t0, float(len(self.t))], y0, self.t, dat, sd]
        emax = self._max_events()
        if emax:                                # (csrc/dz_ode.h: E_c, then Emax records padded with zeros -- one stride for all conditions)
            rec = np.zeros((emax, 4))
            rec[:len(events)] = np.asarray(events, dtype=float).reshape(-1, 4)
            blk += [[float(len(events))], rec.reshape(-1)]
        if self._equilibrates():                # (csrc/dz_ode.h: on, rtol_ss, atol_ss, horizon, max_step, max_steps_ss at the very end)
            eq = equilibrate
            blk += [[1.0, eq["rtol"], eq["atol"], eq["horizon"], eq["max_step"], float(eq["max_steps"])] if eq else [0.0] * 6]
        if settle is not None:                  # (csrc/dz_ode.h, STEADY OUTPUT: the phase's six doubles behind the equilibration's, in front of the knots)
            blk += [[1.0, settle["rtol"], settle["atol"], settle["horizon"], settle["max_step"], float(settle["max_steps"])]]
        if self.inputs:                         # (csrc/dz_ode.h: K_c, then Kmax records padded with zeros, behind everything else)
            knots = self._input_knots(inputs)
            rec = np.zeros((self._max_input_knots(), 4))
            rec[:len(knots)] = np.asarray(knots, dtype=float).reshape(-1, 4)
            blk += [[float(len(knots))], rec.reshape(-1)]
        if norm:                                # (csrc/dz_ode.h, NORMALISED READOUTS: behind the knots, in front of the view's pairs)
            blk += [norm]
        if params is not None:                  # (csrc/dz_ode.h, VIEWS: the P pairs (j_i, v_i) at the very end)
            blk += [self._view_table(params)]
        return np.concatenate(blk)

    def condition_block(self, c=0):
        """One experiment's block: condition c's, or (without conditions) the constructor's own."""
        return self._experiment_block(**self._experiments()[c if self.conditions is not None else 0])

    def data_block(self):
        """The block the kernels read (csrc/dz_ode.h): one experiment's, or with conditions [C, stride] and the C experiments' blocks."""
        blocks = [self._experiment_block(**e) for e in self._experiments()]
        return np.concatenate(([[float(len(blocks)), float(len(blocks[0]))]] if self.conditions is not None else []) + blocks)

    def _per_point(self, results):
        """[n, C, ...] from the host build as the caller sees it: the axis of conditions only for an object made with conditions"""
        return results if self.conditions is not None else results[:, 0]

    def _monomials(self):
        """What the generated network needs beyond rate constants of one parameter each, or None: then the source is what it always was
        (a scale factor of exactly 1.0 multiplies nothing)."""
        if (self.y0_monomials or self.constraints or any(isinstance(_rate(r[2]), Monomial) for r in self.reactions)
                or (self.scale is not None and any(f != 1.0 for f in self.scale))):
            return dict(y0=self.y0_monomials, scale=self.scale, constraints=self.constraints)
        return None

    def source(self):
        return _ode_source.generate(self)

    @staticmethod
    def _header_hash(name="dz_ode.h"):
        import hashlib
        import os
        with open(os.path.join(csrc_dir(), name), "rb") as fh:
            return hashlib.sha256(fh.read()).hexdigest()

    def _unit(self):
        """The translation unit both builds compile: the generated source and the hashes of the headers it includes (the cache key)."""
        text = self.source() + "\n// dz_ode.h " + self._header_hash() + "\n"
        if self.lanes_per_point != 1:
            text += "// dz_ode_group.h " + self._header_hash("dz_ode_group.h") + "\n"
        return text

    def code_object(self):
        """The gfx950 code object (kernel dz_ode_batch, or dz_ode_group_batch for a lane group; with conditions dz_ode_item_batch or
        dz_ode_group_item_batch), compiled with hipcc on first use and cached; the key includes csrc/dz_ode.h (and csrc/dz_ode_group.h)."""
        if self.path is None:
            self.path = compile_device_kernel(self._unit(), extra_flags=("-I" + csrc_dir(),))
        return self.path

    def predict_source(self):
        """The prediction kernels' translation unit: source() behind the one line that switches the entry macros (csrc/dz_ode.h, PREDICTION)."""
        return "#define DZODE_PREDICT 1\n" + self.source()

    def predict_kernel(self):
        """The name of the one kernel predict_code_object() exports."""
        return "dz_ode%s%s_predict" % ("" if self.lanes_per_point == 1 else "_group", "" if self.conditions is None else "_item")

    def predict_code_object(self):
        """The gfx950 code object of the prediction kernel (predict_kernel()), compiled with hipcc on first use and cached under a key of
        its own (the unit's first line differs); always from the source, also for an object made with path=."""
        if getattr(self, "_predict_path", None) is None:
            self._predict_path = compile_device_kernel("#define DZODE_PREDICT 1\n" + self._unit(), extra_flags=("-I" + csrc_dir(),))
        return self._predict_path

    def device(self, device=0, max_bytes=256 << 20, chunk_items=None):
        """An ODEDeviceEvaluator of this object on GPU `device` (the class docstring, Prediction); DreamZSError without a GPU."""
        return ODEDeviceEvaluator(self, device=device, max_bytes=max_bytes, chunk_items=chunk_items)

    def with_outputs(self, t, t0=None):
        """A sibling object with the output times t (and start time t0, default: this object's) and every data entry NaN: the same
        network, conditions, y0, events, equilibration, scale and noise (the class docstring, Prediction).  `normalize` carries over
        too: it is checked again against the new times -- a "ref" whose time is not among them is refused -- and the extrema and the
        reference are taken over the new grid, so the maximum over a denser grid is a different number."""
        import copy
        new = copy.copy(self)
        lim = self._checked_shape(self.n_species, self.lanes_per_point, len(self.reactions))[2]
        new.t, new.t0, _ = self._checked_times(t, self.t0 if t0 is None else t0, self.observables, self.n_species, lim)
        shape = (len(self.observables), len(new.t))
        new.data, new.sd = np.full(shape, np.nan), np.ones(shape)
        new.normalize = new._checked_normalize(self.normalize, new.t)    # (a "ref" must name one of the new times; extrema run over the new grid)
        resettle = lambda st, who: (st or new._checked_settle(None, who)) if new._settles() else None      # noqa: E731  (the phase's settings carry over)
        new.settle = resettle(self.settle, "")
        new.events = new._checked_events(self.events, "") or None
        new.inputs = new._checked_inputs(self.inputs, "") or None       # (the tables must cover the new span; the working knots follow it)
        if self.conditions is not None:
            new.conditions = [dict({k: v for k, v in cond.items() if k != "settle"}, data=new.data, sd=new.sd,
                                   events=new._checked_events(cond["events"], "condition %d: " % c),
                                   **({"settle": resettle(cond.get("settle"), "condition %d: " % c)} if new._settles() else {}),
                                   **({"inputs": new._checked_inputs(cond["inputs"], "condition %d: " % c)} if cond.get("inputs") else {}))
                              for c, cond in enumerate(self.conditions)]
        new.path, new._host, new._predict_path = None, None, None
        return new

    def _dz_apply(self, engine):
        kernel = "dz_ode%s%s_batch" % ("" if self.lanes_per_point == 1 else "_group", "" if self.conditions is None else "_item")
        engine.set_likelihood_module(self.code_object(), kernel, self.lanes_per_point, self.data_block(), False, items_per_point=len(self._experiments()))

    # ---- the host build
    def host_library(self):
        """The same generated source compiled for the host (x86-64 SSE2 doubles, -O2 -ffp-contract=off), loaded with ctypes; cached."""
        if self._host is None:
            import ctypes as C
            import os
            cc = "/opt/rocm/llvm/bin/clang++" if os.path.exists("/opt/rocm/llvm/bin/clang++") else "g++"
            flags = ["-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-shared", "-I" + csrc_dir()]
            so = _build_cached(self._unit(), ".so", ".cpp", lambda src, out: [cc] + flags + ["-o", out, src, "-lm"],
                               (os.path.basename(cc), " for the host build of the ODE likelihood"), [cc, _compiler_version(cc)] + flags)
            L = C.CDLL(so)
            P, I64, D, I = C.POINTER(C.c_double), C.c_longlong, C.c_double, C.c_int
            L.dzode_loglike.argtypes = [P, I64, I, P, P, C.POINTER(C.c_int)]
            L.dzode_simulate.argtypes = [P, I64, I, P, P, P]
            L.dzode_fixed.argtypes = [P, P, D, I, I, P]
            L.dzode_fixed.restype = I
            L.dzode_constraints.argtypes = [P, I64, I, P]
            L.dzode_equilibrate.argtypes = [P, I64, I, P, P, C.POINTER(C.c_int)]
            L.dzode_settle.argtypes = [P, I64, I, P, P, C.POINTER(C.c_int)]
            L.dzode_noise.argtypes = [P, I64, I, P]
            L.dzode_exp.argtypes = L.dzode_log.argtypes = [D]
            L.dzode_exp.restype = L.dzode_log.restype = D
            self._host = L
        return self._host

    def _rows(self, X):
        X = np.ascontiguousarray(np.asarray(X, dtype=float))
        X = X.reshape(-1, X.shape[-1] if X.ndim else 1)
        if X.shape[1] < self.d:
            raise ValueError("MassActionODELogLike: points have %d coordinates, the model reads %d" % (X.shape[1], self.d))
        return X

    def _host_call(self, name, *args):
        """The host build's function `name`: arrays go as pointers to their doubles (an int32 array: to its ints), the rest as it is."""
        import ctypes as C
        ptr = lambda a: a.ctypes.data_as(C.POINTER(C.c_int if a.dtype == np.int32 else C.c_double))      # noqa: E731
        return getattr(self.host_library(), name)(*[ptr(a) if isinstance(a, np.ndarray) else a for a in args])

    def batch(self, X, return_steps=False):
        """Host-build log-likelihoods of the rows of X (and the accepted steps of each integration; with conditions: of all of them)."""
        X = self._rows(X)
        out, st = np.zeros(len(X)), np.zeros(len(X), dtype=np.int32)
        self._host_call("dzode_loglike", X, len(X), X.shape[1], self.data_block(), out, st)
        return (out, st) if return_steps else out

    def __call__(self, x):
        return float(self.batch(np.asarray(x, dtype=float).reshape(1, -1))[0])

    def simulate(self, X):
        """The observables at the output times, [n, T, O] -- with conditions [n, C, T, O] -- (NaN where the integration failed), from the
        host build."""
        X = self._rows(X)
        lead = (len(X), len(self._experiments()))
        sim, like = np.full(lead + (len(self.t), len(self.observables)), np.nan), np.zeros(lead)
        self._host_call("dzode_simulate", X, len(X), X.shape[1], self.data_block(), sim, like)
        sim[like == -np.inf] = np.nan
        return self._per_point(sim)

    def batch_conditions(self, X):
        """The per-condition log-likelihoods of the rows of X, [n, C], from the host build: column c is what an object made of condition c
        alone returns, and batch(X) their sum from left to right."""
        if self.conditions is None:
            raise ValueError("MassActionODELogLike: batch_conditions needs an object made with conditions=[...]")
        X = self._rows(X)
        terms = np.zeros((len(X), len(self.conditions)))
        self._host_call("dzode_simulate", X, len(X), X.shape[1], self.data_block(), None, terms)
        return terms

    def steady_state(self, X, return_steps=False):
        """The state handed to the experiment, before the events at t0, from the host build: [n, S], with conditions [n, C, S].  An
        experiment that equilibrates gives the state at which the steady-state test passed (NaN where the phase failed or the point is
        not live), one that does not gives its y0.  return_steps: also the ATTEMPTED steps of the phase, [n] or [n, C] -- what the
        phase's max_steps counts."""
        X = self._rows(X)
        lead = (len(X), len(self._experiments()))
        y, st = np.full(lead + (self.n_species,), np.nan), np.zeros(lead, dtype=np.int32)
        self._host_call("dzode_equilibrate", X, len(X), X.shape[1], self.data_block(), y, st)
        return (self._per_point(y), self._per_point(st)) if return_steps else self._per_point(y)

    def settled_state(self, X, return_attempts=False):
        """The state the steady output is measured at, from the host build: [n, S], with conditions [n, C, S] -- the state at which the
        phase's steady-state test passed, after everything due at t_last (csrc/dz_ode.h, STEADY OUTPUT); NaN where the item failed.
        return_attempts: also the ATTEMPTED steps of the phase, [n] or [n, C] -- what settle's max_steps counts.  The twin of
        steady_state at the experiment's other end; only for an object whose t ends in inf."""
        if not self._settles():
            raise ValueError("MassActionODELogLike: settled_state needs an object with a steady output, t = [..., inf]")
        X = self._rows(X)
        lead = (len(X), len(self._experiments()))
        y, st = np.full(lead + (self.n_species,), np.nan), np.zeros(lead, dtype=np.int32)
        self._host_call("dzode_settle", X, len(X), X.shape[1], self.data_block(), y, st)
        return (self._per_point(y), self._per_point(st)) if return_attempts else self._per_point(y)

    def constraint_terms(self, X):
        """g(x) = sum over the constraints of norm(loc, sd).logpdf(monomial) for the rows of X, from the host build: what the single
        experiment's value, or condition 0's term, holds beyond the data's likelihood (0 without constraints; -inf where a coordinate
        that a monomial or a rate reads, or a monomial's value, is not finite)."""
        X = self._rows(X)
        if self._has_view():                    # (through condition 0's view: the term the constraints are added to)
            X = np.ascontiguousarray(self.viewed(X, 0))
        g = np.zeros(len(X))
        self._host_call("dzode_constraints", X, len(X), X.shape[1], g)
        return g

    def noise_values(self, X):
        """The per-point noise values of the rows of X, [n, O, 2], from the host build: (a_q, b_q) = (sigma_q, rel_q) as the kernels hold
        them (csrc/dz_ode.h, NOISE), whether or not the point is live.  NaN for an observable without a Noise; b is 0 without rel."""
        X = self._rows(X)
        if self._has_view():                    # (each condition's own values: [n, C, O, 2])
            return np.stack([self._noise_values(np.ascontiguousarray(self.viewed(X, c))) for c in range(len(self.conditions))], axis=1)
        return self._noise_values(X)

    def _noise_values(self, X):
        ab = np.full((len(X), len(self.observables), 2), np.nan)
        self._host_call("dzode_noise", X, len(X), X.shape[1], ab)
        return ab

    def fixed_steps(self, x, t1, nsteps, embedded=False, condition=0):
        """The state at t1 after nsteps equal steps from (t0, y0): the order-4 solution, or the embedded order-3 one (order test).
        condition: whose y0, for an object made with conditions.  Inputs are ignored, as events are: every drive is 0 and an input
        species stays at its y0 entry, 0."""
        x = np.ascontiguousarray(np.asarray(x, dtype=float).reshape(-1))
        if self._has_view():                    # (the condition's view of the point)
            x = np.ascontiguousarray(self.viewed(x.reshape(1, -1), condition)[0])
        y = np.zeros(self.n_species)
        ok = self._host_call("dzode_fixed", x, self.condition_block(condition), float(t1), int(nsteps), int(bool(embedded)), y)
        return y if ok else np.full(self.n_species, np.nan)

    def __getstate__(self):                      # (the host library is a handle of this process: loaded again on first use)
        st = dict(self.__dict__); st["_host"] = None
        return st


class ODEDeviceEvaluator:
    """MassActionODELogLike.device(): the object's batch, batch_conditions and simulate evaluated by the device kernels, on an arbitrary
    batch outside the sampler (the class docstring of MassActionODELogLike, Prediction).  It owns a small engine (three chains, no prior)
    that is made on first use and freed by close() or on leaving the `with` block; the likelihood module is set on the first batch(), the
    output module -- and the prediction code object compiled -- on the first simulate() or batch_conditions().

    Chunks: a call processes its rows in chunks of WHOLE points, so no chunk ends in the middle of a point's conditions: points per
    chunk = max(1, chunk_items // C) when chunk_items is given, else as many as keep the output buffer (C * T * O doubles per point)
    within max_bytes, at least one."""

    def __init__(self, like, device=0, max_bytes=256 << 20, chunk_items=None):
        if chunk_items is not None and int(chunk_items) < 1:
            raise ValueError("ODEDeviceEvaluator: chunk_items must be >= 1")
        if int(max_bytes) < 1:
            raise ValueError("ODEDeviceEvaluator: max_bytes must be >= 1")
        self.like, self.device_index, self.max_bytes = like, int(device), int(max_bytes)
        self.chunk_items = None if chunk_items is None else int(chunk_items)
        self._engine, self._have_like, self._have_out = None, False, False
        self._open()                            # (no GPU, no library: DreamZSError here, not at the first call)

    def _open(self):
        if self._engine is None:
            from . import _capi
            self._engine = _capi.Engine(nchains=3, ndim=max(self.like.d, 1), history_capacity=8, device=self.device_index)
            self._have_like = self._have_out = False
        return self._engine

    def close(self):
        if self._engine is not None:
            self._engine.close()
            self._engine = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def __getstate__(self):                      # (the engine is a device handle: made again on first use)
        st = dict(self.__dict__); st["_engine"] = None; st["_have_like"] = st["_have_out"] = False
        return st

    def _shape(self):
        like = self.like
        return len(like._experiments()), len(like.t) * len(like.observables)

    def points_per_chunk(self):
        """The points of one launch (whole points: see the class docstring)."""
        C, per = self._shape()
        items = self.chunk_items if self.chunk_items is not None else self.max_bytes // (8 * per)
        return int(min(max(1, items // C), 1 << 22))

    def _chunks(self, X):
        """The rows as the engine takes them ([n, max(d, 1)]: the kernels read the first d coordinates), in chunks of whole points."""
        X = self.like._rows(X)
        d = self.like.d
        X = np.ascontiguousarray(X[:, :d]) if d else np.zeros((len(X), 1))
        step = self.points_per_chunk()
        return len(X), [X[i:i + step] for i in range(0, len(X), step)]

    def batch(self, X):
        """The log-likelihoods of the rows of X by the likelihood kernel (dz_eval_logp, no prior): the bits of the host batch(X)."""
        eng = self._open()
        if not self._have_like:
            self.like._dz_apply(eng)
            self._have_like = True
        n, chunks = self._chunks(X)
        return np.concatenate([eng.eval_logp(c)[1] for c in chunks]) if n else np.zeros(0)

    def _outputs(self, X):
        like = self.like
        C, per = self._shape()
        eng = self._open()
        if not self._have_out:
            eng.set_output_module(like.predict_code_object(), like.predict_kernel(), like.lanes_per_point, C, per, like.data_block())
            self._have_out = True
        n, chunks = self._chunks(X)
        terms, sim = np.zeros((n, C)), np.zeros((n, C, len(like.t), len(like.observables)))
        i = 0
        for c in chunks:
            tc, oc = eng.eval_outputs(c)
            terms[i:i + len(c)], sim[i:i + len(c)] = tc, oc.reshape((len(c),) + sim.shape[1:])
            i += len(c)
        return terms, sim

    def batch_conditions(self, X):
        """The per-condition terms of the rows of X, [n, C], by the prediction kernel: the bits of the host batch_conditions(X)."""
        if self.like.conditions is None:
            raise ValueError("MassActionODELogLike: batch_conditions needs an object made with conditions=[...]")
        return self._outputs(X)[0]

    def simulate(self, X, return_terms=False):
        """The scaled observables at the output times, [n, T, O] or [n, C, T, O], NaN where the item failed, by the prediction kernel: the
        bits of the host simulate(X).  return_terms: also the items' terms, [n] or [n, C]."""
        terms, sim = self._outputs(X)
        terms, sim = self.like._per_point(terms), self.like._per_point(sim)
        return (sim, terms) if return_terms else sim


def posterior_predictive(sampled_params, like, burnin=0, thin=1, device=True, t=None):
    """The trajectories of a posterior sample: (rows, sim).  sampled_params: the chains run_dream returned (a sequence of [niterations, d]
    arrays); rows: from each chain in turn the iterations burnin, burnin + thin, burnin + 2 thin, ..., stacked chain after chain;
    sim = simulate(rows) of `like`, or with t of like.with_outputs(t) (a denser grid for smooth curves) -- on the device (device=True:
    like.device(), or an int: that GPU) or by the host build (device=False), the same bits either way.  Noise replicates are the caller's:
    numpy draws around sim with like.noise_values(rows)."""
    if not _is_int(burnin, 0) or not _is_int(thin, 1):
        raise ValueError("posterior_predictive: burnin must be an integer >= 0 and thin an integer >= 1")
    chains = [np.asarray(c, dtype=float) for c in sampled_params]
    if not chains or any(c.ndim != 2 or c.shape[1] != chains[0].shape[1] for c in chains):
        raise ValueError("posterior_predictive: sampled_params must be a sequence of [niterations, d] arrays of one d")
    rows = np.concatenate([c[int(burnin)::int(thin)] for c in chains])
    model = like if t is None else like.with_outputs(t)
    if device is False:
        return rows, model.simulate(rows)
    with model.device(device=0 if device is True else int(device)) as ev:
        return rows, ev.simulate(rows)
