"""Built-in likelihoods that run on the device ("batched device callback").

Each object is an ordinary Python callable ``f(x[d]) -> float`` (so it also works with the
reference), and carries a descriptor that ``run_dream`` hands to ``dz_set_likelihood_*`` so the
evaluation happens inside the HIP kernels instead of on the host.
"""
import numpy as np


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


_COMPILER_VERSION = {}
_FALLBACK_DIR = []


def _hipcc():
    import os
    return next((c for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc") if c and os.path.exists(c)), "hipcc")


def _compiler_version(cc):
    """`cc --version` (memoised per process), part of the cache key: an object is only as current as the compiler that made it."""
    import subprocess
    if cc not in _COMPILER_VERSION:
        try:
            _COMPILER_VERSION[cc] = subprocess.run([cc, "--version"], capture_output=True, text=True).stdout
        except OSError:
            _COMPILER_VERSION[cc] = ""
    return _COMPILER_VERSION[cc]


def _private_dir(path):
    """path is a directory (not a link) owned by this user and writable by nobody else."""
    import os
    import stat
    try:
        st = os.lstat(path)
    except OSError:
        return False
    return stat.S_ISDIR(st.st_mode) and st.st_uid == os.getuid() and not (st.st_mode & (stat.S_IWGRP | stat.S_IWOTH))


def kernel_cache_dir():
    """Where compiled likelihood objects are kept: $DREAMZS_KERNEL_CACHE (default ~/.cache/dreamzs_kernels) if it can be written, else
    <tmpdir>/dreamzs_kernels_<uid>.  The last one has a predictable name in a shared directory, so it is created with mode 0700 and
    used only while it is a directory owned by this user and not group- or world-writable; otherwise a fresh private directory
    (mkdtemp) serves this process.  Objects found in the cache are loaded and run, so nobody else may be able to write there."""
    import os
    import tempfile
    cdir = os.environ.get("DREAMZS_KERNEL_CACHE") or os.path.join(os.path.expanduser("~"), ".cache", "dreamzs_kernels")
    try:
        os.makedirs(cdir, exist_ok=True)
        if not os.access(cdir, os.W_OK):
            raise OSError("not writable")
        return cdir
    except OSError:
        pass
    cdir = os.path.join(tempfile.gettempdir(), "dreamzs_kernels_%d" % os.getuid())
    try:
        os.mkdir(cdir, 0o700)
    except OSError:
        pass
    if _private_dir(cdir):
        return cdir
    if not _FALLBACK_DIR or not _private_dir(_FALLBACK_DIR[0]):
        _FALLBACK_DIR[:] = [tempfile.mkdtemp(prefix="dreamzs_kernels_")]
    return _FALLBACK_DIR[0]


def _build_cached(text, suffix, src_ext, cmd_for, what, cached_key_parts, out_path=None):
    # what: (the compiler's name, what it was building) for the error messages
    """Compile `text` with the command cmd_for(src, out) into out_path or, without one, into the kernel cache under a key of
    (cached_key_parts, text).  Built beside the target under a name unique to the process and thread, then renamed into place:
    concurrent builders never see half a file."""
    import hashlib
    import os
    import subprocess
    import threading
    cached = out_path is None
    if cached:
        key = hashlib.sha256(("\0".join(cached_key_parts) + "\0" + text).encode()).hexdigest()[:32]
        out_path = os.path.join(kernel_cache_dir(), key + suffix)
        if os.path.exists(out_path) and os.path.getsize(out_path) > 0:
            return out_path
    tmp = "%s.%d.%d.tmp" % (out_path, os.getpid(), threading.get_ident())
    src = tmp + src_ext
    with open(src, "w") as f:
        f.write(text)
    cmd = cmd_for(src, tmp)
    try:
        res = subprocess.run(cmd, capture_output=True, text=True)
    except OSError as ex:          # (no compiler on this machine: say so -- a code object built elsewhere can be given by path)
        os.remove(src)
        raise Exception("%s failed%s: cannot run %r (%s); set HIPCC, or build the code object where ROCm is installed and pass its path" % (what + (cmd[0], ex)))
    try:
        os.remove(src) if cached else os.replace(src, out_path + src_ext)
    except OSError:
        pass
    if res.returncode != 0:
        if os.path.exists(tmp):
            os.remove(tmp)
        raise Exception("%s failed%s:\n%s" % (what + (res.stderr[-4000:],)))
    os.replace(tmp, out_path)
    return out_path


def compile_device_kernel(source, out_path=None, extra_flags=(), arch="gfx950"):
    """HIP source text -> a code object (.hsaco) for DeviceKernelLogLike: `hipcc --offload-arch=<arch> --genco` (arch: the engine is built
    for gfx950, the MI355X; the argument is there so that an error names what was asked for).
    -ffp-contract=off is on by default so that a density written with + and * rounds like the same expression in numpy (a host
    likelihood and its device twin then make the same accept / reject decisions bit for bit); pass extra_flags=("-ffp-contract=fast",)
    to let the compiler fuse.  Without out_path the code object is CACHED under a key of (source, flags, arch, `hipcc --version`) in
    kernel_cache_dir(): the same source is compiled once, by whichever process or unpickled copy asks first (advisor, round 5: a fresh
    temporary directory and a fresh hipcc run per call).  Returns the path."""
    text = source if "hip_runtime.h" in source else "#include <hip/hip_runtime.h>\n" + source
    flags = ["--offload-arch=%s" % arch, "--genco", "--no-gpu-bundle-output", "-O3", "-std=c++17", "-ffp-contract=off"] + list(extra_flags)
    hipcc = _hipcc()
    key = flags + ([_compiler_version(hipcc)] if out_path is None else [])
    return _build_cached(text, ".hsaco", ".hip", lambda src, out: [hipcc] + flags + ["-o", out, src],
                         ("hipcc", " for the device likelihood (--offload-arch=%s)" % arch), key, out_path)


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


def csrc_dir():
    import os
    return os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc")


class DeviceFunctionLogLike:
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

    def __call__(self, x):
        if self.host is not None:
            return self.host(np.asarray(x, dtype=float))
        if self._eval_engine is None:
            from . import _capi
            self._eval_engine = _capi.Engine(nchains=3, ndim=self.d, history_capacity=8)
            self._dz_apply(self._eval_engine)
        return float(self._eval_engine.eval_logp(np.asarray(x, dtype=float).reshape(1, self.d))[1][0])

    def __getstate__(self):
        st = dict(self.__dict__); st["_eval_engine"] = None
        return st


class DeviceKernelLogLike:
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


# ---------------------------------------------------------------------------------------------------- mass-action ODE models
ODE_LIMITS = dict(species=8, reactions=64, observables=8, times=4096)
ODE_GROUP_LIMITS = dict(species=32, reactions=128, observables=16, times=4096, lanes=(16, 32), conditions=64)      # lanes_per_point=16 | 32: species <= lanes
ODE_WAVE_LIMITS = dict(species=64, reactions=256, observables=16, times=4096, lanes=(64,), conditions=64)            # lanes_per_point=64: 33..64 species
ODE_MAX_CONSTRAINTS = 16    # constraints=[(Monomial, loc, sd), ...]
ODE_MAX_EVENTS = 16         # events=[(time, species, factor, amount), ...] per experiment
ODE_EQUILIBRATE_MAX_STEPS = 2000    # equilibrate=...: the attempted steps of the phase before the experiment, unless its "max_steps" says otherwise
ODE_MAX_CONDITIONS = 64     # conditions=[...], either shape: the engine's DZ_MAX_LIKELIHOOD_ITEMS (ODE_LIMITS: the one-lane shape's own four limits)
_LOG_2PI_HALF = 0.5 * np.log(2.0 * np.pi)


def _hexlit(v):
    """A C++17 hexadecimal floating literal: the double exactly."""
    v = float(v)
    return "(%s)" % v.hex() if np.isfinite(v) else ("(__builtin_huge_val())" if v > 0 else "(-__builtin_huge_val())")


class Monomial:
    """10**(log10_factor + sum_i exponents[i] * x[i]): a product of powers of the sampled constants 10**x[i] times a fixed factor, for
    MassActionODELogLike -- a reaction's rate constant (kr = KD kf: Monomial({i: 1}, log10(kf)); a rate closed by a thermodynamic cycle,
    k4 = k1 k2 / k3: Monomial({0: 1, 1: 1, 2: -1})), a sampled start amount, an observable's scale factor, or the argument of a Gaussian
    constraint.  exponents: a non-empty mapping from parameter index to a finite, non-zero float; log10_factor: finite.  An immutable
    value: `exponents` is the tuple of (index, exponent) pairs in ascending index, the order in which the device and the host build add
    them (csrc/dz_ode.h)."""
    __slots__ = ("exponents", "log10_factor")

    def __init__(self, exponents, log10_factor=0.0):
        if not hasattr(exponents, "items") or len(exponents) == 0:
            raise ValueError("MassActionODELogLike: a Monomial's exponents must be a non-empty mapping {parameter index: exponent}")
        pairs = []
        for i, e in exponents.items():
            if isinstance(i, bool) or not isinstance(i, (int, np.integer)) or i < 0:
                raise ValueError("MassActionODELogLike: a Monomial's parameter index must be a non-negative integer (got %r)" % (i,))
            if isinstance(e, bool) or not isinstance(e, (int, np.integer, float, np.floating)) or not np.isfinite(e) or e == 0:
                raise ValueError("MassActionODELogLike: a Monomial's exponent must be a finite, non-zero number (got %r for index %d)" % (e, i))
            pairs.append((int(i), float(e)))
        if isinstance(log10_factor, bool) or not isinstance(log10_factor, (int, np.integer, float, np.floating)) or not np.isfinite(log10_factor):
            raise ValueError("MassActionODELogLike: a Monomial's log10_factor must be finite (got %r)" % (log10_factor,))
        object.__setattr__(self, "exponents", tuple(sorted(pairs)))
        object.__setattr__(self, "log10_factor", float(log10_factor))

    def __setattr__(self, name, value):
        raise AttributeError("a Monomial is immutable")

    __delattr__ = __setattr__

    @property
    def indices(self):
        return tuple(i for i, _ in self.exponents)

    def value(self, x):
        """10.0**(log10_factor + sum e_i x[i]) in numpy (the solvers' own arithmetic: csrc/dz_ode.h), for the rows of x"""
        x = np.asarray(x, dtype=float)
        s = self.log10_factor
        for i, e in self.exponents:
            s = s + e * x[..., i]
        return 10.0 ** s

    def __eq__(self, other):
        return isinstance(other, Monomial) and self.exponents == other.exponents and self.log10_factor == other.log10_factor

    def __hash__(self):
        return hash((self.exponents, self.log10_factor))

    def __reduce__(self):
        return Monomial, (dict(self.exponents), self.log10_factor)

    def __repr__(self):
        return "Monomial(%r, %r)" % (dict(self.exponents), self.log10_factor)


_INT = (int, np.integer)
_REAL = (int, np.integer, float, np.floating)
ODE_MAX_HILL_EXPONENT = 8   # Hill(species, K, n): n = 1..8, powers as repeated products
ODE_MAX_RATE_FACTORS = 4    # RateLaw(rate, factors): at most 4 Hill factors per reaction


def _checked_constant(v, what):
    """A rate constant or a Hill constant as the generators take it: a parameter index (int), a float or a Monomial."""
    if isinstance(v, Monomial):
        return v
    if isinstance(v, bool) or not isinstance(v, _REAL):
        raise ValueError("MassActionODELogLike: %s is a parameter index (int), a fixed constant (float) or a Monomial (got %r)" % (what, v))
    if isinstance(v, _INT):
        if v < 0:
            raise ValueError("MassActionODELogLike: %s: parameter index %d is negative" % (what, v))
        return int(v)
    return float(v)


class Hill:
    """A saturating factor of one species in a RateLaw: y^n / (K^n + y^n) for kind "activation", K^n / (K^n + y^n) for "repression".
    species: the species' index; K: a parameter index (10**x[i] under rate_scale "log10", x[i] under "linear"), a finite float > 0 or a
    Monomial; n: an integer 1..8 (ODE_MAX_HILL_EXPONENT; powers are repeated products).  An immutable value."""
    __slots__ = ("species", "K", "n", "kind")

    def __init__(self, species, K, n=1, kind="activation"):
        if isinstance(species, bool) or not isinstance(species, _INT) or species < 0:
            raise ValueError("MassActionODELogLike: a Hill factor's species must be a non-negative integer (got %r)" % (species,))
        K = _checked_constant(K, "a Hill factor's K")
        if isinstance(K, float) and not (np.isfinite(K) and K > 0):
            raise ValueError("MassActionODELogLike: a Hill factor's fixed K must be finite and > 0 (got %r)" % (K,))
        if isinstance(n, bool) or not isinstance(n, _INT) or not 1 <= n <= ODE_MAX_HILL_EXPONENT:
            raise ValueError("MassActionODELogLike: a Hill factor's n must be an integer 1..%d (got %r)" % (ODE_MAX_HILL_EXPONENT, n))
        if kind not in ("activation", "repression"):
            raise ValueError('MassActionODELogLike: a Hill factor\'s kind must be "activation" or "repression" (got %r)' % (kind,))
        for name, v in zip(self.__slots__, (int(species), K, int(n), kind)):
            object.__setattr__(self, name, v)

    def __setattr__(self, name, value):
        raise AttributeError("a Hill factor is immutable")

    def __delattr__(self, name):
        raise AttributeError("a Hill factor is immutable")

    def _key(self):
        return (self.species, type(self.K).__name__, self.K, self.n, self.kind)

    def __eq__(self, other):
        return isinstance(other, Hill) and self._key() == other._key()

    def __hash__(self):
        return hash(self._key())

    def __reduce__(self):
        return Hill, (self.species, self.K, self.n, self.kind)

    def __repr__(self):
        return "Hill(%r, %r, %r, %r)" % (self.species, self.K, self.n, self.kind)


class RateLaw:
    """A reaction's rate beyond mass action, where its third element stands: v = k * prod_s y_s^order_s * prod_m h_m(y).
    rate: what the third element may be without it (a parameter index, a float, a Monomial); factors: at most 4 (ODE_MAX_RATE_FACTORS)
    Hill objects, multiplied in the order given; order: None -- the kinetic orders are the reactants' coefficients -- or a mapping
    {species: non-negative integer} that replaces them (kinetics apart from stoichiometry; {}: no mass-action factor).  An immutable
    value: `factors` is a tuple, `order` None or the tuple of (species, order) pairs in ascending species, zeros dropped."""
    __slots__ = ("rate", "factors", "order")

    def __init__(self, rate, factors=(), order=None):
        if isinstance(rate, RateLaw):
            raise ValueError("MassActionODELogLike: a RateLaw's rate is a parameter index, a float or a Monomial, not another RateLaw")
        rate = _checked_constant(rate, "a RateLaw's rate")
        if isinstance(rate, float) and not np.isfinite(rate):
            raise ValueError("MassActionODELogLike: a RateLaw's fixed rate constant must be finite (got %r)" % (rate,))
        try:
            factors = tuple(factors)
        except TypeError:
            factors = (factors,)
        if not all(isinstance(f, Hill) for f in factors):
            raise ValueError("MassActionODELogLike: a RateLaw's factors must be Hill objects (got %r)" % (factors,))
        if len(factors) > ODE_MAX_RATE_FACTORS:
            raise ValueError("MassActionODELogLike: a RateLaw has at most %d factors (got %d)" % (ODE_MAX_RATE_FACTORS, len(factors)))
        if order is not None:
            if not hasattr(order, "items"):
                raise ValueError("MassActionODELogLike: a RateLaw's order must be None or a mapping {species: order} (got %r)" % (order,))
            pairs = []
            for s, c in order.items():
                if isinstance(s, bool) or not isinstance(s, _INT) or s < 0:
                    raise ValueError("MassActionODELogLike: a RateLaw's order names species %r (a non-negative integer)" % (s,))
                if isinstance(c, bool) or not isinstance(c, _INT) or c < 0:
                    raise ValueError("MassActionODELogLike: a RateLaw's kinetic orders must be non-negative integers (got %r for species %d)" % (c, s))
                if c:
                    pairs.append((int(s), int(c)))
            order = tuple(sorted(pairs))
        for name, v in zip(self.__slots__, (rate, factors, order)):
            object.__setattr__(self, name, v)

    def __setattr__(self, name, value):
        raise AttributeError("a RateLaw is immutable")

    def __delattr__(self, name):
        raise AttributeError("a RateLaw is immutable")

    def _key(self):
        return (type(self.rate).__name__, self.rate, self.factors, self.order)

    def __eq__(self, other):
        return isinstance(other, RateLaw) and self._key() == other._key()

    def __hash__(self):
        return hash(self._key())

    def __reduce__(self):
        return RateLaw, (self.rate, self.factors, None if self.order is None else dict(self.order))

    def __repr__(self):
        return "RateLaw(%r, %r, %r)" % (self.rate, list(self.factors), None if self.order is None else dict(self.order))


def _rate(rate):
    """A reaction's rate constant: the third element itself, or a RateLaw's rate."""
    return rate.rate if isinstance(rate, RateLaw) else rate


def _orders(reaction):
    """A reaction's kinetic orders {species: order}: the reactants' coefficients unless a RateLaw's order replaces them."""
    law = reaction[2]
    return dict(law.order) if isinstance(law, RateLaw) and law.order is not None else reaction[0]


def _factors(reaction):
    return reaction[2].factors if isinstance(reaction[2], RateLaw) else ()


def _kinetic_species(reaction):
    """The species a reaction's rate depends on, ascending: those with a kinetic order and those of its Hill factors."""
    return sorted(set(_orders(reaction)) | {f.species for f in _factors(reaction)})


def _hill_slots(reactions):
    """The distinct (K, n) pairs of the network's Hill factors, in the order of their first use: one slot each (csrc/dz_ode.h)."""
    slots = []
    for rx in reactions:
        for f in _factors(rx):
            if not any(type(K) is type(f.K) and K == f.K and n == f.n for K, n in slots):
                slots.append((f.K, f.n))
    return slots


def _slot_of(slots, f):
    return next(m for m, (K, n) in enumerate(slots) if type(K) is type(f.K) and K == f.K and n == f.n)


def _slot_indices(slots):
    """The parameter indices the slots' K read, bare or inside a monomial, ascending."""
    return sorted({K for K, _ in slots if isinstance(K, _INT)} | {i for K, _ in slots if isinstance(K, Monomial) for i in K.indices})


def _slot_code(K, log10):
    """(the C++ expression of a slot's K, the parameter indices it reads)"""
    if isinstance(K, Monomial):
        kv, idx = _mono_value(K), K.indices
    elif isinstance(K, _INT):
        kv, idx = ("dzode::dexp(x[%d] * 2.302585092994046)" % K) if log10 else "x[%d]" % K, (K,)
    else:
        kv, idx = _hexlit(K), ()
    return kv, idx


def _hill_value(f, kn):
    """A Hill factor at y: yn the repeated product of y, den = Kn + yn, yn / den (activation) or Kn / den (repression).  kn: Kn's name."""
    yn = " * ".join(["y[%d]" % f.species] * f.n)
    return "((%s) / (%s + %s))" % (yn if f.kind == "activation" else kn, kn, yn)


def _hill_slope(f, kn):
    """Its derivative: num = ((n * Kn) * y) * y ... (n - 1 factors of y, left to right; n = 1: Kn itself), den = Kn + yn,
    +-num / (den * den): the sign is applied to the quotient."""
    yn = " * ".join(["y[%d]" % f.species] * f.n)
    num = " * ".join((["%d.0" % f.n] if f.n > 1 else []) + [kn] + ["y[%d]" % f.species] * (f.n - 1))
    return "(%s(%s) / ((%s + %s) * (%s + %s)))" % ("" if f.kind == "activation" else "-", num, kn, yn, kn, yn)


def _rate_product(kname, reaction, slotname):
    """v = k * prod y^order (ascending species) * prod h_m (in the order given), left to right."""
    return _product([kname] + _rate_factors(_orders(reaction)) + [_hill_value(f, slotname(f)) for f in _factors(reaction)])


def _rate_slope(kname, reaction, q, slotname):
    """dv / dy_q: the product rule's sum in the order of the product -- the mass-action term (q has a kinetic order), then one term per
    Hill factor on q, each the product v with that one factor replaced by its derivative.  A reaction without factors: the one product
    it always was."""
    order, hills = _orders(reaction), _factors(reaction)
    values = [_hill_value(f, slotname(f)) for f in hills]
    terms = []
    if q in order:
        c = order[q]
        terms.append(_product([kname] + (["%d.0" % c] if c > 1 else []) + _rate_factors(order, skip=q) + values))
    for m, f in enumerate(hills):
        if f.species == q:
            terms.append(_product([kname] + _rate_factors(order) + values[:m] + [_hill_slope(f, slotname(f))] + values[m + 1:]))
    return terms[0] if len(terms) == 1 else " + ".join("(%s)" % t for t in terms)


def _mono_value(m):
    """The C++ expression of a monomial's value: the sum in ascending index, an exponent of +-1 as a plain add or subtract."""
    out = _hexlit(m.log10_factor)
    for i, e in m.exponents:
        out += " + x[%d]" % i if e == 1.0 else " - x[%d]" % i if e == -1.0 else " + %s * x[%d]" % (_hexlit(e), i)
    return "dzode::dexp((%s) * 2.302585092994046)" % out


def _rate_indices(reactions):
    """The parameter indices the rate constants read, bare or inside a monomial, ascending: those whose x is tested for finiteness."""
    rates = [_rate(r) for _, _, r in reactions]
    return sorted({r for r in rates if isinstance(r, _INT)} | {i for r in rates if isinstance(r, Monomial) for i in r.indices})


def _slot_lines(slots, log10, first):
    """The one-lane rates()' statements for the Hill slots, k[first + m] = Kn, and their liveness tests (csrc/dz_ode.h, RATE LAWS)."""
    L, tests = [], ["dzode::finite(x[%d])" % i for i in _slot_indices(slots)]
    for m, (K, n) in enumerate(slots):
        L.append("        const double K%d = %s;" % (m, _slot_code(K, log10)[0]))
        L.append("        k[%d] = %s;" % (first + m, " * ".join(["K%d" % m] * n)))
        tests += ["dzode::finite(K%d)" % m, "dzode::finite(k[%d])" % (first + m), "k[%d] > 0.0" % (first + m)]
    return L, tests


def _monomial_members(mono):
    """The members of a generated network that has monomials (csrc/dz_ode.h's head), for the one-lane and the lane-group source alike.
    mono: dict(y0={species: Monomial}, scale=[float | Monomial] or None, constraints=[(Monomial, loc, sd)])."""
    y0, scale, cons = mono["y0"], mono["scale"] or [], mono["constraints"]
    outside = [m for _, m in sorted(y0.items())] + [f for f in scale if isinstance(f, Monomial)] + [m for m, _, _ in cons]
    tests = ["dzode::finite(x[%d])" % i for i in sorted({i for m in outside for i in m.indices})] + ["dzode::finite(%s)" % _mono_value(m) for m in outside]
    L = ["    static constexpr bool MONOMIALS = true;", "    DZO_HD static bool live(const double* x)", "    {",
         "        return %s;" % (" && ".join(tests) or "true"), "    }",
         "    DZO_HD static double y0_row(int r, const double* x, double b)", "    {"]
    if y0:
        L += ["        const double m%d = %s;" % (s, _mono_value(m)) for s, m in sorted(y0.items())]
        sel = "0.0"
        for s in sorted(y0, reverse=True):
            sel = "r == %d ? m%d : %s" % (s, s, sel)
        L += ["        const double m = %s;" % sel, "        return b != b ? m : b;"]
    else:
        L.append("        return b;")
    L += ["    }", "    DZO_HD static void scale(const double* x, double* o)", "    {"]
    L += ["        o[%d] = %s * o[%d];" % (q, _mono_value(f) if isinstance(f, Monomial) else _hexlit(f), q) for q, f in enumerate(scale) if f != 1.0]
    L.append("    }")
    if cons:
        G0 = float(sum(-np.log(sd) - _LOG_2PI_HALF for _, _, sd in cons))
        L += ["    DZO_HD static double constraints(const double* x)", "    {", "        double acc = 0.0;"]
        L += ["        { const double r = (%s - %s) / %s; acc = acc - 0.5 * r * r; }" % (_mono_value(m), _hexlit(loc), _hexlit(sd)) for m, loc, sd in cons]
        L += ["        return %s + acc;" % _hexlit(G0), "    }"]
    return L


def _stoichiometry(S, reactions):
    N = np.zeros((S, len(reactions)), dtype=np.int64)
    for r, (reac, prod, _) in enumerate(reactions):
        for s, c in reac.items():
            N[s, r] -= c
        for s, c in prod.items():
            N[s, r] += c
    return N


def _product(factors):
    return " * ".join(factors) if factors else "1.0"


def _rate_factors(reac, skip=None):
    out = []
    for s, c in sorted(reac.items()):
        out += ["y[%d]" % s] * (c - (1 if s == skip else 0))
    return out


def _combine(terms):                        # [(integer coefficient, expression)] -> a sum in this order
    out = ""
    for c, e in terms:
        t = e if abs(c) == 1 else "%d.0 * %s" % (abs(c), e)
        out += ("-" if c < 0 else "") + t if not out else (" - " if c < 0 else " + ") + t
    return out or "0.0"


def _obs_lines(S, observables):
    L = []
    for o, row in enumerate(observables):
        terms = ["y[%d]" % s if row[s] == 1.0 else "%s * y[%d]" % (_hexlit(row[s]), s) for s in range(S) if row[s] != 0.0]
        L.append("        o[%d] = %s;" % (o, " + ".join(terms) if terms else "0.0"))
    return L


def _net_source(header, S, R, O, body, observables, entries, events=0, equilibrate=False):
    """The scaffolding every generated source shares: the include, the struct's head, the generator's own members (body, up to the
    closing brace of the last one), the observables and the entry macro.  events: the largest event count over the object's
    experiments; the member EVENTS only if there is one (csrc/dz_ode.h).  equilibrate: some experiment equilibrates first; the member
    EQUILIBRATE only then."""
    L = ["struct Net {", "    static constexpr int S = %d, R = %d, O = %d;" % (S, R, O)]
    L += ["    static constexpr int EVENTS = %d;" % events] if events else []
    L += ["    static constexpr bool EQUILIBRATE = true;"] if equilibrate else []
    L += body
    L += ["    DZO_HD static void obs(const double* y, double* o)", "    {"] + _obs_lines(S, observables) + ["    }", "};", entries, ""]
    return '#include "%s"\n' % header + "\n".join(L)


_ODE_WHOLE_SUMS = 16        # up to this many reactions the one-lane source names every rate and writes each f[s] and J[i] as one sum


def _ode_long_source(S, reactions, observables, log10, entries="DZODE_ENTRIES(Net)", mono=None, events=0, equilibrate=False):
    """The one-lane source for more than _ODE_WHOLE_SUMS reactions.  Every f[s] and J[i] is the same sum in the same (ascending reaction)
    order as in the short form, but built up reaction by reaction, so one rate is live at a time and not all R; DZODE_FENCE between the
    reactions keeps the compiler from starting them all at once (see csrc/dz_ode.h).  k holds one rate constant per parameter that is
    used, not one per reaction, and a fixed rate constant is a literal where it is used: what stays in registers through the
    integration is the number of distinct parameters."""
    R, O = len(reactions), len(observables)
    N = _stoichiometry(S, reactions)
    rates = [_rate(rate) for _, _, rate in reactions]
    used = sorted({rate for rate in rates if isinstance(rate, _INT)})
    for rate in rates:                          # (then a slot per distinct monomial, in the order of their first reactions)
        if isinstance(rate, Monomial) and rate not in used:
            used.append(rate)
    kname = ["k[%d]" % used.index(rate) if isinstance(rate, _INT + (Monomial,)) else _hexlit(rate) for rate in rates]
    slots = _hill_slots(reactions)              # (then the Hill slots: k[len(used) + m] = Kn)
    slotname = lambda f: "k[%d]" % (len(used) + _slot_of(slots, f))      # noqa: E731
    slot_lines, slot_tests = _slot_lines(slots, log10, len(used))

    def add(target, started, c, e):
        t = e if abs(c) == 1 else "%d.0 * %s" % (abs(c), e)
        if target in started:
            return "        %s = %s %s %s;" % (target, target, "-" if c < 0 else "+", t)
        started.add(target)
        return "        %s = %s%s;" % (target, "-" if c < 0 else "", t)

    L = ["    static constexpr int SLOTS = %d;" % len(slots)] if slots else []
    L += ["    DZO_HD static bool rates(const double* x, double* k)", "    {"]
    L += ["        k[%d] = %s;" % (i, _mono_value(p) if isinstance(p, Monomial) else ("dzode::dexp(x[%d] * 2.302585092994046)" % p) if log10 else "x[%d]" % p)
          for i, p in enumerate(used)]
    L += slot_lines
    L.append("        return %s;" % (" && ".join(["dzode::finite(x[%d])" % p for p in _rate_indices(reactions)] + ["dzode::finite(k[%d])" % i for i in range(len(used))]
                                                 + slot_tests) or "true"))
    L += ["    }", "    DZO_HD static void rhs(const double* k, const double* y, double* f)", "    {"]
    started = set()
    for r, reaction in enumerate(reactions):
        rows = [s for s in range(S) if N[s, r] != 0]
        if not rows:
            continue
        L.append("        const double v%d = %s;" % (r, _rate_product(kname[r], reaction, slotname)))
        L += [add("f[%d]" % s, started, int(N[s, r]), "v%d" % r) for s in rows]
        L.append("        " + " ".join("DZODE_FENCE(f[%d]);" % s for s in rows))
    L += ["        f[%d] = 0.0;" % s for s in range(S) if "f[%d]" % s not in started]
    L += ["    }", "    DZO_HD static void jac(const double* k, const double* y, double* J)", "    {"]
    started = set()
    for r, reaction in enumerate(reactions):            # dv_r / dy_q = k nu_q y_q^(nu_q - 1) prod_others y^nu (a RateLaw: _rate_slope)
        rows = [s for s in range(S) if N[s, r] != 0]
        for q in _kinetic_species(reaction):
            if not rows:
                continue
            L.append("        const double d%d_%d = %s;" % (r, q, _rate_slope(kname[r], reaction, q, slotname)))
            L += [add("J[%d]" % (s * S + q), started, int(N[s, r]), "d%d_%d" % (r, q)) for s in rows]
            L.append("        " + " ".join("DZODE_FENCE(J[%d]);" % (s * S + q) for s in rows))
    L += ["        J[%d] = 0.0;" % i for i in range(S * S) if "J[%d]" % i not in started]
    return _net_source("dz_ode.h", S, R, O, L + ["    }"] + (_monomial_members(mono) if mono else []), observables, entries, events, equilibrate)


def _ode_source(S, reactions, observables, log10, items=False, mono=None, events=0, equilibrate=False):
    """The generated network struct (see csrc/dz_ode.h; the scaffolding around it: _net_source): rate constants, right-hand side, analytic Jacobian and observables as
    straight-line code with constant indices; powers as repeated products.  items: the entry points for several conditions per point."""
    R, O = len(reactions), len(observables)
    entries = "DZODE_ITEM_ENTRIES(Net)" if items else "DZODE_ENTRIES(Net)"
    if R > _ODE_WHOLE_SUMS:
        return _ode_long_source(S, reactions, observables, log10, entries, mono, events, equilibrate)
    N = _stoichiometry(S, reactions)
    slots = _hill_slots(reactions)              # (the Hill slots behind the rate constants: k[R + m] = Kn)
    slotname = lambda f: "k[%d]" % (R + _slot_of(slots, f))      # noqa: E731
    slot_lines, slot_tests = _slot_lines(slots, log10, R)
    L = ["    static constexpr int SLOTS = %d;" % len(slots)] if slots else []
    L += ["    DZO_HD static bool rates(const double* x, double* k)", "    {"]
    for r, rate in enumerate(_rate(rate) for _, _, rate in reactions):
        if isinstance(rate, _INT):
            L.append("        k[%d] = %s;" % (r, ("dzode::dexp(x[%d] * 2.302585092994046)" % rate) if log10 else "x[%d]" % rate))
        elif isinstance(rate, Monomial):
            L.append("        k[%d] = %s;" % (r, _mono_value(rate)))
        else:
            L.append("        k[%d] = %s;" % (r, _hexlit(rate)))
    used = _rate_indices(reactions)             # (10**-inf is a finite 0: test x itself)
    L += slot_lines
    L.append("        return %s;" % " && ".join(["dzode::finite(x[%d])" % i for i in used] + ["dzode::finite(k[%d])" % r for r in range(R)] + slot_tests))
    L += ["    }", "    DZO_HD static void rhs(const double* k, const double* y, double* f)", "    {"]
    for r, reaction in enumerate(reactions):
        L.append("        const double v%d = %s;" % (r, _rate_product("k[%d]" % r, reaction, slotname)))
    for s in range(S):
        L.append("        f[%d] = %s;" % (s, _combine([(int(N[s, r]), "v%d" % r) for r in range(R) if N[s, r] != 0])))
    L += ["    }", "    DZO_HD static void jac(const double* k, const double* y, double* J)", "    {"]
    for r, reaction in enumerate(reactions):            # dv_r / dy_q = k nu_q y_q^(nu_q - 1) prod_others y^nu (a RateLaw: _rate_slope)
        for q in _kinetic_species(reaction):
            L.append("        const double d%d_%d = %s;" % (r, q, _rate_slope("k[%d]" % r, reaction, q, slotname)))
    kinetic = [_kinetic_species(reaction) for reaction in reactions]
    for s in range(S):
        for q in range(S):
            terms = [(int(N[s, r]), "d%d_%d" % (r, q)) for r in range(R) if N[s, r] != 0 and q in kinetic[r]]
            L.append("        J[%d] = %s;" % (s * S + q, _combine(terms)))
    return _net_source("dz_ode.h", S, R, O, L + ["    }"] + (_monomial_members(mono) if mono else []), observables, entries, events, equilibrate)


def _ode_group_source(S, reactions, observables, log10, lanes, items=False, mono=None, events=0, equilibrate=False):
    """The generated network struct for the lane-group solver and, with lanes=64, the wave-per-point one (csrc/dz_ode_group.h).  Lane r (or the host build's loop iteration r) gets
    its own f[r] and J[r][q] WITHOUT a branch on r: every reaction's rate is evaluated by every lane and multiplied by that lane's
    stoichiometric coefficient, a select over constants (0 for a species the reaction does not touch), so the lanes of a wave never
    diverge inside the right-hand side.  Every f[r] and J[r][q] is the sum over the reactions (for J: those with q among the reactants)
    in ascending reaction index of coefficient(r) * (k[j] * (nu) * y...) -- written here once, compiled for both sides."""
    R, O = len(reactions), len(observables)
    N = _stoichiometry(S, reactions)

    def coefficient(j):                     # N[r][j] as a function of r
        out = "0.0"
        for s in reversed([s for s in range(S) if N[s, j] != 0]):
            out = "r == %d ? %d.0 : %s" % (s, N[s, j], out)
        return "(%s)" % out

    def weighted_sum(terms, indent):        # [(j, expression)] -> statements that leave the sum in v
        if not terms:
            return [indent + "return 0.0;"]
        out = [indent + "int z = 0;", indent + "double v = %s * (%s);" % (coefficient(terms[0][0]), terms[0][1])]
        for t, (j, e) in enumerate(terms[1:], 1):
            if t % 4 == 0:                  # (a long sum in groups of four terms: see DZODE_SUM_FENCE in csrc/dz_ode_group.h)
                out.append(indent + "DZODE_SUM_FENCE(v, r, z);")
            out.append(indent + "v = v + %s * (%s);" % (coefficient(j), e))
        return out + [indent + "return v;"]

    rates = [_rate(rate) for _, _, rate in reactions]
    slots = _hill_slots(reactions)              # (the Hill slots behind the rate constants: k[R + m] = Kn, by lane (R + m) % L once per point)
    slotname = lambda f: "k[z + %d]" % (R + _slot_of(slots, f))      # noqa: E731
    L = ["    static constexpr bool LOG10 = %s;" % ("true" if log10 else "false"),
         "    DZO_HD static int rate_index(int j)", "    {", "        switch (j) {"]
    L += ["        case %d: return %d;" % (j, -2 if isinstance(rate, Monomial) else rate) for j, rate in enumerate(rates) if isinstance(rate, _INT + (Monomial,))]
    L += ["        default: return -1;", "        }", "    }", "    DZO_HD static double rate_fixed(int j)", "    {", "        switch (j) {"]
    L += ["        case %d: return %s;" % (j, _hexlit(rate)) for j, rate in enumerate(rates) if not isinstance(rate, _INT + (Monomial,))]
    L += ["        default: return 0.0;", "        }", "    }"]
    if slots:
        L += ["    static constexpr int SLOTS = %d;" % len(slots), "    DZO_HD static double slot(int m, const double* x, bool& good)", "    {", "        switch (m) {"]
        for m, (K, n) in enumerate(slots):
            kv, idx = _slot_code(K, log10)
            L.append("        case %d: { const double K = %s; const double v = %s; good = %s; return v; }"
                     % (m, kv, " * ".join(["K"] * n), " && ".join(["dzode::finite(x[%d])" % i for i in idx] + ["dzode::finite(K)", "dzode::finite(v)", "v > 0.0"])))
        L += ["        default: good = false; return 0.0;", "        }", "    }"]
    if mono:                                             # (rate_index -2: the reaction's own expression, by lane j % L once per point)
        L += ["    DZO_HD static double rate_mono(int j, const double* x, bool& good)", "    {", "        switch (j) {"]
        for j, rate in enumerate(rates):
            if isinstance(rate, Monomial):
                L.append("        case %d: { const double v = %s; good = %s; return v; }"
                         % (j, _mono_value(rate), " && ".join(["dzode::finite(x[%d])" % i for i in rate.indices] + ["dzode::finite(v)"])))
        L += ["        default: good = false; return 0.0;", "        }", "    }"]
    L += ["    DZO_HD static double rhs_row(int r, const double* k, const double* y)", "    {"]
    L += weighted_sum([(j, _rate_product("k[z + %d]" % j, reactions[j], slotname)) for j in range(R) if np.any(N[:, j] != 0)], "        ")
    L += ["    }", "    DZO_HD static double jac_entry(int r, int q, const double* k, const double* y)", "    {", "        switch (q) {"]
    for q in range(S):                                   # dv_j / dy_q = k nu_q y_q^(nu_q - 1) prod_others y^nu
        terms = [(j, _rate_slope("k[z + %d]" % j, reactions[j], q, slotname)) for j in range(R) if q in _kinetic_species(reactions[j]) and np.any(N[:, j] != 0)]
        L += ["        case %d: {" % q] + weighted_sum(terms, "            ") + ["        }"]
    L += ["        default: return 0.0;", "        }", "    }"] + (_monomial_members(mono) if mono else [])
    return _net_source("dz_ode_group.h", S, R, O, L, observables, ("DZODE_GROUP_ITEM_ENTRIES(Net, %d)" if items else "DZODE_GROUP_ENTRIES(Net, %d)") % lanes, events, equilibrate)


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
    (ODE_MAX_CONDITIONS) mappings with the optional keys "y0", "data", "sd", "events", "equilibrate"; a missing key is the constructor's own argument,
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
    expressions, time-dependent inputs, rate laws in event amounts."""

    conditions = None       # (an object pickled before the keyword existed)
    events = None           # (likewise)
    equilibrate = None      # (likewise)
    scale, constraints, y0_monomials = None, (), {}     # (likewise: before Monomial existed)

    def __init__(self, n_species, reactions, y0, t, observables, data, sd, rate_scale="log10", t0=0.0, rtol=1.49012e-8, atol=1.49012e-8,
                 max_steps=500, ndim=None, path=None, lanes_per_point=1, conditions=None, scale=None, constraints=None, events=None,
                 equilibrate=None):
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
        if not 1 <= len(reactions) <= lim["reactions"]:
            raise ValueError("MassActionODELogLike: 1..%d reactions are supported (got %d)" % (lim["reactions"], len(reactions)))
        if rate_scale not in ("log10", "linear"):
            raise ValueError('MassActionODELogLike: rate_scale must be "log10" or "linear"')
        rx = []
        for r, reaction in enumerate(reactions):
            if len(reaction) != 3:
                raise ValueError("MassActionODELogLike: reaction %d must be (reactants, products, rate)" % r)
            reac, prod, rate = reaction
            for side in (reac, prod):
                for s, c in dict(side).items():
                    if isinstance(s, bool) or not isinstance(s, (int, np.integer)) or not 0 <= s < S:
                        raise ValueError("MassActionODELogLike: reaction %d names species %r (0..%d)" % (r, s, S - 1))
                    if isinstance(c, bool) or not isinstance(c, (int, np.integer)) or c < 0:
                        raise ValueError("MassActionODELogLike: reaction %d: stoichiometric coefficients must be non-negative integers (got %r)" % (r, c))
            if isinstance(rate, bool) or not isinstance(rate, (int, np.integer, float, np.floating, Monomial, RateLaw)):
                raise ValueError("MassActionODELogLike: reaction %d: the rate is a parameter index (int), a fixed rate constant (float), a Monomial or a RateLaw" % r)
            if isinstance(rate, RateLaw):
                for s in [s for s, _ in rate.order or ()] + [f.species for f in rate.factors]:
                    if not 0 <= s < S:
                        raise ValueError("MassActionODELogLike: reaction %d: its RateLaw names species %r (0..%d)" % (r, s, S - 1))
                if not rate.factors and rate.order is None:          # (nothing beyond its rate: the plain reaction, source and bits)
                    rate = rate.rate
            elif isinstance(rate, Monomial):
                pass
            elif isinstance(rate, (int, np.integer)):
                if rate < 0:
                    raise ValueError("MassActionODELogLike: reaction %d: parameter index %d is negative" % (r, rate))
                rate = int(rate)
            elif not np.isfinite(rate):
                raise ValueError("MassActionODELogLike: reaction %d: the fixed rate constant must be finite" % r)
            else:
                rate = float(rate)
            rx.append(({int(s): int(c) for s, c in dict(reac).items() if c}, {int(s): int(c) for s, c in dict(prod).items() if c}, rate))
        slots = _hill_slots(rx)
        if len(rx) + len(slots) > lim["reactions"]:
            raise ValueError("MassActionODELogLike: reactions plus distinct Hill (K, n) pairs must stay within %d (got %d + %d)" % (lim["reactions"], len(rx), len(slots)))
        idx = _rate_indices(rx) + _slot_indices(slots)
        if conditions is not None:
            conditions = list(conditions)
            if not 1 <= len(conditions) <= ODE_MAX_CONDITIONS:
                raise ValueError("MassActionODELogLike: 1..%d conditions are supported (got %d)" % (ODE_MAX_CONDITIONS, len(conditions)))
            for c, cond in enumerate(conditions):
                if not hasattr(cond, "keys") or set(cond.keys()) - {"y0", "data", "sd", "events", "equilibrate"}:
                    raise ValueError('MassActionODELogLike: condition %d must be a mapping with the keys "y0", "data", "sd", "events", "equilibrate" (each optional)' % c)
                for key, top in (("y0", y0), ("data", data), ("sd", sd)):
                    if cond.get(key) is None and top is None:
                        raise ValueError("MassActionODELogLike: condition %d has no %s, and the constructor's %s is None" % (c, key, key))
        elif y0 is None or data is None or sd is None:
            raise ValueError("MassActionODELogLike: y0, data and sd may be None only when every one of the conditions gives its own")
        y0m = {}                                 # species -> the Monomial its start amount is, wherever a y0 says so (the same in all)
        if y0 is not None:
            y0 = self._checked_y0(y0, S, "", y0m)
        t = np.asarray(t, dtype=float).reshape(-1)
        if not 1 <= len(t) <= lim["times"]:
            raise ValueError("MassActionODELogLike: 1..%d output times are supported (got %d)" % (lim["times"], len(t)))
        if not np.isfinite(t0) or not np.all(np.isfinite(t)) or np.any(np.diff(t) < 0) or t[0] < t0:
            raise ValueError("MassActionODELogLike: output times must be finite, sorted and >= t0 = %r" % t0)
        obs = np.atleast_2d(np.asarray(observables, dtype=float))
        if obs.ndim != 2 or obs.shape[1] != S or not 1 <= len(obs) <= lim["observables"] or not np.all(np.isfinite(obs)):
            raise ValueError("MassActionODELogLike: observables must be an O x %d finite matrix with O = 1..%d" % (S, lim["observables"]))
        O, T = len(obs), len(t)
        if data is not None and sd is not None:
            data, sd = self._checked_data(data, sd, O, T, "")
        events = self._checked_events(events, S, float(t0), t, "")
        if not (rtol > 0 and atol > 0 and np.isfinite(rtol) and np.isfinite(atol)) or int(max_steps) < 1:
            raise ValueError("MassActionODELogLike: rtol and atol must be > 0, max_steps >= 1")
        span = max(float(t[-1]) - float(t0), 1e-300)
        equilibrate = self._checked_equilibrate(equilibrate, float(rtol), float(atol), span, "")
        if conditions is not None:              # every condition as the single experiment: its own values, else the constructor's (checked above)
            full = []
            for c, cond in enumerate(conditions):
                who = "condition %d: " % c
                cy0 = y0 if cond.get("y0") is None else self._checked_y0(cond["y0"], S, who, y0m)
                cdata, csd = (data if cond.get("data") is None else cond["data"]), (sd if cond.get("sd") is None else cond["sd"])
                if cond.get("data") is not None or cond.get("sd") is not None or data is None or sd is None:
                    cdata, csd = self._checked_data(cdata, csd, O, T, who)
                cev = events if "events" not in cond or cond["events"] is None else self._checked_events(cond["events"], S, float(t0), t, who)
                ceq = equilibrate if cond.get("equilibrate") is None else self._checked_equilibrate(cond["equilibrate"], float(rtol), float(atol), span, who)
                full.append(dict(y0=cy0, data=cdata, sd=csd, events=cev, **({"equilibrate": ceq} if ceq else {})))
            conditions = full
        if scale is not None:
            scale = list(scale) if hasattr(scale, "__len__") or hasattr(scale, "__iter__") else [scale]
            if len(scale) != O or not all(isinstance(f, Monomial) or (not isinstance(f, bool) and isinstance(f, (int, np.integer, float, np.floating)) and np.isfinite(f))
                                          for f in scale):
                raise ValueError("MassActionODELogLike: scale must hold O = %d finite numbers or Monomials" % O)
            scale = [f if isinstance(f, Monomial) else float(f) for f in scale]
        cons = []
        for m, entry in enumerate(() if constraints is None else constraints):
            if not isinstance(entry, (tuple, list)) or len(entry) != 3 or not isinstance(entry[0], Monomial):
                raise ValueError("MassActionODELogLike: constraint %d must be (Monomial, loc, sd)" % m)
            try:
                loc, csd = float(entry[1]), float(entry[2])
            except (TypeError, ValueError):
                loc = csd = np.nan
            if not (np.isfinite(loc) and np.isfinite(csd) and csd > 0):
                raise ValueError("MassActionODELogLike: constraint %d: loc must be finite and sd finite and > 0" % m)
            cons.append((entry[0], loc, csd))
        if len(cons) > ODE_MAX_CONSTRAINTS:
            raise ValueError("MassActionODELogLike: at most %d constraints are supported (got %d)" % (ODE_MAX_CONSTRAINTS, len(cons)))
        idx += [i for m in list(y0m.values()) + [f for f in scale or [] if isinstance(f, Monomial)] + [c[0] for c in cons] for i in m.indices]
        self.d = (max(idx) + 1 if idx else 0) if ndim is None else int(ndim)
        if idx and max(idx) >= self.d:
            raise ValueError("MassActionODELogLike: parameter index %d is not < ndim = %d" % (max(idx), self.d))
        self.scale, self.constraints, self.y0_monomials = scale, tuple(cons), y0m
        self.n_species, self.reactions, self.observables, self.log10 = S, rx, obs, rate_scale == "log10"
        self.rate_scale, self.y0, self.t, self.t0 = rate_scale, y0, t, float(t0)
        self.data, self.sd = data, sd
        self.events = events or None            # None, or the checked (time, species, factor, amount) tuples sorted by time
        self.equilibrate = equilibrate          # None, or dict(rtol, atol, horizon, max_step, max_steps), every default filled in
        self.conditions = conditions            # None, or a list of dict(y0, data, sd, events[, equilibrate]): checked, the fallbacks filled in
        self.rtol, self.atol, self.max_steps = float(rtol), float(atol), int(max_steps)
        self.path, self.lanes_per_point = path, lanes
        self._host = None

    @staticmethod
    def _checked_y0(y0, S, who, monomials):
        """The start amounts as S doubles, NaN where the entry is a Monomial (csrc/dz_ode.h: "take the network's monomial"); monomials:
        species -> Monomial, filled in here -- a species has the same one wherever a y0 gives it one."""
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

    @staticmethod
    def _checked_equilibrate(eq, rtol, atol, span, who):
        """None (no phase) or the phase's settings, every default filled in: dict(rtol, atol, horizon, max_step, max_steps)."""
        real = lambda v: not isinstance(v, bool) and isinstance(v, (int, np.integer, float, np.floating)) and np.isfinite(v)      # noqa: E731
        if eq is None or eq is False:
            return None
        if eq is True:
            eq = {}
        keys = ("rtol", "atol", "horizon", "max_step", "max_steps")
        if not hasattr(eq, "keys") or set(eq.keys()) - set(keys):
            raise ValueError('MassActionODELogLike: %sequilibrate must be None, False, True or a mapping with the keys "rtol", "atol", "horizon", '
                             '"max_step", "max_steps" (each optional; got %r)' % (who, eq))
        out = dict(rtol=eq.get("rtol", rtol), atol=eq.get("atol", atol), horizon=eq.get("horizon", span))
        for key in ("rtol", "atol", "horizon"):
            if not real(out[key]) or not out[key] > 0:
                raise ValueError("MassActionODELogLike: %sequilibrate: %s must be finite and > 0 (got %r)" % (who, key, out[key]))
            out[key] = float(out[key])
        out["max_step"] = eq.get("max_step", 1e6 * out["horizon"])
        if not real(out["max_step"]) or not out["max_step"] > 0:
            raise ValueError("MassActionODELogLike: %sequilibrate: max_step must be finite and > 0 (got %r)" % (who, out["max_step"]))
        out["max_step"] = float(out["max_step"])
        n = eq.get("max_steps", ODE_EQUILIBRATE_MAX_STEPS)
        if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or n < 1:
            raise ValueError("MassActionODELogLike: %sequilibrate: max_steps must be an integer >= 1 (got %r)" % (who, n))
        out["max_steps"] = int(n)
        return out

    @staticmethod
    def _checked_events(events, S, t0, t, who):
        """The events as a tuple of (time, species, factor, amount), stably sorted by time (events at one time keep the order given)."""
        real = lambda v: not isinstance(v, bool) and isinstance(v, (int, np.integer, float, np.floating)) and np.isfinite(v)      # noqa: E731
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
            if not real(time) or not t0 <= time <= t[-1]:
                raise ValueError("MassActionODELogLike: %sevent %d: the time must be finite and lie in t0 = %r <= time <= t[-1] = %r (got %r)"
                                 % (who, e, t0, float(t[-1]), time))
            if isinstance(species, bool) or not isinstance(species, (int, np.integer)) or not 0 <= species < S:
                raise ValueError("MassActionODELogLike: %sevent %d names species %r (an int in 0..%d)" % (who, e, species, S - 1))
            if isinstance(factor, Monomial) or isinstance(amount, Monomial):
                raise ValueError("MassActionODELogLike: %sevent %d: factor and amount are numbers; a Monomial (a sampled dose) is not supported" % (who, e))
            if not real(factor) or factor < 0 or not real(amount) or amount < 0:
                raise ValueError("MassActionODELogLike: %sevent %d: factor and amount must be finite and >= 0 (got %r, %r)" % (who, e, factor, amount))
            out.append((float(time), int(species), float(factor), float(amount)))
        return tuple(sorted(out, key=lambda ev: ev[0]))

    @staticmethod
    def _checked_data(data, sd, O, T, who):
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
        return data, np.array(sd)

    # ---- the data block (csrc/dz_ode.h) and the generated source
    def _event_lists(self):
        """Every experiment's events (a condition made before the keyword existed has none)."""
        if self.conditions is None:
            return [self.events or ()]
        return [cond.get("events") or () for cond in self.conditions]

    def _max_events(self):
        """Emax, the generated network's EVENTS: the largest event count over the object's experiments (0: a network without events)."""
        return max(len(ev) for ev in self._event_lists())

    def _equilibrate_list(self):
        """Every experiment's equilibration settings, None where it has none (so for an object from before the keyword existed)."""
        if self.conditions is None:
            return [self.equilibrate or None]
        return [cond.get("equilibrate") or None for cond in self.conditions]

    def _equilibrates(self):
        """Some experiment of the object equilibrates: the generated network's EQUILIBRATE and the six doubles at each block's end."""
        return any(eq is not None for eq in self._equilibrate_list())

    def _experiment_block(self, y0, data, sd, events=(), equilibrate=None):
        seen = np.isfinite(data)
        C = float(np.sum(-np.log(sd[seen]) - _LOG_2PI_HALF))
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
        return np.concatenate(blk)

    def condition_block(self, c=0):
        """One experiment's block: condition c's, or (without conditions) the constructor's own."""
        if self.conditions is None:
            return self._experiment_block(self.y0, self.data, self.sd, self.events or (), self.equilibrate)
        cond = self.conditions[c]
        return self._experiment_block(cond["y0"], cond["data"], cond["sd"], cond.get("events") or (), cond.get("equilibrate"))

    def data_block(self):
        """The block the kernels read (csrc/dz_ode.h): one experiment's, or with conditions [C, stride] and the C experiments' blocks."""
        if self.conditions is None:
            return self.condition_block()
        blocks = [self.condition_block(c) for c in range(len(self.conditions))]
        return np.concatenate([[float(len(blocks)), float(len(blocks[0]))]] + blocks)

    def _monomials(self):
        """What the generated network needs beyond rate constants of one parameter each, or None: then the source is what it always was
        (a scale factor of exactly 1.0 multiplies nothing)."""
        if (self.y0_monomials or self.constraints or any(isinstance(_rate(r[2]), Monomial) for r in self.reactions)
                or (self.scale is not None and any(f != 1.0 for f in self.scale))):
            return dict(y0=self.y0_monomials, scale=self.scale, constraints=self.constraints)
        return None

    def source(self):
        items = self.conditions is not None
        if self.lanes_per_point == 1:
            return _ode_source(self.n_species, self.reactions, self.observables, self.log10, items, self._monomials(), self._max_events(),
                               self._equilibrates())
        return _ode_group_source(self.n_species, self.reactions, self.observables, self.log10, self.lanes_per_point, items, self._monomials(),
                                 self._max_events(), self._equilibrates())

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

    def _dz_apply(self, engine):
        if self.conditions is None:
            kernel = "dz_ode_batch" if self.lanes_per_point == 1 else "dz_ode_group_batch"
            engine.set_likelihood_module(self.code_object(), kernel, self.lanes_per_point, self.data_block(), False)
        else:
            kernel = "dz_ode_item_batch" if self.lanes_per_point == 1 else "dz_ode_group_item_batch"
            engine.set_likelihood_module(self.code_object(), kernel, self.lanes_per_point, self.data_block(), False, items_per_point=len(self.conditions))

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
        lead = (len(X),) if self.conditions is None else (len(X), len(self.conditions))
        sim, like = np.full(lead + (len(self.t), len(self.observables)), np.nan), np.zeros(lead)
        self._host_call("dzode_simulate", X, len(X), X.shape[1], self.data_block(), sim, like)
        sim[like == -np.inf] = np.nan
        return sim

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
        lead = (len(X),) if self.conditions is None else (len(X), len(self.conditions))
        y, st = np.full(lead + (self.n_species,), np.nan), np.zeros(lead, dtype=np.int32)
        self._host_call("dzode_equilibrate", X, len(X), X.shape[1], self.data_block(), y, st)
        return (y, st) if return_steps else y

    def constraint_terms(self, X):
        """g(x) = sum over the constraints of norm(loc, sd).logpdf(monomial) for the rows of X, from the host build: what the single
        experiment's value, or condition 0's term, holds beyond the data's likelihood (0 without constraints; -inf where a coordinate
        that a monomial or a rate reads, or a monomial's value, is not finite)."""
        X = self._rows(X)
        g = np.zeros(len(X))
        self._host_call("dzode_constraints", X, len(X), X.shape[1], g)
        return g

    def fixed_steps(self, x, t1, nsteps, embedded=False, condition=0):
        """The state at t1 after nsteps equal steps from (t0, y0): the order-4 solution, or the embedded order-3 one (order test).
        condition: whose y0, for an object made with conditions."""
        x = np.ascontiguousarray(np.asarray(x, dtype=float).reshape(-1))
        y = np.zeros(self.n_species)
        ok = self._host_call("dzode_fixed", x, self.condition_block(condition), float(t1), int(nsteps), int(bool(embedded)), y)
        return y if ok else np.full(self.n_species, np.nan)

    def __getstate__(self):                      # (the host library is a handle of this process: loaded again on first use)
        st = dict(self.__dict__); st["_host"] = None
        return st
