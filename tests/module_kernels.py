"""A small family of user likelihood kernels (dz_set_likelihood_module, dz_set_likelihood_items, DeviceKernelLogLike, DeviceFunctionLogLike),
each with a numpy twin written operation for operation and batched over points -- the HIP engine runs the kernel, the oracle gets the twin
through set_likelihood_host, and the two runs must agree bit for bit (tests/fuzz_parity.py's module arm, tests/test_module_modes_gpu.py).

The density of every shape is  -1/2 sum_j ( w_j t_j^2 + 0.001 t_j^4 ),  t_j = x_j - c_j,  written with + - * and comparisons only (no
division, no library call: nothing the compiler and numpy could round differently; contraction is off in compile_device_kernel).  What the
shapes differ in is WHO adds WHAT in WHICH order:

  thread    one thread per point, a sequential sum over ascending j
  wave      lanes_per_point = 64: lane l adds j = l, l + 64, ...; then the xor butterfly 32, 16, .., 1
  group16   lanes_per_point = 16: lane l of the group adds j = l, l + 16, ...; the butterfly 8, .., 1 inside the group only
  group32   lanes_per_point = 32: likewise, 16, .., 1
  items     items_per_point = C: one thread per item, item c of a point adds j = c, c + C, ...; the engine adds a point's items left to right
  function  a DeviceFunctionLogLike (a wave per point, dz_wave_sum): eligible for the persistent kernel k_generations_user

One source per shape: the data block carries c[d], w[d], the cut and C, so the same code object serves every d.  Every shape but `function`
has a NON-FINITE variant -- the same kernel with a finite cut in its data block and always_finite=False: a point with x[0] > cut is -inf (for
`items`: item 1 alone is, so the -inf comes out of the engine's sum).
Every shape, `function` included, has a POISON variant as well: three band edges e1 <= e2 <= e3 in the data block, and a point whose
frac(x[0]) = x[0] - floor(x[0]) lies in [0, e1) is NaN, in [e1, e2) +inf, in [e2, e3) -inf (for `items`: item 1 alone) -- what a user's density
may return, and what the sampler's select / accept rule must decide on exactly as the oracle does (tests/test_nonfinite_gpu.py)."""
import numpy as np

POISON_BANDS = (0.06, 0.12, 0.30)      # band widths 0.06, 0.06, 0.18
SHAPES = ("thread", "wave", "group16", "group32", "items", "function")
LANES = dict(thread=1, wave=64, group16=16, group32=32, items=1, function=64)
ITEM_COUNTS = (2, 3, 5)

# the poison bands of the data block (behind the cut and C) applied to the value v of the point at x
_POISON = ("(x[0] - floor(x[0]) < c[2 * d + 2] ? __builtin_nan(\"\") : x[0] - floor(x[0]) < c[2 * d + 3] ? __builtin_huge_val() : "
           "x[0] - floor(x[0]) < c[2 * d + 4] ? -__builtin_huge_val() : v)")
_TERM = "const double t = x[j] - c[j]; acc = (acc + w[j] * (t * t)) + 0.001 * ((t * t) * (t * t));"

THREAD_SRC = r"""
extern "C" __global__ void mk_thread(const double* X, long long n, int d, int ld, double* like, const void* data)
{
    const long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double* x = X + i * ld;
    const double* c = (const double*)data; const double* w = c + d; const double cut = c[2 * d];
    double acc = 0.0;
    for (int j = 0; j < d; ++j) { %s }
    const double v = x[0] > cut ? -__builtin_huge_val() : -0.5 * acc;
    like[i] = %s;
}
""" % (_TERM, _POISON)

# a group of L lanes per point (L = 64: a wave): point i on lanes [i L, (i + 1) L) of the grid; the groups of the last block beyond n are
# predicated, not returned, in front of the cross-lane butterfly
GROUP_SRC = r"""
extern "C" __global__ void mk_group%(L)d(const double* X, long long n, int d, int ld, double* like, const void* data)
{
    const long long i = (blockIdx.x * 256ll + threadIdx.x) / %(L)d;
    const int g = threadIdx.x & (%(L)d - 1);
    const bool live = i < n;
    const double* x = X + (live ? i : 0) * ld;
    const double* c = (const double*)data; const double* w = c + d; const double cut = c[2 * d];
    double acc = 0.0;
    if (live) for (int j = g; j < d; j += %(L)d) { %(term)s }
    for (int o = %(L)d / 2; o > 0; o >>= 1) acc = acc + __shfl_xor(acc, o, %(L)d);
    if (live && g == 0) { const double v = x[0] > cut ? -__builtin_huge_val() : -0.5 * acc; like[i] = %(poison)s; }
}
"""

ITEMS_SRC = r"""
extern "C" __global__ void mk_items(const double* X, long long n, int d, int ld, double* like, const void* data)
{
    const long long u = blockIdx.x * (long long)blockDim.x + threadIdx.x;      // the item: term u %% C of point u / C
    if (u >= n) return;
    const double* c = (const double*)data; const double* w = c + d; const double cut = c[2 * d];
    const int C = (int)c[2 * d + 1];
    const double* x = X + (u / C) * ld;
    const int term = (int)(u %% C);
    double acc = 0.0;
    for (int j = term; j < d; j += C) { %s }
    const double v = (term == 1 && x[0] > cut) ? -__builtin_huge_val() : -0.5 * acc;
    like[u] = term == 1 ? %s : v;
}
""" % (_TERM, _POISON)

FUNCTION_SRC = r"""
__device__ double mk_function(const double* x, int d, const void* data, int lane)
{
    const double* c = (const double*)data; const double* w = c + d;
    double acc = 0.0;
    for (int j = lane; j < d; j += 64) { %s }
    const double v = -0.5 * dz_wave_sum(acc);
    return %s;
}
""" % (_TERM, _POISON)


def centre_and_weights(d):
    """the density's c and w at dimension d (the fuzzer's archives are uniform on [-5, 15]: the centre lies inside)"""
    return np.linspace(0.0, 8.0, d), 0.05 + (np.arange(d) % 7) / 70.0


def data_block(d, cut=np.inf, items=1, poison=None):
    c, w = centre_and_weights(d)
    return np.concatenate([c, w, [float(cut), float(items)], np.asarray(poison or (0.0, 0.0, 0.0), dtype=float)])


# ------------------------------------------------------------------------------------------------------------ the numpy twins
def _term(acc, X, c, w, j):
    t = X[:, j] - c[j]
    return (acc + w[j] * (t * t)) + 0.001 * ((t * t) * (t * t))


def _cut(X, cut, v):
    return np.where(X[:, 0] > cut, -np.inf, v)


def _poison(X, poison, v):
    """the three bands of frac(x[0]) in front of the value"""
    if poison is None:
        return v
    f = X[:, 0] - np.floor(X[:, 0])
    return np.where(f < poison[0], np.nan, np.where(f < poison[1], np.inf, np.where(f < poison[2], -np.inf, v)))


def butterfly(part):
    """the xor butterfly over the L columns of part, offsets L/2, .., 1: every column ends with the total"""
    L = part.shape[1]
    o = L // 2
    while o > 0:
        part = part + part[:, np.arange(L) ^ o]
        o >>= 1
    return part


def sum_items(items):
    """k_sum_items: ((v0 + v1) + v2) + ..."""
    s = items[:, 0]
    for c in range(1, items.shape[1]):
        s = s + items[:, c]
    return s


def thread_sum(X, c, w):
    acc = np.zeros(len(X))
    for j in range(X.shape[1]):
        acc = _term(acc, X, c, w, j)
    return acc


def strided_sums(X, c, w, L):
    """[n, L]: column l = the sum over j = l, l + L, ... in ascending order (strips of L dimensions, all columns of a strip at once)"""
    d = X.shape[1]
    part = np.zeros((len(X), L))
    for j0 in range(0, d, L):
        m = min(L, d - j0)
        t = X[:, j0:j0 + m] - c[j0:j0 + m]
        part[:, :m] = (part[:, :m] + w[j0:j0 + m] * (t * t)) + 0.001 * ((t * t) * (t * t))
    return part


def twin(shape, d, cut=np.inf, items=1, poison=None):
    """-> f(X[n, d]) -> (prior[n] = 0, like[n]): what set_likelihood_host takes (the poison bands' NaN unmapped: the engine maps it)"""
    c, w = centre_and_weights(d)

    def f(X):
        X = np.asarray(X, dtype=float).reshape(-1, d)
        if shape == "thread":
            v = _poison(X, poison, _cut(X, cut, -0.5 * thread_sum(X, c, w)))
        elif shape == "items":
            it = -0.5 * strided_sums(X, c, w, items)
            if items > 1:
                it[:, 1] = _poison(X, poison, _cut(X, cut, it[:, 1]))
            v = sum_items(it)
        else:
            v = -0.5 * butterfly(strided_sums(X, c, w, LANES[shape]))[:, 0]
            if shape != "function":
                v = _cut(X, cut, v)
            v = _poison(X, poison, v)
        return np.zeros(len(X)), v
    return f


# ------------------------------------------------------------------------------------------------------------ the device side
_OBJECTS = {}


def code_object(shape):
    """the shape's gfx950 code object (hipcc on first use, then the kernel cache) -> (path, kernel name)"""
    from pydream_amd.likelihoods import DeviceFunctionLogLike, compile_device_kernel
    if shape not in _OBJECTS:
        if shape == "function":
            _OBJECTS[shape] = (DeviceFunctionLogLike(FUNCTION_SRC, "mk_function", 1).code_object(), "dz_user_batch")
        elif shape == "thread":
            _OBJECTS[shape] = (compile_device_kernel(THREAD_SRC), "mk_thread")
        elif shape == "items":
            _OBJECTS[shape] = (compile_device_kernel(ITEMS_SRC), "mk_items")
        else:
            L = LANES[shape]
            _OBJECTS[shape] = (compile_device_kernel(GROUP_SRC % dict(L=L, term=_TERM, poison=_POISON)), "mk_group%d" % L)
    return _OBJECTS[shape]


def likelihood(shape, d, cut=np.inf, items=1, finite=None, poison=None):
    """the shape as the object a user would hand to run_dream (its _dz_apply(engine) sets it on a HIP engine); finite: always_finite, by
    default whether the cut is infinite and there are no poison bands"""
    from pydream_amd.likelihoods import DeviceFunctionLogLike, DeviceKernelLogLike
    path, name = code_object(shape)
    finite = bool(np.isinf(cut) and poison is None) if finite is None else bool(finite)
    if shape == "function":
        return DeviceFunctionLogLike(FUNCTION_SRC, "mk_function", d, data=data_block(d, poison=poison), always_finite=poison is None, path=path)
    return DeviceKernelLogLike(name, d, path=path, data=data_block(d, cut, items, poison), lanes_per_point=LANES[shape], always_finite=finite,
                               items_per_point=items if shape == "items" else 1)


def apply(engine, shape, d, cut=np.inf, items=1, oracle=False, poison=None):
    """the kernel on a HIP engine, the twin on an oracle engine"""
    if oracle:
        engine.set_likelihood_host(twin(shape, d, cut, items, poison))
    else:
        likelihood(shape, d, cut, items, poison=poison)._dz_apply(engine)
