"""The three built-in densities as plain formulas in extended precision, the error bounds a binary64 evaluation of them must keep, and
the seeded inputs tests/test_density_reference_cpu.py (the oracle) and tests/test_density_reference_gpu.py (every device copy) are held to.

Nothing here knows the oracle, the engine or scipy: numpy only.  np.longdouble must be the x87 80-bit format (64-bit significand) or
wider; the import fails otherwise.

THE FORMULAS (all arithmetic in np.longdouble, unit roundoff 2^-64; the inputs are binary64 numbers, taken exactly)

    MVN, y = x - mu     dense        logF - 1/2 y.(P y)
                        triangular   logF - 1/2 |U y|^2, U upper triangular (only U[i, j >= i] is read), as
                                     set_likelihood_mvn(mu, U, 1, logF) takes it
    mixture             log sum_j exp(F_j - 1/2 |x - mu_j|^2), the largest exponent taken out
    prior, per dimension and summed     kind 0: 0
                                        kind 1: -((x - a) / b)^2 / 2 - 1/2 log 2 pi - log b
                                        kind 2: -log b on [a, a + b], -inf outside
                        (1/2 log 2 pi from a 40-digit decimal string)

THE BOUNDS, u = 2^-53.  They follow from the standard model fl(a op b) = (a op b)(1 + e), |e| <= u (a fused multiply-add makes one
rounding of two) and from the bound for a sum of n products evaluated in ANY order, gamma_n sum |a_i b_i| with gamma_n = n u / (1 - n u)
(Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., section 3.1); n u < 3e-13 here, so gamma_n = n u to twelve digits and the
counts below are counts of roundings.  None of the bounds is measured.  dz::dexp / dz::dlog (and the oracle's orc_exp / orc_log, the same
code) are within 1.5 and 2 ulp (tests/test_contract_primitives.py).

    MVN     |device - ref| <= 2 (d + 8) u A + 2 u |ref|
            dense, A = |y|.(|P| |y|): y_j = fl(x_j - mu_j) carries one rounding; row r's product p_r = sum_c P_rc y_c at most d more (d
            products, d - 1 additions, one rounding per fused pair); Q = sum_r y_r p_r is a second sum of products, at most d roundings a
            term.  Every |y_r| |P_rc| |y_c| therefore carries at most 2 (the two y) + d + d = 2 d + 2 roundings: (2 d + 2) u A < 2 (d + 8) u A.
            triangular, A = sum_i a_i^2 with a_i = sum_j |U_ij| |y_j|: z_i = sum_j U_ij y_j is off by at most (d + 1) u a_i (the rounding of y
            and a row of at most d terms), z_i^2 by twice that relative to a_i^2, and the sum of the squares adds one rounding per square and
            one per addition a square passes through.  Kernels and oracle add the squares of a row tile of 16 in a four-way split and a
            butterfly and the tiles in ascending order: at most d / 16 + 5 additions for a square, so 2 (d + 1) + 1 +
            d / 16 + 5 roundings, which is within 2 d + 16 up to d = 144.  Beyond that the strict worst case of the model -- every rounding of
            the first row's sum in the same direction -- is up to 3 % above the constant (d = 1024: 2120 against 2064 roundings); the constant
            is kept as it is: a value outside it would be a finding to read, and the measured ratios (the GPU file's docstring) stay
            below 0.4 of it.  Last: logF - Q / 2 is one subtraction (the halving is exact), u |ref|; the second u |ref| is slack.
    mixture |device - ref| <= max_j [(d + 6) u S_j + 2 u |lh_j|] + (J + 8) u + 4 u |ref|,  S_j = |x - mu_j|^2, lh_j = F_j - S_j / 2
            S_j: one rounding per difference (it counts twice in the square), one per square, at most d - 1 in the sum: (d + 2) u S_j,
            halved with S_j (exactly) -- the bound keeps the whole and the + 6.  lh_j = F_j - S_j / 2: u |lh_j|; the subtraction of the
            maximum m: exact for the maximum itself, at most u |lh_j - m| <= u (|lh_j| + |m|) otherwise; 2 u |lh_j| per component with the
            4 u |ref| below (|m| <= |ref| + log J) covers both.  log-sum-exp moves by at most e when every lh_j moves by at most e: the
            first term.  sum_j exp(lh_j - m) lies in [1, J]: each exponential is within 1.5 ulp of a value <= 1, the J - 1 additions add
            at most (J - 1) u relative, the logarithm (derivative 1 / sum <= 1) passes relative errors of the sum on as absolute ones and adds
            its own 2 ulp of a value <= log J <= 3.5: (1.5 + J - 1 + 7) u < (J + 8) u.  The final addition of m: u |ref|.
    prior   |device - ref| <= (d + 12) u sum_j (z_j^2 + 1/2 log 2 pi + |log b_j|) + 2 u |ref|, the sum over the non-flat dimensions
            z_j = (x_j - a_j) (1 / b_j): a rounding each for the difference, the reciprocal and the product, so z_j^2 carries 7 with its
            own; the constant is rounded once; log b_j is within 2 ulp; two subtractions inside the term; the sum of the d terms in any
            order at most d - 1 roundings each: 7 + 2 + 2 + d - 1 < d + 12.  A uniform dimension contributes |log b_j| (2 ulp) only.  All-flat
            priors: the bound is 0, the value is exactly 0.  Where the reference is -inf (a uniform dimension outside its support, nothing
            else in these inputs) the other side must be exactly -inf.

THE INPUTS are described at the functions that make them.  They avoid tests/helpers.mvn_precision, the mean linspace(-1, 1, d), logF = 0,
the scale 30 alone and uniform(-6, 22): what every earlier test uses."""
import numpy as np

LD = np.longdouble
assert np.finfo(LD).nmant >= 63, "np.longdouble has a %d-bit significand here: the density reference needs the 80-bit extended format or wider" % (np.finfo(LD).nmant + 1)

U = LD(2) ** -53
HALF_LOG_2PI = LD("0.9189385332046727417803297364056176398614")      # 1/2 log(2 pi), 40 digits
RESOLVE = 100.0      # a mutation of the formula must move it by this many bounds (a condition on the inputs, not a measurement)


def _ld(a):
    return np.asarray(a, dtype=np.float64).astype(LD)


def _mm(Y, M):
    """Y[n, d] times M[d, d]^T in longdouble: out[i, r] = sum_c M[r, c] Y[i, c]  (einsum: numpy's matmul has no fast path for longdouble)"""
    return np.einsum("ic,rc->ir", Y, M)


# ----------------------------------------------------------------------------------------------------------------- the three formulas
def mvn(X, mu, M, logF, tri):
    """-> (value[n], bound[n]) in longdouble.  M: P (tri false) or U (tri true: only its upper triangle is read)."""
    X = np.atleast_2d(np.asarray(X, dtype=np.float64))
    d = X.shape[1]
    M64 = np.asarray(M, dtype=np.float64)
    if tri:
        M64 = np.triu(M64)
    Y = _ld(X) - _ld(mu)[None, :]
    aY = np.abs(Y).astype(np.float64)
    diagonal = not (M64 - np.diag(np.diag(M64))).any()
    if diagonal:                              # (the product of a diagonal matrix: no need for d^2 work per point)
        Z = Y * _ld(np.diag(M64))[None, :]
        aZ = aY * np.abs(np.diag(M64))[None, :]
    else:
        Z = _mm(Y, _ld(M64))
        aZ = aY @ np.abs(M64).T                # the magnitude: binary64 is enough for a factor of the bound
    if tri:
        Q = np.sum(Z * Z, axis=1)
        A = np.sum(aZ * aZ, axis=1)
    else:
        Q = np.sum(Y * Z, axis=1)
        A = np.sum(aY * aZ, axis=1)
    ref = LD(logF) - Q / 2
    bound = 2 * (d + 8) * U * _ld(A) + 2 * U * np.abs(ref)
    return ref, bound


def mixture(X, mus, F):
    """-> (value[n], bound[n], lh[n, J], S[n, J])"""
    X = np.atleast_2d(np.asarray(X, dtype=np.float64))
    mus = np.atleast_2d(np.asarray(mus, dtype=np.float64))
    J, d = mus.shape
    T = _ld(X)[:, None, :] - _ld(mus)[None, :, :]
    S = np.sum(T * T, axis=2)
    lh = _ld(F)[None, :] - S / 2
    m = lh.max(axis=1)
    ref = np.log(np.sum(np.exp(lh - m[:, None]), axis=1)) + m
    bound = np.max((d + 6) * U * S + 2 * U * np.abs(lh), axis=1) + (J + 8) * U + 4 * U * np.abs(ref)
    return ref, bound, lh, S


def prior(X, kind, a, b, swap_scale=False):
    """-> (value[n], bound[n]).  swap_scale: the mutation `b where 1 / b belongs, and log b dropped' of the normal term."""
    X = np.atleast_2d(np.asarray(X, dtype=np.float64))
    kind = np.asarray(kind)
    d = X.shape[1]
    x, a_, b_ = _ld(X), _ld(a)[None, :], _ld(b)[None, :]
    logb = np.log(b_)
    z = (x - a_) * b_ if swap_scale else (x - a_) / b_
    nrm = -(z * z) / 2 - HALF_LOG_2PI - (0 if swap_scale else logb)
    inside = (x >= a_) & (x <= a_ + b_)                      # (a + b is exact for these inputs, in longdouble for any)
    uni = np.where(inside, -logb, LD(-np.inf))
    k = kind[None, :]
    terms = np.where(k == 1, nrm, np.where(k == 2, uni, LD(0)))
    mag = np.where(k == 1, z * z + HALF_LOG_2PI + np.abs(logb), np.where(k == 2, np.abs(logb), LD(0)))
    ref = np.sum(terms, axis=1)
    fin = np.isfinite(ref)
    bound = (d + 12) * U * np.sum(mag, axis=1) + 2 * U * np.where(fin, np.abs(ref), LD(0))
    return ref, bound


def ratios(got, ref, bound):
    """|got - ref| / bound per point (0 / 0 = 0); where ref is -inf, got must be -inf exactly (ratio 0, else inf)"""
    got = _ld(got)
    out = np.zeros(len(ref))
    inf = np.isneginf(ref)
    out[inf] = np.where(np.isneginf(got[inf]), 0.0, np.inf)
    err = np.abs(got[~inf] - ref[~inf])
    b = bound[~inf]
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, LD(0), err / b)
    out[~inf] = np.where(np.isfinite(r), r, np.inf).astype(np.float64)
    return out


def check(got, ref, bound, what):
    """every point within its bound; -> the worst error-to-bound ratio"""
    r = ratios(got, ref, bound)
    worst = float(r.max()) if len(r) else 0.0
    bad = np.nonzero(~(r <= 1.0))[0]
    assert len(bad) == 0, "%s: %d of %d points outside the bound, first: point %d got %r reference %r bound %r (ratio %g)" % (
        what, len(bad), len(r), bad[0], float(np.asarray(got)[bad[0]]), ref[bad[0]], bound[bad[0]], r[bad[0]])
    return worst


# ----------------------------------------------------------------------------------------------------------------- the inputs
FAMILIES = ("a", "b", "c", "d")
NDISTINCT = 600      # larger point sets repeat the first 600 in a permuted order: one reference value per distinct point
SPECIAL = (5, 6)     # indices of the two special points of a point set: the mean itself (Q = 0) and +-0.0 coordinates
SCALES = (0.1, 1.0, 30.0, 1.0e4)


def _seed(*key):
    return np.random.default_rng([20261019] + [int(k) for k in key])


def matrices(family, d):
    """-> (P, Uf): the dense matrix and the upper factor of the family (each form is held to its own matrix)
    a: S = B B^T / d + diag(U(0.05, 2)), P = sym(inv S), Uf = chol(P)^T     b: diagonal, 10^-6 .. 10^6 in a shuffled order (both forms)
    c: Uf[i, j >= i] = 1 + i / 1024 + j / 2^20 and P the same pattern symmetrised: every element distinct and exact     d: the identity"""
    rng = _seed(1, ord(family), d)
    if family == "a":
        B = rng.normal(size=(d, d))
        S = B @ B.T / d + np.diag(rng.uniform(0.05, 2.0, d))
        P = np.linalg.inv(S)
        P = (P + P.T) / 2
        return P, np.linalg.cholesky(P).T.copy()
    if family == "b":
        v = 10.0 ** np.linspace(-6.0, 6.0, d) if d > 1 else np.array([1.0e6])
        rng.shuffle(v)
        return np.diag(v), np.diag(v)
    if family == "c":
        i = np.arange(d, dtype=np.float64)
        Uf = np.triu(1.0 + i[:, None] / 1024.0 + i[None, :] / 2.0 ** 20)
        P = Uf + np.triu(Uf, 1).T
        return P, Uf
    if family == "d":
        return np.eye(d), np.eye(d)
    raise ValueError(family)


def mean(d, zero):
    """the zero mean (the kernels' short path) or 3 normal(d) -- with the last element at least 3 in size, so that losing it shows at every scale"""
    if zero:
        return np.zeros(d)
    mu = 3.0 * _seed(2, d).normal(size=d)
    mu[-1] = np.copysign(max(abs(mu[-1]), 3.0), mu[-1])
    return mu


def log_f(d):
    return -1.2345 * d


def mvn_points(d, mu, n=NDISTINCT, key=0):
    """n distinct points around mu: point i at scale SCALES[i % 4]; SPECIAL[0] is the mean itself, SPECIAL[1] has +-0.0 coordinates in
    turn.  (Point 0 is an ordinary one: n = 1 is no special case.)"""
    rng = _seed(3, d, key)
    X = mu[None, :] + np.array(SCALES)[np.arange(n) % 4, None] * rng.normal(size=(n, d))
    if n > SPECIAL[0]:
        X[SPECIAL[0]] = mu
    if n > SPECIAL[1]:
        X[SPECIAL[1], :] = 0.0
        X[SPECIAL[1], 1::2] = -0.0
    return X


def generic(n):
    """mask of the points a mutation of the formula can be expected to move (not the mean itself, not the zeros)"""
    m = np.ones(n, bool)
    m[[i for i in SPECIAL if i < n]] = False
    return m


def spread(n, distinct=NDISTINCT, key=0):
    """index array of length n into `distinct` points: the identity up to `distinct`, beyond it the distinct points repeated in permuted
    orders, so that every copy sits in another tile or block"""
    if n <= distinct:
        return np.arange(n)
    rng = _seed(4, n, key)
    idx = [np.arange(distinct)]
    while sum(len(i) for i in idx) < n:
        idx.append(rng.permutation(distinct))
    return np.concatenate(idx)[:n]


PRIOR_PATTERNS = ("mixed", "uniform", "flat")


def priors(d, pattern):
    """-> (kind, a, b): a on a grid of eighths in [-5, 5], b = 2^k {1, 1.25, 1.5}, k = -3 .. 5, never 1: a + b is exact"""
    rng = _seed(5, d, PRIOR_PATTERNS.index(pattern))
    kind = {"mixed": rng.integers(0, 3, d), "uniform": np.full(d, 2), "flat": np.zeros(d, np.int64)}[pattern].astype(np.int32)
    if pattern == "mixed" and d >= 3:
        kind[rng.permutation(d)[:3]] = [0, 1, 2]              # (every kind is present)
    elif pattern == "mixed":
        kind[:] = [1, 2][:d] if d == 2 else [1]
    a = rng.integers(-40, 41, d) / 8.0
    k = rng.integers(-3, 6, d)
    m = rng.integers(0, 3, d)
    m[(k == 0) & (m == 0)] = 1
    b = 2.0 ** k * np.array([1.0, 1.25, 1.5])[m]
    assert not (b == 1.0).any() and ((a + b) - a == b).all()
    return kind, a, b


def prior_points(d, kind, a, b, n=64, key=0):
    """-> (X[n, d], tags[n]): 'in' inside the support (normal dimensions at 0.1 .. 10^4 scales of b, flat ones anywhere), 'lo' / 'hi' every
    uniform dimension ON its lower / upper end, 'out' one uniform dimension one ulp outside (above or below), the others inside"""
    rng = _seed(6, d, key)
    sc = np.array(SCALES)[np.arange(n) % 4, None]
    X = np.where(kind[None, :] == 2, a + b * rng.uniform(0.0, 1.0, (n, d)), a + b * sc * rng.normal(size=(n, d)))
    tags = np.array(["in"] * n, dtype=object)
    uni = np.nonzero(kind == 2)[0]
    if len(uni):
        for i in range(n):
            if i % 8 == 3:
                X[i, uni] = a[uni]; tags[i] = "lo"
            elif i % 8 == 5:
                X[i, uni] = a[uni] + b[uni]; tags[i] = "hi"
            elif i % 8 == 7:
                j = uni[rng.integers(len(uni))]
                X[i, j] = np.nextafter(a[j] + b[j], np.inf) if (i // 8) % 2 == 0 else np.nextafter(a[j], -np.inf)
                tags[i] = "out"
    return X, tags


MIX_J = (1, 2, 3, 32)
MIX_SEP = (0.5, 5.0)


def mixtures(d, J, sep):
    """-> (mus[J, d], F[J]): centre j at (j - 1/2) sep w (w a unit vector; centres 0 and 1 are exact mirror images), weights from a Dirichlet
    draw with the first two made equal (their mean), F_j = log w_j - d / 2 log 2 pi.  J = 1: one centre at sep w / 2."""
    rng = _seed(7, d, J, int(sep * 10))
    w = rng.normal(size=d)
    w /= np.linalg.norm(w)
    mus = np.array([(j - 0.5) * sep * w for j in range(J)])
    if J >= 2:
        mus[0] = -mus[1]
    wt = rng.dirichlet(np.ones(J))
    if J >= 2:
        wt[:2] = wt[:2].mean()
    F = np.log(wt) - 0.5 * d * np.log(2.0 * np.pi)
    return mus, F


def mixture_points(d, mus, n=64, key=0):
    """-> (X, tags): 'near' a centre at the four scales (the last coordinate at least one scale away), 'centre' a centre itself (S = 0), 'tie' the origin (centres 0 and 1 mirror each other),
    'far' 2000 / sep beyond centre 0 on the centres' line (every other term underflows), 'last' next to the last centre"""
    J = len(mus)
    rng = _seed(8, d, J, key)
    sc = np.array(SCALES)[np.arange(n) % 4, None]
    X = mus[np.arange(n) % J] + sc * rng.normal(size=(n, d))
    X[:, -1] = mus[np.arange(n) % J, -1] + sc[:, 0] * np.copysign(1.0 + np.abs(rng.normal(size=n)), rng.normal(size=n))      # (the last coordinate at least one scale off the centre: a dropped last dimension shows)
    tags = np.array(["near"] * n, dtype=object)
    for i in range(n):
        if i % 8 == 2:
            X[i] = mus[(i // 8) % J]; tags[i] = "centre"
        elif i % 8 == 4 and J >= 2:
            X[i] = 0.0; tags[i] = "tie"
        elif i % 8 == 6 and J >= 2:
            step = mus[1] - mus[0]
            X[i] = mus[0] - step * (2000.0 / float(step @ step)); tags[i] = "far"
        elif i % 8 == 7:
            X[i] = mus[-1] + 0.1 * rng.normal(size=d) / np.sqrt(d); tags[i] = "last"
    return X, tags


# ----------------------------------------------------------------------------------------------------------------- the shapes of the GPU file
# eval_logp's MVN kernels by the dimensions and point counts that reach them (selection rule: eval_logp, dz_engine.hip)
LDS_D_BOTH = (1, 2, 15, 16, 17, 33, 64, 97, 112)
LDS_D_TRI = (113, 127, 128)
LDS_N = (1, 15, 16, 17, 67)
LDS_BIG_N = (20483, 33001)              # at d = 17: more than four waves per block
MFMA_D = (113, 127, 128)                # dense only (the square does not fit LDS)
MFMA_N = (1, 63, 65)
MFMA2_N = 16403                         # more than 1024 point tiles: the two-point-tile instantiation
TILED_D = (129, 143, 144, 145, 257, 1023, 1024)
TILED_N = (1, 31, 33, 511)
GEMM_D = (129, 333, 1000)
GEMM_N = (512, 513, 600)
PRIOR_D = (1, 127, 128, 129, 256, 257, 384, 385, 1000, 1024)
# the sampler's copies
GEN_D = (5, 16, 17, 97, 112)
GEN_D_MORE = (64, 80, 96, 100)          # the row-tile counts 4, 5, 6 and the headline's 100 (one chain count each)
W4_D = (48, 100)
D2_D = (113, 128, 129, 160, 228, 229, 256)
D2_D_MORE = (176, 192, 200, 224)        # the row-tile counts 11 .. 14 (one chain count each)
MIX_D = (10, 100, 129, 256)
MULTI_D = (100, 333)


def mvn_shapes():
    """every (d, tri) an MVN kernel of the GPU file is run at"""
    out = set()
    for d in LDS_D_BOTH + TILED_D + GEMM_D + GEN_D + GEN_D_MORE + W4_D + MULTI_D:
        out.update({(d, False), (d, True)})
    for d in LDS_D_TRI + D2_D + D2_D_MORE:
        out.add((d, True))
    for d in MFMA_D:
        out.add((d, False))
    return sorted(out)


def prior_shapes():
    """every dimension a prior or mixture copy of the GPU file is run at"""
    return sorted(set(PRIOR_D + MIX_D + GEN_D + GEN_D_MORE + MULTI_D + (4, 160)))


def nch_of(d):
    """the prior / mixture kernels' chunk count template argument: 128-dimension chunks rounded up to 1, 2, 4, 8 (dz_create)"""
    c = (d + 127) // 128
    return 1 if c <= 1 else 2 if c <= 2 else 4 if c <= 4 else 8


def chunks_of(d):
    return (d + 127) // 128


def row_tiles_of(d):
    return (d + 15) // 16
