"""Independent references for the mass-action ODE solvers' tests, none of which touches the code under test: a grammar of random
reaction networks, scipy's Radau on a right-hand side and Jacobian built from the reaction list, and a restatement of one fixed-step
Rodas4 integration (Hairer & Wanner, "Solving ODEs II", IV.7, RODAS) in 40-digit mpmath and, to size a tolerance, in numpy float64."""
import numpy as np

KINDS = ("source", "degradation", "conversion", "dimerisation", "third_order", "a_2b", "catalyst", "autocatalysis", "exchange")


def _side(*species):
    out = {}
    for s in species:
        out[int(s)] = out.get(int(s), 0) + 1
    return out


def random_network(rng, S, R, P, kinds=KINDS):
    """(reactions, kinds): R reactions over S species, each drawn from `kinds` (all of KINDS, or a subset of its names)
        0 -> a,  a -> 0,  a -> b,  2a -> b,  3a -> b + 2c,  a + 2b -> c,  a + c -> b + c,  a + b -> 2a,  a + b -> c + d
    with distinct species where S allows it (S < 4: species are reused, so coefficients merge).  About 70 % of the rates are a parameter
    index below P (shared between reactions), the rest fixed floats in [0.2, 1.5].  Deterministic in rng's seed."""
    reactions, drawn = [], []
    for _ in range(R):
        kind = kinds[int(rng.integers(len(kinds)))]
        a, b, c, d = (int(s) for s in (rng.choice(S, 4, replace=False) if S >= 4 else rng.integers(0, S, 4)))
        reac, prod = {"source": (_side(), _side(a)), "degradation": (_side(a), _side()), "conversion": (_side(a), _side(b)),
                      "dimerisation": (_side(a, a), _side(b)), "third_order": (_side(a, a, a), _side(b, c, c)),
                      "a_2b": (_side(a, b, b), _side(c)), "catalyst": (_side(a, c), _side(b, c)),
                      "autocatalysis": (_side(a, b), _side(a, a)), "exchange": (_side(a, b), _side(c, d))}[kind]
        rate = int(rng.integers(P)) if rng.uniform() < 0.7 else float(rng.uniform(0.2, 1.5))
        reactions.append((reac, prod, rate))
        drawn.append(kind)
    return reactions, drawn


def rate_constants(reactions, x, rate_scale):
    """The rate constants as doubles: x[index] ("linear": exactly what the solver uses) or 10**x[index] ("log10"), or the fixed float."""
    x = np.asarray(x, dtype=float)
    return np.array([(x[r] if rate_scale == "linear" else 10.0 ** x[r]) if isinstance(r, (int, np.integer)) else r for _, _, r in reactions], dtype=float)


def stoichiometry(S, reactions):
    """(N [S, R] = products - reactants, nu [R, S] = the reactants' coefficients), integers"""
    N, nu = np.zeros((S, len(reactions)), dtype=np.int64), np.zeros((len(reactions), S), dtype=np.int64)
    for r, (reac, prod, _) in enumerate(reactions):
        for s, c in reac.items():
            N[s, r] -= c
            nu[r, s] += c
        for s, c in prod.items():
            N[s, r] += c
    return N, nu


def _rhs_and_jacobian(S, reactions, k, y, zero):
    """f [S] and J [S][S] at y as lists, by plain loops in whatever number type k and y hold (zero: that type's 0)"""
    N, nu = stoichiometry(S, reactions)
    f = [zero] * S
    J = [[zero] * S for _ in range(S)]
    for r in range(len(reactions)):
        reactants = [(int(s), int(nu[r, s])) for s in np.flatnonzero(nu[r])]
        net = [(int(s), int(N[s, r])) for s in np.flatnonzero(N[:, r])]
        v = k[r]
        for s, c in reactants:
            v = v * y[s] ** c
        for s, n in net:
            f[s] = f[s] + n * v
        for q, cq in reactants:
            dv = k[r] * cq * y[q] ** (cq - 1)
            for s, c in reactants:
                if s != q:
                    dv = dv * y[s] ** c
            for s, n in net:
                J[s][q] = J[s][q] + n * dv
    return f, J


def radau(S, reactions, k, y0, t, t0=0.0, rtol=1e-12, atol=1e-14):
    """The states at the output times t (sorted, >= t0, repeats allowed) by scipy's Radau IIA, [T, S]; k: the rate constants."""
    from scipy.integrate import solve_ivp
    k, y0, t = np.asarray(k, dtype=float), np.asarray(y0, dtype=float), np.asarray(t, dtype=float)
    N, nu = stoichiometry(S, reactions)

    def f(_, y):
        return N @ (k * np.prod(y[None, :] ** nu, axis=1))

    def jac(_, y):
        return np.array(_rhs_and_jacobian(S, reactions, k, y, 0.0)[1], dtype=float)
    tu, back = np.unique(t, return_inverse=True)
    if tu[-1] == t0:
        return np.tile(y0, (len(t), 1))
    sol = solve_ivp(f, (t0, tu[-1]), y0, method="Radau", t_eval=tu, rtol=rtol, atol=atol, jac=jac)
    assert sol.success, sol.message
    return sol.y.T[back]


# Hairer & Wanner's RODAS (METH = 1) for an autonomous system: W k_i = f(y + sum_j a_ij k_j) + (1/h) sum_j c_ij k_j, W = I / (h gamma) - J;
# stage 6 is evaluated at y5 + k5, which is the embedded order-3 solution; that plus k6 is the order-4 one.
GAMMA = 0.25
A = [[], [1.544], [0.9466785280815826, 0.2557011698983284], [3.314825187068521, 2.896124015972201, 0.9986419139977817],
     [1.221224509226641, 6.019134481288629, 12.53708332932087, -0.687886036105895]]
C = [[], [-5.6688], [-2.430093356833875, -0.2063599157091915], [-0.1073529058151375, -9.594562251023355, -20.47028614809616],
     [7.496443313967647, -10.24680431464352, -33.99990352819905, 11.7089089320616],
     [8.083246795921522, -7.981132988064893, -31.52159432874371, 16.31930543123136, -6.058818238834054]]


def _rodas4_fixed(S, reactions, k, y0, t0, t1, n, embedded, num, factor, solve, on_matrix=None):
    """n equal Rodas4 steps from (t0, y0) to t1 in the arithmetic of num(); factor(W) -> a handle, solve(handle, b) -> x (lists)"""
    k = [num(float(v)) for v in k]
    y = [num(float(v)) for v in y0]
    h = (num(float(t1)) - num(float(t0))) / n
    zero = num(0.0)
    for step in range(n):
        _, J = _rhs_and_jacobian(S, reactions, k, y, zero)
        W = [[(1 / (h * num(GAMMA)) if s == q else zero) - J[s][q] for q in range(S)] for s in range(S)]
        if on_matrix is not None:
            on_matrix(step, W)
        lu = factor(W)
        ks, arg = [], y
        for i in range(6):
            arg = [y[s] + sum((num(A[i][j]) * ks[j][s] for j in range(i)), zero) for s in range(S)] if i < 5 else [arg[s] + ks[4][s] for s in range(S)]
            f, _ = _rhs_and_jacobian(S, reactions, k, arg, zero)
            b = [f[s] + sum((num(C[i][j]) * ks[j][s] for j in range(i)), zero) / h for s in range(S)]
            ks.append(solve(lu, b))
        y = list(arg) if embedded else [arg[s] + ks[5][s] for s in range(S)]
    return y


def rodas4_fixed_mp(S, reactions, k, y0, t0, t1, n, embedded=False, dps=40, on_matrix=None):
    """The state at t1 after n equal Rodas4 steps, in dps-digit arithmetic (the coefficients and inputs are the doubles, taken exactly);
    a list of mpf.  on_matrix(step, W): called with every step's iteration matrix (a list of rows)."""
    import mpmath
    mp = mpmath.mp
    with mp.workdps(dps):
        def factor(W):
            return mp.LU_decomp(mp.matrix(W))

        def solve(lu, b):
            LU, p = lu
            return list(mp.U_solve(LU, mp.L_solve(LU, mp.matrix(b), p)))
        return _rodas4_fixed(S, reactions, k, y0, t0, t1, n, embedded, mp.mpf, factor, solve, on_matrix)


def rodas4_fixed_f64(S, reactions, k, y0, t0, t1, n, embedded=False):
    """The same integration in numpy float64 with np.linalg.solve: another valid order of the same operations, to size a tolerance."""
    def solve(W, b):
        return list(np.linalg.solve(W, np.array(b, dtype=np.float64)))
    return np.array(_rodas4_fixed(S, reactions, k, y0, t0, t1, n, embedded, np.float64, lambda W: np.array(W, dtype=np.float64), solve), dtype=float)


def pivot_rows(W):
    """The row that pivots in every column of W under the solvers' rule (the head of csrc/dz_ode_group.h), restated in numpy float64:
    per column the largest |w| among the rows that have not pivoted yet (equal maxima: the lowest row; a NaN counts as +inf), the other
    such rows subtract their multiple of the pivot's row, rows do not move.  A column k pivots off the diagonal where the result is
    not k.  For conditions on a test's INPUT, on the reference's own matrices (on_matrix below); never applied to the code under test."""
    W = np.array([[float(v) for v in row] for row in W], dtype=np.float64)
    S = len(W)
    free, piv = np.ones(S, dtype=bool), np.zeros(S, dtype=np.int64)
    for k in range(S):
        key = np.abs(W[:, k])
        key = np.where(free, np.where(np.isnan(key), np.inf, key), -1.0)
        p = int(np.argmax(key))                                               # (the first of equal maxima)
        piv[k], free[p] = p, False
        W[free, k + 1:] -= np.outer(W[free, k] / W[p, k], W[p, k + 1:])
    return piv


def fixed_step_reference(S, reactions, k, y0, t0, t1, n, embedded, on_matrix=None):
    """(the mp solution, max |mp|, tol) with tol = 64 max|f64 - mp| / max|mp| + 16 eps: what a correct float64 implementation with
    another operation order (a pivoted LU of up to 64 rows: one lane, a group of 16 or 32, a wave of 64) may deviate from the mp
    solution, relative to max |mp|.  on_matrix(step, W): handed to the mp integration."""
    import mpmath
    ref = rodas4_fixed_mp(S, reactions, k, y0, t0, t1, n, embedded, on_matrix=on_matrix)
    f64 = rodas4_fixed_f64(S, reactions, k, y0, t0, t1, n, embedded)
    with mpmath.mp.workdps(40):
        scale = max(abs(v) for v in ref)
        dev = max(abs(mpmath.mpf(float(a)) - b) for a, b in zip(f64, ref))
        tol = float(64 * dev / scale) + 16 * np.finfo(float).eps
    return ref, scale, tol


def deviation(y, ref, scale):
    """max |y - ref| / scale, y doubles, ref and scale mpf"""
    import mpmath
    with mpmath.mp.workdps(40):
        return float(max(abs(mpmath.mpf(float(a)) - b) for a, b in zip(y, ref)) / scale)
