"""Independent references for the rate-law tests (RateLaw, Hill): a right-hand side and an analytic Jacobian built from the reaction list
by plain loops in whatever number type they are handed (float64 or mpmath.mpf), scipy's Radau on them, and the fixed-step Rodas4
restatement of tests/ode_reference.py with the right-hand side passed in, in 40-digit mpmath and in float64.  Nothing here calls into
pydream_amd.likelihoods or the headers: a RateLaw, a Hill and a Monomial are read as records (their attributes), never evaluated by
their own code."""
import numpy as np

from .ode_reference import A, C, GAMMA, deviation      # noqa: F401  (Rodas4's coefficients and the deviation measure: data and a norm)


def constant(c, x, rate_scale):
    """A rate or Hill constant as a double: a parameter index (x[i] under "linear", 10**x[i] under "log10"), a fixed float, or a
    monomial record 10**(log10_factor + sum e_i x[i])."""
    if isinstance(c, (int, np.integer)):
        return float(x[c]) if rate_scale == "linear" else float(10.0 ** x[c])
    if isinstance(c, (float, np.floating)):
        return float(c)
    return float(10.0 ** (c.log10_factor + sum(e * x[i] for i, e in c.exponents)))


def resolve(reactions, x, rate_scale):
    """The reaction list with every constant a double: [(net {species: integer}, k, orders {species: integer}, factors [(species, K,
    n, kind)])].  A plain third element: the orders are the reactants' coefficients and there is no factor."""
    x = np.asarray(x, dtype=float)
    out = []
    for reac, prod, rate in reactions:
        net = {}
        for s, c in reac.items():
            net[s] = net.get(s, 0) - c
        for s, c in prod.items():
            net[s] = net.get(s, 0) + c
        law = rate if hasattr(rate, "factors") else None
        orders = dict(reac) if law is None or law.order is None else dict(law.order)
        factors = [] if law is None else [(f.species, constant(f.K, x, rate_scale), f.n, f.kind) for f in law.factors]
        out.append(({s: c for s, c in net.items() if c}, constant(rate if law is None else law.rate, x, rate_scale),
                    {s: c for s, c in orders.items() if c}, factors))
    return out


def _hill(y, K, n, kind):
    """(h, dh/dy) of one factor"""
    Kn, yn = K ** n, y ** n
    den = Kn + yn
    slope = n * Kn * y ** (n - 1) / den ** 2
    return (yn / den, slope) if kind == "activation" else (Kn / den, -slope)


def rhs_and_jacobian(S, resolved, y, num=float, jacobian=True):
    """f [S] and J [S][S] at y as lists, in the arithmetic of num (jacobian=False: J is left at zero)"""
    zero = num(0.0)
    f = [zero] * S
    J = [[zero] * S for _ in range(S)]
    for net, k, orders, factors in resolved:
        parts = [(s, y[s] ** c, c * y[s] ** (c - 1)) for s, c in sorted(orders.items())]          # (species, value, derivative)
        parts += [(s,) + _hill(y[s], num(K), n, kind) for s, K, n, kind in factors]
        v = num(k)
        for _, value, _ in parts:
            v = v * value
        for s, c in net.items():
            f[s] = f[s] + c * v
        for q in sorted({s for s, _, _ in parts}) if jacobian else ():
            dv = zero
            for m, (s, _, slope) in enumerate(parts):                                           # the product rule, term by term
                if s != q:
                    continue
                term = num(k) * slope
                for j, (_, value, _) in enumerate(parts):
                    if j != m:
                        term = term * value
                dv = dv + term
            for s, c in net.items():
                J[s][q] = J[s][q] + c * dv
    return f, J


def jacobian_error(S, resolved, y, dps=30, columns=None):
    """max |J - mpmath.diff(f)| / (1 + |J|) at y, in dps-digit arithmetic: the reference's own analytic Jacobian against numerical
    differentiation of its right-hand side, every row of the given columns (default: all)"""
    import mpmath
    mp = mpmath.mp
    with mp.workdps(dps):
        y = [mp.mpf(float(v)) for v in y]
        _, J = rhs_and_jacobian(S, resolved, y, mp.mpf)
        worst = mp.mpf(0)
        for q in range(S) if columns is None else columns:
            seen = {}                                   # (mp.diff asks for the same abscissae for every row: evaluate f once at each)

            def row(v, s):
                if v not in seen:
                    seen[v] = rhs_and_jacobian(S, resolved, y[:q] + [v] + y[q + 1:], mp.mpf, jacobian=False)[0]
                return seen[v][s]
            for s in range(S):
                d = mp.diff(lambda v: row(v, s), y[q])
                worst = max(worst, abs(d - J[s][q]) / (1 + abs(J[s][q])))
        return float(worst)


def radau(S, resolved, y0, t, t0=0.0, rtol=1e-12, atol=1e-14):
    """The states at the output times t (sorted, >= t0, repeats allowed) by scipy's Radau IIA, [T, S]"""
    from scipy.integrate import solve_ivp
    y0, t = np.asarray(y0, dtype=float), np.asarray(t, dtype=float)
    tu, back = np.unique(t, return_inverse=True)
    if tu[-1] == t0:
        return np.tile(y0, (len(t), 1))
    sol = solve_ivp(lambda _, y: np.array(rhs_and_jacobian(S, resolved, y, np.float64, jacobian=False)[0], dtype=float), (t0, tu[-1]), y0, method="Radau", t_eval=tu,
                    rtol=rtol, atol=atol, jac=lambda _, y: np.array(rhs_and_jacobian(S, resolved, y, np.float64)[1], dtype=float))
    assert sol.success, sol.message
    return sol.y.T[back]


def piecewise_radau(S, resolved, y0, t, events, t0=0.0, **kw):
    """Radau through events (time, species, factor, amount): an output at an event's time is taken before the event, the events at t0
    apply to y0 first."""
    y, now, out = np.asarray(y0, dtype=float).copy(), t0, []
    pending = sorted(events, key=lambda ev: ev[0])
    for tau in t:
        while True:
            for ev in [ev for ev in pending if ev[0] <= now]:
                y[ev[1]] = ev[2] * y[ev[1]] + ev[3]
            pending = [ev for ev in pending if ev[0] > now]
            stop = min([ev[0] for ev in pending if ev[0] < tau] + [tau])
            if stop > now:
                y = radau(S, resolved, y, [stop], t0=now, **kw)[0]
                now = stop
            if stop == tau:
                break
        out.append(y.copy())
    return np.array(out)


def steady_state(S, resolved, y0, span=1e7):
    """The resting state: Radau to a time far beyond every time scale of the test networks"""
    return radau(S, resolved, y0, [span], rtol=1e-12, atol=1e-14)[0]


def _rodas4_fixed(fj, S, y0, t0, t1, n, embedded, num, factor, solve):
    """tests/ode_reference._rodas4_fixed with the right-hand side passed in: fj(y, jacobian) -> (f, J) as lists in the arithmetic of num"""
    y = [num(float(v)) for v in y0]
    h = (num(float(t1)) - num(float(t0))) / n
    zero = num(0.0)
    for _ in range(n):
        _, J = fj(y, True)
        lu = factor([[(1 / (h * num(GAMMA)) if s == q else zero) - J[s][q] for q in range(S)] for s in range(S)])
        ks, arg = [], y
        for i in range(6):
            arg = [y[s] + sum((num(A[i][j]) * ks[j][s] for j in range(i)), zero) for s in range(S)] if i < 5 else [arg[s] + ks[4][s] for s in range(S)]
            f, _ = fj(arg, False)
            ks.append(solve(lu, [f[s] + sum((num(C[i][j]) * ks[j][s] for j in range(i)), zero) / h for s in range(S)]))
        y = list(arg) if embedded else [arg[s] + ks[5][s] for s in range(S)]
    return y


def rodas4_fixed_mp(S, resolved, y0, t0, t1, n, embedded=False, dps=40):
    import mpmath
    mp = mpmath.mp
    with mp.workdps(dps):
        def solve(lu, b):
            LU, p = lu
            return list(mp.U_solve(LU, mp.L_solve(LU, mp.matrix(b), p)))
        return _rodas4_fixed(lambda y, jac: rhs_and_jacobian(S, resolved, y, mp.mpf, jac), S, y0, t0, t1, n, embedded, mp.mpf, lambda W: mp.LU_decomp(mp.matrix(W)), solve)


def rodas4_fixed_f64(S, resolved, y0, t0, t1, n, embedded=False):
    def solve(W, b):
        return list(np.linalg.solve(W, np.array(b, dtype=np.float64)))
    return np.array(_rodas4_fixed(lambda y, jac: rhs_and_jacobian(S, resolved, y, np.float64, jac), S, y0, t0, t1, n, embedded, np.float64,
                                  lambda W: np.array(W, dtype=np.float64), solve), dtype=float)


def fixed_step_reference(S, resolved, y0, t0, t1, n, embedded):
    """(the mp solution, max |mp|, tol) with tests/ode_reference.fixed_step_reference's formula: tol = 64 max|f64 - mp| / max|mp| + 16 eps"""
    import mpmath
    ref = rodas4_fixed_mp(S, resolved, y0, t0, t1, n, embedded)
    f64 = rodas4_fixed_f64(S, resolved, y0, t0, t1, n, embedded)
    with mpmath.mp.workdps(40):
        scale = max(abs(v) for v in ref)
        dev = max(abs(mpmath.mpf(float(a)) - b) for a, b in zip(f64, ref))
        tol = float(64 * dev / scale) + 16 * np.finfo(float).eps
    return ref, scale, tol
