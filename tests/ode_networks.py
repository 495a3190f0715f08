"""Networks shared by the ODE likelihood tests: Robertson (3 species, stiff), Michaelis-Menten (4 species) and an 8-species chain,
each with a scipy right-hand side and Jacobian for an independent reference solution."""
import numpy as np

from pydream_amd.examples.robertson import robertson_device as ROB
from pydream_amd.likelihoods import MassActionODELogLike

ROB_LOWER = ROB.NOMINAL - 3

# E + S <-> ES -> E + P   (species E, S, ES, P; log10 rates)
MM_REACTIONS = [({0: 1, 1: 1}, {2: 1}, 0), ({2: 1}, {0: 1, 1: 1}, 1), ({2: 1}, {0: 1, 3: 1}, 2)]
MM_Y0 = [0.5, 2.0, 0.0, 0.0]
MM_NOMINAL = np.log10([3.0, 0.5, 1.2])
MM_T = np.linspace(0.5, 10.0, 20)

# 0 <-> 1 <-> ... <-> 7 plus 0 + 7 -> 2 x 3: eight species, 15 reactions, every species observed
CHAIN_REACTIONS = [({i: 1}, {i + 1: 1}, i) for i in range(7)] + [({i + 1: 1}, {i: 1}, 7 + i) for i in range(7)] + [({0: 1, 7: 1}, {3: 2}, 14)]
CHAIN_Y0 = [1.0, 0.5, 0.0, 0.0, 0.2, 0.0, 0.0, 0.3]
CHAIN_NOMINAL = np.log10(np.r_[np.linspace(0.5, 2.0, 7), np.linspace(0.1, 0.4, 7), 3.0])
CHAIN_T = np.linspace(0.0, 5.0, 11)


def stoich(S, reactions):
    N = np.zeros((S, len(reactions)))
    for r, (reac, prod, _) in enumerate(reactions):
        for s, c in reac.items():
            N[s, r] -= c
        for s, c in prod.items():
            N[s, r] += c
    return N


def scipy_model(S, reactions, theta):
    """f(t, y), J(t, y) of a mass-action network with rate constants 10**theta (written independently of the generated code)."""
    k = 10.0 ** np.asarray([theta[r[2]] for r in reactions], dtype=float)
    N = stoich(S, reactions)
    nu = np.zeros((len(reactions), S))
    for r, (reac, _, _) in enumerate(reactions):
        for s, c in reac.items():
            nu[r, s] = c

    def f(t, y):
        return N @ (k * np.prod(y[None, :] ** nu, axis=1))

    def jac(t, y):
        P = y[None, :] ** nu                                                  # [R, S]
        D = np.empty_like(P)
        for q in range(S):
            others = np.prod(np.delete(P, q, axis=1), axis=1)
            D[:, q] = k * nu[:, q] * np.where(nu[:, q] > 0, y[q] ** np.maximum(nu[:, q] - 1, 0), 0.0) * others
        return N @ D
    return f, jac


def radau(S, reactions, y0, t, theta, rtol=1e-12, atol=1e-14, t0=0.0):
    """The states at t by scipy's Radau IIA, [T, S]."""
    from scipy.integrate import solve_ivp
    f, jac = scipy_model(S, reactions, theta)
    t = np.asarray(t, dtype=float)
    sol = solve_ivp(f, (t0, t[-1]), np.asarray(y0, dtype=float), method="Radau", t_eval=t, rtol=rtol, atol=atol, jac=jac)
    assert sol.success, sol.message
    return sol.y.T


def robertson(**kw):
    return ROB.make_likelihood(**kw)


def michaelis_menten(**kw):
    y = radau(4, MM_REACTIONS, MM_Y0, MM_T, MM_NOMINAL)
    data = y[:, [1, 3]].T.copy()
    data[0, 3] = np.nan                                                        # one entry not observed
    return MassActionODELogLike(4, MM_REACTIONS, MM_Y0, MM_T, [[0, 1, 0, 0], [0, 0, 0, 1]], data, 0.05 * np.abs(data) + 0.01, **kw)


def chain8(**kw):
    y = radau(8, CHAIN_REACTIONS, CHAIN_Y0, CHAIN_T, CHAIN_NOMINAL)
    return MassActionODELogLike(8, CHAIN_REACTIONS, CHAIN_Y0, CHAIN_T, np.eye(8), y.T.copy(), 0.02, **kw)


def box_points(nominal, n, seed, width=3.0, outside=0.0):
    """n points uniform in nominal +- width (+ outside on each side)."""
    rng = np.random.default_rng(seed)
    return nominal - width - outside + (2 * (width + outside)) * rng.uniform(size=(n, len(nominal)))
