"""One reference for the networks of tests/ode_combined_networks.py, composed of the references that exist and sharing no code with
pydream_amd: RateLaw, Hill, Monomial, Input and Noise are read as records (their attributes), never evaluated by their own code.

  * trajectories: ode_ratelaw_reference.resolve / rhs_and_jacobian / radau (scipy's Radau IIA at rtol 1e-12 on a right-hand side and an
    analytic Jacobian built from the reaction list), restarted at every knot and event time.  An input is carried as
    ode_input_networks.piecewise_radau carries it, rebuilt on the rate-law right-hand side: the input species is set by hand to
    g * u(tau) at each segment's start and fed by a zero-order source whose rate is the segment's slope times the gain.  An output at a
    breakpoint is taken first, then the knots, then the events in the order given;
  * equilibrate: ode_ratelaw_reference.steady_state (Radau far beyond every time scale) with the inputs held at g * u(t0) and every
    slope 0, then the knot at t0 and the events at t0;
  * likelihood: from the host build's simulate output in 40-digit mpmath, ode_noise_reference.experiment_loglike per condition, the
    constraints' term (the definition: sum norm(loc, sd).logpdf(monomial)) added to condition 0, the conditions added left to right."""
import mpmath as mp
import numpy as np

from . import ode_noise_reference as NR
from . import ode_ratelaw_reference as RR


def _number(c, x, rate_scale):
    """a y0 or scale entry: a plain number, or a Monomial record"""
    return RR.constant(c, x, rate_scale) if hasattr(c, "exponents") else float(c)


def _slope(u, tau):
    """of the table's segment that follows tau (the last segment's for tau at or past the end)"""
    j = int(np.clip(np.searchsorted(u.times, tau, side="right") - 1, 0, len(u.times) - 2))
    return (u.values[j + 1] - u.values[j]) / (u.times[j + 1] - u.times[j])


def states(rec, c, x, rtol=1e-12, atol=1e-14):
    """The states of condition c at the output times, [T, S]"""
    S, t, t0 = rec.S, np.asarray(rec.t, dtype=float), rec.t0
    inputs, events = rec.inputs[c], list(rec.events[c])
    base = RR.resolve(rec.reactions, x, rec.rate_scale)
    g = [1.0 if u.gain is None else RR.constant(u.gain, x, rec.rate_scale) for u in inputs]
    system = lambda tau: base + [({u.species: 1}, gi * (0.0 if tau is None else _slope(u, tau)), {}, []) for u, gi in zip(inputs, g)]      # noqa: E731

    def intervene(y, tau):
        for u, gi in zip(inputs, g):
            y[u.species] = gi * float(np.interp(tau, u.times, u.values))
        for time, s, factor, amount in events:
            if time == tau:
                y[s] = factor * y[s] + amount

    y = np.array([_number(v, x, rec.rate_scale) for v in rec.y0[c]], dtype=float)
    for u, gi in zip(inputs, g):
        y[u.species] = gi * float(np.interp(t0, u.times, u.values))
    if rec.equilibrate[c]:
        y = RR.steady_state(S, system(None), y).copy()
    intervene(y, t0)
    out, done, now = np.empty((len(t), S)), np.zeros(len(t), dtype=bool), t0
    breaks = sorted({tau for u in inputs for tau in u.times if t0 < tau < t[-1]} | {ev[0] for ev in events if t0 < ev[0] < t[-1]})
    for tau in breaks + [None]:
        end = t[-1] if tau is None else tau
        take = ~done & (t <= end)
        ys = RR.radau(S, system(now), y, np.r_[t[take], end], t0=now, rtol=rtol, atol=atol)
        out[take], done = ys[:-1], done | take
        y, now = ys[-1].copy(), end
        if tau is not None:
            intervene(y, tau)
    assert done.all()
    return out


def observed(args):
    """(rec, x) -> the scaled observables of the three conditions, [C, T, O]; for a process pool"""
    rec, x = args
    scale = np.array([_number(f, x, rec.rate_scale) for f in rec.scale])
    return np.array([states(rec, c, x) @ np.asarray(rec.observables, dtype=float).T * scale for c in range(len(rec.events))])


def constraint_term(constraints, x):
    """(value, A, N) of sum norm(loc, sd).logpdf(monomial) in mpmath, A and N as ode_noise_reference.experiment_loglike counts them"""
    C, terms = mp.mpf(0), []
    for m, loc, sd in constraints:
        v = mp.mpf(10) ** (mp.mpf(m.log10_factor) + sum(mp.mpf(e) * mp.mpf(float(x[i])) for i, e in m.exponents))
        C += -mp.log(mp.mpf(sd)) - mp.log(2 * mp.pi) / 2
        terms.append(-((v - mp.mpf(loc)) / mp.mpf(sd)) ** 2 / 2)
    return C + sum(terms), abs(C) + sum(abs(v) for v in terms), len(terms)


def loglike(like, rec, X, sims):
    """(terms [n, C], total [n], A [n, C], N [n, C]) from sims = like.simulate(X), [n, C, T, O]: term c is condition c's log-likelihood
    (condition 0 with the constraints' term), total ((l0 + l1) + l2) in mpmath; a row whose simulation is not finite: NaN."""
    n, C = len(X), len(like.conditions)
    terms, A, N, total = np.full((n, C), np.nan), np.full((n, C), np.nan), np.zeros((n, C)), np.full(n, np.nan)
    for i, x in enumerate(X):
        if not np.all(np.isfinite(sims[i])):
            continue
        parts = [NR.experiment_loglike(like, x, sims[i, c], cond["data"], cond["sd"]) for c, cond in enumerate(like.conditions)]
        g = constraint_term(rec.constraints, x)
        parts[0] = tuple(a + b for a, b in zip(parts[0], g))
        acc = parts[0][0]
        for p in parts[1:]:
            acc = acc + p[0]
        total[i] = float(acc)
        for c, p in enumerate(parts):
            terms[i, c], A[i, c], N[i, c] = float(p[0]), float(p[1]), p[2]
    return terms, total, A, N
