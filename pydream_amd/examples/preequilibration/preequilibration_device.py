"""A receptor at its resting level before the ligand arrives, on the device: an experiment that starts from the STEADY STATE of the
unstimulated system (MassActionODELogLike(equilibrate=...)), a state that depends on the sampled rate constants.

    0 -> R              k_syn       synthesis
    R -> 0              k_deg       degradation
    R + L <-> RL        k_on, k_off
    RL -> 0             k_int       internalisation of the complex

Without ligand the receptor settles at R = k_syn / k_deg: nobody writes that amount down, it follows from the point.  Every
experiment therefore starts from (0, 0, 0) with equilibrate=True -- the solver integrates the unstimulated system, without a clock and
without an end time, until the state would move by less than the tolerance over the length of the experiment -- and the ligand is a
bolus at t0, the event (0, L, 1, dose), applied to the resting state.  Four doses, one condition per dose; the complex is read out in
arbitrary units (scale = Monomial({5: 1})):

    theta = log10 [k_syn, k_deg, k_on, k_off, k_int, scale]

24 readings per dose, every 2.5 time units up to 60, sd 3 % + 0.02; a uniform prior two decades wide around the nominal values.  A
proposal is four work items, each an equilibration and then the experiment.  The data are simulated with scipy's Radau at the nominal
values, started from the closed form (k_syn / k_deg, dose, 0).

    python -m pydream_amd.examples.preequilibration.preequilibration_device [niterations] [nchains]
"""
import sys

import numpy as np

from pydream_amd.likelihoods import MassActionODELogLike, Monomial

SPECIES = ("R", "L", "RL")
R, L, RL = range(3)
K_SYN, K_DEG, K_ON, K_OFF, K_INT, SCALE = range(6)
REACTIONS = [({}, {R: 1}, K_SYN), ({R: 1}, {}, K_DEG), ({R: 1, L: 1}, {RL: 1}, K_ON), ({RL: 1}, {R: 1, L: 1}, K_OFF), ({RL: 1}, {}, K_INT)]
NOMINAL = np.log10([0.1, 0.1, 1.0, 0.1, 0.05, 50.0])
DOSES = (0.1, 0.3, 1.0, 3.0)
TSPAN = np.linspace(2.5, 60.0, 24)
OBSERVABLES = np.zeros((1, 3))
OBSERVABLES[0, RL] = 1.0


def resting_receptor(x):
    """k_syn / k_deg for the rows of x: the receptor's level without ligand"""
    x = np.asarray(x, dtype=float)
    return 10.0 ** (x[..., K_SYN] - x[..., K_DEG])


def simulated_data(rtol=1e-10, atol=1e-12):
    """The scaled readout at TSPAN for the nominal values at every dose, [doses, 1, T], by scipy's Radau from the closed-form resting
    state with the dose added."""
    from scipy.integrate import solve_ivp
    k_syn, k_deg, k_on, k_off, k_int, scale = 10.0 ** NOMINAL

    def f(t, y):
        v = k_on * y[R] * y[L] - k_off * y[RL]
        return [k_syn - k_deg * y[R] - v, -v, v - k_int * y[RL]]
    out = []
    for dose in DOSES:
        sol = solve_ivp(f, (0.0, TSPAN[-1]), [k_syn / k_deg, dose, 0.0], method="Radau", t_eval=TSPAN, rtol=rtol, atol=atol)
        assert sol.success, sol.message
        out.append(scale * (OBSERVABLES @ sol.y))
    return np.array(out)


def make_likelihood(data=None, sd=None, **kw):
    data = simulated_data() if data is None else np.asarray(data, dtype=float)
    sd = 0.03 * np.abs(data) + 0.02 if sd is None else np.broadcast_to(sd, data.shape)
    conditions = [dict(data=data[c], sd=sd[c], events=[(0.0, L, 1.0, dose)]) for c, dose in enumerate(DOSES)]
    kw.setdefault("equilibrate", True)
    return MassActionODELogLike(3, REACTIONS, [0.0, 0.0, 0.0], TSPAN, OBSERVABLES, None, None, rate_scale="log10", conditions=conditions,
                                scale=[Monomial({SCALE: 1})], **kw)


def check_resting_state(like, X):
    """The host build's resting state against the closed form, for the rows of X: no ligand, no complex, and the receptor within what
    the steady-state test allows -- only R moves, so the test |f| horizon <= sqrt(S) (atol + rtol R) with f = k_deg (k_syn / k_deg - R)
    bounds the distance from k_syn / k_deg.  Returns the largest distance in units of that bound (<= 1 up to rounding)."""
    X = np.asarray(X, dtype=float).reshape(-1, len(NOMINAL))
    y = like.steady_state(X)
    worst = 0.0
    for c, cond in enumerate(like.conditions):
        eq = cond["equilibrate"]
        assert np.all(np.isfinite(y[:, c])) and np.all(y[:, c, L] == 0.0) and np.all(y[:, c, RL] == 0.0)
        bound = np.sqrt(3.0) * (eq["atol"] + eq["rtol"] * np.abs(y[:, c, R])) / (10.0 ** X[:, K_DEG] * eq["horizon"])
        worst = max(worst, float(np.max(np.abs(y[:, c, R] - resting_receptor(X)) / bound)))
    assert worst <= 1.0 + 1e-6, worst
    return worst


def main(niterations=1500, nchains=64):
    from scipy.stats import uniform
    from pydream_amd.convergence import Gelman_Rubin
    from pydream_amd.core import run_dream
    from pydream_amd.parameters import SampledParam
    like = make_likelihood()
    lower = NOMINAL - 1
    worst = check_resting_state(like, lower + 2 * np.random.default_rng(1).uniform(size=(64, len(NOMINAL))))
    sampled, log_ps = run_dream([SampledParam(uniform, loc=lower, scale=2)], like, niterations=niterations, nchains=nchains, multitry=5,
                                nseedchains=2 * nchains, model_name="preequilibration_device", verbose=False, save_history=False)
    S_, L_ = np.concatenate(sampled), np.concatenate(log_ps)
    best = S_[np.argmax(L_)]
    half = np.concatenate([s[len(s) // 2:] for s in sampled])
    rest = np.log10(resting_receptor(half))
    lo, hi = np.percentile(rest, [2.5, 97.5])
    truth = float(np.log10(resting_receptor(NOMINAL)))
    print("a receptor equilibrated before the ligand arrives, on the device (%d doses per proposal, each equilibrated first; host check of "
          "the resting state against k_syn / k_deg: %.3f of the test's bound): %d chains x %d iterations; best log p %.3f at log10 [k_syn, "
          "k_deg, k_on, k_off, k_int, scale] = %s (nominal %s); log10 (k_syn / k_deg) of the second half: 95 %% in [%.3f, %.3f], used for "
          "the data: %.3f (%s); R-hat of the second half: %s"
          % (len(DOSES), worst, nchains, niterations, L_.max(), np.round(best, 3), np.round(NOMINAL, 3), lo, hi, truth,
             "covered" if lo <= truth <= hi else "NOT covered", np.round(Gelman_Rubin([s[len(s) // 2:] for s in sampled]), 3)))
    return sampled, log_ps


if __name__ == "__main__":
    main(*(int(a) for a in sys.argv[1:3]))
