"""Association and wash-out of a ligand on the device: the one design that separates k_on from k_off, as a likelihood with an EVENT
during the experiment (MassActionODELogLike(events=...)).

    R + L <-> RL        k_on, k_off

The receptor R (total 1) meets the ligand L at t = 0 and binds it; at T_WASH the free ligand is washed out -- the event
(T_WASH, L, 0, 0): the amount of L becomes 0 * L + 0 -- and the complex RL falls apart again (what dissociates may bind once more: the
amount of ligand stays what the complex releases).  The association phase alone fixes little more than k_on [L] + k_off and the plateau's
KD = k_off / k_on; the decay after the wash-out shows k_off by itself.  The complex is read out in arbitrary units
(scale = Monomial({2: 1})) at four ligand doses, one condition per dose, the same wash-out in each:

    theta = log10 [k_on, k_off, scale]

24 readings per dose, every 2.5 time units up to 60, one of them at T_WASH itself -- taken BEFORE the wash-out: measure, then
intervene --, sd 3 % + 0.02; a uniform prior two decades wide around the nominal values.  A proposal is four integrations, each in two
segments with a restart of the step controller at the wash-out: one launch over proposals x 4 work items.  The data are simulated with
scipy's Radau, restarted at the wash-out, at the nominal values.

    python -m pydream_amd.examples.washout.washout_device [niterations] [nchains]
"""
import sys

import numpy as np

from pydream_amd.likelihoods import MassActionODELogLike, Monomial

SPECIES = ("R", "L", "RL")
R, L, RL = range(3)
K_ON, K_OFF, SCALE = range(3)
REACTIONS = [({R: 1, L: 1}, {RL: 1}, K_ON), ({RL: 1}, {R: 1, L: 1}, K_OFF)]
NOMINAL = np.log10([1.0, 0.1, 50.0])
DOSES = (0.03, 0.1, 0.3, 1.0)
T_WASH = 30.0
TSPAN = np.linspace(2.5, 60.0, 24)
WASHOUT = [(T_WASH, L, 0.0, 0.0)]
OBSERVABLES = np.zeros((1, 3))
OBSERVABLES[0, RL] = 1.0


def start_amounts(dose):
    return [1.0, dose, 0.0]


def simulated_data(rtol=1e-10, atol=1e-12):
    """The scaled readout at TSPAN for the nominal values at every dose, [doses, 1, T], by scipy's Radau: up to the wash-out, the free
    ligand set to 0 by hand, on from there.  The reading at T_WASH is the one before the wash-out."""
    from scipy.integrate import solve_ivp
    k_on, k_off, scale = 10.0 ** NOMINAL

    def f(t, y):
        v = k_on * y[R] * y[L] - k_off * y[RL]
        return [-v, -v, v]
    before = TSPAN <= T_WASH
    out = []
    for dose in DOSES:
        upto = np.unique(np.r_[TSPAN[before], T_WASH])
        a = solve_ivp(f, (0.0, T_WASH), start_amounts(dose), method="Radau", t_eval=upto, rtol=rtol, atol=atol)
        assert a.success, a.message
        y = a.y[:, -1].copy()
        y[L] = 0.0
        b = solve_ivp(f, (T_WASH, TSPAN[-1]), y, method="Radau", t_eval=TSPAN[~before], rtol=rtol, atol=atol)
        assert b.success, b.message
        out.append(scale * (OBSERVABLES @ np.concatenate([a.y[:, np.searchsorted(upto, TSPAN[before])], b.y], axis=1)))
    return np.array(out)


def make_likelihood(data=None, sd=None, **kw):
    data = simulated_data() if data is None else np.asarray(data, dtype=float)
    sd = 0.03 * np.abs(data) + 0.02 if sd is None else np.broadcast_to(sd, data.shape)
    conditions = [dict(y0=start_amounts(dose), data=data[c], sd=sd[c]) for c, dose in enumerate(DOSES)]
    return MassActionODELogLike(3, REACTIONS, None, TSPAN, OBSERVABLES, None, None, rate_scale="log10", conditions=conditions,
                                scale=[Monomial({SCALE: 1})], events=WASHOUT, **kw)


def main(niterations=300, nchains=64):
    from scipy.stats import uniform
    from pydream_amd.convergence import Gelman_Rubin
    from pydream_amd.core import run_dream
    from pydream_amd.parameters import SampledParam
    like = make_likelihood()
    lower = NOMINAL - 1
    sampled, log_ps = run_dream([SampledParam(uniform, loc=lower, scale=2)], like, niterations=niterations, nchains=nchains, multitry=5,
                                nseedchains=2 * nchains, model_name="washout_device", verbose=False, save_history=False)
    S_, L_ = np.concatenate(sampled), np.concatenate(log_ps)
    best = S_[np.argmax(L_)]
    half = np.concatenate([s[len(s) // 2:] for s in sampled])
    print("association and wash-out on the device (%d doses per proposal, a wash-out at t = %g in each): %d chains x %d iterations; "
          "best log p %.3f at log10 [k_on, k_off, scale] = %s (nominal %s); sd of the second half: %s; R-hat of the second half: %s"
          % (len(DOSES), T_WASH, nchains, niterations, L_.max(), np.round(best, 3), np.round(NOMINAL, 3), np.round(half.std(axis=0), 3),
             np.round(Gelman_Rubin([s[len(s) // 2:] for s in sampled]), 3)))
    return sampled, log_ps


if __name__ == "__main__":
    main(*(int(a) for a in sys.argv[1:3]))
