"""A dose-response series on the device: ONE enzyme network, one vector of rate constants, measured at six substrate doses -- the shape
of most calibrations (dose series, knock-outs, wash-outs), written as MassActionODELogLike(conditions=[...]).

    E + S <-> ES -> E + P           k_on = 10**theta[0], k_off = 10**theta[1], k_cat = 10**theta[2]
    E + I <-> EI                    k_i = 10**theta[3], k_-i = 10**theta[4]        (a competitive inhibitor, the same amount in every dose)

From E = 0.2, I = 0.5 and S = 0.25, 0.5, 1, 2, 4, 8; the product P and the free substrate S observed at 12 times in [0.5, 12] with
sd 4 % + 0.01; log10 rate constants under a uniform prior two decades wide around the nominal ones.  One time course does not pin the
five constants down -- at a low dose the enzyme is never saturated and only k_cat k_on / (k_off + k_cat) shows, at a high dose only
k_cat -- the series does.  Every proposal is integrated six times, from six starts: a launch covers proposals x doses work items (one
GPU lane each, the dose the fastest index) and the engine adds each proposal's six terms in a fixed order (dz_set_likelihood_items).
The data are simulated from the nominal constants.

    python -m pydream_amd.examples.dose_response.dose_response_device [niterations] [nchains]
"""
import sys

import numpy as np

from pydream_amd.likelihoods import MassActionODELogLike

SPECIES = ("E", "S", "ES", "P", "I", "EI")
E, S, ES, P, I, EI = range(6)
REACTIONS = [({E: 1, S: 1}, {ES: 1}, 0), ({ES: 1}, {E: 1, S: 1}, 1), ({ES: 1}, {E: 1, P: 1}, 2),
             ({E: 1, I: 1}, {EI: 1}, 3), ({EI: 1}, {E: 1, I: 1}, 4)]
DOSES = (0.25, 0.5, 1.0, 2.0, 4.0, 8.0)
NOMINAL = np.log10([5.0, 1.0, 1.5, 4.0, 0.8])
TSPAN = np.linspace(0.5, 12.0, 12)
OBSERVABLES = np.zeros((2, 6))
OBSERVABLES[[0, 1], [P, S]] = 1.0


def start_amounts(dose):
    y0 = np.zeros(6)
    y0[[E, S, I]] = [0.2, dose, 0.5]
    return y0


def simulated_data(rtol=1e-12, atol=1e-14):
    """P and S at TSPAN for the nominal constants under every dose, [doses, 2, T], integrated tightly on the host."""
    blank = np.zeros((2, len(TSPAN)))
    tight = MassActionODELogLike(6, REACTIONS, None, TSPAN, OBSERVABLES, blank, np.ones_like(blank), rtol=rtol, atol=atol, max_steps=100000,
                                 conditions=[dict(y0=start_amounts(s)) for s in DOSES])
    return tight.simulate(NOMINAL)[0].transpose(0, 2, 1).copy()


def make_likelihood(data=None, sd=None, **kw):
    data = simulated_data() if data is None else np.asarray(data, dtype=float)
    sd = 0.04 * np.abs(data) + 0.01 if sd is None else np.broadcast_to(sd, data.shape)
    conditions = [dict(y0=start_amounts(s), data=data[c], sd=sd[c]) for c, s in enumerate(DOSES)]
    return MassActionODELogLike(6, REACTIONS, None, TSPAN, OBSERVABLES, None, None, rate_scale="log10", conditions=conditions, **kw)


def main(niterations=200, nchains=64):
    from scipy.stats import uniform
    from pydream_amd.core import run_dream
    from pydream_amd.parameters import SampledParam
    like = make_likelihood()
    lower = NOMINAL - 1
    sampled, log_ps = run_dream([SampledParam(uniform, loc=lower, scale=2)], like, niterations=niterations, nchains=nchains, multitry=5,
                                model_name="dose_response_device", verbose=False, save_history=False)
    S_, L = np.concatenate(sampled), np.concatenate(log_ps)
    best = S_[np.argmax(L)]
    print("dose response on the device (%d doses per proposal): %d chains x %d iterations; best log p %.3f at log10 k = %s (nominal %s)"
          % (len(DOSES), nchains, niterations, L.max(), np.round(best, 3), np.round(NOMINAL, 3)))
    return sampled, log_ps


if __name__ == "__main__":
    main(*(int(a) for a in sys.argv[1:3]))
