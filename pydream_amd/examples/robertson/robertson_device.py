"""The Robertson example on the device: robertson_nopysb/example_sample_robertson_nopysb_with_dream.py with its likelihood written as a
MassActionODELogLike instead of a Python function around scipy's odeint.  The three reactions

    A -> B          k1 = 10**theta[0]
    2B -> B + C     k2 = 10**theta[1]
    B + C -> A + C  k3 = 10**theta[2]

from y0 = (1, 0, 0), the total of C observed at 50 times in [0, 40] with sd 0.01, log10 rate constants under a uniform prior six decades
wide around the nominal (0.04, 3e7, 1e4); run_dream with the example's own keyword arguments.  Each proposal's ODE is integrated by the
stiff Rosenbrock solver of csrc/dz_ode.h, one GPU lane per point.  The data are simulated from the nominal constants (the example reads
them from files of the same name).

    python -m pydream_amd.examples.robertson.robertson_device [niterations] [nchains]
"""
import sys

import numpy as np

from pydream_amd.likelihoods import MassActionODELogLike

REACTIONS = [({0: 1}, {1: 1}, 0), ({1: 2}, {1: 1, 2: 1}, 1), ({1: 1, 2: 1}, {0: 1, 2: 1}, 2)]
Y0 = [1.0, 0.0, 0.0]
TSPAN = np.linspace(0, 40)
NOMINAL = np.log10([.04, 3.0e7, 1.0e4])
SD = 0.01


def simulated_data(rtol=1e-12, atol=1e-14):
    """C total at TSPAN for the nominal constants, integrated tightly on the host."""
    tight = MassActionODELogLike(3, REACTIONS, Y0, TSPAN, [[0, 0, 1]], np.zeros((1, len(TSPAN))), np.ones((1, len(TSPAN))), rtol=rtol, atol=atol,
                                 max_steps=100000)
    return tight.simulate(NOMINAL)[0, :, 0]


def make_likelihood(data=None, sd=SD, **kw):
    data = simulated_data() if data is None else np.asarray(data, dtype=float)
    return MassActionODELogLike(3, REACTIONS, Y0, TSPAN, [[0, 0, 1]], data[None, :], np.broadcast_to(sd, data.shape)[None, :],
                                rate_scale="log10", **kw)


def main(niterations=100, nchains=5):
    from scipy.stats import uniform
    from pydream_amd.core import run_dream
    from pydream_amd.parameters import SampledParam
    like = make_likelihood()
    lower = NOMINAL - 3
    sampled, log_ps = run_dream([SampledParam(uniform, loc=lower, scale=6)], like, niterations=niterations, nchains=nchains, multitry=False,
                                gamma_levels=4, adapt_gamma=True, history_thin=1, model_name="robertson_device", verbose=False, save_history=False)
    S, L = np.concatenate(sampled), np.concatenate(log_ps)
    best = S[np.argmax(L)]
    print("robertson on the device: %d chains x %d iterations; best log p %.3f at log10 k = %s (nominal %s)"
          % (nchains, niterations, L.max(), np.round(best, 3), np.round(NOMINAL, 3)))
    return sampled, log_ps


if __name__ == "__main__":
    main(*(int(a) for a in sys.argv[1:3]))
