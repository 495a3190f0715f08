"""A fit with UNKNOWN MEASUREMENT NOISE on the device: the Robertson network of examples/robertson,

    A -> B          k1 = 10**theta[0]
    2B -> B + C     k2 = 10**theta[1]
    B + C -> A + C  k3 = 10**theta[2]

with the total of C read at 49 times in (0, 40] by an instrument whose error nobody wrote down: an additive part and a part proportional
to the signal, sd = sigma + rel * C.  Both are sampled along with the rate constants (MassActionODELogLike with noise=[Noise(3, rel=4)]):

    theta = log10 [k1, k2, k3, sigma, rel]

five coordinates under a uniform prior: the rate constants a decade on each side of the nominal (0.04, 3e7, 1e4), sigma and rel a decade
on each side of the values the data were made with (0.004 and 0.03).  The residual's scale and the term -log s are evaluated at every
output time inside the stiff solver (csrc/dz_ode.h, NOISE), so the whole likelihood stays on the GPU.  The data are simulated from the
nominal constants with seeded normal errors of that size.

    python -m pydream_amd.examples.noise.noise_device [niterations] [nchains] [--host]

--host: the same run with the likelihood's host twin as a plain Python callable (run_dream's host path), which gives the same bits.
"""
import sys

import numpy as np

from pydream_amd.examples.robertson import robertson_device as ROB
from pydream_amd.likelihoods import MassActionODELogLike, Noise

SIGMA, REL = 3, 4                           # the coordinates of the noise model
TRUE = np.r_[ROB.NOMINAL, np.log10([0.004, 0.03])]      # the point the data are simulated from
WIDTH = 1.0                                 # the prior box: TRUE +- WIDTH
TSPAN = ROB.TSPAN[1:]                       # (C is 0 at t = 0: nothing to learn from that reading)


def simulated_data(seed=5):
    """C total at TSPAN for the nominal constants plus normal errors of sd sigma + rel * C."""
    clean = ROB.simulated_data()[1:]
    sigma, rel = 10.0 ** TRUE[[SIGMA, REL]]
    return clean + (sigma + rel * clean) * np.random.default_rng(seed).standard_normal(len(clean))


def make_likelihood(data=None, **kw):
    data = simulated_data() if data is None else np.asarray(data, dtype=float)
    return MassActionODELogLike(3, ROB.REACTIONS, ROB.Y0, TSPAN, [[0, 0, 1]], data[None, :], None, rate_scale="log10",
                                noise=[Noise(SIGMA, rel=REL)], **kw)


class HostTwin:
    """The likelihood as a plain Python callable: run_dream takes the host path"""
    def __init__(self, like):
        self.like = like

    def __call__(self, x):
        return self.like(x)


def main(niterations=300, nchains=64, host=False, like=None):
    from scipy.stats import uniform
    from pydream_amd.core import run_dream
    from pydream_amd.parameters import SampledParam
    like = make_likelihood() if like is None else like
    rng = np.random.default_rng(31)
    starts = [TRUE + 0.25 * WIDTH * rng.uniform(-1, 1, len(TRUE)) for _ in range(nchains)]
    sampled, log_ps = run_dream([SampledParam(uniform, loc=TRUE - WIDTH, scale=2 * WIDTH)], HostTwin(like) if host else like,
                                niterations=niterations, nchains=nchains, multitry=5, start=starts, model_name="noise_device", verbose=False,
                                save_history=False, seed=32)
    S, L = np.concatenate(sampled), np.concatenate(log_ps)
    best = S[np.argmax(L)]
    print("unknown noise on %s: %d chains x %d iterations; best log p %.3f at log10 [k1, k2, k3, sigma, rel] = %s (true %s)"
          % ("the host twin" if host else "the device", nchains, niterations, L.max(), np.round(best, 3), np.round(TRUE, 3)))
    return sampled, log_ps


if __name__ == "__main__":
    argv = [a for a in sys.argv[1:] if a != "--host"]
    main(*(int(a) for a in argv[:2]), host="--host" in sys.argv[1:])
