"""The fit of examples/noise under the PRIORS PEOPLE GIVE SUCH QUANTITIES, all on the device: the Robertson network

    A -> B          k1 = theta[0]
    2B -> B + C     k2 = theta[1]
    B + C -> A + C  k3 = theta[2]

with rate_scale="linear" -- the coordinates are the rate constants themselves -- and the total of C read at 49 times in (0, 40] with an
error of sd = sigma + rel * C, both parts sampled:

    theta = [k1, k2, k3, sigma, rel]

    k1, k2, k3   log-normal around the nominal (0.04, 3e7, 1e4), shape 0.5:   scipy.stats.lognorm(0.5, scale=nominal)
    sigma        half-normal, scale 0.02:                                     scipy.stats.halfnorm(scale=0.02)
    rel          half-Cauchy, scale 0.1:                                      scipy.stats.halfcauchy(scale=0.1)

None of the three is a normal or a uniform distribution.  Each parameter describes itself to the engine (SampledParam.device_prior_ext,
dz_set_prior_ext: kinds 6, 9 and 10 of csrc/dz_prior_ext.h), a kernel of the multi-kernel path adds the priors beside the ODE kernel's
likelihood, and the run never calls the likelihood's host twin.  The data are those of examples/noise.

    python -m pydream_amd.examples.priors.priors_device [niterations] [nchains] [--host]

--host: the same run with the likelihood's host twin as a plain Python callable (run_dream's host path: priors through scipy).
"""
import sys

import numpy as np

from pydream_amd.examples.noise import noise_device as NOISE
from pydream_amd.examples.robertson import robertson_device as ROB
from pydream_amd.likelihoods import MassActionODELogLike, Noise

SIGMA, REL = 3, 4                                         # the coordinates of the noise model
TRUE = np.r_[10.0 ** ROB.NOMINAL, 0.004, 0.03]            # the point the data were simulated from (examples/noise)
TSPAN = NOISE.TSPAN


def make_likelihood(data=None, **kw):
    data = NOISE.simulated_data() if data is None else np.asarray(data, dtype=float)
    return MassActionODELogLike(3, ROB.REACTIONS, ROB.Y0, TSPAN, [[0, 0, 1]], data[None, :], None, rate_scale="linear",
                                noise=[Noise(SIGMA, rel=REL)], **kw)


def make_parameters():
    from scipy.stats import halfcauchy, halfnorm, lognorm
    from pydream_amd.parameters import SampledParam
    return [SampledParam(lognorm, 0.5, scale=TRUE[:3]), SampledParam(halfnorm, scale=0.02), SampledParam(halfcauchy, scale=0.1)]


def starts(nchains, seed=31):
    rng = np.random.default_rng(seed)
    return [TRUE * np.exp(0.2 * rng.uniform(-1, 1, len(TRUE))) for _ in range(nchains)]


def main(niterations=300, nchains=64, host=False, like=None):
    from pydream_amd import core
    like = make_likelihood() if like is None else like
    sampled, log_ps = core.run_dream(make_parameters(), NOISE.HostTwin(like) if host else like, niterations=niterations, nchains=nchains, multitry=5,
                                     start=starts(nchains), model_name="priors_device", verbose=False, save_history=False, seed=32,
                                     nseedchains=max(10 * len(TRUE), 2 * nchains))
    S, L = np.concatenate(sampled), np.concatenate(log_ps)
    best = S[np.argmax(L)]
    print("log-normal, half-normal and half-Cauchy priors on %s: %d chains x %d iterations; best log p %.3f at [k1, k2, k3, sigma, rel] = %s (true %s)"
          % ("the host twin" if host else "the device", nchains, niterations, L.max(), np.array2string(best, precision=4), np.array2string(TRUE, precision=4)))
    print("last_kernel_variant: %s" % core.last_kernel_variant)
    return sampled, log_ps


if __name__ == "__main__":
    argv = [a for a in sys.argv[1:] if a != "--host"]
    main(*(int(a) for a in argv[:2]), host="--host" in sys.argv[1:])
