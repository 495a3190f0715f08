"""A two-step activation cascade whose reporters are known only as a fraction of their own maximum, on the device: readouts
normalised to their own time course (MassActionODELogLike(normalize=[Normalize("max"), ...])) with unknown noise.

    R -> 0              kd      the stimulus decays
    A + R -> Ap + R     k1      the stimulus activates A
    Ap -> A             k2
    B + Ap -> Bp + Ap   k3      active A activates B
    Bp -> B             k4

Ap and Bp are read by two blots.  A blot has no absolute unit: each lane series is reported as a fraction of its own strongest band, so
the data are Ap(t) / max Ap and Bp(t) / max Bp, and nobody knows the noise of a relative readout in advance.  The likelihood normalises
the simulated trajectory the way the data were normalised -- no scale factor to sample, no prior to invent for one -- and samples the
two noise levels:

    theta = log10 [kd, k1, k2, k3, k4, sigma_A, sigma_B]

The maximum runs over every output row, observed or not: the blots were taken at ten times, and thirty more rows with NaN data sample
the peak more densely.  A uniform prior two decades wide around the nominal values.  The data are the host build's own normalised
simulation at the nominal values with one draw of the measurement error.  The run ends with posterior-predictive bands of the
normalised readouts.

    python -m pydream_amd.examples.normalized.normalized_device [niterations] [nchains] [--host]

--host: the same run with the likelihood's host twin as a plain Python callable (run_dream's host path) and the prediction by the host
build, which gives the same bits.
"""
import hashlib
import sys

import numpy as np

from pydream_amd.likelihoods import MassActionODELogLike, Noise, Normalize, posterior_predictive

R_, A, AP, B, BP = range(5)
KD, K1, K2, K3, K4, SIGMA_A, SIGMA_B = range(7)
REACTIONS = [({R_: 1}, {}, KD), ({A: 1, R_: 1}, {AP: 1, R_: 1}, K1), ({AP: 1}, {A: 1}, K2), ({B: 1, AP: 1}, {BP: 1, AP: 1}, K3), ({BP: 1}, {B: 1}, K4)]
Y0 = [1.0, 1.0, 0.0, 1.0, 0.0]
NOMINAL = np.log10([0.5, 3.0, 0.6, 2.0, 0.4, 0.05, 0.05])
WIDTH = 1.0
TSPAN = np.linspace(0.25, 10.0, 40)
OBSERVED = np.arange(3, 40, 4)                  # the ten rows the blots were taken at
OBSERVABLES = np.zeros((2, 5))
OBSERVABLES[0, AP] = OBSERVABLES[1, BP] = 1.0
NORMALIZE = [Normalize("max"), Normalize("max")]
NOISE = [Noise(SIGMA_A), Noise(SIGMA_B)]


def make_likelihood(data=None, **kw):
    data = simulated_data() if data is None else np.asarray(data, dtype=float)
    return MassActionODELogLike(5, REACTIONS, Y0, TSPAN, OBSERVABLES, data, 1.0, rate_scale="log10", normalize=NORMALIZE, noise=NOISE, **kw)


def simulated_data(seed=17):
    """The normalised readouts [2, T] at the nominal values (the host build's simulate of an object without data) with one draw of the
    measurement error at the observed rows; the other rows NaN."""
    clean = make_likelihood(data=np.full((2, len(TSPAN)), np.nan)).simulate(NOMINAL)[0].T
    rng = np.random.default_rng(seed)
    data = np.full(clean.shape, np.nan)
    sigma = 10.0 ** NOMINAL[[SIGMA_A, SIGMA_B]]
    data[:, OBSERVED] = clean[:, OBSERVED] + sigma[:, None] * rng.standard_normal((2, len(OBSERVED)))
    return data


class HostTwin:
    """The likelihood as a plain Python callable: run_dream takes the host path"""
    def __init__(self, like):
        self.like = like

    def __call__(self, x):
        return self.like(x)


def main(niterations=400, nchains=64, host=False, like=None, seed=47):
    from scipy.stats import uniform
    from pydream_amd.core import run_dream
    from pydream_amd.parameters import SampledParam
    like = make_likelihood() if like is None else like
    rng = np.random.default_rng(seed)
    starts = [NOMINAL + 0.25 * WIDTH * rng.uniform(-1, 1, len(NOMINAL)) for _ in range(nchains)]
    sampled, log_ps = run_dream([SampledParam(uniform, loc=NOMINAL - WIDTH, scale=2 * WIDTH)], HostTwin(like) if host else like,
                                niterations=niterations, nchains=nchains, multitry=5, start=starts, model_name="normalized_device", verbose=False,
                                save_history=False, seed=seed + 1, nseedchains=max(10 * like.d, 2 * nchains))
    S, L = np.concatenate(sampled), np.concatenate(log_ps)
    print("a cascade read as fractions of its own maxima on %s (two normalised reporters, unknown noise): %d chains x %d iterations; "
          "best log p %.3f at log10 [kd, k1, k2, k3, k4, sigma_A, sigma_B] = %s (true %s)"
          % ("the host twin" if host else "the device", nchains, niterations, L.max(), np.round(S[np.argmax(L)], 3), np.round(NOMINAL, 3)))
    rows, sim = posterior_predictive(sampled, like, burnin=niterations // 2, thin=5, device=not host)
    sim = sim[np.all(np.isfinite(sim), axis=(1, 2))]
    bands = np.percentile(sim, [5, 50, 95], axis=0)                     # [3, T, 2]: the normalised readouts
    print("posterior predictive on the %s: %d rows; median normalised Ap, Bp at t = %.2f: %s; bands digest %s"
          % ("host" if host else "device", len(sim), TSPAN[OBSERVED[2]], np.round(bands[1, OBSERVED[2]], 3), hashlib.sha256(bands.tobytes()).hexdigest()[:16]))
    return sampled, log_ps, bands


if __name__ == "__main__":
    argv = [a for a in sys.argv[1:] if a != "--host"]
    main(*(int(a) for a in argv[:2]), host="--host" in sys.argv[1:])
