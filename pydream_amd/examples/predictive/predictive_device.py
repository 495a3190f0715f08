"""Checking a fit on the device: posterior-predictive bands for the dose-response model (examples/dose_response: one enzyme network
measured at six substrate doses).

The data are simulated from the nominal constants with the model's own noise (sd 4 % + 0.01).  A short run_dream samples the five log10
rate constants on the device; posterior_predictive then takes the second half of every chain, every fifth row, and integrates each row
at each dose on a grid four times as dense as the measurement times -- MassActionODELogLike.with_outputs(t) and the prediction kernels
behind MassActionODELogLike.device(), points x doses work items per launch, where the host build would loop over them on one core.
What follows is numpy on the host: the 5 / 50 / 95 % bands of the trajectories per dose, the same bands with one noise replicate drawn
around every trajectory (the bands a new measurement should fall into), and the share of the data inside each.

    python -m pydream_amd.examples.predictive.predictive_device [niterations] [nchains] [--host]

--host simulates the rows with the host build instead (posterior_predictive(device=False)); the sampler is the same, and so are the
bands, bit for bit: both modes print the same digest.
"""
import hashlib
import sys

import numpy as np

from pydream_amd.examples.dose_response import dose_response_device as DR
from pydream_amd.likelihoods import posterior_predictive

SD_REL, SD_ABS = 0.04, 0.01
# the measurement times and three more between every two of them
DENSE_T = np.sort(np.r_[DR.TSPAN, (DR.TSPAN[:-1, None] + np.diff(DR.TSPAN)[:, None] * np.array([0.25, 0.5, 0.75])).reshape(-1)])
AT_DATA = np.searchsorted(DENSE_T, DR.TSPAN)


def noisy_data(seed=5):
    """(data, sd), [doses, 2, T]: the nominal trajectories with one draw of the model's noise"""
    clean = DR.simulated_data()
    sd = SD_REL * np.abs(clean) + SD_ABS
    return clean + sd * np.random.default_rng(seed).normal(size=clean.shape), sd


def make_likelihood(**kw):
    data, sd = noisy_data()
    return DR.make_likelihood(data=data, sd=sd, **kw)


def bands(sim):
    """the 5 / 50 / 95 % quantiles over the rows, [3, doses, T, O]"""
    return np.percentile(sim, [5, 50, 95], axis=0)


def coverage(b, data):
    """the share of the data (given as [doses, O, T]) between the 5 % and the 95 % band at the measurement times"""
    at = b[:, :, AT_DATA]
    d = data.transpose(0, 2, 1)
    return float(np.mean((d >= at[0]) & (d <= at[2])))


def main(niterations=200, nchains=64, host=False, seed=3):
    from scipy.stats import uniform
    from pydream_amd.core import run_dream
    from pydream_amd.parameters import SampledParam
    data, _ = noisy_data()
    like = make_likelihood()
    sampled, _ = run_dream([SampledParam(uniform, loc=DR.NOMINAL - 1, scale=2)], like, niterations=niterations, nchains=nchains, multitry=5,
                           model_name="predictive_device", verbose=False, save_history=False, seed=seed, nseedchains=max(10 * like.d, 2 * nchains))
    rows, sim = posterior_predictive(sampled, like, burnin=niterations // 2, thin=5, device=not host, t=DENSE_T)
    keep = np.all(np.isfinite(sim), axis=(1, 2, 3))              # (a row whose integration failed at some dose has NaN there)
    sim = sim[keep]
    replicate = sim + (SD_REL * np.abs(sim) + SD_ABS) * np.random.default_rng(seed + 1).normal(size=sim.shape)
    plain, noisy = bands(sim), bands(replicate)
    digest = hashlib.sha256(plain.tobytes() + noisy.tobytes()).hexdigest()[:16]
    print("posterior predictive on the %s: %d rows x %d doses x %d times (%d rows dropped); median P at t = %.1f by dose: %s"
          % ("host" if host else "device", len(sim), len(DR.DOSES), len(DENSE_T), int(np.sum(~keep)), DENSE_T[-1], np.round(plain[1, :, -1, 0], 3)))
    print("the 5-95 %% bands hold %.0f %% of the data without noise replicates and %.0f %% with them (nominal 90 %%); bands digest %s"
          % (100 * coverage(plain, data), 100 * coverage(noisy, data), digest))
    return rows, plain, noisy


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if a != "--host"]
    main(*(int(a) for a in args[:2]), host="--host" in sys.argv[1:])
