#!/usr/bin/env python3
"""What the extended device priors buy: the model of pydream_amd/examples/priors (the Robertson network with rate_scale="linear", log-normal priors
on the rate constants, a half-normal on the additive noise, a half-Cauchy on the proportional part) through run_dream, as proposals per second.

    python tools/prior_ext_rate.py [niterations] [nchains] [--tree DIR]

--tree DIR: import pydream_amd from another checkout (a built one).  At a commit without SampledParam.device_prior_ext the same call takes run_dream's
host path -- priors through scipy, the likelihood through its host twin --; with it, prior and likelihood stay on the device.  The model is stated here
and not imported from the example, so that the tool runs against either tree.  Prints one JSON line.
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
argv = sys.argv[1:]
TREE = os.path.abspath(argv[argv.index("--tree") + 1]) if "--tree" in argv else ROOT
if "--tree" in argv:
    del argv[argv.index("--tree"):argv.index("--tree") + 2]
sys.path.insert(0, TREE)


def main(niterations=200, nchains=64, multitry=5):
    from scipy.stats import halfcauchy, halfnorm, lognorm
    from pydream_amd import core
    from pydream_amd.examples.noise import noise_device as NOISE
    from pydream_amd.examples.robertson import robertson_device as ROB
    from pydream_amd.likelihoods import MassActionODELogLike, Noise
    from pydream_amd.parameters import SampledParam
    true = np.r_[10.0 ** ROB.NOMINAL, 0.004, 0.03]
    like = MassActionODELogLike(3, ROB.REACTIONS, ROB.Y0, NOISE.TSPAN, [[0, 0, 1]], NOISE.simulated_data()[None, :], None, rate_scale="linear",
                                noise=[Noise(3, rel=4)])
    params = [SampledParam(lognorm, 0.5, scale=true[:3]), SampledParam(halfnorm, scale=0.02), SampledParam(halfcauchy, scale=0.1)]
    rng = np.random.default_rng(31)
    starts = [true * np.exp(0.2 * rng.uniform(-1, 1, len(true))) for _ in range(nchains)]

    def run(n, seed):
        t = time.time()
        core.run_dream(params, like, niterations=n, nchains=nchains, multitry=multitry, start=starts, model_name="prior_ext_rate", verbose=False,
                       save_history=False, seed=seed, nseedchains=max(10 * len(true), 2 * nchains))
        return time.time() - t
    run(10, 1)                                  # builds and loads the likelihood's code object and its host build
    dt = run(niterations, 2)
    device = hasattr(params[0], "device_prior_ext")
    print(json.dumps(dict(tree=os.path.relpath(TREE, ROOT), path="device" if device else "host", kernel_variant=core.last_kernel_variant, chains=nchains,
                          iterations=niterations, multitry=multitry, seconds=round(dt, 4),
                          proposals_per_s=round(nchains * multitry * niterations / dt, 1))), flush=True)      # bench.py's convention: multitry proposals per chain and generation


if __name__ == "__main__":
    main(*(int(a) for a in argv[:2]))
