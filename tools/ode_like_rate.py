#!/usr/bin/env python3
"""Rate of the device ODE likelihood (pydream_amd.likelihoods.MassActionODELogLike, csrc/dz_ode.h) on the Robertson network at
4096 chains x 5 tries over the example's prior box (nominal log10 rate constants +- 3):

  * the likelihood kernel alone: eval_logp on the 20 480 points of one generation -- us per launch, points/s;
  * steps per point (attempted Rodas4 steps, rejections included; from the host build, which takes the same steps) and lane efficiency,
    sum of steps / (64 x the wave's maximum) over the kernel's waves of 64 consecutive points;
  * run_dream generations/s with the likelihood on the device against the host path with 16 worker processes
    (DREAMZS_HOST_WORKERS=16), both for the host build of the same solver and for the reference example's odeint likelihood.

    python tools/ode_like_rate.py [chains] [tries] [generations] [--kernel-only]
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pydream_amd.examples.robertson import robertson_device as ROB      # noqa: E402


class HostOnly:
    """The likelihood as a plain Python callable: run_dream takes the host path"""
    def __init__(self, f):
        self.f = f

    def __call__(self, x):
        return self.f(x)


_DATA = None


def odeint_like(logk):
    """the reference example's likelihood (odeint, norm.logpdf) on the same data"""
    from scipy.integrate import odeint
    from scipy.stats import norm
    global _DATA
    if _DATA is None:
        _DATA = ROB.simulated_data()
    p1, p2, p3 = 10 ** np.asarray(logk, dtype=float)
    y = odeint(lambda y, t: [-p1 * y[0] + p3 * y[1] * y[2], p1 * y[0] - p3 * y[1] * y[2] - p2 * y[1] ** 2, p2 * y[1] ** 2], ROB.Y0, ROB.TSPAN)
    lp = float(np.sum(norm(loc=_DATA, scale=ROB.SD).logpdf(y[:, 2])))
    return lp if np.isfinite(lp) else -np.inf


def gens_per_s(like, N, k, G, host_workers=None):
    """generations/s of run_dream from the difference of a G-generation and a 2G-generation run (setup and compilation cancel)"""
    from scipy.stats import uniform
    from pydream_amd.core import run_dream
    from pydream_amd.parameters import SampledParam
    params = [SampledParam(uniform, loc=ROB.NOMINAL - 3, scale=6)]
    rng = np.random.default_rng(3)
    starts = [ROB.NOMINAL + 0.3 * rng.uniform(-1, 1, 3) for _ in range(N)]
    if host_workers is not None:
        os.environ["DREAMZS_HOST_WORKERS"] = str(host_workers)
    try:
        t = []
        for g in (G, 2 * G):
            t0 = time.perf_counter()
            run_dream(params, like, nchains=N, niterations=g, multitry=k, gamma_levels=4, adapt_gamma=True, history_thin=1, start=starts,
                      verbose=False, save_history=False, seed=7, parallel=host_workers is not None, nseedchains=2 * N)
            t.append(time.perf_counter() - t0)
    finally:
        os.environ.pop("DREAMZS_HOST_WORKERS", None)
    return G / max(t[1] - t[0], 1e-9)


def main(N=4096, k=5, G=20, kernel_only=False):
    from pydream_amd import _capi
    like = ROB.make_likelihood()
    n = N * k
    X = ROB.NOMINAL - 3 + 6 * np.random.default_rng(11).uniform(size=(n, 3))
    eng = _capi.Engine(nchains=N, ndim=3, multitry=k, history_capacity=8)
    eng.set_prior(np.full(3, 2, dtype=np.int32), ROB.NOMINAL - 3, np.full(3, 6.0))
    like._dz_apply(eng)
    for _ in range(3):
        eng.eval_logp(X)
    reps, t0 = 20, time.perf_counter()
    for _ in range(reps):
        pr, lk = eng.eval_logp(X)
    us = (time.perf_counter() - t0) / reps * 1e6
    host, steps = like.batch(X, return_steps=True)
    assert lk.tobytes() == host.tobytes(), "device and host builds differ"
    w = steps[: n // 64 * 64].reshape(-1, 64)
    out = dict(chains=N, tries=k, points=n, us_per_launch=round(us, 1), points_per_s=round(n / us * 1e6),
               steps_median=float(np.median(steps)), steps_max=int(steps.max()), lane_efficiency=round(float(w.sum() / (64 * w.max(axis=1)).sum()), 3),
               failed_points=int(np.sum(lk == -np.inf)))
    print(json.dumps(out), flush=True)
    if kernel_only:
        return out
    out["device_gens_per_s"] = round(gens_per_s(like, N, k, G), 2)
    print(json.dumps(out), flush=True)
    out["host_build_16w_gens_per_s"] = round(gens_per_s(HostOnly(like), N, k, 2, host_workers=16), 3)
    print(json.dumps(out), flush=True)
    out["odeint_16w_gens_per_s"] = round(gens_per_s(odeint_like, N, k, 1, host_workers=16), 3)
    out["speedup_vs_host_build"] = round(out["device_gens_per_s"] / out["host_build_16w_gens_per_s"], 1)
    out["speedup_vs_odeint"] = round(out["device_gens_per_s"] / out["odeint_16w_gens_per_s"], 1)
    print(json.dumps(out), flush=True)
    return out


if __name__ == "__main__":
    main(*(int(a) for a in sys.argv[1:4] if not a.startswith("--")), kernel_only="--kernel-only" in sys.argv)
