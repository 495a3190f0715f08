"""A module driven by a MEASURED TIME COURSE, on the device: a two-tier phosphorylation cycle

    U + X -> U + Xp      k1 = 10**theta[0]       (the upstream kinase activity U phosphorylates X)
    Xp -> X              k2 = 10**theta[1]
    Xp + Y -> Xp + Yp    k3 = 10**theta[2]       (Xp phosphorylates Y)
    Yp -> Y              k4 = 10**theta[3]

whose upstream activity U(t) is not modelled but taken from a measurement, as one would read it off a blot: a pulse that rises, holds a
plateau and decays, given at ten times and interpolated linearly between them (MassActionODELogLike with inputs=[Input(U, times, values,
gain=4)]).  The blot's units are arbitrary, so its amplitude is sampled with the rate constants:

    theta = log10 [k1, k2, k3, k4, gain]

The experiment is done at three pulse amplitudes (half, once and twice the reference pulse), the three conditions of one likelihood; Xp and
Yp are read at 20 times each.  Inside the stiff solver the input is one more species whose right-hand side is the current segment's slope
and whose value is set exactly at every knot (csrc/dz_ode.h, INPUTS), so the whole likelihood stays on the GPU.  The data are simulated
from the nominal constants with seeded normal errors.  At the end posterior_predictive integrates rows of the chains on a denser grid
and prints the 5 / 50 / 95 % bands' digest.

    python -m pydream_amd.examples.input_drive.input_drive_device [niterations] [nchains] [--host]

--host: the same run with the likelihood's host twin as a plain Python callable (run_dream's host path) and the prediction by the host
build, which give the same bits and so the same bands.
"""
import hashlib
import sys

import numpy as np

from pydream_amd.likelihoods import Input, MassActionODELogLike, posterior_predictive

X, XP, Y, YP, U = range(5)
GAIN = 4                                    # the coordinate of the input's amplitude
REACTIONS = [({U: 1, X: 1}, {U: 1, XP: 1}, 0), ({XP: 1}, {X: 1}, 1), ({XP: 1, Y: 1}, {XP: 1, YP: 1}, 2), ({YP: 1}, {Y: 1}, 3)]
Y0 = [1.0, 0.0, 1.0, 0.0, 0.0]              # (the input species' entry is 0: its value comes from the table)
OBSERVABLES = [[0, 1, 0, 0, 0], [0, 0, 0, 1, 0]]
TSPAN = np.linspace(0.5, 10.0, 20)
DENSE_T = np.linspace(0.0, 10.0, 81)
# the measured upstream activity: basal, a rise, a plateau, a decay to nothing
PULSE_T = (0.0, 0.5, 1.0, 1.5, 2.0, 4.0, 5.0, 6.0, 7.5, 10.0)
PULSE_V = (0.05, 0.05, 0.40, 0.85, 1.00, 1.00, 0.60, 0.25, 0.0, 0.0)
AMPLITUDES = (0.5, 1.0, 2.0)
NOMINAL = np.log10([2.0, 0.8, 3.0, 0.5, 1.5])
WIDTH = 1.0                                 # the prior box: NOMINAL +- WIDTH
SD_REL, SD_ABS = 0.04, 0.01


def pulse(amplitude, gain=GAIN):
    return Input(U, PULSE_T, [amplitude * v for v in PULSE_V], gain=gain)


def make_likelihood(data=None, **kw):
    """data: [amplitudes, 2, T] (default: simulated_data())"""
    data = simulated_data() if data is None else np.asarray(data, dtype=float)
    conds = [dict(data=d, sd=SD_REL * np.abs(d) + SD_ABS, inputs=[pulse(a)]) for a, d in zip(AMPLITUDES, data)]
    return MassActionODELogLike(5, REACTIONS, Y0, TSPAN, OBSERVABLES, None, None, rate_scale="log10", conditions=conds, inputs=[pulse(1.0)], **kw)


def simulated_data(seed=7):
    """Xp and Yp at TSPAN under the three pulses at the nominal constants (the host build at a tight tolerance), with one draw of the
    measurement error"""
    blank = np.full((len(AMPLITUDES), 2, len(TSPAN)), np.nan)
    clean = make_likelihood(data=blank, rtol=1e-10, atol=1e-12, max_steps=20000).simulate(NOMINAL)[0].transpose(0, 2, 1)
    return clean + (SD_REL * np.abs(clean) + SD_ABS) * np.random.default_rng(seed).standard_normal(clean.shape)


class HostTwin:
    """The likelihood as a plain Python callable: run_dream takes the host path"""
    def __init__(self, like):
        self.like = like

    def __call__(self, x):
        return self.like(x)


def main(niterations=200, nchains=64, host=False, like=None, seed=41):
    from scipy.stats import uniform
    from pydream_amd.core import run_dream
    from pydream_amd.parameters import SampledParam
    like = make_likelihood() if like is None else like
    rng = np.random.default_rng(seed)
    starts = [NOMINAL + 0.25 * WIDTH * rng.uniform(-1, 1, len(NOMINAL)) for _ in range(nchains)]
    sampled, log_ps = run_dream([SampledParam(uniform, loc=NOMINAL - WIDTH, scale=2 * WIDTH)], HostTwin(like) if host else like,
                                niterations=niterations, nchains=nchains, multitry=5, start=starts, model_name="input_drive_device", verbose=False,
                                save_history=False, seed=seed + 1, nseedchains=max(10 * like.d, 2 * nchains))
    S, L = np.concatenate(sampled), np.concatenate(log_ps)
    print("a measured input on %s: %d chains x %d iterations; best log p %.3f at log10 [k1, k2, k3, k4, gain] = %s (true %s)"
          % ("the host twin" if host else "the device", nchains, niterations, L.max(), np.round(S[np.argmax(L)], 3), np.round(NOMINAL, 3)))
    rows, sim = posterior_predictive(sampled, like, burnin=niterations // 2, thin=5, device=not host, t=DENSE_T)
    sim = sim[np.all(np.isfinite(sim), axis=(1, 2, 3))]
    bands = np.percentile(sim, [5, 50, 95], axis=0)              # [3, amplitudes, T, O]
    print("posterior predictive on the %s: %d rows x %d amplitudes x %d times; median peak of Yp by amplitude: %s; bands digest %s"
          % ("host" if host else "device", len(sim), len(AMPLITUDES), len(DENSE_T), np.round(bands[1, :, :, 1].max(axis=1), 3),
             hashlib.sha256(bands.tobytes()).hexdigest()[:16]))
    return sampled, log_ps, bands


if __name__ == "__main__":
    argv = [a for a in sys.argv[1:] if a != "--host"]
    main(*(int(a) for a in argv[:2]), host="--host" in sys.argv[1:])
