"""The repressilator on the device: a ring of three genes, each repressing the next (Elowitz & Leibler, Nature 403, 2000), as a
likelihood whose synthesis rates are HILL-REPRESSED (MassActionODELogLike with RateLaw and Hill) -- a rate law that is not mass action.

    gene i = 0, 1, 2, repressed by the protein of gene j = (i + 2) % 3:

        0 -> m_i            alpha K^2 / (K^2 + p_j^2)     repressed synthesis, Hill exponent n = 2
        0 -> m_i            alpha0                        the promoter's leak
        m_i -> 0            1                             (time in units of the mRNA's lifetime)
        m_i -> m_i + p_i    beta                          translation ...
        p_i -> 0            beta                          ... and protein decay: beta is the protein / mRNA rate ratio

Six species (mRNA and protein of three genes), 15 reactions, one Hill slot (K^2, shared by the three promoters), four sampled constants:

    theta = log10 [alpha, alpha0, K, beta]

the promoter strength, the leak, the repression threshold and the protein / mRNA rate ratio.  The three proteins are read at 24 times
in [1, 24] with sd 5 % + 0.05; a uniform prior one decade wide (+- 0.5) around the true point.  The data are simulated at the true point
TRUE with scipy's Radau on a right-hand side written out by hand.

    python -m pydream_amd.examples.repressilator.repressilator_device [niterations] [nchains] [--host]

--host: the same run with the likelihood's host twin as a plain Python callable (run_dream's host path), which gives the same bits.
"""
import sys

import numpy as np

from pydream_amd.likelihoods import Hill, MassActionODELogLike, RateLaw

GENES = 3
N_SPECIES = 2 * GENES
ALPHA, ALPHA0, K, BETA = range(4)
HILL_N = 2


def mrna(i):
    return i


def protein(i):
    return GENES + i


def _reactions():
    rx = []
    for i in range(GENES):
        j = (i + 2) % GENES
        rx += [({}, {mrna(i): 1}, RateLaw(ALPHA, [Hill(protein(j), K, HILL_N, "repression")])),
               ({}, {mrna(i): 1}, ALPHA0),
               ({mrna(i): 1}, {}, 1.0),
               ({mrna(i): 1}, {mrna(i): 1, protein(i): 1}, BETA),
               ({protein(i): 1}, {}, BETA)]
    return rx


REACTIONS = _reactions()
Y0 = np.array([0.0, 0.0, 0.0, 2.0, 1.0, 3.0])
TRUE = np.log10([20.0, 0.05, 1.5, 0.5])     # the point the data are simulated from
WIDTH = 0.5                                 # the prior box: TRUE +- WIDTH
TSPAN = np.linspace(1.0, 24.0, 24)
OBSERVABLES = np.eye(N_SPECIES)[GENES:]


def simulated_data(rtol=1e-11, atol=1e-13):
    """The three proteins at TSPAN for the true point, [3, T], by scipy's Radau."""
    from scipy.integrate import solve_ivp
    alpha, alpha0, k, beta = 10.0 ** TRUE

    def f(t, y):
        m, p = y[:GENES], y[GENES:]
        rep = np.roll(p, 1)                 # gene i is repressed by protein (i + 2) % 3
        return np.concatenate([alpha * k ** HILL_N / (k ** HILL_N + rep ** HILL_N) + alpha0 - m, beta * (m - p)])
    sol = solve_ivp(f, (0.0, TSPAN[-1]), Y0, method="Radau", t_eval=TSPAN, rtol=rtol, atol=atol)
    assert sol.success, sol.message
    return OBSERVABLES @ sol.y


def make_likelihood(data=None, sd=None, **kw):
    data = simulated_data() if data is None else np.asarray(data, dtype=float)
    sd = 0.05 * np.abs(data) + 0.05 if sd is None else np.broadcast_to(sd, data.shape)
    return MassActionODELogLike(N_SPECIES, REACTIONS, Y0, TSPAN, OBSERVABLES, data, sd, rate_scale="log10", **kw)


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
    rng = np.random.default_rng(21)
    starts = [TRUE + 0.5 * WIDTH * rng.uniform(-1, 1, len(TRUE)) for _ in range(nchains)]
    sampled, log_ps = run_dream([SampledParam(uniform, loc=TRUE - WIDTH, scale=2 * WIDTH)], HostTwin(like) if host else like,
                                niterations=niterations, nchains=nchains, multitry=5, start=starts, model_name="repressilator_device", verbose=False,
                                save_history=False, seed=22)
    S, L = np.concatenate(sampled), np.concatenate(log_ps)
    best = S[np.argmax(L)]
    print("repressilator on %s: %d chains x %d iterations; best log p %.3f at log10 [alpha, alpha0, K, beta] = %s (true %s)"
          % ("the host twin" if host else "the device", nchains, niterations, L.max(), np.round(best, 3), np.round(TRUE, 3)))
    return sampled, log_ps


if __name__ == "__main__":
    argv = [a for a in sys.argv[1:] if a != "--host"]
    main(*(int(a) for a in argv[:2]), host="--host" in sys.argv[1:])
