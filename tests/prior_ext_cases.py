"""The trajectory configurations tests/test_prior_ext_gpu.py runs on the engine and the oracle, and tests/test_prior_ext_cpu.py on the oracle alone:
8 chains, d = 6, the kinds 3 (laplace), 6 (lognorm), 7 (gamma, k = 1), 9 (halfnorm), 11 (truncnorm) and 1 (norm) mixed in one point.

The oracle knows no extended prior: its likelihood is a host callback whose prior column is filled from the host twin (_capi.prior_ext_host), so the
oracle's decisions are made on the twin's bits, and the engine -- device prior, the same likelihood -- must make the same ones."""
import numpy as np

INF = float("inf")
N, D, GENS = 8, 6, 60
KIND = np.array([3, 6, 7, 9, 11, 1], np.int32)
A = np.array([0.5, 0.1, 0.0, 0.25, 1.0, -1.0])
B = np.array([2.0, 1.5, 0.5, 2.0, 2.0, 3.0])
S1 = np.array([0.0, 0.7, 1.0, 0.0, -1.0, 0.0])
S2 = np.array([0.0, 0.0, 0.0, 0.0, 2.0, 0.0])
PRIOR = (KIND, A, B, S1, S2)
MINS = np.array([-INF, 0.1, 0.0, 0.25, -1.0, -INF])      # the supports, as Dream takes its hard boundaries from interval(1)
MAXS = np.array([INF, INF, INF, INF, 5.0, INF])
CENTRE = np.array([0.3, 1.2, 0.4, 1.0, 2.0, -0.5])
WEIGHT = np.array([1.0, 0.5, 4.0, 0.25, 0.5, 2.0])
SPREAD = 4.0       # how far beyond the supports the archive's rows reach (times the scale): what makes whole proposal sets impossible without boundaries


def like_rows(X):
    """a deterministic numpy likelihood: a diagonal Gaussian, the terms added left to right"""
    out = np.zeros(len(X))
    for j in range(D):
        t = X[:, j] - CENTRE[j]
        out = out - 0.5 * WEIGHT[j] * t * t
    return out


def archive(seed, rows=80):
    """the seed history: the first N rows inside every support (the chains start there), the rest spread beyond the lower ends"""
    rng = np.random.default_rng(seed)
    Z = CENTRE + B * rng.uniform(-SPREAD, SPREAD, (rows, D))
    lo = np.where(np.isfinite(MINS), MINS, -INF)
    hi = np.where(np.isfinite(MAXS), MAXS, INF)
    inside = np.clip(CENTRE + 0.2 * B * rng.uniform(-1, 1, (N, D)), lo + 0.05, hi - 0.05)
    Z[:N] = inside
    return Z


def make(Cls, k, hard, seed=77, likelihood=None):
    """an engine (pydream_amd._capi.Engine or oracle.Engine) ready to step GENS generations; the caller sets the prior and the likelihood"""
    Z0 = archive(seed)
    e = Cls(nchains=N, ndim=D, multitry=k, hardboundaries=1 if hard else 0, snooker=0.1, crossover_burnin=20, adapt_crossover=1, history_thin=5,
            history_capacity=len(Z0) + N * (GENS // 5 + 2), trace_capacity=GENS, seed=seed)
    if hard:
        e.set_bounds(MINS, MAXS)
    e.set_history(Z0)
    if likelihood is not None:
        likelihood(e)
    e.set_state(Z0[:N])
    return e


def oracle_callback(like=like_rows, sizes=None):
    """the oracle's host callback: the prior column from the host twin (NaN mapped to -inf, as the engine's kernel maps it), the likelihood beside it"""
    from pydream_amd import _capi

    def fn(X):
        if sizes is not None:
            sizes.append(len(X))
        pr = _capi.prior_ext_host(*PRIOR, X)
        return np.where(np.isnan(pr), -INF, pr), like(X)
    return fn


def engine_callback(like=like_rows):
    return lambda X: (np.zeros(len(X)), like(X))


def redrawn_fraction(sizes, k):
    """of the oracle's chain steps (one callback batch of k proposals, then one of k - 1 reference points), the fraction whose proposal set was drawn
    again at least once: every redraw round is one more batch of k in front of the step's reference batch"""
    steps = redrawn = run = 0
    for s in sizes:
        if s == k:
            run += 1
        elif s == k - 1 and run:
            steps += 1
            redrawn += run > 1
            run = 0
    return redrawn / steps
