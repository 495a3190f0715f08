"""What the tests of MassActionODELogLike share (a plain module: nothing here is collected): the code object's notes, the error against
reference solutions, the device's log densities of a batch, the check that the device gives the host build's bits, run_dream's own
sequence on the CPU oracle, and the check that run_dream on the device equals it."""
import os
import subprocess
from unittest import mock

import numpy as np

READELF = "/opt/rocm/lib/llvm/bin/llvm-readelf"


def notes(path):
    """registers, scratch and static LDS bytes of the code object's kernel (the one-lane and the lane-group tests had a copy each, the
    former without `lds`; a one-lane kernel has the field too, 0)"""
    txt = subprocess.run([READELF, "--notes", path], capture_output=True, text=True).stdout
    get = lambda key: int(txt.split(key)[1].split()[0])                     # noqa: E731
    return dict(vgpr=get(".vgpr_count:"), agpr=get(".agpr_count:"), scratch=get(".private_segment_fixed_size:"), lds=get(".group_segment_fixed_size:"))


def max_rel_err(like, refs, X, rtol):
    """max over points, times and observables of |sim - ref| / (rtol |ref| + rtol)"""
    sim = like.simulate(X)
    assert np.all(np.isfinite(sim))
    return max(float(np.max(np.abs(s - ref) / (rtol * np.abs(ref) + rtol))) for s, ref in zip(sim, refs))


def device_logp(like, X, lower, width):
    """(prior, likelihood) of the rows of X from the engine's eval_logp, under a uniform prior on [lower, lower + width]"""
    from pydream_amd import _capi
    d = X.shape[1]
    eng = _capi.Engine(nchains=3, ndim=d, history_capacity=8)
    eng.set_prior(np.full(d, 2, dtype=np.int32), np.asarray(lower, dtype=float), np.full(d, float(width)))
    like._dz_apply(eng)
    return eng.eval_logp(X)


def device_equals_host(like, X, nominal, width=1.0):
    """The device likelihood of the rows of X has the bytes of the host build's, and the uniform prior on nominal +- width is -inf exactly
    on the rows outside the box; returns the host build's values."""
    pr, lk = device_logp(like, X, nominal - width, 2 * width)
    host = like.batch(X)
    assert lk.tobytes() == host.tobytes()
    outside = np.any((X < nominal - width) | (X > nominal + width), axis=1)
    assert np.all(pr[outside] == -np.inf) and np.all(np.isfinite(pr[~outside]))
    return host


def oracle_run_dream(params, like, nchains, niterations, start, seed, **kwargs):
    """run_dream's own sequence (core.py) with the CPU oracle as the engine: the checker for API-level runs."""
    from oracle import oracle as O
    from pydream_amd.core import _sample_dream_batched, _setup_mp_dream_pool
    from pydream_amd.Dream import Dream
    from pydream_amd.model import Model
    restart = kwargs.pop("restart", False)
    if restart:
        mn = kwargs["model_name"]
        kwargs.update(history_file=mn + '_DREAM_chain_history.npy', crossover_file=mn + '_DREAM_chain_adapted_crossoverprob.npy',
                      gamma_file=mn + '_DREAM_chain_adapted_gammalevelprob.npy')
    step = Dream(model=Model(like, params), variables=params, verbose=False, **kwargs)
    pool = _setup_mp_dream_pool(nchains, niterations, step, start_pt=start, seed=seed, engine_cls=O.Engine)
    try:
        pool._initializer(*pool._initargs)
        step.save_history = False
        return _sample_dream_batched(pool.engine, step, niterations, False, 10)
    finally:
        pool.close(); pool.join()


def run_dream_equals_oracle(like, params, starts, seed, nchains, niterations, **kw):
    """run_dream with the device likelihood against its own sequence on the oracle with the host build as the Python likelihood (one
    host worker): every log probability finite, more distinct samples than chains, and both arrays equal."""
    from pydream_amd.core import run_dream
    sampled, log_ps = run_dream(params, like, nchains=nchains, niterations=niterations, verbose=False, start=starts, save_history=False, seed=seed, **kw)
    with mock.patch.dict(os.environ, DREAMZS_HOST_WORKERS="1"):
        o_s, o_l = oracle_run_dream(params, lambda x: like(x), nchains, niterations, starts, seed, **kw)
    S = np.concatenate(sampled)
    assert np.all(np.isfinite(np.concatenate(log_ps))) and len(np.unique(S[:, 0])) > nchains
    np.testing.assert_array_equal(np.array(sampled), np.array(o_s))
    np.testing.assert_array_equal(np.array(log_ps), np.array(o_l))
