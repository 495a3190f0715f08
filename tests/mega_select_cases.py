"""The configurations behind tests/golden/mega_selection.json: what the persistent generation kernels' selection (pydream_amd/csrc/dz_mega_select.h)
was recorded at on the parent commit, by tests/golden/record_mega_selection.py, and what tests/test_mega_select_cpu.py and _gpu.py hold it to.

A case is a tests/fuzz_parity.py configuration (what F.build takes) plus `env`, the engine switches set while the engine is made.  Three priors
F.build does not know are set here behind it: "bounds" (hard boundaries, no prior), "uniform_partial" (a uniform prior whose support does NOT
contain the boundaries' box: proposal sets can be impossible, redraw rounds) and, for the user function, finite = 0 on "function" (a
DeviceFunctionLogLike without always_finite).

Every case is stepped in the pieces PIECES (history thin 5, crossover burn-in 3 where the adaptation is on):
  generation 0         -- burn-in where the adaptation is on; ends with an append
  generations 1..3     -- burn-in launches (one each, or up to adapt_lag + 1 per launch)
  generations 4..5     -- behind the burn-in, ends with the append of generation 5
  generations 6..9     -- behind the burn-in, no append
  generations 10..20   -- history lag >= 1 only: the launch 11..20 holds the append of 15 in its middle
The list is designed, not a cross product: every branch of the selection at the smallest shapes that reach it."""
import numpy as np

from tests import fuzz_parity as F
from tests import module_kernels as MK

THIN, BURNIN = 5, 3
SWITCHES = ("DZ_MEGA", "DZ_MEGA_D2", "DZ_MEGA_KC", "DZ_MEGA_REDO", "DZ_MEGA_USER", "DZ_ADAPT_FUSED", "DZ_ADAPT_MULTI", "DZ_MEGA_SEGS")


def pieces(c):
    return (1, 3, 2, 4) + ((11,) if c["lag"] else ())


def case(**kw):
    c = dict(lk="mvn_tri", d=16, N=4096, k=5, depairs=1, prior="flat", adapt=0, adapt_lag=0, lag=0, pt=0, J=3, items=1, finite=1, env={}, refused=0)
    c.update(kw)
    return c


def config(c):
    """the F.build configuration of a case"""
    n = sum(pieces(c))
    return dict(d=c["d"], N=c["N"], k=c["k"], depairs=c["depairs"], ngamma=1, ncr=3, adapt_cr=c["adapt"], adapt_g=0, burnin=BURNIN, n=n, lk=c["lk"],
                items=c["items"], finite=c["finite"], prior=c["prior"], thin=THIN, lag=c["lag"], snooker=0.1, pgu=0.2, lamb=0.05, zeta=1e-12, zero_mean=1,
                J=c["J"], extra_rows=7, seed=4242, pt=c["pt"], world=1, s1=0, adapt_lag=c["adapt_lag"])


def build(Cls, c):
    """the engine of a case, made under its switches (read once, when the engine is made); a setter that refuses the case closes the engine"""
    import os
    saved = {s: os.environ.pop(s, None) for s in SWITCHES}
    os.environ.update(c["env"])
    made = []
    try:
        fc = config(c)
        d = c["d"]
        if c["lk"] == "function" and not c["finite"]:
            from pydream_amd.likelihoods import DeviceFunctionLogLike
            fc["lk"] = "mvn"          # (F.build sets a likelihood; the user function replaces it below)
        if c["lk"] in MK.SHAPES:
            MK.code_object(c["lk"])
        def make(**kw):
            made.append(Cls(**kw))
            return made[-1]
        make.__module__ = Cls.__module__          # (F.build asks whose engine it makes)
        e = F.build(make, fc, dict(trace_capacity=0))
        if c["lk"] == "function" and not c["finite"]:
            DeviceFunctionLogLike(MK.FUNCTION_SRC, "mk_function", d, data=MK.data_block(d), always_finite=False, path=MK.code_object("function")[0])._dz_apply(e)
        if c["prior"] == "bounds":
            e.set_bounds(np.full(d, -6.0), np.full(d, 16.0))
        elif c["prior"] == "uniform_partial":
            e.set_prior(np.full(d, 2, np.int32), np.full(d, -5.5), np.full(d, 35.5))
            e.set_bounds(np.full(d, -6.0), np.full(d, 16.0))
    except Exception:
        for m in made:
            m.close()
        raise
    finally:
        for s in SWITCHES:
            os.environ.pop(s, None)
            if saved[s] is not None:
                os.environ[s] = saved[s]
    return e


ADAPT = [(0, 0), (1, 0), (3, 0), (0, 3), (3, 3)]      # (adapt_lag, history_lag) with the adaptation on


def cases():
    out = []
    D = [2, 16, 100, 112, 113, 128, 129, 200, 228, 229, 256]
    K = [1, 3, 5, 6, 7, 8, 12, 13, 15, 16, 20, 24, 32]          # (multitry 2 is refused by dz_create)
    NS = [3, 48, 512, 1024, 1025, 2048, 3072, 3073, 4096, 5000]
    # the triangular factor at 4096 chains: every try count at five dimensions, five try counts at the others
    out += [case(d=d, k=k) for d in D for k in (K if d in (16, 100, 128, 200, 256) else (1, 3, 5, 8, 16))]
    # the dense matrix
    out += [case(lk="mvn", d=d, k=k) for d in D for k in (1, 5)] + [case(lk="mvn", d=d, k=k) for d in (100, 128) for k in (3, 8, 16)]
    # chain counts: block sizes by CU rounds, split generations, 4 x 4 waves, d2's 1024-chain threshold
    out += [case(d=d, k=k, N=n) for n in NS for d in (16, 100, 200) for k in (1, 5) if n != 4096]
    out += [case(d=100, k=k, N=n) for n in (1024, 1025, 3072, 5000) for k in (3, 6, 7, 8, 16)]
    out += [case(lk="mvn", d=d, k=5, N=n) for n in NS for d in (16, 100) if n != 4096]
    # bounds, priors, DE pairs
    PRI = ["bounds", "uniform", "uniform_partial", "uniform_open", "uniform_narrow", "normal"]
    out += [case(d=d, k=k, prior=pr) for pr in PRI for d in (16, 100, 200) for k in (1, 5)]
    out += [case(d=100, k=5, prior=pr, N=n) for pr in PRI for n in (1024, 3072, 5000)]
    out += [case(lk="mvn", d=d, k=5, prior=pr) for pr in PRI for d in (16, 100)]
    out += [case(d=d, k=k, depairs=dp) for dp in (2, 3) for d in (16, 100, 200) for k in (1, 5, 16)]
    # the adaptation: lag 0, 1, 3; history lag 0 and 3; the MG and the ring modes by block size, split, d2, two-pass, k = 1, dense
    SH = [dict(d=16), dict(d=100), dict(d=100, N=3072), dict(d=100, N=5000), dict(d=100, N=1024), dict(d=200), dict(d=240), dict(d=100, k=1),
          dict(d=128, lk="mvn"), dict(d=100, k=16)]
    out += [case(adapt=1, adapt_lag=al, lag=hl, **s) for s in SH for al, hl in ADAPT]
    out += [case(adapt=1, adapt_lag=al, prior="uniform", **s) for s in SH for al in (0, 1, 3)]
    out += [case(adapt=1, adapt_lag=al, prior="uniform_partial", d=d) for al in (0, 1) for d in (16, 100)]
    out += [case(lag=3, **s) for s in SH]
    out += [case(adapt=a, adapt_lag=al, pt=1, N=n, d=d) for a, al in ((0, 0), (1, 0)) for n, d in ((48, 16), (1024, 100))]      # (temperature swaps: adapt_lag 0 only)
    # the mixture
    out += [case(lk="mix", N=1024, d=d, J=J, k=k) for d in (2, 10, 128, 129, 256) for J in ((1, 3, 32) if d in (10, 129) else (3,)) for k in (1, 3, 5)]
    # what the issue's list holds and the engine refuses when it is made (multitry 2: dz_create; more than 32 components: dz_set_likelihood_mixture)
    out += [case(d=16, k=2, refused=1), case(d=200, k=2, refused=1), case(lk="mix", N=1024, d=10, k=2, refused=1), case(lk="mix", N=1024, d=10, J=33, refused=1)]
    out += [case(lk="mix", N=1024, d=d, k=k, prior="uniform") for d in (2, 10, 128, 129, 256) for k in (1, 5)]
    out += [case(lk="mix", N=1024, d=d, k=5, adapt=1, adapt_lag=al, lag=hl, prior=pr) for d in (10, 129) for al, hl in ADAPT for pr in ("flat", "uniform")]
    out += [case(lk="mix", N=1024, d=10, k=k, adapt=1, adapt_lag=al) for k in (1, 3) for al in (0, 1)]
    out += [case(lk="mix", N=1024, d=10, J=32, k=5, adapt=1, adapt_lag=al) for al in (0, 3)]
    out += [case(lk="mix", N=48, d=10, k=5, adapt=1, pt=1)]
    # user likelihoods: a device function with and without always_finite, a device kernel (no generation kernels), two items per point
    for lk, fin, items in (("function", 1, 1), ("function", 0, 1), ("thread", 1, 1), ("items", 1, 2)):
        out += [case(lk=lk, finite=fin, items=items, N=1024, d=d, k=k, prior=pr) for d in (10, 129) for k in (1, 5) for pr in ("flat", "uniform")]
        out += [case(lk=lk, finite=fin, items=items, N=1024, d=10, k=5, adapt=1, adapt_lag=al) for al in (0, 1)]
    # the switches, one at a time, on a configuration of every family
    REP = [dict(d=100), dict(d=113), dict(d=200, N=1024), dict(d=100, prior="uniform_partial"), dict(d=100, adapt=1, adapt_lag=1), dict(d=100, adapt=1),
           dict(d=100, lag=3), dict(lk="mix", N=1024, d=10, adapt=1, adapt_lag=1), dict(lk="function", N=1024, d=10)]
    for env in ({"DZ_MEGA": "0"}, {"DZ_MEGA_D2": "0"}, {"DZ_MEGA_KC": "0"}, {"DZ_MEGA_REDO": "0"}, {"DZ_MEGA_USER": "0"}, {"DZ_ADAPT_FUSED": "0"},
                {"DZ_ADAPT_MULTI": "0"}, {"DZ_MEGA_D2": "2"}, {"DZ_MEGA_SEGS": "1"}):
        out += [case(env=env, **s) for s in REP]
    seen, uniq = set(), []
    for c in out:
        key = repr(sorted((k, repr(v)) for k, v in c.items()))
        if key not in seen:
            seen.add(key)
            uniq.append(c)
    return uniq
