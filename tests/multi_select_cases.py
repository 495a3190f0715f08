"""The configurations behind tests/golden/multi_selection.json: what the multi-kernel path's selection (pydream_amd/csrc/dz_multi_select.h) was recorded
at on the parent commit, by tests/golden/record_multi_selection.py, and what tests/test_multi_select_cpu.py and _gpu.py hold it to.

A case is a case of tests/mega_select_cases.py (same `case`, `config`, `build`) whose `env` may also hold the switches of this path, plus
  range = (c0, nc): the case is stepped chain range by chain range (dz_step_range, what Dream.astep drives) instead of in lockstep.
Every case is stepped in the pieces of mega_select_cases.PIECES (history thin 5, crossover burn-in 3 where the adaptation is on): generation 0 | 1..3 |
4..5, which ends with the append of generation 5 | 6..9, four generations without an append: the first, the middle and the last of a deferred or fused chain.
The list is designed, not a cross product: every branch of logp_plan, generation_plan and redraw_plan at the smallest shape that reaches it.  Everything
at d <= 256 carries DZ_MEGA=0 unless something else keeps it off the persistent kernels (a host likelihood, a kernel of several items)."""
import os

from tests import mega_select_cases as MC

SWITCHES = ("DZ_PROPOSE_SPLIT", "DZ_QFIN", "DZ_LOGP_GEMM", "DZ_STREAMS")
OFF = {"DZ_MEGA": "0"}
pieces = MC.pieces


def case(**kw):
    c = MC.case(N=64, range=None)
    c.update(kw)
    if c["d"] <= 256:
        c["env"] = dict(OFF, **c["env"])
    return c


def brief(c):
    """what distinguishes a case from the default one (the fixture's key)"""
    base = case()
    return {k: (list(v) if isinstance(v, tuple) else v) for k, v in c.items() if base[k] != v}


def build(Cls, c):
    """MC.build under this path's switches as well (read once, when the engine is made)"""
    saved = {s: os.environ.pop(s, None) for s in SWITCHES}
    try:
        return MC.build(Cls, c)
    finally:
        for s in SWITCHES:
            os.environ.pop(s, None)
            if saved[s] is not None:
                os.environ[s] = saved[s]


def step(e, c, m):
    """one piece: m lockstep generations, or m single-range steps"""
    if c["range"] is None:
        e.step(m)
    else:
        for _ in range(m):
            e.step_range(*c["range"])


def cases():
    out = []
    # the LDS kernel: tries 1, 3, 5, both matrix forms; a prior behind it (not the single profiled launch); two DE pairs
    out += [case(lk=lk, k=k) for lk in ("mvn_tri", "mvn") for k in (1, 3, 5)]
    out += [case(prior=pr, k=k) for pr in ("normal", "uniform") for k in (1, 3)] + [case(depairs=2, k=3)]
    # the register MFMA kernel (the dense 128-D square does not fit LDS)
    out += [case(lk="mvn", d=128, k=k) for k in (1, 5)]
    # the tiled kernel; deferred row-tile sums on the per-chain proposal kernel (nch < 4, one stream); the GEMM kernel at its smallest tile
    out += [case(d=129, k=3), case(d=129, k=1), case(lk="mvn", d=200, k=3), case(d=129, k=5, N=128), case(d=129, k=5, N=128, prior="normal")]
    # nch = 4: streamed proposals, accept + propose fused up to 16 tries; nch = 8: one wave per try
    out += [case(d=300, k=k) for k in (1, 3, 5, 16, 20)] + [case(d=300, k=3, depairs=2)] + [case(d=520, k=k) for k in (1, 3, 5)]
    # the switches
    out += [case(k=3, env={"DZ_PROPOSE_SPLIT": "2"}), case(d=300, k=3, depairs=2, env={"DZ_PROPOSE_SPLIT": "8"}), case(d=129, k=3, env={"DZ_QFIN": "0"}),
            case(d=300, k=3, env={"DZ_QFIN": "0"}), case(d=129, k=5, N=128, env={"DZ_LOGP_GEMM": "0"})]
    out += [case(N=128, env={"DZ_STREAMS": "2"}, **s) for s in (dict(k=3), dict(d=129, k=3), dict(d=300, k=3), dict(k=3, adapt=1), dict(k=3, pt=1))]
    out += [case(N=100, k=3, env={"DZ_STREAMS": "2"})]          # (fewer than 64 chains per stream: one stream)
    # redraw rounds
    out += [case(prior="uniform_partial", k=3), case(prior="uniform_partial", k=3, d=300), case(prior="uniform_partial", k=3, N=128, env={"DZ_STREAMS": "2"})]
    # the mixture; user kernels: a thread, a lane group, a wave per point, two items per point, not always finite; the host callback
    out += [case(lk="mix", d=10, k=k) for k in (1, 5)]
    out += [case(lk=lk, d=10, k=k, items=2 if lk == "items" else 1) for lk in ("thread", "group16", "wave", "items") for k in (1, 3)]
    out += [case(lk="thread", d=10, k=3, finite=0), case(lk="items", items=2, d=10, k=3, N=128, env={"DZ_STREAMS": "2"}), case(lk="thread", d=300, k=3)]
    out += [case(lk="host", d=10, k=k) for k in (1, 3)]
    # the adaptation, lags (0, 0) and (1, 0); temperature swaps
    out += [case(k=3, adapt=1, adapt_lag=al, **s) for al in (0, 1) for s in (dict(), dict(d=300))] + [case(k=1, adapt=1)]
    out += [case(k=3, pt=1, adapt=a) for a in (0, 1)] + [case(d=300, k=3, pt=1)]
    # dz_step_range on one chain, and on two, with and without the adaptation
    out += [case(k=3, adapt=a, range=r) for a in (0, 1) for r in ((0, 1), (5, 2))] + [case(d=300, k=3, range=(0, 1))]
    # thresholds in CU rounds: 16-wave proposal blocks and a fifth LDS-kernel wave; two point tiles per MFMA wave; GEMM tiles of 64 and 128 points
    out += [case(N=4096, k=5), case(lk="mvn", d=128, N=4096, k=5), case(d=1000, N=1024, k=5), case(d=1000, N=2048, k=5)]
    return out
