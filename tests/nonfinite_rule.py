"""What the sampler decides when a log density is NaN, +inf or -inf: Dream.py:279-334 and metrop_select (:980-998) restated literally in
Python floats -- sequential sums in try order, oracle.exp / oracle.log for the elementary functions, so that every result is comparable bit
for bit with the oracle's and the HIP engine's -- and the table of value classes the tests run it over.

    decide(k, lp, B, snooker, slp, slr, cur_snk, last_logp, u_sel, u_acc, amax) -> (sel, ratio, accept)

lp[i] = prior_i + T like_i of try i (:279); B[i] the same of reference point i, B[k-1] the current state's (:877-879, :303); slp, slr the
snooker terms of the proposal and reference sets (:307, :312-313); for k = 1 lp[0] is q_logp, last_logp and cur_snk the current state's terms
of :326-334.  The reference draws the selected try with np.random.multinomial, which RAISES on NaN probabilities; the engine's rule there is
its own: the first i with u_sel < cum_i, else k-1 -- with NaN probabilities no comparison holds, so k-1.

amax: the maximum of :320 and :902 --
    "skip"       fmax: a NaN operand is skipped (the device's rowmax16)
    "propagate"  np.amax: any NaN makes the maximum NaN (the reference)
    "first"      `if (v > mx) mx = v` from slot 0: a NaN in slot 0 stays, elsewhere it is skipped (the oracle's loop)
tests/test_nonfinite_rule_cpu.py asserts that the three decide alike on every row of the table."""
import math
import sys

import numpy as np

INF, NAN = math.inf, math.nan
DBL_MAX = sys.float_info.max
V = (-INF, -DBL_MAX, -800.0, -1.5, 0.0, 700.0, DBL_MAX, INF, NAN)          # the value classes of every lp_i and B_i
V3 = (-INF, -1.5, 700.0, INF, NAN)                                        # ... of the k = 3 full product
U = (2.0 ** -53, 0.25, 0.5, 1.0 - 2.0 ** -53)                             # u_sel, u_acc
SNK1 = (0.0, -3.25, 12.5)                                                 # the single-try snooker terms
SNK = (0.0, -3.25, 12.5, -40.0, 3.0)                                      # the multi-try rows' (finite) snooker terms
SEEDED_K = (5, 16, 17, 24)
CONVENTIONS = ("skip", "propagate", "first")


def _elementary():
    from oracle import oracle as O
    return O.exp, O.log


def nan_to_num(x):
    """numpy.nan_to_num (:323, :332, :334)"""
    if x != x:
        return 0.0
    if x == INF:
        return DBL_MAX
    if x == -INF:
        return -DBL_MAX
    return x


def _div(a, b):
    """a / b in IEEE arithmetic (Python raises on a zero divisor)"""
    if b == 0.0:
        return NAN if (a != a or a == 0.0) else math.copysign(INF, a) * math.copysign(1.0, b)
    return a / b


def amax(vals, convention):
    if convention == "propagate":
        return NAN if any(v != v for v in vals) else max(vals)
    if convention == "first":
        m = vals[0]
        for v in vals[1:]:
            if v > m:
                m = v
        return m
    m = NAN                                                               # "skip": fmax(NaN, v) = v, fmax(m, NaN) = m
    for v in vals:
        if m != m or v > m:
            m = v if v == v else m
    return m


def select(k, lp, u_sel, convention="skip"):
    """mt_choose_proposal_pt (:883-917) with the engine's rule for the multinomial draw"""
    exp, _ = _elementary()
    mx = amax(list(lp[:k]), convention)                                   # :902
    w = [exp(lp[i] - mx) for i in range(k)]                               # :903
    S = 0.0
    for i in range(k):
        S = S + w[i]                                                      # :906
    cum = 0.0
    for i in range(k):
        cum = cum + _div(w[i], S)                                         # :907
        if u_sel < cum:
            return i
    return k - 1


def decide(k, lp, B, snooker, slp, slr, cur_snk, last_logp, u_sel, u_acc, convention="skip"):
    exp, log = _elementary()
    if k == 1:
        q_logp = lp[0]
        if snooker:
            ratio = nan_to_num((q_logp + slp[0]) - (last_logp + cur_snk))                      # :326-332
        else:
            ratio = nan_to_num(q_logp) - nan_to_num(last_logp)                                 # :334
        sel = 0
    else:
        sel = select(k, lp, u_sel, convention)                                                 # :291
        if snooker:                                                                            # :306-313
            A = [lp[i] + slp[i] for i in range(k)]
            Bt = [(B[i] + (slr[i] if i < k - 1 else 0.0)) + slp[i] for i in range(k)]
        else:
            A, Bt = list(lp[:k]), list(B[:k])
        m2 = amax(A + Bt, convention)                                                          # :320
        SA = SB = 0.0
        for i in range(k):
            SA = SA + exp(A[i] - m2)                                                           # :321
        for i in range(k):
            SB = SB + exp(Bt[i] - m2)                                                          # :322
        ratio = nan_to_num(log(_div(SA, SB)))                                                  # :323
    accept = math.isfinite(ratio) and log(u_acc) < ratio                                       # :993
    return sel, ratio, bool(accept)


# ------------------------------------------------------------------------------------------------------------------------ the table
class Rows:
    """n rows of one try count: lp[n, k], B[n, k] (B[:, k-1]: the current state's log density, for k = 1 last_logp), snk[n], slp[n, k],
    slr[n, k] (column k-1 unused), cur[n] (k = 1: cur_snk), u_sel[n], u_acc[n]"""

    def __init__(self, k, lp, B, snk, slp, slr, cur, u_sel, u_acc):
        self.k, self.n = k, len(lp)
        self.lp, self.B, self.snk, self.slp, self.slr, self.cur, self.u_sel, self.u_acc = lp, B, snk, slp, slr, cur, u_sel, u_acc

    def decide(self, r, convention="skip"):
        k = self.k
        return decide(k, self.lp[r].tolist(), self.B[r].tolist(), bool(self.snk[r]), self.slp[r].tolist(), self.slr[r].tolist(), float(self.cur[r]),
                      float(self.B[r, k - 1]), float(self.u_sel[r]), float(self.u_acc[r]), convention)

    def decide_all(self, convention="skip"):
        """-> sel[n] int, ratio[n] float, accept[n] bool"""
        out = [self.decide(r, convention) for r in range(self.n)]
        return np.array([o[0] for o in out]), np.array([o[1] for o in out]), np.array([o[2] for o in out])


def _product(values, m):
    g = np.meshgrid(*([np.array(values)] * m), indexing="ij")
    return np.stack([x.ravel() for x in g], axis=1)


def _finish(k, lp, B, rng):
    """u and the snooker half of a multi-try section: every second row a snooker row with finite terms"""
    n = len(lp)
    r = np.arange(n)
    u_sel, u_acc = np.array(U)[r % 4], np.array(U)[(r // 4) % 4]
    snk = (r % 2).astype(np.uint8)
    slp, slr = rng.choice(SNK, (n, k)), rng.choice(SNK, (n, k))
    slp[snk == 0] = 0.0; slr[snk == 0] = 0.0
    slr[:, k - 1] = 0.0
    return Rows(k, lp, B, snk, slp, slr, np.zeros(n), u_sel, u_acc)


_TABLE = {}


def table(k):
    """the rows of try count k in 1, 2, 3, 5, 16, 17, 24 (made once)"""
    if k in _TABLE:
        return _TABLE[k]
    rng = np.random.default_rng(7700 + k)
    if k == 1:          # q_logp x last_logp over V x V; plain, and snooker with (slp, cur_snk) over SNK1 x SNK1; every u_acc
        qv = _product(V, 2)
        terms = [(0, 0.0, 0.0)] + [(1, a, b) for a in SNK1 for b in SNK1]
        lp, B, snk, slp, cur, ua = [], [], [], [], [], []
        for s, a, b in terms:
            for u in U:
                lp.append(qv[:, :1]); B.append(qv[:, 1:]); snk.append(np.full(len(qv), s, np.uint8))
                slp.append(np.full((len(qv), 1), a)); cur.append(np.full(len(qv), b)); ua.append(np.full(len(qv), u))
        lp, B, snk, slp, cur, ua = (np.concatenate(x) for x in (lp, B, snk, slp, cur, ua))
        t = Rows(1, lp, B, snk, slp, np.zeros_like(slp), cur, np.full(len(lp), 0.5), ua)
    elif k == 2:        # the full product, 9^4 rows
        p = _product(V, 4)
        t = _finish(2, p[:, :2].copy(), p[:, 2:].copy(), rng)
    elif k == 3:        # the full product over V3, 5^6 rows
        p = _product(V3, 6)
        t = _finish(3, p[:, :3].copy(), p[:, 3:].copy(), rng)
    else:               # 4096 rows drawn from V: each row from a palette of 1, 2, 3 or all 9 classes (all 9 alone would leave a NaN in
        n = 4096        # nearly every row of 16 and more tries, and NaN decides those rows whatever else they hold)
        vals = np.array(V)
        lp, B = np.empty((n, k)), np.empty((n, k))
        for r in range(n):
            m = (1, 2, 3, 9)[r % 4]
            pal = rng.choice(9, m, replace=False)
            palB = rng.choice(9, m, replace=False) if (r // 4) % 2 else pal     # (its own palette: rows whose sums divide to 0 or inf)
            lp[r] = vals[rng.choice(pal, k)]; B[r] = vals[rng.choice(palB, k)]
        u = np.array(U)
        t = _finish(k, lp, B, rng)
        t.u_sel, t.u_acc = u[rng.integers(0, 4, n)], u[rng.integers(0, 4, n)]
    _TABLE[k] = t
    return t


def classes(a):
    """the index in V of every element of a"""
    a = np.asarray(a)
    out = np.full(a.shape, 8)
    for i, v in enumerate(V[:8]):
        out[a == v] = i
    return out


def bits(x):
    return np.asarray(x, dtype=np.float64).view(np.uint64)


# ------------------------------------------------------------------------------------------------------------ the poisoned samplers
# (tests/test_nonfinite_gpu.py part B runs them on the HIP engine and the oracle; tests/test_nonfinite_rule_cpu.py checks the oracle's runs alone)
KEYS = ("snooker", "cr_idx", "try_idx", "moved", "X", "logp")
BAND_CENTRES = (0.03, 0.09, 0.21)                                         # frac(x[0]) inside the NaN, +inf and -inf bands of MK.POISON_BANDS
POISON_VALUES = (NAN, INF, -INF)
OPEN_SUPPORT = (-10.0, 30.0)                                              # the open uniform prior's (loc, scale); the archive is U(-5, 15)
HUGE_ROWS = ((1e200, 0), (-1e200, 1), (1e308, 0), (-1e308, 2))            # (entry, column mod d) of the archive rows that make DE differences overflow


def module_config(**kw):
    """a user-kernel (tests/module_kernels.py) sampler with the poison bands"""
    c = dict(kind="module", lk="thread", items=1, d=6, N=64, k=3, n=24, prior="flat", snooker=0.1, thin=5, lag=0, ncr=3, adapt_cr=1, burnin=9,
             seed=4100, steps=None)
    c.update(kw)
    if c["lk"] == "items" and c["items"] == 1:
        c["items"] = 3
    return c


def builtin_config(**kw):
    """a built-in density (MVN by its triangular factor or dense matrix, mixture) poisoned through the initial state and the archive"""
    c = dict(kind="mvn", tri=1, d=7, N=3073, k=5, n=24, prior="flat", snooker=0.5, thin=10, lag=0, ncr=3, adapt_cr=0, burnin=0, seed=5100,
             steps=None, archive=1, env={})
    c.update(kw)
    return c


def _start_values(c, X0, true_like):
    """the chains' start log densities: chains 0, 1, 2 of every nine hold NaN, +inf, -inf"""
    like = np.array(true_like, dtype=float)
    for v in range(3):
        like[v::9] = POISON_VALUES[v]
    return like


def build_sampler(Cls, c):
    """-> engine, start log densities (prior0 + like0): the same inputs to the HIP engine and the oracle"""
    from tests import module_kernels as MK
    from tests import helpers as H
    oracle = Cls.__module__.startswith("oracle")
    d, N, k, n = c["d"], c["N"], c["k"], c["n"]
    rng = np.random.default_rng(c["seed"])
    M0 = max(10 * d, 2 * N if c["kind"] == "module" else 64) + 7
    Z0 = rng.uniform(-5.0, 15.0, (M0, d))
    X0 = rng.uniform(-5.0, 15.0, (N, d))
    open_prior = c["prior"] == "uniform_open"
    e = Cls(nchains=N, ndim=d, multitry=k, ncr=c["ncr"], history_thin=c["thin"], history_lag=c["lag"], crossover_burnin=c["burnin"],
            adapt_crossover=c["adapt_cr"], hardboundaries=0 if open_prior else 1, history_capacity=M0 + N * (n // c["thin"] + 2), trace_capacity=n,
            seed=c["seed"], snooker=c["snooker"], **({"schedule": 2} if oracle else {}))
    e.set_gamma_table(np.array([[2.38 / np.sqrt(2.0 * np.arange(1, d + 1))]]))
    prior0 = np.zeros(N)
    if open_prior:
        e.set_prior(np.full(d, 2, np.int32), np.full(d, OPEN_SUPPORT[0]), np.full(d, OPEN_SUPPORT[1]))      # (no boundaries: proposals leave it)
        prior0 = np.full(N, -np.log(OPEN_SUPPORT[1]) * d)
    if c["kind"] == "module":
        # a third of the chains start inside the bands: chain i < N/3 in band i mod 3 -- the twin's UNMAPPED values seed the state
        third = np.arange(N // 3)
        X0[third, 0] = np.floor(X0[third, 0]) + np.array(BAND_CENTRES)[third % 3]
        MK.apply(e, c["lk"], d, np.inf, c["items"], oracle=oracle, poison=MK.POISON_BANDS)
        like0 = MK.twin(c["lk"], d, np.inf, c["items"], MK.POISON_BANDS)(X0)[1]
    else:
        from oracle import oracle as O
        if c["archive"]:
            for r, (v, j) in enumerate(HUGE_ROWS):
                Z0[3 + 5 * r, j % d] = v
        if c["kind"] == "mvn":
            P = H.mvn_precision(d)
            e.set_likelihood_mvn(np.zeros(d), H.tri_factor(P) if c["tri"] else P, 1 if c["tri"] else 0, 0.0)
        else:
            mu = np.array([np.full(d, m) for m in (-4.0, 1.0, 6.0)])
            e.set_likelihood_mixture(mu, np.log(np.arange(1, 4) / 6.0) - (d / 2.) * np.log(2 * np.pi))
        key = (c["kind"], c["tri"], d, N, c["seed"])
        if key not in _TRUE_LIKE:                                         # the density's own values at the start states, from the oracle (made once)
            o = e if oracle else build_sampler(O.Engine, c)[0]
            _TRUE_LIKE[key] = np.array([o.loglike(x) for x in X0])
            if o is not e:
                o.close()
        like0 = _start_values(c, X0, _TRUE_LIKE[key])
    e.set_history(Z0)
    e.set_state(X0, prior0, like0)
    return e, prior0 + like0


_TRUE_LIKE = {}


def run_sampler(Cls, c):
    """-> dict(trace, Z, cr, state, start, variants, tries, redraws)"""
    import os
    hip = not Cls.__module__.startswith("oracle")
    saved = {name: os.environ.get(name) for name in c.get("env", {})}
    try:
        if hip:
            os.environ.update(c.get("env", {}))
        e, start = build_sampler(Cls, c)
        variants, tries = [], []
        for m in c["steps"] or (c["n"] // 2, c["n"] - c["n"] // 2):
            e.step(m)
            if hip:
                variants.append(e.last_kernel_variant()); tries.append(e.last_kernel_tries())
        out = dict(trace=e.get_trace(0, c["n"]), Z=e.get_history(), cr=e.get_cr_state(), state=e.get_state(), start=start, variants=variants, tries=tries,
                   redraws=e.redraw_rounds() if hip else None)
        e.close()
    finally:
        for name, v in saved.items():
            if v is None:
                os.environ.pop(name, None)
            else:
                os.environ[name] = v
    return out


def starts(run):
    """[n, N]: the log density every chain-generation started from"""
    return np.concatenate([run["start"][None, :], run["trace"]["logp"][:-1]])


def assert_same(a, b):
    for key in KEYS:
        np.testing.assert_array_equal(a["trace"][key], b["trace"][key], err_msg=key)
    np.testing.assert_array_equal(a["Z"], b["Z"])
    for u, v in zip(a["cr"], b["cr"]):
        np.testing.assert_array_equal(u, v)
    for u, v in zip(a["state"], b["state"]):
        np.testing.assert_array_equal(u, v)


_ORACLE_RUNS = {}


def oracle_run(c):
    """the oracle's run of c, made once per configuration"""
    from oracle import oracle as O
    key = repr(sorted((k, repr(v)) for k, v in c.items() if k != "env"))
    if key not in _ORACLE_RUNS:
        _ORACLE_RUNS[key] = run_sampler(O.Engine, c)
    return _ORACLE_RUNS[key]


MODULE_SHAPES = ("thread", "wave", "group16", "group32", "items")
# (two tries are refused by both engines -- deviation D4, the reference raises at Dream.py:867-868 -- so the k = 2 rows exist in part A only)
MODULE_CASES = [(lk, k, prior, snk) for lk in MODULE_SHAPES for k in (1, 3, 5, 17) for prior in ("flat", "uniform_open") for snk in (0.1, 0.5)]


def module_case(lk, k, prior, snk):
    return module_config(lk=lk, k=k, prior=prior, snooker=snk, N=64, d=6 + MODULE_SHAPES.index(lk), seed=4100 + 17 * k + MODULE_SHAPES.index(lk))


# `function` (a DeviceFunctionLogLike): with the bands it no longer promises a finite density, so multi-try runs take the multi-kernel path; a
# single try has no redraw rounds whatever the promise and stays in the persistent kernel k_generations_user
FUNCTION_CASES = {"multi-kernel path": module_config(lk="function", k=3, N=64, d=11, seed=4301),
                  "k_generations_user": module_config(lk="function", k=1, N=192, d=8, n=30, seed=4302, snooker=0.5),
                  "k_generations_user<full>": module_config(lk="function", k=1, N=192, d=9, n=30, seed=4303, prior="uniform_open")}

# the persistent built-in kernels, by the copy of the rule they hold: name -> (configuration, what last_kernel_variant() must say, last_kernel_tries())
BUILTIN_CASES = {
    "k_generations, run-time k": (builtin_config(k=4, seed=5101), "k_generations<1,tri,xlds,16,1,lean>", 0),
    "k_generations, multitry-5 KC": (builtin_config(k=5, seed=5102), "k_generations<1,tri,xlds,16,1,lean>", 5),
    "k_generations, dense": (builtin_config(k=3, tri=0, seed=5103), "k_generations<1,dense,", 0),
    "k_generations, single try": (builtin_config(k=1, seed=5104), "k_generations<1,tri,xlds,16,1,lean,k1>", 0),
    "k_generations, REDO": (builtin_config(k=3, N=2048, prior="uniform_open", seed=5105), ",full,redo>", 0),
    "k_generations_w4": (builtin_config(k=5, N=300, seed=5106), "k_generations_w4<1,", 0),
    "k_generations_d2": (builtin_config(k=5, N=1025, d=132, seed=5107), "k_generations_d2<9,", 0),
    "k_generations_d2, 17 tries": (builtin_config(k=17, N=1100, d=48, seed=5108), "k_generations_d2<3,", 0),
    "k_generations_d2, single try": (builtin_config(k=1, N=1025, d=132, seed=5109, thin=3), "k_generations_d2<9,", 0),
    "k_generations_mix": (builtin_config(kind="mix", k=5, N=512, d=10, seed=5110), "k_generations_mix", 0),
    "k_generations_mix, single try": (builtin_config(kind="mix", k=1, N=512, d=10, seed=5111, thin=3), "k_generations_mix", 0),
}
