#!/usr/bin/env python3
"""Rate of the device ODE likelihood (pydream_amd.likelihoods.MassActionODELogLike, csrc/dz_ode.h and csrc/dz_ode_group.h) at
4096 chains x 5 tries over a prior box around the nominal log10 rate constants (Robertson: +- 3, the example's; the others: +- 1):

  * the likelihood kernel alone: eval_logp on the 20 480 points of one generation -- us per launch, points/s;
  * steps per point (attempted Rodas4 steps, rejections included; from the host build, which takes the same steps) and lane efficiency,
    sum of steps / (points per wave x the wave's maximum) over the kernel's waves: 64 consecutive points with one lane per point,
    64 / lanes with a lane group per point;
  * run_dream generations/s with the likelihood on the device against the host path with 16 worker processes
    (DREAMZS_HOST_WORKERS=16), both for the host build of the same solver and (Robertson) for the reference example's odeint likelihood.

    python tools/ode_like_rate.py [chains] [tries] [generations] [--kernel-only] [--network robertson|mm|chain8|enzyme13|chain32|chain64|cascade|binding_cycle|<example>]
                                  [--lanes 1|16|32|64] [--conditions C [--events E | --equilibrate]] [--host-twin] [--noise] [--input] [--view]
                                  [--settle [--t-big T | --search-only] [--before CODE_OBJECT]]
                                  [--normalize max|ref|minmax [--before CODE_OBJECT]]

--conditions C: the network under C experimental conditions (MassActionODELogLike(conditions=...): the start amounts scaled by 0.5 .. 2,
geometrically) -- ONE launch over points x C items plus the engine's sum against the same C conditions as C single-condition launches
over the points (what the class could do before it took conditions), alternately, the median of 7 rounds of 10 calls each and the
rounds' spread; points/s, items/s, and lane efficiency over the waves of the combined launch (consecutive ITEMS).  Kernel only.

--conditions C --events E: what the restarts of dosing and wash-out events cost (MassActionODELogLike(events=...)) -- the network under C
conditions with E events in each (at equal distances inside the time span, on the species with the largest start amount: halved, then
topped up by half its start amount, in turn) against the same C conditions without events, alternately, the median of 7 rounds of 10
calls each and the rounds' spread; proposals/s and the host build's steps per point for both.  --events 0 times the event-less object
alone and never names the keyword (so the same script runs on a checkout from before the keyword existed).  Kernel only.

--conditions C --equilibrate: what equilibrating to the resting state before the experiment costs (MassActionODELogLike(equilibrate=
True)) -- the network under C conditions with the phase on in every condition against the same C conditions without it, alternately,
the median of 7 rounds of 10 calls each and the rounds' spread; proposals/s, the host build's steps per point for both and the phase's
attempted steps per item.  Kernel only.

--noise: what a sampled noise model costs (MassActionODELogLike(noise=...)) -- the network with a Noise(sigma, rel) on every observable,
sigma and rel two further coordinates (10**x, x in 0 +- 0.5 and -1 +- 0.5; the network's sd stays as the entries' weight), against the
same network without the keyword on the same rate constants, alternately, the median of 7 rounds of 10 calls each and the rounds'
spread; proposals/s and the host build's steps per point for both.  The per-entry cost is one dlog and a division at each of the T x O
entries of an integration.  Kernel only.

--input: what a piecewise-linear input time course costs (MassActionODELogLike(inputs=...)) -- --network drive2 | mm | enzyme13 | chain17 |
chain40 of tests/ode_input_networks.py, a network with an input species driven by its table (a pulse of six knots), against what could
be built before inputs existed: the same species and reactions with the input species a plain species fed by a fixed zero-order source,
a single ramp, on the same points; alternately, the median of 7 rounds of 10 calls each and the rounds' spread; proposals/s and the host
build's steps per point for both.  The work per step is the same; knots only add clipped steps.  Kernel only.

--view: what a view of the point per condition costs (MassActionODELogLike(conditions=[dict(params=...)]), csrc/dz_ode.h, VIEWS) --
--network mm | enzyme13 | chain17 | chain33 of tests/ode_view_networks.py (1, 16, 32 and 64 lanes per item) under 3 conditions whose
mappings are explicit identities {i: i} for every coordinate read, so the kernels gather every item's view and the values are the
same, against the same object without "params", on the same points; alternately, the median of 7 rounds of 10 calls each and the
rounds' spread; proposals/s for both, their registers, scratch and LDS from the code objects' notes, and the two launches' values
compared bit for bit (the host build's on the first 64 points).  Kernel only.

--settle: a steady output (MassActionODELogLike(t=[..., inf]), csrc/dz_ode.h, STEADY OUTPUT) against what a user did before t could
end in inf -- --network mm | enzyme13 | chain17 | chain33 of tests/ode_settle_networks.py (1, 16, 32 and 64 lanes per point) with its
last output at inf against the same network, data and points with a FINITE last output at t_last + t_big; alternately, the median of 7
rounds of 10 calls each and the rounds' spread; proposals/s and the host build's steps per point for both, their registers, scratch and
LDS from the code objects' notes, the phase's attempted steps, and how far the late output lies from the steady row.  t_big is chosen
with the reference (scipy's Radau, tests/ode_reference.py): the first power of ten at which Radau's state from the network's y0 passes
numpy's restatement of the steady-state test (the object's horizon and tolerances) at EVERY one of the timed points -- one Radau run per
point on the host (carried on from power to power, ended at the first that passes; about a second per point), before anything is timed,
over DREAMZS_HOST_WORKERS processes (default 16); --search-only does that search alone, needs no GPU and prints t_big and how many
points first rest at each power of ten; --t-big T skips the search and takes T, the value such a run found on the same points.
Kernel only.  The same run times the network WITHOUT the phase (t = [.., t_last]) in the same rounds, and with --before CODE_OBJECT also the
code object that another checkout -- the commit before the phase existed -- built for that network (MassActionODELogLike(path=...)):
networks without the phase generate the source they always did, so the two should take the same time within the rounds' spread.

--normalize KIND: what normalising the readouts to their own time course costs (MassActionODELogLike(normalize=...), csrc/dz_ode.h,
NORMALISED READOUTS) -- --network mm | enzyme13 | chain17 | chain33 (tests/ode_networks.py and tests/ode_equilibrate_networks.py; 1, 16, 32
and 64 lanes per point) with EVERY observable normalised by KIND ("ref": at the last output time) against the same network, data and
points without the keyword; alternately, the median of 7 rounds of 10 calls each and the rounds' spread; proposals/s for both, their
registers, scratch and LDS from the code objects' notes, and the values compared with the host build's bit for bit.  With --before
CODE_OBJECT also the code object that another checkout -- the commit before the keyword existed -- built for the plain network
(MassActionODELogLike(path=...)): a network without the keyword generates the source it always did, so the two should take the same
time within the rounds' spread.  The expected cost of normalising is a few registers and one divide per observable per point.  Kernel only.

--host-twin: the likelihood kernel against the host build of the same solver on the same points, for networks whose host pass is too
long to repeat (chain64, cascade: 0.02 .. 0.04 s per point) -- the device by the protocol above, the median of 7 rounds of 10 eval_logp
calls each and the rounds' spread; the host build ONCE, the points split over DREAMZS_HOST_WORKERS processes (default 16), each in one
call of batch(return_steps=True): that pass also gives the values the device's are compared with, bit for bit, and the steps.  Kernel only.

chain64: tests/ode_wide_networks' chain of 64 species, cascade: pydream_amd/examples/cascade (49 species), both a wave per point
(--lanes 64, their only shape).  --network chain32 --lanes 64 builds chain32 through the wave shape although the class refuses that
(half the wave idles): an internal build of this tool, to see what a whole wave per point costs where half a wave would do.

mm: tests/ode_networks' Michaelis-Menten network (4 species), imported from the test package like chain8, chain32: the chains of tests/ode_wide_networks.py, imported from the test package (run from a checkout; their data come from
scipy's Radau before anything is timed); chain8 runs with 1 lane per point and with 16, on the same points;
enzyme13: pydream_amd/examples/enzyme; binding_cycle: pydream_amd/examples/binding_cycle (monomials; 9 conditions per point, so a
launch covers points x 9 items and steps are counted over a point's nine integrations).  --lanes defaults to the fewest lanes the network fits in.
Any other name is an example of the package, pydream_amd/examples/<name>/<name>_device.py: its make_likelihood(), the box NOMINAL (or
TRUE, where the module has no NOMINAL) +- WIDTH (1.0 where it has none); --lanes goes to make_likelihood as lanes_per_point.
"""
import importlib
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


def network(name, lanes):
    """(likelihood, nominal, half width of the prior box)"""
    if name == "robertson":
        assert lanes in (None, 1), "robertson is the one-lane example"
        return ROB.make_likelihood(), ROB.NOMINAL, 3.0
    if name == "enzyme13":
        from pydream_amd.examples.enzyme import enzyme_device as ENZ
        return ENZ.make_likelihood(lanes_per_point=lanes or 16), ENZ.NOMINAL, 1.0
    if name == "binding_cycle":
        assert lanes in (None, 1), "binding_cycle is a one-lane example"
        from pydream_amd.examples.binding_cycle import binding_cycle_device as BC
        return BC.make_likelihood(), BC.NOMINAL, 1.0
    if name == "mm":
        assert lanes in (None, 1), "mm is a one-lane network"
        from tests import ode_networks as NW
        return NW.michaelis_menten(), NW.MM_NOMINAL, 1.0
    if name == "cascade":
        assert lanes in (None, 64), "cascade is a wave-per-point example"
        from pydream_amd.examples.cascade import cascade_device as CAS
        return CAS.make_likelihood(), CAS.NOMINAL, CAS.WIDTH
    if name not in ("chain8", "chain32", "chain64"):
        mod = importlib.import_module("pydream_amd.examples.%s.%s_device" % (name, name))
        like = mod.make_likelihood(**({} if lanes is None else dict(lanes_per_point=lanes)))
        return like, mod.NOMINAL if hasattr(mod, "NOMINAL") else mod.TRUE, getattr(mod, "WIDTH", 1.0)
    from tests import ode_wide_networks as W
    S = dict(chain8=8, chain32=32, chain64=64)[name]
    if S == 64:
        assert lanes in (None, 64), "chain64 needs a wave per point"
        return W.chain(64, 64), W.CHAIN_NOMINAL, 1.0
    if S == 32 and lanes == 64:                                 # (not through the constructor, which refuses it: see the head)
        like = W.chain(32, 32)
        like.lanes_per_point, like.path, like._host = 64, None, None
        return like, W.CHAIN_NOMINAL, 1.0
    if (lanes or (1 if S == 8 else 32)) == 1:                   # the same network and data through the one-lane kernel
        from pydream_amd.likelihoods import MassActionODELogLike
        grp = W.chain(S, 16)
        rx, y0, obs = W.chain_network(S)
        return MassActionODELogLike(S, rx, y0, W.CHAIN_T, obs, grp.data, grp.sd), W.CHAIN_NOMINAL, 1.0
    return W.chain(S, lanes or 32), W.CHAIN_NOMINAL, 1.0


def with_conditions(like, C):
    """(the network of `like` under C conditions, the C single-condition objects).  Every condition keeps the network's data: the steps a
    point takes depend on where it starts, not on what it is compared with."""
    from pydream_amd.likelihoods import MassActionODELogLike
    scales = [1.0] if C == 1 else [0.5 * 4.0 ** (c / (C - 1)) for c in range(C)]
    shared = dict(rate_scale=like.rate_scale, t0=like.t0, rtol=like.rtol, atol=like.atol, max_steps=like.max_steps, lanes_per_point=like.lanes_per_point)
    args = (like.n_species, like.reactions)
    multi = MassActionODELogLike(*args, None, like.t, like.observables, like.data, like.sd, conditions=[dict(y0=s * like.y0) for s in scales], **shared)
    return multi, [MassActionODELogLike(*args, s * like.y0, like.t, like.observables, like.data, like.sd, **shared) for s in scales]


def box_points(nominal, width, n):
    return nominal - width + 2 * width * np.random.default_rng(11).uniform(size=(n, len(nominal)))


def engine_for(like, N, k, nominal, width):
    """An engine of N chains x k tries with the box prior nominal +- width and the likelihood applied"""
    from pydream_amd import _capi
    d = len(nominal)
    eng = _capi.Engine(nchains=N, ndim=d, multitry=k, history_capacity=8)
    eng.set_prior(np.full(d, 2, dtype=np.int32), nominal - width, np.full(d, 2 * width))
    like._dz_apply(eng)
    return eng


def timed(calls, rounds=7, reps=10):
    """calls: {key: function}.  Three warm-up calls of each, then `rounds` rounds of `reps` timed calls of each, alternately (a drift of
    the machine hits all alike) -> ({key: the last warm-up's result}, {key: the rounds' microseconds per call})"""
    last, us = {}, {key: [] for key in calls}
    for _ in range(3):
        for key, f in calls.items():
            last[key] = f()
    for _ in range(rounds):
        for key, f in calls.items():
            t0 = time.perf_counter()
            for _ in range(reps):
                f()
            us[key].append((time.perf_counter() - t0) / reps * 1e6)
    return last, us


def conditions_rate(N, k, name, lanes, C, rounds=7, reps=10):
    like, nominal, width = network(name, lanes)
    multi, singles = with_conditions(like, C)
    n = N * k
    X = box_points(nominal, width, n)
    one, many = engine_for(multi, N, k, nominal, width), [engine_for(s, N, k, nominal, width) for s in singles]
    last, t = timed(dict(combined=lambda: one.eval_logp(X)[1], separate=lambda: [e.eval_logp(X)[1] for e in many]), rounds, reps)
    lk, parts = last["combined"], last["separate"]
    total = parts[0]
    for p in parts[1:]:
        total = total + p
    assert lk.tobytes() == total.tobytes() == multi.batch(X).tobytes(), "the combined launch, the separate launches and the host build differ"
    steps = np.stack([s.batch(X, return_steps=True)[1] for s in singles], axis=1).reshape(-1)       # item order: the condition fastest
    per_wave = 64 // like.lanes_per_point
    w = steps[: len(steps) // per_wave * per_wave].reshape(-1, per_wave)
    us, us_sep = float(np.median(t["combined"])), float(np.median(t["separate"]))
    out = dict(network=name, lanes=like.lanes_per_point, conditions=C, chains=N, tries=k, points=n, items=n * C, us_per_launch=round(us, 1),
               us_per_launch_min_max=[round(min(t["combined"]), 1), round(max(t["combined"]), 1)], points_per_s=round(n / us * 1e6),
               items_per_s=round(n * C / us * 1e6), lane_efficiency=round(float(w.sum() / (per_wave * np.maximum(w.max(axis=1), 1)).sum()), 3),
               steps_median=float(np.median(steps)), steps_max=int(steps.max()), failed_points=int(np.sum(lk == -np.inf)),
               separate_launches_us=round(us_sep, 1), separate_launches_us_min_max=[round(min(t["separate"]), 1), round(max(t["separate"]), 1)],
               separate_over_combined=round(us_sep / us, 3))
    print(json.dumps(out), flush=True)
    return out


def events_rate(N, k, name, lanes, C, E, rounds=7, reps=10, equilibrate=False):
    """E events per condition against none or (equilibrate) the phase on in every condition against off: see the head"""
    from pydream_amd.likelihoods import MassActionODELogLike
    like, nominal, width = network(name, lanes)
    plain, _ = with_conditions(like, C)
    first, second = ("without_phase", "with_phase") if equilibrate else ("without_events", "with_events")
    objs = {first: plain}
    shared = dict(rate_scale=like.rate_scale, t0=like.t0, rtol=like.rtol, atol=like.atol, max_steps=like.max_steps, lanes_per_point=like.lanes_per_point,
                  conditions=[dict(y0=c["y0"]) for c in plain.conditions])
    if equilibrate:
        objs[second] = MassActionODELogLike(like.n_species, like.reactions, None, like.t, like.observables, like.data, like.sd, equilibrate=True, **shared)
    elif E > 0:
        s = int(np.argmax(like.y0))
        span = like.t[-1] - like.t0
        events = [(like.t0 + (e + 1) * span / (E + 1), s, 0.5, 0.0) if e % 2 == 0 else (like.t0 + (e + 1) * span / (E + 1), s, 1.0, 0.5 * like.y0[s])
                  for e in range(E)]
        objs[second] = MassActionODELogLike(like.n_species, like.reactions, None, like.t, like.observables, like.data, like.sd, events=events, **shared)
    n = N * k
    X = box_points(nominal, width, n)
    engines = {key: engine_for(obj, N, k, nominal, width) for key, obj in objs.items()}
    last, t = timed({key: (lambda eng=eng: eng.eval_logp(X)[1]) for key, eng in engines.items()}, rounds, reps)
    out = dict(network=name, lanes=like.lanes_per_point, conditions=C, chains=N, tries=k, points=n, items=n * C,
               **(dict(equilibrate=True) if equilibrate else dict(events_per_condition=E)))
    for key, lk in last.items():
        host, steps = objs[key].batch(X, return_steps=True)
        assert lk.tobytes() == host.tobytes(), "device and host builds differ (%s)" % key
        out[key] = dict(steps_median=float(np.median(steps)), steps_max=int(steps.max()), failed_points=int(np.sum(lk == -np.inf)))
        if equilibrate and key == second:
            attempts = objs[key].steady_state(X, return_steps=True)[1]
            out[key].update(phase_attempts_median=float(np.median(attempts)), phase_attempts_max=int(attempts.max()))
    for key in engines:
        us = float(np.median(t[key]))
        out[key].update(us_per_launch=round(us, 1), us_per_launch_min_max=[round(min(t[key]), 1), round(max(t[key]), 1)], proposals_per_s=round(n / us * 1e6))
    if second in out:
        out["with_over_without"] = round(out[second]["us_per_launch"] / out[first]["us_per_launch"], 3)
    print(json.dumps(out), flush=True)
    return out


def noise_rate(N, k, name, lanes, rounds=7, reps=10):
    """A Noise(sigma, rel) on every observable against the network as it is: see the head"""
    from pydream_amd.likelihoods import MassActionODELogLike, Noise
    like, nominal, width = network(name, lanes)
    assert like.conditions is None and like.events is None and like.equilibrate is None and not like.y0_monomials and not like.constraints and like.scale is None
    d, n = like.d, N * k
    noisy = MassActionODELogLike(like.n_species, like.reactions, like.y0, like.t, like.observables, like.data, like.sd, rate_scale=like.rate_scale, t0=like.t0,
                                 rtol=like.rtol, atol=like.atol, max_steps=like.max_steps, lanes_per_point=like.lanes_per_point,
                                 noise=[Noise(d, rel=d + 1)] * len(like.observables))
    X = np.concatenate([box_points(nominal, width, n), box_points(np.array([0.0, -1.0]), 0.5, n)], axis=1)
    objs = dict(without_noise=(like, X[:, :d].copy()), with_noise=(noisy, X))
    engines = {}
    for key, (obj, pts) in objs.items():
        engines[key] = engine_for(obj, N, k, pts.mean(axis=0), 4.0)              # (a box that holds every point: the prior is not what is timed)
    last, t = timed({key: (lambda key=key: engines[key].eval_logp(objs[key][1])[1]) for key in objs}, rounds, reps)
    out = dict(network=name, lanes=like.lanes_per_point, species=like.n_species, observables=len(like.observables), times=len(like.t), chains=N, tries=k, points=n)
    for key, lk in last.items():
        host, steps = objs[key][0].batch(objs[key][1], return_steps=True)
        assert lk.tobytes() == host.tobytes(), "device and host builds differ (%s)" % key
        us = float(np.median(t[key]))
        out[key] = dict(steps_median=float(np.median(steps)), steps_max=int(steps.max()), failed_points=int(np.sum(lk == -np.inf)), us_per_launch=round(us, 1),
                        us_per_launch_min_max=[round(min(t[key]), 1), round(max(t[key]), 1)], proposals_per_s=round(n / us * 1e6))
    out["with_over_without"] = round(out["with_noise"]["us_per_launch"] / out["without_noise"]["us_per_launch"], 3)
    print(json.dumps(out), flush=True)
    return out


def input_rate(N, k, name, rounds=7, reps=10):
    """A network with an input against its emulation by a fixed zero-order source: see the head"""
    from tests import ode_input_networks as IN
    nominal = IN.network(name)["nominal"]
    objs = dict(emulated=IN.emulation(name), with_input=IN.single(name))
    import multiprocessing
    n = N * k
    X = box_points(nominal, 1.0, n)
    workers = int(os.environ.get("DREAMZS_HOST_WORKERS", "16"))
    hosts = {}
    for key, obj in objs.items():                                        # (the host passes first: their workers are forked before the device is opened)
        obj.host_library()
        with multiprocessing.get_context("fork").Pool(workers) as pool:
            parts = pool.map(_host_part, [(obj, part) for part in np.array_split(X, workers)])
        hosts[key] = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
    engines = {key: engine_for(obj, N, k, nominal, 1.0) for key, obj in objs.items()}
    last, t = timed({key: (lambda eng=eng: eng.eval_logp(X)[1]) for key, eng in engines.items()}, rounds, reps)
    like = objs["with_input"]
    out = dict(network=name + " + input", lanes=like.lanes_per_point, species=like.n_species, inputs=len(like.inputs),
               working_knots=len(like._input_knots(like.inputs)), chains=N, tries=k, points=n)
    for key, lk in last.items():
        host, steps = hosts[key]
        assert lk.tobytes() == host.tobytes(), "device and host builds differ (%s)" % key
        us = float(np.median(t[key]))
        out[key] = dict(steps_mean=round(float(np.mean(steps)), 1), steps_median=float(np.median(steps)), steps_max=int(steps.max()),
                        failed_points=int(np.sum(lk == -np.inf)), us_per_launch=round(us, 1),
                        us_per_launch_min_max=[round(min(t[key]), 1), round(max(t[key]), 1)], proposals_per_s=round(n / us * 1e6))
    out["with_over_emulated"] = round(out["with_input"]["us_per_launch"] / out["emulated"]["us_per_launch"], 3)
    print(json.dumps(out), flush=True)
    return out


def view_rate(N, k, name, rounds=7, reps=10):
    """Explicit identity views under 3 conditions against the same object without "params": see the head"""
    from tests import ode_view_networks as VN
    from tests.ode_support import notes
    values = (0.5, 1.0, 2.0) if name != "mm" else None
    objs = dict(without_view=VN.basic(name, view=False, identity=True, values=values)[0], with_view=VN.basic(name, identity=True, values=values)[0])
    like = objs["with_view"]
    assert len(like.conditions) == 3 and "VIEW" in like.source() and "VIEW" not in objs["without_view"].source()
    n, d = N * k, like.d
    nominal = VN.nominal_of(name)[:d]
    X = box_points(nominal, 1.0, n)
    engines = {key: engine_for(obj, N, k, nominal, 1.0) for key, obj in objs.items()}
    last, t = timed({key: (lambda eng=eng: eng.eval_logp(X)[1]) for key, eng in engines.items()}, rounds, reps)
    assert last["with_view"].tobytes() == last["without_view"].tobytes(), "the launches with and without a view differ"
    assert last["with_view"][:64].tobytes() == like.batch(X[:64]).tobytes(), "device and host builds differ"
    out = dict(network=name + " x 3", lanes=like.lanes_per_point, species=like.n_species, viewed_coordinates=like._view_size(), chains=N, tries=k, points=n,
               items=3 * n, failed_points=int(np.sum(last["with_view"] == -np.inf)))
    for key in objs:
        us = float(np.median(t[key]))
        out[key] = dict(us_per_launch=round(us, 1), us_per_launch_min_max=[round(min(t[key]), 1), round(max(t[key]), 1)], proposals_per_s=round(n / us * 1e6),
                        code_object=notes(objs[key].code_object()))
    out["with_over_without"] = round(out["with_view"]["us_per_launch"] / out["without_view"]["us_per_launch"], 4)
    lo, hi = (min(t["with_view"]) / max(t["without_view"]), max(t["with_view"]) / min(t["without_view"]))
    out["ratio_over_the_rounds_spread"] = [round(lo, 4), round(hi, 4)]
    print(json.dumps(out), flush=True)
    return out


def _first_rest(args):
    """(S, reactions, y0, k, horizon, rtol, atol, t_last) -> the first exponent p at which Radau's state at t_last + 10**p passes numpy's
    drift test; 99 if none up to 10**9.  One Radau run per point, carried on from power to power and ended at the first that passes
    (ode_settle_networks.radau_at: ode_reference.radau with a numpy Jacobian)."""
    from tests import ode_settle_networks as SN
    S, rx, y0, k, horizon, rtol, atol, t_last = args
    y, now = np.asarray(y0, dtype=float), 0.0
    for p in range(0, 10):
        y, now = SN.radau_at(S, rx, k, y, [t_last + 10.0 ** p], t0=now)[0], t_last + 10.0 ** p
        if SN.drift(S, rx, k, y, horizon, rtol, atol) <= 1.0:
            return p
    return 99


def settle_rate(N, k, name, t_big=None, rounds=7, reps=10, search_only=False, before=None):
    """The last output at inf against a finite last output at t_last + t_big: see the head"""
    import multiprocessing
    from pydream_amd.likelihoods import MassActionODELogLike
    from tests import ode_reference as R
    from tests import ode_settle_networks as SN
    from tests.ode_support import notes
    like = SN.single(name)
    S, rx, y0, _, _, nominal, _, _ = SN.network(name)
    st, n, t_last = like.settle, N * k, like.t_last
    X = box_points(nominal, 1.0, n)
    workers = int(os.environ.get("DREAMZS_HOST_WORKERS", "16"))
    searched = t_big is None
    if searched:                                                         # (the workers are forked before this process opens the device)
        with multiprocessing.get_context("fork").Pool(workers) as pool:
            exps = pool.map(_first_rest, [(S, rx, y0, R.rate_constants(rx, x, "log10"), st["horizon"], st["rtol"], st["atol"], t_last) for x in X], chunksize=8)
        assert max(exps) < 99, "Radau did not come to rest at some point"
        t_big = 10.0 ** max(exps)
        if search_only:                                                  # (no device is opened: the search alone, for a later run's --t-big)
            out = dict(network=name, lanes=like.lanes_per_point, chains=N, tries=k, points=n, t_last=t_last, t_big=t_big,
                       points_first_at_rest_by_power_of_ten=np.bincount(exps).tolist())
            print(json.dumps(out), flush=True)
            return out
    late = MassActionODELogLike(S, rx, like.y0, np.r_[like.t[:-1], t_last + t_big], like.observables, like.data, like.sd, lanes_per_point=like.lanes_per_point)
    objs = dict(late_output=late, steady_output=like)
    # the same network without the phase (t = [.., t_last]): this checkout's kernel and, with --before, the code object another checkout
    # (the commit before the phase existed) built from the same generated source
    objs["without_phase"] = SN.finite_twin(like)
    if before is not None:
        objs["without_phase_before"] = SN.finite_twin(like, path=before)
    for obj in objs.values():
        obj.host_library()
    with multiprocessing.get_context("fork").Pool(workers) as pool:
        hosts = {key: pool.map(_host_part, [(obj, part) for part in np.array_split(X, workers)]) for key, obj in objs.items()}
        sims = {key: np.concatenate(pool.map(_host_rows, [(obj, part) for part in np.array_split(X[:256], workers)])) for key, obj in objs.items()}
    engines = {key: engine_for(obj, N, k, nominal, 1.0) for key, obj in objs.items()}
    last, t = timed({key: (lambda eng=eng: eng.eval_logp(X)[1]) for key, eng in engines.items()}, rounds, reps)
    out = dict(network=name, lanes=like.lanes_per_point, species=S, chains=N, tries=k, points=n, t_last=t_last, t_big=t_big,
               t_big_from="Radau's state passes numpy's drift test at every point" if searched else "--t-big", settle=st)
    for key, lk in last.items():
        host, steps = np.concatenate([p[0] for p in hosts[key]]), np.concatenate([p[1] for p in hosts[key]])
        assert lk.tobytes() == host.tobytes(), "device and host builds differ (%s)" % key
        us = float(np.median(t[key]))
        out[key] = dict(steps_median=float(np.median(steps)), steps_max=int(steps.max()), failed_points=int(np.sum(lk == -np.inf)), us_per_launch=round(us, 1),
                        us_per_launch_min_max=[round(min(t[key]), 1), round(max(t[key]), 1)], proposals_per_s=round(n / us * 1e6),
                        code_object=notes(objs[key].code_object()))
    both = np.all(np.isfinite(sims["late_output"][:, -1]), axis=1) & np.all(np.isfinite(sims["steady_output"][:, -1]), axis=1)
    gap = np.abs(sims["late_output"][both, -1] - sims["steady_output"][both, -1]) / (st["atol"] + st["rtol"] * np.abs(sims["steady_output"][both, -1]))
    out["last_rows_apart_in_units_of_the_tolerance_max_over_256_points"] = round(float(gap.max()), 3)
    if before is not None:
        assert last["without_phase"].tobytes() == last["without_phase_before"].tobytes(), "the two code objects of the phase-less network differ in their values"
        a, b = t["without_phase"], t["without_phase_before"]
        out["without_phase_after_over_before"] = round(float(np.median(a)) / float(np.median(b)), 4)
        out["without_phase_ratio_over_the_rounds_spread"] = [round(min(a) / max(b), 4), round(max(a) / min(b), 4)]
    out["steady_over_late"] = round(out["steady_output"]["us_per_launch"] / out["late_output"]["us_per_launch"], 4)
    lo, hi = (min(t["steady_output"]) / max(t["late_output"]), max(t["steady_output"]) / min(t["late_output"]))
    out["ratio_over_the_rounds_spread"] = [round(lo, 4), round(hi, 4)]
    print(json.dumps(out), flush=True)
    return out


def normalize_rate(N, k, name, kind, rounds=7, reps=10, before=None):
    """Every observable normalised by `kind` against the same network without the keyword: see the head"""
    import multiprocessing
    from pydream_amd.likelihoods import MassActionODELogLike, Normalize
    from tests.ode_support import notes
    if name == "mm":
        from tests import ode_networks as NW
        plain, nominal = NW.michaelis_menten(), NW.MM_NOMINAL
    else:
        from tests import ode_equilibrate_networks as EQ
        plain, nominal = EQ.single(name, equilibrate=False), EQ.network(name)[5]
    z = Normalize("ref", float(plain.t[-1])) if kind == "ref" else Normalize(kind)
    make = lambda **kw: MassActionODELogLike(plain.n_species, plain.reactions, plain.y0, plain.t, plain.observables, plain.data, plain.sd,      # noqa: E731
                                             lanes_per_point=plain.lanes_per_point, **kw)
    objs = dict(plain=plain, normalized=make(normalize=[z] * len(plain.observables)))
    if before is not None:
        objs["plain_before"] = make(path=before)
    n = N * k
    X = box_points(nominal, 1.0, n)
    workers = int(os.environ.get("DREAMZS_HOST_WORKERS", "16"))
    for obj in objs.values():
        obj.host_library()
    with multiprocessing.get_context("fork").Pool(workers) as pool:      # (the workers are forked before this process opens the device)
        hosts = {key: pool.map(_host_part, [(obj, part) for part in np.array_split(X, workers)]) for key, obj in objs.items()}
    engines = {key: engine_for(obj, N, k, nominal, 1.0) for key, obj in objs.items()}
    last, t = timed({key: (lambda eng=eng: eng.eval_logp(X)[1]) for key, eng in engines.items()}, rounds, reps)
    out = dict(network=name, lanes=plain.lanes_per_point, species=plain.n_species, observables=len(plain.observables), times=len(plain.t), kind=kind,
               chains=N, tries=k, points=n)
    for key, lk in last.items():
        host, steps = np.concatenate([p[0] for p in hosts[key]]), np.concatenate([p[1] for p in hosts[key]])
        assert lk.tobytes() == host.tobytes(), "device and host builds differ (%s)" % key
        us = float(np.median(t[key]))
        out[key] = dict(steps_median=float(np.median(steps)), failed_points=int(np.sum(lk == -np.inf)), us_per_launch=round(us, 1),
                        us_per_launch_min_max=[round(min(t[key]), 1), round(max(t[key]), 1)], proposals_per_s=round(n / us * 1e6),
                        code_object=notes(objs[key].code_object()))
    ratio = lambda a, b: (round(float(np.median(t[a])) / float(np.median(t[b])), 4), [round(min(t[a]) / max(t[b]), 4), round(max(t[a]) / min(t[b]), 4)])      # noqa: E731
    out["normalized_over_plain"], out["ratio_over_the_rounds_spread"] = ratio("normalized", "plain")
    if before is not None:
        assert last["plain"].tobytes() == last["plain_before"].tobytes(), "the two code objects of the plain network differ in their values"
        out["plain_after_over_before"], out["plain_ratio_over_the_rounds_spread"] = ratio("plain", "plain_before")
    print(json.dumps(out), flush=True)
    return out


def _host_rows(args):
    like, part = args
    return like.simulate(part)


def _host_part(args):
    like, part = args
    return like.batch(part, return_steps=True)


def host_twin_rate(N, k, name, lanes, rounds=7, reps=10):
    import multiprocessing
    like, nominal, width = network(name, lanes)
    n = N * k
    X = box_points(nominal, width, n)
    like.host_library()                                                 # (compiled before anything is timed or forked)
    workers = int(os.environ.get("DREAMZS_HOST_WORKERS", "16"))
    # (the host pass first: its workers are forked before this process opens the device)
    with multiprocessing.get_context("fork").Pool(workers) as pool:
        pool.map(_host_part, [(like, X[:1])] * workers)                 # (every worker has loaded the library)
        t0 = time.perf_counter()
        parts = pool.map(_host_part, [(like, part) for part in np.array_split(X, workers)])
        host_s = time.perf_counter() - t0
    host, steps = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
    eng = engine_for(like, N, k, nominal, width)
    last, us = timed(dict(device=lambda: eng.eval_logp(X)[1]), rounds, reps)
    lk, t = last["device"], us["device"]
    assert lk.tobytes() == host.tobytes(), "device and host builds differ"
    us = float(np.median(t))
    per_wave = 64 // like.lanes_per_point
    w = steps[: n // per_wave * per_wave].reshape(-1, per_wave)
    out = dict(network=name, lanes=like.lanes_per_point, species=like.n_species, reactions=len(like.reactions), chains=N, tries=k, points=n,
               us_per_launch=round(us, 1), us_per_launch_min_max=[round(min(t), 1), round(max(t), 1)], points_per_s=round(n / us * 1e6),
               steps_median=float(np.median(steps)), steps_max=int(steps.max()),
               lane_efficiency=round(float(w.sum() / (per_wave * np.maximum(w.max(axis=1), 1)).sum()), 3), failed_points=int(np.sum(lk == -np.inf)),
               host_workers=workers, host_pass_s=round(host_s, 2), host_points_per_s=round(n / host_s), device_over_host=round(host_s / (us * 1e-6), 1))
    print(json.dumps(out), flush=True)
    return out


def gens_per_s(like, N, k, G, host_workers=None, nominal=ROB.NOMINAL, width=3.0):
    """generations/s of run_dream from the difference of a G-generation and a 2G-generation run (setup and compilation cancel)"""
    from scipy.stats import uniform
    from pydream_amd.core import run_dream
    from pydream_amd.parameters import SampledParam
    params = [SampledParam(uniform, loc=nominal - width, scale=2 * width)]
    rng = np.random.default_rng(3)
    starts = [nominal + 0.1 * width * rng.uniform(-1, 1, len(nominal)) for _ in range(N)]
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


def main(N=4096, k=5, G=20, kernel_only=False, name="robertson", lanes=None):
    like, nominal, width = network(name, lanes)
    n = N * k
    X = box_points(nominal, width, n)
    eng = engine_for(like, N, k, nominal, width)
    last, us = timed(dict(device=lambda: eng.eval_logp(X)[1]), rounds=1, reps=20)
    lk, us = last["device"], us["device"][0]
    host, steps = like.batch(X, return_steps=True)
    assert lk.tobytes() == host.tobytes(), "device and host builds differ"
    per_wave = 64 // like.lanes_per_point
    w = steps[: n // per_wave * per_wave].reshape(-1, per_wave)
    out = dict(network=name, lanes=like.lanes_per_point, chains=N, tries=k, points=n, us_per_launch=round(us, 1), points_per_s=round(n / us * 1e6),
               steps_median=float(np.median(steps)), steps_max=int(steps.max()),
               lane_efficiency=round(float(w.sum() / (per_wave * w.max(axis=1)).sum()), 3), failed_points=int(np.sum(lk == -np.inf)))
    print(json.dumps(out), flush=True)
    if kernel_only:
        return out
    out["device_gens_per_s"] = round(gens_per_s(like, N, k, G, nominal=nominal, width=width), 2)
    print(json.dumps(out), flush=True)
    out["host_build_16w_gens_per_s"] = round(gens_per_s(HostOnly(like), N, k, 2, host_workers=16, nominal=nominal, width=width), 3)
    out["speedup_vs_host_build"] = round(out["device_gens_per_s"] / out["host_build_16w_gens_per_s"], 1)
    print(json.dumps(out), flush=True)
    if name == "robertson":
        out["odeint_16w_gens_per_s"] = round(gens_per_s(odeint_like, N, k, 1, host_workers=16), 3)
        out["speedup_vs_odeint"] = round(out["device_gens_per_s"] / out["odeint_16w_gens_per_s"], 1)
        print(json.dumps(out), flush=True)
    return out


if __name__ == "__main__":
    argv = sys.argv[1:]
    opt = {}
    for flag in ("--network", "--lanes", "--conditions", "--events", "--t-big", "--before", "--normalize"):
        if flag in argv:
            i = argv.index(flag)
            opt[flag] = argv[i + 1]
            del argv[i:i + 2]
    name, lanes = opt.get("--network", "robertson"), int(opt["--lanes"]) if "--lanes" in opt else None
    nums = [int(a) for a in argv[:2] if not a.startswith("--")]
    nums += [4096, 5][len(nums):]
    if "--host-twin" in argv:
        host_twin_rate(*nums, name, lanes)
    elif "--noise" in argv:
        noise_rate(*nums, name, lanes)
    elif "--input" in argv:
        input_rate(*nums, name)
    elif "--view" in argv:
        view_rate(*nums, name)
    elif "--normalize" in opt:
        normalize_rate(*nums, name, opt["--normalize"], before=opt.get("--before"))
    elif "--settle" in argv:
        settle_rate(*nums, name, float(opt["--t-big"]) if "--t-big" in opt else None, search_only="--search-only" in argv, before=opt.get("--before"))
    elif "--equilibrate" in argv:
        assert "--conditions" in opt and "--events" not in opt, "--equilibrate goes with --conditions C (and without --events)"
        events_rate(*nums, name, lanes, int(opt["--conditions"]), 0, equilibrate=True)
    elif "--events" in opt:
        assert "--conditions" in opt, "--events goes with --conditions C"
        events_rate(*nums, name, lanes, int(opt["--conditions"]), int(opt["--events"]))
    elif "--conditions" in opt:
        conditions_rate(*nums, name, lanes, int(opt["--conditions"]))
    else:
        main(*(int(a) for a in argv[:3] if not a.startswith("--")), kernel_only="--kernel-only" in argv, name=name, lanes=lanes)
