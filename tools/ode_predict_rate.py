#!/usr/bin/env python3
"""What keeping the trajectories costs: dz_eval_outputs (the prediction kernels of csrc/dz_ode.h and csrc/dz_ode_group.h behind
MassActionODELogLike.device().simulate) against dz_eval_logp (the likelihood kernels, the same integrations with the observables thrown
away) on the same batch, for the same object, on one engine in one process:

    Robertson @ 1 lane,   the dose-response example @ 1 lane x 6 items,   enzyme13 @ 16 lanes,   the 49-species cascade @ 64 lanes

The batch: N points (default 4096) uniform in the example's prior box.  Both calls upload the rows, launch, synchronise and download --
eval_logp two doubles per point, eval_outputs a term and T * O doubles per item --; the time is the wall time of the whole call, the
median of REPEATS (default 7) calls after one warm-up, the two kernels alternately, with the repeats' minimum and maximum as the
spread.  Beside them the FLOOR of either call: the same call with a kernel that integrates nothing (a thread per item that writes its
term, and for eval_outputs its doubles_per_item values), so what the upload, the launch, the stores and the downloads cost by
themselves.  The host build's simulate on the first HOST_POINTS (default 64) rows gives the scale.  The results of the two device calls
are compared on the way: the terms' sums are eval_logp's values, and the trajectories are the host build's on those rows, byte for byte.

    python tools/ode_predict_rate.py [N] [REPEATS] [HOST_POINTS] [--out profiles/ode_predict_rate.json]
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pydream_amd import _capi                                                  # noqa: E402
from pydream_amd.examples.cascade import cascade_device as CAS                # noqa: E402
from pydream_amd.examples.dose_response import dose_response_device as DR     # noqa: E402
from pydream_amd.examples.enzyme import enzyme_device as ENZ                  # noqa: E402
from pydream_amd.examples.robertson import robertson_device as ROB            # noqa: E402
from pydream_amd.likelihoods import compile_device_kernel                      # noqa: E402

CASES = [("robertson@1", ROB.make_likelihood, ROB.NOMINAL, 3.0), ("dose_response@1x6", DR.make_likelihood, DR.NOMINAL, 1.0),
         ("enzyme13@16", ENZ.make_likelihood, ENZ.NOMINAL, 1.0), ("cascade49@64", CAS.make_likelihood, CAS.NOMINAL, CAS.WIDTH)]


FLOOR = r'''
extern "C" __global__ __launch_bounds__(256) void floor_logp(const double* X, long long n, int d, int ld, double* like, const void* data)
{
    const long long w = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (w < n) like[w] = 0.0;
}
extern "C" __global__ __launch_bounds__(256)
void floor_outputs(const double* X, long long n, int d, int ld, double* like, const void* data, double* out, long long out_ld)
{
    const long long w = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= n) return;
    for (long long m = 0; m < out_ld; ++m) out[w * out_ld + m] = (double)m;
    like[w] = 0.0;
}'''


def timed(f):
    t = time.perf_counter()
    r = f()
    return time.perf_counter() - t, r


def measure(name, make, nominal, width, n, repeats, host_points):
    like = make()
    C, per = len(like._experiments()), len(like.t) * len(like.observables)
    X = nominal - width + 2 * width * np.random.default_rng(11).uniform(size=(n, len(nominal)))
    eng = _capi.Engine(nchains=3, ndim=like.d, history_capacity=8)
    like._dz_apply(eng)
    eng.set_output_module(like.predict_code_object(), like.predict_kernel(), like.lanes_per_point, C, per, like.data_block())
    lk = eng.eval_logp(X)[1]                    # the warm-up of both, and the values
    terms, out = eng.eval_outputs(X)
    total = terms[:, 0].copy()
    for c in range(1, C):
        total = total + terms[:, c]
    assert total.tobytes() == lk.tobytes(), name
    t_like, t_out = [], []
    for _ in range(repeats):
        t_like.append(timed(lambda: eng.eval_logp(X))[0])
        t_out.append(timed(lambda: eng.eval_outputs(X))[0])
    eng.close()
    floor = _capi.Engine(nchains=3, ndim=like.d, history_capacity=8)       # the same calls around kernels that integrate nothing
    path = compile_device_kernel(FLOOR)
    floor.set_likelihood_module(path, "floor_logp", 1, None, False, items_per_point=C)
    floor.set_output_module(path, "floor_outputs", 1, C, per)
    floor.eval_logp(X), floor.eval_outputs(X)
    f_like, f_out = [], []
    for _ in range(repeats):
        f_like.append(timed(lambda: floor.eval_logp(X))[0])
        f_out.append(timed(lambda: floor.eval_outputs(X))[0])
    floor.close()
    t_host, sim = timed(lambda: like.simulate(X[:host_points]))
    dev = out[:host_points].reshape((host_points, C) + sim.shape[-2:])
    dev = dev if like.conditions is not None else dev[:, 0]
    assert np.array_equal(dev, sim, equal_nan=True) and dev[np.isfinite(sim)].tobytes() == sim[np.isfinite(sim)].tobytes(), name
    ml, mo = float(np.median(t_like)), float(np.median(t_out))
    res = dict(network=name, lanes_per_point=like.lanes_per_point, items_per_point=C, points=n, doubles_per_item=per,
               failed_items=int(np.sum(terms == -np.inf)), output_megabytes=round(8e-6 * n * C * per, 3),
               eval_logp_ms=round(1e3 * ml, 3), eval_logp_ms_min_max=[round(1e3 * min(t_like), 3), round(1e3 * max(t_like), 3)],
               eval_outputs_ms=round(1e3 * mo, 3), eval_outputs_ms_min_max=[round(1e3 * min(t_out), 3), round(1e3 * max(t_out), 3)],
               eval_logp_floor_ms=round(1e3 * float(np.median(f_like)), 3), eval_outputs_floor_ms=round(1e3 * float(np.median(f_out)), 3),
               ratio_outputs_over_logp=round(mo / ml, 4),
               ratio_spread=[round(min(t_out) / max(t_like), 4), round(max(t_out) / min(t_like), 4)],
               device_points_per_s=round(n / mo), host_simulate_points=host_points, host_simulate_points_per_s=round(host_points / t_host, 1))
    print(json.dumps(res), flush=True)
    return res


def main(argv):
    out = None
    if "--out" in argv:
        i = argv.index("--out")
        out = argv[i + 1]
        argv = argv[:i] + argv[i + 2:]
    n, repeats, host_points = (int(a) for a in (argv + ["4096", "7", "64"][len(argv):])[:3])
    if repeats < 5:
        raise SystemExit("at least five repeats")
    results = [measure(*case, n, repeats, host_points) for case in CASES]
    if out:
        with open(out, "w") as fh:
            json.dump(dict(tool="tools/ode_predict_rate.py", protocol="wall time of the whole call (upload, launch, synchronise, download); the "
                           "median of %d alternating calls after one warm-up; min_max: the repeats' extremes" % repeats, results=results), fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main(sys.argv[1:])
