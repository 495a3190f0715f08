"""A receptor that binds two ligands in either order, on the device: every sampled coordinate enters the model as part of a PRODUCT of
constants (likelihoods.Monomial) -- dissociation constants, a total amount, a readout's scale, a thermodynamic cycle.

    R + A <-> RA        R + B <-> RB        RA + B <-> RAB        RB + A <-> RAB        RAB -> R + P

The four association rate constants are fixed (diffusion-limited, kf = 10); what is sampled are the dissociation CONSTANTS, so every
backward rate is kr = KD kf = Monomial({i: 1}, log10(kf)).  The two paths from R to RAB close a cycle: KD_A KD_AB = KD_B KD_BA, held to
1 +- 0.01 by one Gaussian constraint on Monomial({0: 1, 2: 1, 1: -1, 3: -1}).  The receptor's total amount is unknown (y0[R] =
Monomial({5: 1})), and the product is read out in arbitrary units (scale = Monomial({6: 1})):

    theta = log10 [KD_A, KD_B, KD_AB, KD_BA, kcat, R_total, scale]

Nine experiments, the doses A, B in {0.3, 1, 3} x {0.3, 1, 3}, the readout at the final time only, sd 5 % + 0.01; a uniform prior two
decades wide around the nominal values.  A proposal is nine integrations from nine starts: one launch over proposals x 9 work items, the
constraint's term added to the first.  The data are simulated with scipy's Radau at the nominal values.

    python -m pydream_amd.examples.binding_cycle.binding_cycle_device [niterations] [nchains]
"""
import sys

import numpy as np

from pydream_amd.likelihoods import MassActionODELogLike, Monomial

SPECIES = ("R", "A", "B", "RA", "RB", "RAB", "P")
R, A, B, RA, RB, RAB, P = range(7)
KF = 10.0                                          # every association rate constant
LOG_KF = float(np.log10(KF))
KD_A, KD_B, KD_AB, KD_BA, KCAT, R_TOTAL, SCALE = range(7)
REACTIONS = [({R: 1, A: 1}, {RA: 1}, KF), ({RA: 1}, {R: 1, A: 1}, Monomial({KD_A: 1}, LOG_KF)),
             ({R: 1, B: 1}, {RB: 1}, KF), ({RB: 1}, {R: 1, B: 1}, Monomial({KD_B: 1}, LOG_KF)),
             ({RA: 1, B: 1}, {RAB: 1}, KF), ({RAB: 1}, {RA: 1, B: 1}, Monomial({KD_AB: 1}, LOG_KF)),
             ({RB: 1, A: 1}, {RAB: 1}, KF), ({RAB: 1}, {RB: 1, A: 1}, Monomial({KD_BA: 1}, LOG_KF)),
             ({RAB: 1}, {R: 1, P: 1}, KCAT)]
CYCLE = (Monomial({KD_A: 1, KD_AB: 1, KD_B: -1, KD_BA: -1}), 1.0, 1e-2)
NOMINAL = np.log10([0.5, 2.0, 1.0, 0.25, 0.3, 0.2, 50.0])          # (KD_A KD_AB = KD_B KD_BA = 0.5)
DOSES = tuple((a, b) for a in (0.3, 1.0, 3.0) for b in (0.3, 1.0, 3.0))
TSPAN = np.array([5.0])
OBSERVABLES = np.zeros((1, 7))
OBSERVABLES[0, P] = 1.0


def start_amounts(dose_a, dose_b):
    return [Monomial({R_TOTAL: 1}), dose_a, dose_b, 0.0, 0.0, 0.0, 0.0]


def simulated_data(rtol=1e-10, atol=1e-12):
    """The scaled readout at TSPAN for the nominal values under every pair of doses, [doses, 1, T], by scipy's Radau."""
    from scipy.integrate import solve_ivp
    k = np.array([r.value(NOMINAL) if isinstance(r, Monomial) else 10.0 ** NOMINAL[r] if isinstance(r, int) else r for _, _, r in REACTIONS])
    N, nu = np.zeros((7, len(REACTIONS))), np.zeros((len(REACTIONS), 7))
    for j, (reac, prod, _) in enumerate(REACTIONS):
        for s, c in reac.items():
            N[s, j] -= c
            nu[j, s] = c
        for s, c in prod.items():
            N[s, j] += c
    out = []
    for a, b in DOSES:
        y0 = np.array([10.0 ** NOMINAL[R_TOTAL], a, b, 0.0, 0.0, 0.0, 0.0])
        sol = solve_ivp(lambda t, y: N @ (k * np.prod(y[None, :] ** nu, axis=1)), (0.0, TSPAN[-1]), y0, method="Radau", t_eval=TSPAN, rtol=rtol, atol=atol)
        assert sol.success, sol.message
        out.append(10.0 ** NOMINAL[SCALE] * (OBSERVABLES @ sol.y))
    return np.array(out)


def make_likelihood(data=None, sd=None, **kw):
    data = simulated_data() if data is None else np.asarray(data, dtype=float)
    sd = 0.05 * np.abs(data) + 0.01 if sd is None else np.broadcast_to(sd, data.shape)
    conditions = [dict(y0=start_amounts(a, b), data=data[c], sd=sd[c]) for c, (a, b) in enumerate(DOSES)]
    return MassActionODELogLike(7, REACTIONS, None, TSPAN, OBSERVABLES, None, None, rate_scale="log10", conditions=conditions,
                                scale=[Monomial({SCALE: 1})], constraints=[CYCLE], **kw)


def main(niterations=300, nchains=64):
    from scipy.stats import uniform
    from pydream_amd.convergence import Gelman_Rubin
    from pydream_amd.core import run_dream
    from pydream_amd.parameters import SampledParam
    like = make_likelihood()
    lower = NOMINAL - 1
    rng = np.random.default_rng(5)
    starts = [NOMINAL + 0.02 * rng.uniform(-1, 1, len(NOMINAL)) for _ in range(nchains)]      # (near the cycle's surface: 1 % wide in a box of two decades)
    sampled, log_ps = run_dream([SampledParam(uniform, loc=lower, scale=2)], like, niterations=niterations, nchains=nchains, multitry=5,
                                start=starts, model_name="binding_cycle_device", verbose=False, save_history=False)
    S_, L = np.concatenate(sampled), np.concatenate(log_ps)
    best = S_[np.argmax(L)]
    cycle = best[KD_A] + best[KD_AB] - best[KD_B] - best[KD_BA]
    print("binding cycle on the device (%d dose pairs per proposal): %d chains x %d iterations; best log p %.3f at theta = %s (nominal %s); "
          "log10 of the cycle's ratio there %.4f; R-hat of the second half: %s"
          % (len(DOSES), nchains, niterations, L.max(), np.round(best, 3), np.round(NOMINAL, 3), cycle,
             np.round(Gelman_Rubin([s[len(s) // 2:] for s in sampled]), 3)))
    return sampled, log_ps


if __name__ == "__main__":
    main(*(int(a) for a in sys.argv[1:3]))
