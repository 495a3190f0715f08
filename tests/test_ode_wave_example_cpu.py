"""The shipped cascade example (pydream_amd/examples/cascade: 49 species, a wave per point) without a GPU: its network is the one its
docstring describes, and its data are scipy Radau's (its prior box never fails: test_ode_wave_cpu).  The GPU half (test_ode_wave_example_gpu) runs main() at a
reduced size, ode_wave_networks.N_ITER and N_CHAINS, on the device and through the host twin."""
import numpy as np

from pydream_amd.examples.cascade import cascade_device as CAS

from . import ode_networks as NW
from . import ode_wave_networks as WN

def test_the_cascade_is_six_tiers_of_eight_species_and_twelve_reactions():
    assert CAS.N_SPECIES == 49 and len(CAS.REACTIONS) == 72 and CAS.LANES == 64 and len(CAS.NOMINAL) == 12
    assert sorted({r[2] for r in CAS.REACTIONS}) == list(range(12))
    N = np.zeros((49, 72))
    for j, (reac, prod, _) in enumerate(CAS.REACTIONS):
        for s, c in reac.items():
            N[s, j] -= c
        for s, c in prod.items():
            N[s, j] += c
    for i in range(CAS.TIERS):                                              # every tier conserves its kinase and its phosphatase
        b = CAS.tier_base(i)
        kinase = np.zeros(49)
        kinase[[b + CAS.K, b + CAS.KP, b + CAS.KPP, b + CAS.XK, b + CAS.XKP, b + CAS.PKPP, b + CAS.PKP]] = 1.0
        if i + 1 < CAS.TIERS:                                               # (K-PP bound as the next tier's enzyme)
            kinase[[CAS.tier_base(i + 1) + CAS.XK, CAS.tier_base(i + 1) + CAS.XKP]] = 1.0
        pase = np.zeros(49)
        pase[[b + CAS.PASE, b + CAS.PKPP, b + CAS.PKP]] = 1.0
        assert not np.any(kinase @ N) and not np.any(pase @ N), i
    like = WN.cascade()
    assert like.lanes_per_point == 64 and like.n_species == 49 and like.data.shape == (6, 16)


def test_the_cascades_data_are_radaus():
    """simulated_data comes from the solver under test at rtol 1e-11: against Radau (rtol 1e-12, atol 1e-14) within ten tolerances of
    1e-9, the tightest tolerance test_host_twin_is_accurate_against_radau_and_error_shrinks_with_tolerance verifies"""
    ref = (NW.radau(49, CAS.REACTIONS, CAS.Y0, CAS.TSPAN, CAS.NOMINAL) @ CAS.OBSERVABLES.T).T
    err = float(np.max(np.abs(WN.cascade().data - ref) / (1e-9 * np.abs(ref) + 1e-9)))
    print("cascade49 data: %.3g tolerances of 1e-9" % err)
    assert err < 10
