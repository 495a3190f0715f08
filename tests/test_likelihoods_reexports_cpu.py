"""pydream_amd.likelihoods is the public face of the modules its code lives in: every name the repository imports from it is the object
of its home module (so a pickle that names pydream_amd.likelihoods.<Class> loads), and the ODE values pickle round."""
import pickle

import numpy as np
import pytest

from pydream_amd import _kernel_cache, _ode_values
from pydream_amd import likelihoods as LK

HOMES = {
    LK: ("MVNormalLogLike", "GaussianMixtureLogLike", "DeviceFunctionLogLike", "DeviceKernelLogLike", "MassActionODELogLike",
         "KERNEL_SIGNATURE", "FUNCTION_SIGNATURE"),
    _kernel_cache: ("compile_device_kernel", "csrc_dir", "kernel_cache_dir"),
    _ode_values: ("Monomial", "Hill", "RateLaw", "ODE_LIMITS", "ODE_GROUP_LIMITS", "ODE_WAVE_LIMITS", "ODE_MAX_CONSTRAINTS", "ODE_MAX_EVENTS",
                  "ODE_MAX_CONDITIONS", "ODE_EQUILIBRATE_MAX_STEPS", "ODE_MAX_HILL_EXPONENT", "ODE_MAX_RATE_FACTORS"),
}


@pytest.mark.parametrize("name", [name for names in HOMES.values() for name in names])
def test_a_public_name_is_its_home_modules_object(name):
    home = next(module for module, names in HOMES.items() if name in names)
    assert getattr(LK, name) is getattr(home, name)
    obj = getattr(LK, name)
    if isinstance(obj, type):                                   # a class pickles by reference to a module that has it
        assert getattr(__import__(obj.__module__, fromlist=[name]), name) is obj and pickle.loads(pickle.dumps(obj)) is obj


def test_the_ode_values_and_a_likelihood_with_conditions_pickle_round():
    m = LK.Monomial({0: 1, 2: -0.5}, 0.25)
    h = LK.Hill(1, m, 3, "repression")
    law = LK.RateLaw(0, [h, LK.Hill(0, 1.5)], order={1: 2})
    for value in (m, h, law):
        again = pickle.loads(pickle.dumps(value))
        assert again == value and type(again) is type(value) and repr(again) == repr(value)
    t = np.array([0.5, 1.0])
    like = LK.MassActionODELogLike(2, [({0: 1}, {1: 1}, law), ({1: 1}, {}, m)], [1.0, 0.5], t, np.eye(2), np.ones((2, 2)), 1.0,
                                   conditions=[{}, {"y0": [LK.Monomial({1: 1}), 0.0], "events": [(0.75, 0, 1.0, 0.5)], "equilibrate": True}])
    again = pickle.loads(pickle.dumps(like))
    assert again.source() == like.source() and again.data_block().tobytes() == like.data_block().tobytes()
    assert again.reactions == like.reactions and again.y0_monomials == like.y0_monomials and len(again.conditions) == 2 and again.d == like.d == 3
