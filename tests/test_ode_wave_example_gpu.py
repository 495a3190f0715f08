"""The shipped cascade example (pydream_amd/examples/cascade: 49 species, a wave per point) on the MI355X at a reduced size: main() on
the device gives, sample for sample, what main(host=True) gives through the host twin."""
import os

import numpy as np
import pytest

from pydream_amd.examples.cascade import cascade_device as CAS

from . import ode_wave_networks as WN

pytestmark = pytest.mark.gpu


def test_the_example_on_the_device_equals_its_host_twin_run(tmp_path, capsys):
    os.chdir(tmp_path)
    like = WN.cascade()
    sampled, log_ps = CAS.main(WN.N_ITER, WN.N_CHAINS, like=like)
    assert "the device (64 lanes per point)" in capsys.readouterr().out
    h_sampled, h_log_ps = CAS.main(WN.N_ITER, WN.N_CHAINS, host=True, like=like)
    assert np.all(np.isfinite(np.array(log_ps))) and len(np.unique(np.concatenate(sampled)[:, 0])) > WN.N_CHAINS
    np.testing.assert_array_equal(np.array(sampled), np.array(h_sampled))
    np.testing.assert_array_equal(np.array(log_ps), np.array(h_log_ps))
