"""The oracle against the REFERENCE ITSELF on configurations drawn at random -- tests/golden/fuzz_reference.py as a test (CPU only).

The reference's side of every case (its inputs and outputs) was recorded by `fuzz_reference.py --record` into tests/golden/fuzz_*.npz; the
oracle is replayed against those recordings here, so the test needs nothing outside the repository.  What is compared, per case: snooker /
CR / selected-try / accept sequences exactly, log densities to 1e-10, states to 1e-9 relative, the archive, delta_m / ncr_updates, and --
in lockstep cases with an adaptation -- the shared probabilities after EVERY generation (what pins `adapt_lag`)."""
import glob
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
ARM_NAMES = {"": "main", "--adapt-lag": "adapt_lag", "--tri": "tri"}

_spec = importlib.util.spec_from_file_location("_fuzz_reference", os.path.join(GOLDEN, "fuzz_reference.py"))
F = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(F)


@pytest.mark.parametrize("arm,n,seed", [
    ("", 26, 60601),               # both schedules, multitry 1..32, pairs, gamma levels, every prior / boundary combination, redraw rounds, history_lag, parallel tempering, half of the adaptations with an adapt_lag
    ("--adapt-lag", 18, 60602),    # every lockstep adaptation case with adapt_lag in {1, 2, 3, 9, 19}, burn-ins ending inside and beyond the run
    ("--tri", 12, 60603),          # MVN up to 100-D, each case also with the triangular factor bench.py's headline times
])
def test_oracle_equals_reference_on_random_configurations(arm, n, seed):
    paths = sorted(glob.glob(os.path.join(GOLDEN, "fuzz_%s_s%d_*.npz" % (ARM_NAMES[arm], seed))))
    assert paths, "no recording of the %r arm (seed %d) under tests/golden" % (arm, seed)
    cases, bad, redrawn, skipped, _ = F.replay(paths)
    assert cases == n and bad == 0, "%d cases, %d mismatches" % (cases, bad)
