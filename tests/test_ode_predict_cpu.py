"""Prediction with MassActionODELogLike, the part that needs no GPU: the prediction kernels' translation unit (predict_source) is the
likelihood's behind one line, cross-compiles for gfx950 into a code object with exactly one kernel and no scratch where the likelihood
has none; with_outputs makes the sibling object the class docstring describes; posterior_predictive selects the rows it says it
selects; and without a GPU device() raises."""
import re
import subprocess

import numpy as np
import pytest

from pydream_amd import _capi, build as dzbuild
from pydream_amd.likelihoods import MassActionODELogLike, posterior_predictive

from . import ode_networks as NW
from . import ode_pinned_corpus as PC
from . import ode_ratelaw_networks as RN
from . import ode_wave_networks as WN
from .ode_support import READELF, max_rel_err, notes

PREFIX = "#define DZODE_PREDICT 1\n"

# one object of each of the five shapes of generated source: the corpus's "every feature at once" networks, and the 49-species cascade
SHAPES = {
    "one-lane-short": (lambda: PC.everything_on(RN.network(PC.SHAPES["one-lane-short"])), "dz_ode_item_predict"),
    "one-lane-long": (lambda: PC.everything_on(RN.network(PC.SHAPES["one-lane-long"])), "dz_ode_item_predict"),
    "16-lanes": (lambda: PC.everything_on(RN.network(PC.SHAPES["16-lanes"])), "dz_ode_group_item_predict"),
    "32-lanes": (lambda: PC.everything_on(RN.network(PC.SHAPES["32-lanes"])), "dz_ode_group_item_predict"),
    "64-lanes": (lambda: WN.cascade(), "dz_ode_group_predict"),
}


@pytest.mark.parametrize("shape", list(SHAPES))
def test_predict_source_is_the_source_behind_one_line_and_compiles_to_one_kernel(shape):
    make, kernel = SHAPES[shape]
    like = make()
    assert PC.shape_of(like) == shape
    assert like.predict_source() == PREFIX + like.source() and like.predict_kernel() == kernel
    path = like.predict_code_object()
    assert open(path, "rb").read(4) == b"\x7fELF" and like.predict_code_object() == path and path != like.code_object()
    syms = subprocess.run([READELF, "-s", path], capture_output=True, text=True).stdout
    assert set(re.findall(r"(\w+)\.kd\b", syms)) == {kernel}
    twin_syms = subprocess.run([READELF, "-s", like.code_object()], capture_output=True, text=True).stdout
    assert set(re.findall(r"(\w+)\.kd\b", twin_syms)) == {kernel.replace("predict", "batch")}      # (the likelihood's object is what it was)
    n, twin = notes(path), notes(like.code_object())
    print("%s: prediction %d VGPRs (%d AGPRs), scratch %d, LDS %d; likelihood %d VGPRs (%d AGPRs), scratch %d, LDS %d"
          % (shape, n["vgpr"], n["agpr"], n["scratch"], n["lds"], twin["vgpr"], twin["agpr"], twin["scratch"], twin["lds"]))
    assert n["lds"] == twin["lds"]                     # the output path adds no LDS
    if twin["scratch"] == 0:
        assert n["scratch"] == 0


def _live_points(like, nominal, n, seed, width=0.5):
    X = NW.box_points(nominal, n, seed, width=width)
    assert np.all(np.isfinite(like.batch(X)))
    return X


def test_with_outputs_on_the_same_times_simulates_to_the_same_bytes():
    net = RN.network(PC.SHAPES["one-lane-short"])
    for like, nominal in ((NW.chain8(), NW.CHAIN_NOMINAL), (PC.everything_on(net), net.nominal())):
        X = _live_points(like, nominal, 6, 3)
        sib = like.with_outputs(like.t)
        assert sib is not like and sib.source() == like.source()
        a = like.simulate(X)
        assert np.all(np.isfinite(a)) and a.tobytes() == sib.simulate(X).tobytes()


class _AtTimes:
    """simulate() of a sibling object read at the original's output times: what ode_support.max_rel_err compares with a reference"""

    def __init__(self, like, index):
        self.like, self.index = like, index

    def simulate(self, X):
        return self.like.simulate(X)[:, self.index]


def test_with_outputs_on_a_denser_grid_agrees_at_the_original_times():
    """The measure and the margin of tests/test_ode_likelihood_cpu.py's accuracy test (max_rel_err < 10 at the object's rtol), with the
    original object's trajectories as the reference: the denser grid clips other steps, so the two differ by integration error."""
    like = NW.chain8()
    X = _live_points(like, NW.CHAIN_NOMINAL, 8, 5)
    mid = 0.5 * (like.t[1:] + like.t[:-1])
    dense = np.sort(np.r_[like.t, mid, mid[:3] + 0.01])
    index = np.searchsorted(dense, like.t)
    assert np.array_equal(dense[index], like.t)
    sib = like.with_outputs(dense)
    err = max_rel_err(_AtTimes(sib, index), like.simulate(X), X, like.rtol)
    print("denser grid against the original at its times: max_rel_err %.3g at rtol %g" % (err, like.rtol))
    assert err < 10
    assert sib.simulate(X).shape == (len(X), len(dense), len(like.observables))


def test_with_outputs_observes_nothing_and_keeps_the_model():
    like = PC.everything_on(RN.network(PC.SHAPES["one-lane-short"]))
    t = np.linspace(0.0, float(like.t[-1]), 7)
    sib = like.with_outputs(t)
    assert np.array_equal(sib.t, t) and sib.t0 == like.t0 and len(sib.conditions) == len(like.conditions)
    for e, own in zip(sib._experiments(), like._experiments()):
        assert np.all(np.isnan(e["data"])) and e["data"].shape == (len(like.observables), len(t))
        assert e["events"] == own["events"] and e["equilibrate"] == own["equilibrate"] and np.array_equal(e["y0"], own["y0"], equal_nan=True)
    assert sib.scale == like.scale and sib.constraints == like.constraints and sib.reactions == like.reactions
    X = NW.box_points(np.zeros(like.d), 8, 11, width=0.5)
    live = like.batch(X) != -np.inf
    assert live.any()
    const = sum(sib.condition_block(c)[0] for c in range(len(sib.conditions)))
    assert const == 0.0
    np.testing.assert_array_equal(sib.batch(X)[live], (const + sib.constraint_terms(X))[live])
    plain = NW.chain8().with_outputs([0.5, 1.0])
    np.testing.assert_array_equal(plain.batch(_live_points(NW.chain8(), NW.CHAIN_NOMINAL, 4, 2)), np.full(4, plain.condition_block()[0]))
    assert plain.condition_block()[0] == 0.0


def test_with_outputs_events_outside_the_new_span_raise():
    like = NW.chain8(events=[(2.0, 0, 1.0, 0.5)])
    assert like.with_outputs([1.0, 2.0]).events == like.events
    with pytest.raises(ValueError, match=r"event 0: the time must be finite and lie in t0"):
        like.with_outputs([0.5, 1.5])
    with pytest.raises(ValueError, match=r"event 0: the time must be finite and lie in t0"):
        like.with_outputs([3.0, 4.0], t0=2.5)
    with pytest.raises(ValueError, match="output times must be finite, sorted"):
        like.with_outputs([2.0, 1.0])
    multi = PC.everything_on(RN.network(PC.SHAPES["one-lane-short"]))
    with pytest.raises(ValueError, match=r"event 0: the time must be finite"):
        multi.with_outputs([0.1, 0.2])


def test_posterior_predictive_selects_rows_exactly_and_simulates_them_on_the_host():
    like = NW.chain8()
    d = like.d
    rng = np.random.default_rng(4)
    sampled = [NW.CHAIN_NOMINAL + 0.3 * rng.uniform(-1, 1, (7, d)) for _ in range(3)]
    rows, sim = posterior_predictive(sampled, like, burnin=2, thin=2, device=False)
    expect = np.stack([sampled[c][i] for c in range(3) for i in (2, 4, 6)])
    assert rows.tobytes() == expect.tobytes() and rows.shape == (9, d)
    assert np.array_equal(sim, like.simulate(rows), equal_nan=True) and sim.shape == (9, len(like.t), 8)
    rows0, _ = posterior_predictive(sampled, like, device=False)
    assert rows0.tobytes() == np.concatenate(sampled).tobytes()
    t = np.linspace(0.0, 5.0, 25)
    rows_t, sim_t = posterior_predictive(sampled, like, burnin=2, thin=2, device=False, t=t)
    assert rows_t.tobytes() == rows.tobytes() and np.array_equal(sim_t, like.with_outputs(t).simulate(rows), equal_nan=True)
    for bad in (dict(burnin=-1), dict(thin=0), dict(thin=1.5)):
        with pytest.raises(ValueError, match="burnin must be"):
            posterior_predictive(sampled, like, device=False, **bad)


def test_device_without_a_gpu_raises():
    dzbuild.build()
    if _capi.device_count() > 0:
        pytest.skip("a GPU is present")
    like = NW.robertson()
    with pytest.raises(_capi.DreamZSError, match="no HIP device|no CPU fallback"):
        like.device()
    with pytest.raises(_capi.DreamZSError, match="no HIP device|no CPU fallback"):
        posterior_predictive([np.zeros((3, like.d))], like)


def test_the_binding_lists_the_two_new_entry_points():
    assert {"dz_set_output_module", "dz_eval_outputs"} <= set(_capi.SYMBOLS)
    assert isinstance(MassActionODELogLike.device, type(MassActionODELogLike.simulate))
