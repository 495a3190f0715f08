"""The differential fuzzer's draws are part of the record: tests/test_gpu_fuzz.py's seeds (11-14 without an arm, 21-22 with the adapt_lag
arm) and every recorded profile name configurations by seed, so an arm added to tests/fuzz_parity.draw_config must leave the draws without
it exactly as they were -- the same random numbers consumed in the same order.  The literals are the first three configurations of each of
the six seeds as drawn before the module arm existed."""
import numpy as np
import pytest

from tests import fuzz_parity as F

# seed -> (adapt_lag_arm, the first configurations)
PINNED = {
    11: (False, [
        dict(d=5, N=5, k=5, depairs=2, ngamma=2, ncr=1, adapt_cr=1, adapt_g=0, burnin=6, n=28, lk='mvn_tri', prior='flat', thin=10, lag=1, snooker=0.4, pgu=0.2, lamb=0.05, zeta=1e-06, zero_mean=0, J=3, extra_rows=11, seed=1837640958, pt=0, world=1, s1=0, adapt_lag=0),
        dict(d=5, N=1024, k=5, depairs=1, ngamma=1, ncr=2, adapt_cr=0, adapt_g=0, burnin=0, n=28, lk='mix', prior='normal', thin=10, lag=1, snooker=0.1, pgu=0.0, lamb=0.2, zeta=1e-06, zero_mean=0, J=3, extra_rows=5, seed=1672291623, pt=0, world=2, s1=0, adapt_lag=0),
        dict(d=333, N=256, k=3, depairs=1, ngamma=4, ncr=3, adapt_cr=1, adapt_g=0, burnin=6, n=41, lk='mvn_tri', prior='flat', thin=1, lag=0, snooker=0.1, pgu=0.2, lamb=0.2, zeta=1e-12, zero_mean=0, J=3, extra_rows=27, seed=1601837552, pt=1, world=1, s1=0, adapt_lag=0),
    ]),
    12: (False, [
        dict(d=100, N=16, k=1, depairs=1, ngamma=1, ncr=1, adapt_cr=1, adapt_g=0, burnin=6, n=26, lk='mix', prior='uniform_narrow', thin=1, lag=0, snooker=0.1, pgu=0.6, lamb=0.2, zeta=1e-12, zero_mean=0, J=2, extra_rows=4, seed=1545076076, pt=0, world=1, s1=1, adapt_lag=0),
        dict(d=17, N=256, k=20, depairs=1, ngamma=1, ncr=3, adapt_cr=0, adapt_g=0, burnin=0, n=32, lk='mvn_tri', prior='uniform_open', thin=2, lag=0, snooker=0.4, pgu=0.6, lamb=0.05, zeta=1e-06, zero_mean=0, J=3, extra_rows=16, seed=1685548515, pt=0, world=1, s1=0, adapt_lag=0),
        dict(d=16, N=3, k=9, depairs=3, ngamma=1, ncr=2, adapt_cr=1, adapt_g=0, burnin=26, n=34, lk='mix', prior='normal', thin=10, lag=0, snooker=0.1, pgu=0.2, lamb=0.05, zeta=1e-06, zero_mean=0, J=2, extra_rows=26, seed=1963926595, pt=0, world=1, s1=0, adapt_lag=4),
    ]),
    13: (False, [
        dict(d=129, N=256, k=1, depairs=3, ngamma=4, ncr=2, adapt_cr=1, adapt_g=0, burnin=35, n=30, lk='mix', prior='flat', thin=10, lag=3, snooker=0.0, pgu=0.6, lamb=0.2, zeta=1e-12, zero_mean=0, J=3, extra_rows=3, seed=1412031031, pt=0, world=1, s1=0, adapt_lag=4),
        dict(d=5, N=1100, k=9, depairs=1, ngamma=1, ncr=2, adapt_cr=0, adapt_g=0, burnin=0, n=35, lk='mvn_tri', prior='uniform', thin=2, lag=2, snooker=0.1, pgu=0.6, lamb=0.2, zeta=1e-12, zero_mean=0, J=3, extra_rows=38, seed=605021745, pt=0, world=1, s1=0, adapt_lag=0),
        dict(d=5, N=65, k=6, depairs=1, ngamma=2, ncr=1, adapt_cr=0, adapt_g=1, burnin=18, n=13, lk='mvn_dense', prior='flat', thin=10, lag=1, snooker=0.1, pgu=0.2, lamb=0.2, zeta=1e-06, zero_mean=1, J=2, extra_rows=37, seed=1298325422, pt=0, world=1, s1=0, adapt_lag=2),
    ]),
    14: (False, [
        dict(d=10, N=1024, k=1, depairs=2, ngamma=1, ncr=5, adapt_cr=0, adapt_g=0, burnin=0, n=17, lk='mvn_tri', prior='flat', thin=10, lag=0, snooker=0.1, pgu=0.6, lamb=0.05, zeta=1e-06, zero_mean=0, J=3, extra_rows=36, seed=136502477, pt=0, world=1, s1=0, adapt_lag=0),
        dict(d=128, N=48, k=1, depairs=1, ngamma=4, ncr=3, adapt_cr=0, adapt_g=1, burnin=15, n=28, lk='mvn_tri', prior='uniform', thin=2, lag=0, snooker=0.1, pgu=0.2, lamb=0.2, zeta=1e-12, zero_mean=1, J=2, extra_rows=34, seed=701906793, pt=1, world=1, s1=0, adapt_lag=0),
        dict(d=10, N=1024, k=20, depairs=3, ngamma=4, ncr=5, adapt_cr=0, adapt_g=1, burnin=26, n=34, lk='mix', prior='uniform', thin=1, lag=0, snooker=0.4, pgu=0.2, lamb=0.2, zeta=1e-12, zero_mean=1, J=2, extra_rows=34, seed=362288686, pt=0, world=1, s1=0, adapt_lag=1),
    ]),
    21: (True, [
        dict(d=31, N=1000, k=5, depairs=2, ngamma=1, ncr=1, adapt_cr=1, adapt_g=0, burnin=15, n=30, lk='mvn_dense', prior='normal', thin=10, lag=0, snooker=0.1, pgu=0.6, lamb=0.2, zeta=1e-06, zero_mean=1, J=3, extra_rows=26, seed=1087642834, pt=0, world=1, s1=0, adapt_lag=19),
        dict(d=100, N=1000, k=3, depairs=1, ngamma=4, ncr=2, adapt_cr=1, adapt_g=0, burnin=6, n=22, lk='mvn_tri', prior='uniform_open', thin=1, lag=3, snooker=0.1, pgu=0.6, lamb=0.05, zeta=1e-06, zero_mean=0, J=3, extra_rows=25, seed=923836790, pt=0, world=1, s1=0, adapt_lag=1),
        dict(d=16, N=256, k=6, depairs=1, ngamma=1, ncr=2, adapt_cr=1, adapt_g=0, burnin=27, n=35, lk='mvn_tri', prior='uniform', thin=1, lag=0, snooker=0.1, pgu=0.0, lamb=0.2, zeta=1e-06, zero_mean=0, J=2, extra_rows=23, seed=2066329777, pt=0, world=1, s1=0, adapt_lag=4),
    ]),
    22: (True, [
        dict(d=127, N=48, k=20, depairs=1, ngamma=1, ncr=3, adapt_cr=1, adapt_g=0, burnin=15, n=16, lk='mvn_tri', prior='uniform_open', thin=1, lag=0, snooker=0.1, pgu=0.2, lamb=0.05, zeta=1e-06, zero_mean=1, J=2, extra_rows=19, seed=1955177781, pt=0, world=1, s1=0, adapt_lag=2),
        dict(d=33, N=100, k=1, depairs=1, ngamma=4, ncr=2, adapt_cr=1, adapt_g=1, burnin=6, n=23, lk='mvn_tri', prior='uniform', thin=5, lag=3, snooker=0.4, pgu=0.2, lamb=0.2, zeta=1e-06, zero_mean=0, J=3, extra_rows=35, seed=1268730981, pt=0, world=2, s1=0, adapt_lag=9),
        dict(d=129, N=48, k=6, depairs=1, ngamma=1, ncr=1, adapt_cr=1, adapt_g=0, burnin=13, n=17, lk='mvn_tri', prior='uniform_narrow', thin=1, lag=0, snooker=0.4, pgu=0.2, lamb=0.2, zeta=1e-12, zero_mean=0, J=3, extra_rows=0, seed=1333209604, pt=0, world=1, s1=0, adapt_lag=2),
    ]),
}


@pytest.mark.parametrize("seed", sorted(PINNED))
def test_the_fuzzers_draws_without_the_module_arm_are_those_of_before_it(seed):
    arm, want = PINNED[seed]
    rng = np.random.default_rng(seed)
    got = [F.draw_config(rng, adapt_lag_arm=arm) for _ in want]
    assert got == want
    assert all(type(g[key]) is type(w[key]) for g, w in zip(got, want) for key in w)


def test_the_module_arm_draws_every_shape_and_respects_its_caps():
    from tests import module_kernels as MK
    rng = np.random.default_rng(5)
    cs = [F.draw_config(rng, module_arm=True) for _ in range(300)]
    assert {c["lk"] for c in cs} == set(MK.SHAPES)
    assert all(c["N"] <= 1100 and c["d"] <= 200 for c in cs)
    assert all(c["finite"] == 1 for c in cs if c["lk"] == "function") and {c["finite"] for c in cs if c["lk"] != "function"} == {0, 1}
    assert {c["items"] for c in cs if c["lk"] == "items"} == set(MK.ITEM_COUNTS) and all(c["items"] == 1 for c in cs if c["lk"] != "items")
    assert any(c["world"] > 1 for c in cs) and any(c["pt"] for c in cs) and any(c["s1"] for c in cs) and any(c["lag"] for c in cs) and any(c["adapt_lag"] for c in cs)


def test_the_module_kernels_twins_are_the_density_and_the_kernels_cross_compile():
    """every twin against the density summed in extended precision (they differ in the order of the additions only: a few ulps), the
    non-finite variants' -inf where the cut says, and the batch kernels' sources through hipcc for gfx950"""
    from tests import module_kernels as MK
    d = 33
    X = np.random.default_rng(0).uniform(-5.0, 15.0, (50, d))
    c, w = MK.centre_and_weights(d)
    T = (X - c).astype(np.longdouble)
    ref = (-0.5 * np.sum(w * T * T + 0.001 * T ** 4, axis=1)).astype(float)
    for shape in MK.SHAPES:
        prior, v = MK.twin(shape, d, items=3)(X)
        assert not prior.any() and np.max(np.abs(v - ref) / np.abs(ref)) < 64 * np.finfo(float).eps, shape
        cut = MK.twin(shape, d, cut=5.0, items=3)(X)[1]
        beyond = X[:, 0] > 5.0
        assert beyond.any() and not beyond.all()
        if shape == "function":
            assert cut.tobytes() == v.tobytes()
        else:
            assert np.all(np.isneginf(cut[beyond])) and cut[~beyond].tobytes() == v[~beyond].tobytes(), shape
    for shape in ("thread", "wave", "group16", "group32", "items"):
        path, name = MK.code_object(shape)
        assert open(path, "rb").read(4) == b"\x7fELF" and name.startswith("mk_")
