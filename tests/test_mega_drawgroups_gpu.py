"""The draw groups of the persistent kernel's <.., KC = 5, PLAIN> instantiations (dz_megakernel.h group_draws: one Philox pass makes the slot draws of three
consecutive generations, the archive row numbers and the control decisions are finished in the lanes that hold the words, and the registers move down by
21 lanes from one generation of the group to the next) against the instantiation that draws once per generation (DZ_MEGA_KC=0), the multi-kernel path (DZ_MEGA=0)
and the oracle: trace, archive and final state bit for bit.

The shape and the comparison are tests/test_mega_cursors_gpu.py's and tests/test_mega_kc_gpu.py's (imported, not touched): 3073 chains -- 193 blocks of 16,
the last with one live chain --, multitry 5.  What varies here is what a group can get wrong:
  * the launch length: `step` in uneven pieces gives launches of 1, 2, 4, 10 and 20 generations -- a launch of n generations ends with a group of n mod 3,
    whose spare lanes belong to generations the launch does not run;
  * the archive row count INSIDE a group: with history lag 3 a launch makes an append in its middle, and the generations behind it -- the later lanes of the
    same Philox pass -- sample N more rows.  thin 1, 4, 7 and 10 with pieces cut so that such an append falls on the first, second and third generation of a
    group (test_the_cases_cover_every_group_position checks the plan below against the engine's launch rule, and every run checks its launch count against it);
  * the snooker flag each lane's row numbers are made with: snooker 0 (no lane), 1 (every lane), 0.5 (they differ inside a group);
  * d = 97 / 100, the dense matrix with the states in LDS (d = 7) and in HBM (d = 100), no trace buffer, trace_reset() between the pieces."""
import numpy as np
import pytest

from tests import helpers as H
from tests import test_mega_cursors_gpu as CUR
from tests import test_mega_kc_gpu as KC

pytestmark = pytest.mark.gpu

N = KC.N
GROUP = 3          # generations per draw group at five tries: 64 lanes / 21 slots


def plan(pieces, thin, lag, segs):
    """The persistent kernel's launches [(first generation, generations)] of a run stepped in `pieces` (dz_engine.hip mega_segment: a launch ends with a
    history append, or -- once `lag` appends are made -- with its min(lag + 1, DZ_MEGA_SEGS)-th, or with the piece; the archive is sized for
    sum(pieces) // thin + 2 appends and no launch asks for more room than is left), and the group positions of the appends made INSIDE a launch
    (not by its last generation: the generations behind such an append sample N more rows)."""
    cap = sum(pieces) // thin + 2
    g, napp, out, inside = 0, 0, [], []
    for m in pieces:
        rem = m
        while rem > 0:
            s = min(lag + 1, segs or (1 << 20)) if (lag >= 1 and napp >= lag) else 1
            s = max(1, min(s, cap - napp))
            n = apps = 0
            while n < rem:
                n += 1
                if (g + n - 1) % thin == 0:
                    apps += 1
                    if apps >= s:
                        break
            for gi in range(n):
                if (g + gi) % thin == 0:
                    napp += 1
                    if gi < n - 1:
                        inside.append(gi % GROUP)
            out.append((g, n))
            g += n
            rem -= n
    return out, inside


# (thin, lag) -> pieces.  Lag 0: a launch ends with its append.  Lag 3: the launches behind the third append hold two appends (DZ_MEGA_SEGS=2); the pieces
# cut them so that the one in the middle falls on each group position.  thin 10 is the headline's schedule: launches of 1, 2, 4, 4, 10, 20 and 4 generations.
PIECES = {
    (1, 0): (1, 2, 4), (1, 3): (1, 2, 4, 3),
    (4, 0): (1, 2, 9, 2), (4, 3): (1, 2, 7, 9, 6),
    (7, 0): (1, 2, 18), (7, 3): (1, 2, 13, 14, 13),
    (10, 0): (1, 2, 4, 14, 4), (10, 3): (1, 2, 4, 4, 10, 20, 4),
}


def run(Cls, d, kind, thin, lag, snooker, trace, seed, want=None, reset=False):
    """-> outputs;  want = (variant, tries, launches or None): a GPU run, which checks after each piece what its last launch ran as"""
    pieces = PIECES[thin, lag]
    GENS = sum(pieces)
    Z0 = H.seed_history(max(10 * d, 64), d, seed)
    X0 = H.seed_history(N, d, seed + 1)
    e = Cls(nchains=N, ndim=d, multitry=5, history_thin=thin, history_lag=lag, snooker=snooker, schedule=2, seed=seed,
            history_capacity=len(Z0) + N * (GENS // thin + 2), trace_capacity=GENS if trace else 0)
    e.set_history(Z0)
    e.set_state(X0)
    P = H.mvn_precision(d)
    if kind == "tri":
        e.set_likelihood_mvn(np.zeros(d), H.tri_factor(P), 1, 0.0)
    else:
        e.set_likelihood_mvn(np.zeros(d), P, 0, 0.0)
    if want:
        e.profile_enable(True); e.profile_reset()
    parts = []
    for i, m in enumerate(pieces):
        e.step(m)
        if want:
            assert e.last_kernel_variant() == want[0]
            assert e.last_kernel_tries() == want[1]
        if reset and trace:
            parts.append(e.get_trace(0, m))
            if i + 1 < len(pieces):
                e.trace_reset()
    if want:
        if want[2] is not None:
            assert e.profile_get("generations")[1] == want[2]
        e.profile_enable(False)
    out = dict(history=e.get_history())
    out["X"], out["lprior"], out["llike"] = e.get_state()
    if trace:
        tr = {key: np.concatenate([p[key] for p in parts]) for key in CUR.TRACE_KEYS} if reset else e.get_trace(0, GENS)
        out.update({"trace_" + key: tr[key] for key in CUR.TRACE_KEYS})
    return out


REFS = {}      # (d, kind, thin, lag, snooker, trace) -> the oracle's outputs and what the other two GPU paths gave, compared once (computed once, never changed)


def seed_of(d, thin, lag):
    return 7500 + 13 * d + 3 * thin + lag


def variant_of(d, kind, xl):
    return "k_generations<%d,%s,%s,16,1,lean>" % ((d + 15) // 16, kind, xl)


def four_way(G, O, monkeypatch, d, kind, thin, lag, segs, snooker=0.5, trace=True, xl="xlds", reset=False):
    for name in ("DZ_MEGA", "DZ_MEGA_KC", "DZ_MEGA_SEGS"):
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setenv("DZ_MEGA_SEGS", str(segs))
    pieces, seed, variant = PIECES[thin, lag], seed_of(d, thin, lag), variant_of(d, kind, xl)
    launches = len(plan(pieces, thin, lag, segs)[0])
    new = run(G.Engine, d, kind, thin, lag, snooker, trace, seed, (variant, 5, launches), reset)
    key = (d, kind, thin, lag, snooker, trace)
    if key not in REFS:      # the three references do not depend on how the launches are cut
        ora = run(O.Engine, d, kind, thin, lag, snooker, trace, seed)
        monkeypatch.setenv("DZ_MEGA_KC", "0")
        gen = run(G.Engine, d, kind, thin, lag, snooker, trace, seed, (variant, 0, launches))
        monkeypatch.delenv("DZ_MEGA_KC")
        KC.assert_identical(gen, ora, "DZ_MEGA_KC=0 against the oracle")
        monkeypatch.setenv("DZ_MEGA", "0")
        mk = run(G.Engine, d, kind, thin, lag, snooker, trace, seed, ("multi-kernel path", 0, None))
        monkeypatch.delenv("DZ_MEGA")
        KC.assert_identical(mk, ora, "the multi-kernel path against the oracle")
        for v in ora.values():
            v.setflags(write=False)
        REFS[key] = ora
    KC.assert_identical(new, REFS[key], "draw groups against the oracle, DZ_MEGA_KC=0 and the multi-kernel path")
    if trace:
        assert abs(new["trace_snooker"].mean() - snooker) < 0.1
        if snooker == 0.5:
            assert 0.02 < new["trace_moved"].mean() < 0.98
    assert len(new["history"]) == max(10 * d, 64) + N * ((sum(pieces) - 1) // thin + 1)          # every append was made, each where it belongs
    return new


def test_the_cases_cover_every_group_position():
    # the plan the cases below rely on: launch lengths 1, 2, 4, 10 and 20, short (n mod 3 = 1, 2) and full last groups, and an append inside a launch on
    # each of the three group positions
    lengths, inside = set(), set()
    for (thin, lag), pieces in PIECES.items():
        for segs in (1, 2):
            ls, ins = plan(pieces, thin, lag, segs)
            lengths |= {n for _, n in ls}
            inside |= set(ins)
            assert sum(n for _, n in ls) == sum(pieces)
            if lag == 0 or segs == 1:
                assert not ins                                                      # such a launch ends with its append
    assert {1, 2, 4, 10, 20} <= lengths
    assert {n % GROUP for n in lengths} == {0, 1, 2}
    assert inside == {0, 1, 2}
    assert plan(KC.PIECES[3], KC.THIN, 3, 2)[0] == [(0, 1), (1, 10), (11, 10), (21, 20), (41, 4)]      # the launches tests/test_mega_kc_gpu.py documents
    assert len(plan(KC.PIECES[3], KC.THIN, 3, 1)[0]) == KC.LAUNCHES[3, 1] and len(plan(KC.PIECES[0], KC.THIN, 0, None)[0]) == KC.LAUNCHES[0, None]


@pytest.fixture(scope="module")
def G():
    from pydream_amd import _capi
    return _capi


@pytest.fixture(scope="module")
def O():
    from oracle import oracle
    return oracle


@pytest.mark.parametrize("segs", [1, 2])
@pytest.mark.parametrize("lag", [0, 3])
@pytest.mark.parametrize("thin", [1, 4, 7, 10])
def test_groups_across_launch_lengths_and_appends(G, O, monkeypatch, thin, lag, segs):
    four_way(G, O, monkeypatch, 100, "tri", thin, lag, segs)


@pytest.mark.parametrize("snooker", [0.0, 1.0])
def test_groups_with_no_and_with_only_snooker_moves(G, O, monkeypatch, snooker):
    new = four_way(G, O, monkeypatch, 100, "tri", 4, 3, 2, snooker=snooker)
    assert new["trace_snooker"].min() == new["trace_snooker"].max() == int(snooker)


def test_groups_at_an_odd_dimension(G, O, monkeypatch):
    four_way(G, O, monkeypatch, 97, "tri", 7, 3, 2)


@pytest.mark.parametrize("d,xl", [(100, "xhbm"), (7, "xlds")])
def test_groups_dense_matrix(G, O, monkeypatch, d, xl):
    four_way(G, O, monkeypatch, d, "dense", 4, 3, 2, xl=xl)


def test_groups_without_a_trace_buffer(G, O, monkeypatch):
    four_way(G, O, monkeypatch, 100, "tri", 10, 3, 2, trace=False)


def test_groups_with_trace_reset_between_the_pieces(G, O, monkeypatch):
    four_way(G, O, monkeypatch, 97, "tri", 7, 3, 2, reset=True)
