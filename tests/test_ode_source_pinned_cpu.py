"""The generated C++ text and the data block are the interface to everything downstream of MassActionODELogLike -- both builds, the
kernel cache's key and so the bits -- so a change that only reorganises the Python holds them to the byte: sha256(source()) and
sha256(data_block().tobytes()) of every object in tests/ode_pinned_corpus.corpus() against tests/golden/ode_source_parent.json.

The table was recorded on the PARENT of the commit that split likelihoods.py into modules, never from the code under test: a worktree of
that parent commit, tests/ode_pinned_corpus.py copied into its tests/, and there `python -m tests.ode_pinned_corpus
ode_source_parent.json`.  The corpus: the grammar's and the rate-law grammar's networks, the named rate-law networks, the Monomial specs,
make_likelihood() of the eight ODE examples, and for each of the five shapes of source (one lane up to 16 reactions, one lane above, 16,
32 and 64 lanes) a network with conditions, Monomials, events, equilibration and a Hill factor at once."""
import json
import os

import pytest

from . import ode_pinned_corpus as PC

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ode_source_parent.json")) as _f:
    PARENT = json.load(_f)


@pytest.fixture(scope="module")
def built():
    """{name: (shape, source, hashes)}: the corpus, built once"""
    return {name: (PC.shape_of(like), like.source(), PC.hashes(like)) for name, like in PC.corpus()}


def test_the_table_is_the_corpus(built):
    assert sorted(built) == sorted(PARENT) and len(built) >= 70


def test_every_source_and_data_block_is_the_parents(built):
    moved = [name for name, (_, _, got) in built.items() if got != PARENT[name]]
    assert not moved, moved


def test_every_shape_is_pinned_with_every_feature_on(built):
    for shape in PC.SHAPES:
        sources = [source for s, source, _ in built.values() if s == shape]
        for feature in PC.FEATURES:
            assert any(feature in source for source in sources), (shape, feature)
