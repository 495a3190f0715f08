"""The corpus of tests/test_ode_source_pinned_cpu.py: every way the tests and the examples build a MassActionODELogLike, as (name, object)
pairs, and the table of their hashes.  `python -m tests.ode_pinned_corpus OUT.json` writes the table {name: [sha256(source()),
sha256(data_block().tobytes())]} of the checkout it runs in -- how tests/golden/ode_source_parent.json was recorded, on the parent
commit."""
import hashlib
import importlib
import json
import sys

import numpy as np

from pydream_amd.likelihoods import Hill, Monomial, RateLaw

from . import ode_grammar as G
from . import ode_monomial_networks as MN
from . import ode_ratelaw_networks as RN

EXAMPLES = ("robertson", "enzyme", "cascade", "dose_response", "binding_cycle", "washout", "preequilibration", "repressilator")
# The five shapes of generated source and the rate-law network that carries the "everything on" variant of each
SHAPES = {"one-lane-short": 1, "one-lane-long": 3, "16-lanes": 5, "32-lanes": 8, "64-lanes": 11}
FEATURES = ("MONOMIALS", "EVENTS =", "EQUILIBRATE", "SLOTS =", "ITEM_ENTRIES")


def shape_of(like):
    if like.lanes_per_point != 1:
        return "%d-lanes" % like.lanes_per_point
    return "one-lane-long" if len(like.reactions) > 16 else "one-lane-short"


def everything_on(net):
    """The network with every optional construct at once: three conditions (one with its own start, one with its own events and no
    equilibration), a Monomial rate under a Hill factor, a Monomial scale, a constraint, two events and equilibrate=True."""
    reactions = list(net.reactions)
    reactions[0] = (reactions[0][0], reactions[0][1], RateLaw(Monomial({0: 1, 1: -1}, 0.25), [Hill(0, 1, 2, "repression")]))
    O = len(np.eye(net.S)[:G.OBS_LIMIT[net.lanes]])
    conditions = [{}, {"y0": 0.5 * net.y0}, {"events": [(0.5, 0, 1.0, 0.25)], "equilibrate": False}]
    return net.like(reactions=reactions, conditions=conditions, scale=[Monomial({0: 1}, -0.5)] + [1.0] * (O - 1),
                    constraints=[(Monomial({0: 1, 1: -1}), 1.0, 0.5)], events=[(0.25, 0, 1.0, 0.5), (1.0, net.S - 1, 0.0, 0.0)], equilibrate=True)


def corpus():
    """(name, object) of every case, in a fixed order"""
    for i in range(len(G.CASES)):
        net = G.network(i)
        yield "grammar/%d/%s" % (i, net.name), net.like()
    for i in range(len(RN.CASES)):
        net = RN.network(i)
        yield "ratelaw/%d/%s" % (i, net.name), net.like()
    for name in sorted(RN.NAMED):
        yield "ratelaw-named/" + name, RN.build(RN.NAMED[name])
    for name in sorted(MN.SPECS):
        yield "monomial/" + name, MN.build(name)[0]
    for name in EXAMPLES:
        yield "example/" + name, importlib.import_module("pydream_amd.examples.%s.%s_device" % (name, name)).make_likelihood()
    for shape, i in SHAPES.items():
        like = everything_on(RN.network(i))
        assert shape_of(like) == shape, (shape, shape_of(like))
        yield "everything-on/" + shape, like


def hashes(like):
    return [hashlib.sha256(like.source().encode()).hexdigest(), hashlib.sha256(like.data_block().tobytes()).hexdigest()]


if __name__ == "__main__":
    with open(sys.argv[1], "w") as out:
        json.dump({name: hashes(like) for name, like in corpus()}, out, indent=1, sort_keys=True)
        out.write("\n")
