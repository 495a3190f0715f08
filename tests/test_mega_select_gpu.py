"""The engine feeds the persistent kernels' selection (dz_mega_select.h) the facts tests/test_mega_select_cpu.py assumes: for one case of every distinct
answer recorded in tests/golden/mega_selection.json -- the cheapest one (chains x padded dimensions x tries) -- the engine as built reports the recorded
variant, compiled-in try count and number of generation launches after each piece of tests/mega_select_cases.py (generation 0; burn-in launches; a launch
behind the burn-in that ends with an append; one without; with a history lag, one that holds an append in its middle).  Two answers are distinct when the
variants of their pieces (the row-tile count aside) or their burn-in modes differ.  The chain counts named in ALSO ride along whatever is cheapest: the
smallest populations that give 16-chain blocks (3073), a non-16 block size (1025), a split generation (5000) and 4 x 4 waves with whole blocks (48) on 256
CUs, and d2 with and without the two-pass set at 4096 chains."""
import json
import os
import re

import pytest

from tests import mega_select_cases as MC

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mega_selection.json")
ALSO = [dict(N=3073), dict(N=1025), dict(N=5000), dict(N=48), dict(d=129), dict(d=229)]


def strip(text):
    return re.sub(r" @\d+,\d+,\d+", "", text)


def selected():
    with open(FIXTURE) as f:
        entries = json.load(f)["entries"]
    best, also = {}, []
    for i, (en, c) in enumerate(zip(entries, MC.cases())):
        if "ran" not in en:
            continue
        if en["case"] in ALSO:
            also.append(i)
        key = (tuple(sorted({re.sub(r"<\d+,", "<", strip(r[0])) + " kc%d" % r[1] for r in en["ran"]})), en["shape"][-1])
        cost = c["N"] * en["shape"][1] * c["k"]
        if key not in best or cost < best[key][0]:
            best[key] = (cost, i)
    idx = sorted({i for _, i in best.values()} | set(also))
    return [pytest.param(MC.cases()[i], entries[i]["ran"], id="%d-%s" % (i, "-".join("%s%s" % kv for kv in sorted(entries[i]["case"].items()) if kv[0] != "env") or "base")) for i in idx]


@pytest.mark.parametrize("case,ran", selected())
def test_engine_runs_what_was_recorded(case, ran):
    from pydream_amd import _capi
    e = MC.build(_capi.Engine, case)
    try:
        e.profile_enable(True)
        e.profile_reset()
        for m, (text, tries, launches) in zip(MC.pieces(case), ran):
            e.step(m)
            assert e.last_kernel_variant() == strip(text)
            assert e.last_kernel_tries() == tries
            assert e.profile_get("generations")[1] == launches
        e.profile_enable(False)
    finally:
        e.close()
