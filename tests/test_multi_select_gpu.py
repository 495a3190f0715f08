"""The engine feeds the multi-kernel path's selection (dz_multi_select.h) the facts tests/test_multi_select_cpu.py assumes: for one case of every distinct
answer recorded in tests/golden/multi_selection.json -- the cheapest one (chains x padded dimensions x tries) -- the engine as built reports the multi-kernel
path after each piece of tests/multi_select_cases.py and the recorded launch counts of the classes propose, logp and accept (a plan that dropped, doubled or
moved a launch between the launch-timed and the scope-timed form would change them).  Two answers are distinct when their generation signatures differ with
the grids, blocks and LDS sizes left out, so the large populations of the list, recorded for their geometry, are represented by their small twins."""
import json
import os
import re

import pytest

from tests import multi_select_cases as XC

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "multi_selection.json")


def selected():
    with open(FIXTURE) as f:
        entries = json.load(f)["entries"]
    cases, best = XC.cases(), {}
    for i, (en, c) in enumerate(zip(entries, cases)):
        key = (json.dumps([[re.sub(r"@\d+,\d+,\d+$", "", ln) if not ln.startswith("R ") else "R" for ln in sig] for sig in en["sigs"]]),
               json.dumps([r["gens"] for r in en["ran"]]) if not any(ln.startswith("R ") for sig in en["sigs"] for ln in sig) else "redraws")
        cost = c["N"] * en["shape"][1] * c["k"]
        if key not in best or cost < best[key][0]:
            best[key] = (cost, i)
    idx = sorted(i for _, i in best.values())
    return [pytest.param(cases[i], entries[i]["ran"], id="%d-%s" % (i, "-".join("%s%s" % kv for kv in sorted(entries[i]["case"].items()) if kv[0] != "env") or "base")) for i in idx]


@pytest.mark.parametrize("case,ran", selected())
def test_engine_runs_what_was_recorded(case, ran):
    from pydream_amd import _capi
    e = XC.build(_capi.Engine, case)
    try:
        e.profile_enable(True)
        e.profile_reset()
        for m, rec in zip(XC.pieces(case), ran):
            XC.step(e, case, m)
            assert e.last_kernel_variant() == "multi-kernel path"
            assert e.last_kernel_tries() == 0
            assert [int(e.profile_get(w)[1]) for w in ("propose", "logp", "accept")] == rec["counts"]
        e.profile_enable(False)
    finally:
        e.close()
