#!/usr/bin/env python3
"""Record tests/golden/mega_selection.json: what the persistent generation kernels' selection decides for every case of
tests/mega_select_cases.py, on a GPU, with a library of the commit whose selection is to be the reference.

That library is a scratch build with the recording patch of EXPERIMENTS.md ("After round 6: one host function decides each persistent-kernel launch (a refactor)"): it
appends " @grid,block,lds" to every launch's name in dz_last_kernel_variant and " #<the derived shape>" behind them (the fields SHAPE below, the last
one the burn-in mode).  It is selected with DREAMZS_LIB.  One process; the engines run one after another, each closed before the next; the
first error ends the run.  Run it under a time limit:

    DREAMZS_LIB=/path/to/patched/libdreamzs.so timeout -k 10 900 python tests/golden/record_mega_selection.py [out.json]
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from tests import mega_select_cases as MC  # noqa: E402

SHAPE = ("d ld k depairs npt nslots ncr ngamma J tri mtp hard have_prior nl N ncu lk lk_items gen0 gen1 gen2 gen3 redo_possible ad_multi ad_R1 ad_nbp adapt_lag "
         "adapt_fused adapt_groups tempering world mega mega_d2 mega_kc mega_redo_on burnin_mode").split()


def main():
    from pydream_amd import _capi
    assert os.environ.get("DREAMZS_LIB"), "select the patched library with DREAMZS_LIB"
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "mega_selection.json")
    entries = []
    for i, c in enumerate(MC.cases()):
        if c["refused"]:          # (recorded as refused: the pure functions are asked about such shapes by the sweep only)
            try:
                MC.build(_capi.Engine, c)
            except _capi.DreamZSError as err:
                entries.append(dict(case={k: v for k, v in c.items() if MC.case()[k] != v}, refused=str(err)))
                continue
            raise AssertionError("not refused: %r" % (c,))
        e = MC.build(_capi.Engine, c)
        e.profile_enable(True)
        e.profile_reset()
        ran, shape = [], None
        for m in MC.pieces(c):
            e.step(m)
            text, _, dump = e.last_kernel_variant().partition(" #")
            assert dump, "the library does not carry the recording patch"
            shape = [int(v) for v in dump.split()]
            assert len(shape) == len(SHAPE)
            ran.append([text, e.last_kernel_tries(), int(e.profile_get("generations")[1])])
        e.profile_enable(False)
        e.close()
        entries.append(dict(case={k: v for k, v in c.items() if MC.case()[k] != v}, shape=shape, ran=ran))
        print(i, entries[-1]["case"], ran[-1][0], flush=True)
    with open(out, "w") as f:
        f.write('{"shape_fields": %s,\n "entries": [\n' % json.dumps(SHAPE))
        f.write(",\n".join(json.dumps(en, separators=(",", ":")) for en in entries))
        f.write("\n]}\n")
    print("recorded %d cases" % len(entries))


if __name__ == "__main__":
    main()
