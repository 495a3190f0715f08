#!/usr/bin/env python3
"""Record tests/golden/multi_selection.json: what the multi-kernel path launches for every case of tests/multi_select_cases.py, on a GPU, with a
library of the commit whose selection is to be the reference.

That library is a scratch build with the recording patch of EXPERIMENTS.md ("After round 6: one host function decides each launch of the multi-kernel
path"): it writes a line per kernel launch of dz_engine.hip ("L <the launch's kernel as the source spells it> |<NCH> @grid,block,lds") and a marker per generation
("G g c0 nc traced more_follow ntrace"), eval_logp call ("E n defer"), redraw read-back ("R chains listed round batch") and persistent launch ("M")
to the file DZ_RECORD names, and appends " #<the derived shape>" (the fields SHAPE) to dz_last_kernel_variant.  It is selected with DREAMZS_LIB.  One
process; the engines run one after another, each closed before the next; the first error ends the run.  Run it under a time limit:

    DREAMZS_LIB=/path/to/patched/libdreamzs.so timeout -k 10 600 python tests/golden/record_multi_selection.py [out.json]

Per case the fixture holds the shape, the distinct generation signatures ("sigs": the G marker without g and ntrace, then the launches and R markers of
this path in order) and per piece the launches before its first generation ("pre"), the run-length-encoded list of signatures ([[count, index], ..]) and
the launch counts profile_get reports for propose, logp and accept.  Launches of the adaptation, the exchange and the housekeeping copies (k_copy_rows,
k_own_probs) are not part of the path's selection and are left out."""
import json
import os
import re
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from tests import multi_select_cases as XC  # noqa: E402

SHAPE = ("d ld k depairs nslots nch tri mtp_len mu_zero have_prior nl N ncu nlanes lk lk_lanes lk_items redo_possible adapt tempering world thin burnin history_lag "
         "adapt_lag adapt_groups trace propose_split q_defer logp_gemm").split()
KERNELS = ("k_draws k_propose k_propose_stream k_accept k_accept_propose k_logp_mvn_lds k_logp_mvn_mfma k_logp_mvn_mfma_tiled k_logp_mvn_gemm k_logp_mix k_q_finish "
           "k_prior_only k_prior_add k_sum_items module k_redo_flags k_gather_sets k_scatter_logp k_pt_swap").split()
NAME = re.compile(r"^\(?(?:dz::)?(.*?)\)? \|(\d) (@\d+,\d+,\d+)$")          # the launch's source text, NCH_DISPATCH's constant, the geometry


def read(path, at):
    """the records written since offset `at` -> (pre, [signature per generation], new offset)"""
    with open(path) as f:
        f.seek(at)
        lines = f.read().splitlines()
        at = f.tell()
    pre, gens, cur = [], [], None
    for ln in lines:
        tag, _, rest = ln.partition(" ")
        assert tag != "M", "a persistent launch: the case does not stay on the multi-kernel path"
        if tag == "G":
            g, c0, nc, traced, more, ntrace = rest.split()
            cur = ["G %s %s %s %s" % (c0, nc, traced, more)]
            gens.append(cur)
        elif tag == "R":
            cur.append(ln)
        elif tag == "L":
            m = NAME.search(rest)
            assert m, ln
            name = m.group(1).replace(" ", "").replace("<NCH>", "<%s>" % m.group(2)).replace("<PT,RTC>", "<2,4>")      # (eval_logp: constexpr int PT = 2, RTC = 4)
            if name.split("<")[0] in KERNELS:
                assert re.match(r"^\w+(<[0-9a-z,]+>)?$", name), ln          # every template argument as a value
                (pre if cur is None else cur).append(name + m.group(3))
    return pre, gens, at


def main():
    from pydream_amd import _capi
    assert os.environ.get("DREAMZS_LIB"), "select the patched library with DREAMZS_LIB"
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "multi_selection.json")
    log = os.path.join(tempfile.mkdtemp(), "launches.txt")
    os.environ["DZ_RECORD"] = log
    open(log, "w").close()
    entries, at = [], 0
    for i, c in enumerate(XC.cases()):
        e = XC.build(_capi.Engine, c)
        e.profile_enable(True)
        e.profile_reset()
        e.last_kernel_variant()          # (flushes the records of the engine's making)
        at = os.path.getsize(log)
        sigs, ran, shape = [], [], None
        for m in XC.pieces(c):
            XC.step(e, c, m)
            text, _, dump = e.last_kernel_variant().partition(" #")
            assert dump, "the library does not carry the recording patch"
            assert text == "multi-kernel path", text
            shape = [int(v) for v in dump.split()]
            assert len(shape) == len(SHAPE)
            pre, gens, at = read(log, at)
            assert len(gens) == m
            rle = []
            for sig in gens:
                if sig not in sigs:
                    sigs.append(sig)
                j = sigs.index(sig)
                if rle and rle[-1][1] == j:
                    rle[-1][0] += 1
                else:
                    rle.append([1, j])
            ran.append(dict(pre=pre, gens=rle, counts=[int(e.profile_get(w)[1]) for w in ("propose", "logp", "accept")]))
        e.profile_enable(False)
        e.close()
        entries.append(dict(case=XC.brief(c), shape=shape, sigs=sigs, ran=ran))
        print(i, entries[-1]["case"], len(sigs), ran[-1]["counts"], flush=True)
    with open(out, "w") as f:
        f.write('{"shape_fields": %s,\n "entries": [\n' % json.dumps(SHAPE))
        f.write(",\n".join(json.dumps(en, separators=(",", ":")) for en in entries))
        f.write("\n]}\n")
    print("recorded %d cases" % len(entries))


if __name__ == "__main__":
    main()
