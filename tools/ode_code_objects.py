#!/usr/bin/env python3
"""The ODE kernels (csrc/dz_ode_group.h; the view networks: also csrc/dz_ode.h's one lane per item) of a fixed list of networks, cross-compiled for gfx950 from the checkout given as
the argument: one line per code object with its resources and a digest of its instructions, to lay two checkouts side by side (no GPU
needed).

    python tools/ode_code_objects.py TREE [--cache DIR] [--jobs N] [--match TEXT]

TREE: the checkout whose pydream_amd and tests packages are imported (this script may live in another one).  --cache: the kernel cache
directory of this run (default: a fresh temporary one, so nothing comes from an earlier build); --jobs: compilers at a time (default 8);
--match: only the objects whose name contains TEXT.

Per object: name, S, R, lanes; from the code object's notes VGPRs, AGPRs, SGPRs, scratch bytes, static LDS bytes and both spill counts;
the number of lines of `llvm-objdump -d` and the SHA-256 of that text without its address and encoding columns (the comment after each
instruction, the address before each label and the line naming the file).  Equal digests: the same instructions in the same order.
The tool only counts and hashes.
"""
import hashlib
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

LLVM = "/opt/rocm/lib/llvm/bin"
NOTE_KEYS = (("vgpr", ".vgpr_count:"), ("agpr", ".agpr_count:"), ("sgpr", ".sgpr_count:"), ("scratch", ".private_segment_fixed_size:"),
             ("lds", ".group_segment_fixed_size:"), ("sgpr_spill", ".sgpr_spill_count:"), ("vgpr_spill", ".vgpr_spill_count:"))


def objects():
    """name -> constructor of the likelihood object (the tests' networks, imported from TREE)"""
    from tests import ode_condition_networks as CN
    from tests import ode_equilibrate_networks as EQ
    from tests import ode_event_networks as EV
    from tests import ode_monomial_networks as MN
    from tests import ode_wave_networks as WN
    from tests import ode_wide_networks as W
    wave = EQ.smallest_wave_chain()
    out = {}
    for name, case in W.CASES.items():
        out["wide." + name] = case[0]
    for name, case in WN.CASES.items():
        out["wave." + name] = case[0]
    out["dense32x128@32"] = lambda: W.dense_network(32, 128, 32)
    out["dense16x128@16"] = lambda: W.dense_network(16, 128, 16)
    out["dense64x256@64"] = lambda: W.dense_network(64, 256, 64)
    out["conditions.enzyme13"] = lambda: CN.enzyme13()[0]
    out["conditions.chain17@32"] = lambda: CN.chain(17, 32, (1.0, 2.0))[0]
    out["events.enzyme13_conditions"] = lambda: EV.enzyme13_conditions()[0]
    out["events.chain17"] = lambda: EV.single("chain17")
    out["equilibrate.enzyme13_conditions"] = lambda: EQ.conditions("enzyme13")[0]
    out["equilibrate.chain17+bolus"] = lambda: EQ.single("chain17", events=[EQ.BOLUS["chain17"]])
    out["equilibrate." + wave] = lambda: EQ.single(wave)
    for name in MN.SPECS:
        if MN.spec_and_data(name)[0]["lanes"] != 1:
            out["monomials." + name] = lambda name=name: MN.build(name)[0]
    out["wave.%s_conditions+events+monomials" % wave] = lambda: WN.chain_conditions(int(wave[5:]), 3, events=True, monomials=True)[0]
    try:                                    # (a checkout from before conditions had "params": the list ends here)
        from tests import ode_view_networks as VN
    except ImportError:
        return out
    # the networks whose conditions view the point, each beside its twin without a view (one lane per item among them)
    for name in ("mm", "enzyme13", "chain17", VN.WAVE):
        out["view.%s" % name] = lambda name=name: VN.basic(name)[0]
        out["view.%s.twin" % name] = lambda name=name: VN.basic(name, view=False)[0]
    for lanes in (1, 16, 32, 64):
        out["view.readers@%d" % lanes] = lambda lanes=lanes: VN.readers(lanes)[0]
        out["view.readers@%d.twin" % lanes] = lambda lanes=lanes: VN.readers(lanes, view=False)[0]
    import tests
    if not os.path.exists(os.path.join(os.path.dirname(tests.__file__), "ode_normalize_networks.py")):
        return out                          # (a checkout from before `normalize`: the list ends here)
    from tests import ode_normalize_networks as NN
    # the networks with normalised readouts, each beside its twin without the keyword: one lane (4 species; 8 species, the shape with
    # the most registers; items), 16, 32 and 64 lanes
    from tests import ode_networks as NW
    for kind in NN.KINDS:
        out["normalize.mm.%s" % kind] = lambda kind=kind: NN.mm(NN.mm_normalize(kind))
    out["normalize.mm.twin"] = lambda: NN.mm_twin(None)
    out["normalize.mm.minmax+noise"] = lambda: NN.mm(NN.mm_normalize("minmax"), noisy=True)
    out["normalize.mm_conditions"] = lambda: NN.mm_conditions(NN.mm_normalize("max"))[0]
    out["normalize.mm_conditions.twin"] = lambda: NN.mm_conditions(None)[0]
    out["normalize.chain8"] = lambda: NW.chain8(normalize=NN.group_normalize(8, NW.CHAIN_T))
    out["normalize.chain8.twin"] = lambda: NW.chain8()
    for name in ("enzyme13", "chain17", wave):
        out["normalize.%s" % name] = lambda name=name: NN.group(name)[0]
        out["normalize.%s.twin" % name] = lambda name=name: EQ.single(name, equilibrate=False)
    return out


def notes(path):
    txt = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", path], capture_output=True, text=True, check=True).stdout
    return {key: int(txt.split(label)[1].split()[0]) for key, label in NOTE_KEYS}


def disassembly(path):
    """`llvm-objdump -d` without what depends on where the code lies: [lines]"""
    txt = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", path], capture_output=True, text=True, check=True).stdout
    lines = []
    for line in txt.splitlines():
        if "file format" in line:
            continue
        line = re.sub(r"\s*//.*$", "", line)
        line = re.sub(r"^[0-9a-fA-F]+ <", "<", line)
        if line.strip():
            lines.append(line.rstrip())
    return lines


def describe(name, make):
    like = make()
    path = like.code_object()
    n = notes(path)
    lines = disassembly(path)
    digest = hashlib.sha256("\n".join(lines).encode()).hexdigest()
    return ("%-46s S=%-2d R=%-3d lanes=%-2d vgpr=%-3d agpr=%-3d sgpr=%-3d scratch=%d lds=%-5d sgpr_spill=%d vgpr_spill=%d lines=%-6d sha256=%s"
            % (name, like.n_species, len(like.reactions), like.lanes_per_point, n["vgpr"], n["agpr"], n["sgpr"], n["scratch"], n["lds"],
               n["sgpr_spill"], n["vgpr_spill"], len(lines), digest))


def main(argv):
    opt = {}
    for flag in ("--cache", "--jobs", "--match"):
        if flag in argv:
            i = argv.index(flag)
            opt[flag] = argv[i + 1]
            del argv[i:i + 2]
    if len(argv) != 1:
        sys.exit(__doc__)
    tree = os.path.abspath(argv[0])
    sys.path.insert(0, tree)
    os.environ["DREAMZS_KERNEL_CACHE"] = opt.get("--cache") or tempfile.mkdtemp(prefix="ode_code_objects_")
    os.makedirs(os.environ["DREAMZS_KERNEL_CACHE"], exist_ok=True)
    import pydream_amd
    assert os.path.abspath(pydream_amd.__file__).startswith(tree + os.sep), "pydream_amd was imported from %s" % pydream_amd.__file__
    todo = {name: make for name, make in objects().items() if opt.get("--match", "") in name}
    with ThreadPoolExecutor(int(opt.get("--jobs", 8))) as pool:             # (the compiler is a child process: threads suffice)
        for line in pool.map(lambda item: describe(*item), todo.items()):
            print(line, flush=True)


if __name__ == "__main__":
    main(sys.argv[1:])
