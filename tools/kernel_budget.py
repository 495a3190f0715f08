"""Register, spill and scalar-load budget of the kernels of ONE translation unit, from a cross-compile (no GPU needed).

    python tools/kernel_budget.py [--nrt 7] [--full] [--match SUBSTRING] [--src pydream_amd/csrc/dz_mega_tu.hip] [--asm file.s] [--keep file.s] [--flat-nesting] [-- extra hipcc flags]

Compiles the unit with the library's flags (pydream_amd/build.py CFLAGS; -DDZ_TU_NRT=<nrt>, and -DDZ_TU_FAST unless --full: the multi-try
16-chain and 4 x 4 instantiations only, tools/fastbuild.sh) and -S into a temporary directory that it removes again (--keep: the listing stays
at that path), or reads a listing made earlier (--asm), and prints per kernel symbol

    vgpr  sgpr  scratch  sgpr_spills  vgpr_spills | loop: lane_rd  lane_wr  params_ld  kernarg_ld  vmcnt0  nop  SALU  branch | static VALU

vgpr .. vgpr_spills are the code object's own metadata.  The loop columns are static counts inside the kernel's LARGEST outermost loop (by
instruction count: the generation loop of the persistent kernels), the blocks of the loops nested in it included:
  lane_rd / lane_wr   v_readlane_b32 / v_writelane_b32 on a register the kernel uses as an SGPR-spill register -- one that some
                      v_writelane_b32 of the kernel writes from a scalar register (the kernels' own code never writes lanes);
  params_ld           scalar loads whose base is not the kernel-argument pointer (in these kernels: fields of Params, read on demand);
  kernarg_ld          scalar loads from the kernel-argument segment (the base of the kernel's first scalar load);
  vmcnt0              s_waitcnt with vmcnt(0): the wave drains every outstanding vector-memory operation;
  nop                 s_nop: wait states the hazard recognizer inserts (a vector write of a scalar register read by the next vector instruction,
                      a vector write read by a DPP move, an asm statement next to a vector instruction) -- issued like any instruction;
  SALU                scalar ALU instructions: every s_* that is not s_nop, s_waitcnt, a branch, a scalar load, s_barrier, s_setprio, s_sleep, s_endpgm;
  branch              s_branch and s_cbranch_*.
They are static: a block inside the try loop runs several times per generation, one in the snooker branch for one chain in ten.  In the headline
kernel every issued instruction counts, the scalar ones and the wait states as much as the vector ones.
--flat-nesting reproduces the figures recorded before the nested loops' inner blocks were attributed: a block of a loop at depth 2 or deeper that is
not that loop's header names only its own loop in the listing, and used to be left out of the loop columns.
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def compile_listing(src, nrt, full, extra, out):
    from pydream_amd import build as dzbuild
    cmd = [dzbuild.hipcc()] + dzbuild.CFLAGS + ["-DDZ_TU_NRT=%d" % nrt] + ([] if full else ["-DDZ_TU_FAST"]) + extra + \
          ["--cuda-device-only", "-S", src, "-o", out]
    subprocess.check_call(cmd)


def metadata(lines):
    """{symbol: {key: int}} from the amdhsa.kernels note (one top-level list entry per kernel)"""
    keys = ("private_segment_fixed_size", "sgpr_count", "sgpr_spill_count", "vgpr_count", "vgpr_spill_count", "agpr_count")
    start = next((i for i, l in enumerate(lines) if l.startswith("amdhsa.kernels:")), len(lines))
    md, cur = {}, None
    for l in lines[start + 1:]:
        if l and not l.startswith(" "):
            break
        if l.startswith("  - "):
            cur = {}
        m = re.match(r"^  (?:- |  )\.(\w+):\s+(\S+)", l)
        if m and cur is not None:
            cur[m.group(1)] = m.group(2)
            if m.group(1) == "name":
                md[m.group(2)] = cur
    return {n: {k: int(v[k]) for k in keys if k in v} for n, v in md.items()}


def kernel_body(lines, sym):
    start = next(i for i, l in enumerate(lines) if l.startswith(sym + ":"))
    end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end") or ".end_amdhsa_kernel" in lines[i])
    return lines[start + 1:end]


def loop_parents(body):
    """{label of a loop header at depth >= 2: label of the depth-1 loop around it}, from the headers' own "Parent Loop .. Depth=1" notes"""
    top = {}
    for i, t in enumerate(body):
        lab = re.match(r"^\.(LBB[0-9_]+):", t)
        if not lab:
            continue
        notes, j = [t], i + 1
        while j < len(body) and body[j].strip().startswith(";") and not body[j].startswith("; %bb."):
            notes.append(body[j])
            j += 1
        txt = " ".join(notes)
        m = re.search(r"Parent Loop (BB[0-9_]+) Depth=1\b", txt)
        if m and re.search(r"Loop Header: Depth=\d+", txt):
            top[lab.group(1)[1:]] = "L" + m.group(1)
    return top


def outer_loops(body, flat=False):
    """instruction list with the Depth=1 loop each instruction belongs to (None outside every loop)"""
    out, cur = [], None
    top = {} if flat else loop_parents(body)
    i = 0
    while i < len(body):
        t = body[i]
        if re.match(r"^(\.LBB[0-9_]+:|; %bb\.)", t):
            # the block's loop comments: on the label line and on the comment-only lines that follow it
            notes = [t.split(";", 1)[1] if ";" in t else ""]
            j = i + 1
            while j < len(body) and body[j].strip().startswith(";") and not body[j].startswith("; %bb."):
                notes.append(body[j])
                j += 1
            txt = " ".join(notes)
            lab = re.match(r"^\.(LBB[0-9_]+):", t)
            m = re.search(r"Parent Loop (BB[0-9_]+) Depth=1\b", txt) or re.search(r"in Loop: Header=(BB[0-9_]+) Depth=1\b", txt)
            if m:
                cur = "L" + m.group(1)
            elif re.search(r"=>This (?:Inner )?Loop Header: Depth=1\b", txt) and lab:
                cur = lab.group(1)
            else:       # a block of a nested loop that is not its header: "in Loop: Header=<that loop> Depth=2.."
                m = re.search(r"in Loop: Header=(BB[0-9_]+) Depth=\d+", txt)
                cur = top.get(m.group(1)) if m else None
            i = j
            continue
        code = t.split(";")[0].strip()
        if code and not code.startswith(".") and not code.endswith(":"):
            out.append((code, cur))
        i += 1
    return out


NOT_SALU = ("s_nop", "s_waitcnt", "s_branch", "s_cbranch", "s_load", "s_buffer_load", "s_barrier", "s_setprio", "s_sleep", "s_endpgm")


def counts(body, flat=False):
    ins = outer_loops(body, flat)
    size = {}
    for _, lp in ins:
        if lp:
            size[lp] = size.get(lp, 0) + 1
    main = max(size, key=size.get) if size else None
    spill_regs = set()
    for code, _ in ins:
        m = re.match(r"v_writelane_b32 (v\d+), s\d+", code)
        if m:
            spill_regs.add(m.group(1))
    karg = None
    for code, _ in ins:
        m = re.match(r"s_load_\w+ \S+, (s\[\d+:\d+\])", code)
        if m:
            karg = m.group(1)
            break
    r = {"lane_rd": 0, "lane_wr": 0, "params_ld": 0, "kernarg_ld": 0, "vmcnt0": 0, "nop": 0, "salu": 0, "branch": 0, "loop_instr": size.get(main, 0)}
    valu = 0
    for code, lp in ins:
        if code.startswith("v_") and not code.startswith("v_mfma"):
            valu += 1
        if lp != main or main is None:
            continue
        m = re.match(r"v_readlane_b32 s\d+, (v\d+)", code)
        if m and m.group(1) in spill_regs:
            r["lane_rd"] += 1
        m = re.match(r"v_writelane_b32 (v\d+), s\d+", code)
        if m:
            r["lane_wr"] += 1
        m = re.match(r"s_load_\w+ \S+, (s\[\d+:\d+\])", code)
        if m:
            r["kernarg_ld" if m.group(1) == karg else "params_ld"] += 1
        if code.startswith("s_waitcnt") and re.search(r"vmcnt\(0\)", code):
            r["vmcnt0"] += 1
        op = code.split()[0]
        if op == "s_nop":
            r["nop"] += 1
        elif op == "s_branch" or op.startswith("s_cbranch"):
            r["branch"] += 1
        elif op.startswith("s_") and not op.startswith(NOT_SALU):
            r["salu"] += 1
    r["valu"] = valu
    return r


def main():
    argv = sys.argv[1:]
    extra = []
    if "--" in argv:
        extra = argv[argv.index("--") + 1:]
        argv = argv[:argv.index("--")]
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--nrt", type=int, default=7)
    ap.add_argument("--full", action="store_true", help="every instantiation of the unit (slow), not the DZ_TU_FAST subset")
    ap.add_argument("--match", default="", help="only symbols that contain this")
    ap.add_argument("--src", default=os.path.join(ROOT, "pydream_amd", "csrc", "dz_mega_tu.hip"))
    ap.add_argument("--asm", default=None, help="a listing made earlier (hipcc -S or --save-temps) instead of compiling")
    ap.add_argument("--keep", default=None, help="write the listing the compile makes to this path and leave it there")
    ap.add_argument("--flat-nesting", action="store_true", help="leave the inner blocks of nested loops out of the loop columns, as the figures recorded earlier did")
    a = ap.parse_args(argv)
    if a.asm:
        lines = open(a.asm).read().split("\n")
    else:
        with tempfile.TemporaryDirectory(prefix="kernel_budget_") as tmp:
            path = a.keep or os.path.join(tmp, "unit.s")
            compile_listing(a.src, a.nrt, a.full, extra, path)
            lines = open(path).read().split("\n")
    md = metadata(lines)
    print("%-5s %-5s %-7s %-6s %-6s | %-7s %-7s %-9s %-10s %-6s %-5s %-5s %-6s | %-6s %s" %
          ("vgpr", "sgpr", "scratch", "sspill", "vspill", "lane_rd", "lane_wr", "params_ld", "kernarg_ld", "vmcnt0", "nop", "SALU", "branch", "VALU", "kernel"))
    for sym in sorted(md):
        if a.match not in sym:
            continue
        m, c = md[sym], counts(kernel_body(lines, sym), a.flat_nesting)
        name = sym
        try:
            name = subprocess.run(["c++filt", sym], capture_output=True, text=True, check=True).stdout.strip().split("(")[0]
        except (OSError, subprocess.CalledProcessError):
            pass
        print("%-5d %-5d %-7d %-6d %-6d | %-7d %-7d %-9d %-10d %-6d %-5d %-5d %-6d | %-6d %s" %
              (m.get("vgpr_count", -1), m.get("sgpr_count", -1), m.get("private_segment_fixed_size", -1), m.get("sgpr_spill_count", -1),
               m.get("vgpr_spill_count", -1), c["lane_rd"], c["lane_wr"], c["params_ld"], c["kernarg_ld"], c["vmcnt0"], c["nop"], c["salu"], c["branch"],
               c["valu"], name))


if __name__ == "__main__":
    main()
