"""The persistent generation kernels' selection (pydream_amd/csrc/dz_mega_select.h: mega_choose, mega_launch_plan), compiled with the host compiler alone.

1. Against tests/golden/mega_selection.json -- what the parent of the commit that introduced the header launched on an MI355X for every case of
   tests/mega_select_cases.py, recorded by tests/golden/record_mega_selection.py.  From each entry's recorded shape the pure functions must give the
   recorded eligibility, burn-in mode and number of parts, and per part every field of the recorded name (family, row tiles, tri / dense, xlds / xhbm,
   chains per block, waves per chain, lean / full, the suffix flags, "+ring"), the compiled-in try count, grid, block and LDS bytes, exactly.
   What this file states about the engine is its schedule, not its policy: the last launch of a piece is burn-in (publish) where the adaptation is on and
   the generation is not behind the crossover burn-in, and it has no adaptation totals pending behind the burn-in (dz_step flushes them at its end, and
   every piece behind the burn-in ends with the only launch that follows a launch of the same kind).
2. A sweep with nothing recorded behind it, over d 1..256, tries 1..32, the chain counts of the issue and both matrix forms, with the adaptation off and
   on: every eligible plan asks for no more LDS than the limit and no more than 1024 threads, its blocks hold its chains, and the parts of a split cover
   the local chains exactly once.  (Why those bounds: 160 KiB of LDS and 1024 threads are what a gfx950 block can have; a chain without a block is not stepped.)
"""
import ctypes
import json
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "pydream_amd", "csrc", "dz_mega_select.h")
FIXTURE = os.path.join(ROOT, "tests", "golden", "mega_selection.json")
BURNIN = 3                      # tests/mega_select_cases.py
FAMILY = {0: None, 1: "k_generations", 2: "k_generations", 3: "k_generations_d2", 4: "k_generations_mix", 5: "k_generations_user"}      # MegaFamily (W4: per part, by its flag)
CHOICE = "family need_x pb pb_lds xlds redo ch split_c ch_b d2_ch d2_sp wpc burnin".split()
PART = "c0 c1 grid block lds ring fused wide tri xlds pb k1 redo ahead sp multi kc ch wpc".split()

SOURCE = """
#include "%s"
static dz::MegaShape shape(const int* v)
{
    dz::MegaShape s;
    s.d = v[0]; s.ld = v[1]; s.k = v[2]; s.depairs = v[3]; s.npt = v[4]; s.nslots = v[5]; s.ncr = v[6]; s.ngamma = v[7]; s.J = v[8];
    s.tri = v[9]; s.mtp = v[10]; s.hard = v[11]; s.have_prior = v[12]; s.nl = v[13]; s.N = v[14]; s.ncu = v[15]; s.lk = v[16]; s.lk_items = v[17];
    for (int i = 0; i < 4; ++i) s.gen_fn[i] = v[18 + i];
    s.redo_possible = v[22]; s.ad_multi = v[23]; s.ad_R1 = v[24]; s.ad_nbp = v[25]; s.adapt_lag = v[26]; s.adapt_fused = v[27]; s.adapt_groups = v[28];
    s.tempering = v[29]; s.world = v[30]; s.mega = v[31]; s.mega_d2 = v[32]; s.mega_kc = v[33]; s.mega_redo = v[34];
    return s;
}
extern "C" long long lds_limit() { return (long long)dz::LDS_LIMIT; }
extern "C" void choose(const int* v, long long* o)
{
    const dz::MegaChoice c = dz::mega_choose(shape(v));
    const long long r[] = {c.family, c.need_x, c.pb, c.pb_lds, c.xlds, c.redo, c.ch, c.split_c, c.ch_b, c.d2_ch, c.d2_sp, c.wpc, c.burnin};
    for (int i = 0; i < 13; ++i) o[i] = r[i];
}
extern "C" int plan(const int* v, int publish, int applies, long long* o)
{
    const dz::MegaShape s = shape(v);
    const dz::MegaLaunchPlan P = dz::mega_launch_plan(dz::mega_choose(s), s, publish != 0, applies != 0);
    for (int i = 0; i < P.nparts; ++i) {
        const dz::MegaPart& q = P.part[i];
        const long long r[] = {q.c0, q.c1, q.grid, q.block, (long long)q.lds, q.ring, q.fused, q.wide, q.f.tri, q.f.xlds, q.f.pb, q.f.k1, q.f.redo, q.f.ahead, q.f.sp,
                               q.f.multi, q.f.kc, q.f.ch, q.f.wpc};
        for (int j = 0; j < 19; ++j) o[19 * i + j] = r[j];
    }
    return P.nparts;
}
"""


class Select:
    def __init__(self, lib):
        self.L = ctypes.CDLL(lib)
        self.L.lds_limit.restype = ctypes.c_longlong

    def choose(self, shape):
        v, o = (ctypes.c_int * 35)(*shape[:35]), (ctypes.c_longlong * 13)()
        self.L.choose(v, o)
        return dict(zip(CHOICE, o))

    def plan(self, shape, publish, applies):
        v, o = (ctypes.c_int * 35)(*shape[:35]), (ctypes.c_longlong * 38)()
        n = self.L.plan(v, int(publish), int(applies), o)
        return [dict(zip(PART, o[19 * i:19 * i + 19])) for i in range(n)]


@pytest.fixture(scope="module")
def sel(tmp_path_factory):
    cxx = next((c for c in ("g++", "c++", "clang++", "/opt/rocm/lib/llvm/bin/clang++") if shutil.which(c)), None)
    assert cxx, "no host C++ compiler"
    tmp = tmp_path_factory.mktemp("mega_select")
    src, lib = str(tmp / "select.cpp"), str(tmp / "libselect.so")
    with open(src, "w") as f:
        f.write(SOURCE % HEADER)
    subprocess.check_call([cxx, "-O1", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", src, "-o", lib])      # (no HIP header on the include path)
    return Select(lib)


@pytest.fixture(scope="module")
def fixture():
    with open(FIXTURE) as f:
        return json.load(f)


NAME = re.compile(r"^(k_generations\w*)(?:<([^>]*)>)? @(\d+),(\d+),(\d+)$")


def parse(text):
    """a recorded variant -> (ring, [per part: dict(name, args, grid, block, lds)])"""
    ring = " +ring" in text
    parts = []
    for t in text.replace(" +ring", "").split(" + "):
        m = NAME.match(t)
        assert m, text
        parts.append(dict(name=m.group(1), args=m.group(2).split(",") if m.group(2) else [], grid=int(m.group(3)), block=int(m.group(4)), lds=int(m.group(5))))
    return ring, parts


def test_fixture_covers_what_it_was_designed_to(fixture):
    from tests import mega_select_cases as MC
    cases = MC.cases()
    assert len(fixture["entries"]) == len(cases) >= 300
    for en, c in zip(fixture["entries"], cases):
        assert en["case"] == {k: v for k, v in c.items() if MC.case()[k] != v}
        assert ("refused" in en) == bool(c["refused"])
    seen = {re.sub(r"<\d+,", "<", re.sub(r" @\d+,\d+,\d+", "", r[0])) for en in fixture["entries"] if "ran" in en for r in en["ran"]}
    for want in ("k_generations<tri,xlds,16,1,lean>", "k_generations<tri,xlds,12,1,lean>", "k_generations<dense,xhbm,16,1,lean>", "k_generations_w4<tri,xlds,4,4,lean,ahead>",
                 "k_generations<tri,xlds,16,1,lean> + k_generations_w4<tri,xlds,4,4,lean,ahead>", "k_generations<tri,xlds,16,1,full,redo>", "k_generations<tri,xlds,16,1,lean,multi>",
                 "k_generations<tri,xlds,12,1,lean> +ring", "k_generations_d2<tri,xhbm,16,1,lean,two-pass>", "k_generations_d2<tri,xhbm,8,2,lean,two-pass>",
                 "k_generations_d2<tri,xhbm,4,4,lean>", "k_generations_d2<tri,xhbm,16,1,full,k1>", "k_generations_mix<multi>", "k_generations_mix<full,wide> +ring",
                 "k_generations_user<full,wide>", "k_generations_user +ring", "multi-kernel path"):
        assert want in seen, want
    assert {en["shape"][-1] for en in fixture["entries"] if "ran" in en} == {0, 1, 2}          # every burn-in mode


def test_pure_functions_reproduce_the_recorded_selection(sel, fixture):
    from tests import mega_select_cases as MC
    F = fixture["shape_fields"]
    assert F[:35] == ("d ld k depairs npt nslots ncr ngamma J tri mtp hard have_prior nl N ncu lk lk_items gen0 gen1 gen2 gen3 redo_possible ad_multi ad_R1 ad_nbp "
                      "adapt_lag adapt_fused adapt_groups tempering world mega mega_d2 mega_kc mega_redo_on").split() and F[35] == "burnin_mode"
    checked = 0
    for en, c in zip(fixture["entries"], MC.cases()):
        if "refused" in en:
            continue
        shape = en["shape"]
        ch = sel.choose(shape)
        eligible = en["ran"][-1][0] != "multi-kernel path"
        assert (ch["family"] != 0) == eligible, en
        assert ch["burnin"] == shape[35], en
        g = 0
        for m, (text, tries, _) in zip(MC.pieces(c), en["ran"]):
            g += m                                                   # the piece's last launch ends with generation g - 1
            assert (text != "multi-kernel path") == eligible, en     # (nothing the selection reads changes between the pieces)
            if not eligible:
                continue
            publish = bool(c["adapt"]) and g - 1 <= BURNIN
            ring, rec = parse(text)
            got = sel.plan(shape, publish, False)
            assert len(got) == len(rec), (en, got)
            for q, r in zip(got, rec):
                what = (en["case"], text, q)
                assert (q["grid"], q["block"], q["lds"]) == (r["grid"], r["block"], r["lds"]), what
                assert bool(q["ring"]) == ring, what
                if ch["family"] in (4, 5):
                    assert r["name"] == FAMILY[ch["family"]], what
                    assert set(r["args"]) == {n for n in ("full", "wide", "multi") if q[{"full": "pb"}.get(n, n)]}, what
                    continue
                assert r["name"] == ("k_generations_w4" if q["ahead"] else FAMILY[ch["family"]]), what
                nrt, mat, xl, chp, wpc, code = r["args"][:6]
                assert (int(nrt), mat, xl, int(chp), int(wpc), code) == (shape[1] // 16, "tri" if q["tri"] else "dense", "xlds" if q["xlds"] else "xhbm", q["ch"], q["wpc"],
                                                                         "full" if q["pb"] else "lean"), what
                assert set(r["args"][6:]) == {n for n, f in (("k1", "k1"), ("redo", "redo"), ("multi", "multi"), ("ahead", "ahead"), ("two-pass", "sp")) if q[f]}, what
            assert got[-1]["kc"] == tries, (en, got)
            checked += 1
    assert checked > 800


def test_pending_adaptation_totals_keep_the_generic_instantiation(sel, fixture):
    """applies = true (the launch's prologue applies the previous launch's adaptation totals) is the one per-launch input no piece's last launch has.  The
    instantiation with the try count compiled in has no code for it: wherever it was recorded, the plan with totals pending must be the plan of the same
    shape under DZ_MEGA_KC=0 -- which the fixture's DZ_MEGA_KC=0 cases hold to the recording -- and nowhere else may the input change anything."""
    kc = 0
    for en in fixture["entries"]:
        if "refused" in en or en["ran"][-1][0] == "multi-kernel path":
            continue
        shape = en["shape"]
        for publish in (False, True):
            plain, pending = sel.plan(shape, publish, False), sel.plan(shape, publish, True)
            if plain[-1]["kc"]:
                assert not publish
                assert pending[-1]["kc"] == 0, en
                assert pending == sel.plan(shape[:33] + [0] + shape[34:], False, False), en
                assert pending[-1]["lds"] < plain[-1]["lds"], en          # (without the output cursors' words)
                kc += 1
            else:
                assert pending == plain, en
    assert kc > 50 and kc == sum(1 for en in fixture["entries"] if "ran" in en and any(r[1] for r in en["ran"]))


def sweep_shape(d, k, N, tri, adapt_lag=0, hard=0, ncu=256):
    ld, npt = (d + 15) // 16 * 16, 1 + (2 * 1 + 3) // 4          # dz_create: depairs 1
    return [d, ld, k, 1, npt, 3 + (2 * k - 1) * npt, 3, 1, 1, tri, tri, hard, 0, N, N, ncu, 1, 1, 0, 0, 0, 0, 0, int(adapt_lag > 0), adapt_lag + 1, 4 if adapt_lag else 0,
            adapt_lag, 1, 0, 0, 1, 1, 1, 1, 1]


def test_every_eligible_plan_fits_the_device(sel):
    limit = sel.L.lds_limit()
    assert limit == 160 * 1024
    eligible = split = 0
    for N in (3, 48, 512, 1024, 1025, 2048, 3072, 3073, 4096, 5000):
        for tri in (1, 0):
            for d in range(1, 257):
                for k in range(1, 33):
                    for adapt_lag, hard in ((0, 0), (3, 1)) if (d % 8 == 0 or d % 16 == 1) else ((0, 0),):
                        shape = sweep_shape(d, k, N, tri, adapt_lag, hard)
                        if sel.choose(shape)["family"] == 0:
                            continue
                        eligible += 1
                        for publish in (False, True) if adapt_lag else (False,):
                            parts = sel.plan(shape, publish, False)
                            assert 1 <= len(parts) <= 2
                            split += len(parts) == 2
                            at = 0
                            for q in parts:
                                what = (shape, publish, q)
                                assert q["lds"] <= limit and q["block"] <= 1024, what
                                assert q["c0"] == at and q["c1"] > q["c0"], what              # the parts cover [0, nl) exactly once
                                assert q["grid"] * q["ch"] >= q["c1"] - q["c0"], what
                                assert q["block"] == 64 * q["ch"] * q["wpc"], what
                                at = q["c1"]
                            assert at == N, (shape, publish, parts)
    assert eligible > 50000 and split > 100


def test_shapes_the_engine_refuses_are_not_eligible(sel):
    # multitry 2 and more than 32 mixture components never reach the selection through dz_create / dz_set_likelihood_mixture (the fixture records the refusals)
    for d in (16, 100, 200):
        assert sel.choose(sweep_shape(d, 2, 4096, 1))["family"] == 0
    mix = sweep_shape(10, 5, 1024, 0)
    mix[16], mix[8] = 2, 33
    assert sel.choose(mix)["family"] == 0
    mix[8] = 32
    assert sel.choose(mix)["family"] == 4
