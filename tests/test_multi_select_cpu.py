"""The multi-kernel path's selection (pydream_amd/csrc/dz_multi_select.h: logp_plan, generation_plan, redraw_plan), compiled with the host compiler alone.

1. Against tests/golden/multi_selection.json -- what the parent of the commit that introduced the header launched on an MI355X for every case of
   tests/multi_select_cases.py, recorded by tests/golden/record_multi_selection.py.  From each entry's recorded shape the pure functions must give every
   recorded launch of every generation of every piece -- kernel, template arguments, grid, block, LDS bytes, in order -- stepping the carry themselves.
   What this file states about the engine is its schedule, not its policy: dz_step evaluates the chains' states once before its first generation, forgets
   a proposal set made ahead when it starts, passes more_follow for every generation but its last, and every generation is traced; dz_step_range passes
   neither.  The order of a generation's launches is the engine's (per stream group: draws, proposal set, its evaluation, redraw rounds, reference set,
   its evaluation, accept; then the temperature swap); how many chains a redraw read-back lists is data, taken from the recording.
2. A sweep with nothing recorded behind it (made in C++: a few million shapes, each stepped through a dz_step of eight generations and a single-range
   step), over d 1..1100, tries 1..32, chains {3, 64, 100, 1025, 4096, 5000}, 64 / 256 / 304 CUs, both matrix forms -- and, on a thinner grid of d and
   tries, 1..8 stream groups, every likelihood kind, adaptation and tempering on and off.  Bounds: 160 KiB of LDS; the block size each kernel is compiled for
   (__launch_bounds__, listed in the header); a point, chain or draw without a thread is not computed."""
import ctypes
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "pydream_amd", "csrc", "dz_multi_select.h")
FIXTURE = os.path.join(ROOT, "tests", "golden", "multi_selection.json")
FIELDS = ("d ld k depairs nslots nch tri mtp_len mu_zero have_prior nl N ncu nlanes lk lk_lanes lk_items redo_possible adapt tempering world thin burnin history_lag "
          "adapt_lag adapt_groups trace propose_split q_defer logp_gemm").split()
FLAGS = "streamed redo have_prop fused_in need_draws append publish fuse_next defer qdefer prep_next join_first own_probs publish_start join_last swap swap_join".split()

SOURCE = r"""
#include "%s"
#include <stdio.h>
#include <string.h>
#include <string>
#include <vector>
using namespace dz;

static MultiShape shape(const int* v)
{
    MultiShape s;
    s.d = v[0]; s.ld = v[1]; s.k = v[2]; s.depairs = v[3]; s.nslots = v[4]; s.nch = v[5]; s.tri = v[6]; s.mtp_len = v[7]; s.mu_zero = v[8]; s.have_prior = v[9];
    s.nl = v[10]; s.N = v[11]; s.ncu = v[12]; s.nlanes = v[13]; s.lk = v[14]; s.lk_lanes = v[15]; s.lk_items = v[16]; s.redo_possible = v[17]; s.adapt = v[18];
    s.tempering = v[19]; s.world = v[20]; s.thin = v[21]; s.burnin = v[22]; s.history_lag = v[23]; s.adapt_lag = v[24]; s.adapt_groups = v[25]; s.trace = v[26];
    s.propose_split = v[27]; s.q_defer = v[28]; s.logp_gemm = v[29];
    return s;
}
// ---- a generation as the list of its launches, in the engine's order
struct Item { MultiKernel kern; std::string name; MultiLaunch l; long long work, per; };      // work: what the grid must cover, per: how much of it a block takes
struct List {
    std::vector<Item> it; int n = 0; std::string notes;
    void add(MultiKernel kern, const std::string& name, const MultiLaunch& l, long long work, long long per) { it.push_back(Item{kern, name, l, work, per}); ++n; }
};
static std::string nchs(const char* name, const MultiShape& s) { return std::string(name) + "<" + std::to_string(s.nch) + ">"; }
static void logp_items(const MultiShape& s, int n, bool defer, List& o)
{
    const LogpPlan P = logp_plan(s, n, defer);
    const std::string td = P.tri ? "true" : "false";
    switch (P.family) {
        case LOGP_LDS: o.add(MK_LOGP_LDS, "k_logp_mvn_lds<" + std::to_string(P.nrt) + "," + td + ">", P.main, 1, 1); break;      // (its blocks loop over the tiles)
        case LOGP_MFMA: o.add(MK_LOGP_MFMA, "k_logp_mvn_mfma<" + std::to_string(P.pt) + "," + std::to_string(P.nrt) + "," + td + ">", P.main, n, 64 * P.pt); break;
        case LOGP_TILED: o.add(MK_LOGP_TILED, "k_logp_mvn_mfma_tiled<2,4>", P.main, (long long)((n + 31) / 32) * ((P.nrtb + 3) / 4), 4); break;
        case LOGP_GEMM: o.add(MK_LOGP_GEMM, "k_logp_mvn_gemm<" + std::to_string(P.gemm_tile) + ">", P.main, (long long)((n + 32 * P.gemm_tile - 1) / (32 * P.gemm_tile)) * ((P.nrtb * 16 + 63) / 64), 1); break;
        case LOGP_MIX: o.add(MK_LOGP_MIX, nchs("k_logp_mix", s), P.main, n, 4); break;
        case LOGP_MODULE: if (P.grid_overflow) o.notes += "overflow "; o.add(MK_MODULE, "module", P.main, P.items, P.per_block); break;
        default: break;
    }
    if (P.family == LOGP_LDS && (P.nwv < 4 || P.nwv > 8 || P.main.block != 64u * P.nwv || P.main.grid > (unsigned)((n + 15) / 16))) o.notes += "nwv ";
    if ((P.family == LOGP_TILED || P.family == LOGP_GEMM) != (P.qpart_doubles != 0) || (P.family == LOGP_MODULE && s.lk_items > 1) != (P.scratch_doubles != 0)) o.notes += "scratch ";
    if (P.q_finish) o.add(MK_Q_FINISH, "k_q_finish", P.finish, n, 64);
    if (P.sum_items) o.add(MK_SUM_ITEMS, "k_sum_items", P.sum, n, 256);
    if (P.prior_only) o.add(MK_PRIOR_ONLY, nchs("k_prior_only", s), P.prior, n, 4);
    if (P.prior_add) o.add(MK_PRIOR_ADD, nchs("k_prior_add", s), P.prior, n, 4);
}
// listed: the chains each redraw read-back of the generation found (the recording's; the sweep has none: the first read-back finds nothing)
static GenerationPlan generation_items(const MultiShape& s, const MultiStep& t, const MultiCarry& c, const int* listed, int nlisted, List& o)
{
    const GenerationPlan G = generation_plan(s, t, c);
    if (G.refuse) return G;
    for (int i = 0; i < G.ngroups; ++i) {
        const MultiGroup& q = G.grp[i];
        const long long wpb = G.wpb;
        if (G.need_draws) o.add(MK_DRAWS, "k_draws", q.draws, (long long)q.nc * s.nslots, 256);
        if (G.prop0 == PROP_STREAM) o.add(MK_PROPOSE_STREAM, "k_propose_stream", q.prop0, (long long)q.nc * s.k, 4);
        else if (G.prop0 == PROP_FUSED_ACCEPT) o.add(MK_PROPOSE, nchs("k_propose", s), q.prop0, q.nc, wpb);
        else if (G.prop0 == PROP_CHAIN) o.add(MK_PROPOSE, nchs("k_propose", s), q.prop0, (long long)q.nc * G.sp0, wpb);
        logp_items(s, q.n0, G.qdefer, o);
        if (G.redo) {
            int at = 0;
            for (int round = 1; round <= MULTI_MAX_REDRAWS;) {
                o.add(MK_REDO_FLAGS, "k_redo_flags", redraw_plan(s, q.nc, 0, round).flags, q.nc, 256);
                const int n = at < nlisted ? listed[at++] : 0;
                if (n == 0) break;
                const RedrawPlan R = redraw_plan(s, q.nc, n, round);
                char b[96]; snprintf(b, sizeof b, "R %%d %%d %%d %%d", q.nc, n, round, R.batch);
                o.add(MK_COUNT, b, MultiLaunch{1, 1, 0}, 0, 1);
                for (int j = 0; j < R.batch; ++j, ++round) {
                    if (j) o.add(MK_REDO_FLAGS, "k_redo_flags", R.flags, q.nc, 256);
                    o.add(MK_PROPOSE, nchs("k_propose", s), R.propose, (long long)n * R.sp0, multi_wpb(s, q.nc));
                    o.add(MK_GATHER_SETS, "k_gather_sets", R.gather, (long long)n * s.k * s.ld / 2, 256);
                    logp_items(s, R.points, false, o);
                    o.add(MK_SCATTER_LOGP, "k_scatter_logp", R.scatter, (long long)n * s.k, 256);
                }
            }
        }
        if (q.n1 > 0) {
            if (G.streamed) o.add(MK_PROPOSE_STREAM, "k_propose_stream", q.prop1, (long long)q.nc * (s.k - 1), 4);
            else o.add(MK_PROPOSE, nchs("k_propose", s), q.prop1, (long long)q.nc * G.sp1, wpb);
            logp_items(s, q.n1, G.qdefer, o);
        }
        if (G.acc == ACC_ACCEPT_PROPOSE) o.add(MK_ACCEPT_PROPOSE, nchs("k_accept_propose", s), q.accept, q.nc, 1);
        else if (G.acc == ACC_ACCEPT) o.add(MK_ACCEPT, nchs("k_accept", s), q.accept, q.nc, wpb);
    }
    if (G.swap) o.add(MK_COUNT, nchs("k_pt_swap", s), MultiLaunch{1, 64, 0}, 1, 1);
    return G;
}
static int text(const List& o, char* out, int cap)
{
    std::string t;
    for (int i = 0; i < o.n; ++i) {
        char b[64] = "";
        if (o.it[i].name[0] != 'R') snprintf(b, sizeof b, "@%%u,%%u,%%zu", o.it[i].l.grid, o.it[i].l.block, o.it[i].l.lds);
        t += o.it[i].name + b + "\n";
    }
    if ((int)t.size() + 1 > cap) return -1;
    memcpy(out, t.c_str(), t.size() + 1);
    return o.n;
}
extern "C" long long lds_limit() { return (long long)LDS_LIMIT; }
extern "C" int logp(const int* v, int n, int defer, char* out, int cap) { List o; logp_items(shape(v), n, defer != 0, o); return text(o, out, cap); }
// step: c0 nc g traced more_follow ntrace; carry (in and out): pending_accept pending_slot pending_qfin draws_gen stream_prop_gen need_join; flags: FLAGS of the test, then L, ngroups, refuse
extern "C" int generation(const int* v, const long long* step, long long* carry, const int* listed, int nlisted, long long* flags, char* out, int cap)
{
    const MultiShape s = shape(v);
    const MultiStep t = {(int)step[0], (int)step[1], (unsigned)step[2], step[3] != 0, step[4] != 0, step[5]};
    MultiCarry c; c.pending_accept = carry[0]; c.pending_slot = carry[1]; c.pending_qfin = carry[2]; c.draws_gen = carry[3]; c.stream_prop_gen = carry[4]; c.need_join = carry[5];
    List o;
    const GenerationPlan G = generation_items(s, t, c, listed, nlisted, o);
    const long long f[] = {G.streamed, G.redo, G.have_prop, G.fused_in, G.need_draws, G.append, G.publish, G.fuse_next, G.defer, G.qdefer, G.prep_next, G.join_first, G.own_probs, G.publish_start,
                           G.join_last, G.swap, G.swap_join, G.L, G.ngroups, G.refuse};
    for (int i = 0; i < 20; ++i) flags[i] = f[i];
    const MultiCarry& x = G.next;
    const long long nc[] = {x.pending_accept, x.pending_slot, x.pending_qfin, x.draws_gen, x.stream_prop_gen, x.need_join};
    if (!G.refuse) for (int i = 0; i < 6; ++i) carry[i] = nc[i];
    return text(o, out, cap);
}

// ---- the sweep
static std::string g_why;
static bool bad(const MultiShape& s, const char* what, long long a = 0, long long b = 0)
{
    char m[512];
    snprintf(m, sizeof m, "%%s (%%lld, %%lld): d %%d k %%d depairs %%d nl %%d ncu %%d tri %%d nlanes %%d lk %%d lanes %%d items %%d redo %%d adapt %%d tempering %%d prior %%d trace %%d split %%d qdefer %%d gemm %%d", what, a, b, s.d, s.k, s.depairs,
             s.nl, s.ncu, (int)s.tri, s.nlanes, s.lk, s.lk_lanes, s.lk_items, (int)s.redo_possible, (int)s.adapt, (int)s.tempering, (int)s.have_prior, (int)s.trace, s.propose_split, (int)s.q_defer, (int)s.logp_gemm);
    g_why = m;
    return false;
}
static bool check_items(const MultiShape& s, const List& o)
{
    if (!o.notes.empty()) return bad(s, o.notes.c_str());
    for (int i = 0; i < o.n; ++i) {
        const Item& x = o.it[i];
        if (x.kern == MK_COUNT) continue;
        if (x.l.lds > LDS_LIMIT) return bad(s, ("LDS of " + x.name).c_str(), (long long)x.l.lds);
        if (x.l.block < 1 || (int)x.l.block > multi_max_threads(x.kern, s.nch)) return bad(s, ("block of " + x.name).c_str(), x.l.block);
        if (x.l.grid < 1 || (long long)x.l.grid * x.per < x.work) return bad(s, ("grid of " + x.name).c_str(), x.l.grid, x.work);
    }
    return true;
}
static bool check_generation(const MultiShape& s, const MultiStep& t, const MultiCarry& c, const GenerationPlan& G, const List& o)
{
    if (!check_items(s, o)) return false;
    int at = t.c0;
    for (int i = 0; i < G.ngroups; ++i) { if (G.grp[i].c0 != at || G.grp[i].nc < 1) return bad(s, "the stream groups' ranges", i, at); at += G.grp[i].nc; }
    if (at != t.c0 + t.nc || G.ngroups > s.nlanes || G.ngroups > 8) return bad(s, "the stream groups do not partition the chains", at, G.ngroups);
    if (!G.full && (G.ngroups != 1 || G.L != 1)) return bad(s, "a sub-range step on several stream groups", G.L);
    if (G.defer && G.fuse_next) return bad(s, "defer and fuse_next together", t.g);
    const MultiCarry& x = G.next;
    if (!t.more_follow && (G.defer || G.fuse_next || x.pending_accept || x.pending_qfin || x.stream_prop_gen >= 0 || x.pending_slot >= 0)) return bad(s, "deferred with nothing to follow", t.g);
    if (x.pending_accept != G.defer || x.pending_qfin > x.pending_accept) return bad(s, "the carry's deferred accept", t.g);
    if (G.fused_in != (G.full && c.pending_accept) || G.fused_in != (G.prop0 == PROP_FUSED_ACCEPT)) return bad(s, "a deferred accept is consumed by the next plan and nothing else", t.g);
    if (c.pending_accept && (G.need_draws || G.have_prop)) return bad(s, "a deferred accept's generation makes its own draws", t.g);
    if (G.have_prop && (G.prop0 != PROP_NONE || c.stream_prop_gen != (long long)t.g)) return bad(s, "a proposal set made ahead", t.g);
    if (G.qdefer && !(s.lk == MULTI_LK_MVN && s.ld / 16 > 8)) return bad(s, "deferred sums outside the MVN above eight row tiles", t.g);
    if (G.fuse_next && s.k > 16) return bad(s, "accept + propose fused above 16 tries", s.k);
    if ((G.acc == ACC_NONE) != G.defer) return bad(s, "no accept without a deferral", t.g);
    return true;
}
static long long g_plans = 0;
static bool sweep_shape(MultiShape s)
{
    for (int n : {1, s.nl, s.nl * s.k, 4097}) { List o; logp_items(s, n, false, o); if (!check_items(s, o)) return false; }
    MultiCarry c;
    long long ntrace = 0;
    for (unsigned g = 0; g < 8; ++g) {          // a dz_step of eight generations: appends at 0 and 5, burn-in 0..3 where the adaptation is on
        const MultiStep t = {0, s.nl, g, true, g + 1 < 8, ntrace};
        List o;
        const GenerationPlan G = generation_items(s, t, c, nullptr, 0, o);
        ++g_plans;
        if (G.refuse) return bad(s, "a lockstep generation refused");
        if (!check_generation(s, t, c, G, o)) return false;
        if (G.slot >= 0) ++ntrace;
        c = G.next;
    }
    const MultiStep t = {s.nl / 2, 1, 8, false, false, ntrace};
    List o;
    const GenerationPlan G = generation_items(s, t, c, nullptr, 0, o);
    if (G.refuse != (s.world > 1 ? REFUSE_SHARDED : s.history_lag ? REFUSE_HISTORY_LAG : s.adapt_lag ? REFUSE_ADAPT_LAG : REFUSE_NONE)) return bad(s, "the refusals of a sub-range step");
    return G.refuse || check_generation(s, t, c, G, o);
}
static MultiShape base_shape(int d, int k, int nl, int ncu, bool tri)
{
    MultiShape s = {};
    const int chunks = (d + 127) / 128, ks4 = 4 * ((d + 3) / 4);          // dz_create
    s.d = d; s.ld = (d + 15) / 16 * 16; s.k = k; s.depairs = 1; s.nslots = 3 + (2 * k - 1) * 2; s.nch = chunks <= 1 ? 1 : chunks <= 2 ? 2 : chunks <= 4 ? 4 : 8;
    s.tri = tri; s.mtp_len = tri ? tri_row_offset(ks4) : 0; s.mu_zero = false; s.nl = s.N = nl; s.ncu = ncu; s.nlanes = 1; s.lk = MULTI_LK_MVN; s.lk_lanes = 1; s.lk_items = 1;
    s.world = 1; s.thin = 5; s.burnin = 3; s.trace = true; s.q_defer = true; s.logp_gemm = true;
    return s;
}
extern "C" const char* why() { return g_why.c_str(); }
extern "C" long long sweep()
{
    g_plans = 0;
    const int chains[] = {3, 64, 100, 1025, 4096, 5000}, cus[] = {64, 256, 304};
    for (int d = 1; d <= 1100; ++d)
        for (int k = 1; k <= 32; ++k) {
            if (k == 2) continue;          // (dz_create refuses it)
            for (int nl : chains) for (int ncu : cus) for (int tri = 0; tri < 2; ++tri)
                if (!sweep_shape(base_shape(d, k, nl, ncu, tri != 0))) return -1;
            if (!(d <= 20 || d %% 16 <= 1 || d %% 128 == 127) || !(k == 1 || k == 3 || k == 5 || k == 16 || k == 17 || k == 32)) continue;
            for (int nl : chains) for (int nlanes = 1; nlanes <= 8; ++nlanes) for (int kind = 0; kind < 7; ++kind) for (int sched = 0; sched < 8; ++sched) {
                MultiShape s = base_shape(d, k, nl, 256, kind != 1);
                s.nlanes = nl < 64 * nlanes ? 1 : nlanes;          // dz_create
                s.lk = kind < 2 ? MULTI_LK_MVN : kind == 2 ? MULTI_LK_MIX : kind == 3 ? MULTI_LK_HOST : MULTI_LK_MODULE;
                if (kind >= 4) { s.lk_lanes = kind == 4 ? 1 : kind == 5 ? 16 : 64; s.lk_items = kind == 5 ? 3 : 1; }
                s.adapt = sched & 1; s.tempering = (sched & 2) != 0; s.have_prior = (sched & 4) != 0; s.depairs = (sched & 4) ? 2 : 1; s.mu_zero = (sched & 1) != 0;
                if (s.depairs == 2) s.nslots = 3 + (2 * k - 1) * (1 + (2 * 2 + 3) / 4);
                s.redo_possible = k > 1 && (s.lk == MULTI_LK_HOST || kind == 6 || (sched == 6));
                s.trace = !(sched & 2); s.q_defer = sched != 3; s.logp_gemm = sched != 5; s.propose_split = sched == 7 ? 2 : 0;
                s.history_lag = (sched == 4 && !s.tempering) ? 1 : 0; s.adapt_lag = (sched == 5) ? 1 : 0;
                if (!sweep_shape(s)) return -1;
            }
        }
    return g_plans;
}
"""


class Select:
    def __init__(self, lib):
        self.L = ctypes.CDLL(lib)
        self.L.lds_limit.restype = ctypes.c_longlong
        self.L.sweep.restype = ctypes.c_longlong
        self.L.why.restype = ctypes.c_char_p
        self.buf = ctypes.create_string_buffer(1 << 16)

    def logp(self, shape, n, defer=False):
        got = self.L.logp((ctypes.c_int * 30)(*shape), n, int(defer), self.buf, len(self.buf))
        assert got >= 0
        return self.buf.value.decode().split("\n")[:-1]

    def generation(self, shape, step, carry, listed=()):
        """-> (launches, flags); carry (a list) is stepped in place"""
        st, ca, fl = (ctypes.c_longlong * 6)(*step), (ctypes.c_longlong * 6)(*carry), (ctypes.c_longlong * 20)()
        got = self.L.generation((ctypes.c_int * 30)(*shape), st, ca, (ctypes.c_int * max(1, len(listed)))(*listed), len(listed), fl, self.buf, len(self.buf))
        assert got >= 0
        carry[:] = list(ca)
        return self.buf.value.decode().split("\n")[:-1], dict(zip(FLAGS + ["L", "ngroups", "refuse"], fl))


@pytest.fixture(scope="module")
def sel(tmp_path_factory):
    cxx = next((c for c in ("g++", "c++", "clang++", "/opt/rocm/lib/llvm/bin/clang++") if shutil.which(c)), None)
    assert cxx, "no host C++ compiler"
    tmp = tmp_path_factory.mktemp("multi_select")
    src, lib = str(tmp / "select.cpp"), str(tmp / "libselect.so")
    with open(src, "w") as f:
        f.write(SOURCE % HEADER)
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", src, "-o", lib])      # (no HIP header on the include path)
    return Select(lib)


@pytest.fixture(scope="module")
def fixture():
    with open(FIXTURE) as f:
        return json.load(f)


CARRY0 = [0, -1, 0, -1, -1, 1]          # MultiCarry's defaults: what dz_reset leaves


def replay(sel, en, c):
    """-> [(piece, generation, recorded signature, launches from the plans, flags)] for every generation of the case, the carry stepped here"""
    from tests import multi_select_cases as XC
    shape, carry, g, ntrace, out = en["shape"], list(CARRY0), 0, 0, []
    nl = shape[FIELDS.index("nl")]
    for piece, (m, ran) in enumerate(zip(XC.pieces(c), en["ran"])):
        sigs = [en["sigs"][j] for count, j in ran["gens"] for _ in range(count)]
        assert len(sigs) == m
        if c["range"] is None:
            carry[4] = -1                                      # dz_step forgets a proposal set made ahead
        for i, sig in enumerate(sigs):
            step = [0, nl, g, 1, int(i + 1 < m), ntrace] if c["range"] is None else [c["range"][0], c["range"][1], g, 0, 0, ntrace]
            listed = [int(ln.split()[2]) for ln in sig if ln.startswith("R ")]
            got, flags = sel.generation(shape, step, carry, listed)
            out.append((piece, g, sig, ["G %d %d %d %d" % (step[0], step[1], step[3], step[4])] + got, flags))
            g += 1
    return out


def test_fixture_covers_what_it_was_designed_to(sel, fixture):
    from tests import multi_select_cases as XC
    cases = XC.cases()
    assert fixture["shape_fields"] == FIELDS
    assert len(fixture["entries"]) == len(cases) >= 70
    assert os.path.getsize(FIXTURE) < 400 * 1024
    flags, kernels = {f: set() for f in FLAGS}, set()
    for en, c in zip(fixture["entries"], cases):
        assert en["case"] == XC.brief(c)
        assert len(en["ran"]) == len(XC.pieces(c)) and [sum(n for n, _ in r["gens"]) for r in en["ran"]] == list(XC.pieces(c))
        kernels |= {ln.split("@")[0] for sig in en["sigs"] for ln in sig[1:]} | {ln.split("@")[0] for r in en["ran"] for ln in r["pre"]}
        for _, _, _, _, fl in replay(sel, en, c):
            for f in FLAGS:
                flags[f].add(bool(fl[f]))
    # every family of logp_plan with every value of its template arguments the list was designed to reach ...
    for want in ("k_logp_mvn_lds<1,true>", "k_logp_mvn_lds<1,false>", "k_logp_mvn_mfma<1,8,false>", "k_logp_mvn_mfma<2,8,false>", "k_logp_mvn_mfma_tiled<2,4>", "k_logp_mvn_gemm<1>",
                 "k_logp_mvn_gemm<2>", "k_logp_mvn_gemm<4>", "k_logp_mix<1>", "module", "k_sum_items", "k_q_finish", "k_prior_only<1>", "k_prior_only<4>", "k_prior_add<1>",
                 "k_propose<1>", "k_propose<2>", "k_propose<4>", "k_propose<8>", "k_propose_stream", "k_accept<1>", "k_accept<8>", "k_accept_propose<4>", "k_accept_propose<8>",
                 "k_redo_flags", "k_gather_sets", "k_scatter_logp", "k_pt_swap<1>", "k_pt_swap<4>", "k_draws"):
        assert want in kernels, want
    assert any(ln.startswith("R ") for en in fixture["entries"] for sig in en["sigs"] for ln in sig)          # redraw rounds that found chains
    # ... and every flag of generation_plan in both states
    for f in FLAGS:
        assert flags[f] == {False, True}, f
    shapes = [dict(zip(FIELDS, en["shape"])) for en in fixture["entries"]]
    for f, want in (("nlanes", {1, 2}), ("lk", {1, 2, 3, 4}), ("lk_lanes", {1, 16, 64}), ("lk_items", {1, 2}), ("redo_possible", {0, 1}), ("adapt", {0, 1}), ("tempering", {0, 1}),
                    ("adapt_lag", {0, 1}), ("propose_split", {0, 2, 8}), ("q_defer", {0, 1}), ("logp_gemm", {0, 1}), ("nch", {1, 2, 4, 8}), ("tri", {0, 1}), ("have_prior", {0, 1})):
        assert {s[f] for s in shapes} == want, f


def test_pure_functions_reproduce_every_recorded_launch(sel, fixture):
    from tests import multi_select_cases as XC
    checked = 0
    for en, c in zip(fixture["entries"], XC.cases()):
        nl = en["shape"][FIELDS.index("nl")]
        for piece, ran in enumerate(en["ran"]):          # what precedes a piece's first generation: the evaluation of the start states, once
            assert ran["pre"] == (sel.logp(en["shape"], nl) if piece == 0 else []), (en["case"], piece)
        for piece, g, sig, got, flags in replay(sel, en, c):
            assert got == sig, (en["case"], piece, g, flags)
            assert not flags["refuse"]
            checked += 1
    assert checked == sum(sum(XC.pieces(c)) for c in XC.cases())


def test_the_sweep(sel):
    assert sel.L.lds_limit() == 160 * 1024
    plans = sel.L.sweep()
    assert plans > 0, sel.L.why().decode()
    assert plans > 10_000_000
