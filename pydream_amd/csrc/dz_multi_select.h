// dz_multi_select.h -- the multi-kernel path (one_generation, eval_logp, redraw_impossible_sets in dz_engine.hip): which kernels a generation launches, with what
// template arguments, grid, block and LDS size, as pure functions of plain structs, and the LDS carvings of the two kernels of this path that take dynamic LDS.
// No HIP header: the kernels (dz_kernels.h), the engine and a host-only test (tests/test_multi_select_cpu.py) compile the same lines.
//
//   logp_plan(MultiShape, n, defer_finish) -> LogpPlan                    one eval_logp call on n points
//   generation_plan(MultiShape, MultiStep, MultiCarry) -> GenerationPlan  one generation; GenerationPlan::next is the carry of the one behind it
//   redraw_plan(MultiShape, nc, listed, round) -> RedrawPlan              the redraw rounds queued behind one read-back of the flags
#pragma once
#include "dz_mega_select.h"      // LDS_LIMIT, DZ_SELECT_HD

namespace dz {

// ---- LDS carvings (doubles) ------------------------------------------------------------------------------------------------------------------------
// k_logp_mvn_lds: matrix (packed triangle, or the square of 4 ceil(d / 4) k-rows) | mean | one padded tile of 16 points per wave
struct LogpLdsLayout { int off_mu, off_tiles, tile, total; };
DZ_SELECT_HD inline LogpLdsLayout logp_lds_layout(int d, int ld, bool tri, int mtp_len, int nwv)
{
    LogpLdsLayout L;
    L.off_mu = tri ? mtp_len : 4 * ((d + 3) / 4) * ld;
    L.off_tiles = L.off_mu + ld;
    L.tile = 16 * (ld + 1);          // padded tile row: the A-layout reads hit distinct banks
    L.total = L.off_tiles + nwv * L.tile;
    return L;
}
// k_accept_propose: the chain's new state | 64 draws (uint4) | the chain's decisions (ChainCtl).  The two HIP types enter by size (dz_kernels.h pins them).
constexpr int MULTI_UINT4_BYTES = 16, MULTI_CHAINCTL_BYTES = 32;
struct AcceptProposeLayout { int off_draws, off_ctl, total; };
DZ_SELECT_HD inline AcceptProposeLayout accept_propose_layout(int ld)
{
    AcceptProposeLayout L;
    L.off_draws = ld;
    L.off_ctl = L.off_draws + 64 * MULTI_UINT4_BYTES / 8;
    L.total = L.off_ctl + MULTI_CHAINCTL_BYTES / 8;
    return L;
}

// ---- the shape -------------------------------------------------------------------------------------------------------------------------------------
// Every fact this path's selection reads that does not change within a dz_step or dz_step_range, and nothing else (multi_shape in dz_engine.hip fills it).
enum { MULTI_LK_MVN = 1, MULTI_LK_MIX = 2, MULTI_LK_HOST = 3, MULTI_LK_MODULE = 4 };      // the engine's likelihood kinds (LK_*)
struct MultiShape {
    int d, ld, k, depairs, nslots, nch;                      // nch: 128-dimension chunks a wave's lanes cover (1, 2, 4, 8: the kernels' NCH)
    bool tri; int mtp_len; bool mu_zero, have_prior;
    int nl, N, ncu, nlanes;                                  // local chains, all chains, compute units, stream groups
    int lk, lk_lanes, lk_items;
    bool redo_possible;                                      // a whole proposal set can be impossible (redraw rounds, Dream.py:281-289)
    bool adapt, tempering; int world, thin, burnin, history_lag, adapt_lag; bool adapt_groups, trace;
    int propose_split; bool q_defer, logp_gemm;              // DZ_PROPOSE_SPLIT (0: by shape), DZ_QFIN, DZ_LOGP_GEMM
    bool prior_ext = false;                                  // dz_set_prior_ext with a kind above 2: have_prior is false, the built-in kernels write a zero prior, k_prior_ext adds every dimension's
};

// The kernels of this path and the block size each is compiled for (__launch_bounds__; 1024 where it has none).
enum MultiKernel { MK_DRAWS, MK_PROPOSE, MK_PROPOSE_STREAM, MK_ACCEPT, MK_ACCEPT_PROPOSE, MK_LOGP_LDS, MK_LOGP_MFMA, MK_LOGP_TILED, MK_LOGP_GEMM, MK_LOGP_MIX, MK_Q_FINISH,
                   MK_PRIOR_ONLY, MK_PRIOR_ADD, MK_SUM_ITEMS, MK_MODULE, MK_REDO_FLAGS, MK_GATHER_SETS, MK_SCATTER_LOGP, MK_PRIOR_EXT, MK_COUNT };
inline int multi_max_threads(MultiKernel kern, int nch)
{
    switch (kern) {
        case MK_PROPOSE: return nch >= 4 ? 256 : 1024;
        case MK_LOGP_LDS: return 512;
        case MK_PROPOSE_STREAM: case MK_LOGP_MFMA: case MK_LOGP_TILED: case MK_LOGP_GEMM: case MK_LOGP_MIX: case MK_PRIOR_ONLY: case MK_PRIOR_ADD: case MK_PRIOR_EXT: case MK_MODULE: return 256;
        default: return 1024;      // (k_accept, k_accept_propose: a wave per try -- fused only up to 16 tries)
    }
}
struct MultiLaunch { unsigned grid, block; size_t lds; };
inline unsigned multi_blocks(long long n, long long per) { return (unsigned)((n + per - 1) / per); }

// ---- one eval_logp call ----------------------------------------------------------------------------------------------------------------------------
enum LogpFamily { LOGP_NONE = 0, LOGP_LDS, LOGP_MFMA, LOGP_TILED, LOGP_GEMM, LOGP_MIX, LOGP_MODULE, LOGP_HOST };
struct LogpPlan {
    LogpFamily family;
    int nrt; bool tri; int pt, gemm_tile;      // the template arguments: row tiles, tri / dense, point tiles per wave (MFMA 1 / 2; tiled: 2), GEMM tile 1 / 2 / 4 (x 32 points)
    int nwv;                                   // LDS kernel: waves per block
    MultiLaunch main;                          // the family's kernel (module: of the user's kernel; host: none)
    bool one_kernel;                           // the LDS kernel alone: timed by the launch's own events, not by the enclosing scope
    bool q_finish, prior_only, prior_add, sum_items;
    MultiLaunch finish, prior, sum;            // k_q_finish; k_prior_only / k_prior_add; k_sum_items
    int nrtb; size_t qpart_doubles;            // tiled families: row tiles of d, doubles of the row-tile sums
    unsigned per_block; long long items; bool grid_overflow; size_t scratch_doubles;      // module: points (items) per block, the item count, more items than one grid holds, the items' scratch
    bool prior_ext, ext_fix_like; MultiLaunch ext;      // k_prior_ext, last of the call, in the place of k_prior_only / k_prior_add; ... which also maps the likelihood column's nan, as k_prior_add would have
};
constexpr int TILED_PT = 2, TILED_RTC = 4;      // k_logp_mvn_mfma_tiled: point tiles x row tiles per wave

inline size_t logp_lds_bytes(const MultiShape& s, int nwv) { return sizeof(double) * (size_t)logp_lds_layout(s.d, s.ld, s.tri, s.mtp_len, nwv).total; }

inline LogpPlan logp_plan(const MultiShape& s, int n, bool defer_finish)
{
    LogpPlan P = {};
    if (n <= 0) return P;
    P.nrt = s.ld / 16; P.tri = s.tri;
    P.prior = {multi_blocks(n, 4), 256u, 0};
    if (s.lk == MULTI_LK_MVN) {
        const int ntiles = (n + 15) / 16;
        // LDS kernel: matrix (packed triangle or square) + mean + at least 4 wave tiles must fit 160 KB
        // (the dense 128-D square does not: 131 KB + 66 KB; it runs on the register-operand MFMA kernel)
        if (P.nrt <= 8 && logp_lds_bytes(s, 4) <= LDS_LIMIT) {
            P.family = LOGP_LDS;
            // one wave per point tile of the CU's share when LDS allows (4..8 waves): 1280 tiles on 256 CUs run as
            // 5-wave blocks instead of 4-wave blocks of which a quarter does a second tile
            int nwv = (ntiles + s.ncu - 1) / s.ncu;
            nwv = nwv < 4 ? 4 : (nwv > 8 ? 8 : nwv);
            while (nwv > 4 && logp_lds_bytes(s, nwv) > LDS_LIMIT) --nwv;
            const int blocks = (ntiles + nwv - 1) / nwv;
            P.nwv = nwv;
            P.main = {(unsigned)(blocks < s.ncu ? blocks : s.ncu), 64u * nwv, logp_lds_bytes(s, nwv)};
            P.one_kernel = !s.have_prior;
        } else if (P.nrt <= 8) {
            P.family = LOGP_MFMA;
            P.pt = ntiles > 1024 ? 2 : 1;   // 1024 SIMDs: share B operands between two point tiles once every SIMD has work
            P.main = {multi_blocks(n, 64 * P.pt), 256u, 0};
        } else {
            // tiled product: waves = point-tile groups x row-tile groups; per-row-tile sums through a scratch array
            P.nrtb = (s.d + 15) / 16; P.pt = TILED_PT;
            P.qpart_doubles = (size_t)n * P.nrtb;
            if (s.logp_gemm && n >= 512) {            // enough points to fill the chip with 64 x 64 block tiles
                P.family = LOGP_GEMM;
                const int nbn = (P.nrtb * 16 + 63) / 64;
                // Points per block (128 / 64 / 32): the kernel is bound by how many blocks a CU has in flight (each one is a
                // chain of barrier -> LDS reads -> MFMAs -> LDS store), so the largest tile that still leaves five blocks per
                // CU: 2560 points x 1000 rows: 32 points 65 us, 64 points 70 us, 128 points 98 us per launch.
                const int bm = ((n + 127) / 128) * nbn >= 5 * s.ncu ? 128 : ((n + 63) / 64) * nbn >= 5 * s.ncu ? 64 : 32;
                P.gemm_tile = bm / 32;
                P.main = {(unsigned)(((n + bm - 1) / bm) * nbn), 256u, s.mu_zero ? 0 : sizeof(double) * (size_t)s.ld};
            } else {
                P.family = LOGP_TILED;
                const int nrg = (P.nrtb + TILED_RTC - 1) / TILED_RTC, npg = (n + 16 * TILED_PT - 1) / (16 * TILED_PT);
                P.main = {multi_blocks((long long)npg * nrg, 4), 256u, 0};
            }
            P.q_finish = !defer_finish;
            P.finish = {multi_blocks(n, 64), 64u, 0};
        }
        P.prior_only = s.have_prior;
    } else if (s.lk == MULTI_LK_MIX) {
        P.family = LOGP_MIX;
        P.main = P.prior;
    } else if (s.lk == MULTI_LK_MODULE) {
        // the user's kernel writes like[n]; the engine zeroes prior[n] first and then adds the device priors and maps nan -> -inf (k_prior_add),
        // exactly what follows a host callback
        P.family = LOGP_MODULE;
        P.per_block = 256u / (unsigned)s.lk_lanes;      // 1, 16, 32 or 64 lanes per point, 256 threads per block
        // several items per point (dz_set_likelihood_items): the kernel's n is the item count and its like the engine's scratch, item w
        // of it belonging to point w / C; k_sum_items then leaves each point's sum where a one-item kernel would have written
        P.items = (long long)n * s.lk_items;
        const long long blocks = (P.items + P.per_block - 1) / P.per_block;
        P.sum_items = s.lk_items != 1;
        P.grid_overflow = P.sum_items && blocks > 0x7fffffffll;
        P.scratch_doubles = P.sum_items ? (size_t)P.items : 0;
        P.main = {(unsigned)blocks, 256u, 0};
        P.sum = {multi_blocks(n, 256), 256u, 0};
        P.prior_add = true;
    } else if (s.lk == MULTI_LK_HOST) {
        P.family = LOGP_HOST;
        P.prior_add = true;
    }
    if (s.prior_ext && P.family != LOGP_NONE) {
        // extended priors: the family's kernels have written prior = 0 (have_prior is false; a host callback: its own prior column); one launch adds every
        // dimension's prior where k_prior_only / k_prior_add would have run -- for the MVN kernels, k_logp_mix, the host callback, a module kernel (after k_sum_items)
        P.prior_ext = true; P.ext_fix_like = P.prior_add; P.ext = P.prior;
        P.prior_only = false; P.prior_add = false; P.one_kernel = false;
    }
    return P;
}

// ---- one generation --------------------------------------------------------------------------------------------------------------------------------
// waves per k_propose / k_accept block: 16 (one block fills a CU's 4 SIMDs evenly) once there is at least one such block per CU
inline int multi_wpb(const MultiShape& s, int chains_per_group) { return s.nch >= 4 ? 4 : (chains_per_group >= 16 * s.ncu ? 16 : 4); }    // (k_propose<NCH >= 4> is built for 4-wave blocks)
// waves per chain in k_propose: one wave per (chain, try) pays when a try is long and the chains are few: d > 512 (measured at 512 x 1000-D: +17%;
// at d <= 200 the per-chain wave with its fused Metropolis step is faster)
inline int multi_split(const MultiShape& s) { return s.propose_split > 0 ? s.propose_split : (s.nch >= 8 ? s.k : 1); }
inline int multi_clamp(int v, int hi) { return v > hi ? (hi < 1 ? 1 : hi) : (v < 1 ? 1 : v); }

struct MultiStep { int c0, nc; unsigned g; bool traced, more_follow; long long ntrace; };      // ntrace: trace rows written so far (the slot a traced generation takes)
// what a generation leaves for the next one
struct MultiCarry {
    bool pending_accept = false;      // the generation's Metropolis step has been deferred into the next proposal kernel
    long long pending_slot = -1;      // ... its trace slot
    bool pending_qfin = false;        // ... and with it the reference set's row-tile sums, still in the scratch array
    long long draws_gen = -1;         // the generation whose draws and decisions the accept kernel has already made
    long long stream_prop_gen = -1;   // the generation whose proposal set k_accept_propose has already made
    bool need_join = true;            // shared state changed: the stream groups meet before anything reads it
};
enum { PROP_NONE = 0, PROP_STREAM, PROP_FUSED_ACCEPT, PROP_CHAIN };      // phase-0 proposal launch: made already / k_propose_stream / k_propose with the accept of g - 1 in front / k_propose
enum { ACC_NONE = 0, ACC_ACCEPT, ACC_ACCEPT_PROPOSE };                   // deferred into the next generation / k_accept / k_accept_propose
enum { REFUSE_NONE = 0, REFUSE_SHARDED, REFUSE_HISTORY_LAG, REFUSE_ADAPT_LAG };
struct MultiGroup {               // one stream group's share of the generation
    int stream, c0, nc, n0, n1;   // its stream, its chains, the points of its two eval_logp calls (proposal set, reference set)
    MultiLaunch draws, prop0, prop1, accept;
};
struct GenerationPlan {
    int refuse;
    bool full; int L, wpb, split, sp0, sp1; long long slot; int nrows;
    bool streamed, redo, have_prop, fused_in, need_draws, append, publish, fuse_next, defer, qdefer, prep_next;      // (prep_next: k_accept makes the next generation's draws and decisions)
    bool join_first, own_probs, publish_start, exchange_positions, join_last, swap, swap_join;      // the groups meet before the generation; single-chain view with adaptation; start positions published; they meet behind it; temperature swap; ... before it
    int prop0, acc;               // PROP_*, ACC_*
    int ngroups; MultiGroup grp[8];
    MultiCarry next;
};

inline GenerationPlan generation_plan(const MultiShape& s, const MultiStep& t, const MultiCarry& c)
{
    GenerationPlan P = {};
    const int k = s.k;
    P.full = t.c0 == 0 && t.nc == s.nl;
    if (!P.full) P.refuse = s.world > 1 ? REFUSE_SHARDED : s.history_lag ? REFUSE_HISTORY_LAG : s.adapt_lag ? REFUSE_ADAPT_LAG : REFUSE_NONE;
    if (P.refuse) return P;
    P.redo = s.redo_possible;         // (then the proposal set's evaluation is followed by a check on the host: nothing is deferred)
    P.L = (P.full && s.lk != MULTI_LK_HOST && !P.redo) ? s.nlanes : 1;     // the host-callback likelihood is synchronous anyway; redraw rounds use shared buffers
    P.join_first = c.need_join || !P.full;
    P.own_probs = !P.full && s.adapt;
    P.publish_start = P.full && t.g == 0 && s.adapt;      // (Dream_shared_vars.current_positions)
    P.fused_in = P.full && c.pending_accept;                                             // generation g-1's accept rides in front of this phase-0 kernel
    P.need_draws = !P.fused_in && (!P.full || c.draws_gen != (long long)t.g);            // not prepared by the accept of the previous generation
    P.append = (t.g % (unsigned)s.thin) == 0;                                            // Dream.py:360
    P.publish = s.adapt && (long long)t.g < (long long)s.burnin + 1;                     // Dream.py:364
    P.nrows = P.full ? s.N : t.nc;
    P.prep_next = P.full && !P.publish;      // while adapting, next generation's decisions must wait for the new probabilities
    P.wpb = multi_wpb(s, t.nc / P.L);
    P.split = multi_split(s);
    P.sp0 = multi_clamp(P.split, k); P.sp1 = multi_clamp(P.split, k - 1);
    P.slot = (t.traced && s.trace) ? t.ntrace : -1;
    // ld > 256, one DE pair, multi-try: one wave per (chain, try) streaming over the dimension chunks (dz_kernels.h)
    P.streamed = s.nch >= 4 && s.depairs == 1 && k >= 3 && !P.redo;     // (redraw rounds go through k_propose)
    P.have_prop = P.streamed && P.full && c.stream_prop_gen == (long long)t.g;
    // the Metropolis step of this generation can ride in front of the next generation's proposal kernel when
    // nothing shared changes in between (no history append, no published positions, no temperature swap) and a generation follows ...
    const bool quiet = P.full && t.more_follow && !P.append && !P.publish && !s.tempering;
    P.defer = quiet && !P.streamed && P.split == 1 && s.lk != MULTI_LK_HOST && !P.redo;
    // ... and the streamed form of the same: accept(g) + proposal set(g+1) in one launch (k_accept_propose, a wave per try)
    P.fuse_next = quiet && P.streamed && k <= 16;
    // large d: the row-tile sums of the likelihood product are added by the kernels that use them (no k_q_finish launches)
    // (round 5: also the per-chain proposal kernels of 128 < d <= 256 -- the reference example's own d = 200 --: two launches of six fewer)
    const bool tiled_mvn = s.lk == MULTI_LK_MVN && s.ld / 16 > 8;
    const bool chain_sums = P.full && k >= 3 && !P.redo && s.nch < 4 && s.nlanes == 1;
    P.qdefer = s.q_defer && tiled_mvn && (P.streamed || chain_sums) && !s.prior_ext;      // (the kernels that finish deferred sums write a zero prior beside them)
    P.prop0 = (P.streamed && P.have_prop) ? PROP_NONE : (P.streamed && !P.fused_in) ? PROP_STREAM : P.fused_in ? PROP_FUSED_ACCEPT : PROP_CHAIN;
    P.acc = P.fuse_next ? ACC_ACCEPT_PROPOSE : P.defer ? ACC_NONE : ACC_ACCEPT;
    for (int g = 0; g < P.L; ++g) {
        const int lc0 = t.c0 + (int)((long long)t.nc * g / P.L), lc1 = t.c0 + (int)((long long)t.nc * (g + 1) / P.L), lnc = lc1 - lc0;
        if (lnc <= 0) continue;
        MultiGroup& q = P.grp[P.ngroups++];
        q.stream = g; q.c0 = lc0; q.nc = lnc; q.n0 = lnc * k; q.n1 = lnc * (k - 1);
        q.draws = {multi_blocks((long long)lnc * s.nslots, 256), 256u, 0};
        const unsigned pb = 64u * P.wpb;
        if (P.prop0 == PROP_STREAM) q.prop0 = {multi_blocks((long long)lnc * k, 4), 256u, 0};
        else if (P.prop0 == PROP_FUSED_ACCEPT) q.prop0 = {multi_blocks(lnc, P.wpb), pb, 0};
        else if (P.prop0 == PROP_CHAIN) q.prop0 = {multi_blocks((long long)lnc * P.sp0, P.wpb), pb, 0};
        if (k > 1) q.prop1 = P.streamed ? MultiLaunch{multi_blocks((long long)lnc * (k - 1), 4), 256u, 0} : MultiLaunch{multi_blocks((long long)lnc * P.sp1, P.wpb), pb, 0};
        if (P.acc == ACC_ACCEPT_PROPOSE) q.accept = {(unsigned)lnc, 64u * k, sizeof(double) * (size_t)accept_propose_layout(s.ld).total};
        else if (P.acc == ACC_ACCEPT) q.accept = {multi_blocks(lnc, P.wpb), pb, 0};
    }
    P.exchange_positions = P.publish && P.full && !s.adapt_groups;      // (ranks that own whole groups of chains exchange their groups' sums instead)
    P.join_last = (P.publish || P.append) && P.L > 1;
    P.swap = s.tempering && P.full;      // temperature swap (core.py:185-221): after every chain's step and the updates above
    P.swap_join = P.swap && P.L > 1;
    P.next.stream_prop_gen = P.fuse_next ? (long long)t.g + 1 : -1;
    P.next.pending_accept = P.defer; P.next.pending_slot = P.defer ? P.slot : -1;
    P.next.pending_qfin = P.defer && P.qdefer && k > 1;      // (one stream group when deferred sums are in play: chain_sums)
    P.next.draws_gen = P.prep_next ? (long long)t.g + 1 : -1;
    P.next.need_join = P.publish || P.append || P.swap_join;
    return P;
}

// ---- redraw rounds ---------------------------------------------------------------------------------------------------------------------------------
// nc: the chains of the (one) stream group; listed: how many of them the read-back found with every try impossible; round: the first round to queue (1 ..)
constexpr int MULTI_MAX_REDRAWS = 64;      // DZ_MAX_REDRAWS (dreamzs.h; the engine pins it)
struct RedrawPlan { int batch, sp0, points; MultiLaunch flags, propose, gather, scatter; };      // rounds queued; k_propose's waves per chain; points evaluated per round
inline RedrawPlan redraw_plan(const MultiShape& s, int nc, int listed, int round)
{
    RedrawPlan R = {};
    const int wpb = multi_wpb(s, nc), sp0 = multi_clamp(multi_split(s), s.k), left = MULTI_MAX_REDRAWS - round + 1, want = listed >= 16 ? 4 : (listed >= 4 ? 3 : 2);
    // up to four rounds per read-back (chains that succeed in between drop out by their flag)
    // (a host likelihood costs more than a round trip: one round per read-back, no point is evaluated that did not have to be)
    R.batch = s.lk == MULTI_LK_HOST ? 1 : (left < want ? left : want);
    R.flags = {multi_blocks(nc, 256), 256u, 0};
    R.propose = {multi_blocks((long long)listed * sp0, wpb), 64u * wpb, 0};
    R.gather = {multi_blocks((long long)listed * s.k * s.ld / 2, 256), 256u, 0};
    R.scatter = {multi_blocks((long long)listed * s.k, 256), 256u, 0};
    R.sp0 = sp0; R.points = listed * s.k;
    return R;
}

}  // namespace dz
