// dz_mega_select.h -- which instantiation of the persistent generation kernels runs, with what grid, block and LDS size: the LDS layout arithmetic the
// kernels and the host share, and the selection as two pure functions of plain structs.  No HIP header: the kernels (dz_kernels.h, dz_megakernel.h), the
// engine (dz_engine.hip) and a host-only test (tests/test_mega_select_cpu.py) compile the same lines.
//
//   mega_choose(MegaShape) -> MegaChoice                              once per dz_step: eligibility, family, block plan, burn-in mode
//   mega_launch_plan(MegaChoice, MegaShape, publish, applies) -> ...  once per launch: per part grid, block, LDS bytes and the launcher's flags
#pragma once
#include <stddef.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define DZ_SELECT_HD __host__ __device__
#else
#define DZ_SELECT_HD
#endif

namespace dz {

constexpr int MAXK = 32;      // multitry limit (tries 17..32: the multi-kernel path; the persistent kernels hold a generation's draw slots in one wave's lanes: multitry <= 15)
constexpr int MEGA_CHAINS = 16;      // chains (= waves) per block at full size; 8 or 4 when there are too few chains to give every CU a block
constexpr size_t LDS_LIMIT = 160 * 1024;      // bytes of LDS a block of any kernel may ask for (gfx950)

// Output cursors of the <.., KC, PLAIN> instantiations: where a chain's stores of generation index 0 go, as 64-bit byte addresses in LDS.  What a chain writes per
// generation moves by a launch constant (a trace row: ld doubles; a history append: N rows; a scalar column: nl elements), so the prologue builds each address
// once and the generation loop adds index x stride -- no 64-bit address is rebuilt from kernel arguments and Params fields that would have to live in scalar
// registers (or their spill lanes) across the whole loop.  Per chain: the trace row | the append row (for an archive of 0 rows: + M rows at use) | the state row |
// the five scalar trace columns (log p, moved, try, CR index, snooker) | log prior | log likelihood.  Per block: the chain count nl, the columns' stride (one word
// and one of padding: the area stays a whole number of 16-byte pairs).
constexpr int MEGA_CUR_WORDS = 10, MEGA_CUR_BLOCK = 2;

// offset of k-row r in the packed triangular layout: row block b = r/16 has 16*(b+1) columns
DZ_SELECT_HD inline int tri_row_offset(int r) { const int b = r >> 4; return 128 * b * (b + 1) + (r - 16 * b) * 16 * (b + 1); }

struct MegaLayout { int LDM, LDP, rows, off_P, off_q, off_sP, off_sS, off_sL, off_rP, off_rS, off_mu, off_pr, off_st, off_dec, off_gt, off_X, off_pc, pcn, off_Xo, off_tab, off_cur, total; };

// point rows of a block: try i of chain c at row i*ch + c; tiles are 16 consecutive rows, from row 0 (k tries) or from
// row ch (the k-1 reference tries); rows past the last point stay zero
DZ_SELECT_HD inline int mega_rows(int k, int ch)
{
    const int a = 16 * ((k * ch + 15) / 16), b = ch + 16 * (((k - 1) * ch + 15) / 16);
    return a > b ? a : b;
}
// pb: room for the per-dimension prior / boundary constants of the full-code instantiations (PBConsts: five double arrays and one int
// array of pcn = 16 nrt entries)
// xo: room for the chains' states as they were at the start of the launch (crossover burn-in: the block's adaptation sums need the jumps)
// nomat: the matrix is NOT staged (k_generations_d2, 128 < d <= 256: it does not fit next to the point tiles and is read from L2)
// ntab: rows of the table of crossover / gamma-level probabilities per generation of the launch (adapt_lag >= 1: several burn-in generations per
// launch, the MG instantiations; rows of (ncr + ngamma + 1) & ~1 doubles)
// cur (k_generations<.., KC, PLAIN>): room for the launch's output cursors -- MEGA_CUR_WORDS 64-bit words per chain and MEGA_CUR_BLOCK for the block (see the kernel's prologue)
// sp (k_generations_d2<.., SP>, round 6): the proposal set goes through the point tiles in two passes (tries 0 .. k-2, then the last one), the selected
// proposal stays in registers: k - 1 tries' rows instead of k
DZ_SELECT_HD inline MegaLayout mega_layout(int d, int k, int nrt, int ncr, int ngamma, bool tri, bool xlds, int ch = MEGA_CHAINS, bool pb = false, bool xo = false, bool nomat = false, int ntab = 0,
                                           bool sp = false, bool cur = false)
{
    MegaLayout L;
    const int ks4 = 4 * ((d + 3) / 4);
    L.LDM = d + 2;                    // dense matrix row (k index c): d entries + pad; rows d..ks4-1 are zero
    L.LDP = ks4 + 1;                  // point row: zero padded to the k-steps; odd stride keeps the A-layout reads (16 rows x 4 cols) off one bank
    L.off_P = nomat ? 0 : (tri ? tri_row_offset(ks4) : ks4 * L.LDM + 16);       // (+16: the last row tile's column reads run past the last row's end)
    L.rows = sp ? 16 * (((k - 1) * ch + 15) / 16) : mega_rows(k, ch);
    L.off_q = L.off_P + L.rows * L.LDP;
    L.off_sP = L.off_q + L.rows * nrt;
    L.off_sS = L.off_sP + ch * k;
    L.off_sL = L.off_sS + ch * k;
    L.off_rP = L.off_sL + ch * k;
    L.off_rS = L.off_rP + ch * k;
    L.off_mu = L.off_rS + ch * k;
    L.off_pr = L.off_mu + ks4 + 4;               // (mu zero padded to the k-steps) crossover / gamma-level probabilities
    L.off_st = L.off_pr + ncr + ngamma + 2 - ((ncr + ngamma) & 1);      // (the offsets behind stay even; one word of the gap: the log prior of a point inside every uniform support, PBConsts::inside) per chain: lprior, llike, sel|fin
    L.off_dec = L.off_st + 4 * ch;      // per chain and generation: u_sel, u_acc, snooker, CR index, gamma level
    L.off_gt = L.off_dec + 8 * ch;      // gamma_arr[level-1][0][:]
    L.off_X = L.off_gt + ngamma * d + (d & 1);   // chain states (XLDS)
    L.total = L.off_X + (xlds ? ch * L.LDP : 0);
    L.total += L.total & 1;
    L.off_pc = L.total; L.pcn = 16 * nrt;
    if (pb) L.total += 5 * L.pcn + L.pcn / 2;
    L.total += L.total & 1;
    L.off_Xo = L.total;
    if (xo) L.total += ch * L.LDP + ((ch * L.LDP) & 1);
    L.off_tab = L.total;
    L.total += ntab * ((ncr + ngamma + 1) & ~1);
    L.off_cur = L.total;
    if (cur) L.total += MEGA_CUR_WORDS * ch + MEGA_CUR_BLOCK;
    return L;
}

// the mixture / user kernels (k_generations_mix, k_generations_user): doubles of LDS per wave
constexpr int MIXW = 4;       // waves (= chains) per block
DZ_SELECT_HD inline int mega_mix_wave_doubles(int d, int k, int J) { const int n = k * (4 * ((d + 3) / 4) + 1) + 6 * k + k * J + 8; return n + (n & 1); }

// ---- the selection ---------------------------------------------------------------------------------------------------------------------------------
// Every fact the selection reads, and nothing else (the engine fills it in one place: mega_shape in dz_engine.hip).
enum { MEGA_LK_MVN = 1, MEGA_LK_MIX = 2, MEGA_LK_MODULE = 4 };      // the engine's likelihood kinds (LK_*) that have persistent kernels
struct MegaShape {
    int d, ld, k, depairs, npt, nslots, ncr, ngamma, J;
    bool tri, mtp, hard, have_prior;         // triangular factor; its packed copy exists (Params::Mtp); hard boundaries; any prior
    int nl, N, ncu;                          // local chains, all chains, compute units
    int lk, lk_items; bool gen_fn[4];        // likelihood kind; items per point; the user's code object has dz_user_generations [wide ? 2 : 0) + (full ? 1 : 0)]
    bool redo_possible;                      // a whole proposal set can be impossible (redraw rounds, Dream.py:281-289)
    bool ad_multi; int ad_R1, ad_nbp, adapt_lag; bool adapt_fused, adapt_groups, tempering; int world;
    bool mega; int mega_d2; bool mega_kc, mega_redo;      // the path switches (read_switches): DZ_MEGA, DZ_MEGA_D2, DZ_MEGA_KC, DZ_MEGA_REDO
    bool prior_ext = false;                               // dz_set_prior_ext with a kind above 2: no persistent kernel evaluates those (the multi-kernel path's k_prior_ext does)
};
enum MegaFamily { MEGA_NONE = 0, MEGA_CLASSIC, MEGA_W4, MEGA_D2, MEGA_MIX, MEGA_USER };
struct MegaChoice {
    MegaFamily family;                       // MEGA_NONE: not eligible, the multi-kernel path (W4: the first part is 4 chains x 4 waves with the tries' halves made ahead)
    bool need_x, pb, pb_lds, xlds, redo;     // need_x: priors / bounds / several pairs; pb: the full proposal code; its constants in LDS; chain states in LDS; redraw rounds in the kernel
    int ch, split_c, ch_b;                   // the block plan: chains per block of the (first) launch; local chains [0, split_c) in it, the rest in blocks of ch_b (split_c == nl: one launch)
    int d2_ch; bool d2_sp;                   // k_generations_d2: chains per block (0: not d2), the proposal set in two passes
    int wpc;                                 // waves per chain of the (first) launch
    int burnin;                              // adapt_lag >= 1, burn-in generations per launch: 0 one; 1 several, the blocks make their unit sums (MG); 2 several, through the ring of positions
};
// what mega_launch hands to the translation units' launchers (dz_mega_launch.h: MegaLaunch adds the HIP side)
struct MegaFlags {
    bool tri, xlds, pb, k1, redo;     // triangular factor / chain states in LDS / full proposal code (priors, bounds, DEpairs > 1) / multitry off / redraw rounds inside the kernel (with pb and multitry on)
    bool ahead = false;               // 4 chains x 4 waves, lean, multitry 3..6: k_generations_w4 (the tries' base-independent halves made ahead)
    bool d2 = false;                  // k_generations_d2 (the matrix read from L2)
    bool sp = false;                  // k_generations_d2, 16 chains per block whose proposal set goes through the point tiles in two passes (229..256 dimensions at 5 tries)
    bool multi = false;               // adapt_lag >= 1: several burn-in generations per launch (16 chains per block, one wave each, states in LDS: the MG instantiations)
    int kc = 0;                       // 5: multitry 5 and a launch that publishes nothing and adapts nothing (lean, 16 chains per block, one wave each, one launch per
                                      // generation run): the instantiation with the try count compiled in (k_generations' KC, PLAIN); 0: the generic one
    int ch, wpc;                      // chains per block (16, 12, 8, 4), waves per chain (1; 2 / 4 at 8 / 4 chains per block of k_generations_d2; 4 at 4 chains per block with multitry on)
};
struct MegaPart {
    int c0, c1;                       // the part's local chains
    unsigned grid, block; size_t lds;
    bool ring, fused, wide;           // the positions go to the ring (burn-in mode 2); the block makes its unit's adaptation sums; mixture / user: 128 < d <= 256
    MegaFlags f;
};
struct MegaLaunchPlan { int nparts; MegaPart part[2]; };

inline size_t mega_lds(const MegaShape& s, bool tri, bool xlds, int ch, bool pb = false, bool xo = false, bool nomat = false, int ntab = 0, bool sp = false, bool cur = false)
{
    return sizeof(double) * (size_t)mega_layout(s.d, s.k, s.ld / 16, s.ncr, s.ngamma, tri, xlds, ch, pb, xo, nomat, ntab, sp, cur).total;
}
inline bool mega_fits(size_t bytes) { return bytes <= LDS_LIMIT; }

// chains (= waves) per block: 16 once that still gives every CU a block, else 8 or 4 (C2: 1024 chains -> 256 blocks of 4); split_c / ch_b: a generation as TWO
// launches -- whole rounds of ch-chain blocks for the local chains [0, split_c), the remainder in blocks of ch_b chains
inline void mega_block_plan(const MegaShape& s, bool need_x, bool pb_lds, MegaChoice& c)
{
    // One block per CU is resident (LDS), so a launch takes ceil(blocks / CUs) rounds of a block's time; measured at 100-D a block of 12
    // chains needs 0.82 (round 6), one of 8 chains 0.67 and one of 4 chains (four waves per chain) 0.49 of the time of a block of 16.  The
    // smallest product wins, the larger block on a tie: 4096 chains -> 16, 3072 -> 12 (round 6: 256 blocks of 12 -- 677 M proposals/s; as
    // 192 blocks of 16, a quarter of the chip idle, 561), 2048 -> 8, 1024 -> 4 ... among the block sizes whose LDS layout fits at all (round
    // 4): at 113..128 dimensions the point tiles of 16 chains no longer fit next to the matrix, those of 8 do.
    // A chain count just above whole rounds -- 5000 chains: 313 blocks of 16 -- pays a whole round for its remainder; the remainder can go in
    // a SECOND launch of smaller blocks (whole rounds of the large blocks first).  The second launch's blocks start while the first one's
    // last blocks drain, worth about 0.12 of a 16-chain block's time (5000 chains: 16 + 8 measured 39.8 us per generation, modelled without
    // the overlap 46.4; 12 + 8: 40.0; 417 blocks of 12 in two rounds: 43.1).
    const int ncu = s.ncu > 0 ? s.ncu : 1;
    const int cand[4] = {16, 12, 8, 4};
    const double cost[4] = {1.0, 0.82, 0.67, 0.49};
    const bool k1 = s.k == 1;
    bool fits[4];
    for (int i = 0; i < 4; ++i)      // (the layout asked about has need_x, not pb: see mega_choose)
        fits[i] = !(cand[i] == 12 && k1) && mega_fits(mega_lds(s, s.tri, need_x, cand[i], need_x && pb_lds));
    c.ch = MEGA_CHAINS; c.split_c = s.nl; c.ch_b = 0; double tb = -1.0;
    for (int i = 0; i < 4; ++i) {
        if (!fits[i]) continue;
        const int ch = cand[i], blocks = (s.nl + ch - 1) / ch, rounds = (blocks + ncu - 1) / ncu;
        const double t = rounds * cost[i];
        if (tb < 0.0 || t < tb - 1e-9) { c.ch = ch; c.split_c = s.nl; c.ch_b = 0; tb = t; }
        if (k1 || ch < 12 || blocks <= ncu || blocks % ncu == 0) continue;
        const int full = (blocks / ncu) * ncu * ch, r = s.nl - full;
        for (int j = i + 1; j < 4; ++j) {
            if (!fits[j]) continue;
            const int rb = ((r + cand[j] - 1) / cand[j] + ncu - 1) / ncu;
            const double t2 = (blocks / ncu) * cost[i] + rb * cost[j] - 0.12;
            if (t2 < tb - 1e-9) { c.ch = ch; c.split_c = full; c.ch_b = cand[j]; tb = t2; }
        }
    }
}
// (round 6) k_generations_d2 whose k tries' point tiles do not fit but k - 1 do (16 chains per block: 229..256 dimensions at 5 tries): the proposal set in two
// passes (k_generations_d2<.., SP>); 3..15 tries, 128 < d
inline bool mega_d2_two_pass(const MegaShape& s, int ch)
{
    if (s.ld <= 128 || s.k < 3 || s.nslots > 64) return false;
    if (mega_fits(mega_lds(s, true, false, ch, false, false, true))) return false;
    return mega_fits(mega_lds(s, true, false, ch, false, false, true, 0, true));
}
// 128 < d <= 256 (the reference example's d = 200): k_generations_d2 -- configurations with the triangular factor (what
// MVNormalLogLike builds) whose point tiles of 16 chains fit LDS without the matrix (it is read from L2): d <= ~230 at 5 tries.  Measured and
// left on the multi-kernel path: the dense matrix (its 16-chain instantiation spills a hundred registers; at 8 chains per block 156 against 148 us
// at d = 200).  -> chains per block, 0: not this family
inline int mega_d2_chains(const MegaShape& s, bool need_x, bool pb_lds)
{
    if (!s.mega || !s.mega_d2 || s.lk != MEGA_LK_MVN || s.ld > 256) return 0;
    if (s.ld < 80 && s.nslots <= 64) return 0;
    // (round 6) more than 15 tries: a generation's draw slots exceed a wave's lanes, the classic kernels do not take them; this one keeps one phase's
    // slots at a time (k npt <= 64: up to 32 tries with one or two DE pairs)
    const bool bigk = s.nslots > 64;
    if (bigk && (s.k * s.npt > 64 || s.k > MAXK)) return 0;
    // d <= 128: only where the classic kernel's 16-chain layout (matrix in LDS) does not fit -- it then runs 8 chains per block (113..128 dimensions at 5 tries,
    // 100 dimensions at 8 or more)
    if (s.ld <= 128 && !bigk && (mega_fits(mega_lds(s, true, need_x, 16, need_x && pb_lds)) || s.k == 1)) return 0;
    if (s.mega_d2 == 1 && s.nl <= 1024) return 0;      // (64 blocks or fewer leave three CUs in four idle: 57 against 52 us per generation at 1024 x 200-D; DZ_MEGA_D2=2 forces it)
    if (s.redo_possible) return 0;      // (whole proposal sets that can be impossible: the multi-kernel path's redraw rounds)
    if (s.k != 1 && s.k < 3) return 0;
    if (!s.tri || !s.mtp) return 0;
    if (mega_fits(mega_lds(s, true, false, 16, false, false, true))) return 16;
    if (mega_d2_two_pass(s, 16)) return 16;
    // round 6: 8 chains x 2 waves per block where the point tiles of 16 chains do not fit (128 < d: 229..256 dimensions at 5 tries) -- multi-try only
    // (13..15 tries at 100 dimensions: the classic kernel would run 4 chains x 4 waves -- 603 M proposals/s at k = 15 against 693 for 8 x 2 here at k = 16)
    if (s.ld <= 128 && !bigk && mega_fits(mega_lds(s, true, need_x, 8, need_x && pb_lds))) return 0;
    if (s.k >= 3 && mega_fits(mega_lds(s, true, false, 8, false, false, true))) return 8;
    if (s.k >= 3 && mega_d2_two_pass(s, 8)) return 8;      // 8 x 2 with the two-pass set (256 dimensions at 8 tries)
    // ... and 4 chains x 4 waves where not even those fit (24..32 tries at 100 dimensions, 20..32 at 128, 8 at 256): four rounds of 1024 blocks at 4096
    // chains, still ahead of the multi-kernel path
    if (s.k >= 4 && mega_fits(mega_lds(s, true, false, 4, false, false, true))) return 4;
    return 0;
}
// adapt_lag >= 1, several burn-in generations in a launch whose blocks of 16 chains (= one unit) make their unit sums generation by generation (the MG
// instantiations): the wave regions / the layout, + the states before the generation, + the table of probabilities per generation
inline size_t mega_mix_multi_lds(const MegaShape& s)
{
    const size_t LDP = (size_t)4 * ((s.d + 3) / 4) + 1;
    return sizeof(double) * ((size_t)16 * mega_mix_wave_doubles(s.d, s.k, s.J) + (size_t)s.ad_R1 * s.ad_nbp + 64 * LDP + 32);
}
inline size_t mega_mvn_multi_lds(const MegaShape& s, bool pb_lds) { return mega_lds(s, s.tri, true, 16, pb_lds, true, false, s.ad_R1); }

// -> MegaChoice::burnin of an eligible choice.  1: the kernel makes its blocks' unit sums generation by generation (the MG instantiations: blocks of 16 chains =
// one unit);  2: any other persistent kernel (blocks of 12 / 8 / 4 chains, split generations, 128 < d <= 256, multitry off, redraw rounds) -- every generation's
// positions go to a ring of published positions and ONE k_adapt_partials_ring launch behind it makes the sums of all its generations;  0: one burn-in generation per launch
inline int mega_burnin_mode(const MegaShape& s, const MegaChoice& c)
{
    if (!s.ad_multi || s.tempering) return 0;
    const size_t tab = sizeof(double) * (size_t)s.ad_R1 * s.ad_nbp;
    const bool ring_ok = sizeof(double) * (size_t)(s.adapt_lag + 2) * s.N * s.ld <= ((size_t)8 << 30);
    if (c.family == MEGA_MIX || c.family == MEGA_USER) {
        if (s.lk == MEGA_LK_MIX && s.adapt_fused && s.k >= 3 && s.ld <= 128 && mega_fits(mega_mix_multi_lds(s))) return 1;
        return (ring_ok && mega_fits(sizeof(double) * (size_t)MIXW * mega_mix_wave_doubles(s.d, s.k, s.J) + tab)) ? 2 : 0;
    }
    if (c.family == MEGA_D2) return (ring_ok && mega_fits(mega_lds(s, s.tri, false, c.d2_ch, false, false, true, s.ad_R1, c.d2_sp))) ? 2 : 0;
    if (s.adapt_fused && s.k >= 3 && !s.redo_possible && c.ch == 16 && c.split_c == s.nl && (c.pb || c.xlds) && mega_fits(mega_mvn_multi_lds(s, c.pb_lds))) return 1;
    if (!ring_ok) return 0;
    for (int part = 0; part < (c.split_c == s.nl ? 1 : 2); ++part)
        if (!mega_fits(mega_lds(s, s.tri, c.pb || c.xlds, part ? c.ch_b : c.ch, c.pb_lds, false, false, s.ad_R1))) return 0;
    return 2;
}

inline MegaChoice mega_choose(const MegaShape& s)
{
    MegaChoice c = {};
    // The instantiations with the full proposal code: per-dimension priors, hard boundaries, several DE pairs (need_x) -- or redraw rounds inside the kernel
    // (redo: multi-try, device MVN likelihood).  redo implies need_x for every shape the engine makes: under the MVN likelihood redo_possible is true only with a
    // uniform prior, which sets have_prior.  The block plan, d2 and the mixture / user kernels ask with need_x (none of them runs with redo), the rest with pb.
    c.need_x = s.hard || s.have_prior || s.depairs > 1;
    c.redo = s.redo_possible && s.lk == MEGA_LK_MVN && s.k > 1 && s.mega_redo;
    c.pb = c.need_x || c.redo;
    // the full-code instantiations stage the per-dimension prior / boundary constants in LDS (Params::pb_lds) when that still fits -- at the block size planned with
    // them; without them the plan is made again
    mega_block_plan(s, c.need_x, c.pb, c);
    c.pb_lds = c.pb && mega_fits(mega_lds(s, s.tri, true, c.ch, true));
    if (c.pb && !c.pb_lds) mega_block_plan(s, c.need_x, false, c);
    c.xlds = mega_fits(mega_lds(s, s.tri, true, c.ch, c.pb_lds));
    // waves per chain: 4 when a block holds only 4 chains (fewer than 8 chains per CU) -- the tries of a phase then run side by
    // side (1024 chains: 238 -> 249 M proposals/s, 512: 120 -> 131); at 8 chains per block two waves per chain lose (405 -> 368).
    // multitry off: one try, one wave per chain whatever the block size
    c.wpc = (c.ch == 4 && s.k != 1) ? 4 : 1;
    const bool tries_ok = (s.k == 1 || s.k >= 3) && s.k <= MAXK && s.nslots <= 64;
    c.d2_ch = mega_d2_chains(s, c.need_x, c.pb_lds);
    if (c.d2_ch) {
        c.family = MEGA_D2;
        c.d2_sp = (c.d2_ch == 16 || c.d2_ch == 8) && mega_d2_two_pass(s, c.d2_ch);
        c.wpc = c.d2_ch == 8 ? 2 : (c.d2_ch == 4 ? 4 : 1);
    } else if (s.redo_possible && !c.redo) {
        c.family = MEGA_NONE;
    } else if (s.mega && (s.lk == MEGA_LK_MIX || (s.lk == MEGA_LK_MODULE && s.lk_items == 1 && s.gen_fn[(s.ld > 128 ? 2 : 0) + (c.need_x ? 1 : 0)])) && !s.redo_possible &&
               s.ld <= 256 && tries_ok && s.J <= 32) {
        c.family = s.lk == MEGA_LK_MIX ? MEGA_MIX : MEGA_USER;      // the barrier-free kernels: a wave carries its chain on its own
    } else if (c.pb && !c.xlds) {
        c.family = MEGA_NONE;      // (the full-code instantiations keep the states in LDS)
    } else if (s.mega && s.lk == MEGA_LK_MVN && s.ld <= 128 && tries_ok && (!s.tri || s.mtp) && mega_fits(mega_lds(s, s.tri, false, c.ch, c.pb_lds))) {
        c.family = (c.ch == 4 && c.wpc == 4 && !c.pb && c.xlds && s.k >= 3 && s.k <= 6) ? MEGA_W4 : MEGA_CLASSIC;
    }
    if (s.prior_ext) c.family = MEGA_NONE;
    c.burnin = c.family == MEGA_NONE ? 0 : mega_burnin_mode(s, c);
    return c;
}

// publish: the launch's generations are crossover burn-in (their positions are published);  applies: the previous launch's adaptation totals are pending
// and this launch's prologue applies them.  The only per-launch inputs.
inline MegaLaunchPlan mega_launch_plan(const MegaChoice& c, const MegaShape& s, bool publish, bool applies)
{
    MegaLaunchPlan P = {};
    const bool ring = s.adapt_lag > 0, k1 = s.k == 1;
    const int mmode = (publish && ring) ? c.burnin : 0;
    const bool multi = mmode == 1, rmulti = mmode == 2;
    // crossover burn-in with adapt_lag 0: a block of 16 chains is one unit of the adaptation's column sums (contract v3) and may make them itself
    const bool may_fuse = publish && !ring && s.adapt_fused && (s.world == 1 || s.adapt_groups) && s.k >= 3;
    P.nparts = 1;
    MegaPart& a = P.part[0];
    a.c0 = 0; a.c1 = s.nl; a.ring = rmulti;
    a.f.tri = s.tri; a.f.k1 = k1; a.f.pb = c.need_x; a.f.xlds = false; a.f.redo = false;
    if (c.family == MEGA_MIX || c.family == MEGA_USER) {
        const size_t W = sizeof(double) * (size_t)mega_mix_wave_doubles(s.d, s.k, s.J);
        const size_t lds_probs = sizeof(double) * (size_t)((s.ncr + s.ngamma + 1) & ~1), lds_xo = sizeof(double) * (size_t)16 * (4 * ((s.d + 3) / 4) + 1);
        a.fused = !multi && may_fuse && s.ld <= 128 && mega_fits(16 * W + lds_probs + lds_xo);
        const int mw = (multi || a.fused) ? 16 : MIXW;
        a.wide = s.ld > 128; a.f.multi = multi; a.f.ch = mw; a.f.wpc = 1;
        a.grid = (unsigned)((s.nl + mw - 1) / mw); a.block = 64u * mw;
        a.lds = multi ? mega_mix_multi_lds(s) : mw * W + (rmulti ? sizeof(double) * (size_t)s.ad_R1 * s.ad_nbp : lds_probs) + (a.fused ? lds_xo : 0);
        return P;
    }
    if (c.family == MEGA_D2) {
        a.f.d2 = true; a.f.ch = c.d2_ch; a.f.wpc = c.wpc; a.f.sp = c.d2_sp;
        a.grid = (unsigned)((s.nl + c.d2_ch - 1) / c.d2_ch); a.block = 64u * c.d2_ch * c.wpc;
        a.lds = mega_lds(s, s.tri, false, c.d2_ch, false, false, true, rmulti ? s.ad_R1 : 0, c.d2_sp);
        return P;
    }
    // (a chain count just above whole rounds of blocks: the remainder in a second launch of smaller blocks -- mega_block_plan)
    const bool split = c.split_c != s.nl;
    P.nparts = split ? 2 : 1;
    for (int i = 0; i < P.nparts; ++i) {
        MegaPart& q = P.part[i];
        const int chp = i ? c.ch_b : c.ch, wpcp = (chp == 4 && !k1) ? 4 : 1;
        q.c0 = i ? c.split_c : 0; q.c1 = i ? s.nl : c.split_c; q.ring = rmulti;
        q.f.tri = s.tri; q.f.xlds = c.pb || c.xlds; q.f.pb = c.pb; q.f.k1 = k1; q.f.ch = chp; q.f.wpc = wpcp; q.f.redo = c.redo; q.f.multi = multi;
        q.f.ahead = chp == 4 && wpcp == 4 && !c.pb && c.xlds && !k1 && s.k >= 3 && s.k <= 6;
        q.lds = mega_lds(s, s.tri, q.f.xlds, chp, c.pb_lds, false, false, rmulti ? s.ad_R1 : 0);
        if (multi) q.lds = mega_mvn_multi_lds(s, c.pb_lds);      // (one launch of 16-chain blocks, the states in LDS)
        else if (!rmulti && !split && may_fuse && chp == 16 && wpcp == 1 && !k1 && (c.pb || c.xlds)) {      // (the new and old states are read from LDS; a split generation's unit sums come from k_adapt_partials)
            const size_t with_xo = mega_lds(s, s.tri, true, chp, c.pb_lds, true);
            if (mega_fits(with_xo)) { q.fused = true; q.lds = with_xo; }
        }
        // five tries (the reference's multitry=True), nothing but the chains' own steps to leave behind, ONE launch of 16-chain blocks: the instantiation with
        // the try count compiled in and no publishing / adaptation code (same arithmetic, same draws, same name: k_generations' KC and PLAIN parameters) ...
        q.f.kc = (s.mega_kc && s.k == 5 && !c.pb && !k1 && (c.xlds || !s.tri) && chp == 16 && wpcp == 1 && !split && !publish && !applies) ? 5 : 0;
        if (q.f.kc) {      // ... which keeps its output cursors in LDS behind the layout (MegaLayout::off_cur); where they do not fit, the generic instantiation runs
            const size_t with_cur = mega_lds(s, s.tri, c.xlds, chp, false, false, false, 0, false, true);
            if (mega_fits(with_cur)) q.lds = with_cur; else q.f.kc = 0;
        }
        q.grid = (unsigned)((q.c1 - q.c0 + chp - 1) / chp); q.block = 64u * chp * wpcp;
    }
    return P;
}

}  // namespace dz
