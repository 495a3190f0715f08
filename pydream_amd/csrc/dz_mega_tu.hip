// dz_mega_tu.hip -- the instantiations of k_generations (dz_megakernel.h) for ONE row-tile count, -DDZ_TU_NRT=1..8.
#define DZ_TEMPLATES_ONLY
#include "dz_megakernel.h"
#include "dz_megakernel_w4.h"
#include "dz_megakernel_d2.h"
#include "dz_mega_launch.h"
#include <hip/hip_ext.h>

#ifndef DZ_TU_NRT
#error "compile with -DDZ_TU_NRT=<1..16>"
#endif

namespace dz {

#define DZ_CAT_(a, b) a##b
#define DZ_CAT(a, b) DZ_CAT_(a, b)
#define DZ_STR_(x) #x
#define DZ_STR(x) DZ_STR_(x)

// k_generations_d2 (dz_megakernel_d2.h): the triangular factor read from L2, CH chains x WPC waves per block, multitry off (K1), the proposal set in two passes
// (SP).  The full / lean branch is taken here and names what it launched.
template <int CH, int WPC, bool K1, bool SP>
static const char* launch_d2(const MegaLaunch& a)
{
    if (a.pb) {
        hipExtLaunchKernelGGL((k_generations_d2<DZ_TU_NRT, true, CH, K1, true, WPC, SP>), a.grid, a.block, a.lds, a.st, a.ka, a.kb, 0, a.pp, a.g, a.n, a.M, a.slot0, a.zappend, a.seg0, *a.publish);
        return K1 ? "k_generations_d2<" DZ_STR(DZ_TU_NRT) ",tri,xhbm,%d,%d,full,k1>" : SP ? "k_generations_d2<" DZ_STR(DZ_TU_NRT) ",tri,xhbm,%d,%d,full,two-pass>" : "k_generations_d2<" DZ_STR(DZ_TU_NRT) ",tri,xhbm,%d,%d,full>";
    }
    hipExtLaunchKernelGGL((k_generations_d2<DZ_TU_NRT, true, CH, K1, false, WPC, SP>), a.grid, a.block, a.lds, a.st, a.ka, a.kb, 0, a.pp, a.g, a.n, a.M, a.slot0, a.zappend, a.seg0, *a.publish);
    return K1 ? "k_generations_d2<" DZ_STR(DZ_TU_NRT) ",tri,xhbm,%d,%d,lean,k1>" : SP ? "k_generations_d2<" DZ_STR(DZ_TU_NRT) ",tri,xhbm,%d,%d,lean,two-pass>" : "k_generations_d2<" DZ_STR(DZ_TU_NRT) ",tri,xhbm,%d,%d,lean>";
}
// 128 < ld <= 256 (two 128-dimension chunks per lane): 16 chains per block, with multitry off or the two-pass set where the tiles of k tries do not fit (229..256
// dimensions at 5 tries, round 6); 8 chains x 2 waves where the point tiles of 16 chains do not fit (d > ~228 at 5 tries), with the two-pass set at 256 dimensions
// and 8 tries; 4 chains x 4 waves where not even those fit.
// ld <= 128 (one chunk per lane), where the point tiles of 16 chains do NOT fit next to the matrix in LDS (113..128 dimensions at 5 tries, 100 dimensions at 8 or
// more) and (round 6) for more than 15 tries: multitry on and one pass only -- 16 chains per block, 8 x 2 (100 dimensions at 16..20 tries), 4 x 4 (24..32 tries at
// 100 dimensions, 20..32 at 128).  (The host only sends the triangular factor here: mega_d2_chains.)
// (A template so that the WIDE branch is not instantiated in the units with ld <= 128: their set of kernels holds no multitry-off or two-pass d2 instantiation.)
template <bool WIDE = (DZ_TU_NRT > 8)>
static const char* launch_d2_ch(const MegaLaunch& a)
{
    if constexpr (WIDE) {
        if (a.k1) return launch_d2<16, 1, true, false>(a);
        if (a.sp && a.ch == 16) return launch_d2<16, 1, false, true>(a);
        if (a.sp && a.ch == 8) return launch_d2<8, 2, false, true>(a);
    }
    if (a.ch == 4) return launch_d2<4, 4, false, false>(a);
    if (a.ch == 8) return launch_d2<8, 2, false, false>(a);
    return launch_d2<16, 1, false, false>(a);
}

#if DZ_TU_NRT > 8
const char* DZ_CAT(mega_launch_nrt, DZ_TU_NRT)(const MegaLaunch& a) { return launch_d2_ch<>(a); }
#else
template <bool TRI, bool X, int CH, int WPC, bool PB, bool K1>
static const char* launch_one(const MegaLaunch& a)
{
    if constexpr (PB && !K1) {
        if (a.redo) {
            hipExtLaunchKernelGGL((k_generations<DZ_TU_NRT, TRI, X, CH, WPC, PB, K1, true>), a.grid, a.block, a.lds, a.st, a.ka, a.kb, 0,
                                  a.pp, a.g, a.n, a.M, a.slot0, a.zappend, a.seg0, *a.publish);
            return TRI ? "k_generations<" DZ_STR(DZ_TU_NRT) ",tri,xlds,%d,%d,full,redo>" : "k_generations<" DZ_STR(DZ_TU_NRT) ",dense,xlds,%d,%d,full,redo>";
        }
    }
    if constexpr (X && CH == 16 && WPC == 1 && !K1) {
        if (a.multi) {      // adapt_lag >= 1: several burn-in generations per launch
            hipExtLaunchKernelGGL((k_generations<DZ_TU_NRT, TRI, X, CH, WPC, PB, K1, false, true>), a.grid, a.block, a.lds, a.st, a.ka, a.kb, 0,
                                  a.pp, a.g, a.n, a.M, a.slot0, a.zappend, a.seg0, *a.publish);
            return TRI ? (PB ? "k_generations<" DZ_STR(DZ_TU_NRT) ",tri,xlds,%d,%d,full,multi>" : "k_generations<" DZ_STR(DZ_TU_NRT) ",tri,xlds,%d,%d,lean,multi>")
                       : (PB ? "k_generations<" DZ_STR(DZ_TU_NRT) ",dense,xlds,%d,%d,full,multi>" : "k_generations<" DZ_STR(DZ_TU_NRT) ",dense,xlds,%d,%d,lean,multi>");
        }
    }
    // multitry 5, nothing published, nothing adapted (MegaLaunch::kc): the try count compiled in.  The same kernel by name -- what it computes is the generic
    // instantiation's, bit for bit.  (The packed triangle leaves room for the states in LDS wherever 16 chains fit: no <tri, xhbm> copy.)
    if constexpr (CH == 16 && WPC == 1 && !PB && !K1 && (X || !TRI)) {
        if (a.kc == 5)
            hipExtLaunchKernelGGL((k_generations<DZ_TU_NRT, TRI, X, CH, WPC, PB, K1, false, false, 5, true>), a.grid, a.block, a.lds, a.st, a.ka, a.kb, 0,
                                  a.pp, a.g, a.n, a.M, a.slot0, a.zappend, a.seg0, *a.publish);
        else
            hipExtLaunchKernelGGL((k_generations<DZ_TU_NRT, TRI, X, CH, WPC, PB, K1>), a.grid, a.block, a.lds, a.st, a.ka, a.kb, 0,
                                  a.pp, a.g, a.n, a.M, a.slot0, a.zappend, a.seg0, *a.publish);
    } else
    hipExtLaunchKernelGGL((k_generations<DZ_TU_NRT, TRI, X, CH, WPC, PB, K1>), a.grid, a.block, a.lds, a.st, a.ka, a.kb, 0,
                          a.pp, a.g, a.n, a.M, a.slot0, a.zappend, a.seg0, *a.publish);
    // (NRT, matrix, chain states, chains per block, waves per chain, proposal code)
    return TRI ? (X ? (PB ? (K1 ? "k_generations<" DZ_STR(DZ_TU_NRT) ",tri,xlds,%d,%d,full,k1>" : "k_generations<" DZ_STR(DZ_TU_NRT) ",tri,xlds,%d,%d,full>")
                          : (K1 ? "k_generations<" DZ_STR(DZ_TU_NRT) ",tri,xlds,%d,%d,lean,k1>" : "k_generations<" DZ_STR(DZ_TU_NRT) ",tri,xlds,%d,%d,lean>"))
                      : (K1 ? "k_generations<" DZ_STR(DZ_TU_NRT) ",tri,xhbm,%d,%d,lean,k1>" : "k_generations<" DZ_STR(DZ_TU_NRT) ",tri,xhbm,%d,%d,lean>"))
               : (X ? (PB ? (K1 ? "k_generations<" DZ_STR(DZ_TU_NRT) ",dense,xlds,%d,%d,full,k1>" : "k_generations<" DZ_STR(DZ_TU_NRT) ",dense,xlds,%d,%d,full>")
                          : (K1 ? "k_generations<" DZ_STR(DZ_TU_NRT) ",dense,xlds,%d,%d,lean,k1>" : "k_generations<" DZ_STR(DZ_TU_NRT) ",dense,xlds,%d,%d,lean>"))
                      : (K1 ? "k_generations<" DZ_STR(DZ_TU_NRT) ",dense,xhbm,%d,%d,lean,k1>" : "k_generations<" DZ_STR(DZ_TU_NRT) ",dense,xhbm,%d,%d,lean>"));
}

template <bool TRI, bool X, bool PB>
static const char* launch_ch(const MegaLaunch& a)
{
    if constexpr (!PB && X) {
        if (a.ahead && a.ch == 4 && !a.k1) {      // small populations: four waves per chain, the tries' base-independent halves made ahead (dz_megakernel_w4.h)
            hipExtLaunchKernelGGL((k_generations_w4<DZ_TU_NRT, TRI>), a.grid, a.block, a.lds, a.st, a.ka, a.kb, 0, a.pp, a.g, a.n, a.M, a.slot0, a.zappend, a.seg0, *a.publish);
            return TRI ? "k_generations_w4<" DZ_STR(DZ_TU_NRT) ",tri,xlds,%d,%d,lean,ahead>" : "k_generations_w4<" DZ_STR(DZ_TU_NRT) ",dense,xlds,%d,%d,lean,ahead>";
        }
    }
#ifdef DZ_TU_FAST      // experiment builds (tools/fastbuild.sh): multi-try only, 16 chains per block or 4 x 4 waves -- a third of the instantiations
    if (a.ch == 4) return launch_one<TRI, X, 4, 4, PB, false>(a);
    return launch_one<TRI, X, 16, 1, PB, false>(a);
#endif
    if (a.k1) {
        if (a.ch == 16) return launch_one<TRI, X, 16, 1, PB, true>(a);
        if (a.ch == 8) return launch_one<TRI, X, 8, 1, PB, true>(a);
        return launch_one<TRI, X, 4, 1, PB, true>(a);
    }
    if (a.ch == 16) return launch_one<TRI, X, 16, 1, PB, false>(a);
    if (a.ch == 12) return launch_one<TRI, X, 12, 1, PB, false>(a);      // (round 6: 2049 .. 3072 chains on 256 CUs -- multi-try only)
    if (a.ch == 8) return launch_one<TRI, X, 8, 1, PB, false>(a);
    return launch_one<TRI, X, 4, 4, PB, false>(a);
}

// (priors / boundaries / several pairs: only with the chain states in LDS -- mega_choose -- which keeps the number of kernels down)
const char* DZ_CAT(mega_launch_nrt, DZ_TU_NRT)(const MegaLaunch& a)
{
    if (a.d2) return launch_d2_ch<>(a);
    if (a.pb) return a.tri ? launch_ch<true, true, true>(a) : launch_ch<false, true, true>(a);
    if (a.tri) return a.xlds ? launch_ch<true, true, false>(a) : launch_ch<true, false, false>(a);
    return a.xlds ? launch_ch<false, true, false>(a) : launch_ch<false, false, false>(a);
}
#endif      // DZ_TU_NRT <= 8

}  // namespace dz
