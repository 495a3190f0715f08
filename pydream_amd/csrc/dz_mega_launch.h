// dz_mega_launch.h -- the launch interface between dz_engine.hip and the translation units that hold the instantiations of the
// persistent generation kernel (dz_mega_tu.hip, compiled once per row-tile count NRT = ld / 16 so that the ~300 instantiations
// build in parallel: pydream_amd/build.py).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "dz_mega_select.h"

namespace dz {

struct Params;
struct Publish;

struct MegaLaunch : MegaFlags {      // (what the selection decided: dz_mega_select.h)
    dim3 grid, block; size_t lds; hipStream_t st;
    hipEvent_t ka, kb;          // the launch's own start / stop events (profiling pass) or null
    const Params* pp; uint32_t g; int n; uint32_t M; int64_t slot0; int64_t zappend; int seg0 = 0; const Publish* publish;      // seg0: generations up to and including the launch's first history append
};

// returns a static string naming the instantiation that was launched ("k_generations<7,tri,xlds,16,1,lean>")
#define DZ_MEGA_DECL(N_) const char* mega_launch_##N_(const MegaLaunch& a);
DZ_MEGA_DECL(nrt1) DZ_MEGA_DECL(nrt2) DZ_MEGA_DECL(nrt3) DZ_MEGA_DECL(nrt4) DZ_MEGA_DECL(nrt5) DZ_MEGA_DECL(nrt6) DZ_MEGA_DECL(nrt7) DZ_MEGA_DECL(nrt8)
DZ_MEGA_DECL(nrt9) DZ_MEGA_DECL(nrt10) DZ_MEGA_DECL(nrt11) DZ_MEGA_DECL(nrt12) DZ_MEGA_DECL(nrt13) DZ_MEGA_DECL(nrt14) DZ_MEGA_DECL(nrt15) DZ_MEGA_DECL(nrt16)      // (9..16: k_generations_d2 only)
#undef DZ_MEGA_DECL

}  // namespace dz
