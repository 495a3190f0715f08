// dz_draw_groups.h -- the archive row count of the generations of one draw group (k_generations<.., KC, PLAIN>, dz_megakernel.h).
//
// The slot draws of a generation are addressed by (slot, stream, global chain, generation) and never by the chain's state, so one Philox pass over the
// wave's 64 lanes makes the draws of G = 64 / nslots consecutive generations.  The row numbers made from them need the archive row count of EACH of those
// generations: a history append inside the group raises it by N for the generations behind it.  Plain C++: the kernel and the host-side test
// (tests/test_draw_groups_cpu.py) compile the same lines.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define DZ_DRAW_GROUPS_HD __host__ __device__
#else
#define DZ_DRAW_GROUPS_HD
#endif

namespace dz {

// Rows generation index gi0 + j of a launch samples from, when generation index gi0 samples from M of them.  next_app: the index of the first generation
// >= gi0 that appends N rows behind its Metropolis step (the generations behind it see them), -1: none; the appends after it follow `thin` generations apart.
DZ_DRAW_GROUPS_HD inline uint32_t draw_group_rows(uint32_t M, uint32_t N, int next_app, int thin, int gi0, int j)
{
    int a = next_app;
    for (int t = 0; t < j; ++t)
        if (gi0 + t == a) { M += N; a += thin; }
    return M;
}

}  // namespace dz
