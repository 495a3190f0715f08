// dz_engine.hip -- host side of libdreamzs.so: device-resident state of the MT-DREAM(ZS)
// sampler (Z archive, chain states, adaptation accumulators, trace) and the per-generation
// launch sequence, behind the C ABI of include/dreamzs.h.
//
// Replaces, for the hot path: pydream/core.py:250-327 (_setup_mp_dream_pool / _mp_dream_init:
// shared arrays -> HBM buffers), core.py:89-129 (_sample_dream loop -> dz_step) and
// pydream/Dream.py:193-422 (astep -> the kernels of dz_kernels.h).
#include "../../include/dreamzs.h"
#include "dz_kernels.h"
#include "dz_megakernel.h"
#include "dz_mega_launch.h"
#include "dz_multi_select.h"

#include <hip/hip_ext.h>
#include <dlfcn.h>
#include <sys/mman.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <type_traits>
#include <thread>
#include <utility>
#include <vector>

namespace {

thread_local std::string g_err;
int fail(const std::string& m) { g_err = m; return -1; }

#define HIPCK(expr)                                                                                   \
    do {                                                                                              \
        hipError_t _e = (expr);                                                                       \
        if (_e != hipSuccess) return fail(std::string(#expr) + ": " + hipGetErrorString(_e));         \
    } while (0)
#define DZCK(expr) do { int _r = (expr); if (_r) return _r; } while (0)

constexpr int RA_STRIDE = 32;             // host run-ahead: a marker every RA_STRIDE generations (dz_step)
constexpr int MEGA_MAX_GEN = 1 << 20;     // generations per launch of the persistent kernels, at most

enum { LK_NONE = 0, LK_MVN = 1, LK_MIX = 2, LK_HOST = 3, LK_MODULE = 4 };
enum { PR_PROPOSE = 0, PR_LOGP = 1, PR_ACCEPT = 2, PR_ADAPT = 3, PR_EXCHANGE = 4, PR_GENERATIONS = 5, PR_EMPTY = 6, PR_COUNT = 7 };

struct Rccl {
    void* lib = nullptr;
    ncclResult_t (*GetUniqueId)(ncclUniqueId*) = nullptr;
    ncclResult_t (*CommInitRank)(ncclComm_t*, int, ncclUniqueId, int) = nullptr;
    ncclResult_t (*AllGather)(const void*, void*, size_t, ncclDataType_t, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    ncclResult_t (*CommCount)(const ncclComm_t, int*) = nullptr;
    const char* (*GetErrorString)(ncclResult_t) = nullptr;
    std::string path, hip_path;
    // RCCL must sit on the SAME HIP runtime as this library: device pointers and streams of one runtime instance mean nothing to
    // another.  A process that also imports PyTorch holds a second ROCm stack (torch/lib/librccl.so + its own libamdhip64), and a
    // bare dlopen("librccl.so.1") hands back whichever copy was loaded first.  So the library is opened by path, next to the
    // libamdhip64 this engine is linked against (DZ_RCCL_LIB overrides), and the HIP runtime it resolves is checked against ours.
    int load()
    {
        if (lib) return 0;
        Dl_info hi;
        if (!dladdr((void*)&hipGetDeviceCount, &hi) || !hi.dli_fname) return fail("cannot locate the HIP runtime this library is linked against");
        hip_path = hi.dli_fname;
        const std::string dir = hip_path.substr(0, hip_path.find_last_of('/'));
        std::vector<std::string> cand;
        if (const char* ov = getenv("DZ_RCCL_LIB")) cand.push_back(ov);
        cand.push_back(dir + "/librccl.so.1");
        cand.push_back(dir + "/librccl.so");
        cand.push_back("librccl.so.1");        // installs that keep RCCL apart from HIP (split packages, LD_LIBRARY_PATH): the runtime check below still applies
        std::string tried;
        for (const std::string& c : cand) {
            lib = dlopen(c.c_str(), RTLD_NOW | RTLD_LOCAL);
            if (lib) { path = c; break; }
            tried += c + " (" + dlerror() + "); ";
        }
        if (!lib) return fail("cannot load librccl (next to " + hip_path + " or by soname): " + tried);
        GetUniqueId = (decltype(GetUniqueId))dlsym(lib, "ncclGetUniqueId");
        CommInitRank = (decltype(CommInitRank))dlsym(lib, "ncclCommInitRank");
        AllGather = (decltype(AllGather))dlsym(lib, "ncclAllGather");
        CommDestroy = (decltype(CommDestroy))dlsym(lib, "ncclCommDestroy");
        GetErrorString = (decltype(GetErrorString))dlsym(lib, "ncclGetErrorString");
        CommCount = (decltype(CommCount))dlsym(lib, "ncclCommCount");
        if (!GetUniqueId || !CommInitRank || !AllGather || !CommDestroy) { dlclose(lib); lib = nullptr; return fail("librccl lacks required symbols: " + path); }
        Dl_info ri, rh;
        if (dladdr((void*)GetUniqueId, &ri) && ri.dli_fname) path = ri.dli_fname;
        void* their_hip = dlsym(lib, "hipGetDeviceCount");         // (searches librccl and its dependencies: the runtime it was built against)
        if (their_hip && dladdr(their_hip, &rh) && rh.dli_fname && hip_path != rh.dli_fname && !getenv("DZ_RCCL_ALLOW_MISMATCH")) {
            const std::string theirs = rh.dli_fname;
            dlclose(lib); lib = nullptr;
            return fail("librccl " + path + " uses the HIP runtime " + theirs + " but this engine uses " + hip_path +
                        ": two ROCm stacks in one process (set DZ_RCCL_LIB to the matching librccl)");
        }
        return 0;
    }
};
Rccl g_rccl;

template <class T> int dalloc(T** p, size_t n)
{
    HIPCK(hipMalloc((void**)p, sizeof(T) * (n ? n : 1)));
    HIPCK(hipMemset(*p, 0, sizeof(T) * (n ? n : 1)));
    // hipMemset on device memory may return before the fill has run, and the fill is queued on the NULL stream, which the engine's
    // non-blocking streams do not wait for: without this wait a late fill can wipe what the first kernels wrote (seen as zeroed
    // log_ps of a short run_dream call right after another engine's work)
    HIPCK(hipStreamSynchronize(nullptr));
    return 0;
}

}  // namespace

struct dz_engine {
    dz_config c{};
    dz::Params p{};
    hipStream_t stream = nullptr;
    // independent chain groups ("lanes") run their propose/logp/accept kernels on separate streams: between two
    // history appends the groups share nothing, so one group's likelihood (matrix pipe) overlaps another's
    // proposal generation (VALU) -- lane 0 is `stream`
    int nlanes = 1; hipStream_t lane_stream[8] = {nullptr}; hipEvent_t lane_ev[8] = {nullptr};
    // bounded host run-ahead: a marker every RA_STRIDE generations, the host never gets more than 3 markers ahead
    dz::Params p_shadow; bool params_uploaded = false;    // what d_params holds
    void* h_pin = nullptr; hipEvent_t pin_ev[2] = {nullptr, nullptr};          // page-locked bounce buffer (two halves) for downloads into pageable memory (d2h_2d)
    double* d_bar = nullptr;                // dz_comm_barrier's all-gather buffer (one element per rank)
    double* d_qpart = nullptr; size_t qpart_len = 0; bool logp_gemm = true;    // row-tile sums of the tiled large-d likelihood; DZ_LOGP_GEMM=0: no LDS-tiled product
    hipEvent_t ra_ev[4] = {nullptr}; bool ra_used[4] = {false, false, false, false}; int64_t ra_n = 0;
    int nch = 1;
    int64_t M = 0, gen = 0, ntrace = 0;
    int64_t napp = 0;               // appends made since the archive was set (dz_config.history_lag: the last `lag` of them are not sampleable yet)
    std::vector<int64_t> gen_c;     // per-chain generation counters (differ only under single-chain stepping)
    uint4* d_draws[2] = {nullptr, nullptr};
    dz::ChainCtl* d_ctl[2] = {nullptr, nullptr};
    bool have_logp = false, adapt = false;
    int lk = LK_NONE;
    dz_logp_cb cb = nullptr; void* cb_user = nullptr;
    // a user-supplied DEVICE likelihood (dz_set_likelihood_module): a kernel of a code object the user built, launched where k_logp_* run
    hipModule_t lk_module = nullptr; hipFunction_t lk_fn = nullptr; void* d_lk_data = nullptr; int lk_lanes = 1; bool lk_finite = false;
    // dz_set_likelihood_items: the kernel writes lk_items values per point into d_items (a slice per chain-group stream, grown on demand), k_sum_items adds them
    int lk_items = 1; double* d_items = nullptr; size_t items_len = 0;
    // ... and, when the code object has them, the persistent kernels with that density inlined (generations_wave_body<.., UserLike>): [0] lean, [1] full proposal code
    hipFunction_t lk_gen_fn[4] = {nullptr, nullptr, nullptr, nullptr};      // ([2], [3]: 128 < d <= 256)
    // an OUTPUT kernel beside the likelihood (dz_set_output_module / dz_eval_outputs): its own module, data block and device buffers
    // (d_out: items x out_doubles, d_out_like: items; both grown on demand and reused)
    hipModule_t out_module = nullptr; hipFunction_t out_fn = nullptr; void* d_out_data = nullptr; int out_lanes = 1, out_items = 1;
    int64_t out_doubles = 0; double* d_out = nullptr; double* d_out_like = nullptr; size_t out_len = 0, out_like_len = 0;
    dz_exchange_cb xcb = nullptr; void* xcb_user = nullptr;
    ncclComm_t comm = nullptr; int rank = 0, world = 1;
    // peer transport (dz_peer_export / dz_peer_attach): the other ranks' archives, position buffers and flag words mapped into this
    // process; rows travel on copy streams (one per peer: xGMI is point to point), never through a kernel
    struct Peer { double* Z = nullptr; double* cp[3] = {nullptr, nullptr, nullptr}; double* gs[2] = {nullptr, nullptr}; unsigned long long* flags = nullptr; hipStream_t st = nullptr; };
    std::vector<Peer> peers; bool peer_on = false;
    unsigned long long* d_flags = nullptr;      // [4][world]: exchange number received from every rank -- [0] history appends, [1] published positions, [2] the attach-time self-test, [3] adaptation group sums
    unsigned long long* d_seq = nullptr; int64_t seq_cap = 0;     // seq[i] = i: the source of the flag pushes
    unsigned long long* h_gate = nullptr;       // host-mapped: ticks waited, gates passed, error (k_peer_gate)
    hipEvent_t push_ev[8] = {nullptr}; int push_n = 0;
    int64_t z_pushed = 0, z_gated = 0, pos_pushed = 0, hello_seq = 1;      // (hello 1 = the attach-time self-test)
    double* d_cp[3] = {nullptr, nullptr, nullptr}; int cp_idx = 1;      // published positions rotate through three buffers (a peer may run one generation ahead)
    // owned device buffers (also referenced from p)
    double *d_mins = nullptr, *d_maxs = nullptr, *d_gtab = nullptr, *d_mu = nullptr, *d_Mt = nullptr, *d_Mtp = nullptr, *d_mixF = nullptr;
    double *d_pa = nullptr, *d_pb = nullptr, *d_plogb = nullptr, *d_pc2 = nullptr; int32_t* d_pkind = nullptr;
    double *d_shared = nullptr;      // cr_probs|cr_delta|cr_n|g_probs|g_delta|g_n -- two copies: e->p points at the current one (sh_cur); a persistent launch
    int sh_cur = 0;                  // that applies pending adaptation totals in its prologue reads the current copy and leaves the new state in the other
    bool adapt_pending = false;      // d_TOT / d_CNT hold totals that no launch has applied yet (only between two launches inside dz_step)
    double *d_partial = nullptr, *d_mean = nullptr, *d_sd = nullptr, *d_sdc = nullptr, *d_dl = nullptr, *d_dlg = nullptr;
    int *d_binc = nullptr, *d_bing = nullptr;
    double* d_binsum = nullptr;     // k_adapt_update's scratch: [strips of 64 chains][ncr + ngamma] sums, then the same shape of counts
    // lockstep adaptation, contract v3 (dz_kernels.h adapt_unit_sums): the units' sums [units][nq][ld] and counts [units][ncr + ngamma], their totals
    double *d_PR = nullptr, *d_PC = nullptr, *d_TOT = nullptr, *d_CNT = nullptr;
    bool adapt_fused = true;        // the persistent kernels make their block's unit sums themselves (DZ_ADAPT_FUSED=0: k_adapt_partials does)
    // dz_config.adapt_lag = L >= 1 (round 6): d_TOT / d_CNT are rings of L + 1 slots (slot = generation mod (L + 1); d_CNT rows of ad_nbp), d_DOT
    // [L + 1][ad_nbp] the bins' dot products (k_adapt_dots), d_PR / d_PC rings as well when launches hold several burn-in generations (ad_multi).
    // Updates of generations (ad_applied, ad_made] are pending: made, not yet added to the shared state.  d_x0ring [2 (L + 1)][ld]: global chain
    // 0's published position after generation h at slot h mod 2 (L + 1); d_x0start: before generation 0.
    int ad_R1 = 1, ad_nbp = 0; bool ad_multi = false; int64_t ad_applied = -1, ad_made = -1; size_t ad_tot_stride = 0, ad_pr_stride = 0, ad_pc_stride = 0;
    double *d_DOT = nullptr, *d_x0ring = nullptr, *d_x0start = nullptr;
    // ... and for the kernels that do not make their blocks' unit sums (MegaChoice::burnin == 2): d_posring [L + 2][N][ld] the published positions of the last
    // L + 2 generations (slot = generation mod (L + 2); made on first use), posring_gen the last generation in it; d_PG [L + 1][ad_nbp] the probabilities
    // the last launch's generations decided with (k_adapt_partials_ring)
    double *d_posring = nullptr, *d_PG = nullptr; int64_t posring_gen = -2;
    // sharded crossover burn-in (round 5): a rank that owns whole groups of 256 chains exchanges its groups' sums (dz_kernels.h k_adapt_groups /
    // k_group_totals) instead of its positions.  d_GS[parity of the generation]: [world][gs_rec] records (two buffers: a peer may be one
    // generation ahead); d_shift[parity]: global chain 0's position after that generation (the shift of the next one's column sums)
    bool adapt_groups_on = true, adapt_multi_on = true;      // DZ_ADAPT_GROUPS=0 / DZ_ADAPT_MULTI=0: neither the group sums nor several burn-in generations per launch
    bool adapt_groups = false; double* d_GS[2] = {nullptr, nullptr}; double* d_shift[2] = {nullptr, nullptr}; size_t gs_rec = 0; int gs_nbp = 0;
    int64_t gs_pushed = 0, gs_last_gen = -1, gs_launches = 0;
    int64_t bytes_z = 0, bytes_pos = 0, bytes_sums = 0;      // bytes this rank has sent to EACH other rank, by kind (dz_exchange_bytes)
    dz::Params* d_params = nullptr;  // device copy of `p` for kernels that take it by pointer
    double *d_scratch = nullptr; size_t scratch_rows = 0;   // debug / eval staging [rows, ld]
    double *d_cmean = nullptr, *d_cvar = nullptr, *d_rhat = nullptr;
    std::vector<double> h_stage;     // host staging (callback likelihood / exchange)
    bool prof = false;
    int num_cu = 256;
    bool q_defer = true;            // streamed generations: no k_q_finish launches, the proposal / Metropolis kernels add the row-tile sums (DZ_QFIN=0: off)
    double* last_qpart = nullptr;   // the scratch slice the last tiled likelihood launch wrote
    bool mega = true;               // the persistent generation kernel serves every eligible configuration (mega_choose, dz_mega_select.h); DZ_MEGA=0 forces the multi-kernel path
    bool mega_redo_on = true;       // redraw rounds (Dream.py:281-289) inside the persistent kernel; DZ_MEGA_REDO=0: such configurations take the multi-kernel path
    unsigned long long* d_redraw_count = nullptr;
    int mega_d2 = 1;                // 128 < d <= 256: k_generations_d2 from 1025 chains on (DZ_MEGA_D2=0: the multi-kernel path there; 2: at any chain count)
    bool mega_user = true;          // a user's device function inside the persistent kernel when its code object has it; DZ_MEGA_USER=0: the batch kernel only
    int mega_segs = 1 << 20;        // DZ_MEGA_SEGS: history appends per launch cap (1: a launch ends with its append, as without a lag)
    bool mega_kc = true;            // multitry 5 outside the burn-in: the instantiation with the try count compiled in (MegaLaunch::kc); DZ_MEGA_KC=0: the generic one
    bool tempering = false; double* d_Tc = nullptr; int32_t* d_tswap = nullptr;    // parallel tempering (dz_set_temperatures)
    // Dream.py:281-289: a proposal set whose tries are all impossible is drawn again (redo_possible / one_generation)
    uint8_t* d_redo = nullptr; int32_t* d_redo_list = nullptr; uint8_t* h_redo = nullptr; int32_t* h_redo_list = nullptr;     // (host side: page-locked)
    std::vector<int32_t> h_pkind; std::vector<double> h_pa, h_pb, h_mins, h_maxs;     // host copies: is the uniform priors' support covered by the hard boundaries?
    // dz_set_prior_ext with a kind above 2: the table k_prior_ext reads (its own kernel argument; Params does not know it) and the host copy of the shapes
    bool prior_ext = false; dz::PriorExtTable xt = {}; int32_t* d_xkind = nullptr; double* d_xtab = nullptr; std::vector<double> h_ps1, h_ps2;
    hipStream_t copy_stream = nullptr; hipEvent_t copy_ev[8] = {nullptr};   // dz_trace_download_begin / _wait: trace rows leave while later generations run
    int64_t redraw_rounds = 0;      // redraw launches so far (dz_redraw_rounds)
    double *d_own_cr = nullptr, *d_own_g = nullptr; std::vector<char> own_init;      // per-instance probabilities of single-chain stepping (Params::own_cr)
    std::string broken;             // non-empty: a failed dz_continue_run left the engine without some of its buffers -- dz_step refuses
    dz::MegaShape mshape; dz::MegaChoice mchoice;      // the persistent kernels' selection, made at the start of every dz_step (mega_select)
    dz::MultiShape multi;           // what the multi-kernel path's selection reads (multi_shape), refreshed by every entry point that reaches eval_logp or one_generation
    dz::MultiCarry carry;           // what the last generation of that path left for the next one (GenerationPlan::next)
    std::string last_variant;       // what the last dz_step launched for its generations (dz_last_kernel_variant)
    int last_kc = 0;                // ... and the try count compiled into it (MegaLaunch::kc; dz_last_kernel_tries)
    int propose_split = 0;          // waves per chain in k_propose (DZ_PROPOSE_SPLIT); 0 = by problem shape
    std::vector<hipEvent_t> ev_pool;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> ev[PR_COUNT];
    std::vector<void*> to_free;
};

namespace {

struct ProfScope {
    dz_engine* e; int which; hipStream_t st; hipEvent_t a = nullptr, b = nullptr;
    bool on;
    ProfScope(dz_engine* e_, int w, hipStream_t st_ = nullptr, bool active = true) : e(e_), which(w), st(st_ ? st_ : e_->stream), on(active && e_->prof)
    {
        if (on) {
            for (hipEvent_t* x : {&a, &b}) {
                if (!e->ev_pool.empty()) { *x = e->ev_pool.back(); e->ev_pool.pop_back(); }
                else (void)hipEventCreate(x);
            }
            (void)hipEventRecord(a, st);
        }
    }
    ~ProfScope() { if (on) { (void)hipEventRecord(b, st); e->ev[which].emplace_back(a, b); } }
};

hipEvent_t prof_event(dz_engine* e)
{
    hipEvent_t x = nullptr;
    if (!e->ev_pool.empty()) { x = e->ev_pool.back(); e->ev_pool.pop_back(); }
    else (void)hipEventCreate(&x);
    return x;
}
// One kernel launch of profile class CLS.  While profiling, the launch carries its own start/stop events
// (hipExtLaunchKernelGGL): they take the dispatch's begin/end timestamps -- the figures rocprofv3's kernel trace
// reports -- instead of bracketing the launch with two extra barrier packets that each add microseconds.
#define DZ_KLAUNCH(E, CLS, ST, KERN, GRID, BLOCK, LDS, ...)                                               \
    do {                                                                                                   \
        if ((E)->prof) {                                                                                   \
            hipEvent_t ka_ = prof_event(E), kb_ = prof_event(E);                                           \
            hipExtLaunchKernelGGL(KERN, GRID, BLOCK, LDS, ST, ka_, kb_, 0, __VA_ARGS__);                   \
            (E)->ev[CLS].emplace_back(ka_, kb_);                                                           \
        } else hipLaunchKernelGGL(KERN, GRID, BLOCK, LDS, ST, __VA_ARGS__);                                \
    } while (0)

// archive rows the next generation samples from: everything written, less the rows of the last `history_lag` appends
int64_t visible_rows(const dz_engine* e)
{
    const int64_t lag = std::min<int64_t>(e->napp, (int64_t)e->c.history_lag);
    return e->M - (int64_t)e->p.N * lag;
}

int peer_check(dz_engine* e);
// everything this engine has queued: the lane streams AND the per-peer copy streams -- a row or flag push still in flight when the
// caller goes on to a control-plane barrier and then frees or unmaps buffers would be a DMA write into memory that is gone
int sync_all(dz_engine* e)
{
    for (int s = 0; s < e->nlanes; ++s) HIPCK(hipStreamSynchronize(e->lane_stream[s]));
    for (auto& pr : e->peers) if (pr.st) HIPCK(hipStreamSynchronize(pr.st));
    return peer_check(e);
}

// Device -> pageable host, 2-D: through a page-locked bounce buffer owned by the engine (stream-ordered copy, wait, then
// plain memcpy).  Asynchronous and blocking 2-D copies straight into pageable memory both misbehaved on this stack
// (a rare late landing after the stream wait; zeros from the blocking form once several engines had lived in the process).
int d2h_2d(dz_engine* e, void* dst, size_t dpitch, const void* src, size_t spitch, size_t width, size_t height)
{
    if (!width || !height) return 0;
    constexpr size_t CAP = (size_t)64 << 20, HALF = CAP / 2;
    if (!e->h_pin) { if (hipHostMalloc(&e->h_pin, CAP, hipHostMallocDefault) != hipSuccess) { e->h_pin = nullptr; return fail("hipHostMalloc (bounce buffer) failed"); } }
    if (width > HALF) return fail("row too long for the bounce buffer");
    // two halves: the DMA of the next batch of rows runs while the host copies the batch before out of the other half
    const size_t rows_per = std::max<size_t>(1, HALF / width);
    auto issue = [&](size_t r0, int half) -> hipError_t {
        const size_t nr = std::min(rows_per, height - r0);
        return hipMemcpy2DAsync((char*)e->h_pin + (size_t)half * HALF, width, (const char*)src + r0 * spitch, spitch, width, nr, hipMemcpyDeviceToHost, e->stream);
    };
    if (!e->pin_ev[0]) for (int i = 0; i < 2; ++i) HIPCK(hipEventCreateWithFlags(&e->pin_ev[i], hipEventDisableTiming));
    HIPCK(issue(0, 0));
    HIPCK(hipEventRecord(e->pin_ev[0], e->stream));
    int half = 0;
    for (size_t r0 = 0; r0 < height; r0 += rows_per, half ^= 1) {
        const size_t nr = std::min(rows_per, height - r0);
        if (r0 + rows_per < height) { HIPCK(issue(r0 + rows_per, half ^ 1)); HIPCK(hipEventRecord(e->pin_ev[half ^ 1], e->stream)); }
        HIPCK(hipEventSynchronize(e->pin_ev[half]));
        const char* from = (const char*)e->h_pin + (size_t)half * HALF;
        if (dpitch == width) memcpy((char*)dst + r0 * dpitch, from, nr * width);
        else for (size_t r = 0; r < nr; ++r) memcpy((char*)dst + (r0 + r) * dpitch, from + r * width, width);
    }
    HIPCK(hipStreamSynchronize(e->stream));
    return 0;
}

template <class T> int ealloc(dz_engine* e, T** p, size_t n)
{
    DZCK(dalloc(p, n));
    e->to_free.push_back((void*)*p);
    return 0;
}

int upload_padded(dz_engine* e, double* dst, const double* src, int rows, double padval)
{   // src [rows,d] -> dst [rows,ld]
    const int d = e->p.d, ld = e->p.ld;
    std::vector<double> h((size_t)rows * ld, padval);
    for (int r = 0; r < rows; ++r) memcpy(&h[(size_t)r * ld], src + (size_t)r * d, sizeof(double) * d);
    HIPCK(hipMemcpyAsync(dst, h.data(), sizeof(double) * h.size(), hipMemcpyHostToDevice, e->stream));
    DZCK(sync_all(e));
    return 0;
}
int download_rows(dz_engine* e, double* dst, const double* src, size_t rows)
{   // src [rows,ld] device -> dst [rows,d] host
    DZCK(sync_all(e));
    return d2h_2d(e, dst, sizeof(double) * e->p.d, src, sizeof(double) * e->p.ld, sizeof(double) * e->p.d, rows);
}

#define NCH_DISPATCH(e, CALL)                      \
    switch ((e)->nch) {                            \
        case 1: { constexpr int NCH = 1; CALL; } break; \
        case 2: { constexpr int NCH = 2; CALL; } break; \
        case 4: { constexpr int NCH = 4; CALL; } break; \
        default: { constexpr int NCH = 8; CALL; } break; \
    }

int launch_check(const char* what)
{
    hipError_t err = hipGetLastError();
    if (err != hipSuccess) return fail(std::string(what) + ": " + hipGetErrorString(err));
    return 0;
}

// A device buffer of doubles that only grows: *have counts in the caller's units (`want` of them are `alloc` doubles); zeroed or not.  On failure
// the buffer is gone, *have is 0 and the HIP error comes back for the caller's message.
hipError_t grow_doubles(double** buf, size_t* have, size_t want, size_t alloc, bool zeroed)
{
    if (*have >= want) return hipSuccess;
    if (*buf) (void)hipFree(*buf);
    *buf = nullptr; *have = 0;
    hipError_t err = hipMalloc((void**)buf, sizeof(double) * (alloc ? alloc : 1));
    if (err == hipSuccess && zeroed) {      // (as dalloc: the fill is queued on the NULL stream, which the engine's streams do not wait for)
        err = hipMemset(*buf, 0, sizeof(double) * (alloc ? alloc : 1));
        if (err == hipSuccess) err = hipStreamSynchronize(nullptr);
    }
    if (err != hipSuccess) { (void)hipGetLastError(); if (*buf) (void)hipFree(*buf); *buf = nullptr; return err; }
    *have = want;
    return hipSuccess;
}
// Every chain-group stream has its own slice of a scratch array of `need` doubles per stream (grown behind sync_all) -> the slice of `st`
int stream_slice(dz_engine* e, hipStream_t st, double** buf, size_t* len, size_t need, const std::string& what, double** slice)
{
    int sl = 0;
    for (int s2 = 1; s2 < e->nlanes; ++s2) if (e->lane_stream[s2] == st) sl = s2;
    if (need * e->nlanes > *len) {
        DZCK(sync_all(e));
        const hipError_t err = grow_doubles(buf, len, need * e->nlanes, need * e->nlanes, true);
        if (err != hipSuccess) return fail(what + hipGetErrorString(err));
    }
    *slice = *buf + (size_t)sl * (*len / e->nlanes);
    return 0;
}

// The instantiations of the two small-d MVN kernels, indexed by the plan's template arguments (both take the same arguments)
using MvnKernel = void (*)(dz::Params, const double*, int, double*, double*);
template <int NRT> constexpr MvnKernel mvn_lds_kernel(bool tri) { return tri ? dz::k_logp_mvn_lds<NRT, true> : dz::k_logp_mvn_lds<NRT, false>; }
template <int NRT> constexpr MvnKernel mvn_mfma_kernel(int pt, bool tri)
{
    return pt == 2 ? (tri ? dz::k_logp_mvn_mfma<2, NRT, true> : dz::k_logp_mvn_mfma<2, NRT, false>) : (tri ? dz::k_logp_mvn_mfma<1, NRT, true> : dz::k_logp_mvn_mfma<1, NRT, false>);
}
template <size_t... I> MvnKernel mvn_kernel(const dz::LogpPlan& P, std::index_sequence<I...>)
{
    const MvnKernel lds[] = {mvn_lds_kernel<I + 1>(P.tri)...}, mfma[] = {mvn_mfma_kernel<I + 1>(P.pt, P.tri)...};
    return (P.family == dz::LOGP_LDS ? lds : mfma)[P.nrt - 1];
}
inline dim3 g3(const dz::MultiLaunch& l) { return dim3(l.grid); }
inline dim3 b3(const dz::MultiLaunch& l) { return dim3(l.block); }

// Model.total_logp for n points stored [n,ld] on the device; what is launched, with what geometry: dz::logp_plan (dz_multi_select.h)
// defer_finish (large-d MVN only): the row-tile sums stay in the scratch array (e->last_qpart) for the consuming kernel to add
// (Params::qfin_*) instead of a k_q_finish launch
int eval_logp(dz_engine* e, const double* pts, int n, double* prior, double* like, hipStream_t st = nullptr, bool defer_finish = false)
{
    if (n <= 0) return 0;
    if (!st) st = e->stream;
    const dz::LogpPlan P = dz::logp_plan(e->multi, n, defer_finish);
    ProfScope ps(e, PR_LOGP, st, !P.one_kernel);
    switch (P.family) {
    case dz::LOGP_LDS: case dz::LOGP_MFMA: {
        const MvnKernel kern = mvn_kernel(P, std::make_index_sequence<8>());
        if (P.one_kernel) DZ_KLAUNCH(e, PR_LOGP, st, kern, g3(P.main), b3(P.main), P.main.lds, e->p, pts, n, prior, like);
        else hipLaunchKernelGGL(kern, g3(P.main), b3(P.main), P.main.lds, st, e->p, pts, n, prior, like);
    } break;
    case dz::LOGP_TILED: case dz::LOGP_GEMM: {
        double* qpart = nullptr;
        DZCK(stream_slice(e, st, &e->d_qpart, &e->qpart_len, P.qpart_doubles, "hipMalloc((void**)p, sizeof(T) * (n ? n : 1)): ", &qpart));
        if (P.family == dz::LOGP_TILED) hipLaunchKernelGGL((dz::k_logp_mvn_mfma_tiled<dz::TILED_PT, dz::TILED_RTC>), g3(P.main), b3(P.main), 0, st, e->p, pts, n, qpart);
        else if (P.gemm_tile == 1) hipLaunchKernelGGL(dz::k_logp_mvn_gemm<1>, g3(P.main), b3(P.main), P.main.lds, st, e->p, pts, n, qpart, e->num_cu);
        else if (P.gemm_tile == 2) hipLaunchKernelGGL(dz::k_logp_mvn_gemm<2>, g3(P.main), b3(P.main), P.main.lds, st, e->p, pts, n, qpart, e->num_cu);
        else hipLaunchKernelGGL(dz::k_logp_mvn_gemm<4>, g3(P.main), b3(P.main), P.main.lds, st, e->p, pts, n, qpart, e->num_cu);
        e->last_qpart = qpart;
        if (P.q_finish) hipLaunchKernelGGL(dz::k_q_finish, g3(P.finish), b3(P.finish), 0, st, e->p, (const double*)qpart, n, P.nrtb, prior, like);
    } break;
    case dz::LOGP_MIX:
        NCH_DISPATCH(e, hipLaunchKernelGGL(dz::k_logp_mix<NCH>, g3(P.main), b3(P.main), 0, st, e->p, pts, n, prior, like));
        break;
    case dz::LOGP_MODULE: {
        struct { const double* X; long long n; int d; int ld; double* like; const void* data; } a = {pts, (long long)n, e->p.d, e->p.ld, like, e->d_lk_data};
        size_t asz = sizeof(a);
        void* extra[] = {HIP_LAUNCH_PARAM_BUFFER_POINTER, &a, HIP_LAUNCH_PARAM_BUFFER_SIZE, &asz, HIP_LAUNCH_PARAM_END};
        HIPCK(hipMemsetAsync(prior, 0, sizeof(double) * (size_t)n, st));
        if (P.grid_overflow) return fail("dz_set_likelihood_items: " + std::to_string(P.items) + " items are more than one launch's grid holds");
        double* scratch = nullptr;
        if (P.sum_items) {
            DZCK(stream_slice(e, st, &e->d_items, &e->items_len, P.scratch_doubles,
                              "dz_set_likelihood_items: cannot allocate the scratch for " + std::to_string(P.items) + " items x " + std::to_string(e->nlanes) + " streams: hipMalloc((void**)p, sizeof(T) * (n ? n : 1)): ", &scratch));
            a.n = P.items; a.like = scratch;
        }
        HIPCK(hipModuleLaunchKernel(e->lk_fn, P.main.grid, 1, 1, P.main.block, 1, 1, 0, st, nullptr, extra));
        if (P.sum_items) hipLaunchKernelGGL(dz::k_sum_items, g3(P.sum), b3(P.sum), 0, st, (const double*)scratch, n, e->multi.lk_items, like);
    } break;
    case dz::LOGP_HOST: {
        const int d = e->p.d;
        e->h_stage.resize((size_t)n * (d + 2));
        double* hx = e->h_stage.data(); double* hp = hx + (size_t)n * d; double* hl = hp + n;
        DZCK(download_rows(e, hx, pts, (size_t)n));
        for (int i = 0; i < n; ++i) { hp[i] = 0.0; hl[i] = 0.0; }
        if (e->cb(hx, n, d, hp, hl, e->cb_user)) return fail("host likelihood callback failed");
        HIPCK(hipMemcpyAsync(prior, hp, sizeof(double) * n, hipMemcpyHostToDevice, e->stream));
        HIPCK(hipMemcpyAsync(like, hl, sizeof(double) * n, hipMemcpyHostToDevice, e->stream));
        DZCK(sync_all(e));
    } break;
    default: return fail("no likelihood set");
    }
    if (P.prior_only) NCH_DISPATCH(e, hipLaunchKernelGGL(dz::k_prior_only<NCH>, g3(P.prior), b3(P.prior), 0, st, e->p, pts, n, prior));
    if (P.prior_add) NCH_DISPATCH(e, hipLaunchKernelGGL(dz::k_prior_add<NCH>, g3(P.prior), b3(P.prior), 0, st, e->p, pts, n, prior, like));
    if (P.prior_ext) NCH_DISPATCH(e, hipLaunchKernelGGL(dz::k_prior_ext<NCH>, g3(P.ext), b3(P.ext), 0, st, e->xt, pts, n, e->p.d, e->p.ld, prior, like, P.ext_fix_like ? 1 : 0));
    return launch_check("logp kernel");
}

enum { XK_Z = 0, XK_POS = 1, XK_HELLO = 2, XK_SUMS = 3, XK_KINDS = 4 };
double gate_timeout_s()
{
    // (liveness of the other ranks is the control plane's business; the bound only keeps a kernel from spinning for ever -- a rank with
    //  a host-callback likelihood or a slow start can legitimately be minutes late)
    if (const char* s = getenv("DZ_PEER_TIMEOUT_S")) return std::max(0.01, atof(s));
    return 600.0;
}
// peer transport: this rank's rows of `buf` (global layout [N,ld], rows [off, off+nl) at `row0`) go to every peer's copy of the
// buffer, each followed by this rank's flag word for exchange number `seq` of that kind
// (XK_SUMS: `buf` = d_GS[which_cp], this rank's record of gs_rec doubles at rank * gs_rec)
int peer_push(dz_engine* e, int kind, double* buf, int which_cp, size_t row0, unsigned long long seq, size_t sums_cnt = 0)
{
    if ((int64_t)seq >= e->seq_cap) return fail("peer exchange: sequence capacity exceeded");
    hipEvent_t ev = e->push_ev[e->push_n++ & 7];
    HIPCK(hipEventRecord(ev, e->stream));
    const size_t srec = sums_cnt ? sums_cnt : e->gs_rec;      // (a launch of several burn-in generations: that many records per rank, back to back)
    const size_t first = kind == XK_SUMS ? (size_t)e->rank * srec : (row0 + (size_t)e->p.off) * e->p.ld;
    const size_t cnt = kind == XK_SUMS ? srec : (size_t)e->p.nl * e->p.ld;
    for (int r = 0; r < e->world; ++r) {
        if (r == e->rank) continue;
        dz_engine::Peer& pr = e->peers[r];
        double* dst = kind == XK_Z ? pr.Z : (kind == XK_SUMS ? pr.gs[which_cp] : pr.cp[which_cp]);
        HIPCK(hipStreamWaitEvent(pr.st, ev, 0));
        if (kind != XK_HELLO) HIPCK(hipMemcpyAsync(dst + first, buf + first, sizeof(double) * cnt, hipMemcpyDeviceToDevice, pr.st));
        HIPCK(hipMemcpyAsync(pr.flags + (size_t)kind * e->world + e->rank, e->d_seq + seq, sizeof(unsigned long long), hipMemcpyDeviceToDevice, pr.st));
    }
    return 0;
}
// ... and the wait for everybody else's rows of exchange `need`: a one-wave kernel on the engine's stream (k_peer_gate)
int peer_gate(dz_engine* e, int kind, unsigned long long need, double timeout_s = 0.0)
{
    const unsigned long long ticks = (unsigned long long)((timeout_s > 0.0 ? timeout_s : gate_timeout_s()) * 1e8);
    // (rendezvous gates keep their own counters, [4..6]: what they wait for is the other ranks' lateness, not an exchange)
    hipLaunchKernelGGL(dz::k_peer_gate, dim3(1), dim3(64), 0, e->stream, (const unsigned long long*)(e->d_flags + (size_t)kind * e->world), e->world, e->rank, need, ticks,
                       e->h_gate + (kind == XK_HELLO ? 4 : 0));
    return launch_check("k_peer_gate");
}
// did a gate give up?  h_gate is host-mapped, so this costs nothing: dz_step asks before it queues each launch (a timed-out gate is
// fatal for the run: whatever was queued behind it sampled rows that never arrived, and no getter hands such results out), every
// synchronising entry point asks after its wait
int peer_check(dz_engine* e)
{
    if (e->peer_on && e->h_gate && (e->h_gate[2] || e->h_gate[6])) {
        const int r = (int)(e->h_gate[2] ? e->h_gate[2] : e->h_gate[6]) - 1;
        return fail("peer exchange: no rows from rank " + std::to_string(r) + " within " + std::to_string(gate_timeout_s()) + " s (DZ_PEER_TIMEOUT_S)");
    }
    return 0;
}
// before generations that sample the archive: the rows of every append that is visible now have arrived from every rank
// (ahead: history appends the launch makes itself in front of its last generation -- the generations behind the j-th of them sample the rows
//  of one more append)
int ensure_visible(dz_engine* e, int ahead = 0)
{
    if (!e->peer_on) return 0;
    const int64_t made = e->napp + ahead;
    const int64_t need = made - std::min<int64_t>(made, (int64_t)e->c.history_lag);
    if (need > e->z_gated) { DZCK(peer_gate(e, XK_Z, (unsigned long long)need)); e->z_gated = need; }
    return 0;
}

// Replicates this rank's rows of `buf` (global layout [N,ld]; the rank's nl rows sit at row0 + off) on every rank.
//   RCCL: in-place ncclAllGather on the engine's stream;  host: staged through the exchange callback (tests, gloo);
//   peer: pushed by the copy engines into the peers' mapped buffers -- history appends are waited for only when their rows become
//   sampleable (ensure_visible: with history_lag >= 1 a whole thin-cycle later), published positions at once.
// XK_SUMS (sharded crossover burn-in): buf = d_GS[which], [world][gs_rec]; this rank's record is replicated, waited for at once.
int exchange_rows(dz_engine* e, int kind, double* buf, size_t row0, int which = 0, size_t sums_cnt = 0)
{
    if (!e->comm && !e->peer_on && e->p.nl == e->p.N) return 0;     // single GPU, no communicator: the kernels wrote the rows in place
    ProfScope ps(e, PR_EXCHANGE);
    const size_t srec = sums_cnt ? sums_cnt : e->gs_rec;      // (XK_SUMS: doubles per rank -- one record, or the records of a launch's generations back to back)
    const size_t cnt = kind == XK_SUMS ? srec : (size_t)e->p.nl * e->p.ld;
    double* base = kind == XK_SUMS ? buf : buf + row0 * e->p.ld;
    double* mine = kind == XK_SUMS ? buf + (size_t)e->rank * srec : base + (size_t)e->p.off * e->p.ld;
    (kind == XK_Z ? e->bytes_z : kind == XK_SUMS ? e->bytes_sums : e->bytes_pos) += (int64_t)(sizeof(double) * cnt);
    if (e->peer_on) {
        if (kind == XK_Z) { DZCK(peer_push(e, XK_Z, buf, 0, row0, (unsigned long long)(e->z_pushed + 1))); e->z_pushed++; return 0; }
        if (kind == XK_SUMS) {
            DZCK(peer_push(e, XK_SUMS, buf, which, 0, (unsigned long long)(e->gs_pushed + 1), srec)); e->gs_pushed++;
            return peer_gate(e, XK_SUMS, (unsigned long long)e->gs_pushed);
        }
        DZCK(peer_push(e, XK_POS, buf, e->cp_idx, row0, (unsigned long long)(e->pos_pushed + 1))); e->pos_pushed++;
        return peer_gate(e, XK_POS, (unsigned long long)e->pos_pushed);
    }
    if (e->comm) {
        ncclResult_t r = g_rccl.AllGather(mine, base, cnt, ncclDouble, e->comm, e->stream);
        if (r != ncclSuccess) return fail(std::string("ncclAllGather: ") + (g_rccl.GetErrorString ? g_rccl.GetErrorString(r) : "error"));
        return 0;
    }
    if (!e->xcb) return fail("sharded run needs dz_comm_init_rccl, dz_peer_attach or dz_set_exchange");
    const size_t nranks = (size_t)e->p.N / e->p.nl;
    e->h_stage.resize(cnt * (nranks + 1));
    double* hs = e->h_stage.data(); double* hr = hs + cnt;
    HIPCK(hipMemcpyAsync(hs, mine, sizeof(double) * cnt, hipMemcpyDeviceToHost, e->stream));
    DZCK(sync_all(e));
    if (e->xcb(hs, hr, (int64_t)(sizeof(double) * cnt), e->xcb_user)) return fail("exchange callback failed");
    HIPCK(hipMemcpyAsync(base, hr, sizeof(double) * cnt * nranks, hipMemcpyHostToDevice, e->stream));
    DZCK(sync_all(e));
    return 0;
}

void point_shared(dz_engine* e)
{   // e->p's six pointers at the current copy of the shared adaptation state
    dz::Params& p = e->p; const int ncr = e->c.ncr, ng = e->c.ngamma;
    p.cr_probs = e->d_shared + (size_t)e->sh_cur * 3 * (ncr + ng); p.cr_delta = p.cr_probs + ncr; p.cr_n = p.cr_delta + ncr;
    p.g_probs = p.cr_n + ncr; p.g_delta = p.g_probs + ng; p.g_n = p.g_delta + ng;
}
// adapt_lag >= 1: the last generation whose update generation g decides with -- g - 1 - lag inside the burn-in, everything that was made from the
// hand-over on (g > crossover_burnin: Dream.py:385-415)
int64_t adapt_due(const dz_engine* e, int64_t g)
{
    return g > (int64_t)e->p.burnin ? e->ad_made : std::min<int64_t>(e->ad_made, g - 1 - (int64_t)e->c.adapt_lag);
}
// ... and the pending updates up to there added to the shared state, on their own (k_adapt_apply_pending: in place)
int adapt_apply_due(dz_engine* e, int64_t g)
{
    const int64_t due = adapt_due(e, g);
    if (due <= e->ad_applied) return 0;
    hipLaunchKernelGGL(dz::k_adapt_apply_pending, dim3(1), dim3(64), 0, e->stream, e->p, (const double*)e->d_DOT, (const double*)e->d_CNT, e->ad_nbp, e->ad_R1,
                       (long long)(e->ad_applied + 1), (long long)(e->ad_made + 1), (long long)g, e->c.adapt_lag);
    e->ad_applied = due;
    return launch_check("k_adapt_apply_pending");
}
// totals left by the last generation's adaptation that no launch has applied yet: the update on its own
int adapt_flush(dz_engine* e)
{
    if (e->c.adapt_lag > 0) return adapt_apply_due(e, e->gen);
    if (!e->adapt_pending) return 0;
    NCH_DISPATCH(e, hipLaunchKernelGGL(dz::k_adapt_apply<NCH>, dim3(1), dim3(64), 0, e->stream, e->p, (const double*)e->d_TOT, (const double*)e->d_CNT));
    e->adapt_pending = false;
    return launch_check("k_adapt_apply");
}
// adapt_lag >= 1: behind the totals of generations g .. g + n - 1 (ring slots), their bins' dot products; the updates are then "made"
int adapt_dots(dz_engine* e, uint32_t g, int n)
{
    NCH_DISPATCH(e, hipLaunchKernelGGL(dz::k_adapt_dots<NCH>, dim3(n), dim3(64), 0, e->stream, e->p, (const double*)e->d_TOT, (const double*)e->d_CNT, e->d_DOT,
                                       (long long)g, e->ad_R1, (long long)e->ad_tot_stride, e->ad_nbp));
    e->ad_made = (int64_t)g + n - 1;
    return launch_check("k_adapt_dots");
}
// the totals of the units' sums (k_adapt_totals) of generations g .. g + n - 1 (pr_ring: a launch that can hold several burn-in generations, adapt_lag
// >= 1, has left their units' sums in ring slots; else d_PR / d_PC hold one generation's); adapt_lag 0: the update itself (adapt_apply_wave) is left to the next persistent launch's prologue
// when `defer` says one follows, else made at once (k_adapt_apply); adapt_lag >= 1: the dot products follow, the update waits until it is due
int adapt_finish(dz_engine* e, bool defer, uint32_t g = 0, int n = 1, bool pr_ring = false)
{
    const dz::Params& p = e->p;
    const int nq = 2 + p.ncr + p.ngamma, units = (p.N + 15) / 16, nb = p.ncr + p.ngamma;
    const bool ring = e->c.adapt_lag > 0;
    hipLaunchKernelGGL(dz::k_adapt_totals, dim3((nq * p.d + 15) / 16 + 1, n), dim3(256), 0, e->stream, (const double*)e->d_PR, (const double*)e->d_PC, units, nq, p.d, p.ld, nb, e->d_TOT, e->d_CNT,
                       (long long)g, ring ? e->ad_R1 : 1, (long long)(pr_ring ? e->ad_pr_stride : 0), (long long)(pr_ring ? e->ad_pc_stride : 0), (long long)e->ad_tot_stride, ring ? e->ad_nbp : 0);
    DZCK(launch_check("k_adapt_totals"));
    if (ring) return adapt_dots(e, g, n);
    e->adapt_pending = true;
    return defer ? 0 : adapt_flush(e);
}

// the row the column sums of generation g are taken around: global chain 0's previous published position (contract v3).  Ranks that exchange
// group sums instead of positions get it with the records of generation g - 1 (k_group_totals), generation 0's from the start positions.
// adapt_lag = L >= 1: global chain 0's position after generation g - 1 - L (its start position before there is one)
const double* adapt_shift(const dz_engine* e, uint32_t g)
{
    if (e->c.adapt_lag > 0) {
        const int64_t hs = (int64_t)g - 1 - e->c.adapt_lag;
        return hs < 0 ? e->d_x0start : e->d_x0ring + (size_t)(hs % (2 * e->ad_R1)) * e->p.ld;
    }
    return (e->adapt_groups && g > 0) ? e->d_shift[(g - 1u) & 1u] : e->p.cp_prev;
}
// Sharded (whole groups per rank), adapt_lag >= 1, a launch of n burn-in generations g .. g + n - 1 whose units' sums (this rank's units) sit in the
// rings' slots: every generation's group sums into one record each, the n records of every rank everywhere in ONE exchange, then the totals of
// every generation (the same additions in the same order as adapt_generation makes them one generation at a time) and their dot products.
// Buffers by the parity of the LAUNCH (a peer may be one launch ahead); rank r's records of this launch at r * n * gs_rec.
int adapt_finish_groups(dz_engine* e, uint32_t g, int n)
{
    const dz::Params& p = e->p;
    const int units_l = p.nl / 16, gl = p.nl / 256, nq = 2 + p.ncr + p.ngamma, nb = p.ncr + p.ngamma, nbp = e->gs_nbp, R1 = e->ad_R1;
    const int par = (int)(e->gs_launches++ & 1);
    const size_t rstride = (size_t)n * e->gs_rec;
    hipLaunchKernelGGL(dz::k_adapt_groups, dim3((gl * nq * p.d + gl * nbp + p.ld + 255) / 256, n), dim3(256), 0, e->stream, (const double*)e->d_PR, (const double*)e->d_PC, units_l, nq, p.d, p.ld, nb, nbp,
                       (const double*)e->d_x0ring, e->d_GS[par] + (size_t)e->rank * rstride, (long long)g, R1, (long long)e->ad_pr_stride, (long long)e->ad_pc_stride, (long long)e->gs_rec, 2 * R1);
    DZCK(launch_check("k_adapt_groups"));
    DZCK(exchange_rows(e, XK_SUMS, e->d_GS[par], 0, par, rstride));
    hipLaunchKernelGGL(dz::k_group_totals, dim3((nq * p.d + nb + p.ld + 255) / 256, n), dim3(256), 0, e->stream, (const double*)e->d_GS[par], e->world, rstride, gl, nq, p.d, p.ld, nb, nbp,
                       e->d_TOT, e->d_CNT, e->d_x0ring, (long long)g, R1, (long long)e->gs_rec, (long long)e->ad_tot_stride, (long long)e->ad_nbp, 2 * R1);
    DZCK(launch_check("k_group_totals"));
    e->gs_last_gen = (int64_t)g + n - 1;
    return adapt_dots(e, g, n);
}
// fused = the generation's persistent launch has already left its units' sums in d_PR / d_PC (adapt_unit_sums in its epilogue)
int adapt_generation(dz_engine* e, uint32_t g, int gc0, int ngc, bool fused = false, bool defer = false)
{
    ProfScope ps(e, PR_ADAPT);
    const dz::Params& p = e->p;
    // lockstep generations (schedule S2): reduction contract v3 -- one pass over the positions makes, per unit of 16 chains, the column
    // sums the standard deviations need AND the per-bin column sums of squared jumps; their totals; the update.
    // A single chain's update (Dream.astep, schedule S1): the reference's own chain-by-chain form, all rows in row order (numpy's).
    const bool single = ngc != p.N;
    const bool ring = e->c.adapt_lag > 0;
    const int slot = ring ? (int)(g % (uint32_t)e->ad_R1) : 0;
    double* x0_out = ring ? e->d_x0ring + (size_t)(g % (uint32_t)(2 * e->ad_R1)) * p.ld : nullptr;      // global chain 0's position after this generation
    if (!single && e->adapt_groups) {
        // sharded, whole groups per rank: own units' sums -> own groups' sums -> every rank's record everywhere -> the totals (the same
        // additions in the same order as k_adapt_totals makes them from all units: dz_kernels.h)
        const int units_l = p.nl / 16, gl = p.nl / 256, nq = 2 + p.ncr + p.ngamma, nb = p.ncr + p.ngamma, nbp = e->gs_nbp, par = (int)(g & 1u);
        if (!ring && g > 0 && e->gs_last_gen != (int64_t)g - 1) return fail("sharded adaptation: the previous burn-in generation left no shift row");
        if (!fused) {
            hipLaunchKernelGGL(dz::k_adapt_partials, dim3(units_l), dim3(1024), 0, e->stream, p, g, e->d_PR, e->d_PC, p.off / 16, adapt_shift(e, g));
            DZCK(launch_check("k_adapt_partials"));
        }
        hipLaunchKernelGGL(dz::k_adapt_groups, dim3((gl * nq * p.d + gl * nbp + p.ld + 255) / 256), dim3(256), 0, e->stream, (const double*)e->d_PR, (const double*)e->d_PC, units_l, nq, p.d, p.ld, nb, nbp,
                           (const double*)(p.cp_new + (size_t)p.off * p.ld), e->d_GS[par] + (size_t)e->rank * e->gs_rec, 0ll, 1, 0ll, 0ll, 0ll, 0);
        DZCK(launch_check("k_adapt_groups"));
        DZCK(exchange_rows(e, XK_SUMS, e->d_GS[par], 0, par));
        hipLaunchKernelGGL(dz::k_group_totals, dim3((nq * p.d + nb + p.ld + 255) / 256), dim3(256), 0, e->stream, (const double*)e->d_GS[par], e->world, e->gs_rec, gl, nq, p.d, p.ld, nb, nbp,
                           e->d_TOT + (size_t)slot * e->ad_tot_stride, e->d_CNT + (size_t)slot * e->ad_nbp, ring ? x0_out : e->d_shift[par], 0ll, 1, 0ll, 0ll, 0ll, 0);
        DZCK(launch_check("k_group_totals"));
        e->gs_last_gen = (int64_t)g;
        if (ring) return adapt_dots(e, g, 1);
        e->adapt_pending = true;
        return defer ? 0 : adapt_flush(e);
    }
    if (!single) {
        if (ring) HIPCK(hipMemcpyAsync(x0_out, p.cp_new, sizeof(double) * p.ld, hipMemcpyDeviceToDevice, e->stream));
        if (!fused) {
            hipLaunchKernelGGL(dz::k_adapt_partials, dim3((p.N + 15) / 16), dim3(1024), 0, e->stream, p, g, e->d_PR, e->d_PC, 0, ring ? adapt_shift(e, g) : (const double*)nullptr);
            DZCK(launch_check("k_adapt_partials"));
        }
        return adapt_finish(e, defer, g, 1);
    }
    const int strip = p.N, nstrips = 1;
    const dim3 b(128), gcol((p.d + 127) / 128, nstrips);
    double* partial1 = e->d_partial + (size_t)((p.N + 63) / 64) * p.ld;
    hipLaunchKernelGGL(dz::k_strip_partial, gcol, b, 0, e->stream, p.cp_new, p.N, p.d, p.ld, e->d_mean, 0, e->d_partial, strip, 1);
    hipLaunchKernelGGL(dz::k_strip_dev, gcol, b, 0, e->stream, p.cp_new, p.N, p.d, p.ld, (const double*)e->d_partial, nstrips, partial1, e->d_mean, strip, 1);
    NCH_DISPATCH(e, hipLaunchKernelGGL(dz::k_jump<NCH>, dim3((p.N + dz::JUMP_CHAINS - 1) / dz::JUMP_CHAINS), dim3(64 * dz::JUMP_CHAINS), 0, e->stream, p, g, gc0, ngc,
                                       (const double*)partial1, nstrips, e->d_sd, e->d_sdc, e->d_dl, e->d_dlg, e->d_binc, e->d_bing));
    hipLaunchKernelGGL(dz::k_adapt_update, dim3(1), dim3(1024), (size_t)(dz::ADAPT_CHUNK + dz::ADAPT_CHUNK / 64) * 24, e->stream, p,
                       (const double*)e->d_dl, (const double*)e->d_dlg, (const int*)e->d_binc, (const int*)e->d_bing, e->d_binsum);
    if (e->d_own_cr)      // the chains that updated the shared probabilities adopt them (Dream.py:375, :383, :409-415)
        hipLaunchKernelGGL(dz::k_own_probs, dim3((ngc + 63) / 64), dim3(64), 0, e->stream, p, gc0 - p.off, ngc, (const int*)e->d_binc, (const int*)e->d_bing, 0, e->d_own_cr, e->d_own_g);
    return launch_check("adaptation kernels");
}

// Can every try of a multi-try proposal set be impossible (log density -inf or nan)?  Not with the built-in likelihoods under priors of
// unbounded support; yes with a host likelihood, and with a prior of bounded support unless hard boundaries keep every proposal inside it
// and away from an end where the log density is not finite (dz::covered, dz_prior_ext.h; for a uniform prior: inside its support).
// Those configurations take the multi-kernel path, which checks after the proposal set's evaluation and draws again (Dream.py:281-289).
bool redo_possible(const dz_engine* e)
{
    const dz::Params& p = e->p;
    if (p.k <= 1) return false;
    if (e->lk == LK_HOST) return true;
    if (e->lk == LK_MODULE && !e->lk_finite) return true;      // (a user's density may be -inf anywhere unless the caller promises otherwise: DZ_LIKE_ALWAYS_FINITE)
    const double inf = __builtin_huge_val();
    for (size_t j = 0; j < e->h_pkind.size(); ++j) {
        const bool have = j < e->h_mins.size(), shapes = e->prior_ext && j < e->h_ps1.size();
        if (!dz::covered(e->h_pkind[j], e->h_pa[j], e->h_pb[j], shapes ? e->h_ps1[j] : 0.0, shapes ? e->h_ps2[j] : 0.0, p.hard && have, have ? e->h_mins[j] : -inf, have ? e->h_maxs[j] : inf)) return true;
    }
    return false;
}
// every lane waits for everything queued so far on every other lane
int join_all(dz_engine* e)
{
    if (e->nlanes <= 1) return 0;
    for (int s = 0; s < e->nlanes; ++s) HIPCK(hipEventRecord(e->lane_ev[s], e->lane_stream[s]));
    for (int s = 0; s < e->nlanes; ++s)
        for (int t = 0; t < e->nlanes; ++t) if (t != s) HIPCK(hipStreamWaitEvent(e->lane_stream[s], e->lane_ev[t], 0));
    return 0;
}
// Dream.py:281-289: while every try of a chain's proposal set is impossible, the set is generated again with the same decisions
// (snooker, CR, DE pairs, gamma level) and evaluated again.  Redraw round r >= 1 takes its point and dimension streams from the Philox
// key seed + r * DZ_REDRAW_KEY_STEP, evaluated in place (the precomputed draw table holds round 0).  A round:
// k_redo_flags, k_propose over the listed chains whose flag is still set, the listed sets packed into the (not yet used)
// reference-set buffers, evaluated there -- a host likelihood sees only those points -- and their log densities scattered back.
// The list comes from one read-back of the flags; up to four rounds are queued per read-back (chains that succeed in between drop
// out by their flag: same result as a round-by-round loop, fewer host round trips).  The reference's loop is unbounded; after
// DZ_MAX_REDRAWS rounds the step is a rejection (k_accept: no finite try), deviation D1.
int redraw_impossible_sets(dz_engine* e, uint32_t g, int lc0, int lnc, hipStream_t st)
{
    dz::Params& p = e->p;
    if (!e->d_redo) DZCK(ealloc(e, &e->d_redo, (size_t)p.nl));
    if (!e->d_redo_list) DZCK(ealloc(e, &e->d_redo_list, (size_t)p.nl));
    if (!e->h_redo && hipHostMalloc((void**)&e->h_redo, (size_t)p.nl, hipHostMallocDefault) != hipSuccess) { e->h_redo = nullptr; return fail("hipHostMalloc (redraw flags) failed"); }
    if (!e->h_redo_list && hipHostMalloc((void**)&e->h_redo_list, sizeof(int32_t) * (size_t)p.nl, hipHostMallocDefault) != hipSuccess) { e->h_redo_list = nullptr; return fail("hipHostMalloc (redraw list) failed"); }
    static_assert(dz::MULTI_MAX_REDRAWS == DZ_MAX_REDRAWS, "redraw rounds");
    for (int round = 1; round <= DZ_MAX_REDRAWS;) {
        const dz::MultiLaunch fl = dz::redraw_plan(e->multi, lnc, 0, round).flags;
        hipLaunchKernelGGL(dz::k_redo_flags, g3(fl), b3(fl), 0, st, p, lc0, lnc, e->d_redo);
        DZCK(launch_check("k_redo_flags"));
        HIPCK(hipMemcpyAsync(e->h_redo, e->d_redo + lc0, (size_t)lnc, hipMemcpyDeviceToHost, st));
        HIPCK(hipStreamSynchronize(st));
        int n = 0;
        for (int t = 0; t < lnc; ++t) if (e->h_redo[t]) e->h_redo_list[n++] = lc0 + t;
        if (n == 0) break;
        HIPCK(hipMemcpyAsync(e->d_redo_list, e->h_redo_list, sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice, st));
        const dz::RedrawPlan R = dz::redraw_plan(e->multi, lnc, n, round);
        for (int b = 0; b < R.batch; ++b, ++round) {
            if (b) hipLaunchKernelGGL(dz::k_redo_flags, g3(R.flags), b3(R.flags), 0, st, p, lc0, lnc, e->d_redo);
            dz::Params pr = p;
            const uint64_t key = e->c.seed + (uint64_t)round * DZ_REDRAW_KEY_STEP;
            pr.k0 = (uint32_t)key; pr.k1 = (uint32_t)(key >> 32);
            pr.draws = nullptr; pr.redo_list = e->d_redo_list; pr.redo = e->d_redo;
            NCH_DISPATCH(e, DZ_KLAUNCH(e, PR_PROPOSE, st, dz::k_propose<NCH>, g3(R.propose), b3(R.propose), 0, pr, 0, g, (uint32_t)visible_rows(e), 0, n, R.sp0, 0, (int64_t)-1));
            DZCK(launch_check("propose(redraw)"));
            hipLaunchKernelGGL(dz::k_gather_sets, g3(R.gather), b3(R.gather), 0, st, p, (const int32_t*)e->d_redo_list, n, p.R);
            DZCK(eval_logp(e, p.R, R.points, p.r_prior, p.r_like, st));
            hipLaunchKernelGGL(dz::k_scatter_logp, g3(R.scatter), b3(R.scatter), 0, st, p, (const int32_t*)e->d_redo_list, n, (const double*)p.r_prior, (const double*)p.r_like);
            DZCK(launch_check("redraw gather/scatter"));
            e->redraw_rounds++;
        }
    }
    return 0;
}

// one transition of local chains [c0, c0+nc) at generation g.  Full range = a lockstep generation
// (schedule S2); a sub-range is the single-chain view used by Dream.astep: its end-of-generation
// updates (append, publish, adaptation) take effect immediately, as when the reference is driven
// round-robin in one process.  What is launched, on which stream group, with what geometry, and what the
// generation leaves for the next one: dz::generation_plan (dz_multi_select.h).
int one_generation(dz_engine* e, int c0, int nc, uint32_t g, bool traced, bool more_follow)
{
    dz::Params& p = e->p;
    const dz::GenerationPlan G = dz::generation_plan(e->multi, dz::MultiStep{c0, nc, g, traced, more_follow, (long long)e->ntrace}, e->carry);
    if (G.refuse == dz::REFUSE_SHARDED) return fail("single-chain stepping is not available on a sharded engine");
    if (G.refuse == dz::REFUSE_HISTORY_LAG) return fail("single-chain stepping (Dream.astep) appends with immediate effect: history_lag must be 0");
    if (G.refuse == dz::REFUSE_ADAPT_LAG) return fail("single-chain stepping (Dream.astep) updates the crossover probabilities with immediate effect: adapt_lag must be 0");
    DZCK(adapt_flush(e));               // (these kernels read the shared probabilities in place)
    DZCK(ensure_visible(e));
    const uint32_t Mv = (uint32_t)visible_rows(e);
    if (G.join_first) DZCK(join_all(e));
    p.own_cr = nullptr; p.own_g = nullptr;
    if (G.own_probs) {
        // Dream.astep chain by chain: every Dream instance decides with its OWN copy of the crossover / gamma-level probabilities
        // (Dream.py:134, :143; refreshed at :375, :383, :409-415) -- the shared vectors may have moved on through other chains' updates
        if (!e->d_own_cr) {
            DZCK(ealloc(e, &e->d_own_cr, (size_t)p.nl * p.ncr)); DZCK(ealloc(e, &e->d_own_g, (size_t)p.nl * p.ngamma));
            e->own_init.assign((size_t)p.nl, 0);
        }
        for (int c = c0; c < c0 + nc; ++c) if (!e->own_init[c]) {
            hipLaunchKernelGGL(dz::k_own_probs, dim3(1), dim3(64), 0, e->stream, p, c, 1, (const int*)nullptr, (const int*)nullptr, 1, e->d_own_cr, e->d_own_g);
            e->own_init[c] = 1;
        }
        p.own_cr = e->d_own_cr; p.own_g = e->d_own_g;
    }
    if (G.publish_start) {   // publish the start positions (Dream_shared_vars.current_positions)
        const size_t n = (size_t)p.nl * p.ld;
        hipLaunchKernelGGL(dz::k_copy_rows, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, e->stream, p.X, p.cp_new + (size_t)p.off * p.ld, n);
        DZCK(exchange_rows(e, XK_POS, p.cp_new, 0));
        if (e->c.adapt_lag > 0) HIPCK(hipMemcpyAsync(e->d_x0start, p.cp_new, sizeof(double) * p.ld, hipMemcpyDeviceToDevice, e->stream));      // global chain 0's start position
        DZCK(join_all(e));
    }
    p.draws = e->d_draws[g & 1]; p.draws_next = e->d_draws[(g + 1) & 1];
    p.ctl = e->d_ctl[g & 1]; p.ctl_next = e->d_ctl[(g + 1) & 1];
    if (G.append && e->M + G.nrows > e->c.history_capacity) return fail("history capacity exceeded");
    if (G.publish) {
        if (G.full) { e->cp_idx = (e->cp_idx + 1) % 3; p.cp_prev = p.cp_new; p.cp_new = e->d_cp[e->cp_idx]; }      // (three buffers: a peer may be one generation ahead)
        else {   // the jump of a single chain is measured from its state at the start of the step
            const size_t n = (size_t)nc * p.ld;
            hipLaunchKernelGGL(dz::k_copy_rows, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, e->stream, p.X + (size_t)c0 * p.ld, p.cp_prev + (size_t)(p.off + c0) * p.ld, n);
        }
    }
    const int k = p.k;
    const int64_t slot = G.slot, zbase = G.full ? e->M : e->M - (int64_t)(p.off + c0);
    const double* pending_qfin_r = e->carry.pending_qfin ? e->last_qpart : nullptr;      // the deferred accept's reference-set sums, still in the scratch array
    p.qfin_p = nullptr; p.qfin_r = nullptr; p.qfin_nrt = (p.d + 15) / 16;
    for (int i = 0; i < G.ngroups; ++i) {
        const dz::MultiGroup& q = G.grp[i];
        const int lc0 = q.c0, lnc = q.nc;
        hipStream_t st = e->lane_stream[q.stream];
        if (G.need_draws) hipLaunchKernelGGL(dz::k_draws, g3(q.draws), b3(q.draws), 0, st, p, g, lc0, lnc, e->d_draws[g & 1], e->d_ctl[g & 1]);
        if (G.prop0 == dz::PROP_STREAM) DZ_KLAUNCH(e, PR_PROPOSE, st, dz::k_propose_stream, g3(q.prop0), b3(q.prop0), 0, p, 0, g, Mv, lc0, lnc);
        else if (G.prop0 == dz::PROP_FUSED_ACCEPT) {      // (the Metropolis step of generation g - 1 in front: its reference set's row-tile sums may still be in the scratch array)
            p.qfin_r = pending_qfin_r; p.qfin_c0 = lc0; p.qfin_nc = lnc;
            NCH_DISPATCH(e, DZ_KLAUNCH(e, PR_PROPOSE, st, dz::k_propose<NCH>, g3(q.prop0), b3(q.prop0), 0, p, 0, g, Mv, lc0, lnc, 1, 1, e->carry.pending_slot));
            p.qfin_r = nullptr;
        } else if (G.prop0 == dz::PROP_CHAIN)
            NCH_DISPATCH(e, DZ_KLAUNCH(e, PR_PROPOSE, st, dz::k_propose<NCH>, g3(q.prop0), b3(q.prop0), 0, p, 0, g, Mv, lc0, lnc, G.sp0, 0, (int64_t)-1));
        DZCK(launch_check("propose"));                    // (PROP_NONE: made by the k_accept_propose launch of the generation before)
        DZCK(eval_logp(e, p.P + (size_t)lc0 * k * p.ld, q.n0, p.p_prior + (size_t)lc0 * k, p.p_like + (size_t)lc0 * k, st, G.qdefer));
        if (G.redo) DZCK(redraw_impossible_sets(e, g, lc0, lnc, st));
        if (q.n1 > 0) {
            if (G.qdefer) { p.qfin_p = e->last_qpart; p.qfin_c0 = lc0; p.qfin_nc = lnc; }
            if (G.streamed) DZ_KLAUNCH(e, PR_PROPOSE, st, dz::k_propose_stream, g3(q.prop1), b3(q.prop1), 0, p, 1, g, Mv, lc0, lnc);
            else NCH_DISPATCH(e, DZ_KLAUNCH(e, PR_PROPOSE, st, dz::k_propose<NCH>, g3(q.prop1), b3(q.prop1), 0, p, 1, g, Mv, lc0, lnc, G.sp1, 0, (int64_t)-1));
            DZCK(launch_check("propose(ref)"));
            p.qfin_p = nullptr;
            DZCK(eval_logp(e, p.R + (size_t)lc0 * (k - 1) * p.ld, q.n1, p.r_prior + (size_t)lc0 * (k - 1), p.r_like + (size_t)lc0 * (k - 1), st, G.qdefer));
            if (G.qdefer) { p.qfin_r = e->last_qpart; p.qfin_c0 = lc0; p.qfin_nc = lnc; }
        }
        if (G.acc == dz::ACC_ACCEPT_PROPOSE) {
            NCH_DISPATCH(e, DZ_KLAUNCH(e, PR_ACCEPT, st, dz::k_accept_propose<NCH>, g3(q.accept), b3(q.accept), q.accept.lds, p, g, zbase, lc0, lnc, slot, Mv));
            DZCK(launch_check("accept + propose"));
        } else if (G.acc == dz::ACC_ACCEPT) {
            NCH_DISPATCH(e, DZ_KLAUNCH(e, PR_ACCEPT, st, dz::k_accept<NCH>, g3(q.accept), b3(q.accept), 0, p, g, zbase, lc0, lnc, slot, G.append ? 1 : 0, G.publish ? 1 : 0, G.prep_next ? 1 : 0));
            DZCK(launch_check("accept"));
        }
        p.qfin_r = nullptr;
    }
    e->carry = G.next;
    if (G.publish || G.append) {         // shared state changed: the lanes meet before anything reads it
        if (G.join_last) DZCK(join_all(e));
        if (G.publish) {
            if (G.exchange_positions) DZCK(exchange_rows(e, XK_POS, p.cp_new, 0));      // (ranks that own whole groups exchange their groups' sums: adapt_generation)
            DZCK(adapt_generation(e, g, G.full ? 0 : p.off + c0, G.nrows));
        }
        if (G.append) { if (G.full) DZCK(exchange_rows(e, XK_Z, p.Z, (size_t)e->M)); e->M += G.nrows; e->napp += 1; }
    }
    if (G.swap) {      // temperature swap (core.py:185-221): after every chain's step and the updates above
        if (G.swap_join) DZCK(join_all(e));
        NCH_DISPATCH(e, hipLaunchKernelGGL(dz::k_pt_swap<NCH>, dim3(1), dim3(64), 0, e->stream, p, g, slot, G.publish ? 1 : 0));
        DZCK(launch_check("k_pt_swap"));
    }
    e->last_variant = "multi-kernel path"; e->last_kc = 0;
    for (int c = c0; c < c0 + nc; ++c) e->gen_c[c] = (int64_t)g + 1;
    if (G.full) e->gen = (int64_t)g + 1;
    if (slot >= 0) e->ntrace++;
    return 0;
}

// ---- persistent generation kernel (dz_megakernel.h) -------------------------------------------------
// chain states, gamma table and decisions ride in LDS next to the matrix whenever that fits (the packed triangle at
// d=100 leaves room; the dense square does not)
// Which instantiation runs, with what grid, block and LDS size, is decided in dz_mega_select.h: mega_choose once per dz_step from the facts gathered
// here -- the only selection code that reads the engine -- and mega_launch_plan once per launch.
static_assert(LK_MVN == dz::MEGA_LK_MVN && LK_MIX == dz::MEGA_LK_MIX && LK_MODULE == dz::MEGA_LK_MODULE, "likelihood kinds");
// ... and dz_multi_select.h decides the multi-kernel path's launches from the facts gathered here, the only selection code of that path that reads the engine
static_assert(LK_MVN == dz::MULTI_LK_MVN && LK_MIX == dz::MULTI_LK_MIX && LK_HOST == dz::MULTI_LK_HOST && LK_MODULE == dz::MULTI_LK_MODULE, "likelihood kinds");
dz::MultiShape multi_shape(const dz_engine* e)
{
    const dz::Params& p = e->p;
    dz::MultiShape s;
    s.d = p.d; s.ld = p.ld; s.k = p.k; s.depairs = p.depairs; s.nslots = p.nslots; s.nch = e->nch;
    s.tri = p.tri != 0; s.mtp_len = p.mtp_len; s.mu_zero = p.mu_zero != 0; s.have_prior = p.have_prior != 0;
    s.nl = p.nl; s.N = p.N; s.ncu = e->num_cu; s.nlanes = e->nlanes;
    s.lk = e->lk; s.lk_lanes = e->lk_lanes; s.lk_items = e->lk_items;
    s.redo_possible = redo_possible(e);
    s.adapt = e->adapt; s.tempering = e->tempering; s.world = e->world; s.thin = p.thin; s.burnin = p.burnin; s.history_lag = e->c.history_lag; s.adapt_lag = e->c.adapt_lag;
    s.adapt_groups = e->adapt_groups; s.trace = e->c.trace_capacity != 0;
    s.propose_split = e->propose_split; s.q_defer = e->q_defer; s.logp_gemm = e->logp_gemm;
    s.prior_ext = e->prior_ext;
    return s;
}
dz::MegaShape mega_shape(const dz_engine* e)
{
    const dz::Params& p = e->p;
    dz::MegaShape s;
    s.d = p.d; s.ld = p.ld; s.k = p.k; s.depairs = p.depairs; s.npt = p.npt; s.nslots = p.nslots; s.ncr = p.ncr; s.ngamma = p.ngamma; s.J = p.J;
    s.tri = p.tri != 0; s.mtp = p.Mtp != nullptr; s.hard = p.hard != 0; s.have_prior = p.have_prior != 0;
    s.nl = p.nl; s.N = p.N; s.ncu = e->num_cu;
    s.lk = e->lk; s.lk_items = e->lk_items; for (int i = 0; i < 4; ++i) s.gen_fn[i] = e->lk_gen_fn[i] != nullptr;
    s.redo_possible = e->multi.redo_possible;      // (multi_shape's evaluation: mega_select)
    s.ad_multi = e->ad_multi; s.ad_R1 = e->ad_R1; s.ad_nbp = e->ad_nbp; s.adapt_lag = e->c.adapt_lag; s.adapt_fused = e->adapt_fused; s.adapt_groups = e->adapt_groups;
    s.tempering = e->tempering; s.world = e->world;
    s.mega = e->mega; s.mega_d2 = e->mega_d2; s.mega_kc = e->mega_kc; s.mega_redo = e->mega_redo_on;
    s.prior_ext = e->prior_ext;
    return s;
}
// dz_step: the choice for its generations (nothing the selection reads changes inside a dz_step), and the two Params fields that follow from it
bool mega_select(dz_engine* e)
{
    e->mshape = mega_shape(e);
    e->mchoice = dz::mega_choose(e->mshape);
    e->p.pb_lds = e->mchoice.pb_lds ? 1 : 0;
    // uniform / flat priors whose supports contain the hard boundaries' box: the log prior of every proposal is one constant
    bool cst = e->p.have_prior && e->p.prior_nonormal && e->p.hard;
    for (size_t j = 0; cst && j < e->h_pkind.size(); ++j)
        if (e->h_pkind[j] == 2 && !(j < e->h_mins.size() && e->h_mins[j] >= e->h_pa[j] && e->h_maxs[j] <= e->h_pa[j] + e->h_pb[j])) cst = false;
    e->p.prior_const = cst ? 1 : 0;
    return e->mchoice.family != dz::MEGA_NONE;
}
// number of generations, starting at g, that one launch may cover: none of them publishes positions
// (crossover burn-in), and only the last one may append to the history
// The persistent kernels read Params through a pointer: the device copy is refreshed when a field THEY read has changed (the buffers
// that rotate from generation to generation -- published positions, the draw tables of the multi-kernel path -- are not among them).
int upload_params(dz_engine* e)
{
    dz::Params q = e->p;
    q.cp_prev = nullptr; q.cp_new = nullptr; q.draws = nullptr; q.draws_next = nullptr; q.ctl = nullptr; q.ctl_next = nullptr;
    q.own_cr = nullptr; q.own_g = nullptr; q.redo = nullptr; q.redo_list = nullptr;
    q.cr_probs = nullptr; q.cr_delta = nullptr; q.cr_n = nullptr; q.g_probs = nullptr; q.g_delta = nullptr; q.g_n = nullptr;     // (the persistent kernels get the state through Publish::sh)
    if (e->params_uploaded && memcmp(&e->p_shadow, &q, sizeof(dz::Params)) == 0) return 0;
    // (through a staging copy that outlives the call: the source of an asynchronous copy from pageable memory must not be a local)
    memcpy(&e->p_shadow, &q, sizeof(dz::Params));
    HIPCK(hipMemcpyAsync(e->d_params, &e->p_shadow, sizeof(dz::Params), hipMemcpyHostToDevice, e->stream));
    e->params_uploaded = true;
    return 0;
}
bool publishing(const dz_engine* e, uint32_t g) { return e->adapt && (int64_t)g < (int64_t)e->p.burnin + 1; }      // Dream.py:364
// History appends one launch of the persistent kernels may hold (the last one at its end), a: a generation behind i appends samples the rows
// of the first i - lag of them, and no generation of a launch may sample rows the launch itself writes (blocks do not meet): a <= lag + 1.
// Several GPUs (round 6): the rows the launch's own chains append travel AFTER the launch -- by an all-gather or through the host at once
// (then a <= lag + 1 as well: the exchange stays exposed, between two launches), or by the copy engines while the next launch computes: that
// launch must not sample them either, so 2 a - 1 <= lag (lag 1: one append per launch; lag 3: two, the 20 generations per launch one GPU runs).
int mega_appends_per_launch(const dz_engine* e)
{
    const int lag = e->c.history_lag;
    const int a = (e->world > 1 && e->peer_on) ? (lag + 1) / 2 : lag + 1;
    return std::max(1, std::min(a, e->mega_segs));
}
int mega_segment(const dz_engine* e, uint32_t g, int64_t remaining)
{
    // crossover burn-in: the positions are published and the probabilities adapted after every generation -- one generation per launch, or
    // (adapt_lag = L >= 1, one GPU, a kernel that makes its units' sums generation by generation: MegaChoice::burnin) up to L + 1 of them
    const bool pub0 = publishing(e, g);
    if (e->tempering) return remaining > 0 ? 1 : 0;       // parallel tempering: a temperature swap follows every generation (core.py:185-221)
    if (pub0 && !e->mchoice.burnin) return remaining > 0 ? 1 : 0;
    const int maxg = pub0 ? e->c.adapt_lag + 1 : MEGA_MAX_GEN;      // (adapt_lag <= 1023: dz_create)
    // A launch ends with a history append -- unless the rows it writes are not sampleable yet anyway (history_lag >= 1, every lagged append
    // already made): the kernel then makes the append itself and runs on, up to mega_appends_per_launch of them (the generations behind the
    // j-th one sample j * N more rows: all of them written -- and, sharded, received -- before the launch).
    const int lag = e->c.history_lag;
    int segs = (lag >= 1 && e->napp >= lag) ? mega_appends_per_launch(e) : 1;
    segs = (int)std::max<int64_t>(1, std::min<int64_t>(segs, (e->c.history_capacity - e->M) / std::max(1, e->p.N)));      // (an archive sized to the last append: no launch asks for more rows than one append at a time would)
    int n = 0, apps = 0;
    for (uint32_t gg = g; n < remaining && n < maxg; ++gg) {
        if (publishing(e, gg) != pub0) break;
        ++n;
        if (gg % (uint32_t)e->p.thin == 0 && ++apps >= segs) break;
    }
    return n;
}
// the translation units' launchers by row-tile count nrt = ld / 16 (dz_mega_tu.hip; 9..16: k_generations_d2 only)
const char* (*const MEGA_LAUNCHERS[17])(const dz::MegaLaunch&) = {
    nullptr, dz::mega_launch_nrt1, dz::mega_launch_nrt2, dz::mega_launch_nrt3, dz::mega_launch_nrt4, dz::mega_launch_nrt5, dz::mega_launch_nrt6, dz::mega_launch_nrt7, dz::mega_launch_nrt8,
    dz::mega_launch_nrt9, dz::mega_launch_nrt10, dz::mega_launch_nrt11, dz::mega_launch_nrt12, dz::mega_launch_nrt13, dz::mega_launch_nrt14, dz::mega_launch_nrt15, dz::mega_launch_nrt16};
int run_mega_segment(dz_engine* e, uint32_t g, int n, bool mega_follows)
{
    dz::Params& p = e->p;
    e->last_kc = 0;
    // the history appends of generations g .. g + n - 1 (one at the end, or -- mega_segment -- up to history_lag + 1, the last one at the end)
    int napps = 0, seg0 = 0;
    for (int i = 0; i < n; ++i) if ((g + (uint32_t)i) % (uint32_t)p.thin == 0) { if (!napps) seg0 = i + 1; ++napps; }
    const bool append_last = napps > 0;
    const bool ends_with_one = ((g + (uint32_t)n - 1) % (uint32_t)p.thin) == 0;
    // no generation of the launch may sample rows the launch itself writes: at most history_lag appends in front of any generation
    if (napps > 1 && (e->napp < e->c.history_lag || napps > mega_appends_per_launch(e) - (ends_with_one ? 0 : 1))) return fail("internal: too many history appends in one launch");
    if (append_last && e->M + (int64_t)napps * p.N > e->c.history_capacity) return fail("history capacity exceeded");
    DZCK(join_all(e));
    // the rows the launch samples have arrived: its last generation may sit behind all but the last of its own appends
    DZCK(ensure_visible(e, std::max(0, napps - (ends_with_one ? 1 : 0))));
    const bool publish = publishing(e, g);            // (then n == 1: mega_segment -- or, adapt_lag >= 1 and a burn-in mode, up to adapt_lag + 1)
    const bool ring = e->c.adapt_lag > 0;
    const int mmode = (publish && ring) ? e->mchoice.burnin : 0;
    const bool multi = mmode == 1;      // the launch applies the pending updates itself and makes its units' sums generation by generation
    const bool rmulti = mmode == 2;     // ... or leaves every generation's positions in the ring; the sums follow (k_adapt_partials_ring)
    if (ring && !mmode) DZCK(adapt_apply_due(e, (int64_t)g));   // (every generation of such a launch decides with the same state: one burn-in generation, or none)
    if (publish && n > 1 && !mmode) return fail("internal: several burn-in generations in a launch that cannot hold them");
    if (g == 0 && e->adapt) {   // publish the start positions (Dream_shared_vars.current_positions)
        const size_t nn = (size_t)p.nl * p.ld;
        hipLaunchKernelGGL(dz::k_copy_rows, dim3((unsigned)((nn + 255) / 256)), dim3(256), 0, e->stream, p.X, p.cp_new + (size_t)p.off * p.ld, nn);
        DZCK(exchange_rows(e, XK_POS, p.cp_new, 0));
        if (e->c.adapt_lag > 0) HIPCK(hipMemcpyAsync(e->d_x0start, p.cp_new, sizeof(double) * p.ld, hipMemcpyDeviceToDevice, e->stream));      // global chain 0's start position
    }
    if (publish && !rmulti) { e->cp_idx = (e->cp_idx + 1) % 3; p.cp_prev = p.cp_new; p.cp_new = e->d_cp[e->cp_idx]; }
    const size_t pos_stride = (size_t)p.N * p.ld; const int RP = e->c.adapt_lag + 2;
    if (rmulti) {      // the ring of published positions; the positions before this launch's first generation are the chains' states now
        if (!e->d_posring) { DZCK(ealloc(e, &e->d_posring, (size_t)RP * pos_stride)); DZCK(ealloc(e, &e->d_PG, (size_t)e->ad_R1 * e->ad_nbp)); }
        if (e->posring_gen != (int64_t)g - 1)
            HIPCK(hipMemcpyAsync(e->d_posring + (size_t)(((int64_t)g - 1 + RP) % RP) * pos_stride + (size_t)p.off * p.ld, p.X, sizeof(double) * (size_t)p.nl * p.ld, hipMemcpyDeviceToDevice, e->stream));
    }
    const int64_t slot0 = e->c.trace_capacity ? e->ntrace : -1;
    dz::Publish pub; pub.to = publish ? p.cp_new : nullptr; pub.shift = nullptr; pub.PR = nullptr; pub.PC = nullptr;
    pub.sh = p.cr_probs; pub.sh_out = nullptr; pub.TOT = nullptr; pub.CNT = nullptr; pub.c0 = 0; pub.c1 = p.nl;
    const bool applies = e->adapt_pending;      // the previous generation's adaptation totals: applied by this launch's prologue, new state into the other copy
    if (applies) { pub.TOT = e->d_TOT; pub.CNT = e->d_CNT; pub.sh_out = e->d_shared + (size_t)(e->sh_cur ^ 1) * 3 * (p.ncr + p.ngamma); }
    if (mmode) {      // adapt_lag >= 1: the pending updates, the rings, the table of probabilities per generation (Publish, dz_kernels.h)
        pub.multi = mmode; pub.lag = e->c.adapt_lag; pub.burnin = p.burnin; pub.nbp = e->ad_nbp; pub.pend0 = e->ad_applied + 1; pub.pend1 = e->ad_made + 1;
        pub.DOT = e->d_DOT; pub.CNTR = e->d_CNT; pub.sh_out = e->d_shared + (size_t)(e->sh_cur ^ 1) * 3 * (p.ncr + p.ngamma);
        if (multi) { pub.x0ring = e->d_x0ring; pub.x0start = e->d_x0start; pub.pr_stride = (long long)e->ad_pr_stride; pub.pc_stride = (long long)e->ad_pc_stride; pub.PR = e->d_PR; pub.PC = e->d_PC; }
        else { pub.to = e->d_posring; pub.pos_stride = (long long)pos_stride; pub.PG = e->d_PG; }
    }
    bool fused = false;
    const dz::MegaChoice& ch = e->mchoice;
    const dz::MegaLaunchPlan plan = dz::mega_launch_plan(ch, e->mshape, publish, applies);
    DZCK(upload_params(e));
    const int nrt = p.ld / 16;
    const uint32_t Mvis = (uint32_t)visible_rows(e);
    const int64_t zappend = append_last ? e->M : (int64_t)-1;
    std::string variant;
    for (int i = 0; i < plan.nparts; ++i) {
        const dz::MegaPart& part = plan.part[i];
        dz::Publish pp = pub; pp.c0 = part.c0; pp.c1 = part.c1;
        // crossover burn-in on one GPU: a block of 16 chains is one unit of the adaptation's column sums (contract v3) and makes them itself
        if (part.fused) { fused = true; pp.shift = adapt_shift(e, g); pp.PR = e->d_PR; pp.PC = e->d_PC; }
        const dim3 grid(part.grid), block(part.block);
        const bool full = part.f.pb;
        if (ch.family == dz::MEGA_USER) {      // the user's density inside the mixture kernel's scheme: the code object's own instantiation (dz_set_likelihood_module)
            const dz::Params* pp_ = (const dz::Params*)e->d_params; uint32_t g_ = g; int n_ = n; uint32_t M_ = Mvis; int64_t s_ = slot0, z_ = zappend; int seg_ = seg0;
            void* args[] = {&pp_, &g_, &n_, &M_, &s_, &z_, &seg_, &pp};
            const hipFunction_t fn = e->lk_gen_fn[(part.wide ? 2 : 0) + (full ? 1 : 0)];
            if (e->prof) {
                hipEvent_t ka = prof_event(e), kb = prof_event(e);
                e->ev[PR_GENERATIONS].emplace_back(ka, kb);
                HIPCK(hipExtModuleLaunchKernel(fn, grid.x * block.x, 1, 1, block.x, 1, 1, part.lds, e->stream, args, nullptr, ka, kb, 0));
            } else HIPCK(hipModuleLaunchKernel(fn, grid.x, 1, 1, block.x, 1, 1, (unsigned)part.lds, e->stream, args, nullptr));
            variant = part.wide ? (full ? "k_generations_user<full,wide>" : "k_generations_user<wide>") : (full ? "k_generations_user<full>" : "k_generations_user");
        } else if (ch.family == dz::MEGA_MIX) {      // (wide: 128 < d <= 256, a lane owns four dimensions; multi: several burn-in generations per launch)
            const auto kern = part.wide ? (full ? dz::k_generations_mix<true, false, 2> : dz::k_generations_mix<false, false, 2>)
                            : part.f.multi ? (full ? dz::k_generations_mix<true, true> : dz::k_generations_mix<false, true>)
                                           : (full ? dz::k_generations_mix<true> : dz::k_generations_mix<false>);
            DZ_KLAUNCH(e, PR_GENERATIONS, e->stream, kern, grid, block, part.lds, (const dz::Params*)e->d_params, g, n, Mvis, slot0, zappend, seg0, pp);
            variant = part.wide ? (full ? "k_generations_mix<full,wide>" : "k_generations_mix<wide>")
                    : part.f.multi ? (full ? "k_generations_mix<full,multi>" : "k_generations_mix<multi>") : (full ? "k_generations_mix<full>" : "k_generations_mix");
        } else {      // the instantiations live in one translation unit per row-tile count (dz_mega_tu.hip)
            dz::MegaLaunch ml;
            static_cast<dz::MegaFlags&>(ml) = part.f;
            ml.grid = grid; ml.block = block; ml.lds = part.lds; ml.st = e->stream; ml.ka = nullptr; ml.kb = nullptr;
            ml.pp = (const dz::Params*)e->d_params; ml.g = g; ml.n = n; ml.M = Mvis; ml.slot0 = slot0; ml.zappend = zappend; ml.seg0 = seg0; ml.publish = &pp;
            if (e->prof) { ml.ka = prof_event(e); ml.kb = prof_event(e); e->ev[PR_GENERATIONS].emplace_back(ml.ka, ml.kb); }
            if (nrt < 1 || nrt > 16) return fail("persistent kernel: ld out of range");
            char buf[96]; snprintf(buf, sizeof buf, MEGA_LAUNCHERS[nrt](ml), part.f.ch, part.f.wpc);
            variant += (variant.empty() ? "" : " + ") + std::string(buf);
            e->last_kc = part.f.kc;
        }
    }
    e->last_variant = variant + (rmulti ? " +ring" : "");
    DZCK(launch_check(ch.family == dz::MEGA_USER ? "dz_user_generations" : ch.family == dz::MEGA_MIX ? "k_generations_mix" : ch.family == dz::MEGA_D2 ? "k_generations_d2" : "k_generations"));
    if (applies) { e->sh_cur ^= 1; point_shared(e); e->adapt_pending = false; }
    if (mmode) { e->sh_cur ^= 1; point_shared(e); e->ad_applied = std::max(e->ad_applied, adapt_due(e, (int64_t)g + n - 1)); }
    // end of the generation(s): positions -> adaptation -> history append (schedule S2)
    const bool sharded = e->world > 1;      // (then the ranks own whole groups: their groups' sums travel, one exchange per launch -- adapt_finish_groups)
    if (multi) { ProfScope ps(e, PR_ADAPT); DZCK(sharded ? adapt_finish_groups(e, g, n) : adapt_finish(e, false, g, n, true)); }      // the totals and dot products of the launch's n generations
    else if (rmulti) {
        ProfScope ps(e, PR_ADAPT);
        hipLaunchKernelGGL(dz::k_adapt_partials_ring, dim3(sharded ? p.nl / 16 : (p.N + 15) / 16, n), dim3(1024), 0, e->stream, p, g, e->ad_R1, (const double*)e->d_posring, (long long)pos_stride,
                           (const double*)e->d_PG, e->ad_nbp, e->d_PR, e->d_PC, (long long)e->ad_pr_stride, (long long)e->ad_pc_stride, e->d_x0ring, (const double*)e->d_x0start, p.off / 16);
        DZCK(launch_check("k_adapt_partials_ring"));
        DZCK(sharded ? adapt_finish_groups(e, g, n) : adapt_finish(e, false, g, n, true));
        e->posring_gen = (int64_t)g + n - 1;
        p.cp_new = e->d_posring + (size_t)(e->posring_gen % RP) * pos_stride;      // (what a later launch that is not of this kind measures its jumps from)
    }
    else if (publish) {
        if (!e->adapt_groups) DZCK(exchange_rows(e, XK_POS, p.cp_new, 0));      // (ranks that own whole groups exchange their groups' sums instead: adapt_generation)
        DZCK(adapt_generation(e, g, 0, p.N, fused, mega_follows));
    }
    for (int a = 0; a < napps; ++a) { DZCK(exchange_rows(e, XK_Z, p.Z, (size_t)e->M)); e->M += p.N; e->napp += 1; }
    if (e->tempering) {          // (then n == 1) the temperature swap: after every chain's step and the updates above, as on the multi-kernel path
        NCH_DISPATCH(e, hipLaunchKernelGGL(dz::k_pt_swap<NCH>, dim3(1), dim3(64), 0, e->stream, p, g, slot0, publish ? 1 : 0));
        DZCK(launch_check("k_pt_swap"));
    }
    e->carry.need_join = true;
    e->carry.draws_gen = -1;
    e->gen = (int64_t)g + n;
    for (auto& gcv : e->gen_c) gcv = e->gen;
    if (slot0 >= 0) e->ntrace += n;
    return 0;
}

// The engine's path switches: environment variables that force or forbid a path for the tests and measurements, read once when the engine is
// made.  The selection logic reads only the fields set here.  _capi.ENGINE_SWITCHES lists the same names (every rank of a sharded run must agree).
void read_switches(dz_engine* e)
{
    if (const char* kv = getenv("DZ_MEGA")) e->mega = atoi(kv) != 0;
    if (const char* kv = getenv("DZ_MEGA_D2")) e->mega_d2 = atoi(kv);
    if (const char* kv = getenv("DZ_MEGA_SEGS")) e->mega_segs = std::max(1, atoi(kv));
    if (const char* kv = getenv("DZ_MEGA_KC")) e->mega_kc = atoi(kv) != 0;
    if (const char* kv = getenv("DZ_MEGA_REDO")) e->mega_redo_on = atoi(kv) != 0;
    if (const char* kv = getenv("DZ_MEGA_USER")) e->mega_user = atoi(kv) != 0;
    if (const char* kv = getenv("DZ_PROPOSE_SPLIT")) e->propose_split = atoi(kv);
    if (const char* kv = getenv("DZ_LOGP_GEMM")) e->logp_gemm = atoi(kv) != 0;
    if (const char* kv = getenv("DZ_QFIN")) e->q_defer = atoi(kv) != 0;
    if (const char* kv = getenv("DZ_STREAMS")) e->nlanes = atoi(kv);      // (chain groups on separate streams: clamped in dz_create)
    if (const char* kv = getenv("DZ_ADAPT_FUSED")) e->adapt_fused = atoi(kv) != 0;
    if (const char* kv = getenv("DZ_ADAPT_MULTI")) e->adapt_multi_on = atoi(kv) != 0;
    if (const char* kv = getenv("DZ_ADAPT_GROUPS")) e->adapt_groups_on = atoi(kv) != 0;
}

}  // namespace

extern "C" {

int dz_version(void) { return DZ_VERSION; }
const char* dz_last_error(void) { return g_err.c_str(); }
int dz_device_count(int32_t* count)
{
    int n = 0;
    hipError_t err = hipGetDeviceCount(&n);
    if (err != hipSuccess) { *count = 0; return fail(std::string("hipGetDeviceCount: ") + hipGetErrorString(err)); }
    *count = n; return 0;
}

int dz_create(const dz_config* cfg, dz_engine** out)
{
    if (!cfg || !out) return fail("null argument");
    if (cfg->ndim < 1 || cfg->nchains < 1 || cfg->nchains_local < 1 || cfg->multitry < 1) return fail("bad sizes");
    if (cfg->ndim > 1024) return fail("ndim > 1024 not supported by this build");
    if (cfg->multitry == 2) return fail("multitry=2 is broken in the reference (Dream.py:867-868); rejected");
    if (cfg->multitry > dz::MAXK) return fail("multitry too large");
    if (cfg->depairs < 1 || cfg->depairs > dz::MAXPAIR) return fail("DEpairs must be 1..8");
    if (cfg->ncr < 1 || cfg->ngamma < 1 || cfg->ncr > 32 || cfg->ngamma > 32) return fail("bad nCR/gamma_levels");
    if (cfg->schedule != 2) return fail("the device engine runs schedule 2 (lockstep generations) only");
    if (cfg->chain_offset < 0 || cfg->chain_offset + cfg->nchains_local > cfg->nchains) return fail("bad shard");
    if (cfg->nchains % cfg->nchains_local) return fail("nchains must be a multiple of nchains_local");
    if (cfg->history_thin < 1) return fail("history_thin must be >= 1");
    if (cfg->history_lag < 0 || cfg->history_lag > 64) return fail("history_lag must be 0..64");
    if (cfg->adapt_lag < 0 || cfg->adapt_lag > 1023 || cfg->reserved0 != 0) return fail("adapt_lag must be 0..1023 (and dz_config.reserved0 zero)");
    int ndev = 0;
    hipError_t derr = hipGetDeviceCount(&ndev);
    if (derr != hipSuccess || ndev < 1) return fail("no HIP device available: libdreamzs has no CPU fallback");
    HIPCK(hipSetDevice(cfg->device));
    dz_engine* e = new dz_engine();
    e->c = *cfg;
    e->gen_c.assign((size_t)cfg->nchains_local, 0);
    static_assert(dz::DZ_MAX_REDRAWS_DEV == DZ_MAX_REDRAWS && dz::DZ_REDRAW_KEY_STEP_DEV == DZ_REDRAW_KEY_STEP, "redraw constants");
    read_switches(e);
    dz::Params& p = e->p;
    p.N = cfg->nchains; p.nl = cfg->nchains_local; p.off = cfg->chain_offset; p.d = cfg->ndim;
    p.ld = (cfg->ndim + 15) / 16 * 16;
    p.k = cfg->multitry; p.depairs = cfg->depairs; p.ncr = cfg->ncr; p.ngamma = cfg->ngamma; p.thin = cfg->history_thin;
    p.burnin = cfg->crossover_burnin; p.adapt_cr = cfg->adapt_crossover; p.adapt_g = cfg->adapt_gamma; p.hard = 0;   // set by dz_set_bounds
    p.k0 = (uint32_t)cfg->seed; p.k1 = (uint32_t)(cfg->seed >> 32);
    p.lamb = cfg->lamb; p.zeta = cfg->zeta; p.snooker = cfg->snooker; p.pgu = cfg->p_gamma_unity; p.T = cfg->temperature;
    {   // contract constants made once (dz_device.h uniform16; dz_kernels.h crossover_threshold)
        const double low = -cfg->lamb, high = cfg->lamb;
        p.ec1 = (high - low) * (1.0 / 65536.0); p.ec0 = low + (high - low) * (1.0 / 131072.0);
        for (int m = 0; m < 32; ++m) p.crthr[m] = m < cfg->ncr ? dz::crossover_threshold((double)(m + 1) / (double)cfg->ncr) : 0u;
        const double q = std::min(1.0, std::max(0.0, cfg->p_gamma_unity));
        p.pgu_thr = (unsigned long long)std::ceil(std::ldexp(q, 53));
        const double sn = std::min(1.0, std::max(0.0, cfg->snooker));
        p.snk_thr = (unsigned long long)std::ceil(std::ldexp(sn, 53));
    }
    const int chunks = (p.ld + 127) / 128;
    e->nch = chunks <= 1 ? 1 : chunks <= 2 ? 2 : chunks <= 4 ? 4 : 8;
    e->adapt = cfg->adapt_crossover || cfg->adapt_gamma;
    e->world = cfg->nchains / cfg->nchains_local; e->rank = cfg->chain_offset / cfg->nchains_local;
    HIPCK(hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking));
    {
        // chain groups on separate streams (DZ_STREAMS, default 1): 2 gains ~3% at 4096 chains but shows occasional 2x-slow passes
        e->nlanes = std::max(1, std::min(8, e->nlanes));
        if (cfg->nchains_local < 64 * e->nlanes) e->nlanes = 1;
        e->lane_stream[0] = e->stream;
        for (int s = 1; s < e->nlanes; ++s) HIPCK(hipStreamCreateWithFlags(&e->lane_stream[s], hipStreamNonBlocking));
        for (int s = 0; s < e->nlanes; ++s) HIPCK(hipEventCreateWithFlags(&e->lane_ev[s], hipEventDisableTiming));
        for (int s = 0; s < 4; ++s) HIPCK(hipEventCreateWithFlags(&e->ra_ev[s], hipEventDisableTiming));
    }
    { hipDeviceProp_t prop; if (hipGetDeviceProperties(&prop, cfg->device) == hipSuccess && prop.multiProcessorCount > 0) e->num_cu = prop.multiProcessorCount; }
    const size_t ld = p.ld, nl = p.nl, N = p.N, k = p.k, tc = (size_t)cfg->trace_capacity;
    int rc = 0;
    rc |= ealloc(e, &p.Z, (size_t)cfg->history_capacity * ld);
    rc |= ealloc(e, &p.X, nl * ld); rc |= ealloc(e, &p.lprior, nl); rc |= ealloc(e, &p.llike, nl);
    rc |= ealloc(e, &p.P, nl * k * ld); rc |= ealloc(e, &p.R, nl * k * ld);
    rc |= ealloc(e, &p.p_prior, nl * k); rc |= ealloc(e, &p.p_like, nl * k); rc |= ealloc(e, &p.p_slogp, nl * k);
    rc |= ealloc(e, &p.r_prior, nl * k); rc |= ealloc(e, &p.r_like, nl * k); rc |= ealloc(e, &p.r_slogp, nl * k);
    rc |= ealloc(e, &p.cur_snk, nl);
    p.npt = 1 + (2 * cfg->depairs + 3) / 4; p.nslots = 3 + (2 * cfg->multitry - 1) * p.npt;
    rc |= ealloc(e, &e->d_draws[0], nl * (size_t)p.nslots); rc |= ealloc(e, &e->d_draws[1], nl * (size_t)p.nslots);
    rc |= ealloc(e, &e->d_ctl[0], nl); rc |= ealloc(e, &e->d_ctl[1], nl);
    rc |= ealloc(e, &p.sel, nl);
#ifdef DZ_EXPERIMENTS
    { void* hp = nullptr; if (hipHostMalloc(&hp, (size_t)4 * nl * 16 * 8, hipHostMallocDefault) == hipSuccess) { memset(hp, 0, (size_t)4 * nl * 16 * 8); p.dbg = (unsigned long long*)hp; } }
#endif
    rc |= ealloc(e, &e->d_params, 1);
    rc |= ealloc(e, &e->d_redraw_count, 1); p.redraw_count = e->d_redraw_count;
    rc |= ealloc(e, &e->d_mins, ld); rc |= ealloc(e, &e->d_maxs, ld);
    rc |= ealloc(e, &e->d_gtab, (size_t)cfg->ngamma * cfg->depairs * p.d);
    rc |= ealloc(e, &e->d_shared, (size_t)2 * 3 * (cfg->ncr + cfg->ngamma));
    rc |= ealloc(e, &e->d_pkind, ld); rc |= ealloc(e, &e->d_pa, ld); rc |= ealloc(e, &e->d_pb, ld); rc |= ealloc(e, &e->d_plogb, ld); rc |= ealloc(e, &e->d_pc2, ld);
    if (e->adapt) {
        for (int i = 0; i < 3; ++i) rc |= ealloc(e, &e->d_cp[i], N * ld);
        p.cp_prev = e->d_cp[0]; p.cp_new = e->d_cp[1]; e->cp_idx = 1;
        rc |= ealloc(e, &e->d_partial, (size_t)2 * ((N + 63) / 64) * ld);      // strip sums of pass 0 | of pass 1
        rc |= ealloc(e, &e->d_mean, ld); rc |= ealloc(e, &e->d_sd, ld); rc |= ealloc(e, &e->d_sdc, ld);
        rc |= ealloc(e, &e->d_dl, N); rc |= ealloc(e, &e->d_dlg, N); rc |= ealloc(e, &e->d_binc, N); rc |= ealloc(e, &e->d_bing, N);
        rc |= ealloc(e, &e->d_binsum, (size_t)2 * ((N + 63) / 64) * (cfg->ncr + cfg->ngamma));
        const size_t nq = 2 + (size_t)cfg->ncr + cfg->ngamma, units = (N + 15) / 16;
        // adapt_lag = L >= 1: rings of L + 1 generations (engine fields ad_*); several burn-in generations per launch on one GPU (ad_multi)
        e->ad_R1 = cfg->adapt_lag + 1; e->ad_nbp = (cfg->ncr + cfg->ngamma + 1) & ~1;
        // sharded, and this rank owns whole groups of 256 chains (then every rank does: equal shards): the burn-in exchanges group sums
        const bool groups = e->world > 1 && e->adapt_groups_on && p.off % 256 == 0 && p.nl % 256 == 0;
        // (several GPUs: only ranks that exchange group sums -- the records of a launch's generations travel in one exchange, adapt_finish_groups)
        e->ad_multi = cfg->adapt_lag > 0 && (e->world == 1 || groups) && e->adapt_multi_on;
        e->ad_tot_stride = cfg->adapt_lag > 0 ? nq * ld : 0;
        e->ad_pr_stride = units * nq * ld; e->ad_pc_stride = units * (size_t)(cfg->ncr + cfg->ngamma);
        const size_t prs = e->ad_multi ? (size_t)e->ad_R1 : 1;
        rc |= ealloc(e, &e->d_PR, prs * e->ad_pr_stride); rc |= ealloc(e, &e->d_PC, prs * e->ad_pc_stride);
        rc |= ealloc(e, &e->d_TOT, (size_t)e->ad_R1 * nq * ld); rc |= ealloc(e, &e->d_CNT, (size_t)e->ad_R1 * e->ad_nbp);
        if (cfg->adapt_lag > 0) {
            rc |= ealloc(e, &e->d_DOT, (size_t)e->ad_R1 * e->ad_nbp);
            rc |= ealloc(e, &e->d_x0ring, (size_t)2 * e->ad_R1 * ld); rc |= ealloc(e, &e->d_x0start, ld);
        }
        if (groups) {
            e->adapt_groups = true;
            e->gs_nbp = (cfg->ncr + cfg->ngamma + 15) / 16 * 16;
            e->gs_rec = (size_t)(p.nl / 256) * (nq * ld + (size_t)e->gs_nbp) + ld;
            // (adapt_lag = L >= 1: room for the records of a launch of L + 1 generations from every rank)
            for (int i = 0; i < 2; ++i) { rc |= ealloc(e, &e->d_GS[i], (size_t)e->world * e->gs_rec * (e->ad_multi ? (size_t)e->ad_R1 : 1)); rc |= ealloc(e, &e->d_shift[i], ld); }
        }
    }
    if (tc) {
        p.tcap = (long long)tc;
        rc |= ealloc(e, &p.tX, tc * nl * ld); rc |= ealloc(e, &p.tlogp, tc * nl);
        rc |= ealloc(e, &p.tmoved, tc * nl); rc |= ealloc(e, &p.tsnk, tc * nl); rc |= ealloc(e, &p.ttry, tc * nl); rc |= ealloc(e, &p.tcr, tc * nl);
    }
    rc |= ealloc(e, &e->d_cmean, nl * (size_t)p.d); rc |= ealloc(e, &e->d_cvar, nl * (size_t)p.d); rc |= ealloc(e, &e->d_rhat, (size_t)p.d);
    if (rc) { dz_destroy(e); return -1; }
    p.mins = e->d_mins; p.maxs = e->d_maxs; p.gtab = e->d_gtab;
    point_shared(e);
    p.pkind = e->d_pkind; p.pa = e->d_pa; p.pb = e->d_pb; p.plogb = e->d_plogb; p.pc2 = e->d_pc2; p.have_prior = 0; p.prior_nonormal = 1;
    // defaults: unbounded, uniform CR / gamma-level probabilities (Dream.py:134, :143), computed gamma table
    {
        std::vector<double> lo(ld, -HUGE_VAL), hi(ld, HUGE_VAL);
        HIPCK(hipMemcpy(e->d_mins, lo.data(), sizeof(double) * ld, hipMemcpyHostToDevice));
        HIPCK(hipMemcpy(e->d_maxs, hi.data(), sizeof(double) * ld, hipMemcpyHostToDevice));
        std::vector<double> sh((size_t)3 * (cfg->ncr + cfg->ngamma), 0.0);
        for (int m = 0; m < cfg->ncr; ++m) sh[m] = 1.0 / (double)cfg->ncr;
        for (int m = 0; m < cfg->ngamma; ++m) sh[(size_t)3 * cfg->ncr + m] = 1.0 / (double)cfg->ngamma;
        HIPCK(hipMemcpy(e->d_shared, sh.data(), sizeof(double) * sh.size(), hipMemcpyHostToDevice));
    }
    *out = e;
    return dz_set_gamma_table(e, nullptr);
}

int dz_destroy(dz_engine* e)
{
#ifdef DZ_EXPERIMENTS
    if (e && e->p.dbg) {
        hipDeviceSynchronize();
        if (FILE* f = fopen("gpurun_out/stamps.bin", "wb")) { fwrite(e->p.dbg, 8, (size_t)4 * e->p.nl * 16, f); fclose(f); }
    }
#endif
    if (!e) return 0;
    (void)hipSetDevice(e->c.device);
    for (int s2 = 0; s2 < e->nlanes; ++s2) if (e->lane_stream[s2]) (void)hipStreamSynchronize(e->lane_stream[s2]);
    for (int s2 = 1; s2 < e->nlanes; ++s2) if (e->lane_stream[s2]) (void)hipStreamDestroy(e->lane_stream[s2]);
    for (int s2 = 0; s2 < e->nlanes; ++s2) if (e->lane_ev[s2]) (void)hipEventDestroy(e->lane_ev[s2]);
    for (int s2 = 0; s2 < 4; ++s2) if (e->ra_ev[s2]) (void)hipEventDestroy(e->ra_ev[s2]);
    for (auto& v : e->ev) for (auto& pr : v) { (void)hipEventDestroy(pr.first); (void)hipEventDestroy(pr.second); }
    for (hipEvent_t x : e->ev_pool) (void)hipEventDestroy(x);
    if (e->comm && g_rccl.CommDestroy) g_rccl.CommDestroy(e->comm);
    if (e->lk_module) (void)hipModuleUnload(e->lk_module);
    if (e->d_lk_data) (void)hipFree(e->d_lk_data);
    if (e->out_module) (void)hipModuleUnload(e->out_module);
    if (e->d_out_data) (void)hipFree(e->d_out_data);
    if (e->d_out) (void)hipFree(e->d_out);
    if (e->d_out_like) (void)hipFree(e->d_out_like);
    for (auto& pr : e->peers) {
        if (pr.st) { (void)hipStreamSynchronize(pr.st); (void)hipStreamDestroy(pr.st); }
        if (pr.Z) (void)hipIpcCloseMemHandle(pr.Z);
        if (pr.flags) (void)hipIpcCloseMemHandle(pr.flags);
        for (double* q : pr.cp) if (q) (void)hipIpcCloseMemHandle(q);
        for (double* q : pr.gs) if (q) (void)hipIpcCloseMemHandle(q);
    }
    for (hipEvent_t x : e->push_ev) if (x) (void)hipEventDestroy(x);
    if (e->h_gate) (void)hipHostFree(e->h_gate);
    for (void* q : e->to_free) (void)hipFree(q);
    if (e->d_scratch) (void)hipFree(e->d_scratch);
    if (e->d_qpart) (void)hipFree(e->d_qpart);
    if (e->d_items) (void)hipFree(e->d_items);
    if (e->h_pin) (void)hipHostFree(e->h_pin);
    for (hipEvent_t x : e->pin_ev) if (x) (void)hipEventDestroy(x);
    if (e->h_redo) (void)hipHostFree(e->h_redo);
    if (e->h_redo_list) (void)hipHostFree(e->h_redo_list);
    if (e->copy_stream) { (void)hipStreamSynchronize(e->copy_stream); (void)hipStreamDestroy(e->copy_stream); }
    for (hipEvent_t ev : e->copy_ev) if (ev) (void)hipEventDestroy(ev);
    if (e->stream) (void)hipStreamDestroy(e->stream);
    delete e;
    return 0;
}

int dz_set_bounds(dz_engine* e, const double* mins, const double* maxs)
{
    HIPCK(hipSetDevice(e->c.device));
    bool any_finite = false;
    for (int j = 0; j < e->p.d; ++j) any_finite = any_finite || std::isfinite(mins[j]) || std::isfinite(maxs[j]);
    e->p.hard = (e->c.hardboundaries && any_finite) ? 1 : 0;     // with all bounds infinite the reflection code can never trigger
    e->h_mins.assign(mins, mins + e->p.d); e->h_maxs.assign(maxs, maxs + e->p.d);
    DZCK(upload_padded(e, e->d_mins, mins, 1, -HUGE_VAL));
    return upload_padded(e, e->d_maxs, maxs, 1, HUGE_VAL);
}

int dz_set_gamma_table(dz_engine* e, const double* table)
{   // Dream.py:172-179
    HIPCK(hipSetDevice(e->c.device));
    const int d = e->p.d, ng = e->c.ngamma, np = e->c.depairs;
    std::vector<double> t((size_t)ng * np * d);
    if (table) memcpy(t.data(), table, sizeof(double) * t.size());
    else {
        double dec = 1.0;
        for (int lev = 1; lev <= ng; ++lev) {
            for (int delta = 1; delta <= np; ++delta)
                for (int dp = 1; dp <= d; ++dp)
                    t[((size_t)(lev - 1) * np + (delta - 1)) * d + (dp - 1)] = (2.38 / std::sqrt((double)(2 * delta) * (double)dp)) / dec;
            dec = dec * 2.0;
        }
    }
    HIPCK(hipMemcpy(e->d_gtab, t.data(), sizeof(double) * t.size(), hipMemcpyHostToDevice));
    return 0;
}

int dz_set_history(dz_engine* e, const double* Z, int64_t rows)
{
    HIPCK(hipSetDevice(e->c.device));
    if (rows > e->c.history_capacity) return fail("history exceeds capacity");
    if (rows > 0xffffffffll) return fail("history too long");
    // (the peers' flag words count this rank's appends from the attach on: an archive reset underneath them would leave the gates
    //  comparing exchange numbers of two different histories)
    if (e->peer_on) return fail("dz_set_history: the archive of an engine attached to the peer transport cannot be reset (set it before dz_peer_attach)");
    DZCK(upload_padded(e, e->p.Z, Z, (int)rows, 0.0));
    e->M = rows; e->napp = 0;
    return 0;
}

int dz_set_state(dz_engine* e, const double* X, const double* prior, const double* like)
{
    HIPCK(hipSetDevice(e->c.device));
    DZCK(upload_padded(e, e->p.X, X, e->p.nl, 0.0));
    if (prior && like) {
        HIPCK(hipMemcpy(e->p.lprior, prior, sizeof(double) * e->p.nl, hipMemcpyHostToDevice));
        HIPCK(hipMemcpy(e->p.llike, like, sizeof(double) * e->p.nl, hipMemcpyHostToDevice));
        e->have_logp = true;
    } else e->have_logp = false;
    return 0;
}

int dz_set_cr_probs(dz_engine* e, const double* pr, int32_t n)
{
    if (n != e->c.ncr) return fail("nCR mismatch");
    HIPCK(hipSetDevice(e->c.device));
    DZCK(adapt_flush(e));
    DZCK(sync_all(e));
    HIPCK(hipMemcpy(e->p.cr_probs, pr, sizeof(double) * n, hipMemcpyHostToDevice));
    std::fill(e->own_init.begin(), e->own_init.end(), 0);
    e->carry.draws_gen = -1;
    return 0;
}
int dz_set_gamma_probs(dz_engine* e, const double* pr, int32_t n)
{
    if (n != e->c.ngamma) return fail("ngamma mismatch");
    HIPCK(hipSetDevice(e->c.device));
    DZCK(adapt_flush(e));
    DZCK(sync_all(e));
    HIPCK(hipMemcpy(e->p.g_probs, pr, sizeof(double) * n, hipMemcpyHostToDevice));
    std::fill(e->own_init.begin(), e->own_init.end(), 0);
    e->carry.draws_gen = -1;
    return 0;
}

int dz_set_prior(dz_engine* e, const int32_t* kind, const double* a, const double* b)
{
    HIPCK(hipSetDevice(e->c.device));
    const int d = e->p.d;
    bool any = false;
    for (int j = 0; j < d; ++j) { if (kind[j] < 0 || kind[j] > 2) return fail("prior kind must be 0,1,2"); any = any || kind[j] != 0; }
    HIPCK(hipMemcpy(e->d_pkind, kind, sizeof(int32_t) * d, hipMemcpyHostToDevice));
    HIPCK(hipMemcpy(e->d_pa, a, sizeof(double) * d, hipMemcpyHostToDevice));
    HIPCK(hipMemcpy(e->d_pb, b, sizeof(double) * d, hipMemcpyHostToDevice));
    {   // Params::pc2: normal: the reciprocal of the scale; uniform: the upper end of the support
        std::vector<double> c2((size_t)d, 0.0);
        bool normal = false;
        for (int j = 0; j < d; ++j) { c2[j] = kind[j] == 1 ? 1.0 / b[j] : (kind[j] == 2 ? a[j] + b[j] : 0.0); normal = normal || kind[j] == 1; }
        HIPCK(hipMemcpy(e->d_pc2, c2.data(), sizeof(double) * d, hipMemcpyHostToDevice));
        e->p.prior_nonormal = normal ? 0 : 1;
    }
    hipLaunchKernelGGL(dz::k_prior_consts, dim3((d + 127) / 128), dim3(128), 0, e->stream, (const double*)e->d_pb, d, e->d_plogb);
    DZCK(launch_check("k_prior_consts"));
    e->p.have_prior = any ? 1 : 0;
    e->h_pkind.assign(kind, kind + d); e->h_pa.assign(a, a + d); e->h_pb.assign(b, b + d);
    e->prior_ext = false;
    return 0;
}

// Every dimension's row of the extended priors' table (dz_prior_ext.h), or the first dimension that is refused
static int prior_ext_rows(const int32_t* kind, const double* a, const double* b, const double* s1, const double* s2, int d, std::vector<dz::PriorExtRow>& rows)
{
    rows.assign((size_t)d, dz::PriorExtRow{0.0, 0.0, 0.0, 0.0, 0.0});
    for (int j = 0; j < d; ++j) {
        const bool shaped = kind[j] > 2;
        if (const char* why = dz::prior_ext_row(kind[j], a[j], b[j], shaped && s1 ? s1[j] : 0.0, shaped && s2 ? s2[j] : 0.0, rows[j]))
            return fail("dz_set_prior_ext: dimension " + std::to_string(j) + ": " + why);
    }
    return 0;
}

int dz_set_prior_ext(dz_engine* e, const int32_t* kind, const double* a, const double* b, const double* s1, const double* s2)
{
    HIPCK(hipSetDevice(e->c.device));
    const int d = e->p.d, ld = e->p.ld;
    std::vector<dz::PriorExtRow> rows;
    DZCK(prior_ext_rows(kind, a, b, s1, s2, d, rows));
    bool ext = false;
    for (int j = 0; j < d; ++j) ext = ext || kind[j] > 2;
    if (!ext) return dz_set_prior(e, kind, a, b);      // the same device constants, the same kernels, the same bits
    if (!e->d_xkind) { DZCK(ealloc(e, &e->d_xkind, (size_t)ld)); DZCK(ealloc(e, &e->d_xtab, (size_t)5 * ld)); }
    std::vector<int32_t> hk((size_t)ld, 0);
    std::vector<double> tab((size_t)5 * ld, 0.0);
    for (int j = 0; j < d; ++j) {
        hk[j] = kind[j];
        tab[j] = rows[j].a; tab[(size_t)ld + j] = rows[j].rb; tab[(size_t)2 * ld + j] = rows[j].c; tab[(size_t)3 * ld + j] = rows[j].p1; tab[(size_t)4 * ld + j] = rows[j].p2;
    }
    DZCK(sync_all(e));
    HIPCK(hipMemcpy(e->d_xkind, hk.data(), sizeof(int32_t) * ld, hipMemcpyHostToDevice));
    HIPCK(hipMemcpy(e->d_xtab, tab.data(), sizeof(double) * tab.size(), hipMemcpyHostToDevice));
    e->xt = dz::PriorExtTable{e->d_xkind, e->d_xtab, e->d_xtab + ld, e->d_xtab + (size_t)2 * ld, e->d_xtab + (size_t)3 * ld, e->d_xtab + (size_t)4 * ld};
    // the built-in kernels run without a prior of their own (they write a zero prior); k_prior_ext adds every dimension's
    e->p.have_prior = 0; e->p.prior_nonormal = 1;
    e->h_pkind.assign(kind, kind + d); e->h_pa.assign(a, a + d); e->h_pb.assign(b, b + d);
    e->h_ps1.assign((size_t)d, 0.0); e->h_ps2.assign((size_t)d, 0.0);
    for (int j = 0; j < d; ++j) { if (s1) e->h_ps1[j] = s1[j]; if (s2) e->h_ps2[j] = s2[j]; }
    e->prior_ext = true;
    return 0;
}

int dz_prior_ext_host(const int32_t* kind, const double* a, const double* b, const double* s1, const double* s2, int32_t d, const double* X, int64_t n, double* out)
{
    if (d < 1 || n < 0) return fail("dz_prior_ext_host: d >= 1 and n >= 0");
    std::vector<dz::PriorExtRow> rows;
    DZCK(prior_ext_rows(kind, a, b, s1, s2, d, rows));
    for (int64_t i = 0; i < n; ++i) out[i] = dz::prior_ext_point_host(kind, rows.data(), d, X + (size_t)i * d);
    return 0;
}

int dz_set_likelihood_mvn(dz_engine* e, const double* mu, const double* M, int32_t kind, double log_F)
{
    HIPCK(hipSetDevice(e->c.device));
    const int d = e->p.d, ld = e->p.ld;
    if (!e->d_mu) DZCK(ealloc(e, &e->d_mu, (size_t)32 * ld));
    if (!e->d_Mt) DZCK(ealloc(e, &e->d_Mt, (size_t)ld * ld));
    std::vector<double> mt((size_t)ld * ld, 0.0), m(ld, 0.0);
    for (int r = 0; r < d; ++r) for (int c = 0; c < d; ++c) mt[(size_t)c * ld + r] = M[(size_t)r * d + c];
    memcpy(m.data(), mu, sizeof(double) * d);
    HIPCK(hipMemcpy(e->d_Mt, mt.data(), sizeof(double) * mt.size(), hipMemcpyHostToDevice));
    HIPCK(hipMemcpy(e->d_mu, m.data(), sizeof(double) * ld, hipMemcpyHostToDevice));
    e->p.mu = e->d_mu; e->p.Mt = e->d_Mt; e->p.logF = log_F; e->p.tri = kind != 0; e->lk = LK_MVN;
    e->p.Mtp = nullptr; e->p.mtp_len = 0;
    e->p.mu_zero = 1;
    for (int j = 0; j < d; ++j) if (!(mu[j] == 0.0) || std::signbit(mu[j])) e->p.mu_zero = 0;
    if (kind != 0 && ld <= 256) {   // packed triangle for k_logp_mvn_lds and the persistent kernels (dz_kernels.h tri_row_offset); 128 < ld <= 256: k_generations_d2 reads it from L2
        const int rows = 4 * ((d + 3) / 4);
        std::vector<double> pk((size_t)dz::tri_row_offset(rows), 0.0);
        for (int r = 0; r < rows; ++r)
            for (int c = 0; c < 16 * (r / 16 + 1); ++c) pk[(size_t)dz::tri_row_offset(r) + c] = mt[(size_t)r * ld + c];
        if (!e->d_Mtp) DZCK(ealloc(e, &e->d_Mtp, (size_t)dz::tri_row_offset(256)));
        HIPCK(hipMemcpy(e->d_Mtp, pk.data(), sizeof(double) * pk.size(), hipMemcpyHostToDevice));
        e->p.Mtp = e->d_Mtp; e->p.mtp_len = (int)pk.size();
    }
    return 0;
}

int dz_set_likelihood_mixture(dz_engine* e, int32_t J, const double* mu, const double* log_F)
{
    HIPCK(hipSetDevice(e->c.device));
    if (J < 1 || J > 32) return fail("mixture components must be 1..32");
    const int d = e->p.d, ld = e->p.ld;
    if (!e->d_mu) DZCK(ealloc(e, &e->d_mu, (size_t)32 * ld));
    if (!e->d_mixF) DZCK(ealloc(e, &e->d_mixF, 32));
    std::vector<double> m((size_t)J * ld, 0.0);
    for (int j = 0; j < J; ++j) memcpy(&m[(size_t)j * ld], mu + (size_t)j * d, sizeof(double) * d);
    HIPCK(hipMemcpy(e->d_mu, m.data(), sizeof(double) * m.size(), hipMemcpyHostToDevice));
    HIPCK(hipMemcpy(e->d_mixF, log_F, sizeof(double) * J, hipMemcpyHostToDevice));
    e->p.mu = e->d_mu; e->p.mixF = e->d_mixF; e->p.J = J; e->lk = LK_MIX;
    return 0;
}

int dz_set_likelihood_host(dz_engine* e, dz_logp_cb cb, void* user)
{
    if (!cb) return fail("null callback");
    e->cb = cb; e->cb_user = user; e->lk = LK_HOST;
    return 0;
}

// A user's code object, one kernel of it and its data block on the device: all three or, on failure, none (the engine's module, function and data change
// together, and only once every step has succeeded -- a failure leaves the engine as it was: advisor, round 5).  `who`: the caller's name in the messages.
static int load_user_module(dz_engine* e, const char* who, const char* code_object_path, const char* kernel_name, const void* data, int64_t data_bytes, hipModule_t* mod, hipFunction_t* fn, void** d_data)
{
    HIPCK(hipSetDevice(e->c.device));
    DZCK(sync_all(e));
    hipError_t err = hipModuleLoad(mod, code_object_path);
    if (err != hipSuccess) { (void)hipGetLastError(); return fail(std::string("hipModuleLoad(") + code_object_path + "): " + hipGetErrorString(err) + " (a gfx950 code object is expected: hipcc --offload-arch=gfx950 --genco)"); }
    err = hipModuleGetFunction(fn, *mod, kernel_name);
    if (err != hipSuccess) { (void)hipGetLastError(); (void)hipModuleUnload(*mod); return fail(std::string("hipModuleGetFunction(") + kernel_name + "): " + hipGetErrorString(err) + " (the kernel must be extern \"C\")"); }
    *d_data = nullptr;
    if (data_bytes > 0) {
        hipError_t me = hipMalloc(d_data, (size_t)data_bytes);
        if (me == hipSuccess) me = hipMemcpy(*d_data, data, (size_t)data_bytes, hipMemcpyHostToDevice);
        if (me != hipSuccess) {
            (void)hipGetLastError();
            if (*d_data) (void)hipFree(*d_data);
            (void)hipModuleUnload(*mod);
            return fail(std::string(who) + ": data block: " + hipGetErrorString(me));
        }
    }
    return 0;
}

int dz_set_likelihood_module(dz_engine* e, const char* code_object_path, const char* kernel_name, int32_t lanes_per_point, int32_t flags,
                             const void* data, int64_t data_bytes)
{
    if (!e || !code_object_path || !kernel_name) return fail("null argument");
    if (lanes_per_point != 1 && lanes_per_point != 16 && lanes_per_point != 32 && lanes_per_point != 64)
        return fail("dz_set_likelihood_module: lanes_per_point must be 1 (a thread per point), 16 or 32 (a lane group per point) or 64 (a wave per point)");
    if (data_bytes < 0 || (data_bytes > 0 && !data)) return fail("dz_set_likelihood_module: bad data block");
    hipModule_t mod = nullptr; hipFunction_t fn = nullptr; void* d_new = nullptr;
    DZCK(load_user_module(e, "dz_set_likelihood_module", code_object_path, kernel_name, data, data_bytes, &mod, &fn, &d_new));
    hipFunction_t gen[4] = {nullptr, nullptr, nullptr, nullptr};      // optional: the persistent kernels around the same density (a code object built by DeviceFunctionLogLike has them)
    const char* gen_name[4] = {"dz_user_generations_v" DZ_USER_STR(DZ_USER_ABI), "dz_user_generations_full_v" DZ_USER_STR(DZ_USER_ABI), "dz_user_generations_wide_v" DZ_USER_STR(DZ_USER_ABI),
                               "dz_user_generations_wide_full_v" DZ_USER_STR(DZ_USER_ABI)};
    for (int i = 0; i < 4; ++i) if (!e->mega_user || hipModuleGetFunction(&gen[i], mod, gen_name[i]) != hipSuccess) { (void)hipGetLastError(); gen[i] = nullptr; }
    if (e->lk_module) { (void)hipModuleUnload(e->lk_module); e->lk_module = nullptr; e->lk_fn = nullptr; }
    if (e->d_lk_data) { (void)hipFree(e->d_lk_data); e->d_lk_data = nullptr; }
    e->d_lk_data = d_new;
    for (int i = 0; i < 4; ++i) e->lk_gen_fn[i] = gen[i];
    e->p.udata = d_new; e->p.J = 1;      // (J: the wave's scratch row in the persistent kernel's layout)
    e->lk_module = mod; e->lk_fn = fn; e->lk_lanes = lanes_per_point; e->lk_finite = (flags & DZ_LIKE_ALWAYS_FINITE) != 0;
    e->lk = LK_MODULE; e->have_logp = false;
    e->lk_items = 1;
    return 0;
}

int dz_set_likelihood_items(dz_engine* e, int32_t items_per_point)
{
    if (!e) return fail("null argument");
    if (e->lk != LK_MODULE) return fail("dz_set_likelihood_items: call dz_set_likelihood_module first (the items are those of its kernel)");
    if (items_per_point < 1 || items_per_point > DZ_MAX_LIKELIHOOD_ITEMS)
        return fail("dz_set_likelihood_items: items_per_point must be 1.." DZ_USER_STR(DZ_MAX_LIKELIHOOD_ITEMS) " (got " + std::to_string(items_per_point) + ")");
    e->lk_items = items_per_point; e->have_logp = false;
    return 0;
}

int dz_set_output_module(dz_engine* e, const char* code_object_path, const char* kernel_name, int32_t lanes_per_point, int32_t items_per_point,
                         int64_t doubles_per_item, const void* data, int64_t data_bytes)
{
    if (!e || !code_object_path || !kernel_name) return fail("null argument");
    if (lanes_per_point != 1 && lanes_per_point != 16 && lanes_per_point != 32 && lanes_per_point != 64)
        return fail("dz_set_output_module: lanes_per_point must be 1 (a thread per item), 16 or 32 (a lane group per item) or 64 (a wave per item) (got " + std::to_string(lanes_per_point) + ")");
    if (items_per_point < 1 || items_per_point > DZ_MAX_LIKELIHOOD_ITEMS)
        return fail("dz_set_output_module: items_per_point must be 1.." DZ_USER_STR(DZ_MAX_LIKELIHOOD_ITEMS) " (got " + std::to_string(items_per_point) + ")");
    if (doubles_per_item < 1) return fail("dz_set_output_module: doubles_per_item must be >= 1 (got " + std::to_string(doubles_per_item) + ")");
    if (data_bytes < 0 || (data_bytes > 0 && !data)) return fail("dz_set_output_module: bad data block");
    hipModule_t mod = nullptr; hipFunction_t fn = nullptr; void* d_new = nullptr;
    DZCK(load_user_module(e, "dz_set_output_module", code_object_path, kernel_name, data, data_bytes, &mod, &fn, &d_new));
    if (e->out_module) (void)hipModuleUnload(e->out_module);
    if (e->d_out_data) (void)hipFree(e->d_out_data);
    e->d_out_data = d_new;
    e->out_module = mod; e->out_fn = fn; e->out_lanes = lanes_per_point; e->out_items = items_per_point; e->out_doubles = doubles_per_item;
    return 0;
}

const char* dz_comm_library(void)
{   // path of the librccl the engine uses (loads it if necessary); NULL with dz_last_error set if it cannot be loaded
    if (g_rccl.load()) return nullptr;
    return g_rccl.path.c_str();
}

const char* dz_hip_library(void)
{   // path of the HIP runtime this library's calls are bound to (in a process that imported PyTorch first that is torch's copy)
    static std::string path;
    Dl_info hi;
    if (!dladdr((void*)&hipGetDeviceCount, &hi) || !hi.dli_fname) { fail("cannot locate the HIP runtime"); return nullptr; }
    path = hi.dli_fname;
    return path.c_str();
}

int dz_comm_unique_id(void* id128)
{
    DZCK(g_rccl.load());
    ncclUniqueId id;
    if (g_rccl.GetUniqueId(&id) != ncclSuccess) return fail("ncclGetUniqueId failed");
    static_assert(sizeof(ncclUniqueId) == 128, "unexpected ncclUniqueId size");
    memcpy(id128, &id, 128);
    return 0;
}

int dz_comm_init_rccl(dz_engine* e, int32_t rank, int32_t world, const void* id128)
{
    HIPCK(hipSetDevice(e->c.device));
    if (world != e->world || rank != e->rank) return fail("rank/world do not match the chain shard in dz_config");
    DZCK(g_rccl.load());
    ncclUniqueId id;
    memcpy(&id, id128, 128);
    ncclResult_t r = g_rccl.CommInitRank(&e->comm, world, id, rank);
    if (r != ncclSuccess) return fail(std::string("ncclCommInitRank: ") + (g_rccl.GetErrorString ? g_rccl.GetErrorString(r) : "error"));
    return 0;
}

int dz_comm_count(dz_engine* e, int32_t* ranks)
{   // ncclCommCount of the engine's communicator: how many ranks RCCL itself says take part (0: no communicator)
    if (!e || !ranks) return fail("null argument");
    *ranks = 0;
    if (!e->comm) return 0;
    if (!g_rccl.CommCount) return fail("librccl has no ncclCommCount");
    int n = 0;
    ncclResult_t r = g_rccl.CommCount(e->comm, &n);
    if (r != ncclSuccess) return fail(std::string("ncclCommCount: ") + (g_rccl.GetErrorString ? g_rccl.GetErrorString(r) : "error"));
    *ranks = n;
    return 0;
}

int dz_set_exchange(dz_engine* e, dz_exchange_cb cb, void* user) { e->xcb = cb; e->xcb_user = user; return 0; }

// ---- peer transport: rows pushed by the copy engines into the other ranks' buffers, mapped through HIP IPC ----
namespace {
struct PeerBlob {          // what a rank publishes about itself (DZ_PEER_BLOB_BYTES)
    uint32_t magic, nchains, nchains_local, ld; int64_t capacity; int32_t has_cp, rank;
    hipIpcMemHandle_t z, flags, cp[3], gs[2];      // (has_cp: 1 = position buffers, 3 = ... and the group-sum records of the sharded burn-in)
};
static_assert(sizeof(PeerBlob) <= DZ_PEER_BLOB_BYTES, "PeerBlob does not fit DZ_PEER_BLOB_BYTES");
}  // namespace

int dz_peer_export(dz_engine* e, void* blob)
{
    HIPCK(hipSetDevice(e->c.device));
    if (e->world < 2) return fail("dz_peer_export: the engine is not sharded");
    if (e->world > 64) return fail("dz_peer_export: more than 64 ranks (the gate kernel polls one flag word per lane)");
    if (!e->d_flags) {
        // The flag words are written by OTHER GPUs' copy engines while a kernel of this GPU polls them: ordinary (coarse-grained) device
        // memory may sit in this GPU's L2, which a write arriving over the fabric does not update -- the poll would spin on its own cached
        // copy.  Uncached device memory (what RCCL uses for its peer-to-peer flags) is read from memory by every system-scope load.
        {
            void* q = nullptr;
            if (hipExtMallocWithFlags(&q, sizeof(unsigned long long) * XK_KINDS * (size_t)e->world, hipDeviceMallocUncached) != hipSuccess) {
                (void)hipGetLastError();
                return fail("hipExtMallocWithFlags(hipDeviceMallocUncached) for the peer flags failed");
            }
            HIPCK(hipMemset(q, 0, sizeof(unsigned long long) * XK_KINDS * (size_t)e->world));
            HIPCK(hipStreamSynchronize(nullptr));
            e->d_flags = (unsigned long long*)q; e->to_free.push_back(q);
        }
        // one flag push per history append and per published generation: bounded by the archive's capacity and the burn-in
        e->seq_cap = (e->c.history_capacity / std::max(1, e->p.N)) + (int64_t)e->c.crossover_burnin + 65536;      // (+ rendezvous numbers: dz_comm_barrier)
        if (e->seq_cap > ((int64_t)1 << 24)) e->seq_cap = (int64_t)1 << 24;
        DZCK(ealloc(e, &e->d_seq, (size_t)e->seq_cap));
        std::vector<unsigned long long> h((size_t)e->seq_cap);
        for (size_t i = 0; i < h.size(); ++i) h[i] = i;
        HIPCK(hipMemcpy(e->d_seq, h.data(), sizeof(unsigned long long) * h.size(), hipMemcpyHostToDevice));
        HIPCK(hipHostMalloc((void**)&e->h_gate, 8 * sizeof(unsigned long long), hipHostMallocMapped));
        memset(e->h_gate, 0, 8 * sizeof(unsigned long long));
    }
    PeerBlob b; memset(&b, 0, sizeof b);
    b.magic = 0x445a5058u; b.nchains = (uint32_t)e->p.N; b.nchains_local = (uint32_t)e->p.nl; b.ld = (uint32_t)e->p.ld; b.capacity = e->c.history_capacity;
    b.has_cp = e->adapt ? (e->adapt_groups ? 3 : 1) : 0; b.rank = e->rank;
    HIPCK(hipIpcGetMemHandle(&b.z, e->p.Z));
    HIPCK(hipIpcGetMemHandle(&b.flags, e->d_flags));
    if (e->adapt) for (int i = 0; i < 3; ++i) HIPCK(hipIpcGetMemHandle(&b.cp[i], e->d_cp[i]));
    if (e->adapt_groups) for (int i = 0; i < 2; ++i) HIPCK(hipIpcGetMemHandle(&b.gs[i], e->d_GS[i]));
    memset(blob, 0, DZ_PEER_BLOB_BYTES);
    memcpy(blob, &b, sizeof b);
    return 0;
}

int dz_peer_attach(dz_engine* e, int32_t rank, int32_t world, const void* blobs)
{
    HIPCK(hipSetDevice(e->c.device));
    if (world != e->world || rank != e->rank) return fail("rank/world do not match the chain shard in dz_config");
    if (!e->d_flags) return fail("dz_peer_attach: call dz_peer_export first");
    if (e->peer_on) return fail("dz_peer_attach: already attached");
    e->peers.assign((size_t)world, dz_engine::Peer());
    for (int r = 0; r < world; ++r) {
        if (r == rank) continue;
        PeerBlob b; memcpy(&b, (const char*)blobs + (size_t)r * DZ_PEER_BLOB_BYTES, sizeof b);
        if (b.magic != 0x445a5058u || b.rank != r) return fail("dz_peer_attach: blob " + std::to_string(r) + " is not rank " + std::to_string(r) + "'s export");
        if ((int)b.nchains != e->p.N || (int)b.nchains_local != e->p.nl || (int)b.ld != e->p.ld || b.capacity != e->c.history_capacity || b.has_cp != (e->adapt ? (e->adapt_groups ? 3 : 1) : 0))
            return fail("dz_peer_attach: rank " + std::to_string(r) + " was created with a different configuration");
        dz_engine::Peer& pr = e->peers[r];
        HIPCK(hipIpcOpenMemHandle((void**)&pr.Z, b.z, hipIpcMemLazyEnablePeerAccess));
        HIPCK(hipIpcOpenMemHandle((void**)&pr.flags, b.flags, hipIpcMemLazyEnablePeerAccess));
        if (e->adapt) for (int i = 0; i < 3; ++i) HIPCK(hipIpcOpenMemHandle((void**)&pr.cp[i], b.cp[i], hipIpcMemLazyEnablePeerAccess));
        if (e->adapt_groups) for (int i = 0; i < 2; ++i) HIPCK(hipIpcOpenMemHandle((void**)&pr.gs[i], b.gs[i], hipIpcMemLazyEnablePeerAccess));
        HIPCK(hipStreamCreateWithFlags(&pr.st, hipStreamNonBlocking));
    }
    for (int i = 0; i < 8; ++i) HIPCK(hipEventCreateWithFlags(&e->push_ev[i], hipEventDisableTiming));
    e->peer_on = true;
    // Self-test before anything depends on it: every rank pushes one flag word into every peer and waits for theirs (a mapping that
    // cannot be written, a write this GPU's poll does not see: better a refusal here -- the caller then falls back to another
    // transport -- than a timeout in the middle of a run).
    {
        const double t_self = getenv("DZ_PEER_SELFTEST_S") ? std::max(0.5, atof(getenv("DZ_PEER_SELFTEST_S"))) : 30.0;
        int rc = peer_push(e, XK_HELLO, nullptr, 0, 0, 1ull);
        if (!rc) rc = peer_gate(e, XK_HELLO, 1ull, t_self);
        if (!rc && hipStreamSynchronize(e->stream) != hipSuccess) rc = fail("peer self-test: stream error");
        if (!rc) for (int r = 0; r < world; ++r) if (r != rank && hipStreamSynchronize(e->peers[r].st) != hipSuccess) rc = fail("peer self-test: copy stream error");
        if (!rc) rc = peer_check(e);
        if (rc) {
            const std::string why = g_err;
            e->peer_on = false; e->h_gate[2] = 0; e->h_gate[6] = 0;
            return fail("peer transport self-test failed: " + why);
        }
    }
    return 0;
}

int dz_peer_detach(dz_engine* e)
{   // stop using the peer transport (another rank could not attach: every rank moves on to the same fallback); the mappings stay until dz_destroy
    HIPCK(hipSetDevice(e->c.device));
    DZCK(sync_all(e));
    for (auto& pr : e->peers) if (pr.st) HIPCK(hipStreamSynchronize(pr.st));
    e->peer_on = false;
    return 0;
}

int dz_exchange_stats(dz_engine* e, int64_t* exchanges, int64_t* gates, double* gate_wait_us)
{   // (k_peer_gate's counters; call after dz_sync)
    if (exchanges) *exchanges = e->z_pushed + e->pos_pushed + e->gs_pushed;
    if (gates) *gates = e->h_gate ? (int64_t)e->h_gate[1] : 0;
    if (gate_wait_us) *gate_wait_us = e->h_gate ? (double)e->h_gate[0] * 0.01 : 0.0;      // 100 MHz ticks
    return 0;
}

int dz_exchange_bytes(dz_engine* e, int64_t* history_bytes, int64_t* position_bytes, int64_t* sums_bytes)
{   // bytes this rank has handed to the transport FOR EACH other rank so far, by what they were
    if (!e) return fail("null engine");
    if (history_bytes) *history_bytes = e->bytes_z;
    if (position_bytes) *position_bytes = e->bytes_pos;
    if (sums_bytes) *sums_bytes = e->bytes_sums;
    return 0;
}

// A rendezvous of the ranks on the device: a one-element all-gather on the engine's stream, then a stream synchronise.  Ranks leave
// an RCCL collective within microseconds of each other (a host barrier's exits are spread by tens of microseconds), which is what a
// timed region over a few hundred microseconds wants in front of it.  No communicator (one GPU, or the host transport): just the sync.
int dz_comm_barrier(dz_engine* e)
{
    HIPCK(hipSetDevice(e->c.device));
    DZCK(sync_all(e));
    if (e->peer_on) {   // peer transport: every rank pushes its next "hello" number to every peer and waits for theirs
        e->hello_seq++;
        DZCK(peer_push(e, XK_HELLO, nullptr, 0, 0, (unsigned long long)e->hello_seq));
        DZCK(peer_gate(e, XK_HELLO, (unsigned long long)e->hello_seq));
        HIPCK(hipStreamSynchronize(e->stream));
        return peer_check(e);
    }
    if (!e->comm) return 0;
    if (!e->d_bar) DZCK(ealloc(e, &e->d_bar, (size_t)std::max(1, e->world)));
    ncclResult_t r = g_rccl.AllGather(e->d_bar + e->rank, e->d_bar, 1, ncclDouble, e->comm, e->stream);
    if (r != ncclSuccess) return fail(std::string("ncclAllGather: ") + (g_rccl.GetErrorString ? g_rccl.GetErrorString(r) : "error"));
    HIPCK(hipStreamSynchronize(e->stream));
    return 0;
}

int dz_set_temperatures(dz_engine* e, const double* T, int32_t swaps)
{   // core.py:133-136 (the ladder is the host's), :185-221 (swaps != 0: one swap attempt per generation)
    HIPCK(hipSetDevice(e->c.device));
    if (swaps && e->world > 1) return fail("temperature swaps need all chains on one GPU");
    if (swaps && e->c.adapt_lag > 0) return fail("temperature swaps are not available with adapt_lag > 0");
    DZCK(sync_all(e));
    if (!e->d_Tc) DZCK(ealloc(e, &e->d_Tc, (size_t)e->p.N));
    HIPCK(hipMemcpy(e->d_Tc, T, sizeof(double) * e->p.N, hipMemcpyHostToDevice));
    e->p.Tc = e->d_Tc;
    e->tempering = swaps != 0;
    if (e->tempering && !e->d_tswap) { DZCK(ealloc(e, &e->d_tswap, (size_t)3 * std::max<int64_t>(1, e->c.trace_capacity))); e->p.tswap = e->d_tswap; }
    e->carry.draws_gen = -1;
    return 0;
}
int dz_get_swaps(dz_engine* e, int64_t g0, int64_t ng, int32_t* out)
{
    HIPCK(hipSetDevice(e->c.device));
    if (!e->d_tswap || g0 < 0 || ng < 0 || g0 + ng > e->ntrace) return fail("swap log range");
    DZCK(sync_all(e));
    HIPCK(hipMemcpy(out, e->d_tswap + 3 * g0, sizeof(int32_t) * 3 * (size_t)ng, hipMemcpyDeviceToHost));
    return 0;
}

// A new run on the live engine, as run_dream(restart=True) starts one from the files the previous run left (core.py:46-62, 255-263;
// Dream.py:128-147): the archive as it stands is the new run's seed history (it is what the history file holds), the crossover /
// gamma-level probabilities stay (the two probability files), their accumulators start from zero (core.py:287-293), the generation
// counter restarts (Dream.iter = 0: generation 0 appends, the crossover burn-in runs again), the random contract takes the new key.
// Chain states come from dz_set_state afterwards.  Nothing is uploaded: a grown archive is copied device to device.
int dz_continue_run(dz_engine* e, int64_t history_capacity, int64_t trace_capacity, uint64_t seed, int32_t crossover_burnin)
{
    if (!e) return fail("null engine");
    HIPCK(hipSetDevice(e->c.device));
    if (e->peer_on || e->comm || e->world > 1) return fail("dz_continue_run: not on a sharded engine");
    if (e->tempering || e->p.Tc) return fail("dz_continue_run: not on a tempering engine");
    DZCK(adapt_flush(e));           // (the probabilities the new run starts from: everything that was due is in)
    DZCK(sync_all(e));
    if (e->copy_stream) HIPCK(hipStreamSynchronize(e->copy_stream));
    dz::Params& p = e->p;
    if (history_capacity < e->M) return fail("dz_continue_run: capacity below the rows already in the archive");
    // keep == 0 (the trace buffers: nothing of the old run's trace is used again): the old buffer is freed BEFORE the new one is allocated,
    // so the peak is max(old, new), not old + new (advisor, round 4); a failed allocation leaves the slot null and the engine says so
    auto swap_buffer = [&](auto** slot, size_t count, size_t keep) -> int {
        using T = std::remove_pointer_t<std::remove_pointer_t<decltype(slot)>>;
        auto drop_old = [&]() {
            auto it = std::find(e->to_free.begin(), e->to_free.end(), (void*)*slot);
            if (it != e->to_free.end()) e->to_free.erase(it);
            (void)hipFree((void*)*slot);
            *slot = nullptr;
        };
        if (!keep) drop_old();
        T* fresh = nullptr;
        if (dalloc(&fresh, count)) {
            if (!keep) { e->c.trace_capacity = 0; e->p.tcap = 0; e->broken = "dz_continue_run could not allocate the new trace buffers; the engine has none now: destroy it"; }
            return -1;
        }
        if (keep && hipMemcpy(fresh, *slot, sizeof(T) * keep, hipMemcpyDeviceToDevice) != hipSuccess) { (void)hipFree(fresh); return fail("dz_continue_run: device copy failed"); }
        if (keep) drop_old();
        *slot = fresh; e->to_free.push_back((void*)fresh);
        return 0;
    };
    if (history_capacity > e->c.history_capacity) {
        DZCK(swap_buffer(&p.Z, (size_t)history_capacity * p.ld, (size_t)e->M * p.ld));
        e->c.history_capacity = history_capacity;
    }
    if (trace_capacity > e->c.trace_capacity) {
        const size_t tc = (size_t)trace_capacity, nl = (size_t)p.nl;
        if (!e->c.trace_capacity) {
            DZCK(ealloc(e, &p.tX, tc * nl * p.ld)); DZCK(ealloc(e, &p.tlogp, tc * nl)); DZCK(ealloc(e, &p.tmoved, tc * nl));
            DZCK(ealloc(e, &p.tsnk, tc * nl)); DZCK(ealloc(e, &p.ttry, tc * nl)); DZCK(ealloc(e, &p.tcr, tc * nl));
        } else {
            DZCK(swap_buffer(&p.tX, tc * nl * p.ld, 0)); DZCK(swap_buffer(&p.tlogp, tc * nl, 0)); DZCK(swap_buffer(&p.tmoved, tc * nl, 0));
            DZCK(swap_buffer(&p.tsnk, tc * nl, 0)); DZCK(swap_buffer(&p.ttry, tc * nl, 0)); DZCK(swap_buffer(&p.tcr, tc * nl, 0));
        }
        p.tcap = (long long)tc; e->c.trace_capacity = trace_capacity;
    }
    e->c.seed = seed; p.k0 = (uint32_t)seed; p.k1 = (uint32_t)(seed >> 32);
    e->c.crossover_burnin = crossover_burnin; p.burnin = crossover_burnin;
    // delta_m / ncr_updates and the gamma analogue start from zero; the probabilities stay (layout: cr_probs|cr_delta|cr_n|g_probs|g_delta|g_n)
    HIPCK(hipMemset(p.cr_delta, 0, sizeof(double) * 2 * (size_t)p.ncr));
    HIPCK(hipMemset(p.g_delta, 0, sizeof(double) * 2 * (size_t)p.ngamma));
    if (e->d_redraw_count) HIPCK(hipMemset(e->d_redraw_count, 0, sizeof(unsigned long long)));
    HIPCK(hipStreamSynchronize(nullptr));
    e->gen = 0; std::fill(e->gen_c.begin(), e->gen_c.end(), (int64_t)0);
    e->napp = 0; e->ntrace = 0; e->carry = dz::MultiCarry();
    e->have_logp = false; e->redraw_rounds = 0;
    e->ad_applied = -1; e->ad_made = -1;
    std::fill(e->own_init.begin(), e->own_init.end(), 0);
    if (e->adapt) { p.cp_prev = e->d_cp[0]; p.cp_new = e->d_cp[1]; e->cp_idx = 1; }
    e->params_uploaded = false;
    return 0;
}

int dz_step(dz_engine* e, int64_t generations)
{
    if (!e) return fail("null engine");
    HIPCK(hipSetDevice(e->c.device));
    if (!e->broken.empty()) return fail(e->broken);
    if (e->lk == LK_NONE) return fail("no likelihood set");
    if (e->M < 2 * e->c.depairs) return fail("history not seeded");
    if (e->c.trace_capacity && e->ntrace + generations > e->c.trace_capacity) return fail("trace capacity exceeded");
    e->multi = multi_shape(e);      // (nothing either selection reads changes inside a dz_step)
    if (!e->have_logp) {   // Dream.py:266-268
        DZCK(eval_logp(e, e->p.X, e->p.nl, e->p.lprior, e->p.llike));
        e->have_logp = true;
    }
    for (int c = 1; c < e->p.nl; ++c) if (e->gen_c[c] != e->gen_c[0]) return fail("chains are out of lockstep (single-chain stepping in progress)");
    e->gen = e->gen_c[0];
    e->p.own_cr = nullptr; e->p.own_g = nullptr;                   // lockstep generations read the shared probabilities;
    std::fill(e->own_init.begin(), e->own_init.end(), 0);          // a later single-chain step starts from them again
    const bool mega = mega_select(e);
    e->carry.stream_prop_gen = -1;
    for (int64_t i = 0; i < generations;) {
        DZCK(peer_check(e));            // a gate that gave up is fatal: nothing more is queued behind it
        const int n = mega ? mega_segment(e, (uint32_t)e->gen, generations - i) : 0;
        if (n > 0) { DZCK(run_mega_segment(e, (uint32_t)e->gen, n, i + n < generations && mega_segment(e, (uint32_t)e->gen + (uint32_t)n, 1) > 0)); i += n; }
        else { DZCK(one_generation(e, 0, e->p.nl, (uint32_t)e->gen, true, i + 1 < generations && !(mega && mega_segment(e, (uint32_t)e->gen + 1, 1) > 0))); i += 1; }
        if ((++e->ra_n % RA_STRIDE) == 0) {
            // keep the launch queue short: thousands of queued dispatches exhaust the runtime's kernarg/signal pools
            // and the whole pass then runs several times slower (measured; DESIGN.md "Host run-ahead")
            const int slot = (int)((e->ra_n / RA_STRIDE) & 3), oldest = (slot + 1) & 3;
            HIPCK(hipEventRecord(e->ra_ev[slot], e->lane_stream[0]));
            e->ra_used[slot] = true;
            if (e->ra_used[oldest]) HIPCK(hipEventSynchronize(e->ra_ev[oldest]));
        }
    }
    // (adapt_lag 0: adaptation totals are left pending only between two launches of this loop; adapt_lag >= 1: updates that are due stay pending
    //  until a launch or a getter needs the state -- adapt_flush in dz_get_cr_state & co. -- instead of a launch of their own behind every dz_step)
    return e->c.adapt_lag > 0 ? 0 : adapt_flush(e);
}

int dz_step_range(dz_engine* e, int32_t c0, int32_t nc)
{
    if (!e) return fail("null engine");
    HIPCK(hipSetDevice(e->c.device));
    if (c0 < 0 || nc < 1 || c0 + nc > e->p.nl) return fail("bad chain range");
    if (e->lk == LK_NONE) return fail("no likelihood set");
    if (e->M < 2 * e->c.depairs) return fail("history not seeded");
    e->multi = multi_shape(e);
    if (!e->have_logp) { DZCK(eval_logp(e, e->p.X, e->p.nl, e->p.lprior, e->p.llike)); e->have_logp = true; }
    for (int c = c0 + 1; c < c0 + nc; ++c) if (e->gen_c[c] != e->gen_c[c0]) return fail("chains of the range are at different generations");
    return one_generation(e, c0, nc, (uint32_t)e->gen_c[c0], false, false);
}

int dz_set_chain_state(dz_engine* e, int32_t c, const double* x, const double* prior, const double* like)
{
    HIPCK(hipSetDevice(e->c.device));
    if (c < 0 || c >= e->p.nl) return fail("bad chain index");
    e->multi = multi_shape(e);
    if (!e->have_logp) { DZCK(eval_logp(e, e->p.X, e->p.nl, e->p.lprior, e->p.llike)); e->have_logp = true; }
    DZCK(upload_padded(e, e->p.X + (size_t)c * e->p.ld, x, 1, 0.0));
    if (prior && like) {
        HIPCK(hipMemcpy(e->p.lprior + c, prior, sizeof(double), hipMemcpyHostToDevice));
        HIPCK(hipMemcpy(e->p.llike + c, like, sizeof(double), hipMemcpyHostToDevice));
    } else DZCK(eval_logp(e, e->p.X + (size_t)c * e->p.ld, 1, e->p.lprior + c, e->p.llike + c));   // Dream.py:266-268
    return 0;
}

int dz_get_chain_state(dz_engine* e, int32_t c, double* x, double* prior, double* like)
{
    HIPCK(hipSetDevice(e->c.device));
    if (c < 0 || c >= e->p.nl) return fail("bad chain index");
    if (x) DZCK(download_rows(e, x, e->p.X + (size_t)c * e->p.ld, 1));
    DZCK(sync_all(e));
    if (prior) HIPCK(hipMemcpy(prior, e->p.lprior + c, sizeof(double), hipMemcpyDeviceToHost));
    if (like) HIPCK(hipMemcpy(like, e->p.llike + c, sizeof(double), hipMemcpyDeviceToHost));
    return 0;
}

int dz_get_chain_probs(dz_engine* e, int32_t c, double* cr_probs, double* gamma_probs)
{   // Dream.CR_probabilities / Dream.gamma_probabilities of the instance that drives chain c (Dream.py:375, :383)
    HIPCK(hipSetDevice(e->c.device));
    if (c < 0 || c >= e->p.nl) return fail("bad chain index");
    DZCK(adapt_flush(e));
    DZCK(sync_all(e));
    const bool own = e->d_own_cr && c < (int)e->own_init.size() && e->own_init[c];
    if (cr_probs) HIPCK(hipMemcpy(cr_probs, own ? e->d_own_cr + (size_t)c * e->p.ncr : e->p.cr_probs, sizeof(double) * e->p.ncr, hipMemcpyDeviceToHost));
    if (gamma_probs) HIPCK(hipMemcpy(gamma_probs, own ? e->d_own_g + (size_t)c * e->p.ngamma : e->p.g_probs, sizeof(double) * e->p.ngamma, hipMemcpyDeviceToHost));
    return 0;
}

int dz_sync(dz_engine* e)
{
    HIPCK(hipSetDevice(e->c.device));
    DZCK(sync_all(e));
    return peer_check(e);
}
int dz_trace_reset(dz_engine* e) { e->ntrace = 0; return 0; }
int64_t dz_generation(dz_engine* e) { return e->gen; }
int64_t dz_redraw_rounds(dz_engine* e)
{   // launches of the multi-kernel path's redraw rounds + (block, round) pairs of the persistent kernel's
    unsigned long long dev = 0;
    if (e->d_redraw_count && hipSetDevice(e->c.device) == hipSuccess && sync_all(e) == 0)
        (void)hipMemcpy(&dev, e->d_redraw_count, sizeof dev, hipMemcpyDeviceToHost);
    return e->redraw_rounds + (int64_t)dev;
}
const char* dz_last_kernel_variant(dz_engine* e) { return e->last_variant.c_str(); }
int dz_last_kernel_tries(dz_engine* e) { return e->last_kc; }

int dz_get_state(dz_engine* e, double* X, double* prior, double* like)
{
    HIPCK(hipSetDevice(e->c.device));
    if (X) DZCK(download_rows(e, X, e->p.X, (size_t)e->p.nl));
    DZCK(sync_all(e));
    if (prior) HIPCK(hipMemcpy(prior, e->p.lprior, sizeof(double) * e->p.nl, hipMemcpyDeviceToHost));
    if (like) HIPCK(hipMemcpy(like, e->p.llike, sizeof(double) * e->p.nl, hipMemcpyDeviceToHost));
    return 0;
}

// device trace rows are chain-major [nl][tcap][ld]; X_out[c][i][:] = sample g0+i of chain c at X_out + (c*chain_stride + i)*d
static int download_trace_rows(dz_engine* e, double* X, int64_t g0, int64_t ng, int64_t chain_stride_rows)
{
    const size_t nl = e->p.nl, d = e->p.d, ld = e->p.ld, tcap = (size_t)e->p.tcap;
    DZCK(sync_all(e));
    if (ng == 0) return 0;
    // pinning the destination lets the DMA engines write it directly (several times the pageable rate); not fatal if refused
    const size_t span = sizeof(double) * d * ((nl - 1) * (size_t)chain_stride_rows + (size_t)ng);
    const bool pinned = span >= ((size_t)64 << 20) && hipHostRegister(X, span, hipHostRegisterDefault) == hipSuccess;
    if (!pinned) (void)hipGetLastError();
    int rc = 0;
    auto copy2d = [&](double* dst, size_t dpitch, const double* src, size_t spitch, size_t width, size_t height) {
        if (pinned) return hipMemcpy2DAsync(dst, dpitch, src, spitch, width, height, hipMemcpyDeviceToHost, e->stream);
        return d2h_2d(e, dst, dpitch, src, spitch, width, height) ? hipErrorUnknown : hipSuccess;
    };
    if ((size_t)ng == tcap && (size_t)chain_stride_rows == (size_t)ng) {
        // whole buffer: the chains' blocks are back to back on both sides -- one strided copy
        if (copy2d(X, sizeof(double) * d, e->p.tX, sizeof(double) * ld, sizeof(double) * d, nl * (size_t)ng) != hipSuccess) rc = -1;
    } else {
        for (size_t c = 0; c < nl && !rc; ++c)
            if (copy2d(X + c * (size_t)chain_stride_rows * d, sizeof(double) * d, e->p.tX + (c * tcap + (size_t)g0) * ld, sizeof(double) * ld,
                       sizeof(double) * d, (size_t)ng) != hipSuccess) rc = -1;
    }
    if (hipStreamSynchronize(e->stream) != hipSuccess) rc = -1;
    if (pinned) (void)hipHostUnregister(X);
    return rc ? fail(std::string("trace download: ") + hipGetErrorString(hipGetLastError())) : 0;
}

int dz_get_trace(dz_engine* e, int64_t g0, int64_t ng, double* X, double* logp, uint8_t* moved, int32_t* try_idx, int32_t* cr_idx, uint8_t* snooker)
{
    HIPCK(hipSetDevice(e->c.device));
    if (g0 < 0 || ng < 0 || g0 + ng > e->ntrace) return fail("trace range");
    const size_t nl = e->p.nl, o = (size_t)g0 * nl, n = (size_t)ng * nl;
    if (X && ng > 0) {   // generation-major output [ng][nl][d]: one strided copy per chain (rows nl*d apart on the host side)
        const size_t d = e->p.d, ld = e->p.ld, tcap = (size_t)e->p.tcap;
        DZCK(sync_all(e));
        for (size_t c = 0; c < nl; ++c)
            DZCK(d2h_2d(e, X + c * d, sizeof(double) * nl * d, e->p.tX + (c * tcap + (size_t)g0) * ld, sizeof(double) * ld, sizeof(double) * d, (size_t)ng));
    }
    DZCK(sync_all(e));
    if (logp) HIPCK(hipMemcpy(logp, e->p.tlogp + o, sizeof(double) * n, hipMemcpyDeviceToHost));
    if (moved) HIPCK(hipMemcpy(moved, e->p.tmoved + o, n, hipMemcpyDeviceToHost));
    if (try_idx) HIPCK(hipMemcpy(try_idx, e->p.ttry + o, sizeof(int32_t) * n, hipMemcpyDeviceToHost));
    if (cr_idx) HIPCK(hipMemcpy(cr_idx, e->p.tcr + o, sizeof(int32_t) * n, hipMemcpyDeviceToHost));
    if (snooker) HIPCK(hipMemcpy(snooker, e->p.tsnk + o, n, hipMemcpyDeviceToHost));
    return 0;
}

int dz_get_trace_chains(dz_engine* e, int64_t g0, int64_t ng, double* X, int64_t chain_stride_rows, double* logp)
{
    HIPCK(hipSetDevice(e->c.device));
    if (g0 < 0 || ng < 0 || g0 + ng > e->ntrace) return fail("trace range");
    if (chain_stride_rows < ng) return fail("bad destination");
    if (X) DZCK(download_trace_rows(e, X, g0, ng, chain_stride_rows));
    if (logp && ng > 0) {   // log_ps chain by chain: transposed on the device, then one strided copy
        const size_t nl = e->p.nl, need = nl * (size_t)ng;
        if (need > e->qpart_len) {
            DZCK(sync_all(e));
            if (e->d_qpart) (void)hipFree(e->d_qpart);
            e->d_qpart = nullptr; e->qpart_len = 0;
            DZCK(dalloc(&e->d_qpart, need));
            e->qpart_len = need;
        }
        hipLaunchKernelGGL(dz::k_transpose_logp, dim3((unsigned)((need + 255) / 256)), dim3(256), 0, e->stream, (const double*)e->p.tlogp, (int)nl, g0, (int)ng, e->d_qpart);
        DZCK(launch_check("k_transpose_logp"));
        DZCK(d2h_2d(e, logp, sizeof(double) * (size_t)chain_stride_rows, e->d_qpart, sizeof(double) * (size_t)ng, sizeof(double) * (size_t)ng, nl));
    }
    return 0;
}

// Samples [g0, g0+ng) of every local chain into X (as dz_get_trace_chains) WITHOUT stopping the engine: the copy is queued on a
// stream of its own behind everything queued so far on the engine's streams and the call returns; generations stepped afterwards
// run while the DMA engines move the rows.  X must be page-locked (dz_host_register) -- a copy into pageable memory would block --
// and stay untouched until dz_trace_download_wait.  One 3-D copy (row = d of ld doubles, rows = generations, slices = chains).
int dz_trace_download_begin(dz_engine* e, int64_t g0, int64_t ng, double* X, int64_t chain_stride_rows)
{
    HIPCK(hipSetDevice(e->c.device));
    if (g0 < 0 || ng < 0 || g0 + ng > e->ntrace) return fail("trace range");
    if (chain_stride_rows < ng || !X) return fail("bad destination");
    if (ng == 0) return 0;
    if (!e->copy_stream) {
        HIPCK(hipStreamCreateWithFlags(&e->copy_stream, hipStreamNonBlocking));
        for (int s = 0; s < e->nlanes; ++s) HIPCK(hipEventCreateWithFlags(&e->copy_ev[s], hipEventDisableTiming));
    }
    for (int s = 0; s < e->nlanes; ++s) {
        HIPCK(hipEventRecord(e->copy_ev[s], e->lane_stream[s]));
        HIPCK(hipStreamWaitEvent(e->copy_stream, e->copy_ev[s], 0));
    }
    const size_t nl = e->p.nl, d = e->p.d, ld = e->p.ld, tcap = (size_t)e->p.tcap;
    hipMemcpy3DParms c;
    memset(&c, 0, sizeof(c));
    c.srcPtr = make_hipPitchedPtr((void*)(e->p.tX + (size_t)g0 * ld), sizeof(double) * ld, sizeof(double) * ld, tcap);
    c.dstPtr = make_hipPitchedPtr((void*)X, sizeof(double) * d, sizeof(double) * d, (size_t)chain_stride_rows);
    c.extent = make_hipExtent(sizeof(double) * d, (size_t)ng, nl);
    c.kind = hipMemcpyDeviceToHost;
    HIPCK(hipMemcpy3DAsync(&c, e->copy_stream));
    return 0;
}
int dz_trace_download_wait(dz_engine* e)
{
    HIPCK(hipSetDevice(e->c.device));
    if (e->copy_stream) HIPCK(hipStreamSynchronize(e->copy_stream));
    return 0;
}

// page-lock a host array ahead of a download (first-touch faults and pinning then overlap the run instead of the copy)
int dz_host_register(void* ptr, int64_t bytes)
{
    // Page-locking a freshly allocated array is mostly the kernel faulting its pages in, one at a time, on the calling thread (6.5 GB:
    // 0.27 s).  Large ranges are first populated by several threads after asking for huge pages -- madvise(MADV_POPULATE_WRITE) where the
    // kernel has it (5.14+), else an atomic add of zero to a byte of every page: either way nothing another thread writes meanwhile is
    // lost --; hipHostRegister then finds the pages present.  DZ_PIN_THREADS (default 8, 1 = off).
    int nt = 8;
    if (const char* s = getenv("DZ_PIN_THREADS")) nt = std::max(1, std::min(64, atoi(s)));
    if (bytes >= ((int64_t)64 << 20) && nt > 1) {
        const uintptr_t page = 4096, lo = ((uintptr_t)ptr + page - 1) & ~(page - 1), hi = ((uintptr_t)ptr + (uintptr_t)bytes) & ~(page - 1);
        if (hi > lo) {
            (void)madvise((void*)lo, hi - lo, MADV_HUGEPAGE);
            const uintptr_t npages = (hi - lo) / page;
            std::vector<std::thread> th;
            for (int t = 0; t < nt; ++t)
                th.emplace_back([=] {
                    const uintptr_t i0 = npages * t / nt, i1 = npages * (t + 1) / nt;
                    if (i1 <= i0) return;
#ifdef MADV_POPULATE_WRITE
                    if (madvise((void*)(lo + i0 * page), (i1 - i0) * page, MADV_POPULATE_WRITE) == 0) return;
#endif
                    unsigned char* q = (unsigned char*)lo;
                    for (uintptr_t i = i0; i < i1; ++i) __atomic_fetch_add(q + i * page, (unsigned char)0, __ATOMIC_RELAXED);
                });
            for (auto& x : th) x.join();
        }
    }
    if (hipHostRegister(ptr, (size_t)bytes, hipHostRegisterDefault) != hipSuccess) { (void)hipGetLastError(); return fail("hipHostRegister failed"); }
    return 0;
}
int dz_host_unregister(void* ptr)
{
    if (hipHostUnregister(ptr) != hipSuccess) { (void)hipGetLastError(); return fail("hipHostUnregister failed"); }
    return 0;
}

int dz_get_history(dz_engine* e, double* Z, int64_t cap_rows, int64_t* rows)
{
    HIPCK(hipSetDevice(e->c.device));
    if (rows) *rows = e->M;
    if (Z) {
        if (cap_rows < e->M) return fail("buffer too small");
        // peer transport with history_lag: the rows of the last appends may still be on their way
        if (e->peer_on && e->z_gated < e->napp) { DZCK(peer_gate(e, XK_Z, (unsigned long long)e->napp)); e->z_gated = e->napp; }
        DZCK(download_rows(e, Z, e->p.Z, (size_t)e->M));
        DZCK(peer_check(e));
    }
    return 0;
}

int dz_get_history_range(dz_engine* e, int64_t row0, int64_t nrows, double* Z)
{   // rows [row0, row0 + nrows) of the archive (what a continued run appends to the history file of the run before)
    HIPCK(hipSetDevice(e->c.device));
    if (row0 < 0 || nrows < 0 || row0 + nrows > e->M || !Z) return fail("history range");
    if (e->peer_on && e->z_gated < e->napp) { DZCK(peer_gate(e, XK_Z, (unsigned long long)e->napp)); e->z_gated = e->napp; }
    return download_rows(e, Z, e->p.Z + (size_t)row0 * e->p.ld, (size_t)nrows);
}

int dz_history_checksum(dz_engine* e, uint64_t* sum, int64_t* rows)
{   // every appended row of every rank has arrived (as dz_get_history), then one pass over the archive on the device
    HIPCK(hipSetDevice(e->c.device));
    if (!sum) return fail("null argument");
    if (e->peer_on && e->z_gated < e->napp) { DZCK(peer_gate(e, XK_Z, (unsigned long long)e->napp)); e->z_gated = e->napp; }
    DZCK(join_all(e));
    if (!e->d_bar) DZCK(ealloc(e, &e->d_bar, (size_t)std::max(1, e->world)));
    unsigned long long* acc = (unsigned long long*)e->d_bar;         // (the rendezvous buffer: idle between barriers)
    HIPCK(hipMemsetAsync(acc, 0, sizeof(unsigned long long), e->stream));
    if (e->M > 0) {
        const unsigned blocks = (unsigned)std::min<int64_t>((e->M + 3) / 4, (int64_t)e->num_cu * 16);
        hipLaunchKernelGGL(dz::k_checksum, dim3(blocks), dim3(256), 0, e->stream, (const double*)e->p.Z, (long long)e->M, e->p.d, e->p.ld, acc);
        DZCK(launch_check("k_checksum"));
    }
    unsigned long long h = 0;
    HIPCK(hipMemcpyAsync(&h, acc, sizeof h, hipMemcpyDeviceToHost, e->stream));
    DZCK(sync_all(e));
    *sum = (uint64_t)h;
    if (rows) *rows = e->M;
    return 0;
}

static int get_shared(dz_engine* e, const double* probs, const double* delta, const double* n, int nb, double* o_probs, double* o_delta, double* o_n)
{
    DZCK(sync_all(e));
    if (o_probs) HIPCK(hipMemcpy(o_probs, probs, sizeof(double) * nb, hipMemcpyDeviceToHost));
    if (o_delta) HIPCK(hipMemcpy(o_delta, delta, sizeof(double) * nb, hipMemcpyDeviceToHost));
    if (o_n) HIPCK(hipMemcpy(o_n, n, sizeof(double) * nb, hipMemcpyDeviceToHost));
    return 0;
}
int dz_get_cr_state(dz_engine* e, double* probs, double* delta_m, double* n_updates)
{
    HIPCK(hipSetDevice(e->c.device));
    DZCK(adapt_flush(e));           // (adapt_lag >= 1: the updates the next generation decides with are in; later ones stay pending)
    return get_shared(e, e->p.cr_probs, e->p.cr_delta, e->p.cr_n, e->c.ncr, probs, delta_m, n_updates);
}
int dz_get_gamma_state(dz_engine* e, double* probs, double* delta_m, double* n_updates)
{
    HIPCK(hipSetDevice(e->c.device));
    DZCK(adapt_flush(e));
    return get_shared(e, e->p.g_probs, e->p.g_delta, e->p.g_n, e->c.ngamma, probs, delta_m, n_updates);
}

static int chain_moments(dz_engine* e)
{
    if (e->ntrace < 2) return fail("need at least 2 traced generations");
    const dz::Params& p = e->p;
    hipLaunchKernelGGL(dz::k_chain_moments, dim3((p.d + 127) / 128, p.nl), dim3(128), 0, e->stream, p.tX, p.nl, p.d, p.ld, p.tcap, (int)e->ntrace, e->d_cmean, e->d_cvar);
    return launch_check("chain moments");
}
int dz_get_chain_moments(dz_engine* e, double* mean, double* var)
{
    HIPCK(hipSetDevice(e->c.device));
    DZCK(chain_moments(e));
    DZCK(sync_all(e));
    const size_t n = (size_t)e->p.nl * e->p.d;
    HIPCK(hipMemcpy(mean, e->d_cmean, sizeof(double) * n, hipMemcpyDeviceToHost));
    HIPCK(hipMemcpy(var, e->d_cvar, sizeof(double) * n, hipMemcpyDeviceToHost));
    return 0;
}
int dz_get_rhat(dz_engine* e, double* rhat)
{
    HIPCK(hipSetDevice(e->c.device));
    DZCK(chain_moments(e));
    const dz::Params& p = e->p;
    hipLaunchKernelGGL(dz::k_rhat, dim3((p.d + 15) / 16), dim3(1024), sizeof(double) * 16 * (size_t)((p.nl + 63) / 64), e->stream, e->d_cmean, e->d_cvar, p.nl, p.d, (int)e->ntrace, e->d_rhat);
    DZCK(launch_check("rhat"));
    DZCK(sync_all(e));
    HIPCK(hipMemcpy(rhat, e->d_rhat, sizeof(double) * p.d, hipMemcpyDeviceToHost));
    return 0;
}

static int need_scratch(dz_engine* e, size_t rows)
{
    const hipError_t err = grow_doubles(&e->d_scratch, &e->scratch_rows, rows, rows * e->p.ld + 4 * rows, false);
    if (err != hipSuccess) return fail(std::string("hipMalloc((void**)&e->d_scratch, sizeof(double) * (rows * e->p.ld + 4 * rows)): ") + hipGetErrorString(err));
    return 0;
}

int dz_eval_logp(dz_engine* e, const double* X, int64_t n, double* prior, double* like)
{
    HIPCK(hipSetDevice(e->c.device));
    if (n > (1 << 22)) return fail("too many points in one call");
    DZCK(need_scratch(e, (size_t)n));
    double* pts = e->d_scratch; double* dp = pts + (size_t)n * e->p.ld; double* dl = dp + n;
    DZCK(upload_padded(e, pts, X, (int)n, 0.0));
    e->multi = multi_shape(e);
    DZCK(eval_logp(e, pts, (int)n, dp, dl));
    DZCK(sync_all(e));
    HIPCK(hipMemcpy(prior, dp, sizeof(double) * n, hipMemcpyDeviceToHost));
    HIPCK(hipMemcpy(like, dl, sizeof(double) * n, hipMemcpyDeviceToHost));
    return 0;
}

int dz_eval_outputs(dz_engine* e, const double* X, int64_t n, double* like_items, double* out)
{
    if (!e || !X || !like_items || !out) return fail("null argument");
    if (!e->out_fn) return fail("dz_eval_outputs: call dz_set_output_module first");
    if (n < 1) return fail("dz_eval_outputs: n must be >= 1");
    if (n > (1 << 22)) return fail("too many points in one call");
    HIPCK(hipSetDevice(e->c.device));
    const unsigned per_block = 256u / (unsigned)e->out_lanes;      // the grid rules of dz_set_likelihood_module, over items
    const long long items = (long long)n * e->out_items, blocks = (items + per_block - 1) / per_block;
    if (blocks > 0x7fffffffll) return fail("dz_eval_outputs: " + std::to_string(items) + " items are more than one launch's grid holds");
    DZCK(need_scratch(e, (size_t)n));
    DZCK(sync_all(e));
    const struct { double** buf; size_t* have; size_t want; const char* what; } outs[] = {{&e->d_out, &e->out_len, (size_t)items * (size_t)e->out_doubles, "the outputs"}, {&e->d_out_like, &e->out_like_len, (size_t)items, "the terms"}};
    for (const auto& o : outs) {
        const hipError_t err = grow_doubles(o.buf, o.have, o.want, o.want, false);
        if (err != hipSuccess) return fail(std::string("dz_eval_outputs: cannot allocate ") + std::to_string(o.want) + " doubles for " + o.what + ": " + hipGetErrorString(err));
    }
    double* pts = e->d_scratch;
    DZCK(upload_padded(e, pts, X, (int)n, 0.0));
    struct { const double* X; long long n; int d; int ld; double* like; const void* data; double* out; long long out_ld; } a =
        {pts, items, e->p.d, e->p.ld, e->d_out_like, e->d_out_data, e->d_out, (long long)e->out_doubles};
    size_t asz = sizeof(a);
    void* extra[] = {HIP_LAUNCH_PARAM_BUFFER_POINTER, &a, HIP_LAUNCH_PARAM_BUFFER_SIZE, &asz, HIP_LAUNCH_PARAM_END};
    HIPCK(hipModuleLaunchKernel(e->out_fn, (unsigned)blocks, 1, 1, 256, 1, 1, 0, e->stream, nullptr, extra));
    DZCK(sync_all(e));
    HIPCK(hipMemcpy(like_items, e->d_out_like, sizeof(double) * (size_t)items, hipMemcpyDeviceToHost));
    HIPCK(hipMemcpy(out, e->d_out, sizeof(double) * (size_t)items * (size_t)e->out_doubles, hipMemcpyDeviceToHost));
    return 0;
}

int dz_debug_propose(dz_engine* e, int32_t chain_local, int64_t gen, int32_t phase, const double* base,
                     int32_t run_snooker, int32_t cr_idx, int32_t delta, int32_t glev, double* pts, double* slogp)
{
    HIPCK(hipSetDevice(e->c.device));
    const int n = phase == 0 ? e->p.k : e->p.k - 1;
    if (n < 1) return fail("no reference phase for multitry=1");
    DZCK(need_scratch(e, (size_t)n + 1));
    double* dbase = e->d_scratch; double* dout = dbase + e->p.ld; double* dsl = dout + (size_t)n * e->p.ld;
    DZCK(upload_padded(e, dbase, base, 1, 0.0));
    NCH_DISPATCH(e, hipLaunchKernelGGL(dz::k_propose_debug<NCH>, dim3(1), dim3(64), 0, e->stream, e->p, phase, (uint32_t)gen, (uint32_t)e->M,
                                       chain_local, n, dbase, dout, dsl, run_snooker, cr_idx, delta, glev));
    DZCK(launch_check("propose(debug)"));
    DZCK(download_rows(e, pts, dout, (size_t)n));
    HIPCK(hipMemcpy(slogp, dsl, sizeof(double) * n, hipMemcpyDeviceToHost));
    return 0;
}

int dz_profile_enable(dz_engine* e, int32_t on)
{
    e->prof = on != 0;
    if (on > 1) {   // on = number of event pairs to pre-create, so that the timed region only records
        HIPCK(hipSetDevice(e->c.device));
        while ((int64_t)e->ev_pool.size() < 2 * (int64_t)on) { hipEvent_t x; HIPCK(hipEventCreate(&x)); e->ev_pool.push_back(x); }
    }
    return 0;
}
int dz_profile_reset(dz_engine* e)
{
    HIPCK(hipSetDevice(e->c.device));
    DZCK(sync_all(e));
    for (auto& v : e->ev) { for (auto& pr : v) { e->ev_pool.push_back(pr.first); e->ev_pool.push_back(pr.second); } v.clear(); }
    if (e->prof) {   // class 6: event pairs with nothing in between = what one bracket adds to every measured launch
        for (int i = 0; i < 64; ++i) { ProfScope ps(e, PR_EMPTY, e->stream); }
        DZCK(sync_all(e));
    }
    return 0;
}
int dz_profile_get(dz_engine* e, int32_t which, double* total_ms, int64_t* launches)
{
    if (which < 0 || which >= PR_COUNT) return fail("bad profile class");
    HIPCK(hipSetDevice(e->c.device));
    DZCK(sync_all(e));
    double tot = 0.0;
    for (auto& pr : e->ev[which]) { float ms = 0.f; HIPCK(hipEventElapsedTime(&ms, pr.first, pr.second)); tot += ms; }
    if (total_ms) *total_ms = tot;
    if (launches) *launches = (int64_t)e->ev[which].size();
    return 0;
}

int dz_profile_get_list(dz_engine* e, int32_t which, double* ms, int64_t cap, int64_t* launches)
{   // the individual launches of a class, in launch order (dz_profile_get gives their sum)
    if (which < 0 || which >= PR_COUNT) return fail("bad profile class");
    HIPCK(hipSetDevice(e->c.device));
    DZCK(sync_all(e));
    int64_t i = 0;
    for (auto& pr : e->ev[which]) { if (i >= cap) break; float t = 0.f; HIPCK(hipEventElapsedTime(&t, pr.first, pr.second)); ms[i++] = t; }
    if (launches) *launches = (int64_t)e->ev[which].size();
    return 0;
}

}  // extern "C"
