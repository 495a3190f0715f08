// dz_ode_group.h -- dz_ode.h's solver for networks of 9..64 species: a GROUP of L = 16, 32 or 64 lanes integrates one point together
// (likelihoods.MassActionODELogLike(..., lanes_per_point=16 | 32) for up to 32 species, lanes_per_point=64, a whole wave per point, for
// 33..64).  A group never straddles a wave.  There is ONE solver, Group<Net, L> and the functions it calls, for the three lane counts;
// L decides only how lanes talk to each other (Lanes<L>) and where the replicated state lives (Replica<Net, L>): see "a wave per point".
// The method is dz_ode.h's, and so is the code: its stepping loop
// (dzode::integrate: step controller, negativity rule, max_steps per output interval, exact landing on the output times, events, -inf on
// any failure) runs here on the shape Group below, with Rodas4's coefficients and the start step's formulas; what changes is who holds what.  Lane r of a group (r = threadIdx.x % L) owns
//     row r of W = I / (h gamma) - J in registers (S doubles, constant column indices after unrolling),
//     entry r of y, of the stage argument u and of k1..k6;
// every lane reads, at constant indices, one replicated copy of the state the right-hand side is evaluated at (S doubles, refilled once
// per stage): with 16 or 32 lanes its own S registers, with 64 lanes the wave's S doubles of LDS.
// Lanes r >= S idle: they carry zeros, never pivot, and are masked out of every reduction.  The rate constants (up to 128; 256 for a wave
// per point) are computed once per point, reaction j by lane j % L, and kept in static LDS (256 / L points x (R + 1) doubles per block).
//
// Linear algebra over the group (16 | 32 lanes: ds_bpermute through __shfl / __shfl_xor with width L; no LDS round trip, no MFMA: a pivoted
// f64 LU of S <= 64 is a chain of S dependent column steps, latency- and not throughput-bound):
//   LU, implicit partial pivoting: per column k a butterfly arg-max of |w[k]| over the lanes that have not pivoted yet (equal maxima:
//     the lowest row; a NaN counts as +inf), the pivot's reciprocal and its row right of k broadcast, one multiplier and one rank-1 row
//     update per remaining lane.  Rows do not move: piv[k] is the row that pivoted in column k, pos the column a row pivoted in.
//   Solves, column-oriented: forward, k ascending: b[piv[k]] broadcast, rows with pos > k subtract their multiple; backward, k descending:
//     x_k = b[piv[k]] / pivot broadcast, rows with pos < k subtract their multiple, lane k keeps x_k.
//   Sums (error norm, start step norms): the xor butterfly, i.e. the pairwise tree ((v0 + v1) + (v2 + v3)) + ... over L entries, idle
//     lanes adding 0.  neg / finite predicates: a ballot restricted to the group's lanes.
// Control flow is uniform per group (every lane of a group computes h, t, err2, ... from the same broadcast values and so holds the same
// bits); the groups of a wave may diverge from each other, so nothing inside a step loop is wider than a group.
//
// The host twin (HostGroup below) is a plain loop over rows that performs the same floating-point operations in the same order: the same
// generated rhs_row / jac_entry, the same pivot rule, the same column-oriented solves, the same summation tree.  It holds only those
// parts; loop, start step and fixed steps are dz_ode.h's, written on HostGroup's rhs, wnorm2 and step.  It does not give the
// bits of dz_ode.h on a network both can run (lu_solve's row-oriented back substitution sums in the other direction).
//
// The network comes from generated code (likelihoods._ode_group_source): a struct with
//     static constexpr int S, R, O;  static constexpr bool LOG10;
//     static int rate_index(int j);       the parameter index of reaction j's rate constant, -1 for a fixed one
//     static double rate_fixed(int j);    the fixed rate constant of reaction j
//     static double rhs_row(int r, const double* k, const double* y);              f[r] = sum over reactions j, ascending, of N[r][j] v_j(y),
//                                                                                  N[r][j] a select over constants: no branch on r
//     static double jac_entry(int r, int q, const double* k, const double* y);     J[r][q], same order (0 where no reaction links them)
//     static void obs(const double* y, double* o);
// and, for a network with monomials (dz_ode.h's head: the construct, its arithmetic and the members live, y0_row, scale, constraints),
//     static double rate_mono(int j, const double* x, bool& good);    the rate constant of a reaction whose rate_index is -2
// and, for a network with rate laws (dz_ode.h's head, RATE LAWS: Hill factors and kinetic orders inside rhs_row / jac_entry),
//     static constexpr int SLOTS;  static double slot(int m, const double* x, bool& good);    Kn of the distinct (K, n) pair m: entry R + m of k
// and, for a network with sampled noise (dz_ode.h's head, NOISE: the members NOISE, noise_value and noise_terms), the point's 2 O noise
// values at the very end of its LDS row (noise_row), value m evaluated by lane m % L when the rate constants are; the host twin takes
// them from dz_ode.h's noise_point, the same generated function value by value.
// and, for a network with inputs (dz_ode.h's head, INPUTS: the members INPUTS, DRIVE = R + SLOTS + I, input_species, input_scaled and
//     static double gain(int i, const double* x, bool& good);         g_i and its liveness (an input without a gain: 1)
// ), 2 I more doubles of the point's LDS row right behind the rate constants and slots: entry R + SLOTS + i is the gain g_i, evaluated by
// lane (R + SLOTS + i) % L when the rate constants are, entry DRIVE + i the drive, which one lane of the group writes when a knot is
// applied (Group::knot) and the generated rhs_row of the input's row selects; the host twin keeps the same 2 I entries in its array k.
// Data block: dz_ode.h's (with several conditions: its [C, stride] header and C sub-blocks; with events: its records after sd; with the
// equilibration phase: its six doubles at the end; with inputs: the knot records behind those.  The phase itself is dz_ode.h's loop on this shape's drift2: the lane's rhs_row and
// the group's norm, a group-wide value; with a steady output, dz_ode.h's STEADY OUTPUT: its six doubles behind the equilibration's and in
// front of the knots, and the same loop on the same drift2 at the experiment's end).
#pragma once
#include "dz_ode.h"

// Inside a generated sum, every four terms: on the device the partial sum v, the row index r and an offset z (always 0) added to the
// rate constants' index pass through an empty asm statement together, so the next terms' LDS reads and stoichiometric selects depend on the previous terms' sum and
// cannot be issued ahead of it.  Values and order of operations are unchanged; what it bounds is the registers a sum of R terms holds
// at once (without it the compiler starts all R reads and selects up front, and R = 128 does not fit the register file).
#if defined(__HIP_DEVICE_COMPILE__)
#define DZODE_SUM_FENCE(v, r, z) asm volatile("" : "+v"(v), "+v"(r), "+v"(z))
#else
#define DZODE_SUM_FENCE(v, r, z) ((void)0)
#endif

namespace dzode {

// The stage arguments and the (1/h) sum c_ij k_j terms of dz_ode.h's rodas4_step, entry by entry, shared by both builds.
// stage 5's argument is stage 4's plus k5 (u: the previous stage's argument).
DZO_HD double stage_arg(int st, double y, double u, double k1, double k2, double k3, double k4, double k5)
{
    typedef Rodas4 M;
    switch (st) {
    case 0: return y;
    case 1: return y + M::a21 * k1;
    case 2: return y + M::a31 * k1 + M::a32 * k2;
    case 3: return y + M::a41 * k1 + M::a42 * k2 + M::a43 * k3;
    case 4: return y + M::a51 * k1 + M::a52 * k2 + M::a53 * k3 + M::a54 * k4;
    default: return u + k5;
    }
}

DZO_HD double stage_add(int st, double ih, double k1, double k2, double k3, double k4, double k5)
{
    typedef Rodas4 M;
    switch (st) {
    case 1: return (M::c21 * k1) * ih;
    case 2: return (M::c31 * k1 + M::c32 * k2) * ih;
    case 3: return (M::c41 * k1 + M::c42 * k2 + M::c43 * k3) * ih;
    case 4: return (M::c51 * k1 + M::c52 * k2 + M::c53 * k3 + M::c54 * k4) * ih;
    default: return (M::c61 * k1 + M::c62 * k2 + M::c63 * k3 + M::c64 * k4 + M::c65 * k5) * ih;
    }
}

// The doubles at the head of a point's row of values: rate constants, Hill slots and, with inputs, their gains and drives.
template <class Net> constexpr int ROW_VALUES = Net::R + has_slots<Net>::count + 2 * has_inputs<Net>::count;
// ... of which the first are evaluated once per point (the drives are per-experiment state, written when a knot is applied)
template <class Net> constexpr int ROW_CONSTANTS = Net::R + has_slots<Net>::count + has_inputs<Net>::count;

DZO_HD double pivot_key(double a)          // |a|, a NaN as +inf: the arg-max is then over a total order
{
    const double v = dabs(a);
    return v == v ? v : __builtin_huge_val();
}

template <class Net>
DZO_HD double rate_constant(int j, const double* x, bool& good)
{
    if constexpr (has_inputs<Net>::value) {     // (entry R + SLOTS + i of the row: the gain of input i, dz_ode.h's INPUTS)
        if (j >= Net::R + has_slots<Net>::count) return Net::gain(j - Net::R - has_slots<Net>::count, x, good);
    }
    if constexpr (has_slots<Net>::value) {      // (entry R + m of the row: the Hill slot m, dz_ode.h's RATE LAWS)
        if (j >= Net::R) return Net::slot(j - Net::R, x, good);
    }
    const int pi = Net::rate_index(j);
    if constexpr (has_monomials<Net>::value) {
        if (pi == -2) return Net::rate_mono(j, x, good);
    }
    if (pi < 0) {
        const double kv = Net::rate_fixed(j);
        good = finite(kv);
        return kv;
    }
    const double xv = x[pi];
    const double kv = Net::LOG10 ? dexp(xv * 2.302585092994046) : xv;
    good = finite(xv) && finite(kv);          // (10**-inf is a finite 0: test x itself)
    return kv;
}

#if defined(__HIP__)
// ---------------------------------------------------------------- the device side: one lane's share
// The lane's row index as the network's functions see it: the same value, but one the compiler cannot trace back to threadIdx.  The
// stoichiometric selects of rhs_row / jac_entry depend on r alone; hoisted out of the step loop they would be hundreds of live registers.
__device__ __forceinline__ int row_index(int r)
{
    asm volatile("" : "+v"(r));
    return r;
}

template <int L>
struct Lanes {
    static_assert(L == 16 || L == 32, "a group is 16 or 32 lanes");
    __device__ __forceinline__ static double from(double v, int src) { return __shfl(v, src, L); }        // lane src of this group
    __device__ __forceinline__ static int from(int v, int src) { return __shfl(v, src, L); }
    __device__ __forceinline__ static double sum(double v)
    {
#pragma unroll
        for (int m = 1; m < L; m <<= 1) v = v + __shfl_xor(v, m, L);
        return v;
    }
    __device__ __forceinline__ static bool any(bool p)
    {
        const unsigned long long mask = (L == 32 ? 0xffffffffull : 0xffffull) << ((threadIdx.x & 63) & ~(L - 1));
        return (__ballot(p) & mask) != 0;
    }
};

// ---------------------------------------------------------------- a wave per point: 33..64 species
// The same solver with L = 64: the same method, pivot rule, column-oriented solves, summation tree and roundings, and HostGroup<Net, 64>
// is its twin.  Two things are placed differently, because a row of 64 doubles (128 registers) and a replicated state beside it do not
// fit 512 registers:
//     the replicated state            in LDS, S doubles per wave behind the wave's rate constants (wave_state): lane r writes entry r,
//                                     every lane reads entry q at a constant q -- one address per read, a broadcast without a bank conflict.
//                                     Only this wave touches them, so a wave-scope fence orders the write and the reads; there is NO
//                                     block barrier anywhere in or after the step loop (the four waves of a block take different numbers
//                                     of steps);
//     pivot reciprocal, pivot row,    the pivot index is the same in every lane of the wave (the butterfly arg-max is over a total
//     b[piv[k]] in the solves         order), so it goes to a scalar register (readfirstlane) and the value is read with v_readlane into
//                                     scalar registers: no LDS-crossbar round trip on the dependent chain, and piv[] costs no VGPR.
// Row r of W stays in lane r's registers.  The arg-max, the sums and the ballots span the wave and need no mask.
template <>
struct Lanes<64> {
    // lane src of this wave; src must hold the same value in every lane (it is read from the first active one)
    __device__ __forceinline__ static int from(int v, int src) { return __builtin_amdgcn_readlane(v, __builtin_amdgcn_readfirstlane(src)); }
    __device__ __forceinline__ static double from(double v, int src)
    {
        const int s = __builtin_amdgcn_readfirstlane(src);
        const uint64_t b = d2bits(v);
        const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)b, s), hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(b >> 32), s);
        return bits2d(((uint64_t)hi << 32) | lo);
    }
    __device__ __forceinline__ static double sum(double v)
    {
#pragma unroll
        for (int m = 1; m < 64; m <<= 1) v = v + __shfl_xor(v, m, 64);
        return v;
    }
    __device__ __forceinline__ static bool any(bool p) { return __ballot(p) != 0; }
};

// A wave-uniform index in a scalar register the compiler cannot trace back (the scalar twin of row_index).
__device__ __forceinline__ int uniform_index(int v)
{
    v = __builtin_amdgcn_readfirstlane(v);
    asm volatile("" : "+s"(v));
    return v;
}

// The wave's copy of the state in LDS, behind its R + 1 rate constants (a network with rate laws: R + SLOTS + 1; with inputs: + 2 I).
template <class Net>
__device__ __forceinline__ double* wave_state(double* ks) { return ks + ROW_VALUES<Net> + 1; }

// Lane r's entry into the wave's copy.  The fences keep the compiler from moving the reads of the previous copy below the write and the
// reads of this copy above it; the hardware executes one wave's LDS operations in order.
template <int S>
__device__ __forceinline__ void wave_publish(double* ys, int r, double v)
{
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
    if (r < S) ys[r] = v;
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

constexpr int WAVE_LU_AHEAD = 8;          // 64 lanes: columns of one rank-1 update whose pivot-row broadcasts may be in flight together

// ---------------------------------------------------------------- the solver, for every L
// The replicated state: fill(r, own) makes every lane's entry visible to the group, y is where every lane then reads the S entries.
// ks: the point's row of LDS (group_lds_row).  (fill returns nothing and the callers read through the member: a pointer held in a local
// of the stage loop was enough to change the register allocation of the loop.)
template <class Net, int L>
struct Replica {                              // 16 | 32 lanes: S registers per lane, refilled by S group broadcasts
    double y[Net::S];
    __device__ __forceinline__ explicit Replica(double*) {}
    __device__ __forceinline__ void fill(int, double own)
    {
#pragma unroll
        for (int q = 0; q < Net::S; ++q) y[q] = Lanes<L>::from(own, q);
    }
};
template <class Net>
struct Replica<Net, 64> {                     // a wave: its S doubles of LDS; a wave that is not live touches nothing but its own row
    double* y;
    __device__ __forceinline__ explicit Replica(double* ks) : y(wave_state<Net>(ks)) {}
    __device__ __forceinline__ void fill(int r, double own) { wave_publish<Net::S>(y, r, own); }
};

// The point's noise values in its row of LDS: behind the rate constants, the slots and (64 lanes) the wave's state.
template <class Net, int L>
__device__ __forceinline__ double* noise_row(double* ks) { return ks + ROW_VALUES<Net> + 1 + (L == 64 ? Net::S : 0); }

// The item's viewed row (dz_ode.h's VIEWS) in its row of LDS: P doubles behind everything else.
template <class Net, int L>
__device__ __forceinline__ double* view_row(double* ks) { return noise_row<Net, L>(ks) + has_noise<Net>::count; }

// The row a group's item reads in the point's place.  A network with a view: lane r gathers the entries r, r + L, ... of the view
// from the table at the end of the item's sub-block (item w of C to a point: sub-block w % C of the block behind hdr, stride doubles
// each) into the group's row, and ONE block-wide barrier follows, before group_rates reads them; every group of the block gets here,
// the padding groups with the last item's view.  Else: the point's own row, no barrier, and nothing computed from the other arguments
// (the code objects of networks without a view are what they were).
template <class Net, int L>
__device__ __forceinline__ const double* group_viewed_row(const double* x, const double* hdr, long long w, long long C, long long stride, double* ks,
                                                          int r)
{
    if constexpr (has_view<Net>::value) {
        double* xv = view_row<Net, L>(ks);
        const double* tab = hdr + 2 + (w - (w / C) * C + 1) * stride - 2 * Net::VIEW;
        for (int i = r; i < Net::VIEW; i += L) xv[i] = view_entry(x, tab, i);
        __syncthreads();
        return xv;
    } else {
        return x;
    }
}

template <class Net, int L>
__device__ __forceinline__ bool group_rates(const double* x, double* ks, int r)
{
    bool good = true;
    for (int j = r; j < ROW_CONSTANTS<Net>; j += L) {
        bool g;
        ks[j] = rate_constant<Net>(j, x, g);
        good = good && g;
    }
    if constexpr (has_noise<Net>::value) {      // (the point's noise values, behind everything else in its row: dz_ode.h's NOISE)
        for (int m = r; m < has_noise<Net>::count; m += L) {
            bool g;
            noise_row<Net, L>(ks)[m] = Net::noise_value(m, x, g);
            good = good && g;
        }
    }
    return !Lanes<L>::any(!(good && monomials_live<Net>(x)));
}

// piv: the row that pivoted in column k, four columns to an int
__device__ __forceinline__ int pivot_row(const int* piv, int k) { return (piv[k >> 2] >> (8 * (k & 3))) & 0xff; }

template <int S, int L>
__device__ __forceinline__ bool group_lu_factor(double* w, int* piv, int& pos, int r)
{
    bool ok = true, done = r >= S;
    pos = -1;
#pragma unroll
    for (int k = 0; k < S; ++k) {
        double key = done ? -1.0 : pivot_key(w[k]);
        int p = r;
#pragma unroll
        for (int m = 1; m < L; m <<= 1) {
            const double okey = __shfl_xor(key, m, L);
            const int op = __shfl_xor(p, m, L);
            const bool take = (okey > key) | ((okey == key) & (op < p));
            key = take ? okey : key;
            p = take ? op : p;
        }
        if constexpr (L == 64) p = __builtin_amdgcn_readfirstlane(p);          // every lane holds the same p: the arg-max of a total order over the whole wave
        piv[k >> 2] = (k & 3) ? piv[k >> 2] | (p << (8 * (k & 3))) : p;
        ok = ok && key != 0.0;
        const bool me = p == r, upd = !done && !me;
        const double inv = Lanes<L>::from(1.0 / w[k], p);
        double l = w[k] * inv;
        w[k] = me ? inv : (upd ? l : w[k]);
#pragma unroll
        for (int c = k + 1; c < S; ++c) {
            // 64 lanes: every WAVE_LU_AHEAD columns the last updated entry, the multiplier and the pivot's lane pass through an empty asm
            // statement together: the next columns' readlanes depend on it and are not all issued (into scalar registers) ahead of the updates
            if constexpr (L == 64)
                if ((c - k - 1) % WAVE_LU_AHEAD == 0 && c > k + 1) asm volatile("" : "+v"(w[c - 1]), "+v"(l), "+s"(p));
            const double pc = Lanes<L>::from(w[c], p);
            w[c] = upd ? w[c] - l * pc : w[c];
        }
        done = done || me;
        pos = me ? k : pos;
    }
    return ok;
}

template <int S, int L>
__device__ __forceinline__ double group_lu_solve(const double* w, const int* pivp, int pos, int r, double b)
{
    int piv[(S + 3) / 4];          // (opaque copies: the S broadcast addresses and 3 S lane masks the compiler would otherwise carry from
#pragma unroll                     //  the factorisation through all six solves are rebuilt here from these few registers; 64 lanes: scalar ones)
    for (int i = 0; i < (S + 3) / 4; ++i) {
        if constexpr (L == 64) piv[i] = uniform_index(pivp[i]);
        else piv[i] = row_index(pivp[i]);
    }
    pos = row_index(pos);
    r = row_index(r);
#pragma unroll
    for (int k = 0; k < S; ++k) {
        const double bk = Lanes<L>::from(b, pivot_row(piv, k));
        b = pos > k ? b - w[k] * bk : b;
    }
    double x = 0.0;
#pragma unroll
    for (int k = S - 1; k >= 0; --k) {
        const double xk = Lanes<L>::from(b * w[k], pivot_row(piv, k));
        b = (pos >= 0 && pos < k) ? b - w[k] * xk : b;
        x = r == k ? xk : x;
    }
    return x;
}

// w[0..Q) = row r of I / (h gamma) - J, column by column.  A recursion over the column and not a loop: every column index must be a
// constant (w lives in registers), and a loop around the whole generated switch is too long for the compiler to unroll on its own.
// zk is an offset (always 0) into the rate constants: R of them are read from LDS where they are used, not kept in registers across steps.
template <class Net, int Q>
struct JacobianRow {
    __device__ __forceinline__ static void fill(double* w, int& rj, int& zk, const double* ks, const double* yr, int r, double fac)
    {
        JacobianRow<Net, Q - 1>::fill(w, rj, zk, ks, yr, r, fac);
        double m = -Net::jac_entry(rj, Q - 1, ks + zk, yr);
        DZODE_SUM_FENCE(m, rj, zk);             // (column by column, for the same reason as inside a sum)
        w[Q - 1] = Q - 1 == r ? m + fac : m;
    }
};
template <class Net>
struct JacobianRow<Net, 0> {
    __device__ __forceinline__ static void fill(double*, int&, int&, const double*, const double*, int, double) {}
};

// One step of size h: this lane's entry of the order-4 solution and the group's err2.  False if the iteration matrix is singular.
template <class Net, int L>
__device__ __forceinline__ bool group_step(double* ks, double y, double h, double rtol, double atol, int r, double& ynew, double& err2)
{
    constexpr int S = Net::S;
    Replica<Net, L> rep(ks);
    double w[S];
    int piv[(S + 3) / 4], pos;
    const double fac = 1.0 / (h * Rodas4::gamma), ih = 1.0 / h;
    rep.fill(r, y);
    int rj = row_index(r), zk = row_index(0);
    JacobianRow<Net, S>::fill(w, rj, zk, ks, rep.y, r, fac);
    const bool ok = group_lu_factor<S, L>(w, piv, pos, r);
    double k1 = 0.0, k2 = 0.0, k3 = 0.0, k4 = 0.0, k5 = 0.0, f = 0.0, arg = y;
#pragma unroll 1
    for (int st = 0; st < 6; ++st) {          // (one copy of the right-hand side and of the solve in the code object, not six)
        arg = stage_arg(st, y, arg, k1, k2, k3, k4, k5);
        rep.fill(r, arg);                         // (also at stage 0: registers the Jacobian read are not kept alive across the LU)
        f = Net::rhs_row(row_index(r), ks + row_index(0), rep.y);
        if (st > 0) f = f + stage_add(st, ih, k1, k2, k3, k4, k5);
        f = group_lu_solve<S, L>(w, piv, pos, r, f);
        k1 = st == 0 ? f : k1;
        k2 = st == 1 ? f : k2;
        k3 = st == 2 ? f : k3;
        k4 = st == 3 ? f : k4;
        k5 = st == 4 ? f : k5;
    }
    ynew = arg + f;                            // arg: y5 + k5, f: k6
    const double sk = atol + rtol * dmax(dabs(y), dabs(ynew));
    const double q = f / sk;
    err2 = Lanes<L>::sum(r < S ? q * q : 0.0) * (1.0 / S);
    return ok;
}

template <int S, int L>
__device__ __forceinline__ double group_wnorm2(double v, double y, double rtol, double atol, int r)
{
    const double q = v / (atol + rtol * dabs(y));
    return Lanes<L>::sum(r < S ? q * q : 0.0) * (1.0 / S);
}

template <class Net, int L>
__device__ __forceinline__ double group_start_step(double* ks, double y, double rtol, double atol, double span, int r)
{
    constexpr int S = Net::S;
    Replica<Net, L> rep(ks);
    rep.fill(r, y);
    const double f0 = Net::rhs_row(row_index(r), ks, rep.y);
    const double d0 = group_wnorm2<S, L>(y, y, rtol, atol, r), d1 = group_wnorm2<S, L>(f0, y, rtol, atol, r);
    const double h0 = start_h0(d0, d1, span);
    rep.fill(r, y + h0 * f0);
    const double f1 = Net::rhs_row(row_index(r), ks, rep.y) - f0;
    return start_h(h0, d1, group_wnorm2<S, L>(f1, y, rtol, atol, r), span);
}

// The group's shape for dz_ode.h's integrate: lane r's entry of the state.  Every lane of the group returns the same value.  The caller's
// live = false (a point past the batch's end, or a rate constant that is not finite): no step is taken, -inf.
template <class NET, int L>
struct Group {
    typedef NET Net;
    static constexpr int S = Net::S, O = Net::O, EVENTS = has_events<Net>::count, INPUTS = has_inputs<Net>::count;
    static constexpr bool EQUILIBRATE = has_equilibrate<Net>::value, SETTLE = has_settle<Net>::value;
    typedef double State;
    double* ks;                                        // the point's row of LDS: its rate constants (64 lanes: and its state behind them)
    int r;
    const double* x;                                   // the point's row (read only by a network with monomials)
    __device__ __forceinline__ const double* noise() const { return noise_row<Net, L>(ks); }      // (a network with sampled noise)
    __device__ __forceinline__ void init(const double* blk, double& y) const { y = r < S ? start_amount<Net>(r, x, blk[6 + r]) : 0.0; }
    __device__ __forceinline__ double start_step(double y, double rtol, double atol, double span) const
    {
        return group_start_step<Net, L>(ks, y, rtol, atol, span, r);
    }
    // the steady-state test's norm of f(y), group-wide: for the equilibration phase and for the steady output's (dz_ode.h's STEADY OUTPUT)
    // alike -- a member template's function exists only where a loop calls it, so EQUILIBRATE or SETTLE alone brings it in
    __device__ __forceinline__ double drift2(double y, double rtol, double atol) const
    {
        Replica<Net, L> rep(ks);
        rep.fill(r, y);
        return group_wnorm2<S, L>(Net::rhs_row(row_index(r), ks, rep.y), y, rtol, atol, r);
    }
    __device__ __forceinline__ bool step(double y, double h, double rtol, double atol, double& yn, double& err2) const
    {
        return group_step<Net, L>(ks, y, h, rtol, atol, r, yn, err2);
    }
    __device__ __forceinline__ bool all_finite(double yn, bool fin) const { return fin && !Lanes<L>::any(!finite(yn)); }
    __device__ __forceinline__ bool any_negative(double yn, double y, double rtol, double atol) const
    {
        return Lanes<L>::any(yn < -(atol + rtol * dabs(y)));
    }
    __device__ __forceinline__ void observe(double y, double* o) const
    {
        Replica<Net, L> rep(ks);
        rep.fill(r, y);
        observe_scaled<Net>(x, rep.y, o);
    }
    __device__ __forceinline__ void apply(double& y, int species, double factor, double amount) const
    {
        y = r == species ? factor * y + amount : y;
    }
    // A knot of input i (dz_ode.h's INPUTS): the value into the lane that holds its species, the slope into its drive in the point's
    // row of LDS.  One lane of the group writes the drive, between the fence and wave_barrier that wave_publish uses: only the point's
    // own wave reads it, in the right-hand sides that follow, and the hardware executes one wave's LDS operations in order.  No block
    // barrier: the groups of a block take their knots at different times.
    __device__ __forceinline__ void knot(double& y, int i, double value, double slope) const
    {
        if constexpr (INPUTS > 0) {
            const double gv = Net::input_scaled(i, ks, value), gs = Net::input_scaled(i, ks, slope);
            y = r == Net::input_species(i) ? gv : y;
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
            __builtin_amdgcn_wave_barrier();
            if (r == 0) ks[Net::DRIVE + i] = gs;
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
            __builtin_amdgcn_wave_barrier();
        }
    }
};

// The doubles of static LDS a point's lanes share: R + 1 rate constants (with rate laws: R + SLOTS + 1, the Hill slots behind the rate
// constants; with inputs: 2 I more, their gains and drives behind those), for a wave per point the S doubles of its state behind them, for a network with sampled noise its 2 O values and for one with a view (dz_ode.h's VIEWS) the item's P viewed coordinates last.
template <class Net, int L>
constexpr int group_lds_row() { return ROW_VALUES<Net> + 1 + (L == 64 ? Net::S : 0) + has_noise<Net>::count + has_view<Net>::count; }
#endif

#if !defined(__HIP__)
// ---------------------------------------------------------------- the host twin: the same operations, row by row
template <class NET, int L>
struct HostGroup {
    typedef NET Net;
    static constexpr int S = Net::S, R = Net::R;
    static_assert(S <= L, "a lane per species");

    static double sum(double* a)               // a[L], overwritten: the butterfly's tree as lane 0 sees it
    {
        for (int m = 1; m < L; m <<= 1)
            for (int i = 0; i < L; i += 2 * m) a[i] = a[i] + a[i + m];
        return a[0];
    }

    static bool rates(const double* x, double* k)
    {
        bool good = true;
        for (int j = 0; j < ROW_CONSTANTS<Net>; ++j) {
            bool g;
            k[j] = rate_constant<Net>(j, x, g);
            good = good && g;
        }
        return good && monomials_live<Net>(x);
    }

    static bool lu_factor(double* w, int* piv, int* pos)
    {
        bool ok = true, done[S];
        for (int r = 0; r < S; ++r) { done[r] = false; pos[r] = -1; }
        for (int k = 0; k < S; ++k) {
            double best = -1.0;
            int p = -1;
            for (int r = 0; r < S; ++r) {
                if (done[r]) continue;
                const double v = pivot_key(w[r * S + k]);
                if (v > best) { best = v; p = r; }
            }
            piv[k] = p;
            ok = ok && best != 0.0;
            const double inv = 1.0 / w[p * S + k];
            for (int r = 0; r < S; ++r) {
                if (done[r] || r == p) continue;
                const double l = w[r * S + k] * inv;
                w[r * S + k] = l;
                for (int c = k + 1; c < S; ++c) w[r * S + c] = w[r * S + c] - l * w[p * S + c];
            }
            w[p * S + k] = inv;
            done[p] = true;
            pos[p] = k;
        }
        return ok;
    }

    static void lu_solve(const double* w, const int* piv, const int* pos, double* b)       // b: the right-hand side in, the solution out
    {
        double x[S];
        for (int k = 0; k < S; ++k) {
            const double bk = b[piv[k]];
            for (int r = 0; r < S; ++r)
                if (pos[r] > k) b[r] = b[r] - w[r * S + k] * bk;
        }
        for (int k = S - 1; k >= 0; --k) {
            const double xk = b[piv[k]] * w[piv[k] * S + k];
            for (int r = 0; r < S; ++r)
                if (pos[r] < k) b[r] = b[r] - w[r * S + k] * xk;
            x[k] = xk;
        }
        for (int s = 0; s < S; ++s) b[s] = x[s];
    }

    static bool step(const double* k, const double* y, double h, double rtol, double atol, double* ynew, double* yemb, double& err2)
    {
        double w[S * S], kk[5][S], f[S], arg[S], e[L];
        int piv[S], pos[S];
        const double fac = 1.0 / (h * Rodas4::gamma), ih = 1.0 / h;
        for (int r = 0; r < S; ++r)
            for (int q = 0; q < S; ++q) {
                const double m = -Net::jac_entry(r, q, k, y);
                w[r * S + q] = q == r ? m + fac : m;
            }
        const bool ok = lu_factor(w, piv, pos);
        for (int i = 0; i < 5; ++i)
            for (int s = 0; s < S; ++s) kk[i][s] = 0.0;
        for (int s = 0; s < S; ++s) arg[s] = y[s];
        for (int st = 0; st < 6; ++st) {
            for (int s = 0; s < S; ++s) arg[s] = stage_arg(st, y[s], arg[s], kk[0][s], kk[1][s], kk[2][s], kk[3][s], kk[4][s]);
            for (int s = 0; s < S; ++s) {
                f[s] = Net::rhs_row(s, k, arg);
                if (st > 0) f[s] = f[s] + stage_add(st, ih, kk[0][s], kk[1][s], kk[2][s], kk[3][s], kk[4][s]);
            }
            lu_solve(w, piv, pos, f);
            if (st < 5)
                for (int s = 0; s < S; ++s) kk[st][s] = f[s];
        }
        for (int i = 0; i < L; ++i) e[i] = 0.0;
        for (int s = 0; s < S; ++s) {
            yemb[s] = arg[s];
            ynew[s] = arg[s] + f[s];
            const double sk = atol + rtol * dmax(dabs(y[s]), dabs(ynew[s]));
            const double q = f[s] / sk;
            e[s] = q * q;
        }
        err2 = sum(e) * (1.0 / S);
        return ok;
    }

    static double wnorm2(const double* v, const double* y, double rtol, double atol)
    {
        double e[L];
        for (int i = 0; i < L; ++i) e[i] = 0.0;
        for (int s = 0; s < S; ++s) {
            const double q = v[s] / (atol + rtol * dabs(y[s]));
            e[s] = q * q;
        }
        return sum(e) * (1.0 / S);
    }

    static void rhs(const double* k, const double* y, double* f)
    {
        for (int s = 0; s < S; ++s) f[s] = Net::rhs_row(s, k, y);
    }
};
#endif

}  // namespace dzode

// The entry points around a generated network struct NET for groups of LANES = 16, 32 or 64 lanes: the batch kernel the engine's multi-kernel path
// launches (dz_set_likelihood_module with lanes_per_point LANES: 256 threads per block, point i on lanes [i * LANES, (i + 1) * LANES) of
// the grid; with 64 lanes: 4 points per block, one per wave) and the host build's C functions under dz_ode.h's names.  A group whose point index is >= n reads the last point's row,
// takes no step and stores nothing: it stays with its wave through every cross-lane operation.
#if defined(__HIP__) && !defined(DZODE_PREDICT)
#define DZODE_GROUP_ENTRIES(NET, LANES)                                                                                                 \
    extern "C" __global__ __launch_bounds__(256) void dz_ode_group_batch(const double* X, long long n, int d, int ld, double* like,     \
                                                                        const void* data)                                              \
    {                                                                                                                                    \
        static_assert(NET::S <= LANES, "a lane per species");                                                                            \
        __shared__ double ks[256 / LANES][dzode::group_lds_row<NET, LANES>()];        /* (R + 1: the groups of a wave read the same j    \
                                                                                         from different banks; 64 lanes: + the state) */ \
        const long long i = ((long long)blockIdx.x * 256 + threadIdx.x) / LANES;                                                         \
        const int r = threadIdx.x % LANES, g = threadIdx.x / LANES;                                                                      \
        const bool valid = i < n;                                                                                                        \
        const double* x = X + (valid ? i : n - 1) * ld;                                                                                  \
        const bool good = dzode::group_rates<NET, LANES>(x, ks[g], r);                                                                   \
        __syncthreads();                                       /* (before any loop a group can leave early) */                           \
        const double v = dzode::integrate(dzode::Group<NET, LANES>{ks[g], r, x}, (const double*)data, valid && good, nullptr, nullptr); \
        if (valid && r == 0) like[i] = good ? dzode::add_constraints<NET>(v, x, true) : v;                                               \
    }
// ... with C conditions (dz_ode.h's block with the [C, stride] header): a group per ITEM, item w = condition w % C of point w / C; the
// groups past the last item are predicated as above.
#define DZODE_GROUP_ITEM_ENTRIES(NET, LANES)                                                                                            \
    extern "C" __global__ __launch_bounds__(256) void dz_ode_group_item_batch(const double* X, long long n, int d, int ld, double* like, \
                                                                             const void* data)                                         \
    {                                                                                                                                    \
        static_assert(NET::S <= LANES, "a lane per species");                                                                            \
        __shared__ double ks[256 / LANES][dzode::group_lds_row<NET, LANES>()];                                                           \
        const long long w = ((long long)blockIdx.x * 256 + threadIdx.x) / LANES;                                                         \
        const int r = threadIdx.x % LANES, g = threadIdx.x / LANES;                                                                      \
        const bool valid = w < n;                                                                                                        \
        const double* hdr = (const double*)data;                                                                                         \
        const long long C = (long long)hdr[0], stride = (long long)hdr[1], wv = valid ? w : n - 1, i = wv / C;                           \
        const double* x = dzode::group_viewed_row<NET, LANES>(X + i * ld, hdr, wv, C, stride, ks[g], r);                                 \
        const bool good = dzode::group_rates<NET, LANES>(x, ks[g], r);                                                                   \
        __syncthreads();                                                                                                                 \
        const double v = dzode::integrate(dzode::Group<NET, LANES>{ks[g], r, x}, hdr + 2 + (wv - i * C) * stride, valid && good,        \
                                          nullptr, nullptr);                                                                             \
        if (valid && r == 0) like[w] = good ? dzode::add_constraints<NET>(v, x, wv == i * C) : v;                                        \
    }
#elif defined(__HIP__)
// The prediction kernels (dz_ode.h, PREDICTION) of the lane group: every lane of a group holds the same o[], so lane 0 alone is given the
// item's slice and stores each value once -- the other lanes, and the padding groups of the last block, pass sim = nullptr and store
// nothing --, and lane 0 overwrites the slice of a failed item with NaN.  No LDS beyond the likelihood kernel's.
#define DZODE_GROUP_ENTRIES(NET, LANES)                                                                                                 \
    extern "C" __global__ __launch_bounds__(256) void dz_ode_group_predict(const double* X, long long n, int d, int ld, double* like,   \
                                                                          const void* data, double* out, long long out_ld)             \
    {                                                                                                                                    \
        static_assert(NET::S <= LANES, "a lane per species");                                                                            \
        __shared__ double ks[256 / LANES][dzode::group_lds_row<NET, LANES>()];                                                           \
        const long long i = ((long long)blockIdx.x * 256 + threadIdx.x) / LANES;                                                         \
        const int r = threadIdx.x % LANES, g = threadIdx.x / LANES;                                                                      \
        const bool valid = i < n;                                                                                                        \
        const double* x = X + (valid ? i : n - 1) * ld;                                                                                  \
        const bool good = dzode::group_rates<NET, LANES>(x, ks[g], r);                                                                   \
        __syncthreads();                                                                                                                 \
        double* sim = valid && r == 0 ? out + i * out_ld : nullptr;                                                                      \
        const double v = dzode::integrate(dzode::Group<NET, LANES>{ks[g], r, x}, (const double*)data, valid && good, sim, nullptr);     \
        const double term = good ? dzode::add_constraints<NET>(v, x, true) : v;                                                          \
        if (sim) {                                                                                                                       \
            like[i] = term;                                                                                                              \
            dzode::predict_finish(term, (const double*)data, NET::O, sim);                                                               \
        }                                                                                                                                \
    }
#define DZODE_GROUP_ITEM_ENTRIES(NET, LANES)                                                                                            \
    extern "C" __global__ __launch_bounds__(256) void dz_ode_group_item_predict(const double* X, long long n, int d, int ld,            \
                                                                               double* like, const void* data, double* out,            \
                                                                               long long out_ld)                                       \
    {                                                                                                                                    \
        static_assert(NET::S <= LANES, "a lane per species");                                                                            \
        __shared__ double ks[256 / LANES][dzode::group_lds_row<NET, LANES>()];                                                           \
        const long long w = ((long long)blockIdx.x * 256 + threadIdx.x) / LANES;                                                         \
        const int r = threadIdx.x % LANES, g = threadIdx.x / LANES;                                                                      \
        const bool valid = w < n;                                                                                                        \
        const double* hdr = (const double*)data;                                                                                         \
        const long long C = (long long)hdr[0], stride = (long long)hdr[1], wv = valid ? w : n - 1, i = wv / C;                           \
        const double* x = dzode::group_viewed_row<NET, LANES>(X + i * ld, hdr, wv, C, stride, ks[g], r);                                 \
        const double* blk = hdr + 2 + (wv - i * C) * stride;                                                                             \
        const bool good = dzode::group_rates<NET, LANES>(x, ks[g], r);                                                                   \
        __syncthreads();                                                                                                                 \
        double* sim = valid && r == 0 ? out + w * out_ld : nullptr;                                                                      \
        const double v = dzode::integrate(dzode::Group<NET, LANES>{ks[g], r, x}, blk, valid && good, sim, nullptr);                     \
        const double term = good ? dzode::add_constraints<NET>(v, x, wv == i * C) : v;                                                   \
        if (sim) {                                                                                                                       \
            like[w] = term;                                                                                                              \
            dzode::predict_finish(term, blk, NET::O, sim);                                                                               \
        }                                                                                                                                \
    }
#else
#define DZODE_GROUP_ENTRIES(NET, LANES)                                                                                                 \
    typedef dzode::HostGroup<NET, LANES> DzodeHostGroup;                                                                                 \
    DZODE_HOST_ENTRIES(DzodeHostGroup)
#define DZODE_GROUP_ITEM_ENTRIES(NET, LANES)                                                                                            \
    typedef dzode::HostGroup<NET, LANES> DzodeHostGroup;                                                                                 \
    DZODE_HOST_ITEM_ENTRIES(DzodeHostGroup)
#endif
