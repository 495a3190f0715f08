// dz_prior_ext.h -- the per-dimension priors beyond flat, normal and uniform (dz_set_prior_ext, include/dreamzs.h), written once for the device kernel
// (k_prior_ext, dz_kernels.h), its host twin (dz_prior_ext_host, dz_engine.hip) and a host-only test (tests/test_prior_ext_cpu.py): the term of one
// dimension, the constants the host makes for it, its support, and the test redo_possible needs.  Plain C++ on the host: no HIP header is needed there.
//
// A dimension is a distribution in scipy's parametrisation: loc = a, scale = b > 0, shapes s1 and s2.  z = (x - a) rb with rb = 1 / b made once on the
// host; L is dlog; the term is core(z) + c, ONE final addition, the core evaluated left to right as written; c is made once on the host in binary64 from
// <cmath> and includes -log b.
//
//   kind  scipy name            core(z) on the support                          support in z     c before -log b
//   0     (flat)                0                                               all              --        (the term is 0)
//   1     norm                  today's expression (prior_of_point): (-(z z) / 2 - 0.918...) - dlog(b)
//   2     uniform               today's expression: a <= x <= a + b ? -dlog(b) : -inf
//   3     laplace               -|z|                                            all              -log 2
//   4     cauchy                -L(1 + z z)                                     all              -log pi
//   5     t (s1 = nu)           -((nu + 1) / 2) L(1 + (z z)(1 / nu))            all              lgamma((nu + 1) / 2) - lgamma(nu / 2) - log(nu pi) / 2
//   6     lognorm (s1 = s)      w = L(z); -(w w) h - w,  h = 1 / (2 s s)        z > 0            -log s - log(2 pi) / 2
//   7     gamma (s1 = k)        (k - 1) L(z) - z; first term absent at k == 1   z >= 0           -lgamma(k)
//   8     beta (s1, s2 = al,be) (al - 1) L(z) + (be - 1) L(1 - z); a term whose coefficient is exactly 0 is absent
//                                                                               0 <= z <= 1      lgamma(al + be) - lgamma(al) - lgamma(be)
//   9     halfnorm              -(z z) / 2                                      z >= 0           log(2 / pi) / 2
//   10    halfcauchy            -L(1 + z z)                                     z >= 0           log(2 / pi)
//   11    truncnorm (lo, hi)    -(z z) / 2                                      lo <= z <= hi    -log(2 pi) / 2 - log(Phi(hi) - Phi(lo))
//   12    loguniform (lo, hi)   -L(z)                                           lo <= z <= hi    -log(log(hi / lo))
//   13    invgamma (s1 = k)     -(k + 1) L(z) - 1 / z                           z > 0            -lgamma(k)
//
// Outside the support the term is exactly -inf.  At a closed end where a logarithm's argument is 0 the term is decided here and never left to dlog(0); it
// is what scipy says: gamma at z = 0 is +inf for k < 1, c for k = 1, -inf for k > 1; beta likewise at both ends.  A NaN coordinate gives NaN (kinds >= 3)
// or what today's expressions give (kinds 1, 2); the engine's nan_to_ninf maps the point's sum.
#pragma once
#include <stdint.h>
#include <string.h>
#if defined(__HIP__)
#include "dz_device.h"
#define DZ_PE_HD __host__ __device__ __forceinline__
#else
#define DZ_PE_HD inline
#endif
#include <cmath>

namespace dz {

enum { PRIOR_FLAT = 0, PRIOR_NORM, PRIOR_UNIFORM, PRIOR_LAPLACE, PRIOR_CAUCHY, PRIOR_T, PRIOR_LOGNORM, PRIOR_GAMMA, PRIOR_BETA, PRIOR_HALFNORM, PRIOR_HALFCAUCHY,
       PRIOR_TRUNCNORM, PRIOR_LOGUNIFORM, PRIOR_INVGAMMA, PRIOR_KINDS };

// dlog (dz_device.h) restated for the host: the same operation sequence (fma and the division are correctly rounded on both sides)
DZ_PE_HD double pe_log_host(double x)
{
    if (x != x) return x;
    if (x < 0.0) return __builtin_nan("");
    if (x == 0.0) return -__builtin_huge_val();
    if (x == __builtin_huge_val()) return x;
    int e = 0;
    uint64_t b; memcpy(&b, &x, 8);
    if ((b >> 52) == 0) { x = x * 18014398509481984.0; e = -54; memcpy(&b, &x, 8); }
    e += (int)(b >> 52) - 1023;
    b = (b & 0x000fffffffffffffull) | 0x3ff0000000000000ull;
    double m; memcpy(&m, &b, 8);
    if (m > 1.4142135623730951) { m = m * 0.5; e += 1; }
    const double f = m - 1.0;
    const double s = f / (2.0 + f);
    const double z = s * s;
    double p = 1.0 / 23.0;
    p = __builtin_fma(p, z, 1.0 / 21.0);
    p = __builtin_fma(p, z, 1.0 / 19.0);
    p = __builtin_fma(p, z, 1.0 / 17.0);
    p = __builtin_fma(p, z, 1.0 / 15.0);
    p = __builtin_fma(p, z, 1.0 / 13.0);
    p = __builtin_fma(p, z, 1.0 / 11.0);
    p = __builtin_fma(p, z, 1.0 / 9.0);
    p = __builtin_fma(p, z, 1.0 / 7.0);
    p = __builtin_fma(p, z, 1.0 / 5.0);
    p = __builtin_fma(p, z, 1.0 / 3.0);
    const double t = 2.0 * s;
    const double lm = __builtin_fma(t * z, p, t);
    const double ef = (double)e;
    return __builtin_fma(ef, 6.93147180369123816490e-01, __builtin_fma(ef, 1.90821492927058770002e-10, lm));
}
DZ_PE_HD double pe_log(double x)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return dlog(x);
#else
    return pe_log_host(x);
#endif
}

// What the term reads of one dimension.  rb: 1 / b (uniform: a + b, the upper end, as Params::pc2); c: the constant (normal, uniform: dlog(b), as
// Params::plogb); p1, p2: the shapes as the core uses them -- t: (nu + 1) / 2, 1 / nu; lognorm: h; gamma: k - 1; beta: al - 1, be - 1;
// truncnorm, loguniform: lo, hi; invgamma: k + 1.
struct PriorExtRow { double a, rb, c, p1, p2; };

// ---- the term ----------------------------------------------------------------------------------------------------------------------------------------
DZ_PE_HD double prior_ext_term(int kind, double x, double a, double rb, double c, double p1, double p2)
{
    const double ninf = -__builtin_huge_val();
    if (kind == PRIOR_FLAT) return 0.0;
    if (kind == PRIOR_NORM) { const double z = (x - a) * rb; return (-(z * z) / 2.0 - 0.91893853320467274178) - c; }
    if (kind == PRIOR_UNIFORM) return (x >= a && x <= rb) ? -c : ninf;
    const double z = (x - a) * rb;
    if (z != z) return z;
    double core;
    switch (kind) {
        case PRIOR_LAPLACE: core = -(z < 0.0 ? -z : z); break;
        case PRIOR_CAUCHY: core = -pe_log(1.0 + z * z); break;
        case PRIOR_T: core = -(p1 * pe_log(1.0 + (z * z) * p2)); break;
        case PRIOR_LOGNORM: {
            if (!(z > 0.0)) return ninf;
            const double w = pe_log(z);
            core = -(w * w) * p1 - w;
        } break;
        case PRIOR_GAMMA:
            if (z < 0.0) return ninf;
            if (p1 == 0.0) core = -z;
            else {
                if (z == 0.0) return p1 < 0.0 ? __builtin_huge_val() : ninf;
                core = p1 * pe_log(z) - z;
            }
            break;
        case PRIOR_BETA: {
            if (z < 0.0 || z > 1.0) return ninf;
            if (z == 0.0 && p1 != 0.0) return p1 < 0.0 ? __builtin_huge_val() : ninf;
            if (z == 1.0 && p2 != 0.0) return p2 < 0.0 ? __builtin_huge_val() : ninf;
            if (p1 != 0.0 && p2 != 0.0) core = p1 * pe_log(z) + p2 * pe_log(1.0 - z);
            else if (p1 != 0.0) core = p1 * pe_log(z);
            else if (p2 != 0.0) core = p2 * pe_log(1.0 - z);
            else core = 0.0;
        } break;
        case PRIOR_HALFNORM: if (z < 0.0) return ninf; core = -(z * z) / 2.0; break;
        case PRIOR_HALFCAUCHY: if (z < 0.0) return ninf; core = -pe_log(1.0 + z * z); break;
        case PRIOR_TRUNCNORM: if (z < p1 || z > p2) return ninf; core = -(z * z) / 2.0; break;
        case PRIOR_LOGUNIFORM: if (z < p1 || z > p2) return ninf; core = -pe_log(z); break;
        case PRIOR_INVGAMMA: if (!(z > 0.0)) return ninf; core = -(p1 * pe_log(z)) - 1.0 / z; break;
        default: return __builtin_nan("");
    }
    return core + c;
}

// ---- the constants (host) ----------------------------------------------------------------------------------------------------------------------------
// Phi(hi) - Phi(lo) of the standard normal from erfc on the side that does not cancel
inline double prior_ext_normal_mass(double lo, double hi)
{
    const double r = 0.70710678118654752440;
    if (lo > 0.0 && hi > 0.0) return 0.5 * std::erfc(lo * r) - 0.5 * std::erfc(hi * r);       // upper tails
    if (lo < 0.0 && hi < 0.0) return 0.5 * std::erfc(-hi * r) - 0.5 * std::erfc(-lo * r);     // lower tails
    return 1.0 - 0.5 * std::erfc(-lo * r) - 0.5 * std::erfc(hi * r);
}
inline bool pe_finite(double x) { return x - x == 0.0; }
// One dimension's row from scipy's numbers (kinds 1 and 2 keep dlog(b) as their constant, as Params::plogb does).  Returns nullptr, or what is wrong with the dimension.
inline const char* prior_ext_row(int kind, double a, double b, double s1, double s2, PriorExtRow& r)
{
    const double pi = 3.14159265358979323846;
    r = PriorExtRow{0.0, 0.0, 0.0, 0.0, 0.0};
    if (kind < 0 || kind >= PRIOR_KINDS) return "prior kind must be 0..13";
    if (kind == PRIOR_FLAT) return nullptr;
    if (!(pe_finite(b) && b > 0.0)) return "scale must be finite and > 0";
    if (!pe_finite(a)) return "loc must be finite";
    r.a = a; r.rb = 1.0 / b;
    if (kind == PRIOR_NORM) { r.c = pe_log_host(b); return nullptr; }
    if (kind == PRIOR_UNIFORM) { r.rb = a + b; r.c = pe_log_host(b); return nullptr; }
    double c0 = 0.0;
    switch (kind) {
        case PRIOR_LAPLACE: c0 = -std::log(2.0); break;
        case PRIOR_CAUCHY: c0 = -std::log(pi); break;
        case PRIOR_T:
            if (!(pe_finite(s1) && s1 > 0.0)) return "t: the degrees of freedom must be finite and > 0";
            r.p1 = (s1 + 1.0) / 2.0; r.p2 = 1.0 / s1;
            c0 = std::lgamma((s1 + 1.0) / 2.0) - std::lgamma(s1 / 2.0) - 0.5 * std::log(s1 * pi);
            break;
        case PRIOR_LOGNORM:
            if (!(pe_finite(s1) && s1 > 0.0)) return "lognorm: the shape must be finite and > 0";
            r.p1 = 1.0 / (2.0 * (s1 * s1));
            c0 = -std::log(s1) - 0.5 * std::log(2.0 * pi);
            break;
        case PRIOR_GAMMA:
            if (!(pe_finite(s1) && s1 > 0.0)) return "gamma: the shape must be finite and > 0";
            r.p1 = s1 - 1.0; c0 = -std::lgamma(s1);
            break;
        case PRIOR_BETA:
            if (!(pe_finite(s1) && s1 > 0.0 && pe_finite(s2) && s2 > 0.0)) return "beta: both shapes must be finite and > 0";
            r.p1 = s1 - 1.0; r.p2 = s2 - 1.0;
            c0 = std::lgamma(s1 + s2) - std::lgamma(s1) - std::lgamma(s2);
            break;
        case PRIOR_HALFNORM: c0 = 0.5 * std::log(2.0 / pi); break;
        case PRIOR_HALFCAUCHY: c0 = std::log(2.0 / pi); break;
        case PRIOR_TRUNCNORM: {
            if (!(s1 < s2)) return "truncnorm: the ends must satisfy lo < hi";
            const double mass = prior_ext_normal_mass(s1, s2);
            if (!(pe_finite(mass) && mass > 0.0)) return "truncnorm: the truncated mass is not > 0";
            r.p1 = s1; r.p2 = s2;
            c0 = -0.5 * std::log(2.0 * pi) - std::log(mass);
        } break;
        case PRIOR_LOGUNIFORM:
            if (!(pe_finite(s1) && pe_finite(s2) && 0.0 < s1 && s1 < s2)) return "loguniform: the ends must satisfy 0 < lo < hi";
            r.p1 = s1; r.p2 = s2;
            c0 = -std::log(std::log(s2 / s1));
            break;
        case PRIOR_INVGAMMA:
            if (!(pe_finite(s1) && s1 > 0.0)) return "invgamma: the shape must be finite and > 0";
            r.p1 = s1 + 1.0; c0 = -std::lgamma(s1);
            break;
    }
    r.c = c0 - std::log(b);
    if (!pe_finite(r.c)) return "the constant of the density is not finite";
    return nullptr;
}

// ---- a point's prior on the host, in the kernel's order ----------------------------------------------------------------------------------------------
// lane l adds dimensions 128 it + 2 l and 128 it + 2 l + 1 in ascending order per chunk it, chunks ascending; the 64 partial sums meet in the xor
// butterfly 32, 16, 8, 4, 2, 1 (wave_bfly).
inline double prior_ext_point_host(const int32_t* kind, const PriorExtRow* rows, int d, const double* x)
{
    double acc[64], nxt[64];
    for (int l = 0; l < 64; ++l) acc[l] = 0.0;
    for (int it = 0; 128 * it < d; ++it)
        for (int l = 0; l < 64; ++l)
            for (int s = 0; s < 2; ++s) {
                const int j = 128 * it + 2 * l + s;
                if (j < d) acc[l] = acc[l] + prior_ext_term(kind[j], x[j], rows[j].a, rows[j].rb, rows[j].c, rows[j].p1, rows[j].p2);
            }
    for (int off = 32; off >= 1; off >>= 1) {
        for (int l = 0; l < 64; ++l) nxt[l] = acc[l] + acc[l ^ off];
        for (int l = 0; l < 64; ++l) acc[l] = nxt[l];
    }
    return acc[0];
}

// ---- support and the redraw rule (host, pure) --------------------------------------------------------------------------------------------------------
// [lo, hi] in x, and per end whether the log density is finite there (an infinite end: true, nothing reaches it)
struct PriorExtSupport { double lo, hi; bool lo_finite, hi_finite; };
inline PriorExtSupport support(int kind, double a, double b, double s1, double s2)
{
    const double inf = __builtin_huge_val();
    PriorExtSupport S = {-inf, inf, true, true};
    switch (kind) {
        case PRIOR_UNIFORM: S.lo = a; S.hi = a + b; break;
        case PRIOR_LOGNORM: case PRIOR_INVGAMMA: S.lo = a; S.lo_finite = false; break;
        case PRIOR_GAMMA: S.lo = a; S.lo_finite = s1 == 1.0; break;
        case PRIOR_BETA: S.lo = a; S.hi = a + b; S.lo_finite = s1 == 1.0; S.hi_finite = s2 == 1.0; break;
        case PRIOR_HALFNORM: case PRIOR_HALFCAUCHY: S.lo = a; break;
        case PRIOR_TRUNCNORM: case PRIOR_LOGUNIFORM: S.lo = a + b * s1; S.hi = a + b * s2; break;
        default: break;
    }
    return S;
}
// Can no proposal be impossible under this dimension's prior?  A dimension of unbounded support: yes.  Of bounded support: only when hard boundaries are
// on, [mn, mx] lies inside the support, and the log density is finite at every finite end the boundaries reach.  "Inside" is asked of the term's own test
// (z = (x - a) / b against the ends in z, which is monotone in x), so that an end that rounds differently in x cannot be missed.
inline bool covered(int kind, double a, double b, double s1, double s2, bool hard, double mn, double mx)
{
    const PriorExtSupport S = support(kind, a, b, s1, s2);
    if (S.lo == -__builtin_huge_val() && S.hi == __builtin_huge_val()) return true;
    if (!hard) return false;
    if (kind == PRIOR_UNIFORM) return mn >= a && mx <= a + b;
    if (!(mn <= mx)) return false;
    double zlo = 0.0, zhi = __builtin_huge_val();
    if (kind == PRIOR_BETA) zhi = 1.0;
    if (kind == PRIOR_TRUNCNORM || kind == PRIOR_LOGUNIFORM) { zlo = s1; zhi = s2; }
    const double rb = 1.0 / b, z0 = (mn - a) * rb, z1 = (mx - a) * rb;
    if (!(z0 >= zlo && z1 <= zhi)) return false;
    if (z0 == zlo && !S.lo_finite) return false;
    if (z1 == zhi && !S.hi_finite) return false;
    return true;
}
}  // namespace dz
