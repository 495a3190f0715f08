"""Targets and inputs shared by tests/test_serial_primitives_cpu.py and tests/test_mega_serial_gpu.py: the two MVN targets that drive the
special paths of the multi-try selection and ratio (dz::mt_select_vals, dz::mt_log_ratio; oracle: chain_step), and the value sets the
elementary functions and the ordered in-row prefix sum are checked on."""
import numpy as np

from tests import helpers as H

# STEEP: the reference's correlated MVN with its precision times 1e4 -- two tries' log densities differ by far more than 745, so every
#        selection weight but the largest underflows to an exact 0 (dexp's lower cut-off), and in the ratio one of the two sums is an exact 0
#        whenever the largest term stands on the other side: SA / SB is 0 (dlog(0) = -inf -> -DBL_MAX) or +inf (-> +DBL_MAX).
# FLAT:  the precision times 1e-30 under log_F = 1: every log density is 1 - 0.5e-30 Q = 1 to the last bit, so all tries tie, every weight
#        is exp(0), the cumulative probabilities are the rounded multiples of 1/5 and SA / SB is exactly 1.
TARGETS = {"steep": (1e4, 0.0), "flat": (1e-30, 1.0)}


def set_target(e, d, kind, target):
    scale, log_F = TARGETS[target]
    P = H.mvn_precision(d) * scale
    if kind == "tri":
        e.set_likelihood_mvn(np.zeros(d), H.tri_factor(P), 1, log_F)
    else:
        e.set_likelihood_mvn(np.zeros(d), P, 0, log_F)


def f64(bits):
    return np.array(bits, dtype=np.uint64).view(np.float64)


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def elementary_inputs(seed=5):
    """arguments for dexp / dlog: every special case and both sides of every threshold, then random bit patterns and random ordinary values"""
    nxt = lambda v, to: np.nextafter(v, to)
    inf, nan = np.inf, np.nan
    sp = [0.0, -0.0, 1.0, -1.0, inf, -inf, nan, 5e-324, -5e-324, 2.2250738585072014e-308, nxt(2.2250738585072014e-308, 0.0), 1.7976931348623157e308,
          -1.7976931348623157e308, 1e-310, 3e-320, 0.5, 2.0, 1.4142135623730951, nxt(1.4142135623730951, 2.0), nxt(1.4142135623730951, 1.0),
          0.7071067811865476, nxt(1.0, 2.0), nxt(1.0, 0.0), 1e300, -1e300, 1e19, -1e19, 2147483648.0, -2147483649.0]
    for t in (709.782712893384, -745.2, 709.79, -746.0, -745.13321910194122, 709.4361393, -693.14718055994530942, -693.5, -745.4798, -708.3964185322641):
        sp += [t, nxt(t, inf), nxt(t, -inf)]
    sp = np.array(sp)
    sp = np.concatenate([sp, f64([0x7ff0000000000001, 0xfff8000000000123, 0x7ff8000000000000, 0xfff0000000000001, 0x7ffc0de000000001])])   # signalling and payload NaNs
    rng = np.random.default_rng(seed)
    rnd = f64(rng.integers(0, 2**64, 4000, dtype=np.uint64))
    ordinary = np.concatenate([rng.uniform(-760.0, 720.0, 4000), np.exp(rng.uniform(-745.0, 709.0, 4000)), rng.uniform(-1075.5, 1024.5, 2000) * 0.6931471805599453,
                               5e-324 * rng.integers(1, 2**52, 1000).astype(float)])
    return np.concatenate([sp, rnd, ordinary])


def prefix_rows(seed=6):
    """rows of 32 values (two DPP rows of 16 lanes) for the ordered prefix sum: +-0.0 in every leading position, subnormals, terms 2^+-1000
    apart, +inf, -inf (inf - inf), NaN in the middle, and random rows of mixed magnitude where the order of the additions shows in the bits"""
    rng = np.random.default_rng(seed)
    rows = [np.full(32, -0.0), np.full(32, 0.0), np.where(np.arange(32) % 2, 0.0, -0.0), np.where(np.arange(32) % 2, -0.0, 0.0),
            np.concatenate([np.full(3, -0.0), np.ones(29)]), np.full(32, 5e-324), 5e-324 * rng.integers(1, 2**40, 32).astype(float),
            np.where(np.arange(32) % 3 == 0, 2.0**1000, 2.0**-1000) * rng.uniform(1, 2, 32),
            np.where(np.arange(32) % 4 == 1, 1.0715086071862673e301, 9.332636185032189e-302) * rng.choice([-1.0, 1.0], 32)]
    r = rng.uniform(0, 1, 32); r[5] = np.inf; r[21] = np.inf; rows.append(r)
    r = rng.uniform(0, 1, 32); r[2] = np.inf; r[9] = -np.inf; r[18] = -np.inf; rows.append(r)
    r = rng.uniform(0, 1, 32); r[7] = np.nan; r[16] = np.nan; rows.append(r)
    r = np.full(32, 1.7976931348623157e308); rows.append(r)                               # overflows to +inf at the second term
    for _ in range(12):
        rows.append(rng.uniform(-1, 1, 32) * 2.0 ** rng.integers(-60, 60, 32))
    for _ in range(4):
        rows.append(np.exp(rng.uniform(-745, 0, 32)))                                       # what the kernels sum: weights in (0, 1]
    return np.array(rows)


def sequential_prefix(w):
    """the contract's sum: S = 0.0; S = S + w_0; S = S + w_1; ...  -> every prefix, for each row of w (.., n)"""
    out = np.empty_like(w)
    S = np.zeros(w.shape[:-1])
    with np.errstate(all="ignore"):
        for j in range(w.shape[-1]):
            S = S + w[..., j]
            out[..., j] = S
    return out


def row_prefix_model(w, K):
    """dz::row_prefix_ordered<K> on rows of 16 lanes (w: (.., 16)): K - 1 copies of w shifted up by K-1, .., 1 lanes (a source outside the row
    reads +0.0) are added in that order to +0.0, then w itself.  Lanes i < K hold the prefix."""
    assert w.shape[-1] == 16 and 1 <= K <= 16
    c = np.zeros_like(w)
    with np.errstate(all="ignore"):
        for s in range(K - 1, 0, -1):
            sh = np.zeros_like(w)
            sh[..., s:] = w[..., :16 - s]
            c = c + sh
        c = c + w
    return c


def first_hit_loop(u, cum, K):
    """the loop the ballot replaces: the first i < K with u < cum_i, else K - 1"""
    sel, found = K - 1, False
    for i in range(K):
        hit = (not found) and bool(u < cum[i])
        sel = i if hit else sel
        found = found or hit
    return sel


def first_hit_ballot(u, cum, K):
    """one compare in every lane, the mask cut to lanes 0..K-1 with bit K-1 set in any case, find-first-set"""
    with np.errstate(invalid="ignore"):
        mask = sum(1 << i for i in range(len(cum)) if u < cum[i])
    mask = (mask & ((1 << K) - 1)) | (1 << (K - 1))
    return (mask & -mask).bit_length() - 1
