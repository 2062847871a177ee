"""Arguments of the libm tests, shared by the host test (tests/test_libm_restatement.py) and the device test
(tests/test_libm_device.py): for each of the eight restated routines (strelka_amd/csrc/libm_flt32.h, libm_dbl64.h) and for the scalar
functions the kernels build on them, named arrays built from bit patterns -- table-interval edges, rounding boundaries of the table
index, the subnormal-result ranges, the thresholds between a routine's branches -- plus seeded random arguments of the domains
oracle/libm_check.cpp draws from.  Imports neither the product nor a device.

  in_domain(fn)      -> {name: (a, b)}            every element inside the routine's documented domain: restated must be 1
  out_of_domain(fn)  -> {name: (a, b, restated)}  the expected flag spelled out per element, from the documented domain
  composition(fn)    -> {name: (a, b)}            arguments on which the function is promised bit for bit

b is None for the one-argument functions.  No set holds more than 2^20 elements."""
import functools

import numpy as np

F32, F64 = np.float32, np.float64
N_RANDOM = 1 << 18
RAW_FNS = ("logf", "powf", "expf", "log1pf", "exp", "log", "log10", "log1p")


def f32_bits(bits):
    return np.asarray(bits, np.int64).astype(np.uint32).view(F32)


def f64_bits(bits):
    return np.asarray(bits, np.uint64).view(F64)


def around(x, k, dtype):
    """every x[i] and its k neighbours on either side (nextafter: crosses zero into the other sign's subnormals)"""
    x = np.atleast_1d(np.asarray(x, dtype))
    out = [x]
    lo = hi = x
    for _ in range(k):
        with np.errstate(over="ignore"):  # (past the largest finite number lies inf: wanted)
            lo = np.nextafter(lo, dtype(-np.inf))
            hi = np.nextafter(hi, dtype(np.inf))
        out += [lo, hi]
    return np.concatenate(out)


def cross(x, y):
    """every pair (x[i], y[j])"""
    return np.repeat(x, len(y)), np.tile(y, len(x))


def _words(n, seed):
    """n 64-bit words of numpy's generator for `seed` (an int, so that the suite's seed shift applies)"""
    return np.random.default_rng(seed).integers(0, 1 << 63, n, dtype=np.int64).astype(np.uint64)


# ---------------------------------------------------------------------------------------------------------------- float routines

def logf_edges():
    """0x3f330000 + (j << 19) + (k << 23) + d: the 16 table sub-intervals' edges, d in -2..2, at every exponent of a positive normal float"""
    j, k, d = np.meshgrid(np.arange(16, dtype=np.int64), np.arange(-127, 129, dtype=np.int64), np.arange(-2, 3, dtype=np.int64), indexing="ij")
    bits = (0x3f330000 + (j << 19) + (k << 23) + d).ravel()
    bits = bits[(bits >= 0x00800000) & (bits < 0x7f800000)]
    return f32_bits(bits)


def qscore_eprobs():
    """float(10^(-q/10)) +- 3 ulp, q = 0..93"""
    return around(np.power(10.0, -np.arange(94) / 10.0).astype(F32), 3, F32)


POWF_Y = np.array([1, 0.25, 0.5, 0.75, 0.35, 0.6, np.nextafter(F32(1), F32(0)), np.nextafter(F32(1), F32(2)), np.nextafter(F32(0.25), F32(1)),
                   2.0 ** -20, 2, -1, -0.25], F32)
EXPF_UNDERFLOW = f32_bits([0xc2cff1b4])  # -0x1.9fe368p6f: below it expf is +0


def _random_f32(fn):
    r = _words(N_RANDOM, {"logf": 101, "powf": 102, "expf": 103, "log1pf": 104}[fn])
    odd = (np.arange(N_RANDOM) & 1) == 1
    if fn == "logf":  # 2^-25 .. 1
        return f32_bits(0x33000000 + ((r >> np.uint64(8)) % np.uint64(0x0c800000)).astype(np.int64)), None
    if fn == "powf":  # error probabilities of q-scores 3..70 (and neighbouring floats), exponents in (0, 1]
        q = 3 + (r % np.uint64(68)).astype(np.int64)
        e = np.power(10.0, -0.1 * q).astype(F32)
        e = np.where(odd, f32_bits(e.view(np.uint32).astype(np.int64) + ((r >> np.uint64(20)) % np.uint64(2048)).astype(np.int64)), e)
        v = (((r >> np.uint64(32)) % np.uint64(1000000)).astype(F64) / 1000000.0).astype(F32)
        return e, np.where(v <= 0, F32(0.25), v)
    if fn == "expf":  # (-110, 0], dense near 0
        x = -((r % np.uint64(11000000)).astype(F64) / 100000.0).astype(F32)
        return np.where(odd, -(((r >> np.uint64(8)) % np.uint64(1000000)).astype(F64) / 1.0e8).astype(F32), x), None
    # log1pf: ~1e-19 .. 0.01 and 0.01 .. 0.41
    lo = 0x20000000 + ((r >> np.uint64(16)) % np.uint64(0x3c23d70a - 0x20000000)).astype(np.int64)
    hi = 0x3c23d70a + ((r >> np.uint64(16)) % np.uint64(0x3ed413d7 - 0x3c23d70a)).astype(np.int64)
    return f32_bits(np.where((np.arange(N_RANDOM) & 2) != 0, lo, hi)), None


def _log1pf_thresholds():
    return around(f32_bits([0x24800000, 0x31000000, 0x3c23d70a, 0x3ed413d7, 0x00800000, 0x00000001]), 3, F32)


# --------------------------------------------------------------------------------------------------------------- double routines

EXP_POINTS = np.array([-512, -708.3964185322641, -745.1332191019411, -1024, 2.0 ** -54, -2.0 ** -54, 2.0 ** -1022, -2.0 ** -1022, 0.0, -0.0, 512,
                       -600, -700, -720, -740, -750, -800, -1000], F64)


def exp_index_boundaries():
    """(k + h/2) ln2/128 +- 1 ulp: both rounding boundaries of the table index, from -745 to +510; every third k (3 and 128 have
    no common factor: every table entry is met)"""
    ln2_128 = np.log(2.0) / 128
    k = np.arange(int(np.floor(-745.2 / ln2_128)), int(np.ceil(510 / ln2_128)) + 3, 3, dtype=np.int64).astype(F64)  # (past the underflow cut-off)
    x = np.concatenate([k * ln2_128, (k + 0.5) * ln2_128])
    return around(x, 1, F64)


def log_edges():
    """0x3fe6000000000000 + (j << 45) + (k << 52) + d: the 128 table sub-intervals' edges, d in -1..1; every third exponent of a
    positive normal double, and k = -1, 0, 1 whole"""
    ks = np.unique(np.concatenate([np.arange(-1021, 1025, 3, dtype=np.int64), np.array([-1, 0, 1], np.int64)]))
    j, k, d = np.meshgrid(np.arange(128, dtype=np.int64), ks, np.arange(-1, 2, dtype=np.int64), indexing="ij")
    bits = (0x3fe6000000000000 + (j << 45) + (k << 52) + d).ravel()
    bits = bits[(bits >= 0x0010000000000000) & (bits < 0x7ff0000000000000)]
    return f64_bits(bits.astype(np.uint64))


LOG_POINTS = np.array([1 - 2.0 ** -4, 1 + float.fromhex("0x1.09p-4"), 1, 0.5, 2, 10], F64)
DBL_MIN_NORMAL, DBL_MAX = np.finfo(F64).tiny, np.finfo(F64).max
LOG1P_LIMIT = f64_bits([0x3FDA827A << 32])[0]  # the routine's upper end: the high word of sqrt(2) - 1


def _random_f64(fn):
    r = _words(N_RANDOM, {"exp": 105, "log": 106, "log10": 106, "log1p": 107}[fn])
    it = np.arange(N_RANDOM)
    r8 = (r >> np.uint64(8)) % np.uint64(1000000)
    if fn == "exp":  # (-760, 0] incl. the subnormal-result range, dense near 0, tiny, and a few positive
        x = -(r % np.uint64(760000000)).astype(F64) / 1.0e6
        x = np.where((it & 3) == 1, -r8.astype(F64) / 1.0e9, x)
        x = np.where((it & 3) == 2, r8.astype(F64) / 1.0e4, x)
        return np.where((it & 7) == 7, -r8.astype(F64) * 2.0 ** -70, x)
    if fn in ("log", "log10"):  # the range close to 1, and all positive normal magnitudes
        near = 0.9375 + (r % np.uint64(12720000)).astype(F64) / 1.0e8
        return np.where((it & 1) == 1, near, f64_bits(np.uint64(0x0010000000000000) + r % np.uint64(0x7fe0000000000000)))
    # log1p: [0, 0.01) as log1p_switch uses it, and up to 0.41
    small = (r % np.uint64(1000000000)).astype(F64) / 1.0e11
    wide = f64_bits(np.uint64(0x3c00000000000000) + r % np.uint64(0x3fda827a00000000 - 0x3c00000000000000))
    return np.where((it & 1) == 1, small, wide)


def _log1p_thresholds():
    return around(np.concatenate([f64_bits(np.array([0x3c900000, 0x3e200000, 0x3FDA827A], np.uint64) << np.uint64(32)), [0.01, DBL_MIN_NORMAL]]), 3, F64)


# ------------------------------------------------------------------------------------------------------------------- the raw sets

@functools.lru_cache(maxsize=None)
def in_domain(fn):
    """{name: (a, b)} for one of RAW_FNS: every element inside the documented domain"""
    if fn == "logf":  # x a positive normal float
        sets = {"table_edges": logf_edges(), "one": around(F32(1), 2, F32), "ends": f32_bits([0x00800000, 0x7f7fffff]), "random": _random_f32(fn)[0]}
    elif fn == "powf":  # x a positive normal float, y finite and not zero, |y log2 x| < 126
        e = logf_edges()
        sets = {"table_edges": cross(e[(e > F32(1e-12)) & (e <= F32(1))], POWF_Y), "qscores": cross(qscore_eprobs(), POWF_Y), "random": _random_f32(fn)}
        return sets
    elif fn == "expf":  # x <= 88, -inf included
        ln2_32 = np.log(2.0) / 32
        k = np.arange(4901, dtype=F64)
        sets = {"index_boundaries": around(np.concatenate([-k * ln2_32, -(k + 0.5) * ln2_32]).astype(F32), 2, F32),
                "points": np.concatenate([f32_bits([0x00000000, 0x80000000, 0xff800000]), around(EXPF_UNDERFLOW, 3, F32),
                                          f32_bits(0x42b00000 - np.arange(4))]),  # 88.0f and the three floats below it
                "random": _random_f32(fn)[0]}
    elif fn == "log1pf":  # 0 <= x < 0.41422 (bits below 0x3ed413d7)
        t = _log1pf_thresholds()
        sets = {"thresholds": np.concatenate([t[(t.view(np.uint32) < 0x3ed413d7)], f32_bits([0])]), "random": _random_f32(fn)[0]}
    elif fn == "exp":  # x < 512, -inf included
        p = around(EXP_POINTS, 3, F64)
        sets = {"index_boundaries": exp_index_boundaries(), "points": np.concatenate([p[p < 512], [-np.inf]]), "random": _random_f64(fn)}
    elif fn in ("log", "log10"):  # x a positive normal double
        p = around(np.concatenate([LOG_POINTS, [DBL_MIN_NORMAL, DBL_MAX]]), 3, F64)
        sets = {"table_edges": log_edges(), "points": p[(p >= DBL_MIN_NORMAL) & np.isfinite(p)],
                "powers_of_ten": np.array([float("1e%d" % e) for e in range(-307, 309)], F64), "random": _random_f64(fn)}
    elif fn == "log1p":  # 0 <= x < 0.41422 (high word below 0x3FDA827A)
        t = _log1p_thresholds()
        sets = {"thresholds": np.concatenate([t[t < LOG1P_LIMIT], [0.0]]), "random": _random_f64(fn)}
    else:
        raise KeyError(fn)
    return {name: (a, None) for name, a in sets.items()}


def _flags(a, ok):
    return np.ascontiguousarray(np.broadcast_to(np.asarray(ok, bool), np.shape(a))).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def out_of_domain(fn):
    """{name: (a, b, restated)} for one of RAW_FNS: the expected flag of every element, written down from the documented domain"""
    nan, inf = np.nan, np.inf
    if fn == "logf":  # anything but a positive normal float is refused
        a = np.concatenate([np.array([nan, inf, -inf, 0.0, -0.0, -1.5], F32), f32_bits([0x00000001, 0x00400000, 0x007fffff, 0x807fffff])])
        return {"specials_and_subnormals": (a, None, _flags(a, 0))}
    if fn in ("log", "log10"):
        a = np.concatenate([np.array([nan, inf, -inf, 0.0, -0.0, -1.5], F64), f64_bits([1, 0x0008000000000000, 0x000fffffffffffff, 0x800fffffffffffff]),
                            around(DBL_MIN_NORMAL, 3, F64), around(DBL_MAX, 3, F64)])
        ok = (a >= DBL_MIN_NORMAL) & (a <= DBL_MAX)  # the neighbours below the smallest normal and above the largest finite are refused
        return {"specials_and_subnormals": (a, None, _flags(a, ok))}
    if fn == "expf":  # above 88 the routine leaves the overflow range to the caller
        r = np.random.default_rng(111)
        a = np.concatenate([np.nextafter(F32(88), F32(100), dtype=F32).reshape(1), r.uniform(88.0, 88.72, 4096).astype(F32), np.array([88.72], F32)])
        s = np.array([nan, inf, -inf], F32)
        return {"overflow_range": (a, None, _flags(a, 0)), "specials": (s, None, np.array([0, 0, 1], np.uint8))}  # (-inf underflows to +0: taken)
    if fn == "exp":
        r = np.random.default_rng(112)
        a = np.concatenate([around(F64(512), 3, F64), r.uniform(512.0, 709.78, 4096), [709.78]])
        s = np.array([nan, inf, -inf], F64)
        return {"overflow_range": (a, None, _flags(a, a < 512)), "specials": (s, None, np.array([0, 0, 1], np.uint8))}
    if fn == "log1pf":  # [0, 0.41422) only; -0 carries the sign bit and is refused with the negative numbers
        r = np.random.default_rng(113)
        t = _log1pf_thresholds()
        a = np.concatenate([t[t.view(np.uint32) >= 0x3ed413d7], r.uniform(0.41422, 1.0, 4096).astype(F32), np.array([1.0], F32)])
        s = np.array([nan, inf, -inf, -0.0, -0.25, 0.0], F32)
        return {"upper_range_and_negative_neighbours": (a, None, _flags(a, 0)), "specials": (s, None, np.array([0, 0, 0, 0, 0, 1], np.uint8))}
    if fn == "log1p":
        r = np.random.default_rng(114)
        t = _log1p_thresholds()
        a = np.concatenate([t[t >= LOG1P_LIMIT], r.uniform(0.41422, 1.0, 4096), [1.0]])
        s = np.array([nan, inf, -inf, -0.0, -0.25, 0.0], F64)
        return {"upper_range": (a, None, _flags(a, 0)), "specials": (s, None, np.array([0, 0, 0, 0, 0, 1], np.uint8))}
    if fn == "powf":
        # |y log2 x| against 126: x a power of two makes log2 x exact, so the product is y's neighbour times an integer, exactly
        y126 = around(F32(126), 2, F32)
        x = np.concatenate([np.full(5, 0.5, F32), np.full(5, 2.0, F32), np.full(5, 0.5, F32), np.full(5, 0.25, F32)])
        y = np.concatenate([y126, y126, -y126, around(F32(63), 2, F32)])
        ok = np.abs(y.astype(F64) * np.log2(x.astype(F64))) < 126
        sx = np.array([nan, inf, -inf, 0.0, -0.0, -2.0, 0.5, 0.5, 0.5, 0.5, 0.5], F32)
        sy = np.array([0.5, 0.5, 0.5, 0.5, 0.5, 0.5, 0.0, -0.0, inf, -inf, nan], F32)
        sub = f32_bits([0x00000001, 0x007fffff])
        return {"around_126": (x, y, _flags(x, ok)), "specials": (sx, sy, _flags(sx, 0)), "subnormal_x": (sub, np.full(2, 0.5, F32), _flags(sub, 0))}
    raise KeyError(fn)


# ------------------------------------------------------------------------------------------------------------- the compositions

LN_0_01 = np.log(0.01)  # exp(d) crosses log1p_switch's 0.01 at this difference


def _log_sum_pairs(dtype, seed):
    """pairs for getLogSum: differences around the switch, 0, the underflow cut-offs, -inf operands, equal operands, random pairs"""
    t = dtype
    if t is F32:
        cuts = np.concatenate([around(F32(LN_0_01), 2, F32), around(EXPF_UNDERFLOW, 2, F32), around(F32(-87.33654), 2, F32), [F32(0)]]).astype(F32)
        wide = 110.0
    else:
        cuts = np.concatenate([around(F64(LN_0_01), 2, F64), around(F64(-745.1332191019411), 2, F64), around(F64(-708.3964185322641), 2, F64),
                               around(F64(-1024), 2, F64), around(F32(LN_0_01).astype(F64), 2, F64), [0.0]])
        wide = 760.0
    base = np.array([0.0, -2.0 ** -7, -4.0, -1000.0, -2999.5], t)  # (next to a small term the sum keeps the log's low bits)
    x1, d = cross(base, cuts)
    a = [x1, x1 + d]  # (the larger term first and second: getLogSum orders them itself)
    b = [x1 + d, x1]
    ninf = t(-np.inf)
    a.append(np.array([-3.5, ninf, ninf, -12.25, -12.25, 0.0], t))
    b.append(np.array([ninf, -3.5, ninf, -12.25, np.nextafter(t(-12.25), t(0)), 0.0], t))
    r = np.random.default_rng(seed)
    n = 1 << 16
    u1 = -r.uniform(0.0, 3000.0, n)  # log-likelihood size, (-3000, 0]
    u1 = np.where(np.arange(n) % 4 == 2, u1 / 3000.0, u1)  # a quarter in (-1, 0]: the sum then shows the log's last bits
    u2 = np.where(np.arange(n) & 1, -r.uniform(0.0, 3000.0, n), u1 - r.uniform(0.0, wide, n))  # every other pair close enough for a non-zero exp
    a.append(u1.astype(t))
    b.append(np.maximum(u2, -2999.999).astype(t))
    return np.concatenate(a).astype(t), np.concatenate(b).astype(t)


def phred_boundary_probs():
    """10^(-(q + 0.5)/10), q = 0..400: where the rounded phred value changes"""
    return np.power(10.0, -(np.arange(401) + 0.5) / 10.0)


@functools.lru_cache(maxsize=None)
def composition(fn):
    """{name: (a, b)} on which the kernels' scalar functions are promised bit for bit (exact_libm on)"""
    if fn in ("sk_exp", "sk_log", "sk_log10", "sk_log1p"):
        return in_domain(fn[3:])
    if fn == "logf_ref":
        return in_domain("logf")
    if fn == "log_sum2f":
        return {"pairs": _log_sum_pairs(F32, 121)}
    if fn == "log_sum2":
        return {"pairs": _log_sum_pairs(F64, 122)}
    if fn == "log1p_switch_d":  # the argument is an exp() of a difference <= 0: [0, 1]
        r = np.random.default_rng(123)
        x = np.concatenate([around(F64(0.01), 2, F64), around(F32(0.01).astype(F64), 2, F64), [0.0, 1.0, DBL_MIN_NORMAL, 5e-324],
                            r.uniform(0.0, 1.0, 1 << 15), np.exp(-r.uniform(0.0, 745.0, 1 << 15))])
        return {"zero_to_one": (x, None)}
    if fn == "qphred_d":
        p = around(phred_boundary_probs(), 2, F64)
        return {"phred_boundaries": (p, None), "ends": (np.array([0.0, 5e-324, DBL_MIN_NORMAL, 1.0], F64), None)}
    if fn == "ln_qphred_f":  # the argument is ln(prob), a float
        lnp = around((np.log(10.0) * -(np.arange(401) + 0.5) / 10.0).astype(F32), 2, F32)
        with np.errstate(divide="ignore"):
            ends = np.log(np.array([0.0, np.finfo(F32).smallest_subnormal, np.finfo(F32).tiny, 1.0], F64)).astype(F32)
        return {"phred_boundaries": (lnp, None), "ends": (ends, None)}
    if fn == "dependent_eprob":
        return {"qscores": cross(qscore_eprobs(), np.array([0.25, 0.35, 0.6, 1, 0], F32))}
    raise KeyError(fn)


COMPOSITION_FNS = ("sk_exp", "sk_log", "sk_log10", "sk_log1p", "logf_ref", "dependent_eprob", "ln_qphred_f", "qphred_d", "log1p_switch_d", "log_sum2",
                   "log_sum2f")
