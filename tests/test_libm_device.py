"""The device's evaluation of the restated libm routines (csrc/libm_flt32.h, libm_dbl64.h), asked directly: these bits in -- which
bits does the MI355X return, and did it take the restated path?  sk_debug_libm_eval evaluates each routine, and each scalar function
the kernels build on them (the sk_* wrappers and their out-of-line twins, logf_ref, get_dependent_eprob, the q-score conversions, the
log-sums), one element per thread; the expected values are the HOST C library's (oracle: sko_libm_eval), the expected `restated` flags
those of the same headers compiled for the host (sko_libm_header_eval).  The arguments are tests/libm_cases.py's: table-interval
edges, index rounding boundaries, subnormal results, branch thresholds, seeded random draws; tests/test_libm_restatement.py shows on
the CPU that the host-compiled headers agree with the host libm on all of them, so zero mismatches is a bar the restatement meets.

What can only go wrong on the device and is seen here: float(double) into the float-subnormal range, float and double division in
log1pf / log1p, contraction of the unfused routines, the constant-memory tables and their LDS copy, the __noinline__ twins, and the
glue of the compositions (operand order, the 0.01 switch, the -37 / -307 clamps).

Outside the restated domain, and on a host whose libm is not the restated one (sk_debug_force_device_libm), the device library stands
in: special values exactly, everything else to the documented relative 1e-5.  A subnormal expected value has a spacing of its own
(2^-1074, 2^-149) that no relative bound can go below: there the bound is max(1e-5 |want|, one spacing), which is what two
correctly-working exp routines that round differently need; only the stand-in of sk_exp reaches such results (x < -708; through it,
log_sum2 of 0 and a term that far below)."""
import functools

import numpy as np
import pytest

from oracle import pyoracle
from tests import libm_cases as K

pytestmark = pytest.mark.gpu

TABLE_FNS = ("exp", "log", "log10", "sk_exp", "sk_log", "sk_log10", "qphred_d", "log1p_switch_d", "log_sum2")  # take SkLibmTables: variants 0, 1
TWIN_FNS = ("sk_exp", "sk_log", "sk_log10", "qphred_d")                                                       # variant 2 as well
RAW_OF = {"sk_exp": "exp", "sk_log": "log", "sk_log10": "log10", "sk_log1p": "log1p", "logf_ref": "logf"}
BAR = 1e-5  # include/strelka_amd.h (sk_libm_restated), tests/test_limits.py


def variants(fn):
    return (0,) + ((1,) if fn in TABLE_FNS else ()) + ((2,) if fn in TWIN_FNS else ())


def bits(x):
    return np.ascontiguousarray(x).view({4: np.uint32, 8: np.uint64}[x.dtype.itemsize])


def differing(want, got):
    """indices where the results differ: bit patterns, except that NaN equals NaN whatever its payload"""
    if want.dtype.kind == "f":
        return np.flatnonzero((bits(want) != bits(got)) & ~(np.isnan(want) & np.isnan(got)))
    return np.flatnonzero(want != got)


def describe(a, b, want, got, where, limit=6):
    lines = []
    for i in where[:limit]:
        arg = "%#x" % bits(a)[i] + ("" if b is None else ", %#x" % bits(b)[i])
        w, g = (bits(want)[i], bits(got)[i]) if want.dtype.kind == "f" else (want[i], got[i])
        lines.append("  [%d] arg %s (%r): host %#x device %#x" % (i, arg, a[i] if b is None else (a[i], b[i]), w, g))
    return "\n".join(lines)


@functools.lru_cache(maxsize=None)
def host(fn, kind, name):
    """the host libm's results for one case set, computed once"""
    a, b = {"in": K.in_domain, "out": K.out_of_domain, "comp": K.composition}[kind](fn)[name][:2]
    want = pyoracle.libm_eval(fn, a, b)
    want.setflags(write=False)
    return want


@functools.lru_cache(maxsize=None)
def header_flags(fn, kind, name):
    a, b = {"in": K.in_domain, "out": K.out_of_domain}[kind](fn)[name][:2]
    return pyoracle.libm_header_eval(fn, a, b)[1]


def check_raw(gpu, fn, variant):
    for name, (a, b) in K.in_domain(fn).items():
        want = host(fn, "in", name)
        got, restated = gpu.debug_libm_eval(fn, a, b, variant)
        declined = np.flatnonzero(restated != header_flags(fn, "in", name))
        assert len(declined) == 0, "%s/%s variant %d: restated flag differs at\n%s" % (fn, name, variant, describe(a, b, want, got, declined))
        bad = differing(want, got)
        print("%s/%s variant %d: %d elements, %d mismatches" % (fn, name, variant, len(a), len(bad)))
        assert len(bad) == 0, "%s/%s variant %d: %d of %d differ from the host libm\n%s" % (fn, name, variant, len(bad), len(a),
                                                                                           describe(a, b, want, got, bad))
    for name, (a, b, _) in K.out_of_domain(fn).items():
        want = host(fn, "out", name)
        flags = header_flags(fn, "out", name)
        got, restated = gpu.debug_libm_eval(fn, a, b, variant)
        wrong = np.flatnonzero(restated != flags)
        assert len(wrong) == 0, "%s/%s variant %d: restated flag differs at\n%s" % (fn, name, variant, describe(a, b, want, got, wrong))
        assert np.all(bits(got)[flags == 0] == 0), (fn, name)
        bad = differing(want[flags == 1], got[flags == 1])
        assert len(bad) == 0, (fn, name, variant, bad[:6])


@pytest.mark.parametrize("fn,variant", [(fn, v) for fn in K.RAW_FNS for v in variants(fn)])
def test_raw_routines_return_the_host_libms_bits(gpu, fn, variant):
    """case 1: zero mismatches on every in-domain set, and the routine takes and declines exactly what it does on the host"""
    check_raw(gpu, fn, variant)


@pytest.mark.parametrize("fn,variant", [(fn, v) for fn in K.COMPOSITION_FNS for v in variants(fn)])
def test_what_the_kernels_call_is_bit_for_bit(gpu, fn, variant):
    """case 2: the wrappers and compositions with exact_libm on, from constant-memory tables, the LDS copy and the out-of-line twins"""
    assert gpu.lib().sk_libm_restated() == 1
    for name, (a, b) in K.composition(fn).items():
        want = host(fn, "comp", name)
        got, _ = gpu.debug_libm_eval(fn, a, b, variant)
        bad = differing(want, got)
        print("%s/%s variant %d: %d elements, %d mismatches" % (fn, name, variant, len(a), len(bad)))
        assert len(bad) == 0, "%s/%s variant %d: %d of %d differ from the oracle\n%s" % (fn, name, variant, len(bad), len(a),
                                                                                       describe(a, b, want, got, bad))


def is_special(want):
    return ~np.isfinite(want) | (want == 0) | (want == 1)


def check_stand_in(label, a, b, want, got):
    """special values exactly, everything else within the documented bar; returns the largest relative difference"""
    sp = is_special(want)
    bad = differing(want[sp], got[sp])
    assert len(bad) == 0, "%s: special values differ\n%s" % (label, describe(a[sp], None if b is None else b[sp], want[sp], got[sp], bad))
    w, g = want[~sp].astype(np.float64), got[~sp].astype(np.float64)
    if len(w) == 0:
        return 0.0
    fi = np.finfo(want.dtype)
    spacing = np.where(np.abs(w) < float(fi.tiny), float(fi.smallest_subnormal), 0.0)  # (docstring: subnormal expected values)
    diff = np.abs(g - w)
    rel = diff / np.abs(w)
    normal = spacing == 0
    worst = float(rel[normal].max()) if normal.any() else 0.0
    print("%s: %d finite elements, largest relative difference %.3g (normal results)" % (label, len(w), worst))
    over = np.flatnonzero(~(diff <= np.maximum(BAR * np.abs(w), spacing)))
    assert len(over) == 0, "%s: %d beyond relative %g, first want %r got %r" % (label, len(over), BAR, w[over[0]], g[over[0]])
    return worst


@pytest.mark.parametrize("fn", sorted(RAW_OF))
def test_outside_the_restated_domain_the_device_library_keeps_the_bar(gpu, fn):
    """case 3: what the wrapper returns where the restated routine declines"""
    assert gpu.lib().sk_libm_restated() == 1
    raw = RAW_OF[fn]
    for name, (a, b, _) in K.out_of_domain(raw).items():
        want = host(raw, "out", name)
        for v in variants(fn):
            got, _ = gpu.debug_libm_eval(fn, a, b, v)
            check_stand_in("%s/%s variant %d" % (fn, name, v), a, b, want, got)


def test_log1p_switch_below_zero_keeps_the_bar(gpu):
    """log1p_switch_d on (-0.01, 0): log1p_glibc declines negative arguments, the device library's log1p stands in"""
    x = -np.random.default_rng(131).uniform(1e-12, 0.0099, 4096)
    want = pyoracle.libm_eval("log1p_switch_d", x)
    got, _ = gpu.debug_libm_eval("log1p_switch_d", x)
    check_stand_in("log1p_switch_d/negative", x, None, want, got)


STAND_IN_SETS = [("sk_exp", "in", "exp", "random"), ("sk_log", "in", "log", "random"), ("sk_log10", "in", "log10", "random"),
                 ("sk_log1p", "in", "log1p", "random"), ("logf_ref", "in", "logf", "random"), ("dependent_eprob", "in", "powf", "random"),
                 ("log_sum2", "comp", "log_sum2", "pairs"), ("log_sum2f", "comp", "log_sum2f", "pairs"),
                 ("log1p_switch_d", "comp", "log1p_switch_d", "zero_to_one")]


def test_forced_stand_in_keeps_the_bar_and_goes_away_again(gpu):
    """case 4: sk_debug_force_device_libm(1) makes the wrappers evaluate the device library; the raw routines do not look at it"""
    L = gpu.lib()
    oa, ob, oflags = K.out_of_domain("logf")["specials_and_subnormals"]
    ia, _ = K.in_domain("logf")["one"]
    assert L.sk_debug_force_device_libm(1) == 0
    try:
        assert L.sk_libm_restated() == 0
        for fn, kind, src, name in STAND_IN_SETS:
            a, b = (K.in_domain if kind == "in" else K.composition)(src)[name]
            want = pyoracle.libm_eval(fn, a, b)
            got, _ = gpu.debug_libm_eval(fn, a, b)
            check_stand_in("forced %s/%s" % (fn, name), a, b, want, got)
        assert np.array_equal(gpu.debug_libm_eval("logf", oa)[1], oflags)
        assert np.all(gpu.debug_libm_eval("logf", ia)[1] == 1)
    finally:
        L.sk_debug_force_device_libm(0)
    assert L.sk_libm_restated() == 1
    check_raw(gpu, "logf", 0)


def test_launch_shapes(gpu):
    """case 5: the grid-stride loop and the staging are not where a mismatch comes from: n around a wave, a block, and above a whole
    grid's worth of threads (1024 blocks of 256), through log with the LDS tables"""
    x = np.concatenate([K.in_domain("log")["random"][0], K.in_domain("log")["table_edges"][0][:1000]])
    want = pyoracle.libm_eval("log", x)
    for n in (1, 63, 64, 65, 257, 1024 * 256 + 77):
        assert n <= len(x)
        got, restated = gpu.debug_libm_eval("log", x[:n], None, 1)
        assert len(differing(want[:n], got)) == 0 and np.all(restated == 1), n
    # n = 0 returns 0 and touches nothing
    out = np.full(4, 7.0)
    flags = np.full(4, 9, np.uint8)
    assert gpu.lib().sk_debug_libm_eval(5, 1, 0, gpu._p(x), None, gpu._p(out), gpu._p(flags)) == 0
    assert np.all(out == 7.0) and np.all(flags == 9)


def test_pairs_that_do_not_exist_are_refused(gpu):
    x = np.ones(4, np.float32)
    for fn, v in (("logf", 1), ("log1p", 1), ("exp", 2), ("log_sum2f", 1), ("log_sum2", 2), ("sk_exp", 3)):
        with pytest.raises(ValueError, match="variant"):
            gpu.debug_libm_eval(fn, x, x if fn in pyoracle.LIBM_TWO_ARG_FNS else None, v)
    assert gpu.lib().sk_debug_libm_eval(99, 0, 4, gpu._p(x), None, gpu._p(x), None) == -1
