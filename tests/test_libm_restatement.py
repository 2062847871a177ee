"""csrc/libm_flt32.h and libm_dbl64.h restate eight routines of the host C library (glibc >= 2.28: powf, logf, expf, log1pf, exp, log,
log10, log1p) so that the device reproduces the reference's libm calls bit for bit.  The headers are compiled for the host here and
compared with the host libm: on 10^7 pseudo-random arguments (oracle/libm_check.cpp), and on the deterministic edge sets of
tests/libm_cases.py (oracle/libm_header_eval.cpp), which also checks where each routine declines.  The device's evaluation of the same
headers, on the same sets, is checked by tests/test_libm_device.py."""
import os
import subprocess

import numpy as np
import pytest

from oracle import pyoracle
from tests import libm_cases as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_restatement_matches_host_libm(tmp_path):
    exe = str(tmp_path / "libm_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-o", exe, os.path.join(ROOT, "oracle", "libm_check.cpp"), "-lm"],
                   check=True)
    out = subprocess.run([exe, "10000000"], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout
    assert "powf mismatches 0 logf mismatches 0 expf mismatches 0 log1pf mismatches 0 fallbacks 0" in out.stdout


def bits(x):
    return np.ascontiguousarray(x).view({4: np.uint32, 8: np.uint64}[x.dtype.itemsize])


def describe(a, b, want, got, where, limit=6):
    """the first few differing elements: arguments and both results, as hex bit patterns"""
    lines = []
    for i in where[:limit]:
        arg = "%#x" % bits(a)[i] + ("" if b is None else ", %#x" % bits(b)[i])
        lines.append("  [%d] arg %s (%r): want %#x got %#x" % (i, arg, a[i] if b is None else (a[i], b[i]), bits(want)[i], bits(got)[i]))
    return "\n".join(lines)


@pytest.mark.parametrize("fn", K.RAW_FNS)
def test_header_on_host_equals_host_libm_on_the_case_sets(built, fn):
    """every in-domain set: the header compiled for the host returns the host libm's bits and never declines"""
    for name, (a, b) in K.in_domain(fn).items():
        assert 0 < len(a) <= 1 << 20, (fn, name)
        want = pyoracle.libm_eval(fn, a, b)
        got, restated = pyoracle.libm_header_eval(fn, a, b)
        assert np.all(restated == 1), "%s/%s: declined at\n%s" % (fn, name, describe(a, b, want, got, np.flatnonzero(restated != 1)))
        bad = np.flatnonzero(bits(want) != bits(got))
        assert len(bad) == 0, "%s/%s: %d of %d differ\n%s" % (fn, name, len(bad), len(a), describe(a, b, want, got, bad))


@pytest.mark.parametrize("fn", K.RAW_FNS)
def test_header_declines_exactly_outside_its_documented_domain(built, fn):
    """the out-of-domain sets: `restated` is what libm_cases.py writes down from each routine's documented domain; where the routine
    does take an element, its result is the host libm's"""
    for name, (a, b, expect) in K.out_of_domain(fn).items():
        want = pyoracle.libm_eval(fn, a, b)
        got, restated = pyoracle.libm_header_eval(fn, a, b)
        wrong = np.flatnonzero(restated != expect)
        assert len(wrong) == 0, "%s/%s: flag differs at\n%s" % (fn, name, describe(a, b, want, got, wrong))
        assert np.all(bits(got)[expect == 0] == 0), (fn, name)  # (declined: zero bits)
        bad = np.flatnonzero((expect == 1) & (bits(want) != bits(got)))
        assert len(bad) == 0, "%s/%s:\n%s" % (fn, name, describe(a, b, want, got, bad))


def test_case_sets_hold_what_they_say():
    """the sets are built from bit patterns: a slip there would quietly test less"""
    e = K.logf_edges()
    assert 0x3f330000 in bits(e) and 0x3f32fffe in bits(e) and (0x3f330000 + (15 << 19) + 2) in bits(e)
    assert e.min() < 2.0 ** -125 and e.max() > 2.0 ** 127 and np.all(np.isfinite(e)) and len(e) > 16 * 250 * 5  # both end exponents
    x = K.in_domain("expf")["index_boundaries"][0]
    assert x.min() < -104 and np.sum((x > -103.97) & (x < -87.34)) > 5000  # the whole subnormal-result range
    x = K.in_domain("exp")["index_boundaries"][0]
    assert x.min() < -745 and x.max() > 509 and len(x) <= 1 << 20
    le = K.log_edges()
    for k in (-1, 0, 1):
        assert np.uint64(0x3fe6000000000000 + (127 << 45) + (k << 52) + 1) in bits(le)
    assert le.min() < 1e-307 and le.max() > 1e307
    a, b = K.composition("log_sum2f")["pairs"]
    assert np.isneginf(a).sum() >= 2 and np.isneginf(b).sum() >= 2 and np.sum(a == b) >= 2
    both = np.isfinite(a) & np.isfinite(b)
    d = np.minimum(a[both], b[both]) - np.maximum(a[both], b[both])
    assert np.float32(np.log(0.01)) in d and np.float32(0) in d
