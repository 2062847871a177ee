"""libstdc++'s std::sort at the inputs random pileups never give it: lopsided partitions down to introsort's depth limit, the heap-sort
fallback, ties throughout.  adjust_joint_eprob hands the decaying exponents out in the order std::sort leaves equal qualities, and the
project restates that order four times (oracle/strelka_oracle.c; std_sort_emulated in csrc/germline_common.h, used by G1 and by the
fused kernels' global pass; k_top_ranked in csrc/germline_fused.hip, which follows the leftmost chain of partitions only and declines
a group when the depth limit runs out there).

tests/golden/sort_adversary.npz (tests/golden/make_sort_adversary.py) holds key sequences made by an adversary for the genuine std::sort
(oracle/sort_probe.cpp) and the order the genuine std::sort left them in.

  CPU  the oracle's restatement against the fixture and, where the probe library is built, against the live std::sort on fresh
       adversaries of every size 17..511; conditions that keep the fixture informative
  GPU  every case whose keys are qualities a basecall can hold (6 bits: 3..63) as one (strand, base) group of a pileup locus -- alone,
       interleaved with other groups, among filtered and q < 3 calls, with neighbouring-mismatch flags, and in a locus deeper than
       the LDS path takes -- through sk_dependent_eprob and both fused kernels, against the oracle bit for bit

The fixture as committed (test_fixture_stays_informative prints the counts): 80 cases, 35 of which reach the heap fallback; 26 of
those have ties and an order different from a stable descending sort, 21 of them within the first four entries; the smallest fallback
case has n = 36 (mirrored; n = 37 plain).  Plain cases of n >= 512 reach the fallback too: (1023, 17) and (2000, 33)."""
import functools
import os

import numpy as np
import pytest

from oracle import pyoracle
from strelka_amd import capi

HERE = os.path.dirname(os.path.abspath(__file__))
Q_MAX = 63             # a basecall's quality field is 6 bits wide (include/strelka_amd.h, SK_CALL_Q)
MAX_PACKED_DEPTH = 511  # csrc/germline_fused.hip:50 -- deeper loci go straight to the global pass

OPTION_SETS = {
    "defaults": {},
    "every_rank": dict(is_min_vexp=0),  # no floor: every rank has its own exponent, the whole permutation shows in de
    "more_than_four_ranks": dict(min_vexp=0.05),
    "slow_decay": dict(bsnp_ssd_no_mismatch=0.05, bsnp_ssd_one_mismatch=0.1),
}


@functools.lru_cache(maxsize=None)
def fixture_cases():
    g = np.load(os.path.join(HERE, "golden", "sort_adversary.npz"))
    off = g["off"]
    return [dict(n=int(g["n"][i]), k=int(g["k"][i]), mirror=int(g["mirror"][i]), key=np.ascontiguousarray(g["keys"][off[i]:off[i + 1]]),
                 perm=g["perm"][off[i]:off[i + 1]].astype(np.uint32)) for i in range(len(g["n"]))]


def _stable_desc(key):
    return np.argsort(-key.astype(np.int64), kind="stable").astype(np.uint32)


# ------------------------------------------------------------------------------------------------------------------------ CPU

def test_fixture_holds_the_cases_asked_for():
    have = {(c["n"], c["k"], c["mirror"]) for c in fixture_cases()}
    for n in (17, 33, 36, 37, 40, 48, 64, 68):
        assert (n, 1, 0) in have
    for n in (69, 100, 129, 200, 257, 300, 400, 511, 512, 600, 1023, 1100, 2000):
        k0 = -(-n // 68)  # the smallest divisor that leaves <= 68 distinct keys
        assert {(n, k0, 0), (n, k0 + 1, 0), (n, 2 * k0, 0)} <= have, n
    for c in fixture_cases():
        assert len(c["key"]) == c["n"] == len(c["perm"]) and c["key"].min() == 3
        assert len(np.unique(c["key"])) == -(-c["n"] // c["k"])
        assert np.array_equal(np.sort(c["perm"]), np.arange(c["n"]))


def test_restated_sort_equals_std_sort_on_the_fixture(built):
    for c in fixture_cases():
        assert np.array_equal(pyoracle.sort_idx_by_key_desc(c["key"]), c["perm"]), (c["n"], c["k"], c["mirror"])


def test_fixture_stays_informative(built):
    """the counts are in the module's docstring; the bars are the ones the fixture was asked to meet"""
    fallback = []
    for c in fixture_cases():
        pyoracle.heap_sort_runs_reset()
        pyoracle.sort_idx_by_key_desc(c["key"])
        if pyoracle.heap_sort_runs() > 0:
            fallback.append(c)
    tied = [c for c in fallback if len(np.unique(c["key"])) < c["n"] and not np.array_equal(c["perm"], _stable_desc(c["key"]))]
    early = [c for c in tied if not np.array_equal(c["perm"][:4], _stable_desc(c["key"])[:4])]
    print("cases %d, heap fallback %d, tied and unlike a stable sort %d, within the first four %d, smallest fallback n %d (plain %d)" % (
        len(fixture_cases()), len(fallback), len(tied), len(early), min(c["n"] for c in fallback),
        min(c["n"] for c in fallback if not c["mirror"])))
    assert len(fallback) >= 12
    assert len(tied) >= 4
    assert len(early) >= 2
    assert min(c["n"] for c in fallback) <= 40
    # ... and of the cases a pileup can carry, on both sides of the LDS path's depth limit
    dev = [c for c in fallback if c["key"].max() <= Q_MAX]
    assert sum(c["n"] <= MAX_PACKED_DEPTH for c in dev) >= 12 and sum(c["n"] > MAX_PACKED_DEPTH for c in dev) >= 1
    assert sum(c["mirror"] for c in dev) >= 4 and sum(not c["mirror"] for c in dev) >= 4


def test_restated_sort_equals_live_std_sort_on_fresh_adversaries(built):
    """every size the LDS path can meet, plain and mirrored, every divisor 1..8 that leaves <= 68 distinct keys"""
    assert pyoracle.sort_probe() is not None, "oracle/libsort_probe.so was not built"
    cases = fallback = 0
    for n in range(17, 512):
        for mirror in (False, True):
            for k in range(1, 9):
                if -(-n // k) > 68:
                    continue
                key = pyoracle.sort_adversary_keys(n, k, mirror)
                pyoracle.heap_sort_runs_reset()
                got = pyoracle.sort_idx_by_key_desc(key)
                fallback += pyoracle.heap_sort_runs() > 0
                cases += 1
                assert np.array_equal(got, pyoracle.std_sort_idx_by_key_desc(key)), (n, k, mirror)
    assert cases == 2 * 2287 and fallback >= 179


# ------------------------------------------------------------------------------------------------------------------------ GPU

def _merge(rng, streams):
    """one sequence out of several, each stream's own order kept, the streams interleaved at random"""
    owner = np.repeat(np.arange(len(streams)), [len(s) for s in streams])
    rng.shuffle(owner)
    out = np.zeros(len(owner), np.uint16)
    for i, s in enumerate(streams):
        out[owner == i] = s
    return out


def _other_groups(rng, g, how_many, size):
    """calls of `how_many` (strand, base) groups other than g, `size(rng)` calls each"""
    others = rng.choice([x for x in range(8) if x != g], how_many, replace=False)
    return [capi.make_call(rng.integers(3, Q_MAX + 1, size(rng)), x >> 1, x & 1, rng.random() < 0.3) for x in others]


def _loci_of_case(rng, c, g):
    """the variants of one fixture case: (name, calls of the locus, indices of the adversarial group's calls in the locus)"""
    key, n = c["key"], c["n"]
    base, fwd = g >> 1, g & 1
    plain = capi.make_call(key, base, fwd)
    small = lambda r: int(r.integers(1, 7))
    loci = [("alone", plain)]
    loci.append(("interleaved", _merge(rng, [plain] + _other_groups(rng, g, int(rng.integers(2, 4)), small))))
    # calls of the group's own strand and base that must not enter it: filtered ones of any quality, unfiltered ones below q 3
    n_out = max(3, n // 8)
    outsiders = np.where(rng.random(n_out) < 0.5, capi.make_call(rng.integers(0, Q_MAX + 1, n_out), base, fwd, 0, 1),
                         capi.make_call(rng.integers(0, 3, n_out), base, fwd, 0, 0)).astype(np.uint16)
    loci.append(("outsiders", _merge(rng, [plain, outsiders])))
    nmm = rng.random(n) < 0.3
    nmm[int(rng.integers(0, n))] = True
    loci.append(("pending", capi.make_call(key, base, fwd, nmm)))
    if n <= MAX_PACKED_DEPTH:  # the same group where only the global-memory routines see it
        pad = MAX_PACKED_DEPTH + 1 - n
        loci.append(("deep", _merge(rng, [plain] + _other_groups(rng, g, 3, lambda r: pad // 3 + int(r.integers(1, 5))))))
    res = []
    for name, calls in loci:
        member = (((calls >> 6) & 0xf) == base) & (((calls >> 10) & 1) == fwd) & (((calls >> 12) & 1) == 0) & ((calls & 0x3f) >= 3)
        idx = np.flatnonzero(member)
        assert np.array_equal(calls[idx] & 0x3f, key)  # the group is the fixture's keys, in the fixture's order
        if name == "deep":
            assert len(calls) > MAX_PACKED_DEPTH
        res.append((name, calls, idx))
    return res


@functools.lru_cache(maxsize=None)
def adversarial_batch():
    """every fixture case a pileup can carry, all variants, as one batch; loci = [(case, variant name, group's call indices in the batch)]"""
    rng = np.random.default_rng(4100)
    calls, off, loci = [], [0], []
    for i, c in enumerate(fixture_cases()):
        if c["key"].max() > Q_MAX:
            continue
        for name, lc, idx in _loci_of_case(rng, c, i % 8):
            loci.append((c, name, idx + off[-1]))
            calls.append(lc)
            off.append(off[-1] + len(lc))
    n = len(loci)
    pb = capi.HostPileupBatch(np.array(off, np.int64), np.concatenate(calls), rng.integers(0, 4, n).astype(np.uint8))
    pb.ploidy = rng.choice(np.array([1, 2, 2], np.uint8), n)
    pb.ref_base[::31] = 4  # a few 'N' reference bases
    assert n >= 150 and len(pb.calls) < 200000
    return pb, loci


def _options(kw):
    opt, oopt = capi.germline_options(), pyoracle.germline_options()
    for k, v in kw.items():
        setattr(opt, k, v)
        setattr(oopt, k, v)
    return opt, oopt


@functools.lru_cache(maxsize=None)
def expected(name):
    pb, _ = adversarial_batch()
    _, oopt = _options(OPTION_SETS[name])
    de = pyoracle.adjust_joint_eprob(pb, oopt)
    rec = pyoracle.site_digt_call(pb, de, oopt)
    de.setflags(write=False)
    rec.setflags(write=False)
    return de, rec


def test_the_order_shows_in_the_expected_values(built):
    """in at least 4 loci the adversarial group's calls of the highest quality do not all get the same de: which of them std::sort
    puts first is visible in the output (checked on the oracle's values alone)"""
    pb, loci = adversarial_batch()
    for name, least in (("defaults", 4), ("every_rank", 4)):
        de, _ = expected(name)
        seen = 0
        for c, _, idx in loci:
            top = idx[c["key"] == c["key"].max()]
            seen += len(np.unique(de[top].view(np.uint32))) > 1
        assert seen >= least, (name, seen)
    # and without the floor every call has its own exponent, until 0.65^rank is so small that powf gives 1 and de its limit 0.75 (some
    # forty ranks): among the first ten calls every tie shows
    de, _ = expected("every_rank")
    c, _, idx = next(x for x in loci if x[0]["n"] == 100 and x[0]["k"] == 2 and x[1] == "alone")
    for q in np.unique(c["key"])[-5:]:
        same_q = idx[c["key"] == q]
        assert len(np.unique(de[same_q].view(np.uint32))) == len(same_q)


def _mismatches(got, want, pb, loci, what):
    """names of the loci where the two differ (for the assertion message)"""
    bad = []
    for l, (c, name, _) in enumerate(loci):
        a, b = (got[l:l + 1], want[l:l + 1]) if what == "rec" else (got[pb.call_off[l]:pb.call_off[l + 1]], want[pb.call_off[l]:pb.call_off[l + 1]])
        if a.tobytes() != b.tobytes():
            bad.append((c["n"], c["k"], c["mirror"], name))
    return bad[:12]


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(OPTION_SETS))
def test_dependent_eprob_on_adversarial_groups(gpu, name):
    pb, loci = adversarial_batch()
    opt, _ = _options(OPTION_SETS[name])
    want_de, _ = expected(name)
    assert gpu.lib().sk_libm_restated() == 1
    got = gpu.dependent_eprob(pb, opt)
    assert np.array_equal(got.view(np.uint32), want_de.view(np.uint32)), _mismatches(got, want_de, pb, loci, "de")


@pytest.mark.gpu
@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("name", list(OPTION_SETS))
def test_fused_site_call_on_adversarial_groups(gpu, name, variant):
    pb, loci = adversarial_batch()
    opt, _ = _options(OPTION_SETS[name])
    want_de, want = expected(name)
    gpu.lib().sk_debug_set_g3_variant(variant)
    try:
        fused, de = gpu.site_digt_call_fused(pb, opt, want_de=True)
        assert np.array_equal(de.view(np.uint32), want_de.view(np.uint32)), _mismatches(de, want_de, pb, loci, "de")
        assert fused.tobytes() == want.tobytes(), _mismatches(fused, want, pb, loci, "rec")
        again, none = gpu.site_digt_call_fused(pb, opt)
        assert none is None and again.tobytes() == want.tobytes(), _mismatches(again, want, pb, loci, "rec")
    finally:
        gpu.lib().sk_debug_set_g3_variant(-1)


@pytest.mark.gpu
@pytest.mark.parametrize("variant", [0, 1])
def test_lds_path_declines_groups_whose_leftmost_chain_runs_out_of_depth(gpu, variant):
    """the adversarial groups alone in their loci, default options: every locus fits the LDS path's depth, needs 3 term slots and 4
    ranked calls, so a locus reaches the global pass only through k_top_ranked's `return false`.  That can happen only where the
    full sort takes the heap fallback (the oracle's counter says where) and has to happen somewhere, or the path is not exercised."""
    pb, loci = adversarial_batch()
    pick = [l for l, (c, name, _) in enumerate(loci) if name == "alone" and c["n"] <= MAX_PACKED_DEPTH]
    calls = [pb.calls[pb.call_off[l]:pb.call_off[l + 1]] for l in pick]
    off = np.zeros(len(pick) + 1, np.int64)
    np.cumsum([len(x) for x in calls], out=off[1:])
    sub = capi.HostPileupBatch(off, np.concatenate(calls), pb.ref_base[pick] % 4)
    assert 3 * sub.n_loci <= 864 and sub.n_loci <= 128  # one block, the term pool is not the limit
    with_fallback = 0
    for l in pick:
        pyoracle.heap_sort_runs_reset()
        pyoracle.sort_idx_by_key_desc(loci[l][0]["key"])
        with_fallback += pyoracle.heap_sort_runs() > 0
    want_de = pyoracle.adjust_joint_eprob(sub)
    want = pyoracle.site_digt_call(sub, want_de)
    gpu.lib().sk_debug_set_g3_variant(variant)
    try:
        fused, de = gpu.site_digt_call_fused(sub, want_de=True)
        declined = gpu.lib().sk_debug_g3_global_pass_count()
        assert np.array_equal(de.view(np.uint32), want_de.view(np.uint32))
        assert fused.tobytes() == want.tobytes()
        print("declined by the LDS path: %d of %d loci, %d of which take the heap fallback in the full sort" % (declined, sub.n_loci, with_fallback))
        assert 1 <= declined <= with_fallback, (declined, with_fallback)
    finally:
        gpu.lib().sk_debug_set_g3_variant(-1)
