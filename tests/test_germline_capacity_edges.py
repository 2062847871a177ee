"""The fused germline site kernels ON their capacity limits, not somewhere beyond them: small deterministic batches, each built to put
loci exactly at, one below and one above a limit of csrc/germline_fused.hip, through both kernel variants (with and without `de`,
haploid and diploid) and through the two-step path, against the oracle byte for byte.  sk_debug_g3_global_pass_count() tells which
side of the limit a locus fell on; the expected count is worked out here from the table of limits below, never taken from a run."""
import functools

import numpy as np
import pytest

from oracle import pyoracle
from strelka_amd import capi

# csrc/germline_fused.hip:42-52 (a changed constant is a one-line edit here); the quality range is what a basecall's 6 bits hold
LIMITS = dict(
    LOCI_PER_BLOCK=128,    # loci per workgroup, one thread each
    CAP_CALLS=5312,        # calls of one LDS sub-batch
    V0R_POOL=864,          # term slots of one sub-batch, handed out exact-fit
    MAX_RANK=4,            # ranked calls per group on the LDS path
    V0R_PER_LOCUS=16,      # most term slots one locus may hold
    MAX_PACKED_DEPTH=511,  # 9-bit call index inside the u16 sort key
    SORT_THRESHOLD=16,     # libstdc++'s _S_threshold: groups up to it are insertion-sorted only
    Q_MIN=3, Q_MAX=63,
)
L = LIMITS
QCYCLE = np.array([30, 37, 12, 41, 20, 37, 63, 25, 3, 33, 41, 8, 30, 57, 22, 37, 15, 41, 30, 49, 37, 11, 28], np.uint16)


# ----------------------------------------------------------------------------------------------------------------- builder

def locus(counts, nmm=False, q=None, phase=0):
    """calls of one locus: counts[g] calls of (strand, base) group g = fwd + 2 * base, dealt out group after group in turns (so that
    no group's slice is contiguous), qualities from the fixed cycle (or all `q`), the neighbouring-mismatch flag on every group's
    first call when asked for"""
    left = list(counts) + [0] * (8 - len(counts))
    seen = [0] * 8
    out = []
    while any(left):
        for g in range(8):
            if left[g]:
                left[g] -= 1
                qi = int(QCYCLE[(phase + len(out)) % len(QCYCLE)]) if q is None else q
                out.append(int(capi.make_call(qi, g >> 1, g & 1, 1 if (nmm and seen[g] == 0) else 0)))
                seen[g] += 1
    return np.array(out, np.uint16)


def split(depth, n_groups):
    """depth calls over n_groups groups, as evenly as they go (the first groups take the remainder)"""
    return [depth // n_groups + (g < depth % n_groups) for g in range(n_groups)]


def with_need(m, big=0):
    """group sizes of a locus that asks for exactly m term slots: m // 3 groups of 4 calls (3 slots each: ranks 2..4) and one of
    m % 3 + 1 calls; `big` more calls in a group of 4 change nothing (a group never asks for more than MAX_RANK - 1)"""
    per = L["MAX_RANK"] - 1
    counts = [L["MAX_RANK"]] * (m // per) + ([m % per + 1] if m % per else [])
    if m >= per:
        counts[0] += big
    assert 0 < len(counts) <= 8 and need_of(counts) == m
    return counts


def need_of(counts):
    return sum(min(c - 1, L["MAX_RANK"] - 1) for c in counts if c > 1)


def batch(loci):
    off = np.zeros(len(loci) + 1, np.int64)
    np.cumsum([len(x) for x in loci], out=off[1:])
    calls = np.concatenate(loci) if off[-1] else np.zeros(0, np.uint16)
    ref = (np.arange(len(loci)) % 4).astype(np.uint8)
    if len(loci) > 50:
        ref[::41] = 4  # some 'N' reference bases
    return capi.HostPileupBatch(off, calls, ref)


def ordinary(i, nmm=False):
    """an unremarkable locus: two big groups and an error call or two, depth by a fixed pattern"""
    depth = [30, 7, 44, 1, 18, 0, 3, 25, 39, 12][i % 10]
    counts = [0] * 8
    a = (2 * i) % 8
    counts[a], counts[a ^ 1] = depth - depth // 2, depth // 2
    if depth > 10:
        counts[(a + 3) % 8] = 1 + i % 2
    return locus(counts, nmm=nmm, phase=i)


# ------------------------------------------------------------------------------------------------- which loci the LDS path declines

def valid_group_counts(calls):
    valid = (((calls >> 12) & 1) == 0) & ((calls & 0x3f) >= L["Q_MIN"])
    g = ((calls >> 10) & 1) + 2 * ((calls >> 6) & 0xf)
    return np.bincount(g[valid], minlength=8)


def expected_global_pass(pb):
    """how many loci the fused kernels must leave to the global pass with default options, from LIMITS alone: a block takes
    LOCI_PER_BLOCK loci and works through them in sub-batches, each the longest run of loci whose calls fit CAP_CALLS (a locus that
    does not fit on its own is declined); inside a sub-batch a locus is declined when it is deeper than MAX_PACKED_DEPTH, asks for
    more than V0R_PER_LOCUS term slots, or finds the sub-batch's V0R_POOL used up.  The pool is handed out in no fixed order, so the
    count is defined only where the order cannot matter: the requests fit; or they are all alike; or they exceed the pool by less
    than the smallest of them, so that exactly the last one served fails.  (Default options never need more than MAX_RANK ranks; a
    group that would send std::sort into its heap fallback could be declined too, so the batches must hold none: checked.)"""
    off = pb.call_off
    declined = 0
    for b0 in range(0, pb.n_loci, L["LOCI_PER_BLOCK"]):
        nl = min(L["LOCI_PER_BLOCK"], pb.n_loci - b0)
        s = 0
        while s < nl:
            e = s
            while e < nl and off[b0 + e + 1] - off[b0 + s] <= L["CAP_CALLS"]:
                e += 1
            if e == s:
                declined += 1
                s += 1
                continue
            asks = []
            for l in range(b0 + s, b0 + e):
                c = pb.calls[off[l]:off[l + 1]]
                counts = valid_group_counts(c)
                if len(c) > L["MAX_PACKED_DEPTH"] or need_of(counts) > L["V0R_PER_LOCUS"]:
                    declined += 1
                    continue
                for g in np.flatnonzero(counts > L["SORT_THRESHOLD"]):
                    member = (((c >> 12) & 1) == 0) & ((c & 0x3f) >= L["Q_MIN"]) & ((((c >> 10) & 1) + 2 * ((c >> 6) & 0xf)) == g)
                    pyoracle.heap_sort_runs_reset()
                    pyoracle.sort_idx_by_key_desc(c[member] & 0x3f)
                    assert pyoracle.heap_sort_runs() == 0, "batch design: a group takes the heap fallback"
                if need_of(counts):
                    asks.append(need_of(counts))
            total = sum(asks)
            if total > L["V0R_POOL"]:
                if len(set(asks)) == 1:
                    declined += len(asks) - L["V0R_POOL"] // asks[0]
                else:
                    assert total - min(asks) <= L["V0R_POOL"], "batch design: the count would depend on the order of the lanes"
                    declined += 1
            s = e
    return declined


# ------------------------------------------------------------------------------------------------------------------- cases
# name -> (builder of the list of loci, expected global-pass count worked out by hand from LIMITS)

LADDER = [0, 1, 2, 3, 4, 5, 15, 16, 17, 18, 510, 511, 512, 513, 1022, 1023, 1024]


def depth_ladder(n_groups):
    """every depth of the ladder as n_groups groups of (nearly) equal size: with one group the group's size is the depth, which puts the
    insertion-sort threshold (16 / 17) and the packed call index (511 / 512) on the ladder.  Declined: the loci deeper than
    MAX_PACKED_DEPTH and, with eight groups, those of depth 510 and 511, which ask for 8 * 3 slots"""
    def build(nmm):
        return [locus(split(d, n_groups), nmm=nmm, phase=i) for i, d in enumerate(LADDER)]
    deep = sum(d > L["MAX_PACKED_DEPTH"] for d in LADDER)
    too_many = sum(d <= L["MAX_PACKED_DEPTH"] and need_of(split(d, n_groups)) > L["V0R_PER_LOCUS"] for d in LADDER)
    return build, deep + too_many


def cap_block(extra_at=None):
    """128 loci, 64 of depth 41 and 64 of depth 42 in a mixed order: CAP_CALLS calls exactly; each locus asks for 7 term slots (groups of
    4, 2 and the rest), so the block asks for 896 > V0R_POOL -- where the sub-batch ends decides how many loci find the pool empty"""
    def build(nmm):
        loci = []
        for i in range(L["LOCI_PER_BLOCK"]):
            d = 41 + ((i * 5) % 8 < 4) + (1 if i == extra_at else 0)
            loci.append(locus([d - 6, 4, 0, 2], nmm=nmm, phase=i))
        assert sum(len(x) for x in loci) == L["CAP_CALLS"] + (extra_at is not None)
        return loci
    n = L["LOCI_PER_BLOCK"]
    if extra_at is None:  # one sub-batch of 128
        return build, n - L["V0R_POOL"] // 7
    return build, (n - 1) - L["V0R_POOL"] // 7  # the last locus no longer fits: sub-batches of 127 and 1


def first_locus_too_big(nmm):
    return [locus(split(L["CAP_CALLS"] + 1, 4), nmm=nmm)] + [ordinary(i, nmm) for i in range(L["LOCI_PER_BLOCK"] - 1)]


def locus_of_exactly_cap(nmm):
    return [ordinary(0, nmm), locus(split(L["CAP_CALLS"], 3), nmm=nmm), ordinary(2, nmm), ordinary(3, nmm)]


def two_deep_side_by_side(nmm):
    return [ordinary(i, nmm) for i in range(5)] + [locus(split(3000, 2), nmm=nmm), locus(split(3100, 8), nmm=nmm)] + [ordinary(i, nmm) for i in range(5, 9)]


def deep_at_block_edges(nmm):
    n = L["LOCI_PER_BLOCK"]
    return [ordinary(i, nmm) for i in range(n - 1)] + [locus(split(2000, 2), nmm=nmm), locus(split(L["CAP_CALLS"] + 5, 2), nmm=nmm)] + \
        [ordinary(i, nmm) for i in range(20)]


def need_16_and_17(nmm):
    """five groups of at least 4 valid calls and one of 2: 16 slots, the most a locus may hold; with one of 3: 17, declined"""
    return [locus([4, 4, 4, 4, 4, 2], nmm=nmm), locus([4, 4, 4, 4, 4, 3], nmm=nmm, phase=3), locus([9, 4, 5, 4, 30, 2], nmm=nmm, phase=5),
            locus([4, 4, 4, 4, 4, 2, 1, 1], nmm=nmm, phase=7), locus([4, 4, 4, 4, 4, 1, 1, 2], nmm=nmm, phase=9), locus([4, 4, 4, 4, 4, 2, 2], nmm=nmm, phase=11)]


NEED_16_AND_17 = [16, 17, 16, 16, 16, 17]


def pool_uniform(n):
    def build(nmm):
        return [locus([4, 4, 4, 4, 4, 2], nmm=nmm, phase=i) for i in range(n)]
    return build, max(0, n - L["V0R_POOL"] // L["V0R_PER_LOCUS"])


def pool_mix(total):
    def build(nmm):
        asks = list(range(1, 17)) * 6  # 816
        rest = total - sum(asks)
        while rest > 0:
            asks.append(min(16, rest))
            rest -= asks[-1]
        assert sum(asks) == total and len(asks) <= L["LOCI_PER_BLOCK"]
        return [locus(with_need(m, big=i % 3), nmm=nmm, phase=i) for i, m in enumerate(asks)]
    return build, (1 if total > L["V0R_POOL"] else 0)


def n_loci_of(n):
    return (lambda nmm: [ordinary(i, nmm) for i in range(n)]), 0


def empty_edges(nmm):
    n = 2 * L["LOCI_PER_BLOCK"]
    empty = set(range(3)) | set(range(n // 2 - 3, n // 2 + 3)) | set(range(n - 3, n))
    return [np.zeros(0, np.uint16) if i in empty else ordinary(i + (i % 10 == 5), nmm) for i in range(n)]


def empty_block_between(nmm):
    n = L["LOCI_PER_BLOCK"]
    return [ordinary(i, nmm) for i in range(n)] + [np.zeros(0, np.uint16)] * n + [ordinary(i, nmm) for i in range(n)]


def odd_loci(nmm):
    filt = locus([5, 4, 2], nmm=nmm) | np.uint16(1 << 12)   # every call filtered
    low = np.concatenate([locus([3, 2], q=0), locus([2, 2], q=2), locus([1], q=1)])  # every call below q 3
    mixed = np.concatenate([filt[:4], locus([6, 5], nmm=nmm), low[:3]])
    return [ordinary(0, nmm), filt, low, mixed, locus([7, 5, 1], q=L["Q_MIN"], nmm=nmm), locus([7, 5, 1], q=L["Q_MAX"], nmm=nmm),
            locus([20, 18], q=L["Q_MAX"], nmm=nmm), np.concatenate([locus([5, 4], q=L["Q_MIN"]), locus([4, 5, 1], q=L["Q_MAX"], nmm=nmm)]),
            np.concatenate([locus([17], q=L["Q_MAX"]), locus([17], q=L["Q_MIN"], nmm=nmm)]), ordinary(2, nmm)]


CASES = {
    "ladder_one_group": depth_ladder(1),
    "ladder_two_groups": depth_ladder(2),
    "ladder_eight_groups": depth_ladder(8),
    "cap_exact": cap_block(),
    "cap_plus_one_first": cap_block(0),
    "cap_plus_one_middle": cap_block(64),
    "cap_plus_one_last": cap_block(127),
    "first_locus_too_big": (first_locus_too_big, 1),
    "locus_of_exactly_cap": (locus_of_exactly_cap, 1),
    "two_deep_side_by_side": (two_deep_side_by_side, 2),
    "deep_at_block_edges": (deep_at_block_edges, 2),
    "need_16_and_17": (need_16_and_17, sum(m > L["V0R_PER_LOCUS"] for m in NEED_16_AND_17)),
    "pool_54": pool_uniform(54),
    "pool_55": pool_uniform(55),
    "pool_128": pool_uniform(128),
    "pool_mix_863": pool_mix(863),
    "pool_mix_864": pool_mix(864),
    "pool_mix_865": pool_mix(865),
    "n_loci_1": n_loci_of(1),
    "n_loci_2": n_loci_of(2),
    "n_loci_127": n_loci_of(127),
    "n_loci_128": n_loci_of(128),
    "n_loci_129": n_loci_of(129),
    "n_loci_255": n_loci_of(255),
    "n_loci_257": n_loci_of(257),
    "empty_edges": (empty_edges, 0),
    "empty_block_between": (empty_block_between, 0),
    "odd_loci": (odd_loci, 0),
}
# every case runs without neighbouring-mismatch flags (the ranked terms come from the table); the term-pool cases and a few others run
# once more with a flag in every group (every ranked term of variant 1 is pending)
PENDING_TOO = ("need_16_and_17", "pool_54", "pool_55", "pool_128", "pool_mix_863", "pool_mix_864", "pool_mix_865", "cap_exact", "odd_loci")
PARAMS = [(name, False) for name in CASES] + [(name, True) for name in PENDING_TOO]


@functools.lru_cache(maxsize=None)
def case(name, nmm):
    build, by_hand = CASES[name]
    pb = batch(build(nmm))
    want = {}
    for ploidy in (1, 2):
        pb.ploidy = np.full(pb.n_loci, ploidy, np.uint8)
        de = pyoracle.adjust_joint_eprob(pb)
        rec = pyoracle.site_digt_call(pb, de)
        de.setflags(write=False)
        rec.setflags(write=False)
        want[ploidy] = (de, rec)
    return pb, by_hand, want


@pytest.mark.parametrize("name,nmm", PARAMS)
def test_cases_are_what_they_claim(built, name, nmm):
    """(no GPU) the count worked out by hand for each case equals the model's, the model meets no order-dependent pool and no group in
    the heap fallback, and the limits are met exactly where the case says so"""
    pb, by_hand, _ = case(name, nmm)
    assert expected_global_pass(pb) == by_hand
    depth = np.diff(pb.call_off)
    if name.startswith("ladder"):
        assert depth.tolist() == LADDER
    if name == "ladder_one_group":
        assert [int(valid_group_counts(pb.calls[pb.call_off[l]:pb.call_off[l + 1]]).max()) for l in range(pb.n_loci)] == LADDER
    if name == "cap_exact":
        assert pb.call_off[-1] == L["CAP_CALLS"] and sorted(set(depth.tolist())) == [41, 42] and (depth == 41).sum() == 64
    if name == "locus_of_exactly_cap":
        assert L["CAP_CALLS"] in depth
    if name.startswith("pool_mix"):
        asks = [need_of(valid_group_counts(pb.calls[pb.call_off[l]:pb.call_off[l + 1]])) for l in range(pb.n_loci)]
        assert sum(asks) == int(name[-3:]) and set(asks) == set(range(1, 17))
    if name == "need_16_and_17":
        asks = [need_of(valid_group_counts(pb.calls[pb.call_off[l]:pb.call_off[l + 1]])) for l in range(pb.n_loci)]
        assert asks == NEED_16_AND_17


@pytest.mark.gpu
@pytest.mark.parametrize("name,nmm", PARAMS)
def test_fused_kernels_on_the_edge(gpu, name, nmm):
    pb, by_hand, want = case(name, nmm)
    lib = gpu.lib()
    try:
        for ploidy in (1, 2):
            pb.ploidy = np.full(pb.n_loci, ploidy, np.uint8)
            want_de, want_rec = want[ploidy]
            for variant in (0, 1):
                lib.sk_debug_set_g3_variant(variant)
                for with_de in (True, False):
                    rec, de = gpu.site_digt_call_fused(pb, want_de=with_de)
                    where = (name, nmm, ploidy, variant, with_de)
                    assert lib.sk_debug_g3_global_pass_count() == by_hand, where
                    if with_de:
                        assert np.array_equal(de.view(np.uint32), want_de.view(np.uint32)), where
                    bad = np.flatnonzero([rec[l:l + 1].tobytes() != want_rec[l:l + 1].tobytes() for l in range(pb.n_loci)])
                    assert rec.tobytes() == want_rec.tobytes(), (where, bad[:10].tolist())
            # the two-step path
            de2 = gpu.dependent_eprob(pb)
            assert np.array_equal(de2.view(np.uint32), want_de.view(np.uint32)), (name, nmm, ploidy)
            pb.de = de2
            two = gpu.site_digt_call(pb)
            pb.de = None
            assert two.tobytes() == want_rec.tobytes(), (name, nmm, ploidy)
    finally:
        pb.de = None
        lib.sk_debug_set_g3_variant(-1)
