"""The read intake without a device: the model (tests/intake_model.py) against the vectors recorded from the reference
(tests/golden/read_intake/, made by tools/golden/intake_driver.cpp), the closed form of the valid range against the loop as written,
the crafted cases against values worked out by hand, the candidate flag at its boundaries, and the C-ABI's host side (bound,
argument checks, the refusal to compute without a device)."""
import ctypes as C
import math
from fractions import Fraction

import numpy as np
import pytest

from strelka_amd import capi
from tests import intake_cases as K
from tests import intake_model as M


# ---- the model against the reference's own numbers ------------------------------------------------------------------------------------------


def test_model_reproduces_the_reference_golden():
    g = K.golden()
    doc = g["doc"]
    assert len(doc["reads"]) >= 200 and len(doc["sites"]) < 1000
    res = M.read_intake(g["ref"], g["ref_offset"], g["reads"], g["low"], g["win_begin"], g["n_pos"], g["max_indel_size"])
    n_obs = n_noise = 0
    kinds = set()
    for i, want in enumerate(doc["reads"]):
        vb, ve, span, n = res["reads"][i]
        assert [vb, ve] == want["valid"], i
        assert span == want["span"], i
        mine = res["obs"][res["obs_off"][i]:res["obs_off"][i + 1]]
        assert n == len(mine) == len(want["obs"]), i
        code = g["reads"][i]["code"]
        # the driver walks the reference's IndelBuffer, which is ordered by key: compare as sorted lists
        got = sorted((o["pos"], o["type"], o["deletion_length"], M.read_string(code, o["ins_begin"], o["ins_begin"] + o["ins_len"]),
                      M.read_string(code, o["bp_begin"], o["bp_begin"] + o["bp_len"]), o["is_noise"]) for o in mine)
        ref = sorted((o["pos"], o["type"], o["deletion_length"], o["ins"], o["bp"], o["is_noise"]) for o in want["obs"])
        assert got == ref, i
        assert all(o["read"] == i and o["is_low_mapq"] == want["low_mapq"] for o in mine)
        n_obs += len(mine)
        n_noise += sum(o["is_noise"] for o in mine)
        kinds |= {o["type"] for o in mine}
    assert n_obs > 300 and n_noise > 10 and kinds == {M.INDEL_INDEL, M.INDEL_BP_LEFT, M.INDEL_BP_RIGHT}
    assert res["sites"] == [(c, d) for c, d, _ in doc["sites"]]
    assert res["is_candidate"] == [bool(k) for _, _, k in doc["sites"]]
    assert 50 < sum(res["is_candidate"]) < len(doc["sites"]) - 50


# ---- the valid range: closed form == the loop -------------------------------------------------------------------------------------------------


def _crafted_scores():
    z = [0] * 12
    return {
        "sum_exactly_-11": ([-5, -5, -1] + [2] * 9, z),
        "sum_-10": ([-5, -5] + [2] * 10, z),
        "min_tied_at_several_indices": ([-5, -5, -5, 0, 0, 2, 2, 2, 2, 2, 2, 2], [2, 2, 2, 2, 2, 2, 2, 0, 0, -5, -5, -5]),
        "min_at_the_last_base": ([2] * 11 + [-40], [-40] + [2] * 11),
        "empty_range_collapse": ([2] * 9 + [-40, 2, 2], [2, 2, -40] + [2] * 9),  # begin 10, end 2
        "read_length_1": ([-11], [-11]),
        "read_length_1_kept": ([-10], [-10]),
        "reverse_exactly_-11": (z, [2] * 9 + [-1, -5, -5]),
        "reverse_-10": (z, [2] * 10 + [-5, -5]),
        "empty_read": ([], []),
    }


def test_closed_form_of_the_valid_range_equals_the_loop():
    want = {"sum_exactly_-11": (3, 12), "sum_-10": (0, 12), "min_tied_at_several_indices": (5, 7), "min_at_the_last_base": (0, 0),
            "empty_range_collapse": (0, 0), "read_length_1": (0, 0), "read_length_1_kept": (0, 1), "reverse_exactly_-11": (0, 9), "reverse_-10": (0, 12),
            "empty_read": (0, 0)}
    for name, (fwd, rev) in _crafted_scores().items():
        loop = M.reckoning(fwd, rev)
        assert loop == want[name], name  # (worked out by hand)
        assert M.reckoning_closed_form(fwd, rev) == loop, name
    rng = np.random.default_rng(7301)
    cut = 0
    for k in range(10000):
        n = int(rng.integers(1, 80)) if k % 50 else int(rng.integers(900, 1025))
        p = float(rng.choice([0.05, 0.2, 0.5]))
        # the values a base can score: 2, 0, -5, and -10 where a deletion sits beside a mismatch
        fwd = rng.choice([2, 0, -5, -10], n, p=[1 - p, p / 4, p / 2, p / 4]).tolist()
        rev = fwd if k % 3 else rng.choice([2, 0, -5, -10], n, p=[1 - p, p / 4, p / 2, p / 4]).tolist()
        loop = M.reckoning(fwd, rev)
        assert M.reckoning_closed_form(fwd, rev) == loop, (k, fwd, rev)
        cut += loop != (0, n)
    assert cut > 2000


# ---- crafted cases, by hand ----------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("case", K.crafted(), ids=lambda c: c["name"])
def test_crafted_case_matches_the_hand_computed_values(case):
    res = M.read_intake(case["ref"], case["ref_offset"], case["reads"], case["low"], case["win_begin"], case["n_pos"], case["max_indel_size"])
    assert case["expect"]
    for key, want in case["expect"].items():
        assert res[key] == want, key
    assert res["obs_off"][-1] == len(res["obs"]) == sum(r[3] for r in res["reads"])


def test_crafted_cases_cover_what_they_should():
    names = {c["name"] for c in K.crafted()}
    assert names >= {"soft_clips", "insertion", "deletion_1", "deletion_3", "swap", "max_indel_size", "insert_10_invalid", "insert_11_invalid", "low_mapq",
                     "edge_indels", "n_against_n"}


def test_model_refuses_what_the_reference_throws_on():
    for path, n in (([(M.MATCH, 4), (M.SKIP, 3), (M.MATCH, 4)], 8), ([(M.MATCH, 4), (M.PAD, 1), (M.MATCH, 4)], 8), ([(M.INSERT, 4)], 4),
                    ([(M.MATCH, 4), (M.MATCH, 4)], 8), ([(M.MATCH, 4), (M.SOFT_CLIP, 2), (M.MATCH, 2)], 8), ([(M.MATCH, 7)], 8),
                    ([(M.MATCH, 8), (M.INSERT, 0), (M.MATCH, 0)], 8), ([(M.MATCH, 1025)], 1025)):
        with pytest.raises(M.PathError):
            M.check_path(path, n)
    M.check_path([(M.HARD_CLIP, 2), (M.SOFT_CLIP, 1), (M.MATCH, 6), (M.SOFT_CLIP, 1), (M.HARD_CLIP, 3)], 8)


# ---- the candidate flag at its boundaries ---------------------------------------------------------------------------------------------------------

# where evaluating `count >= f * depth` in float differs from the same comparison on the exact values of the float constants: the
# product f * depth rounds DOWN to the integer count (0.2f is a little above 1/5), so the flag is set where exact arithmetic would not set it
FLOAT_DIFFERS_FROM_EXACT = [(d, d // 5) for d in range(45, 201, 5)]


def test_candidate_flag_at_the_boundaries():
    f32, low32 = Fraction(float(np.float32(0.2))), Fraction(float(np.float32(0.35)))
    assert f32 > Fraction(1, 5) and low32 < Fraction(7, 20)
    differs, n = [], 0
    for depth in range(201):
        counts = set()
        for t in (f32 * depth, Fraction(9), low32 * depth):
            counts |= {c for c in range(math.floor(t) - 1, math.ceil(t) + 2) if c >= 0}
        for count in sorted(counts):
            n += 1
            got = M.is_candidate_variant("A", count, depth)
            exact = (count >= 9 and count >= f32 * depth) or count >= low32 * depth
            decimal = (count >= 9 and 5 * count >= depth) or 20 * count >= 7 * depth  # the constants as written: 0.2, 0.35
            assert got == decimal, (depth, count)
            if got != exact:
                assert got, (depth, count)
                differs.append((depth, count))
            assert not M.is_candidate_variant("N", count, depth)
    assert n > 2000
    assert differs == FLOAT_DIFFERS_FROM_EXACT
    assert M.is_candidate_variant("A", 0, 0)  # true at depth 0 with count 0
    assert not M.is_candidate_variant("A", 0, 1)
    assert M.is_candidate_variant("A", 8, 22) and not M.is_candidate_variant("A", 8, 23)   # 0.35 * 23 = 8.05
    assert M.is_candidate_variant("A", 9, 45) and not M.is_candidate_variant("A", 9, 46)   # 9 >= 0.2 * 45
    assert not M.is_candidate_variant("A", 9, 45, min_alt_allele_fraction=0.25)


# ---- the C-ABI without a device -----------------------------------------------------------------------------------------------------------------------


def test_new_symbols_are_declared_and_exported(built):
    from tests.test_abi import declared_symbols
    new = {"sk_intake_options_default", "sk_read_intake_obs_bound", "sk_read_intake", "sk_read_intake_dev", "sk_read_intake_scratch_bytes"}
    assert new <= set(declared_symbols())
    assert new <= set(capi.EXPORTS)
    for name in new:
        assert hasattr(capi.lib(), name)
    assert C.sizeof(capi.IntakeOptions) == 8
    assert (capi.INTAKE_READ_DTYPE.itemsize, capi.INTAKE_OBS_DTYPE.itemsize, capi.INTAKE_SITE_DTYPE.itemsize) == (16, 32, 8)


def test_defaults_are_the_references(built):
    o = capi.intake_options()
    assert o.max_indel_size == M.MAX_INDEL_SIZE == 49
    assert np.float32(o.min_alt_allele_fraction) == np.float32(M.MIN_ALT_ALLELE_FRACTION)


def test_obs_bound_and_scratch_are_host_arithmetic(built):
    assert capi.read_intake_obs_bound(0) == 0
    assert [capi.read_intake_obs_bound(n) for n in (1, 2, 65, 1 << 33)] == [2, 4, 130, 1 << 34]
    assert capi.lib().sk_read_intake_obs_bound(-1) == -1
    s = [capi.lib().sk_read_intake_scratch_bytes(n, 4 * n, 1000) for n in (0, 1, 4096, 4097, 1 << 20)]
    assert all(x > 0 and x % 256 == 0 for x in s) and s == sorted(s)
    assert s[-1] >= 8 * ((1 << 20) // 4096 + 1)


def test_no_cpu_fallback(built):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    c = K.crafted()[1]
    with pytest.raises(capi.StrelkaAmdError) as e:
        capi.read_intake(c["ref"], c["ref_offset"], c["reads"], c["low"], c["win_begin"], c["n_pos"])
    assert "sk_init" in str(e.value)  # (the library computes nothing without a device: there is no CPU fallback)


def _call(reads, low=None, obs_cap=None, n_pos=10, ref="ACGTACGTACGT", n_reads=None, mutate=None):
    """sk_read_intake on raw arrays -> (return code, message)"""
    L = capi.lib()
    read_off, code, path_off, n_seg, path, pos = capi.pack_reads(reads)
    lowa = np.zeros(len(reads) + 1, np.uint8)
    if mutate:
        mutate(dict(read_off=read_off, path_off=path_off, n_seg=n_seg, path=path))
    cap = capi.read_intake_obs_bound(max(int(path_off[-1]), 0)) if obs_cap is None else obs_cap
    rec = np.zeros(len(reads) + 1, capi.INTAKE_READ_DTYPE)
    obs_off = np.zeros(len(reads) + 2, np.int64)
    obs = np.zeros(max(cap, 0) + 1, capi.INTAKE_OBS_DTYPE)
    sites = np.zeros(abs(n_pos) + 1, capi.INTAKE_SITE_DTYPE)
    cand = np.zeros(abs(n_pos) + 1, np.uint8)
    opt = capi.intake_options()
    rc = L.sk_read_intake(ref.encode(), 100, len(ref), len(reads) if n_reads is None else n_reads, capi._p(read_off), capi._p(code), capi._p(path_off),
                          capi._p(n_seg), capi._p(path), capi._p(pos), capi._p(lowa), C.byref(opt), 100, n_pos, capi._p(rec), capi._p(obs_off), capi._p(obs),
                          cap, capi._p(sites), capi._p(cand))
    return rc, capi.last_error()


def test_arguments_are_checked(built):
    """every refusal comes with its message, with or without a device (the checks run before the device is asked for)"""
    def read(path, n=None):
        n = sum(l for t, l in path if M.is_read_length(t)) if n is None else n
        return dict(code=np.full(n, 1, np.uint8), pos=100, path=path)

    ok = read([(M.MATCH, 8)])
    for reads, kw, word in (
            ([read([(M.MATCH, 1025)])], {}, "SK_PILEUP_MAX_READ_LEN"),
            ([ok, read([(M.MATCH, 4), (M.SKIP, 5), (M.MATCH, 4)])], {}, "SKIP"),
            ([read([(M.MATCH, 4), (M.PAD, 1), (M.MATCH, 4)])], {}, "PAD"),
            ([read([(M.MATCH, 4), (M.MATCH, 4)])], {}, "repeated"),
            ([read([(M.MATCH, 4), (M.SOFT_CLIP, 2), (M.MATCH, 4)])], {}, "clipping"),
            ([read([(M.MATCH, 4), (M.HARD_CLIP, 2), (M.MATCH, 4)])], {}, "clipping"),
            ([read([(M.SOFT_CLIP, 4), (M.INSERT, 4)])], {}, "floating"),
            ([read([(0, 4), (M.MATCH, 4)], 4)], {}, "unknown"),
            ([read([(11, 4), (M.MATCH, 4)], 4)], {}, "unknown"),
            ([read([(M.MATCH, 4), (M.INSERT, 0), (M.MATCH, 4)])], {}, "zero-length"),
            ([ok, read([(M.MATCH, 8)], 9)], {}, "read length differs"),
            ([ok, read([(M.MATCH, 8), (M.INSERT, 2), (M.MATCH, 1)], 10)], {}, "read length differs"),
            ([ok], dict(obs_cap=1), "obs_cap"),
            ([ok], dict(obs_cap=-1), "negative"),
            ([ok], dict(n_pos=-1), "negative"),
            ([ok], dict(n_reads=-1), "negative"),
            ([ok, ok], dict(mutate=lambda a: a["read_off"].__setitem__(2, 4)), "negative"),
            ([ok], dict(mutate=lambda a: a["n_seg"].__setitem__(0, 2)), "n_seg"),
            ([ok], dict(mutate=lambda a: a["n_seg"].__setitem__(0, -1)), "n_seg")):
        rc, msg = _call(reads, **kw)
        assert rc != 0 and word in msg, (word, msg)
        if reads[-1] is not ok and len(reads) == 2:
            assert "read 1" in msg, msg
    L = capi.lib()
    opt = capi.intake_options()
    assert L.sk_read_intake(None, 0, 0, 0, *([None] * 7), None, 0, 0, None, None, None, 0, None, None) != 0 and "null" in capi.last_error()
    assert L.sk_read_intake_dev(None, 0, 0, 1, *([None] * 7), C.byref(opt), 0, 0, None, None, None, 0, None, None, None, 0, None) != 0 and "null" in capi.last_error()
    assert L.sk_read_intake_dev(None, 0, 0, -1, *([None] * 7), C.byref(opt), 0, 0, None, None, None, 0, None, None, None, 0, None) != 0 and "negative" in capi.last_error()


def test_batch_generator_gives_what_the_device_tests_need():
    """the seeded batches of tests/test_read_intake.py: every kind of observation, noise, clips, reads off both ends of the segment"""
    ref, off, reads, low = K.random_batch(400, 150, 2000, 3)
    assert all(len(r["code"]) == 150 for r in reads) and [r["pos"] for r in reads] == sorted(r["pos"] for r in reads)
    reads, low = K.usable(reads, low)
    assert len(reads) == 400
    res = M.read_intake(ref, off, reads, low, off - 60, 2200)
    assert {o["type"] for o in res["obs"]} == {M.INDEL_INDEL, M.INDEL_BP_LEFT, M.INDEL_BP_RIGHT}
    assert any(o["is_noise"] for o in res["obs"]) and any(o["is_low_mapq"] for o in res["obs"])
    assert any(r[:2] != (0, 150) for r in res["reads"])
    assert reads[0]["pos"] < off and reads[-1]["pos"] + 150 > off + 2000
