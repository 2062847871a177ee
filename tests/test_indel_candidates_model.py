"""The loop model of indel candidacy (tests/indel_candidates_model.py) against what the reference's own classes gave: the depth buffers, the
four error rates per (key, sample) as bit patterns, getBreakpointInsertSize and isCandidateIndel of every key, recorded by
tools/golden/indel_candidate_driver.cpp under the germline and the somatic configuration and for the scenes that let one test decide
alone (tools/golden/make_indel_candidates_golden.py).  Then each rule function alone, on the cases no recording can reach."""
import math
import sys

import numpy as np
import pytest

from tests import indel_candidates_cases as K
from tests import indel_candidates_model as CM

SCENES = [sc["name"] for sc in CM.golden()["scenes"]]
DBL_MIN = sys.float_info.min
BELOW_HALF = float(np.nextafter(0.5, 0.0))


def _scene(name):
    return next(sc for sc in CM.golden()["scenes"] if sc["name"] == name)


@pytest.mark.parametrize("name", SCENES)
def test_recorded_scene(name):
    sc = _scene(name)
    keys, depth, out, totals = CM.run_recorded(sc)
    assert CM.depth_as_recorded(depth, sc) == sc["depth"]
    got = CM.as_recorded(keys, out)
    assert len(got) == len(sc["keys"])
    for g, w in zip(got, sc["keys"]):
        assert g == w  # (doubles as bit patterns)
    assert totals == [sum(k["is_candidate"] for k in sc["keys"]), 0]


def test_the_recording_covers_what_it_is_meant_to():
    g = CM.golden()
    assert {"germline", "somatic"} <= set(g["configs"]) and g["configs"]["rates_per_sample"]["is_sample_specific_rates"] == 1
    table = {sc["table_scene"] for sc in g["scenes"] if "table_scene" in sc}
    for name in table:
        assert name + "@germline" in SCENES and name + "@somatic" in SCENES
    by = {sc["name"]: sc for sc in g["scenes"]}
    assert [by["n1_%d_at_depth_20" % n]["keys"][0]["is_candidate"] for n in (1, 2, 3)] == [0, 0, 1]  # papprox flips the answer between 2 and 3
    assert [k["bp_insert_size"] for k in by["breakpoint_insert_19"]["keys"] + by["breakpoint_insert_20"]["keys"]] == [19, 19, 20, 20]
    assert by["depth_sum_equal_to_limit"]["keys"][0]["is_candidate"] == 1 and by["depth_sum_one_above_limit"]["keys"][0]["is_candidate"] == 0
    assert by["key_at_window_begin"]["win_begin"] == by["key_at_window_begin"]["keys"][0]["pos"] and by["key_at_window_begin"]["keys"][0]["is_candidate"] == 1
    half = CM.double_bits(0.5)
    rates = [k["rates"][0] for k in by["rates_at_and_above_one_half"]["keys"]]
    assert any(r[0] == half and r[1] == half for r in rates) and any(CM.bits_double(r[0]) > 0.5 for r in rates)
    for cfg in g["configs"].values():
        p = [CM.bits_double(b) for b in cfg["papprox"]]
        assert len(p) == CM.PAPPROX_N and all(a < b for a, b in zip(p, p[1:]))
    # no recorded scene reaches the exact binomial: every depth is far below 1 000
    assert max([v for sc in g["scenes"] for pair in sc["depth"] for _, values in pair for v in values] + [0]) < 1000


# ---- rule D
def test_depth_a_deletion_then_a_match_advances_the_position():
    d1, d2 = CM.depth_buffers([K.read(10, [(K.M, 3), (K.D, 2), (K.M, 2)])], [0], 8, 12)
    assert d1.tolist() == [0, 0, 1, 1, 1, 0, 0, 1, 1, 0, 0, 0] and not d2.any()


def test_depth_insertions_and_clips_neither_count_nor_advance_and_a_skip_advances():
    path = [(K.S, 4), (K.M, 2), (K.I, 3), (K.M, 1), (K.SKIP, 2), (CM.SEG_SEQ_MATCH, 1), (CM.SEG_SEQ_MISMATCH, 1), (CM.SEG_HARD_CLIP, 5)]
    d1, _ = CM.depth_buffers([K.read(0, path)], [0], 0, 8)
    assert d1.tolist() == [1, 1, 1, 0, 0, 1, 1, 0]


def test_depth_by_alignment_type_and_outside_the_window():
    reads = [K.read(-3, [(K.M, 5)]), K.read(2, [(K.M, 10)]), K.read(1, [(K.M, 2)]), K.read(0, [(K.M, 4)])]
    d1, d2 = CM.depth_buffers(reads, [0, 0, 1, 2], 0, 4)
    assert d1.tolist() == [1, 1, 1, 1] and d2.tolist() == [0, 1, 1, 0]
    with pytest.raises(CM.Refused):
        CM.depth_buffers(reads, [0, 0, 3, 0], 0, 4)


# ---- rule E
def test_rate_type():
    assert CM.rate_type(K.key(5, del_len=2)) == CM.RATE_DELETE and CM.rate_type(K.key(5, ins="A")) == CM.RATE_INSERT
    for k in (K.key(5, del_len=1, ins="A"), K.key(5, K.MISMATCH, 1, "A"), K.key(5, K.BP_LEFT), K.key(5, K.BP_RIGHT)):
        assert CM.rate_type(k) == CM.RATE_OTHER


def test_get_rate_clamps_and_reverts():
    rs = [[(0.1, 0.2), (0.3, 0.4)], [(0.5, 0.6)]]
    assert CM.get_rate(rs, 1, 2, CM.RATE_INSERT) == 0.3 and CM.get_rate(rs, 1, 2, CM.RATE_DELETE) == 0.4
    assert CM.get_rate(rs, 1, 40, CM.RATE_INSERT) == 0.3  # past the last repeat count
    assert CM.get_rate(rs, 2, 7, CM.RATE_DELETE) == 0.6
    assert CM.get_rate(rs, 3, 2, CM.RATE_INSERT) == 0.1  # a pattern size that is not represented: back to (1, 1), not to (1, 2)


def test_indel_error_rate_directions_and_other():
    rs = [[(0.01, 0.02), (0.03, 0.04), (0.05, 0.06)]]
    assert CM.indel_error_rate(rs, K.key(5, del_len=1, unit=1, ref_count=3, indel_count=2)) == (0.06, 0.03)  # delete forward, insert back
    assert CM.indel_error_rate(rs, K.key(5, ins="A", unit=1, ref_count=2, indel_count=3)) == (0.03, 0.06)
    assert CM.indel_error_rate(rs, K.key(5, del_len=1)) == (0.02, 0.01)  # counts of 0 read as 1
    assert CM.indel_error_rate(rs, K.key(5, K.MISMATCH, 1, "A", unit=1, ref_count=3, indel_count=3)) == (0.02, 0.02)  # the larger baseline, both ways


@pytest.mark.parametrize("rate", [0.0, DBL_MIN, 1e-3, BELOW_HALF, 0.5, 0.7, 1.0])
def test_scaling_edge_arguments(rate):
    log_factor = math.log(1.8)
    got = CM.scale_indel_error_rate(log_factor, rate)
    assert 0. <= got <= 0.5
    if rate == 0.0:
        assert got == 0.0  # log(0) = -inf, exp(-inf) = 0
    if rate >= 0.5:
        assert got == 0.5  # the cap, then -log(0 / 1) = inf, 1 / (0 + 1)
    if rate == DBL_MIN:
        assert got == 0.5 * (math.exp(math.log(2 * DBL_MIN / (1 - 2 * DBL_MIN)) + log_factor) / (1. + math.exp(math.log(2 * DBL_MIN / (1 - 2 * DBL_MIN)) + log_factor)))
    assert CM.scale_indel_error_rate(0.0, 0.125) == pytest.approx(0.125, rel=1e-15)


def test_the_candidate_pair_is_never_scaled_and_sets_go_by_sample():
    sets = [K.flat(0.001), K.flat(0.01), K.flat(0.02)]
    k = K.key(5, del_len=1, n1=(1, 1))
    opt = K.options(is_indel_ref_error_factor=1, log_indel_ref_error_factor=math.log(1.8), is_sample_specific_rates=1)
    r0, r1 = CM.error_rates(k, 0, sets, opt), CM.error_rates(k, 1, sets, opt)
    assert r0[0] == 0.01 and r1[0] == 0.02 and r0[1] == CM.scale_indel_error_rate(math.log(1.8), 0.01) != 0.01 and r0[2:] == (0.001, 0.001) == r1[2:]
    assert CM.error_rates(k, 1, sets, dict(opt, is_sample_specific_rates=0))[0] == 0.01  # the shared set
    assert CM.error_rates(k, 1, sets, dict(opt, is_indel_ref_error_factor=0))[1] == 0.02


# ---- rule B
def test_breakpoint_insert_size_ignores_what_comes_after_the_257th():
    assert CM.breakpoint_insert_size([3] * 256 + [9]) == 9 and CM.breakpoint_insert_size([3] * 257 + [9]) == 3
    assert CM.breakpoint_insert_size_batch([3] * 256 + [9]) == (9, True) and CM.breakpoint_insert_size_batch([3] * 257 + [9]) == (9, False)
    assert CM.breakpoint_insert_size_batch([]) == (0, True)


# ---- rule C
def test_is_reject_null_cases():
    P = K.PAPPROX
    assert CM.is_reject_null(5, 0.0, 1, P) is True and CM.is_reject_null(5, 0.0, 0, P) is False and CM.is_reject_null(5, -0.0, 2, P) is True
    assert CM.is_reject_null(5, 1e-4, 0, P) is False
    assert [CM.is_reject_null(20, 5e-5, n1, P) for n1 in (1, 2, 3)] == [False, False, True]
    assert CM.is_reject_null(900, 3e-3, 17, P) is False and CM.is_reject_null(900, 3e-3, 18, P) is True and CM.is_reject_null(900, 3e-3, 40, P) is True  # 2.7: min(n1, 18)
    assert CM.is_reject_null(10, 0.02, 3, P) is None  # the variance ratio is above 0.01
    assert CM.is_reject_null(1000, 3e-3, 5, P) is None  # n p = 3 is not below papprox[17]
    p = K.ratio_exactly_one_hundredth()
    assert CM.is_reject_null(18, p, 6, P) is False and CM.is_reject_null(18, p, 7, P) is True  # 0.1782: below papprox[6], not below papprox[5]
    assert CM.is_reject_null(18, p, 7, P, poisson_ratio_inclusive=False) is None  # (< instead of <= is seen)


def _cand(keys, depth1=None, depth2=None, win_begin=0, n_pos=64, sets=None, sample_obs=None, **opt):
    n_samples = len(keys[0]["samples"])
    zeros = [np.zeros(n_pos, np.uint32) for _ in range(n_samples)]
    return CM.indel_candidates(keys, sample_obs or [[] for _ in range(n_samples)], depth1 or zeros, depth2 or zeros, win_begin, sets or [K.ramp(), K.ramp()], K.options(**opt))


def _depth(n_pos, **at):
    d = np.zeros(n_pos, np.uint32)
    for pos, v in at.items():
        d[int(pos[1:])] = v
    return d


def test_signal_floor_fudge_and_first_true():
    zero = [K.flat(0.0), K.ramp()]  # p <= 0: any tier-1 read rejects the null -- here the floor of 2 decides alone
    assert _cand([K.key(10, del_len=1, n1=(1,))], sets=zero)[0][0]["is_candidate"] == 0
    assert _cand([K.key(10, del_len=1, n1=(2,))], sets=zero)[0][0]["is_candidate"] == 1  # total = max(0, 2): n1 above the depth
    assert _cand([K.key(10, del_len=1, n1=(1,))], depth1=[_depth(64, p9=2)], sets=zero)[0][0]["is_candidate"] == 1
    assert _cand([K.key(10, del_len=1, n1=(1,))], depth1=[_depth(64, p10=2)], sets=zero)[0][0]["is_candidate"] == 0  # pos - 1, not pos
    # a later sample says true; an exact-binomial sample before it leaves the key undecided, one after it is never asked
    # p = 3e-3: at depth 5 five reads give 0.015 < papprox[4]; at depth 1 000, n p = 3 is not below papprox[17]
    d = [_depth(64, p9=5), _depth(64, p9=1000)]
    out, totals = _cand([K.key(10, del_len=1, n1=(5, 5))], depth1=d, sets=[K.flat(3e-3), K.ramp()])
    assert (out[0]["is_candidate"], out[0]["undecided"]) == (1, CM.DECIDED) and totals == [1, 0]
    out, totals = _cand([K.key(10, del_len=1, n1=(5, 5))], depth1=d[::-1], sets=[K.flat(3e-3), K.ramp()])
    assert (out[0]["is_candidate"], out[0]["undecided"]) == (0, CM.UNDECIDED_EXACT_BINOMIAL) and totals == [0, 1]


def test_undecided_by_the_exact_binomial():
    d = [_depth(64, p9=30)]
    for cand_rate in (0.02, 0.1):  # p = 0.02: the ratio; 30 * 0.1 = 3.0: not below papprox[17]
        out, totals = _cand([K.key(10, del_len=1, n1=(3,))], depth1=d, sets=[K.flat(cand_rate), K.ramp()])
        assert (out[0]["is_candidate"], out[0]["undecided"]) == (0, CM.UNDECIDED_EXACT_BINOMIAL) and totals == [0, 1]


def test_order_of_the_tests():
    d = [_depth(64, p9=20)]
    ok = dict(del_len=1, n1=(3,))
    assert _cand([K.key(10, **ok)], depth1=d)[0][0]["is_candidate"] == 1
    assert _cand([K.key(10, flags=CM.DO_NOT_GENOTYPE | CM.AR_PENDING, **ok)], depth1=d)[0][0] == dict(_cand([K.key(10, **ok)], depth1=d)[0][0], is_candidate=0)
    out, totals = _cand([K.key(10, flags=CM.AR_PENDING, **ok)], depth1=d)
    assert (out[0]["is_candidate"], out[0]["undecided"]) == (0, CM.UNDECIDED_AR_PENDING) and totals == [0, 1]
    assert _cand([K.key(10, **ok)], depth1=d, is_haplotyping_enabled=1)[0][0]["is_candidate"] == 0
    assert _cand([K.key(10, active_region_id=0, **ok)], depth1=d, is_haplotyping_enabled=1)[0][0]["is_candidate"] == 1
    assert _cand([K.key(10, del_len=1, n1=(0,))], depth1=d, is_candidate_indel_signal_test=0)[0][0]["is_candidate"] == 0
    assert _cand([K.key(10, del_len=1, n1=(0, 1))], is_candidate_indel_signal_test=0)[0][0]["is_candidate"] == 1


def test_breakpoint_length_and_arrival_order():
    d = [_depth(64, p9=20)]
    for n_obs, longest, want in ((3, 19, (0, CM.DECIDED)), (3, 20, (1, CM.DECIDED)), (257, 20, (1, CM.DECIDED)), (258, 19, (0, CM.DECIDED)),
                                 (258, 20, (0, CM.UNDECIDED_BP_OBS_ORDER))):
        obs = [K.bp_obs(10, K.BP_LEFT, 5)] * (n_obs - 1) + [K.bp_obs(10, K.BP_LEFT, longest)]
        out, _ = _cand([K.key(10, K.BP_LEFT, n1=(3,), n_bp_obs=n_obs)], depth1=d, sample_obs=[obs])
        assert (out[0]["is_candidate"], out[0]["undecided"], out[0]["bp_insert_size"]) == want + (longest,), (n_obs, longest)
    with pytest.raises(CM.Refused):
        _cand([K.key(10, K.BP_LEFT, n1=(3,))], sample_obs=[[K.bp_obs(10, K.BP_RIGHT, 5)]])


def test_depth_filter_sums_counted_samples_as_a_double():
    d1 = [_depth(64, p9=20), _depth(64, p9=7)]
    d2 = [_depth(64, p9=4), _depth(64, p9=1)]
    k = [K.key(10, del_len=1, n1=(3, 0))]
    assert _cand(k, d1, d2, max_candidate_depth=32.0)[0][0]["is_candidate"] == 1
    assert _cand(k, d1, d2, max_candidate_depth=31.5)[0][0]["is_candidate"] == 0
    assert _cand(k, d1, d2, max_candidate_depth=24.0, is_count_towards_depth_filter=[1, 0] + [1] * 6)[0][0]["is_candidate"] == 1
    assert _cand(k, d1, d2, max_candidate_depth=0.0)[0][0]["is_candidate"] == 1  # off


def test_refusals():
    k = [K.key(10, del_len=1, n1=(3,))]
    for sets in ([[], K.ramp()], [K.flat(0.1, n_sizes=5), K.ramp()], [K.flat(0.1, n_counts=41), K.ramp()], [[[]], K.ramp()], [K.ramp(), K.flat(1.5)],
                 [K.ramp(), K.flat(-0.1)], [K.ramp(), K.flat(float("nan"))]):
        with pytest.raises(CM.Refused):
            _cand(k, sets=sets)
    with pytest.raises(CM.Refused):
        _cand(k, papprox=[0.] * 18)  # what the defaults leave
    with pytest.raises(CM.Refused):
        _cand(k, papprox=K.PAPPROX[:5] + [K.PAPPROX[4]] + K.PAPPROX[6:])
    with pytest.raises(CM.Refused):
        CM.check_options(9, K.options())
    assert CM.default_options()["papprox"] == [0.] * 18
