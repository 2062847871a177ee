"""Loop model of indel candidacy (sk_read_depth, sk_indel_candidates; csrc/indel_candidates.hip): the header's rules D, E, B and C, one
function each, in plain Python and numpy doubles.  L/ is the reference's src/c++/lib/.

  rule D  depth_buffers            add_alignment_to_depth_buffer (L/blt_util/depth_buffer_util.cpp:30-48) by map level as
                                   load_read_in_depth_buffer does (L/starling_common/starling_pos_processor_base.cpp:626-644)
  rule E  rate_type, get_rate, indel_error_rate, soft_max_transform, soft_max_inverse_transform, scale_indel_error_rate, error_rates
                                   (L/calibration/IndelErrorRateSet.hh:43-60, :82-110; IndelErrorModel.cpp:226-274; L/blt_util/prob_util.hh:45-103;
                                   L/starling_common/IndelData.cpp:118-160)
  rule B  breakpoint_insert_size   BreakpointInsertSequenceManager::addObservation / getSize (L/starling_common/IndelData.hh:147-192), in arrival
                                   order; breakpoint_insert_size_batch: what a batch, which has no order, can say
  rule C  is_reject_null, signal_test, weak_signal_test, is_candidate   (L/starling_common/min_count_binom_gte_cache.cpp:77-153,
                                   L/starling_common/IndelBuffer.cpp:137-263)

log and exp are the host libm's (math.log, math.exp): the reference's.  Imports nothing from the library.  Pinned to vectors recorded from
the reference's own classes by tests/test_indel_candidates_model.py."""
import functools
import json
import math
import os
import struct

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "indel_candidates", "indel_candidates_golden.json")

NONE, INDEL, MISMATCH, BP_LEFT, BP_RIGHT = range(5)  # INDEL::index_t (SK_INDEL_*)
SEG_NONE, SEG_MATCH, SEG_INSERT, SEG_DELETE, SEG_SKIP, SEG_SOFT_CLIP, SEG_HARD_CLIP, SEG_PAD, SEG_SEQ_MATCH, SEG_SEQ_MISMATCH = range(10)  # ALIGNPATH::align_t
IAT_TIER1, IAT_TIER2, IAT_SUBMAP = range(3)
TIER1 = 0  # SK_ITAB_TIER1
DO_NOT_GENOTYPE, AR_PENDING = 1, 2  # SK_ITAB_* flags
RATE_INSERT, RATE_DELETE, RATE_OTHER = range(3)  # IndelErrorRateType as getRateType gives it
DECIDED, UNDECIDED_AR_PENDING, UNDECIDED_EXACT_BINOMIAL, UNDECIDED_BP_OBS_ORDER = range(4)  # SK_ICAND_*
MAX_SIZES, MAX_COUNTS, PAPPROX_N, MAX_BP_OBS, MAX_SAMPLES = 4, 40, 18, 257, 8


class Refused(Exception):
    pass


def double_bits(x):
    return struct.unpack("<Q", struct.pack("<d", float(x)))[0]


def bits_double(b):
    return struct.unpack("<d", struct.pack("<Q", int(b)))[0]


# ---- rule D
def depth_buffers(reads, iat, win_begin, n_pos):
    """reads [dict(pos, path [(type, length)])], iat per read -> (depth1, depth2) uint32[n_pos]; base by base, as the reference counts"""
    depth = [np.zeros(n_pos, np.uint32), np.zeros(n_pos, np.uint32)]
    for rd, t in zip(reads, iat):
        if int(t) > IAT_SUBMAP:
            raise Refused("an iat above 2")
        head = int(rd["pos"])  # ref_head_pos
        for seg_type, length in rd["path"]:
            if not 0 <= int(seg_type) <= SEG_SEQ_MISMATCH:
                raise Refused("a segment type above SK_SEG_SEQ_MISMATCH")
            if seg_type in (SEG_MATCH, SEG_SEQ_MATCH, SEG_SEQ_MISMATCH) and int(t) != IAT_SUBMAP:  # is_segment_align_match
                for j in range(int(length)):
                    if win_begin <= head + j < win_begin + n_pos:
                        depth[int(t)][head + j - win_begin] += 1
            if seg_type in (SEG_MATCH, SEG_DELETE, SEG_SKIP, SEG_SEQ_MATCH, SEG_SEQ_MISMATCH):  # is_segment_type_ref_length
                head += int(length)
    return depth[0], depth[1]


# ---- rule E.  A rate set: [[(insertion rate, deletion rate) for repeat counts 1, 2, ...] for pattern sizes 1, 2, ...]
def check_rate_set(rs):
    if not 1 <= len(rs) <= MAX_SIZES:
        raise Refused("a rate set of no or more than SK_RATE_MAX_SIZES sizes")
    for counts in rs:
        if not 1 <= len(counts) <= MAX_COUNTS:
            raise Refused("a rate set with a count outside 1..SK_RATE_MAX_COUNTS")
        for pair in counts:
            if not all(0. <= float(x) <= 1. for x in pair):
                raise Refused("a rate outside [0, 1]")


def rate_type(key):
    """getRateType: key is a table record (pos, type, del_len, ins)"""
    if key["type"] == INDEL and len(key["ins"]) == 0 and key["del_len"] > 0:
        return RATE_DELETE
    if key["type"] == INDEL and len(key["ins"]) > 0 and key["del_len"] == 0:
        return RATE_INSERT
    return RATE_OTHER


def get_rate(rs, size, count, which):
    """IndelErrorRateSet::getRate"""
    assert size > 0 and count > 0
    if size > len(rs):  # revert back to baseline if the repeating pattern size isn't represented
        size, count = 1, 1
    by_count = rs[min(size - 1, len(rs) - 1)]
    pair = by_count[min(count - 1, len(by_count) - 1)]
    return float(pair[1] if which == RATE_DELETE else pair[0])


def indel_error_rate(rs, key):
    """IndelErrorModel::getIndelErrorRate -> (refToIndelErrorProb, indelToRefErrorProb)"""
    which = rate_type(key)
    if which == RATE_OTHER:
        r = max(get_rate(rs, 1, 1, RATE_INSERT), get_rate(rs, 1, 1, RATE_DELETE))
        return r, r
    size, ref_count, indel_count = max(key["repeat_unit_len"], 1), max(key["ref_repeat_count"], 1), max(key["indel_repeat_count"], 1)
    return get_rate(rs, size, ref_count, which), get_rate(rs, size, indel_count, RATE_INSERT if which == RATE_DELETE else RATE_DELETE)


def _log(x):
    return -math.inf if x == 0. else math.log(x)  # (std::log(0.) is -inf; math.log raises)


def soft_max_transform(real, lo=0., hi=1.):
    if real <= 0.:
        er = math.exp(real)
        t = er / (1. + er)
    else:
        enr = math.exp(-real)
        t = 1. / (enr + 1.)
    return t * (hi - lo) + lo


def soft_max_inverse_transform(ranged, lo=0., hi=1.):
    ranged = (ranged - lo) / (hi - lo)
    assert 0. <= ranged <= 1.
    if ranged <= 0.5:
        return _log(ranged / (1 - ranged))
    return -_log((1 - ranged) / ranged)


def scale_indel_error_rate(log_factor, rate, cap=True):
    """scaleIndelErrorRate; cap=False leaves the min(rate, 0.5) out (what a test that must fail does)"""
    if cap:
        rate = min(rate, 0.5)
    rate = soft_max_inverse_transform(rate, 0.0, 0.5)
    rate += log_factor
    return soft_max_transform(rate, 0.0, 0.5)


def error_rates(key, s, rate_sets, opt):
    """IndelSampleData::initializeAuxInfo -> (refToIndel, indelToRef, candidateRefToIndel, candidateIndelToRef); rate_sets[0] is the candidate set"""
    rs = rate_sets[1 + (s if opt["is_sample_specific_rates"] else 0)]
    ref_to_indel, indel_to_ref = indel_error_rate(rs, key)
    if opt["is_indel_ref_error_factor"]:
        indel_to_ref = scale_indel_error_rate(opt["log_indel_ref_error_factor"], indel_to_ref)
    return (ref_to_indel, indel_to_ref) + indel_error_rate(rate_sets[0], key)


# ---- rule B
def breakpoint_insert_size(lengths_in_arrival_order):
    """addObservation then getSize: observations after the 257th are ignored"""
    obs_count, size = 0, 0
    for n in lengths_in_arrival_order:
        if obs_count > 256:
            continue
        size = max(size, int(n))
        obs_count += 1
    return size


def breakpoint_insert_size_batch(lengths):
    """-> (the maximum over all observations, whether that IS getSize() whatever the arrival order)"""
    return max([int(n) for n in lengths] + [0]), len(lengths) <= MAX_BP_OBS


# ---- rule C
def is_reject_null(n, p, n_success, papprox, poisson_ratio_inclusive=True):
    """min_count_binom_gte_cache::isRejectNull -> True, False, or None where it goes on to min_count_binomial_gte_exact"""
    if p <= 0.:
        return n_success > 0
    if n_success == 0:
        return False
    ratio = p / (1 - p)
    if (ratio <= 0.01) if poisson_ratio_inclusive else (ratio < 0.01):  # isPoissonApprox
        np_ = n * p
        if np_ < papprox[PAPPROX_N - 1]:
            return np_ < papprox[min(n_success, PAPPROX_N) - 1]
    return None


def _depth_at(d, pos, win_begin):
    i = pos - win_begin
    return int(d[i]) if 0 <= i < len(d) else 0  # depth_buffer::val of an absent key


def signal_test(key, rates, depth1, win_begin, opt):
    """isCandidateIndelImplTestSignalNoise -> True, False or None (a sample reached the exact binomial before any said true)"""
    for s, d in enumerate(key["samples"]):
        n1 = len(d["ids"][TIER1])
        total = max(_depth_at(depth1[s], key["pos"] - 1, win_begin), n1)
        if total < 2:
            continue
        r = is_reject_null(total, rates[s][3], n1, opt["papprox"])
        if r is None:
            return None
        if r:
            return True
    return False


def weak_signal_test(key):
    """isCandidateIndelImplTestWeakSignal"""
    return any(len(d["ids"][TIER1]) >= 1 for d in key["samples"])


def depth_filter(key, depth1, depth2, win_begin, opt):
    """the max_depth test (:246-260) -> True when the key fails it"""
    if not opt["max_candidate_depth"] > 0.:
        return False
    total = 0.
    for s in range(len(key["samples"])):
        if opt["is_count_towards_depth_filter"][s]:
            total += _depth_at(depth1[s], key["pos"] - 1, win_begin) + _depth_at(depth2[s], key["pos"] - 1, win_begin)
    return total > opt["max_candidate_depth"]


def is_candidate(key, rates, bp_size, bp_size_certain, depth1, depth2, win_begin, opt):
    """isCandidateIndelImplTest -> (is_candidate, undecided)"""
    if key["flags"] & DO_NOT_GENOTYPE:
        return 0, DECIDED
    if key["flags"] & AR_PENDING:
        return 0, UNDECIDED_AR_PENDING
    if opt["is_haplotyping_enabled"] and key["active_region_id"] < 0:
        return 0, DECIDED
    signal = signal_test(key, rates, depth1, win_begin, opt) if opt["is_candidate_indel_signal_test"] else weak_signal_test(key)
    if signal is None:
        return 0, UNDECIDED_EXACT_BINOMIAL
    if not signal:
        return 0, DECIDED
    if key["type"] in (BP_LEFT, BP_RIGHT):
        if opt["min_candidate_indel_open_length"] > bp_size:
            return 0, DECIDED  # (every subset's maximum is below too)
        if not bp_size_certain:
            return 0, UNDECIDED_BP_OBS_ORDER
    if depth_filter(key, depth1, depth2, win_begin, opt):
        return 0, DECIDED
    return 1, DECIDED


def default_options(**fields):
    """sk_indel_candidate_options_default, as a dict"""
    opt = dict(papprox=[0.] * PAPPROX_N, log_indel_ref_error_factor=0.0, max_candidate_depth=-1.0, min_candidate_indel_open_length=20, is_indel_ref_error_factor=0,
               is_haplotyping_enabled=0, is_candidate_indel_signal_test=1, is_sample_specific_rates=0, is_count_towards_depth_filter=[1] * MAX_SAMPLES)
    opt.update(fields)
    return opt


def check_options(n_samples, opt):
    if not 1 <= n_samples <= MAX_SAMPLES:
        raise Refused("n_samples must be in 1..SK_MAX_SAMPLES")
    if not all(a < b for a, b in zip(opt["papprox"], opt["papprox"][1:])):
        raise Refused("papprox is not ascending")


def indel_candidates(keys, sample_obs, depth1, depth2, win_begin, rate_sets, opt):
    """keys: the table's records (tests/indel_table_model.py's indel_table); sample_obs: per sample the observations the table was made of
    [dict(type, pos, bp_len)]; depth1 / depth2: per sample the arrays over the window -> ([dict(is_candidate, undecided, bp_insert_size,
    rates [[4 doubles as bits] per sample])], [candidates, undecided])"""
    n_samples = len(sample_obs)
    check_options(n_samples, opt)
    for rs in rate_sets[:1 + (n_samples if opt["is_sample_specific_rates"] else 1)]:
        check_rate_set(rs)
    bp_lens = {}
    by_pos_type = {(k["pos"], k["type"]) for k in keys if k["type"] in (BP_LEFT, BP_RIGHT)}
    for obs in sample_obs:  # rule B
        for o in obs:
            if int(o["type"]) in (BP_LEFT, BP_RIGHT):
                if (int(o["pos"]), int(o["type"])) not in by_pos_type:
                    raise Refused("a breakpoint observation whose key the table lacks")
                bp_lens.setdefault((int(o["pos"]), int(o["type"])), []).append(int(o["bp_len"]))
    out, totals = [], [0, 0]
    for key in keys:
        assert len(key["samples"]) == n_samples
        rates = [error_rates(key, s, rate_sets, opt) for s in range(n_samples)]
        bp_size, certain = breakpoint_insert_size_batch(bp_lens.get((key["pos"], key["type"]), []))
        cand, undecided = is_candidate(key, rates, bp_size, certain, depth1, depth2, win_begin, opt)
        out.append(dict(is_candidate=cand, undecided=undecided, bp_insert_size=bp_size, rates=[[double_bits(x) for x in r] for r in rates]))
        totals[0] += cand
        totals[1] += int(undecided != DECIDED)
    return out, totals


# ---- the recorded scenes
@functools.lru_cache(maxsize=None)
def golden():
    """-> dict(configs {name: dict(options, papprox bits, log factor bits, rate sets as bits)}, scenes [dict(name, config, win_begin, n_pos, scene (an
    indel-table scene document, or table_scene: the name of one of tests/golden/indel_table, drop_regions: run without its regions), count_towards_depth, max_candidate_depth, depth
    [per sample [depth1, depth2] as (first position, values)], keys [dict(pos, type, del_len, ins, bp_insert_size, is_candidate, rates)])])"""
    with open(GOLDEN) as f:
        return json.load(f)


def config_options(cfg, sc):
    """a recorded configuration and scene -> (opt, rate_sets) in the model's form"""
    opt = default_options(papprox=[bits_double(b) for b in cfg["papprox"]], log_indel_ref_error_factor=bits_double(cfg["log_indel_ref_error_factor"]),
                          max_candidate_depth=float(sc["max_candidate_depth"]), min_candidate_indel_open_length=cfg["min_candidate_indel_open_length"],
                          is_indel_ref_error_factor=cfg["is_indel_ref_error_factor"], is_haplotyping_enabled=cfg["is_haplotyping_enabled"],
                          is_candidate_indel_signal_test=cfg["is_candidate_indel_signal_test"], is_sample_specific_rates=cfg["is_sample_specific_rates"],
                          is_count_towards_depth_filter=list(sc["count_towards_depth"]) + [1] * (MAX_SAMPLES - len(sc["count_towards_depth"])))
    sets = [[[(bits_double(i), bits_double(d)) for i, d in counts] for counts in rs] for rs in [cfg["candidate_rates"]] + cfg["sample_rates"]]
    return opt, sets


def scene_document(sc):
    """the indel-table scene a recorded scene runs on"""
    if "scene" in sc:
        return sc["scene"]
    from tests import indel_table_model as T
    return next(d for d in T.golden() if d["name"] == sc["table_scene"])


def dense_depth(recorded, win_begin, n_pos):
    """(first position, values) as recorded -> uint32[n_pos] over the window"""
    first, values = recorded
    d = np.zeros(n_pos, np.uint32)
    for j, v in enumerate(values):
        if 0 <= first + j - win_begin < n_pos:
            d[first + j - win_begin] = v
    return d


def run_recorded(sc):
    """a recorded scene through the models: the table (tests/indel_table_model.py), rule D, then rules E, B and C -> (keys, depth [(depth1, depth2) per
    sample], out, totals)"""
    from tests import indel_table_model as T
    doc = scene_document(sc)
    if sc.get("drop_regions"):
        doc = dict(doc, regions=[])
    samples, regions = T.scene_samples(doc)
    keys, _ = T.indel_table(doc["ref"], doc["ref_offset"], samples, regions, doc["prev_end_in"])
    depth = [depth_buffers(sm["reads"], sm["iat"], sc["win_begin"], sc["n_pos"]) for sm in samples]
    opt, sets = config_options(golden()["configs"][sc["config"]], sc)
    out, totals = indel_candidates(keys, [sm["obs"] for sm in samples], [d[0] for d in depth], [d[1] for d in depth], sc["win_begin"], sets, opt)
    return keys, depth, out, totals


def as_recorded(keys, out):
    """the model's keys and results in the form the driver writes them in"""
    assert all(o["undecided"] == DECIDED for o in out)
    return [dict(pos=k["pos"], type=k["type"], del_len=k["del_len"], ins=k["ins"], bp_insert_size=o["bp_insert_size"], is_candidate=o["is_candidate"], rates=o["rates"])
            for k, o in zip(keys, out)]


def depth_as_recorded(depth, sc):
    out = []
    for pair in depth:
        rows = []
        for d in pair:
            nz = np.flatnonzero(d)
            rows.append([sc["win_begin"], []] if len(nz) == 0 else [sc["win_begin"] + int(nz[0]), [int(v) for v in d[nz[0]:nz[-1] + 1]]])
        out.append(rows)
    return out
