"""Loop model of the realignment gate (sk_realign_gate; csrc/realign_gate.hip): the header's rules G1-G5, one function each, in plain Python.
L/ is the reference's src/c++/lib/.

  rule G1  log_rates              LogValuePair::updateValue (L/blt_util/LogValuePair.hh:44-48) over what initializeAuxInfo stores
                                  (L/starling_common/IndelData.cpp:153-154)
  rule G2  unaligned_prefix, unaligned_suffix, ref_length, is_overmax, alignment_zone, cheap_tests
                                  (L/blt_util/align_path.cpp:190-214, L/starling_common/alignment.cpp:32-50, alignment_util.cpp:59-85,
                                  starling_read_align.cpp:2045-2050)
  rule G3  range_iterator, intersects_breakpoints, gate
                                  (L/starling_common/IndelBuffer.cpp:76-92, indel_util.cpp:48-63, starling_read_align.cpp:217-270)
  rule G4  consulted              the keys whose candidate status the gates asked for (L/starling_common/IndelBuffer.hh:153-164)
  rule G5  observed_lists         is_usable_indel's set-membership half (starling_read_align.cpp:289-305)

Built on tests/indel_table_model.py (the keys) and tests/indel_candidates_model.py (candidacy and the rates).  Imports nothing from the
library.  Pinned to vectors recorded from the reference's own classes by tests/test_realign_gate_model.py."""
import functools
import json
import math
import os

from tests import indel_candidates_model as CM

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "realign_gate", "realign_gate_golden.json")

NONE, PASS, OVERMAX, OUTSIDE_RANGE, NO_CANDIDATE, UNDECIDED, SPLICED = range(7)  # SK_RGATE_*
SORT_CAP = 64  # SK_RGATE_SORT_CAP
UNALIGNED_EDGE = (CM.SEG_INSERT, CM.SEG_HARD_CLIP, CM.SEG_SOFT_CLIP)                         # is_segment_type_unaligned_read_edge
READ_LENGTH = (CM.SEG_MATCH, CM.SEG_SEQ_MATCH, CM.SEG_SEQ_MISMATCH, CM.SEG_INSERT, CM.SEG_SOFT_CLIP)  # is_segment_type_read_length
REF_LENGTH = (CM.SEG_MATCH, CM.SEG_SEQ_MATCH, CM.SEG_SEQ_MISMATCH, CM.SEG_DELETE, CM.SEG_SKIP)        # is_segment_type_ref_length


class Refused(Exception):
    pass


# ---- rule G1
def log_rates(rate_bits):
    """the four rates of a (key, sample) as bits -> (ref_to_indel_log_prob, indel_to_ref_log_prob) as bits: std::log; log(0.) is -inf"""
    out = []
    for b in rate_bits[:2]:
        x = CM.bits_double(b)
        out.append(CM.double_bits(-math.inf if x == 0. else math.log(x)))
    return out


# ---- rule G2
def unaligned_prefix(path):
    """unalignedPrefixSize"""
    v = 0
    for t, length in path:
        if t not in UNALIGNED_EDGE:
            return v
        if t in READ_LENGTH:
            v += length
    return v


def unaligned_suffix(path):
    """unalignedSuffixSize"""
    return unaligned_prefix(path[::-1])


def ref_length(path):
    """apath_ref_length"""
    return sum(length for t, length in path if t in REF_LENGTH)


def is_overmax(path, max_indel_size):
    """alignment::is_overmax: the first and the last segment are skipped"""
    for i, (t, length) in enumerate(path):
        if i == 0 or i + 1 == len(path):
            continue
        if t in (CM.SEG_INSERT, CM.SEG_DELETE) and length > max_indel_size:
            return True
    return False


def alignment_zone(pos, path, read_len):
    """get_alignment_zone over get_alignment_range, the clamp at 0 included"""
    begin = pos - unaligned_prefix(path)
    end = pos + ref_length(path) + unaligned_suffix(path)
    return max(0, min(begin, end - read_len)), max(end, begin + read_len)


def cheap_tests(read, zone, max_indel_size):
    """what decides before any key is looked at -> SPLICED, OVERMAX, OUTSIDE_RANGE or None"""
    if any(t == CM.SEG_SKIP for t, _ in read["path"]):
        return SPLICED
    if is_overmax(read["path"], max_indel_size):
        return OVERMAX
    if not (read["realign"][0] <= zone[0] and zone[1] <= read["realign"][1]):  # known_pos_range::is_superset_of
        return OUTSIDE_RANGE
    return None


# ---- rule G3
def right_pos(key):
    return key["pos"] + key["del_len"]


def range_iterator(keys, begin_pos, end_pos, max_indel_size):
    """IndelBuffer::rangeIterator over keys in key order -> (lo, hi)"""
    hi = 0
    while hi < len(keys) and keys[hi]["pos"] < end_pos:  # lower_bound(IndelKey(end_pos)): type NONE sorts first
        hi += 1
    lo = 0
    while lo < len(keys) and keys[lo]["pos"] < begin_pos - max_indel_size:
        lo += 1
    while lo < hi:
        if right_pos(keys[lo]) >= begin_pos:
            break
        lo += 1
    return min(lo, hi), hi


def _point_intersects(zone, p):
    """known_pos_range::is_range_intersect(pos_range(p, p))"""
    return p > zone[0] and p < zone[1]


def intersects_breakpoints(zone, key):
    """is_range_intersect_indel_breakpoints"""
    if key["type"] == CM.MISMATCH:
        return zone[0] <= key["pos"] < zone[1]
    if _point_intersects(zone, key["pos"]):
        return True
    if key["pos"] == right_pos(key):
        return False
    return _point_intersects(zone, right_pos(key))


def gate(keys, cand, zone, max_indel_size):
    """check_for_candidate_indel_overlap's loop -> (status, the key indices whose candidate status it asked for, asked_undecided)"""
    lo, hi = range_iterator(keys, zone[0], zone[1], max_indel_size)
    asked, asked_undecided = [], False
    for k in range(lo, hi):
        if not intersects_breakpoints(zone, keys[k]):
            continue
        asked.append(k)
        if cand[k]["undecided"] != CM.DECIDED:  # asked, and the loop goes on: the answer is not known
            asked_undecided = True
            continue
        if cand[k]["is_candidate"]:
            return PASS, asked, asked_undecided
    return (UNDECIDED if asked_undecided else NO_CANDIDATE), asked, asked_undecided


# ---- rule G4
def consulted(n_keys, asked_lists):
    out = [0] * n_keys
    for asked in asked_lists:
        for k in asked:
            out[k] = 1
    return out


# ---- rule G5
def observed_lists(keys, sample, align_ids):
    """per read of the sample the key indices one of whose four id sets holds the read's align id: ascending, each once"""
    by_id = {a: r for r, a in enumerate(align_ids)}
    out = [[] for _ in align_ids]
    for k, key in enumerate(keys):
        members = set()
        for ids in key["samples"][sample]["ids"]:
            for a in ids:
                if a not in by_id:
                    raise Refused("an id that belongs to none of the sample's reads")
                members.add(a)
        for a in sorted(members):
            out[by_id[a]].append(k)
    return out


def realign_gate(keys, cand, samples, max_indel_size):
    """keys: the table's records; cand: indel_candidates' records; samples: [dict(reads [dict(pos, path, read_len, realign (begin, end))], align_id
    (None: the reads' indices))] -> dict(keys [dict(pos, type, del_len, ins, active_region_id, is_candidate, undecided, gate_consulted, haplotype_id,
    is_haplotyping_bypassed, logs [[2 doubles as bits] per sample])], samples [dict(reads [dict(zone, status, asked_undecided)], observed, asked [per read the
    key indices its gate asked for: what the device folds into gate_consulted])], totals)"""
    n_samples = len(samples)
    if not 1 <= n_samples <= CM.MAX_SAMPLES:
        raise Refused("n_samples must be in 1..SK_MAX_SAMPLES")
    out_samples, asked_lists, totals = [], [], [0, 0] + [0] * CM.MAX_SAMPLES
    for s, sm in enumerate(samples):
        ids = list(range(len(sm["reads"]))) if sm.get("align_id") is None else [int(a) for a in sm["align_id"]]
        if any(not a < b for a, b in zip(ids, ids[1:])):
            raise Refused("align_id is not strictly ascending")
        reads = []
        for rd in sm["reads"]:
            if any(not 0 <= t <= CM.SEG_SEQ_MISMATCH for t, _ in rd["path"]):
                raise Refused("a segment type above SK_SEG_SEQ_MISMATCH")
            zone = alignment_zone(rd["pos"], rd["path"], rd["read_len"])
            status, asked, asked_undecided = cheap_tests(rd, zone, max_indel_size), [], False
            if status is None:
                status, asked, asked_undecided = gate(keys, cand, zone, max_indel_size)
            asked_lists.append(asked)
            reads.append(dict(zone=list(zone), status=status, asked_undecided=int(asked_undecided)))
            totals[0] += status == PASS
            totals[1] += status == UNDECIDED
        observed = observed_lists(keys, s, ids)
        totals[2 + s] = sum(len(o) for o in observed)
        out_samples.append(dict(reads=reads, observed=observed, asked=asked_lists[len(asked_lists) - len(reads):]))
    marks = consulted(len(keys), asked_lists)
    out_keys = []
    for k, (key, c) in enumerate(zip(keys, cand)):
        hap = [int(d["haplotype_id"]) for d in key["samples"]] + [0] * (CM.MAX_SAMPLES - n_samples)
        byp = [int(d["is_haplotyping_bypassed"] != 0) for d in key["samples"]] + [0] * (CM.MAX_SAMPLES - n_samples)
        out_keys.append(dict(pos=key["pos"], type=key["type"], del_len=key["del_len"], ins=key["ins"], active_region_id=key["active_region_id"], is_candidate=c["is_candidate"],
                             undecided=c["undecided"], gate_consulted=marks[k], haplotype_id=hap, is_haplotyping_bypassed=byp, logs=[log_rates(r) for r in c["rates"]]))
    return dict(keys=out_keys, samples=out_samples, totals=totals)


# ---- the recorded scenes
KEY_FIELDS = ("pos", "type", "del_len", "ins", "is_candidate", "active_region_id", "logs", "haplotype_id", "is_haplotyping_bypassed")
READ_FIELDS = ("sample", "id", "zone", "realignable", "gate", "consulted", "member")


@functools.lru_cache(maxsize=None)
def golden():
    """-> dict(scenes [dict(name, candidate_scene (the name of a scene of tests/golden/indel_candidates) or scene (one in that file's form), ranges [[sample,
    read id, begin, end]], keys [dict(pos, type, del_len, ins, is_candidate, active_region_id, logs, haplotype_id, is_haplotyping_bypassed)], reads [dict(sample,
    id, zone, range, realignable, gate, consulted [key indices], member [key indices])])])"""
    with open(GOLDEN) as f:
        doc = json.load(f)
    for sc in doc["scenes"]:  # (the file keeps keys and reads as rows, in the order of KEY_FIELDS and READ_FIELDS)
        sc["keys"] = [dict(zip(KEY_FIELDS, row)) for row in sc["keys"]]
        sc["reads"] = [dict(zip(READ_FIELDS, row)) for row in sc["reads"]]
    return doc


def candidate_scene(rec):
    """the indel-candidates scene a recorded scene runs on"""
    if "scene" in rec:
        return rec["scene"]
    return next(sc for sc in CM.golden()["scenes"] if sc["name"] == rec["candidate_scene"])


def gate_samples(doc, ranges):
    """an indel-table scene document and the recorded ranges -> the samples realign_gate takes"""
    by_read = {(s, i): (b, e) for s, i, b, e in ranges}
    return [dict(reads=[dict(pos=r["pos"], path=[tuple(t) for t in r["path"]], read_len=len(r["seq"]), realign=by_read.get((s, r["id"]), (0, 1 << 30))) for r in sm["reads"]],
                 align_id=[r["id"] for r in sm["reads"]]) for s, sm in enumerate(doc["samples"])]


def run_recorded(rec):
    """a recorded scene through the models: the table, the depth buffers and candidacy (tests/indel_candidates_model.py's run_recorded), then rules G1-G5
    -> (keys, candidacy records, samples, realign_gate's result)"""
    sc = candidate_scene(rec)
    keys, _, cand, _ = CM.run_recorded(sc)
    doc = CM.scene_document(sc)
    samples = gate_samples(doc, rec["ranges"])
    return keys, cand, samples, realign_gate(keys, cand, samples, doc["max_indel_size"])


def as_recorded(doc, out):
    """realign_gate's result in the form the driver writes: (keys, reads in the driver's order: by position, sample, id)"""
    n_samples = len(out["samples"])
    keys = [dict(pos=k["pos"], type=k["type"], del_len=k["del_len"], ins=k["ins"], is_candidate=k["is_candidate"], active_region_id=k["active_region_id"], logs=k["logs"],
                 haplotype_id=k["haplotype_id"][:n_samples], is_haplotyping_bypassed=k["is_haplotyping_bypassed"][:n_samples]) for k in out["keys"]]
    assert all(k["undecided"] == CM.DECIDED for k in out["keys"])
    reads = []
    for s, (sm, so) in enumerate(zip(doc["samples"], out["samples"])):
        for r, rd in enumerate(sm["reads"]):
            g = so["reads"][r]
            assert g["status"] != SPLICED
            reads.append((rd["pos"], s, rd["id"], dict(sample=s, id=rd["id"], zone=g["zone"], realignable=int(g["status"] != OVERMAX), gate=int(g["status"] == PASS),
                                                      consulted=so["asked"][r], member=so["observed"][r])))
    return keys, [x[3] for x in sorted(reads, key=lambda x: x[:3])]
