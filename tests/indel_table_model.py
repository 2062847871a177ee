"""Loop-by-loop model of the indel table (sk_indel_table, csrc/indel_table.hip): the reference's IndelBuffer
(std::map<IndelKey, IndelData>, L/starling_common/IndelBuffer.cpp) after every read observation of a call has been added and the call's
regions have then been closed in order -- region by region and, inside a region, sample by sample (ActiveRegionDetector.cpp:204-250).
One function per rule of the header's block; the map is a Python dict and the steps run one after the other, as the reference's do.

Input (`table`):
  samples   [dict(reads [dict(code, pos, path)], obs [INTAKE_OBS_DTYPE records or dicts of the same fields], align_id [ids] or None,
                  iat [0 | 1 | 2], hap [tests/haplotype_model.py's region records], alleles [tests/alleles_model.py's region records])]
  regions   [(begin, end)] shared by every sample; prev_end_in as sk_region_alleles took it
Output: (keys in IndelKey::operator< order, totals [keys, ids, insert bytes, pending pairs]); floats as their bits.

Imports neither the product nor a device."""
import functools
import json
import os

import numpy as np

from tests import haplotype_model as H
from tests import intake_model as M

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "indel_table", "indel_table_golden.json")

NONE, INDEL, MISMATCH, BP_LEFT, BP_RIGHT = range(5)  # INDEL::index_t (SK_INDEL_*)
TIER1, TIER2, SUBMAP, NOISE = range(4)  # SK_ITAB_*: the id sets; the first three are INDEL_ALIGN_TYPE's values too
DO_NOT_GENOTYPE, AR_PENDING = 1, 2  # SK_ITAB_* flags
IT_INSERT, IT_DELETE, IT_SWAP, IT_BREAKPOINT, IT_OTHER = range(5)  # SimplifiedIndelReportType::index_t
MAX_SAMPLES = 8
PENDING_STATUSES = (H.NO_READS, H.TOO_FEW_COVERING, H.DECLINED)


class Refused(Exception):
    pass


def float_bits(x):
    return int(np.array([x], np.float32).view(np.uint32)[0])


def bits_float(b):
    return np.array([b], np.uint32).view(np.float32)[0]


# ---- rule 1: key identity and order (IndelKey.hh:56-85)
def is_breakpoint(key):
    return key[1] in (BP_LEFT, BP_RIGHT)


def make_key(pos, indel_type, del_len, ins):
    """breakpoint keys compare no further than (pos, type): all breakpoint observations of one (pos, type) are one key"""
    return (int(pos), int(indel_type), 0, "") if indel_type in (BP_LEFT, BP_RIGHT) else (int(pos), int(indel_type), int(del_len), ins)


def key_order(key):
    """operator<: pos, type, then insert length, delete length, insertSequence as std::string::operator< -- ASCII, A < C < G < N < T"""
    pos, indel_type, del_len, ins = key
    return (pos, indel_type, len(ins), del_len, ins.encode("latin-1"))


def _new_data(n_samples):
    return dict(active_region_id=-1, flags=0, n_bp_obs=0, has_read_obs=False, first_region_step=None,
                samples=[dict(ids=[set(), set(), set(), set()], haplotype_id=0, is_haplotyping_bypassed=0, ratio=np.float32(0.0)) for _ in range(n_samples)])


def _find_or_insert(table, key):
    """IndelBuffer::addIndelObservation's find / insert (:105-129) with rule 4 on a novel key"""
    data = table["map"].get(key)
    if data is None:
        data = table["map"][key] = _new_data(table["n_samples"])
        if do_not_genotype(key):
            data["flags"] |= DO_NOT_GENOTYPE
    return data


# ---- rule 2: addIndelObservation from reads (IndelBuffer.cpp:95-133, IndelData.cpp:72-114, 182-215)
def add_read_observations(table, s, sample):
    reads = sample["reads"]
    for o in sample["obs"]:
        r = int(o["read"])
        if not 0 <= r < len(reads):
            raise Refused("an observation names a read outside the sample")
        code = reads[r]["code"]
        b, n = int(o["ins_begin"]), int(o["ins_len"])
        if b + n > len(code):
            raise Refused("an observation's insert lies outside its read")
        if int(o["type"]) not in (INDEL, BP_LEFT, BP_RIGHT):
            raise Refused("an observation of a type the intake does not make")
        ins = "".join(M.read_char(code, i) for i in range(b, b + n))
        key = make_key(o["pos"], int(o["type"]), o["deletion_length"], ins)
        data = _find_or_insert(table, key)
        data["has_read_obs"] = True
        if is_breakpoint(key):
            data["n_bp_obs"] += 1
        which = NOISE if int(o["is_noise"]) else _iat(sample, r)
        data["samples"][s]["ids"][which].add(_align_id(sample, r))


def _iat(sample, r):
    iat = int(sample["iat"][r])
    if iat > SUBMAP:
        raise Refused("an iat above 2")
    return iat


def _align_id(sample, r):
    return int(sample["align_id"][r]) if sample.get("align_id") is not None else r


# ---- rule 4: doNotGenotype (IndelBuffer.cpp:119-128, IndelKey.hh:146-161)
def do_not_genotype(key):
    pos, indel_type, del_len, ins = key
    primitive = indel_type == MISMATCH or (indel_type == INDEL and ((ins and del_len == 0) or (not ins and del_len > 0)))
    return not primitive


# ---- rule 5: the report info (AlleleReportInfoUtil.cpp:96-216)
def get_seq_repeat_unit(seq):
    """L/blt_util/seq_util.cpp:125-164 -> (unit, count): the smallest perfect repeat"""
    n = len(seq)
    for i in range(1, n):
        if n % i == 0 and all(seq[j] == seq[j % i] for j in range(i, n)):
            return seq[:i], n // i
    return seq, 1


def interrupted_homopolymer_length(ref, ref_offset, pos):
    """getInterruptedHomopolymerLength (L/blt_common/ref_context.cpp:237-272) with ihpol_data (:183-232)"""
    get_base = lambda p: M.ref_char(ref, ref_offset, p)
    rs = ref_offset + len(ref)  # ref.end()

    def walk(first, second):
        r = ["N", "N"]
        nr = [0, 0]
        for rng in (first, second):
            for i in rng:
                b = get_base(i)
                if nr[0] == 0:
                    r[0], nr[0] = b, 1
                elif r[0] == b:
                    if nr[1] > 1 or r[0] == "N":
                        break
                    nr[0] += 1
                elif nr[1] == 0:
                    r[1], nr[1] = b, 1
                elif r[1] == b:
                    if nr[0] > 1 or r[1] == "N":
                        break
                    nr[1] += 1
                else:
                    break
        return max(nr)
    up = walk(range(pos, -1, -1), range(pos + 1, rs))
    dn = walk(range(pos, rs), range(pos - 1, -1, -1))
    return max(up, dn)


def report_info(ref, ref_offset, key):
    pos, indel_type, del_len, ins = key
    get_base = lambda p: M.ref_char(ref, ref_offset, p)
    if indel_type == INDEL and not ins and del_len > 0:  # SimplifiedIndelReportType::getRateType (AlleleReportInfo.hh:47-72)
        it = IT_DELETE
    elif indel_type == INDEL and ins and del_len == 0:
        it = IT_INSERT
    elif indel_type == INDEL:
        it = IT_SWAP
    elif is_breakpoint(key):
        it = IT_BREAKPOINT
    else:
        it = IT_OTHER
    right_pos = pos + del_len
    info = dict(it=it, repeat_unit_len=0, ref_repeat_count=0, indel_repeat_count=0)
    unit = None
    insert_count = delete_count = 0
    deleted = "".join(get_base(p) for p in range(pos, right_pos))
    if it == IT_INSERT:
        unit, insert_count = get_seq_repeat_unit(ins)
    elif it == IT_DELETE:
        unit, delete_count = get_seq_repeat_unit(deleted)
    elif it == IT_SWAP:
        insert_ru, insert_count = get_seq_repeat_unit(ins)
        delete_ru, delete_count = get_seq_repeat_unit(deleted)
        if insert_ru == delete_ru and insert_ru:  # :134
            unit = insert_ru
    if unit is not None:
        n = len(unit)
        info["repeat_unit_len"] = n
        context = 0
        i = pos - n
        while i >= 0 and n > 0 and all(get_base(i + j) == unit[j] for j in range(n)):  # upstream :152-165
            context += 1
            i -= n
        rs = ref_offset + len(ref)
        i = right_pos
        while n > 0 and i + n - 1 < rs and all(get_base(i + j) == unit[j] for j in range(n)):  # downstream, stopping at ref.end() :168-182
            context += 1
            i += n
        info["ref_repeat_count"] = context + delete_count
        info["indel_repeat_count"] = context + insert_count
    info["interrupted_hpol_len"] = max(interrupted_hpol_probes(ref, ref_offset, key))
    return info


def interrupted_hpol_probes(ref, ref_offset, key):
    """getInterruptedHomopolymerLength at the positions getAlleleReportInfo probes (:205-215): pos - 1, pos and, where the key deletes
    anything, right_pos - 1 and right_pos"""
    pos, right_pos = key[0], key[0] + key[2]
    probes = [pos - 1, pos] + ([right_pos - 1, right_pos] if right_pos != pos else [])
    return [interrupted_homopolymer_length(ref, ref_offset, p) for p in probes]


# ---- rules 3 and 6: a counted (region, sample) (ActiveRegionProcessor.cpp:709-757)
def add_region_records(table, s, sample, region_index, begin, step):
    hap_rec, rec = sample["hap"][region_index], sample["alleles"][region_index]
    for a in rec["alleles"]:
        if not a["to_indel_buffer"]:  # :731 (a MISMATCH record under doNotAddMismatchesToIndelBuffer creates no key)
            continue
        if not 0 <= a["hap_slot"] < len(hap_rec["haps"]):
            raise Refused("a record names a haplotype its region did not select")
        key = make_key(a["pos"], a["type"], a["del_len"], a["ins"])
        data = _find_or_insert(table, key)
        for r in hap_rec["haps"][a["hap_slot"]]["support"]:  # rule 3: never noise (:736-739); a set, so twice is once
            if not 0 <= r < len(sample["reads"]):
                raise Refused("a support list names a read outside the sample")
            data["samples"][s]["ids"][_iat(sample, r)].add(_align_id(sample, r))
        if data["first_region_step"] is None:
            data["first_region_step"] = step
        data["active_region_id"] = begin  # rule 6 (:745)
        d = data["samples"][s]
        d["haplotype_id"] += a["haplotype_id"]  # :750
        d["ratio"] = np.float32(d["ratio"] + bits_float(a["ratio"]))  # :755, ordered float additions


# ---- rule 7: doNotUseHaplotyping's marks (ActiveRegionProcessor.cpp:265-292)
def mark_bypassed(table, s, begin, end):
    for key, data in table["map"].items():  # (every key in the map exists at this step: the steps run in order)
        if begin <= key[0] < end and not is_breakpoint(key) and key[1] != MISMATCH:
            data["active_region_id"] = begin
            data["samples"][s]["is_haplotyping_bypassed"] = 1


# ---- rule 8: the pairs whose outcome is not known
def is_pending(hap_rec, rec):
    return hap_rec["status"] in PENDING_STATUSES or rec["status"] == H.DECLINED


def mark_pending(table, pending):
    for begin, end, prev_end in pending:
        lo = min(begin, max(prev_end, 0))
        for key, data in table["map"].items():
            if lo <= key[0] < end:
                data["flags"] |= AR_PENDING


# ---- rule 9: what the entry refuses before it looks at a record
def check(samples, regions):
    if not 1 <= len(samples) <= MAX_SAMPLES:
        raise Refused("n_samples outside 1..SK_MAX_SAMPLES")
    for sample in samples:
        if len(sample["hap"]) != len(regions) or len(sample["alleles"]) != len(regions):
            raise Refused("a sample's region records are not the shared list's")
        for r in range(len(sample["reads"])):
            _iat(sample, r)


def indel_table(ref, ref_offset, samples, regions, prev_end_in=-1, counts=None):
    """-> ([dict(pos, type, del_len, ins, active_region_id, flags, n_bp_obs, it, repeat_unit_len, ref_repeat_count, indel_repeat_count,
    interrupted_hpol_len, samples [dict(ids [[tier1], [tier2], [submap], [noise]], haplotype_id, is_haplotyping_bypassed, ratio)])],
    totals).  counts: a dict that receives what rule_counts counts"""
    check(samples, regions)
    table = dict(map={}, n_samples=len(samples))
    note = counts if counts is not None else {}
    for s, sample in enumerate(samples):
        add_read_observations(table, s, sample)
    pending = []
    prev_end = prev_end_in
    for i, (begin, end) in enumerate(regions):
        for s, sample in enumerate(samples):
            step = i * len(samples) + s
            hap_rec, rec = sample["hap"][i], sample["alleles"][i]
            if is_pending(hap_rec, rec):
                pending.append((int(begin), int(end), prev_end))
            elif hap_rec["status"] == H.BYPASSED:
                before = sum(d["samples"][s]["is_haplotyping_bypassed"] for d in table["map"].values())
                mark_bypassed(table, s, int(begin), int(end))
                note["bypass_marks"] = note.get("bypass_marks", 0) + sum(d["samples"][s]["is_haplotyping_bypassed"] for d in table["map"].values()) - before
            else:
                add_region_records(table, s, sample, i, int(begin), step)
        prev_end = int(end)
    mark_pending(table, pending)
    out = []
    n_ids = n_ins = 0
    for key in sorted(table["map"], key=key_order):
        data = table["map"][key]
        rec = dict(pos=key[0], type=key[1], del_len=key[2], ins=key[3], active_region_id=data["active_region_id"], flags=data["flags"], n_bp_obs=data["n_bp_obs"])
        rec.update(report_info(ref, ref_offset, key))
        rec["samples"] = [dict(ids=[sorted(x) for x in d["ids"]], haplotype_id=d["haplotype_id"], is_haplotyping_bypassed=d["is_haplotyping_bypassed"],
                               ratio=float_bits(d["ratio"])) for d in data["samples"]]
        n_ids += sum(len(x) for d in data["samples"] for x in d["ids"])
        n_ins += len(key[3])
        out.append(rec)
    return out, [len(out), n_ids, n_ins, len(pending)]


# The rules a set of recorded vectors has to exercise
RULES = ("rule1_same_pos_different_type", "rule1_insert_length_before_delete_length", "rule1_insert_sequences_differ", "rule2_tier1", "rule2_tier2", "rule2_submap",
         "rule2_noise", "rule2_breakpoint", "rule3_region_ids", "rule3_id_twice", "rule3_mismatch_not_added", "rule4_do_not_genotype", "rule5_insert_repeat",
         "rule5_delete_repeat", "rule5_swap", "rule5_interrupted_hpol", "rule5_ihpol_decided_by_pos_minus_1", "rule5_ihpol_decided_by_pos",
         "rule5_ihpol_decided_by_right_minus_1", "rule5_ihpol_decided_by_right", "rule6_id_3", "rule6_two_samples", "rule7_bypass_marks", "rule7_not_marked_later_key")


def rule_counts(results):
    """results: [(samples, regions, keys as indel_table returns them, ref, ref_offset)] -> how many keys (or scenes) exercise each rule of
    RULES.  "decided by": that probe alone gives the interrupted homopolymer's maximum, so leaving it out would change the field"""
    n = dict.fromkeys(RULES, 0)
    for samples, regions, keys, ref, ref_offset in results:
        for a, b in zip(keys, keys[1:]):
            same_pos = a["pos"] == b["pos"]
            n["rule1_same_pos_different_type"] += same_pos and a["type"] != b["type"]
            both = same_pos and a["type"] == b["type"] == INDEL
            n["rule1_insert_length_before_delete_length"] += both and len(a["ins"]) < len(b["ins"]) and a["del_len"] > b["del_len"]
            n["rule1_insert_sequences_differ"] += both and len(a["ins"]) == len(b["ins"]) and a["del_len"] == b["del_len"]
        region_ids = {}
        for s, sample in enumerate(samples):
            for i, rec in enumerate(sample["alleles"]):
                for a in rec["alleles"]:
                    if a["to_indel_buffer"]:
                        ids = set(_align_id(sample, r) for r in sample["hap"][i]["haps"][a["hap_slot"]]["support"])
                        region_ids.setdefault((make_key(a["pos"], a["type"], a["del_len"], a["ins"]), s), set()).update(ids)
                    else:
                        n["rule3_mismatch_not_added"] += 1
        bypassed_steps = [(i, s) for i in range(len(regions)) for s, sample in enumerate(samples) if sample["hap"][i]["status"] == H.BYPASSED]
        for k in keys:
            key = (k["pos"], k["type"], k["del_len"], k["ins"])
            for which, name in ((TIER1, "rule2_tier1"), (TIER2, "rule2_tier2"), (SUBMAP, "rule2_submap"), (NOISE, "rule2_noise")):
                n[name] += any(d["ids"][which] for d in k["samples"])
            n["rule2_breakpoint"] += k["n_bp_obs"] > 0
            n["rule3_region_ids"] += any((key, s) in region_ids for s in range(len(samples)))
            for s, sample in enumerate(samples):
                own = set(_align_id(sample, int(o["read"])) for o in sample["obs"] if not int(o["is_noise"]) and
                          make_key(o["pos"], int(o["type"]), o["deletion_length"],
                                   "".join(M.read_char(sample["reads"][int(o["read"])]["code"], j) for j in range(int(o["ins_begin"]), int(o["ins_begin"]) + int(o["ins_len"])))) == key)
                n["rule3_id_twice"] += bool(own & region_ids.get((key, s), set()))
            n["rule4_do_not_genotype"] += bool(k["flags"] & DO_NOT_GENOTYPE)
            n["rule5_insert_repeat"] += k["it"] == IT_INSERT and k["indel_repeat_count"] > 1
            n["rule5_delete_repeat"] += k["it"] == IT_DELETE and k["ref_repeat_count"] > 1
            n["rule5_swap"] += k["it"] == IT_SWAP
            n["rule5_interrupted_hpol"] += k["interrupted_hpol_len"] > 1
            probes = interrupted_hpol_probes(ref, ref_offset, key)
            for which, name in enumerate(("pos_minus_1", "pos", "right_minus_1", "right")[:len(probes)]):
                n["rule5_ihpol_decided_by_" + name] += len(probes) == 4 and probes[which] > max(probes[:which] + probes[which + 1:])
            n["rule6_id_3"] += any(d["haplotype_id"] == 3 for d in k["samples"])
            n["rule6_two_samples"] += sum(1 for d in k["samples"] if d["haplotype_id"]) >= 2
            n["rule7_bypass_marks"] += any(d["is_haplotyping_bypassed"] for d in k["samples"])
            for i, s in bypassed_steps:
                inside = regions[i][0] <= k["pos"] < regions[i][1] and k["type"] == INDEL
                n["rule7_not_marked_later_key"] += inside and not k["samples"][s]["is_haplotyping_bypassed"]
    return n


@functools.lru_cache(maxsize=None)
def golden():
    """-> the recorded scenes: [dict(name, ref, ref_offset, max_indel_size, samples [dict(reads, low, fwd, align_id, iat, buf_begin, buf_end)],
    regions [dict(begin, end, ploidy [per sample])], prev_end_in, keys [the reference's map, in its order], assembled)]"""
    with open(GOLDEN) as f:
        return json.load(f)["scenes"]


def scene_samples(sc, max_hap_len=1024):
    """a recorded scene -> (the samples indel_table takes, regions): the chain's models run sample by sample -- the intake
    (tests/intake_model.py), the region haplotypes (tests/haplotype_model.py), the region alleles (tests/alleles_model.py)"""
    from tests import alleles_model as A
    regions = [(int(b), int(e)) for b, e in sc["regions"]]
    samples = []
    for s, sm in enumerate(sc["samples"]):
        reads = [dict(code=M.encode(r["seq"]), pos=r["pos"], path=[tuple(t) for t in r["path"]]) for r in sm["reads"]]
        low = [r["low_mapq"] for r in sm["reads"]]
        fwd = [r["is_fwd"] for r in sm["reads"]]
        intake = M.read_intake(sc["ref"], sc["ref_offset"], reads, low, 0, 0, sc["max_indel_size"])
        hap = H.region_haplotypes(sc["ref"], sc["ref_offset"], reads, low, fwd, regions, sm["buf_begin"], sm["buf_end"], sc["ploidy"][s], sc["max_indel_size"])
        alleles, _ = A.region_alleles(sc["ref"], sc["ref_offset"], regions, hap, sc["max_indel_size"], max_hap_len, sc["prev_end_in"])
        samples.append(dict(reads=reads, low=low, fwd=fwd, obs=intake["obs"], align_id=[r["id"] for r in sm["reads"]], iat=[r["iat"] for r in sm["reads"]], hap=hap,
                            alleles=alleles, buf_begin=sm["buf_begin"], buf_end=sm["buf_end"], ploidy=sc["ploidy"][s]))
    return samples, regions


def as_recorded(keys):
    """indel_table's keys in the form the driver writes the reference's map in"""
    out = []
    for k in keys:
        assert not k["flags"] & AR_PENDING
        out.append(dict(pos=k["pos"], type=k["type"], del_len=k["del_len"], ins=k["ins"], active_region_id=k["active_region_id"],
                        do_not_genotype=int(bool(k["flags"] & DO_NOT_GENOTYPE)), it=k["it"], repeat_unit_len=k["repeat_unit_len"], ref_repeat_count=k["ref_repeat_count"],
                        indel_repeat_count=k["indel_repeat_count"], interrupted_hpol_len=k["interrupted_hpol_len"],
                        samples=[dict(tier1=d["ids"][TIER1], tier2=d["ids"][TIER2], submap=d["ids"][SUBMAP], noise=d["ids"][NOISE], haplotype_id=d["haplotype_id"],
                                      ratio=d["ratio"], is_haplotyping_bypassed=d["is_haplotyping_bypassed"]) for d in k["samples"]]))
    return out
