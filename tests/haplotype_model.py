"""Loop-by-loop model of what the reference's active-region detector keeps per read and what it does with it first: the per-(read,
position) store (ActiveRegionReadBuffer::insertMatch / insertMismatch / insertSoftClipSegment / insertIndel,
L/starling_common/ActiveRegionReadBuffer.cpp:26-141, as addAlignmentIndelsToPosProcessor calls them,
L/starling_common/starling_pos_processor_indel_util.cpp:428-481), getHaplotypeBase (:143-171), getReadSegments (:191-256) with
includePartialReads = false and minReadSegmentLength = 1, and ActiveRegionProcessor's counting path
(L/starling_common/ActiveRegionProcessor.cpp: processHaplotypes' range and size check :45-56, generateHaplotypesWithCounting :79-114,
the phasing-noise filter :296-414, selectHaplotypes / selectOrDropHaplotypesWithSameCount :416-516).

The store is kept under the true (read, position) pair; the reference keeps it under (id % 1000, pos % 1000) and never clears it, so
where two pairs of one region could share a slot the answer is DECLINED (the decline rules below), never a guess.  Imports neither the
product nor a device."""
import numpy as np

from tests import intake_model as M

MAX_REF_SPAN_TO_BYPASS_ASSEMBLY = 250    # ActiveRegionProcessor.hh (MaxRefSpanToBypassAssembly)
MIN_FRAC_READS_COVERING_REGION = 0.65    # MinFracReadsCoveringRegion (a float)
MIN_HAPLOTYPE_COUNT = 3                  # MinHaplotypeCount
MIN_PHASE_ERROR_HPOL_SIZE = 10           # ActiveRegionProcessor.cpp:338
MAX_DEPTH = 1000                         # ActiveRegionReadBuffer::MaxDepth (.hh:65)
MAX_BUFFER_SIZE = 1000                   # ActiveRegionReadBuffer::MaxBufferSize (.hh:61)
MAX_GROUPS = 16                          # libstdc++'s std::sort is a plain insertion sort up to 16 elements (_S_threshold)

MATCH, MISMATCH, SOFT_CLIP, DELETE, INSERT, MISMATCH_INSERT = "MATCH", "MISMATCH", "SOFT_CLIP", "DELETE", "INSERT", "MISMATCH_INSERT"

COUNTED, BYPASSED, NO_READS, TOO_FEW_COVERING, DECLINED = 0, 1, 2, 3, 4                      # SK_HAP_*
DECLINE_NONE, DECLINE_GROUPS, DECLINE_READ_INDEX_SPREAD, DECLINE_READ_SPAN = 0, 1, 2, 3      # SK_HAP_DECLINE_*


class ReadBuffer:
    """the part of ActiveRegionReadBuffer that haplotype generation reads"""

    def __init__(self, ref, ref_offset):
        self.ref, self.ref_offset = ref, ref_offset
        self.variant_info = {}         # (id, pos) -> VariantType
        self.snv = {}                  # (id, pos) -> char
        self.insert_seq = {}           # (id, pos) -> string
        self.position_to_align_ids = {}  # pos -> [id], in insertion order
        self.is_fwd = {}

    def add_align_id_to_pos(self, align_id, pos):  # .hh:281-286
        ids = self.position_to_align_ids.setdefault(pos, [])
        if not ids or ids[-1] != align_id:
            ids.append(align_id)

    def insert_match(self, align_id, pos):  # .cpp:26-31
        self.variant_info[(align_id, pos)] = MATCH
        self.add_align_id_to_pos(align_id, pos)

    def insert_mismatch(self, align_id, pos, base):  # :51-57
        self.variant_info[(align_id, pos)] = MISMATCH
        self.snv[(align_id, pos)] = base
        self.add_align_id_to_pos(align_id, pos)

    def insert_soft_clip_segment(self, align_id, pos, seq):  # :33-49
        self.variant_info[(align_id, pos)] = SOFT_CLIP
        self.insert_seq[(align_id, pos)] = seq
        self.add_align_id_to_pos(align_id, pos)

    def insert_indel(self, obs, code):  # :59-107; `code`: the read's bases, for the key's insert sequence
        if obs["is_low_mapq"]:
            return
        align_id, pos = obs["read"], obs["pos"]
        if obs["type"] != M.INDEL_INDEL:
            return  # BP_LEFT, BP_RIGHT
        if obs["ins_len"] > 0 and obs["deletion_length"] == 0:  # isPrimitiveInsertionAllele
            k = (align_id, pos - 1)
            self.variant_info[k] = MISMATCH_INSERT if self.variant_info.get(k) == MISMATCH else INSERT  # setInsert :135-141
            self.insert_seq[k] = M.read_string(code, obs["ins_begin"], obs["ins_begin"] + obs["ins_len"])
            self.add_align_id_to_pos(align_id, pos - 1)
        elif obs["deletion_length"] > 0 and obs["ins_len"] == 0:  # isPrimitiveDeletionAllele
            for i in range(obs["deletion_length"]):
                self.variant_info[(align_id, pos + i)] = DELETE
                self.add_align_id_to_pos(align_id, pos + i)
        # a swap: ignored

    def get_haplotype_base(self, align_id, pos):  # :143-171 -> (base string, is soft-clipped)
        k = (align_id, pos)
        v = self.variant_info[k]
        ref_base = M.ref_char(self.ref, self.ref_offset, pos)
        if v == MATCH:
            return ref_base, False
        if v == MISMATCH:
            return self.snv[k], False
        if v == DELETE:
            return "", False
        if v == INSERT:
            return ref_base + self.insert_seq[k], False
        if v == SOFT_CLIP:
            return self.insert_seq[k], True
        return self.snv[k] + self.insert_seq[k], False  # MISMATCH_INSERT


def add_read(buf, max_indel_size, code, pos, path, is_low_mapq, align_id, is_fwd):
    """the calls addAlignmentIndelsToPosProcessor makes on the read buffer for a genomic read, in its order (:351-488)"""
    buf.is_fwd[align_id] = bool(is_fwd)  # setAlignInfo :348
    path = [(int(t), int(l)) for t, l in path]
    obs = []
    M.add_alignment_indels(max_indel_size, buf.ref, buf.ref_offset, code, pos, path, bool(is_low_mapq), align_id, M.Counters(), obs)
    ends = M.get_match_edge_segments(path)
    path_index, read_offset, ref_head_pos = 0, 0, pos
    k = 0
    while path_index < len(path):
        t, length = path[path_index]
        is_begin_edge, is_end_edge = path_index < ends[0], path_index > ends[1]
        n_seg = 1
        if is_begin_edge or is_end_edge:
            if t == M.SOFT_CLIP and not is_low_mapq:  # :428-441
                at = ref_head_pos - 1 if is_begin_edge else ref_head_pos
                buf.insert_soft_clip_segment(align_id, at, M.read_string(code, read_offset, read_offset + length))
        elif M.is_segment_swap_start(path, path_index) or M.is_indel(t):  # process_swap / process_simple_indel -> insert_indel -> insertIndel
            if M.is_segment_swap_start(path, path_index):
                n_seg = M.swap_info(path, path_index)[0]
            n_obs = 1 if obs[k]["type"] == M.INDEL_INDEL else 2  # one INDEL, or a BP_LEFT + BP_RIGHT pair above max_indel_size
            for o in obs[k:k + n_obs]:
                buf.insert_indel(o, code)
            k += n_obs
        elif not is_low_mapq and M.is_match(t):  # :463-482
            for j in range(length):
                base = M.read_char(code, read_offset + j)
                if M.ref_char(buf.ref, buf.ref_offset, ref_head_pos + j) != base:
                    buf.insert_mismatch(align_id, ref_head_pos + j, base)
                else:
                    buf.insert_match(align_id, ref_head_pos + j)
        for _ in range(n_seg):
            pt, pl = path[path_index]
            if M.is_match(pt):
                read_offset += pl
                ref_head_pos += pl
            elif pt == M.DELETE:
                ref_head_pos += pl
            elif pt in (M.INSERT, M.SOFT_CLIP):
                read_offset += pl
            path_index += 1
    assert k == len(obs), "every observation goes to insertIndel at its own segment"
    return obs


def build_buffer(ref, ref_offset, reads, low_mapq, is_fwd, max_indel_size=M.MAX_INDEL_SIZE):
    """a read's index in the call is its align id -> (ReadBuffer, per-read observation lists)"""
    buf = ReadBuffer(ref, ref_offset)
    obs = []
    for i, (r, low, fwd) in enumerate(zip(reads, low_mapq, is_fwd)):
        obs.append(add_read(buf, max_indel_size, r["code"], int(r["pos"]), r["path"], low, i, fwd))
    return buf, obs


def get_read_segments(buf, begin, end, buf_begin, buf_end):
    """getReadSegments(posRange, readInfo, false, 1) :191-256 -> (numReadsAlignedToActiveRegion, [(align id, segment)] in id order)"""
    haplotype = {}
    reaching_end, invalid, all_ids = set(), set(), set()
    for pos in range(begin, end):
        if not (buf_begin <= pos < buf_end):  # _readBufferRange.is_pos_intersect
            continue
        for align_id in buf.position_to_align_ids.get(pos, []):
            all_ids.add(align_id)
            if align_id in invalid:
                continue
            if pos == begin:
                haplotype[align_id] = ""
            base, is_soft_clipped = buf.get_haplotype_base(align_id, pos)
            if "N" in base or is_soft_clipped:
                invalid.add(align_id)
            if align_id not in haplotype:
                continue
            if not is_soft_clipped:
                haplotype[align_id] += base
            if pos == end - 1:
                reaching_end.add(align_id)
    segments = []
    for align_id in sorted(haplotype):  # std::map<align_id_t, std::string>
        if align_id in invalid or align_id not in reaching_end:
            continue
        if len(haplotype[align_id]) < 1:
            continue
        segments.append((align_id, haplotype[align_id]))
    return len(all_ids), segments


def meets_phasing_error_condition1(hap1, hap2):  # :297-314
    if len(hap1) == len(hap2) and hap1 != hap2:
        first = next(i for i in range(len(hap1)) if hap1[i] != hap2[i])
        return hap1[first + 1:] == hap2[first + 1:]
    return False


def is_filter_second_haplotype_as_sequencer_phasing_noise(is_fwd, groups, hap1, hap2):  # :330-414
    if not meets_phasing_error_condition1(hap1, hap2):
        return False
    ids1, ids2 = groups[hap1], groups[hap2]
    dups = set(ids1) & set(ids2)
    hap2_unique_count = len(ids2) - len(dups)
    hap2_unique_fwd_count = sum(1 for i in ids2 if i not in dups and is_fwd[i])
    if 0 < hap2_unique_fwd_count < hap2_unique_count:
        return False
    at = next(i for i in range(len(hap1)) if hap1[i] != hap2[i])
    base = hap2[at]
    if hap2_unique_fwd_count == 0:
        it = at
        while it != len(hap2):
            if hap2[it] != base:
                break
            it += 1
        return (it - at) > MIN_PHASE_ERROR_HPOL_SIZE
    it = at
    while True:
        if hap2[it] != base:
            break
        if it == 0:
            break
        it -= 1
    return (at - it) > MIN_PHASE_ERROR_HPOL_SIZE


def select_haplotypes(is_fwd, groups, ref_segment, ploidy):
    """selectHaplotypes :416-484 -> [(haplotype, align ids)] in _selectedHaplotypes order, or None where more than MAX_GROUPS groups reach
    MinHaplotypeCount (std::sort's introsort would then decide the order among equal counts)"""
    haplotype_and_counts = [(len(ids), hap) for hap, ids in sorted(groups.items(), key=lambda kv: kv[0].encode()) if len(ids) >= MIN_HAPLOTYPE_COUNT]
    if not haplotype_and_counts:
        return []
    if len(haplotype_and_counts) > MAX_GROUPS:
        return None
    # std::sort with a comparator on the count alone: __insertion_sort for up to 16 elements
    a = haplotype_and_counts
    for i in range(1, len(a)):
        val = a[i]
        if val[0] > a[0][0]:
            a[1:i + 1] = a[0:i]
            a[0] = val
        else:
            j = i
            while val[0] > a[j - 1][0]:
                a[j] = a[j - 1]
                j -= 1
            a[j] = val
    top = a[0][1]
    selected = []
    state = dict(is_reference_selected=False)
    same_count = []

    def select_or_drop():  # :486-516
        if same_count:
            after = len(selected) + len(same_count)
            if after <= ploidy or (after == ploidy + 1 and state["is_reference_selected"]):
                for h in same_count:
                    selected.append((h, list(groups[h])))
                del same_count[:]

    prev_count = 1 << 32
    for count, hap in a:
        if count < prev_count:
            select_or_drop()
        if len(selected) >= ploidy:
            break
        if not is_filter_second_haplotype_as_sequencer_phasing_noise(is_fwd, groups, top, hap):
            same_count.append(hap)
            if hap == ref_segment:
                state["is_reference_selected"] = True
        prev_count = count
    if same_count:
        select_or_drop()
    return selected


def _registered_reads(buf, begin, end):
    ids = set()
    for pos in range(begin, end):
        ids.update(buf.position_to_align_ids.get(pos, []))
    return sorted(ids)


def read_extents(buf):
    """align id -> (first, last) registered position"""
    ext = {}
    for (align_id, pos) in buf.variant_info:
        lo, hi = ext.get(align_id, (pos, pos))
        ext[align_id] = (min(lo, pos), max(hi, pos))
    return ext


def region_haplotypes(ref, ref_offset, reads, low_mapq, is_fwd, regions, buf_begin, buf_end, ploidy, max_indel_size=M.MAX_INDEL_SIZE, buf=None):
    """the whole of sk_region_haplotypes: regions = [(begin, end)] -> [dict(status, reason, n_reads_aligned, n_reads_covering, haps
    [dict(seq, count, is_reference, support)])]"""
    if buf is None:
        buf, _ = build_buffer(ref, ref_offset, reads, low_mapq, is_fwd, max_indel_size)
    ext = read_extents(buf)
    out = []
    for begin, end in regions:
        begin, end = int(begin), int(end)
        rec = dict(status=COUNTED, reason=DECLINE_NONE, n_reads_aligned=0, n_reads_covering=0, haps=[])
        out.append(rec)
        # processHaplotypes :45-56
        if begin < buf_begin or end > buf_end or end - begin > MAX_REF_SPAN_TO_BYPASS_ASSEMBLY:
            rec["status"] = BYPASSED
            continue
        ids = _registered_reads(buf, begin, end)
        rec["n_reads_aligned"] = len(ids)
        if not ids:  # :86
            rec["status"] = NO_READS
            continue
        # the decline rules: _variantInfo[id % 1000][pos % 1000] must name one (read, position) pair for everything the region reads
        if ids[-1] - ids[0] >= MAX_DEPTH:
            rec["status"], rec["reason"] = DECLINED, DECLINE_READ_INDEX_SPREAD
            continue
        if any(ext[i][1] - ext[i][0] >= MAX_BUFFER_SIZE for i in ids):
            rec["status"], rec["reason"] = DECLINED, DECLINE_READ_SPAN
            continue
        n_aligned, segments = get_read_segments(buf, begin, end, buf_begin, buf_end)
        assert n_aligned == len(ids)
        rec["n_reads_covering"] = len(segments)
        if np.float32(len(segments)) < np.float32(MIN_FRAC_READS_COVERING_REGION) * np.float32(n_aligned):  # :91, unsigned against float * unsigned
            rec["status"] = TOO_FEW_COVERING
            continue
        groups = {}
        for align_id, hap in segments:  # :96-105
            groups.setdefault(hap, []).append(align_id)
        ref_segment = "".join(M.ref_char(ref, ref_offset, p) for p in range(begin, end))
        selected = select_haplotypes(buf.is_fwd, groups, ref_segment, ploidy)
        if selected is None:
            rec["status"], rec["reason"] = DECLINED, DECLINE_GROUPS
            continue
        rec["haps"] = [dict(seq=h, count=len(ids_), is_reference=int(h == ref_segment), support=ids_) for h, ids_ in selected]
    return out
