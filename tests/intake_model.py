"""The read intake, restated rule by rule: the bit-exact reference for sk_read_intake (csrc/read_intake.hip).

Three functions of the reference (L/ = its src/c++/lib), with their loops kept as written:

  * get_valid_alignment_range             L/starling_common/starling_read_util.cpp:218-329
  * addAlignmentIndelsToPosProcessor      L/starling_common/starling_pos_processor_indel_util.cpp:300-491 (process_swap :163-224,
    process_simple_indel :231-296, the edge processors :79-153, increment_path / swap_info L/blt_util/align_path_util.hh:36-103)
  * the active-region detector's counters L/starling_common/ActiveRegionReadBuffer.hh:263-292, .cpp:26-107 and isCandidateVariant
    .cpp:258-269 (float32 arithmetic through numpy.float32)

The counters are kept per position in a dict instead of the reference's ring of 1 000 positions: reads arrive in position order and
a read contributes no further left than al.pos - 1, so what the ring holds when position head - 1 is read is the plain sum over
the reads.  Out of scope, as in the header: pinned edges, external candidates, the haplotype store, the repeat
finder, IndelBuffer bookkeeping.

This module does not import the product."""
import numpy as np

NONE, MATCH, INSERT, DELETE, SKIP, SOFT_CLIP, HARD_CLIP, PAD, SEQ_MATCH, SEQ_MISMATCH = range(10)
INDEL_NONE, INDEL_INDEL, INDEL_MISMATCH, INDEL_BP_LEFT, INDEL_BP_RIGHT = range(5)

MAX_INDEL_SIZE = 49                 # starling_base_shared.hh:124
MIN_ALT_ALLELE_FRACTION = 0.2       # ActiveRegionDetector.hh:68 (a float)
MAX_CAND_FILTER_INSERT_SIZE = 10    # starling_pos_processor_indel_util.cpp:70
MATCH_SCORE, MISMATCH_SCORE, MIN_SEGMENT_SCORE = 2, -5, -11  # starling_read_util.cpp:224-226
MISMATCH_WEIGHT, INDEL_WEIGHT, MIN_NUM_VARIANTS = 1, 4, 9    # ActiveRegionReadBuffer.hh:67-80
LOW_DEPTH_FRACTION = 0.35           # ActiveRegionReadBuffer.hh:84 (a float)
MAX_READ_LEN = 1024                 # SK_PILEUP_MAX_READ_LEN

_CODE_CHAR = {0: "=", 1: "A", 2: "C", 4: "G", 8: "T"}
_CHAR_CODE = {"=": 0, "A": 1, "C": 2, "G": 4, "T": 8, "N": 15}


class PathError(ValueError):
    """what the reference throws on (blt_exception), or indexes out of its arrays on"""


def encode(seq):
    """read string -> BAM 4-bit codes, one per byte"""
    return np.array([_CHAR_CODE[c] for c in seq], np.uint8)


def read_char(code, i):
    """bam_seq::get_char (L/htsapi/bam_seq.hh): '=', A, C, G, T, everything else 'N'; 'N' out of range"""
    if i < 0 or i >= len(code):
        return "N"
    return _CODE_CHAR.get(int(code[i]), "N")


def ref_char(ref, ref_offset, p):
    """reference_contig_segment::get_base: 'N' outside the segment"""
    if p < ref_offset or p >= ref_offset + len(ref):
        return "N"
    return ref[p - ref_offset]


def read_string(code, begin, end):
    """bam_seq_to_str :56-66"""
    return "".join(read_char(code, i) for i in range(begin, end))


def is_match(t):
    return t in (MATCH, SEQ_MATCH, SEQ_MISMATCH)


def is_read_length(t):
    return t in (MATCH, INSERT, SOFT_CLIP, SEQ_MATCH, SEQ_MISMATCH)


def is_indel(t):
    return t in (INSERT, DELETE)


def apath_read_length(path):
    return sum(l for t, l in path if is_read_length(t))


def apath_invalid_reason(path, seq_length):
    """get_apath_invalid_type, L/blt_util/align_path.cpp:928-997 -> None or the issue's name"""
    is_m = False
    last_type = NONE
    n = len(path)
    for i, (t, _) in enumerate(path):
        if t == NONE or t > SEQ_MISMATCH:
            return "UNKNOWN_SEGMENT"
        if i != 0 and t == last_type:
            return "REPEATED_SEGMENT"
        if not is_m and t == SKIP:
            return "EDGE_SKIP"
        if t == HARD_CLIP and not (i == 0 or i + 1 == n):
            return "CLIPPING"
        if t == SOFT_CLIP and not (i == 0 or i + 1 == n):
            if i == 1:
                if n == 3:
                    if path[0][0] != HARD_CLIP and path[i + 1][0] != HARD_CLIP:
                        return "CLIPPING"
                elif path[0][0] != HARD_CLIP:
                    return "CLIPPING"
            elif i + 2 == n:
                if path[i + 1][0] != HARD_CLIP:
                    return "CLIPPING"
            else:
                return "CLIPPING"
        if not is_m and is_match(t):
            is_m = True
        last_type = t
    if not is_m:
        return "FLOATING"
    for i in range(n):
        t = path[n - (i + 1)][0]
        if is_match(t):
            break
        if t == SKIP:
            return "EDGE_SKIP"
    if seq_length != apath_read_length(path):
        return "LENGTH"
    return None


def is_apath_starling_invalid(path):
    """:1005-1013"""
    return any(t == PAD for t, _ in path)


def check_path(path, seq_length):
    """what addAlignmentIndelsToPosProcessor :315-328 throws on, the SKIP it asserts against (:360; get_valid_alignment_range throws on
    it, :296-301), and a zero-length segment (an insertion of length 0 indexes rev_read_score[read_head_pos - 1], :245)"""
    if seq_length > MAX_READ_LEN:
        raise PathError("read longer than %d" % MAX_READ_LEN)
    why = apath_invalid_reason(path, seq_length)
    if why:
        raise PathError(why)
    if is_apath_starling_invalid(path):
        raise PathError("PAD")
    if any(t == SKIP for t, _ in path):
        raise PathError("SKIP")
    if any(l == 0 for _, l in path):
        raise PathError("zero-length segment")


def get_match_edge_segments(path):
    """:735-752"""
    n = len(path)
    first, second = n, n
    is_first_match = False
    for i, (t, _) in enumerate(path):
        if is_match(t):
            if not is_first_match:
                first = i
            is_first_match = True
            second = i
    return first, second


def is_segment_swap_start(path, i):
    """:867-895"""
    is_insert = is_delete = False
    while i < len(path):
        if path[i][0] == INSERT:
            is_insert = True
        elif path[i][0] == DELETE:
            is_delete = True
        else:
            break
        i += 1
    return is_insert and is_delete


def swap_info(path, path_index):
    """align_path_util.hh:75-103 -> (n_seg, insert_length, delete_length)"""
    n_seg, ins, dele = path_index, 0, 0
    while n_seg < len(path) and is_indel(path[n_seg][0]):
        t, l = path[n_seg]
        if t == INSERT:
            ins += l
        else:
            dele += l
        n_seg += 1
    return n_seg - path_index, ins, dele


def read_scores(ref, ref_offset, code, pos, path):
    """the two score vectors of get_valid_alignment_range, :228-302"""
    read_size = len(code)
    fwd = [0] * read_size
    rev = [0] * read_size

    def at(i):
        if i < 0 or i >= read_size:
            raise PathError("score index %d outside the read" % i)
        return i

    ref_head_pos, read_head_pos = pos, 0
    for t, length in path:
        if t in (INSERT, SOFT_CLIP):
            if t == INSERT:
                fwd[at(read_head_pos)] += MISMATCH_SCORE
                rev[at(read_head_pos + length - 1)] += MISMATCH_SCORE
            read_head_pos += length
        elif t == DELETE:
            if read_head_pos > 0:
                fwd[at(read_head_pos - 1)] += MISMATCH_SCORE
            if read_head_pos < read_size:
                rev[at(read_head_pos)] += MISMATCH_SCORE
            ref_head_pos += length
        elif is_match(t):
            for j in range(length):
                read_pos = at(read_head_pos + j)
                rc = read_char(code, read_pos)
                fc = ref_char(ref, ref_offset, ref_head_pos + j)
                if rc != "N" and fc != "N":
                    s = MISMATCH_SCORE if rc != fc else MATCH_SCORE
                    fwd[read_pos] += s
                    rev[read_pos] += s
            read_head_pos += length
            ref_head_pos += length
        elif t == HARD_CLIP:
            pass
        else:
            raise PathError("Can't handle cigar code")
    return fwd, rev


def reckoning(fwd, rev):
    """the loop at :304-328, as written"""
    read_size = len(fwd)
    begin_pos, end_pos = 0, read_size
    fwd_sum, fwd_min = 0, MIN_SEGMENT_SCORE
    rev_sum, rev_min = 0, MIN_SEGMENT_SCORE
    for i in range(read_size):
        fwd_sum += fwd[i]
        if fwd_sum <= fwd_min:
            begin_pos = i + 1
            fwd_min = fwd_sum
        rev_sum += rev[read_size - i - 1]
        if rev_sum <= rev_min:
            end_pos = read_size - i - 1
            rev_min = rev_sum
    if end_pos <= begin_pos:
        begin_pos, end_pos = 0, 0
    return begin_pos, end_pos


def reckoning_closed_form(fwd, rev):
    """what the kernel computes: with S the running sum of fwd, begin = 1 + the LAST index attaining min S when min S <= -11, else 0;
    with P the exclusive running sum of rev and T its total, the reverse sum ending at index k is T - P[k], so end = the FIRST index
    attaining max P when T - max P <= -11, else the read size"""
    n = len(fwd)
    begin_pos, end_pos = 0, n
    if n:
        s = np.cumsum(np.asarray(fwd, np.int64))
        m = int(s.min())
        if m <= MIN_SEGMENT_SCORE:
            begin_pos = 1 + int(np.nonzero(s == m)[0][-1])
        r = np.asarray(rev, np.int64)
        p = np.cumsum(r) - r
        total = int(r.sum())
        pm = int(p.max())
        if total - pm <= MIN_SEGMENT_SCORE:
            end_pos = int(np.nonzero(p == pm)[0][0])
    if end_pos <= begin_pos:
        begin_pos, end_pos = 0, 0
    return begin_pos, end_pos


def get_valid_alignment_range(ref, ref_offset, code, pos, path):
    return reckoning(*read_scores(ref, ref_offset, code, pos, path))


class Counters:
    """_variantCounter / _depth of ActiveRegionReadBuffer, per position"""

    def __init__(self):
        self.count = {}
        self.depth = {}

    def add_variant_count(self, pos, count):  # .hh:263-268
        self.count[pos] = self.count.get(pos, 0) + count
        self.depth[pos] = self.depth.get(pos, 0) + 1

    def add_soft_clip_count(self, pos, count):  # .hh:270-274
        self.count[pos] = self.count.get(pos, 0) + count

    def insert_match(self, pos):  # .cpp:26-31
        self.add_variant_count(pos, 0)

    def insert_mismatch(self, pos):  # .cpp:51-57
        self.add_variant_count(pos, MISMATCH_WEIGHT)

    def insert_soft_clip_segment(self, pos, is_begin_edge):  # .cpp:33-49
        self.add_variant_count(pos, INDEL_WEIGHT)
        self.add_soft_clip_count(pos + 1 if is_begin_edge else pos - 1, INDEL_WEIGHT)

    def insert_indel(self, obs):  # .cpp:59-107 (read observations: not external, not forced)
        if obs["is_low_mapq"]:
            return
        pos = obs["pos"]
        if obs["type"] == INDEL_INDEL and obs["ins_len"] > 0 and obs["deletion_length"] == 0:  # isPrimitiveInsertionAllele
            self.add_variant_count(pos - 1, INDEL_WEIGHT)
            self.add_variant_count(pos, INDEL_WEIGHT)
        elif obs["type"] == INDEL_INDEL and obs["ins_len"] == 0 and obs["deletion_length"] > 0:  # isPrimitiveDeletionAllele
            for i in range(obs["deletion_length"]):
                self.add_variant_count(pos + i, INDEL_WEIGHT)
            self.add_variant_count(pos - 1, INDEL_WEIGHT)


def _obs(read, pos, otype, is_noise, is_low_mapq, deletion_length=0, ins=(0, 0), bp=(0, 0)):
    """one observation; an empty sequence is the range (0, 0)"""
    ib, il = (ins[0], ins[1] - ins[0]) if ins[1] > ins[0] else (0, 0)
    bb, bl = (bp[0], bp[1] - bp[0]) if bp[1] > bp[0] else (0, 0)
    return dict(read=read, pos=pos, deletion_length=deletion_length, ins_begin=ib, ins_len=il, bp_begin=bb, bp_len=bl, type=otype,
                is_noise=int(is_noise), is_low_mapq=int(is_low_mapq))


def add_alignment_indels(max_indel_size, ref, ref_offset, code, pos, path, is_low_mapq, read_index, counters, out):
    """addAlignmentIndelsToPosProcessor for a genomic read (edge_pin = false, false) with the detector on -> (valid range, the
    returned total_indel_ref_span_per_read); observations are appended to `out`, the counters updated"""
    seq_len = len(code)
    check_path(path, seq_len)
    ends = get_match_edge_segments(path)
    valid_begin, valid_end = get_valid_alignment_range(ref, ref_offset, code, pos, path)

    def insert_indel(o):  # starling_pos_processor_base::insert_indel :397-456 -> ActiveRegionReadBuffer::insertIndel
        counters.insert_indel(o)
        out.append(o)

    path_index, read_offset, ref_head_pos = 0, 0, pos
    total_indel_ref_span_per_read = 0
    aps = len(path)
    while path_index < aps:
        t, length = path[path_index]
        is_begin_edge = path_index < ends[0]
        is_end_edge = path_index > ends[1]
        is_edge_segment = is_begin_edge or is_end_edge
        is_swap_start = is_segment_swap_start(path, path_index)
        is_noise = False
        if not is_match(t):
            begin = 0 if read_offset == 0 else read_offset - 1
            rlen = 0
            if is_swap_start:
                _, ins_len, del_len = swap_info(path, path_index)
                rlen = ins_len
                if del_len <= max_indel_size:
                    total_indel_ref_span_per_read += del_len
            elif is_read_length(t):
                rlen = length
            elif t == DELETE:
                if length <= max_indel_size:
                    total_indel_ref_span_per_read += length
            end = min(seq_len, read_offset + 1 + rlen)
            if not (end <= valid_end and begin >= valid_begin):  # pos_range::is_superset_of
                is_noise = True

        n_seg = 1
        if is_edge_segment:
            # edge inserts and deletions on genomic reads give nothing (process_edge_insert :100, :422)
            if t == SOFT_CLIP and not is_low_mapq:
                counters.insert_soft_clip_segment(ref_head_pos - 1 if is_begin_edge else ref_head_pos, is_begin_edge)
        elif is_swap_start:  # process_swap :163-224
            n_seg, ins_len, del_len = swap_info(path, path_index)
            swap_size = max(ins_len, del_len)
            if is_noise and ins_len > MAX_CAND_FILTER_INSERT_SIZE:
                is_noise = False
            if swap_size <= max_indel_size:
                insert_indel(_obs(read_index, ref_head_pos, INDEL_INDEL, is_noise, is_low_mapq, del_len, ins=(read_offset, read_offset + ins_len)))
            else:
                start = read_offset
                size = seq_len - read_offset
                insert_indel(_obs(read_index, ref_head_pos, INDEL_BP_LEFT, is_noise, is_low_mapq, bp=(start, start + min(size, max_indel_size))))
                next_read_offset = read_offset + ins_len
                start_offset = next_read_offset - min(next_read_offset, max_indel_size)
                insert_indel(_obs(read_index, ref_head_pos + del_len, INDEL_BP_RIGHT, is_noise, is_low_mapq, bp=(start_offset, next_read_offset)))
        elif is_indel(t):  # process_simple_indel :231-296
            if is_noise and t == INSERT and length > MAX_CAND_FILTER_INSERT_SIZE:
                is_noise = False
            if length <= max_indel_size:
                if t == DELETE:
                    insert_indel(_obs(read_index, ref_head_pos, INDEL_INDEL, is_noise, is_low_mapq, length))
                else:
                    insert_indel(_obs(read_index, ref_head_pos, INDEL_INDEL, is_noise, is_low_mapq, ins=(read_offset, read_offset + length)))
            else:
                start = read_offset
                size = seq_len - read_offset
                insert_indel(_obs(read_index, ref_head_pos, INDEL_BP_LEFT, is_noise, is_low_mapq, bp=(start, start + min(size, max_indel_size))))
                next_read_offset = read_offset + (length if t == INSERT else 0)
                start_offset = next_read_offset - min(next_read_offset, max_indel_size)
                insert_indel(_obs(read_index, ref_head_pos + (length if t == DELETE else 0), INDEL_BP_RIGHT, is_noise, is_low_mapq,
                                  bp=(start_offset, next_read_offset)))
        elif not is_low_mapq and is_match(t):
            for j in range(length):
                ref_pos = ref_head_pos + j
                if ref_char(ref, ref_offset, ref_pos) != read_char(code, read_offset + j):
                    counters.insert_mismatch(ref_pos)
                else:
                    counters.insert_match(ref_pos)

        for _ in range(n_seg):  # increment_path, align_path_util.hh:36-68
            pt, pl = path[path_index]
            if is_match(pt):
                read_offset += pl
                ref_head_pos += pl
            elif pt in (DELETE, SKIP):
                ref_head_pos += pl
            elif pt in (INSERT, SOFT_CLIP):
                read_offset += pl
            elif pt in (HARD_CLIP, PAD):
                pass
            else:
                raise PathError("Unexpected alignment type")
            path_index += 1
    return (valid_begin, valid_end), total_indel_ref_span_per_read


def is_candidate_variant(ref_base, count, depth, min_alt_allele_fraction=MIN_ALT_ALLELE_FRACTION):
    """isCandidateVariant .cpp:258-269: unsigned count against float * unsigned, all in float"""
    if ref_base == "N":
        return False
    f = np.float32(min_alt_allele_fraction)
    low = np.float32(LOW_DEPTH_FRACTION)
    c = np.float32(count)
    d = np.float32(depth)
    return bool((count >= MIN_NUM_VARIANTS and c >= f * d) or c >= low * d)


def read_intake(ref, ref_offset, reads, low_mapq, win_begin, n_pos, max_indel_size=MAX_INDEL_SIZE,
                min_alt_allele_fraction=MIN_ALT_ALLELE_FRACTION):
    """the whole of sk_read_intake: reads = dicts(code, pos, path) -> dict(reads [(valid_begin, valid_end, span, n_obs)], obs_off, obs
    [dicts], sites [(count, depth)], is_candidate)"""
    counters = Counters()
    per_read, obs_off, obs = [], [0], []
    for r, (rd, low) in enumerate(zip(reads, low_mapq)):
        mine = []
        (vb, ve), span = add_alignment_indels(max_indel_size, ref, ref_offset, rd["code"], int(rd["pos"]), [(int(t), int(l)) for t, l in rd["path"]],
                                              bool(low), r, counters, mine)
        per_read.append((vb, ve, span, len(mine)))
        obs.extend(mine)
        obs_off.append(len(obs))
    sites = [(counters.count.get(win_begin + i, 0), counters.depth.get(win_begin + i, 0)) for i in range(n_pos)]
    cand = [is_candidate_variant(ref_char(ref, ref_offset, win_begin + i), c, d, min_alt_allele_fraction) for i, (c, d) in enumerate(sites)]
    return dict(reads=per_read, obs_off=obs_off, obs=obs, sites=sites, is_candidate=cand)
