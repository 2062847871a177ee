// preamble_core.h -- the realignment preamble (getCandidateAlignments up to its call of candidate_alignment_search,
// L/starling_common/starling_read_align.cpp:1816-1957, with the normalisation of enumerate_read :2001-2057 before it) as container-free
// code that compiles for the device and for the host alike: from a read that passed the gate to the skcore::PRead the search starts
// from.  host/read_realign.cpp (enumerate_read -> get_candidate_alignments -> to_core_read) holds the container-based statement of the
// same rules, which is the one pinned to the reference; tests/test_realign_preamble.py requires this core to make the same record byte
// for byte.  Nothing here keeps an array of its own: every list lives in the record, so a kernel that builds the record in LDS has no
// private memory to spill.
//
//   P1  input normalisation (:2001-2057, DNA reads): is_edge_readref_len_segment (L/blt_util/align_path.cpp:824-846) ->
//       matchify_edge_indels(lead, trail) (L/starling_common/alignment_util.cpp:92-124, :130-174, :190-198); a path that is still soft
//       clipped -> matchify_edge_segment_type(SOFT_CLIP).  A normalised pos < 0 ends the read: SK_RPRE_NEGATIVE_POS.
//   P2  edge keys (:1479-1522): the last INSERT or DELETE before the first match segment and the last one after the last match segment,
//       looked up by (pos, type, del_len, insert bytes); the insert bytes are the read's codes through bam_seq::get_char
//       (L/htsapi/bam_seq.hh:30-46), positions past the codes read 'N'.  Absent: SK_RPRE_EDGE_KEY_MISSING.
//   P3  the initial status map: add_indels_in_range (:311-366) over soft_clip_range of the normalised alignment; is_usable_indel
//       (:289-305) asks candidacy first, then the read's observed list; every key asked is marked in `consulted`.
//   P4  the exemplar's own keys (getAlignmentIndels, L/starling_common/CandidateAlignment.cpp:59-177, include_mismatches): edge segments,
//       swap segments, plain indels, the breakpoint pair above max_indel_size, and mismatch keys when the table holds any.  A
//       non-mismatch key that is not in the table or not in the map: SK_RPRE_EXEMPLAR_KEY_MISSING; an absent mismatch key is skipped.
//       Found keys are present and in_original; a found mismatch key has the alignment recomputed by make_start_pos_alignment.
//   P5  the toggle order (present ascending, absent ascending, sort_remove_only_indels_last :724-751) and clip_clipper (:460-504).
//
// Capacities are reported, never truncated: the read then takes the host path.  Where the container-based code checks its capacities
// last (to_core_read), this core meets two of them first: a path of more than Caps::P segments or a segment above 0xffff at any step of
// P1 is SK_RPRE_CAP_P before P2 looks for keys, and a table above PRE_MAX_TAB keys is SK_RPRE_CAP_K before anything.  The status map
// and the observed list keep the host's order: a read over Caps::K or Caps::OBS still has P2 and P4 report a missing key first.
#pragma once

#include "realign_core.h"

namespace skcore
{

enum { PRE_MAX_TAB = 32000 }; // table indices are int16 in the record (to_core_read)

struct PreRead // one read as the preamble takes it
{
    int32_t pos, n_seg, read_len, sample;
    int32_t realign_b, realign_e;
    int32_t fwd;
    const sk_path_seg* path;
    const uint8_t* code; // BAM 4-bit codes, one per byte
    int32_t n_code;      // positions at or past it read 'N'
    const int32_t* observed; // ascending table indices
    int32_t n_observed;
};

struct PreTable
{
    PJob job;              // tab, n_tab, max_indel_size
    const uint8_t* ins_pool; // tab[k].ins_off indexes it
    int32_t has_mismatch_keys;
    const char* ref;       // the job's reference segment (P4's mismatch branch); positions outside read 'N'
    int32_t ref_offset, ref_len;
    uint8_t* consulted;    // [n_tab]
};

SKC_HD inline char pre_code_char(const uint8_t c) // bam_seq::get_char
{
    switch (c) {
    case SK_BAM_REF: return '=';
    case SK_BAM_A: return 'A';
    case SK_BAM_C: return 'C';
    case SK_BAM_G: return 'G';
    case SK_BAM_T: return 'T';
    default: return 'N';
    }
}
SKC_HD inline uint8_t pre_char_code(const char c)
{
    switch (c) {
    case '=': return SK_BAM_REF;
    case 'A': return SK_BAM_A;
    case 'C': return SK_BAM_C;
    case 'G': return SK_BAM_G;
    case 'T': return SK_BAM_T;
    default: return SK_BAM_ANY;
    }
}
SKC_HD inline char pre_read_char(const PreRead& in, const uint32_t i) { return i < uint32_t(in.n_code) ? pre_code_char(in.code[i]) : 'N'; }

// get_match_edge_segments (align_path.cpp:735-752): n_seg twice when no segment is a match
SKC_HD inline void pre_match_ends(const PCal& c, int& first, int& last)
{
    first = last = c.n_seg;
    bool seen = false;
    for (int i = 0; i < c.n_seg; ++i)
        if (seg_align_match(c.path[i].type)) {
            if (!seen) first = i;
            seen = true;
            last = i;
        }
}
SKC_HD inline void pre_cut_path(PCal& c, const int n) // the segments past n leave; the record's bytes behind the path stay zero
{
    for (int i = n; i < c.n_seg; ++i) c.path[i].type = c.path[i].length = 0;
    c.n_seg = uint8_t(n);
}
// remove_edge_deletions (alignment_util.cpp:92-124), both edges, in place
SKC_HD inline void pre_remove_edge_deletions(PCal& c)
{
    int first, last, w = 0;
    pre_match_ends(c, first, last);
    for (int i = 0; i < c.n_seg; ++i) {
        const PSeg s = c.path[i];
        if (s.type == SK_SEG_DELETE && (i < first || i > last)) {
            if (i < first) c.pos += int32_t(s.length);
        } else {
            c.path[w++] = s;
        }
    }
    pre_cut_path(c, w);
}
// matchify_edge_segment_type (:130-174), both edges, in place; false: a merged match segment above 0xffff
SKC_HD inline bool pre_matchify_edge(PCal& c, const unsigned seg_type)
{
    int first, last, w = 0;
    pre_match_ends(c, first, last);
    for (int i = 0; i < c.n_seg; ++i) {
        const PSeg s = c.path[i];
        const bool le = i < first, te = i > last;
        const bool target = s.type == seg_type && (le || te);
        if (target && le) c.pos -= int32_t(s.length);
        if (target || seg_align_match(s.type)) {
            if (w > 0 && seg_align_match(c.path[w - 1].type)) {
                const unsigned sum = unsigned(c.path[w - 1].length) + s.length;
                if (sum > 0xffffu) return false;
                c.path[w - 1].length = uint16_t(sum);
            } else {
                c.path[w].type = SK_SEG_MATCH;
                c.path[w++].length = s.length;
            }
        } else {
            c.path[w++] = s;
        }
    }
    pre_cut_path(c, w);
    return true;
}

// P1.  `c` is zero at entry.
SKC_HD inline int pre_normalise(const PreRead& in, PCal& c)
{
    if (in.n_seg > Caps::P) return SK_RPRE_CAP_P;
    c.pos = in.pos;
    c.lead = c.trail = -1;
    c.fwd = in.fwd ? 1 : 0;
    bool soft = false;
    for (int i = 0; i < in.n_seg; ++i) {
        if (in.path[i].length > 0xffffu) return SK_RPRE_CAP_P;
        c.path[i].type = uint16_t(in.path[i].type);
        c.path[i].length = uint16_t(in.path[i].length);
    }
    c.n_seg = uint8_t(in.n_seg);
    int first, last;
    pre_match_ends(c, first, last);
    bool edge = false; // is_edge_readref_len_segment
    for (int i = 0; i < c.n_seg; ++i) {
        const unsigned t = c.path[i].type;
        if ((i < first || i > last) && (t == SK_SEG_INSERT || t == SK_SEG_DELETE || t == SK_SEG_SKIP || t == SK_SEG_SOFT_CLIP)) edge = true;
    }
    if (edge) { // matchify_edge_indels
        pre_remove_edge_deletions(c);
        if (!pre_matchify_edge(c, SK_SEG_INSERT)) return SK_RPRE_CAP_P;
    }
    for (int i = 0; i < c.n_seg; ++i)
        if (c.path[i].type == SK_SEG_SOFT_CLIP) soft = true;
    if (soft && !pre_matchify_edge(c, SK_SEG_SOFT_CLIP)) return SK_RPRE_CAP_P;
    return c.pos < 0 ? SK_RPRE_NEGATIVE_POS : SK_RPRE_OK;
}

// IndelKey::operator< (IndelKey.hh:57-80) of table entry k against (pos, type, del, the read's bases [read_at, read_at + ins_len)): < 0, 0, > 0.
// `one`: a single insert character given as such (the mismatch key's), else 0.
SKC_HD inline int pre_key_compare(const PreTable& t, const int k, const PreRead& in, const int32_t pos, const int type, const uint32_t del, const uint32_t ins_len,
                                  const uint32_t read_at, const char one)
{
    const PIndel& e = t.job.tab[k];
    if (e.pos != pos) return e.pos < pos ? -1 : 1;
    if (int(e.type) != type) return int(e.type) < type ? -1 : 1;
    if (type == SK_INDEL_NONE || type == SK_INDEL_BP_LEFT || type == SK_INDEL_BP_RIGHT) return 0;
    if (e.ins_len != ins_len) return e.ins_len < ins_len ? -1 : 1;
    if (e.del != del) return e.del < del ? -1 : 1;
    for (uint32_t i = 0; i < ins_len; ++i) {
        const uint8_t a = t.ins_pool[e.ins_off + i], b = uint8_t(one ? one : pre_read_char(in, read_at + i));
        if (a != b) return a < b ? -1 : 1;
    }
    return 0;
}
// the key's table index, -1: absent
SKC_HD inline int pre_find_key(const PreTable& t, const PreRead& in, const int32_t pos, const int type, const uint32_t del, const uint32_t ins_len, const uint32_t read_at,
                               const char one = 0)
{
    int a = 0, b = t.job.n_tab;
    while (a < b) {
        const int m = (a + b) >> 1;
        if (pre_key_compare(t, m, in, pos, type, del, ins_len, read_at, one) < 0) a = m + 1;
        else b = m;
    }
    return (a < t.job.n_tab && pre_key_compare(t, a, in, pos, type, del, ins_len, read_at, one) == 0) ? a : -1;
}

// P2
SKC_HD inline int pre_edge_keys(const PreTable& t, const PreRead& in, PCal& c)
{
    int first, last;
    pre_match_ends(c, first, last);
    int32_t ref_pos = c.pos;
    uint32_t read_pos = 0;
    bool has_lead = false, has_trail = false;
    int lead = -1, trail = -1;
    for (int i = 0; i < c.n_seg; ++i) {
        const PSeg s = c.path[i];
        if ((s.type == SK_SEG_INSERT || s.type == SK_SEG_DELETE) && (i < first || i > last)) {
            const int k = s.type == SK_SEG_INSERT ? pre_find_key(t, in, ref_pos, SK_INDEL_INDEL, 0, s.length, read_pos) : pre_find_key(t, in, ref_pos, SK_INDEL_INDEL, s.length, 0, 0);
            if (i < first) {
                has_lead = true;
                lead = k;
            } else {
                has_trail = true;
                trail = k;
            }
        }
        if (seg_read_len(s.type)) read_pos += s.length;
        if (seg_ref_len(s.type)) ref_pos += int32_t(s.length);
    }
    if ((has_lead && lead < 0) || (has_trail && trail < 0)) return SK_RPRE_EDGE_KEY_MISSING;
    c.lead = int16_t(lead);
    c.trail = int16_t(trail);
    return SK_RPRE_OK;
}

SKC_HD inline bool pre_observed(const PreRead& in, const int idx)
{
    int a = 0, b = in.n_observed;
    while (a < b) {
        const int m = (a + b) >> 1;
        if (in.observed[m] < idx) a = m + 1;
        else b = m;
    }
    return a < in.n_observed && in.observed[a] == idx;
}
// P3 for one key of rangeIterator(pr): 0 = not in the map, 1 = in it, 2 = in it and remove-only.  In the preamble the map is empty at
// entry and each key of the range is visited once, so add_indels_in_range's "already in the map" branch cannot be taken and is not built.
SKC_HD inline int pre_key_state(const PreTable& t, const PreRead& in, const PRange& pr, const int k, const bool mark)
{
    const PIndel& e = t.job.tab[k];
    if (!range_adjacent_indel_breakpoints(pr, e)) return 0;
    if (mark) t.consulted[k] = 1; // is_usable_indel asks candidacy first (a byte store of 1, whoever writes)
    if (!(e.cand != 0 || pre_observed(in, k))) return 0;
    return range_intersect_indel_breakpoints(pr, e) ? 1 : 2;
}
SKC_HD inline void pre_put_status(PRead& r, const int at, const int k, const int state)
{
    r.sm[at].idx = int16_t(k);
    r.sm[at].is_present = 0;
    r.sm[at].is_remove_only = state == 2 ? 1 : 0;
    r.sm[at].in_original = 0;
    r.sm[at].pad = 0;
}
// P3, one key after the other (the host; the kernel takes the keys 64 to a turn through pre_key_state); false: more than Caps::K entries
SKC_HD inline bool pre_status_map(const PreTable& t, const PreRead& in, const PRange& pr, PRead& r)
{
    int lo, hi, n = 0;
    range_iter(t.job, pr.b, pr.e, lo, hi);
    for (int k = lo; k < hi; ++k) {
        const int state = pre_key_state(t, in, pr, k, true);
        if (!state) continue;
        if (n < Caps::K) pre_put_status(r, n, k, state);
        ++n;
    }
    r.n_sm = uint8_t(n < Caps::K ? n : Caps::K);
    return n <= Caps::K;
}

struct PreView // the record's lists as sort_remove_only_indels_last and sm_find read a frame
{
    PStatus* sm;
    int16_t *order, *current;
    uint8_t n_sm, n_order;
};

// P4's test of one key and its mark: false = the host's Fail.  `whole`: the map holds every entry (no overflow in P3); else membership is
// asked of the rule itself, which is what the map states.
SKC_HD inline bool pre_take_key(const PreTable& t, const PreRead& in, const PRange& pr, const int lo, const int hi, const bool whole, PRead& r, const int idx,
                                const bool is_mm, int& n_valid, bool& recompute)
{
    int at = -1;
    bool in_map = false;
    if (idx >= 0) {
        if (whole) {
            at = sm_find(r, idx);
            in_map = at >= 0;
        } else {
            in_map = idx >= lo && idx < hi && pre_key_state(t, in, pr, idx, false) != 0;
        }
    }
    if (!in_map) return is_mm;
    if (is_mm) recompute = true;
    if (at >= 0) {
        r.sm[at].is_present = r.sm[at].in_original = 1;
        iset_insert(r.cal.indels, n_valid, int16_t(idx)); // (the valid set borrows the alignment's indel list, which a root alignment leaves empty)
    }
    return true;
}

SKC_HD inline char pre_ref_base(const PreTable& t, const int32_t p)
{
    return (p < t.ref_offset || p >= t.ref_offset + t.ref_len) ? 'N' : t.ref[p - t.ref_offset];
}

// P4
SKC_HD inline int pre_exemplar_keys(const PreTable& t, const PreRead& in, const PRange& pr, const bool whole, PRead& r)
{
    PCal& c = r.cal;
    int lo, hi, first, last;
    range_iter(t.job, pr.b, pr.e, lo, hi);
    pre_match_ends(c, first, last);
    const uint32_t max_size = uint32_t(t.job.max_indel_size);
    int n_valid = 0;
    bool recompute = false, ok = true;
    uint32_t read_off = 0;
    int32_t ref_head = c.pos;
    int pi = 0;
    while (pi < c.n_seg && ok) {
        const bool edge = pi < first || pi > last;
        // is_segment_swap_start (align_path.cpp:868-895) and SwapInfo (align_path_util.hh:75-106)
        bool ins = false, del = false;
        uint32_t ins_len = 0, del_len = 0;
        int n_swap = 0;
        for (int i = pi; i < c.n_seg && (c.path[i].type == SK_SEG_INSERT || c.path[i].type == SK_SEG_DELETE); ++i, ++n_swap) {
            if (c.path[i].type == SK_SEG_INSERT) {
                ins = true;
                ins_len += c.path[i].length;
            } else {
                del = true;
                del_len += c.path[i].length;
            }
        }
        const bool swap_start = ins && del;
        const PSeg s = c.path[pi];
        const int n_seg = swap_start ? n_swap : 1;
        const bool indel = s.type == SK_SEG_INSERT || s.type == SK_SEG_DELETE;
        if (edge) {
            if (indel) ok = pre_take_key(t, in, pr, lo, hi, whole, r, pi < first ? c.lead : c.trail, false, n_valid, recompute);
        } else if (swap_start || indel) {
            const uint32_t il = swap_start ? ins_len : (s.type == SK_SEG_INSERT ? s.length : 0), dl = swap_start ? del_len : (s.type == SK_SEG_DELETE ? s.length : 0);
            if ((il > dl ? il : dl) <= max_size) {
                ok = pre_take_key(t, in, pr, lo, hi, whole, r, pre_find_key(t, in, ref_head, SK_INDEL_INDEL, dl, il, read_off), false, n_valid, recompute);
            } else {
                ok = pre_take_key(t, in, pr, lo, hi, whole, r, pre_find_key(t, in, ref_head, SK_INDEL_BP_LEFT, 0, 0, 0), false, n_valid, recompute) &&
                     pre_take_key(t, in, pr, lo, hi, whole, r, pre_find_key(t, in, ref_head + int32_t(dl), SK_INDEL_BP_RIGHT, 0, 0, 0), false, n_valid, recompute);
            }
        } else if (t.has_mismatch_keys && seg_align_match(s.type)) {
            for (uint32_t i = 0; i < s.length; ++i) {
                const uint32_t rp = read_off + i;
                const uint8_t sb = rp < uint32_t(in.n_code) ? in.code[rp] : uint8_t(SK_BAM_ANY);
                if (sb == SK_BAM_REF || sb == SK_BAM_ANY) continue;
                const int32_t refp = ref_head + int32_t(i);
                if (sb == pre_char_code(pre_ref_base(t, refp))) continue;
                (void)pre_take_key(t, in, pr, lo, hi, whole, r, pre_find_key(t, in, refp, SK_INDEL_MISMATCH, 1, 1, 0, pre_code_char(sb)), true, n_valid, recompute);
            }
        }
        for (int i = 0; i < n_seg; ++i, ++pi) { // increment_path
            const PSeg q = c.path[pi];
            if (seg_align_match(q.type)) {
                read_off += q.length;
                ref_head += int32_t(q.length);
            } else if (q.type == SK_SEG_DELETE || q.type == SK_SEG_SKIP) {
                ref_head += int32_t(q.length);
            } else if (q.type == SK_SEG_INSERT || q.type == SK_SEG_SOFT_CLIP) {
                read_off += q.length;
            }
        }
    }
    if (!ok) return SK_RPRE_EXEMPLAR_KEY_MISSING;
    int status = SK_RPRE_OK;
    if (whole && recompute) {
        const int32_t read_start = int32_t(unaligned_prefix(c)), ref_start = c.pos;
        const bool fwd = c.fwd != 0;
        const int n_old = c.n_seg;
        if (make_start_pos_alignment(t.job, ref_start, read_start, fwd, unsigned(in.read_len), c.indels, n_valid, c) != ST_OK) status = SK_RPRE_CAP_P;
        for (int i = c.n_seg; i < n_old; ++i) c.path[i].type = c.path[i].length = 0;
    }
    for (int i = 0; i < n_valid; ++i) c.indels[i] = 0;
    c.n_indels = 0;
    return status;
}

// P5 and the record's plain fields.  r.cal, r.sm and r.n_sm are set; the rest of `r` is zero.
SKC_HD inline int pre_finish(const PreRead& in, const PRange& exemplar, PRead& r)
{
    int n = 0;
    for (int i = 0; i < r.n_sm; ++i)
        if (r.sm[i].is_present) r.order[n++] = r.sm[i].idx;
    for (int i = 0; i < r.n_sm; ++i)
        if (!r.sm[i].is_present) r.order[n++] = r.sm[i].idx;
    r.n_order = uint8_t(n);
    PreView v{ r.sm, r.order, r.cal.indels, r.n_sm, r.n_order };
    sort_remove_only_indels_last(v, 0);
    for (int i = 0; i < n; ++i) r.cal.indels[i] = 0;
    PCal& c = r.cal;
    uint32_t read_length = uint32_t(in.read_len);
    const unsigned t0 = c.n_seg ? c.path[0].type : unsigned(SK_SEG_NONE), t1 = c.n_seg > 1 ? c.path[c.n_seg - 1].type : unsigned(SK_SEG_NONE);
    if (t0 == SK_SEG_SOFT_CLIP || t0 == SK_SEG_HARD_CLIP || t1 == SK_SEG_SOFT_CLIP || t1 == SK_SEG_HARD_CLIP) { // is_clipped (align_path.cpp:770-781) -> clip_clipper
        r.clipped = 1;
        bool lead = true;
        int w = 0;
        for (int i = 0; i < c.n_seg; ++i) {
            const PSeg s = c.path[i];
            if (s.type == SK_SEG_HARD_CLIP) (lead ? r.hc_lead : r.hc_trail) += s.length;
            else if (s.type == SK_SEG_SOFT_CLIP) (lead ? r.sc_lead : r.sc_trail) += s.length;
            else {
                lead = false;
                c.path[w++] = s;
            }
        }
        pre_cut_path(c, w);
        read_length -= r.sc_lead + r.sc_trail;
    }
    if (read_length > 0xffffu) return SK_RPRE_CAP_P;
    if (in.n_observed > Caps::OBS) return SK_RPRE_CAP_OBS;
    r.realign_b = in.realign_b;
    r.realign_e = in.realign_e;
    r.read_length = int32_t(read_length);
    r.sample = in.sample;
    r.exemplar_range.b = exemplar.b;
    r.exemplar_range.e = exemplar.e;
    r.exemplar_range.has_b = r.exemplar_range.has_e = 1;
    for (int i = 0; i < in.n_observed; ++i) r.observed[i] = int16_t(in.observed[i]);
    r.n_observed = uint8_t(in.n_observed);
    return SK_RPRE_OK;
}

// the steps around P3, which the host runs key by key and the kernel 64 keys to a turn
SKC_HD inline int pre_before_map(const PreTable& t, const PreRead& in, PRead& r, PRange& exemplar)
{
    if (t.job.n_tab > PRE_MAX_TAB) return SK_RPRE_CAP_K;
    int status = pre_normalise(in, r.cal);
    if (status == SK_RPRE_OK) status = pre_edge_keys(t, in, r.cal);
    if (status == SK_RPRE_OK) exemplar = soft_clip_range(r.cal);
    return status;
}
SKC_HD inline int pre_after_map(const PreTable& t, const PreRead& in, const PRange& exemplar, const bool whole, PRead& r)
{
    int status = pre_exemplar_keys(t, in, exemplar, whole, r);
    if (status == SK_RPRE_OK && !whole) status = SK_RPRE_CAP_K;
    if (status == SK_RPRE_OK) status = pre_finish(in, exemplar, r);
    return status;
}

// one read, start to end; `r` is zero at entry and holds the record when the status is SK_RPRE_OK
SKC_HD inline int preamble_read(const PreTable& t, const PreRead& in, PRead& r)
{
    PRange exemplar = mk_range(0, 0);
    const int status = pre_before_map(t, in, r, exemplar);
    if (status != SK_RPRE_OK) return status;
    const bool whole = pre_status_map(t, in, exemplar, r);
    return pre_after_map(t, in, exemplar, whole, r);
}

} // namespace skcore
