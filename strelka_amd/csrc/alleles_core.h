// alleles_core.h -- the walk of ActiveRegionProcessor::discoverIndelsAndMismatches after the aligner call
// (L/starling_common/ActiveRegionProcessor.cpp:593-706) as container-free code for the device and the host alike: what ONE segment of
// the aligner's path contributes, given the reference position and the haplotype offset the segments before it leave.  A segment's
// keys depend on nothing else, so the host walks the path in a loop (host/active_region.cpp, sk_discover_indels_and_mismatches) and the
// device gives every segment a lane (csrc/region_alleles.hip); both place the keys in path order.
#pragma once

#include "strelka_amd.h"

#include <stdint.h>

#if defined(__HIP__)
#define SKA_HD __host__ __device__
#else
#define SKA_HD
#endif

namespace skalleles
{

enum {
    ERR_NONE = 0,
    ERR_PATH,       // the path reads past the haplotype's end
    ERR_SEGMENT,    // a segment type the reference asserts on (:703-704)
    ERR_LEFT_SHIFT  // an all-N indel left of an all-N reference: the reference's loop (:645-653, :678-684) would not end
};

struct Walk // what the walk reads besides the path
{
    const char* ref; // reference_contig_segment::get_base: 'N' outside [ref_offset, ref_offset + ref_len)
    int32_t ref_offset, ref_len;
    int32_t ar_end;      // _posRange.end_pos()
    int32_t prev_ar_end; // _prevActiveRegionEnd
    uint32_t max_indel_size;
    const char* hap; // the selected haplotype
    int32_t hap_len;
};
SKA_HD inline char ref_base(const Walk& w, const int64_t pos)
{
    return (pos < int64_t(w.ref_offset) || pos >= int64_t(w.ref_offset) + w.ref_len) ? 'N' : w.ref[pos - w.ref_offset];
}

struct Seg // one path segment's contribution
{
    int32_t d_ref, d_hap; // what it adds to referencePos and haplotypePosOffset
    int32_t n_keys;       // the keys it emits: one per mismatched base at or after prev_ar_end, or one kept indel
    int32_t n_ins;        // their insert bytes
    int32_t n_indels;     // what it adds to numIndels
    int32_t pos;          // its first key's position (an indel's: after the left shift)
    int32_t shift;        // an indel: the positions it moved left; a mismatch segment: its first emitted base
    int32_t err;
};

/// the advance alone (:609-612, :628-629, :664, :695, :700); false: a segment type the reference asserts on
SKA_HD inline bool advance(const uint32_t type, const uint32_t length, int32_t* d_ref, int32_t* d_hap)
{
    const bool is_match = type == SK_SEG_SEQ_MATCH || type == SK_SEG_SEQ_MISMATCH;
    // SOFT_CLIP as the reference does (:698-702): the reference position moves, the haplotype offset does not
    const bool moves_ref = is_match || type == SK_SEG_DELETE || type == SK_SEG_SOFT_CLIP;
    const bool moves_hap = is_match || type == SK_SEG_INSERT;
    *d_ref = moves_ref ? int32_t(length) : 0;
    *d_hap = moves_hap ? int32_t(length) : 0;
    return moves_ref || moves_hap;
}

SKA_HD inline Seg segment(const Walk& w, const uint32_t type, const uint32_t length, const int32_t reference_pos, const int32_t hap_off)
{
    Seg s;
    s.n_keys = s.n_ins = s.n_indels = s.pos = s.shift = 0;
    s.err = advance(type, length, &s.d_ref, &s.d_hap) ? ERR_NONE : ERR_SEGMENT;
    if (s.err) return s;
    const int64_t len = int64_t(length);
    if ((type == SK_SEG_SEQ_MISMATCH || type == SK_SEG_INSERT) && int64_t(hap_off) + len > int64_t(w.hap_len)) {
        s.err = ERR_PATH;
        return s;
    }
    if (type == SK_SEG_SEQ_MISMATCH) { // one MISMATCH key per base; two regions may share a base (:617-626)
        int64_t first = int64_t(w.prev_ar_end) - reference_pos;
        first = first < 0 ? 0 : first;
        if (first < len) {
            s.n_keys = s.n_ins = int32_t(len - first);
            s.pos = int32_t(reference_pos + first);
            s.shift = int32_t(first);
        }
    } else if (type == SK_SEG_INSERT) {
        if (length > w.max_indel_size) return s;
        // left-align: move while the last inserted base equals the base before (:642-653).  After k moves the insert is the first
        // `length` characters of (the k reference bases before reference_pos) + (the haplotype's insert).
        int64_t k = 0;
        char prev = ref_base(w, int64_t(reference_pos) - 1);
        for (;;) {
            const int64_t last = len - 1 - k;
            const char back = last >= 0 ? w.hap[hap_off + last] : ref_base(w, int64_t(reference_pos) - k + len - 1);
            if (back != prev) break;
            ++k;
            prev = ref_base(w, int64_t(reference_pos) - k - 1);
            if (int64_t(reference_pos) - k < int64_t(w.ref_offset) - len) {
                s.err = ERR_LEFT_SHIFT;
                return s;
            }
        }
        const int64_t insert_pos = int64_t(reference_pos) - k;
        if (prev != 'N' && insert_pos >= w.prev_ar_end && insert_pos < w.ar_end) { // (:657)
            s.n_keys = s.n_indels = 1;
            s.n_ins = int32_t(len);
            s.pos = int32_t(insert_pos);
            s.shift = int32_t(k);
        }
    } else if (type == SK_SEG_DELETE) {
        if (length > w.max_indel_size) return s;
        int64_t delete_pos = reference_pos; // (:675-684)
        char prev = ref_base(w, delete_pos - 1);
        char last_del = ref_base(w, delete_pos + len - 1);
        while (last_del == prev) {
            --delete_pos;
            last_del = ref_base(w, delete_pos + len - 1);
            prev = ref_base(w, delete_pos - 1);
            if (delete_pos < int64_t(w.ref_offset) - len) {
                s.err = ERR_LEFT_SHIFT;
                return s;
            }
        }
        if (prev != 'N' && delete_pos >= w.prev_ar_end && delete_pos < w.ar_end) { // (:688)
            s.n_keys = s.n_indels = 1;
            s.pos = int32_t(delete_pos);
            s.shift = int32_t(int64_t(reference_pos) - delete_pos);
        }
    }
    return s;
}

/// key j of a segment's s.n_keys: the IndelKey of :624, :659, :690; its insert bytes (ins_len of them) go to ins_dst
SKA_HD inline void key(const Walk& w, const uint32_t type, const uint32_t length, const int32_t reference_pos, const int32_t hap_off, const Seg& s, const int32_t j,
                       int32_t* pos, int32_t* key_type, uint32_t* del_len, uint32_t* ins_len, char* ins_dst)
{
    if (type == SK_SEG_SEQ_MISMATCH) {
        *pos = s.pos + j;
        *key_type = SK_INDEL_MISMATCH;
        *del_len = 1;
        *ins_len = 1;
        ins_dst[0] = w.hap[hap_off + s.shift + j];
    } else if (type == SK_SEG_INSERT) {
        *pos = s.pos;
        *key_type = SK_INDEL_INDEL;
        *del_len = 0;
        *ins_len = length;
        for (int64_t k = 0; k < int64_t(length); ++k)
            ins_dst[k] = k < s.shift ? ref_base(w, int64_t(reference_pos) - s.shift + k) : w.hap[hap_off + k - s.shift];
    } else {
        *pos = s.pos;
        *key_type = SK_INDEL_INDEL;
        *del_len = length;
        *ins_len = 0;
    }
}

} // namespace skalleles
