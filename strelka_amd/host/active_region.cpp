// active_region.cpp -- host stage after the GlobalAligner kernel: decompose an aligned haplotype into left-shifted
// primitive alleles.  Mirrors ActiveRegionProcessor::discoverIndelsAndMismatches
// (L/starling_common/ActiveRegionProcessor.cpp:572-697); integer/byte work, results identical to the reference's.
// The per-segment rules are csrc/alleles_core.h, which the device chain (csrc/region_alleles.hip) walks as well.
#include "strelka_amd.h"

#include "alleles_core.h"

#include <string>

int sk_fail(const std::string& msg);

extern "C" int sk_discover_indels_and_mismatches(const char* ref_seq, int32_t ref_offset, int32_t ref_len, int32_t ar_begin,
                                                 int32_t ar_end, int32_t prev_ar_end, uint32_t max_indel_size,
                                                 const char* haplotype, int32_t hap_len, int32_t align_begin_pos,
                                                 const sk_path_seg* path, int32_t n_seg, sk_discovered_allele* out,
                                                 int32_t out_cap, char* out_ins_seq, int32_t ins_cap, int32_t* n_out,
                                                 int32_t* n_indels)
{
    if (!ref_seq || !haplotype || (!path && n_seg > 0) || !out || !out_ins_seq || !n_out || !n_indels)
        return sk_fail("sk_discover_indels_and_mismatches: null argument");
    if (align_begin_pos > 0) return sk_fail("sk_discover_indels_and_mismatches: unexpected alignment segment"); // :597-600
    const skalleles::Walk w = { ref_seq, ref_offset, ref_len, ar_end, prev_ar_end, max_indel_size, haplotype, hap_len };
    int32_t reference_pos = ar_begin, hap_off = 0, n = 0, ni = 0, ins_used = 0;
    for (int32_t i = 0; i < n_seg; ++i) {
        const skalleles::Seg s = skalleles::segment(w, path[i].type, path[i].length, reference_pos, hap_off);
        switch (s.err) {
        case skalleles::ERR_NONE: break;
        case skalleles::ERR_PATH: return sk_fail("sk_discover_indels_and_mismatches: path longer than the haplotype");
        case skalleles::ERR_LEFT_SHIFT: return sk_fail("sk_discover_indels_and_mismatches: unbounded left shift");
        default: return sk_fail("sk_discover_indels_and_mismatches: unexpected alignment segment");
        }
        if (s.n_keys > out_cap - n || s.n_ins > ins_cap - ins_used) return sk_fail("sk_discover_indels_and_mismatches: output capacity exceeded");
        for (int32_t j = 0; j < s.n_keys; ++j) {
            sk_discovered_allele& o = out[n++];
            o.ins_off = ins_used;
            skalleles::key(w, path[i].type, path[i].length, reference_pos, hap_off, s, j, &o.pos, &o.type, &o.del_len, &o.ins_len, out_ins_seq + ins_used);
            ins_used += int32_t(o.ins_len);
        }
        ni += s.n_indels;
        reference_pos += s.d_ref;
        hap_off += s.d_hap;
    }
    *n_out = n;
    *n_indels = ni;
    return 0;
}
