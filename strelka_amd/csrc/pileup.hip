// pileup.hip -- row a8: project aligned reads into per-locus basecall columns.
//
// Reference: starling_pos_processor_base::pileup_read_segment (L/starling_common/starling_pos_processor_base.cpp:1127-1421)
// with create_mismatch_filter_map (L/starling_common/starling_read_util.cpp:40-213), qphred_to_mapped_qphred
// (L/blt_util/qscore.hh:104-121), getReadAmbiguousEndLength (L/htsapi/bam_seq_read_util.cpp:29-54), base_call
// (L/blt_common/snp_pos_info.hh:53-123) and, for the cleaned modes, PileupCleaner::CleanPileupFilter
// (L/starling_common/PileupCleaner.cpp:28-66).  Integer/byte work: results are identical to the reference's, including the
// order of the calls inside a column (read order).
//
// The reference appends one basecall at a time to a position-keyed map as each read passes the pileup stage.  Here the
// same columns are built without any ordered scatter:
//   P1 `pileup_read_kernel`   one wave per read, lanes = read positions.  Mismatch-density counts come from the
//        reference's difference array (LDS atomics + a wave scan); every read base gets a 16-bit RECORD in read-major
//        order: the packed base_call, bit 14 = "tier2 stream", bit 15 = "emitted".  Spanning-deletion / submapped
//        counters are order-free and use global atomics.
//   P2 `pileup_column_kernel` one wave per 64 consecutive loci, lanes = loci.  The wave walks the reads overlapping its
//        loci IN READ ORDER (read geometry is wave-uniform, in SGPRs); a lane whose locus falls in a match segment loads
//        that base's record (adjacent lanes read adjacent bases: coalesced) and, if the record belongs to the requested
//        mode, counts it (first launch) or stores it at call_off[locus] + its running count (second launch).  Read order
//        inside a column is therefore exact by construction.
//   Between the two P2 launches an exclusive scan turns counts into CSR offsets; two more scans (prefix max of read
//   ends, suffix min of read begins) bound the read range a wave has to look at.  The scans are rocPRIM's.
//
// Roofline: HBM-bound, ~4 B per read base in P1 (code, quality in; 2-byte record out) and ~2 x 2 B per call in P2.
//
// The device code is in pileup_read.h (constants, PileupArgs, P1), pileup_column.h (P2) and pileup_steps.h (the small launches around them),
// included here and nowhere else; this file is the host side: the blocks a call carves, the check of a read batch, the entry points, the stream.

#include <cstring>

#include <hip/hip_runtime.h>

#include <rocprim/device/device_scan.hpp>

#include "sk_common.h"

#include <algorithm>
#include <chrono>
#include <climits>
#include <iterator>
#include <vector>

#include "pileup_read.h"
#include "pileup_column.h"
#include "pileup_steps.h"

namespace
{

// ---- blocks of device memory.  Each block of a call is stated once, by a carve function over an SkArena placed on the block: on a dry
// arena (no base) the carve only counts, which gives the block's size; on the block it hands out typed pointers.  Every array starts
// on a 256-byte boundary.  An array a call does not need is not carved: it takes no room and its pointer stays null.
inline SkArena arena_on(void* base) { SkArena ar; ar.base = static_cast<char*>(base); return ar; }
template <typename F> size_t carved_bytes(F&& carve) { SkArena dry; (void)carve(dry); return sk_align256(dry.used); }
// the page-locked mirror of a block's array: the same offset from the mirror's base (there is one layout, the device block's)
template <typename T> T* mirror(const SkPinBuf& host, const SkDevBuf& dev, T* dev_array)
{
    return reinterpret_cast<T*>(host.as<char>() + (reinterpret_cast<const char*>(dev_array) - dev.as<char>()));
}

// the one-shot pileup's scratch (sk_pileup_scratch_bytes)
struct ScratchBlock
{
    uint16_t* rec; int2* span; int *begin, *end, *maxend, *minbegin; uint32_t* count;
    char* tmp; size_t tmp_bytes; // the device library's scan storage
};

// with_scans: the one-shot pileup's three device-library scans need temporary storage, sized by asking the library -- which asks the HIP
// runtime about the device.  The STREAM does not use those scans (column_offsets_kernel), carves no such block and must not ask: in a
// client of the broker the question costs ~1 ms per push and wakes a runtime the process is not supposed to have (profiles/r06_v22: 3.8
// of a farm's 5.4 pileup ABI seconds were this line).
ScratchBlock carve_scratch(SkArena& ar, const int32_t n_reads, const int64_t n_bases, const int32_t n_loci, const bool with_scans = true)
{
    const size_t nr = size_t(std::max(n_reads, 1));
    ScratchBlock s;
    s.rec = ar.take<uint16_t>(size_t(std::max<int64_t>(n_bases, 1)));
    s.span = ar.take<int2>(nr);
    s.begin = ar.take<int>(nr); s.end = ar.take<int>(nr);
    s.maxend = ar.take<int>(nr); s.minbegin = ar.take<int>(nr);
    s.count = ar.take<uint32_t>(size_t(n_loci) + 1);
    size_t t1 = 0, t2 = 0, t3 = 0;
    if (with_scans) {
        int* ip = nullptr;
        uint32_t* up = nullptr;
        int64_t* lp = nullptr;
        (void)rocprim::inclusive_scan(nullptr, t1, ip, ip, nr, MaxOp());
        (void)rocprim::inclusive_scan(nullptr, t2, std::make_reverse_iterator(ip), std::make_reverse_iterator(ip), nr, MinOp());
        (void)rocprim::exclusive_scan(nullptr, t3, up, lp, int64_t(0), size_t(n_loci) + 1, rocprim::plus<int64_t>());
    }
    s.tmp_bytes = std::max(t1, std::max(t2, t3)) + 256;
    s.tmp = ar.take<char>(s.tmp_bytes);
    return s;
}

// ---- what the reference rejects of a read batch by throwing / exiting, for the one-shot entry and both streams' pushes (`who`: the
// entry point the messages name).  *quality_above_70: some base's quality is above 70, whether or not that is refused here.
// The bases are scanned without a branch first -- the check is on a window's path -- and only a batch in which that scan found something
// is walked again for the first offender in base order.
int check_read_batch(const char* who, const sk_read_batch* b, const bool is_mapq_adjust, bool* quality_above_70)
{
    auto fail = [who](const char* what) { return sk_fail(std::string(who) + ": " + what); };
    const int n = b->n_reads;
    if (n > 0 && (b->read_off[0] != 0 || b->path_off[0] != 0)) return fail("CSR offsets must start at 0");
    for (int r = 0; r < n; ++r) {
        const int64_t L = b->read_off[r + 1] - b->read_off[r];
        if (L < 0 || b->path_off[r + 1] < b->path_off[r]) return fail("bad CSR offsets");
        if (L > MAX_READ_LEN) return fail("read longer than 1024 bases");
        int64_t plen = 0;
        for (int64_t i = b->path_off[r]; i < b->path_off[r + 1]; ++i) {
            const uint32_t t = b->path[i].type;
            if (seg_read_len(t)) plen += b->path[i].length;
            else if (!(t == SK_SEG_DELETE || t == SK_SEG_HARD_CLIP || t == SK_SEG_SKIP))
                return fail("Can't handle cigar code"); // starling_read_util.cpp:198-203
        }
        if (b->path_off[r + 1] > b->path_off[r] && plen != L) return fail("alignment path does not span its read");
    }
    const int64_t n_bases = n ? b->read_off[n] : 0;
    auto code_ok = [](const uint8_t c) { return c == SK_BAM_REF || c == SK_BAM_A || c == SK_BAM_C || c == SK_BAM_G || c == SK_BAM_T || c == SK_BAM_ANY; };
    unsigned bad_code = 0, bad_q = 0;
    for (int64_t i = 0; i < n_bases; ++i) {
        bad_code |= unsigned(!code_ok(b->read_code[i]));
        bad_q |= unsigned(b->read_qual[i] > 70);
    }
    *quality_above_70 = (bad_q != 0);
    if (!bad_code && !(bad_q && is_mapq_adjust)) return 0;
    for (int64_t i = 0; i < n_bases; ++i) {
        if (!code_ok(b->read_code[i])) return fail("unsupported BAM base code"); // bam_seq_code_to_id base_error, bam_seq.hh:145-147
        if (is_mapq_adjust && b->read_qual[i] > 70)
            return sk_fail("Attempting to lookup basecall quality score " + std::to_string(int(b->read_qual[i])) +
                           " which exceeds the maximum cached basecall quality score of 70");
    }
    return 0;
}

// P2 of one column (the one-shot entry): a launch that fills the device anyway keeps one wave to a block (pileup_column.h)
void launch_column(const PileupArgs& a, const int blocks, hipStream_t st)
{
    if (blocks >= P2_SPLIT_BELOW_BLOCKS) SK_LAUNCH((pileup_column_kernel_t<false, false, false, 1>), dim3(blocks), dim3(WAVE), 0, st, a);
    else SK_LAUNCH(pileup_column_kernel_t<false>, dim3(blocks), dim3(WAVE * P2_WAVES_MAX), 0, st, a);
}

} // namespace

extern "C" {

void sk_pileup_options_default(sk_pileup_options* o)
{
    o->min_basecall_qscore = 17;
    o->mismatch_density_flank_size = 20;
    o->mismatch_density_max_count = 2;
    o->use_tier2_evidence = 0;
    o->tier2_mismatch_density_max_count = 10;
    o->is_mapq_adjust = 1;
    o->min_distance_from_read_edge = 0;
    o->largest_total_indel_ref_span_per_read = 49;
    o->report_begin = 0;
    o->report_end = 0;
}

int64_t sk_pileup_scratch_bytes(const int32_t n_reads, const int64_t n_bases, const int32_t n_loci)
{
    if (n_reads < 0 || n_bases < 0 || n_loci < 0) return -1;
    // (a broker client never asks the device library: the one-shot pileup is not its to run)
    return int64_t(carved_bytes([&](SkArena& ar) { return carve_scratch(ar, n_reads, n_bases, n_loci, !skrt::remote()); }));
}

int sk_pileup_reads_dev(const sk_read_batch* b, const int64_t n_bases, const sk_pileup_options* opt, const int mode,
                        sk_pileup_columns* out, void* dev_scratch, void* hip_stream)
{
    SK_REQUIRE_INIT();
    if (skrt::remote())
        return sk_fail("sk_pileup_reads: the one-shot pileup uses the device library's scans, which a broker client cannot call; a broker client piles up through "
                       "sk_pileup_stream_* (unset STRELKA_AMD_BROKER for this entry point)");
    if (!b || !opt || !out || !dev_scratch) return sk_fail("sk_pileup_reads_dev: null argument");
    if (mode < SK_PILEUP_RAW_TIER1 || mode > SK_PILEUP_CLEAN_TIER2) return sk_fail("sk_pileup_reads_dev: unknown mode");
    if (opt->report_end < opt->report_begin || out->n_loci != opt->report_end - opt->report_begin)
        return sk_fail("sk_pileup_reads_dev: n_loci must equal report_end - report_begin");
    if (b->n_reads < 0 || n_bases < 0) return sk_fail("sk_pileup_reads_dev: negative count");
    if (!out->call_off || !out->calls) return sk_fail("sk_pileup_reads_dev: null output");
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    const int n_loci = out->n_loci;
    SkArena ar = arena_on(dev_scratch);
    const ScratchBlock S = carve_scratch(ar, b->n_reads, n_bases, n_loci);
    PileupArgs a;
    a.b = *b; a.o = *opt; a.tab = sk_ctx().dev_tables;
    a.rec = S.rec; a.span = S.span; a.maxend = S.maxend; a.minbegin = S.minbegin; a.count = S.count;
    a.call_off = out->call_off; a.calls = out->calls; a.spandel = out->spandel_count; a.submapped = out->submapped_count;
    a.n_loci = n_loci; a.mode = mode; a.store = 0; a.r0 = 0;
    size_t tmp_bytes = S.tmp_bytes;

    if (a.spandel && n_loci) SK_HIP(skrt::memsetAsync(a.spandel, 0, 4 * size_t(n_loci), st));
    if (a.submapped && n_loci) SK_HIP(skrt::memsetAsync(a.submapped, 0, 4 * size_t(n_loci), st));
    if (b->n_reads > 0) {
        SK_LAUNCH(pileup_read_kernel, dim3((b->n_reads + P1_WAVES - 1) / P1_WAVES), dim3(P1_WAVES * WAVE), 0, st, a);
        SK_LAUNCH(span_split_kernel, dim3((b->n_reads + 255) / 256), dim3(256), 0, st, a.span, S.begin, S.end, b->n_reads);
        SK_HIP(rocprim::inclusive_scan(S.tmp, tmp_bytes, S.end, S.maxend, size_t(b->n_reads), MaxOp(), st));
        tmp_bytes = S.tmp_bytes;
        SK_HIP(rocprim::inclusive_scan(S.tmp, tmp_bytes, std::make_reverse_iterator(S.begin + b->n_reads),
                                       std::make_reverse_iterator(S.minbegin + b->n_reads), size_t(b->n_reads), MinOp(), st));
    }
    const int blocks = (n_loci + 1 + WAVE - 1) / WAVE; // the extra locus carries the total through the scan
    launch_column(a, blocks, st);
    tmp_bytes = S.tmp_bytes;
    SK_HIP(rocprim::exclusive_scan(S.tmp, tmp_bytes, a.count, out->call_off, int64_t(0), size_t(n_loci) + 1, rocprim::plus<int64_t>(), st));
    // capacity check needs the total on the host
    int64_t total = 0;
    SK_HIP(skrt::memcpyAsync(&total, out->call_off + n_loci, sizeof(int64_t), hipMemcpyDeviceToHost, st));
    SK_HIP(skrt::streamSynchronize(st));
    if (total > out->capacity) return sk_fail("sk_pileup_reads_dev: calls capacity too small");
    a.store = 1;
    if (total > 0) launch_column(a, blocks, st);
    SK_HIP(skrt::getLastError());
    return 0;
}

int sk_pileup_reads(const sk_read_batch* hb, const sk_pileup_options* opt, const int mode, sk_pileup_columns* out)
{
    SK_REQUIRE_INIT();
    if (!hb || !opt || !out) return sk_fail("sk_pileup_reads: null argument");
    if (hb->n_reads < 0) return sk_fail("sk_pileup_reads: negative n_reads");
    if (opt->report_end < opt->report_begin || out->n_loci != opt->report_end - opt->report_begin)
        return sk_fail("sk_pileup_reads: n_loci must equal report_end - report_begin");
    bool quality_above_70;
    if (check_read_batch("sk_pileup_reads", hb, opt->is_mapq_adjust != 0, &quality_above_70)) return 1;
    const size_t n = size_t(hb->n_reads), n_loci = size_t(out->n_loci);
    const int64_t n_bases = n ? hb->read_off[n] : 0, n_segs = n ? hb->path_off[n] : 0;

    SkContext& ctx = sk_ctx();
    SK_HIP(skrt::setDevice(ctx.device));
    hipStream_t st = ctx.stream;
    const size_t scratch = size_t(sk_pileup_scratch_bytes(hb->n_reads, n_bases, out->n_loci));
    struct
    {
        int64_t* read_off; uint8_t* read_code; uint8_t* read_qual; int64_t* path_off; sk_path_seg* path; int32_t* pos; uint8_t* is_fwd;
        uint8_t* mapq; uint8_t* map_level; char* ref_seq; uint8_t* mask; int64_t* call_off; uint16_t* calls; uint32_t* spandel;
        uint32_t* submapped; char* scratch;
    } d;
    int rc = 0;
    if (sk_carve(d, [&](SkArena& ar) {
            // (an array the caller left null -- allowed where nothing reads it: no reads, no reference -- gets its room and no copy)
            auto up = [&](const auto* src, const size_t k) { return ar.up(src, src ? k : 0, src ? 0 : k, st, rc); };
            return decltype(d){ up(hb->read_off, n + 1), up(hb->read_code, size_t(n_bases)), up(hb->read_qual, size_t(n_bases)), up(hb->path_off, n + 1),
                                up(hb->path, size_t(n_segs)), up(hb->pos, n), up(hb->is_fwd, n), up(hb->mapq, n), up(hb->map_level, n),
                                up(hb->ref_seq, size_t(hb->ref_len)), hb->cand_snv_mask ? up(hb->cand_snv_mask, size_t(hb->ref_len)) : nullptr,
                                ar.take<int64_t>(n_loci + 1), ar.take<uint16_t>(size_t(std::max<int64_t>(out->capacity, 1))),
                                ar.take<uint32_t>(std::max<size_t>(n_loci, 1)), ar.take<uint32_t>(std::max<size_t>(n_loci, 1)), ar.take<char>(scratch) };
        }) || rc)
        return 1;
    sk_read_batch db = *hb;
    db.read_off = d.read_off; db.read_code = d.read_code; db.read_qual = d.read_qual; db.path_off = d.path_off; db.path = d.path;
    db.pos = d.pos; db.is_fwd = d.is_fwd; db.mapq = d.mapq; db.map_level = d.map_level; db.ref_seq = d.ref_seq; db.cand_snv_mask = d.mask;
    sk_pileup_columns dc = *out;
    dc.call_off = d.call_off; dc.calls = d.calls; dc.spandel_count = d.spandel; dc.submapped_count = d.submapped;
    if (sk_pileup_reads_dev(&db, n_bases, opt, mode, &dc, d.scratch, st)) return 1;
    SK_HIP(skrt::memcpyAsync(out->call_off, dc.call_off, 8 * (n_loci + 1), hipMemcpyDeviceToHost, st));
    SK_HIP(skrt::streamSynchronize(st));
    const int64_t total = out->call_off[n_loci];
    if (total > 0) SK_HIP(skrt::memcpyAsync(out->calls, dc.calls, 2 * size_t(total), hipMemcpyDeviceToHost, st));
    if (out->spandel_count && n_loci) SK_HIP(skrt::memcpyAsync(out->spandel_count, dc.spandel_count, 4 * n_loci, hipMemcpyDeviceToHost, st));
    if (out->submapped_count && n_loci) SK_HIP(skrt::memcpyAsync(out->submapped_count, dc.submapped_count, 4 * n_loci, hipMemcpyDeviceToHost, st));
    SK_HIP(skrt::streamSynchronize(st));
    return 0;
}

} // extern "C"

// =====================================================================================================================
// The pileup of one sample as a stream over a genome segment (sk_pileup_stream_*, include/strelka_amd.h).
//
// The reference piles reads up one at a time as its READ_BUFFER stage passes them and genotypes a position when the
// POST_ALIGN stage, largest_total_indel_ref_span_per_read positions behind, gets there
// (L/starling_common/starling_pos_processor_base.cpp:141-224, :810-890).  A caller of this stream hands over the reads of
// one stage window at a time, in read-buffer order, together with the position up to which no later read can add a
// basecall (`final_to`, the POST_ALIGN position of the window's end).  A push
//   * runs P1 on the new reads only: their records join, on the device, those of the earlier reads that still reach past
//     the previous `final_to` (the carried tail -- a few dozen reads: two record buffers used alternately, the tail is copied
//     across), so every read meets the candidate-SNV mask exactly once, as in the reference;
//   * runs the three-column P2 over [begin, end) = the not yet finalised positions below `final_to` that the batch covers:
//     raw tier1 / tier2 columns (snp_pos_info::calls / tier2_calls), the CleanPileupFilter'ed tier1 column, the MAPQ
//     tracker; spanning-deletion and submapped counters are P1's region-wide atomics;
//   * chains a9+a10 (germline_site_fused_kernel) on the cleaned columns where they lie in HBM;
//   * brings everything the host-side position processor keeps per position back in one copy.
// One host synchronisation per push.
// =====================================================================================================================

namespace
{

inline int path_ref_length(const sk_path_seg* path, const int nseg)
{
    int n = 0;
    for (int i = 0; i < nseg; ++i)
        if (seg_ref_len(path[i].type)) n += int(path[i].length);
    return n;
}

// diagnostics ($SK_PILEUP_PUSH_SECONDS): where a push's wall time goes -- checks, packing + submissions, the wait, the carry bookkeeping
struct PushSeconds
{
    bool on = std::getenv("SK_PILEUP_PUSH_SECONDS") != nullptr;
    double check = 0, enqueue = 0, wait = 0, finish = 0, enq_buffers = 0, enq_pack = 0, enq_submit = 0;
    // the steps of stream_enqueue: H2D, carry copies, work / output blocks, P1 + span bounds, P2 + offsets, germline chain, D2H
    double lap[10] = { 0, 0, 0, 0, 0, 0, 0, 0, 0, 0 };
    long pushes = 0;
    ~PushSeconds()
    {
        if (!on || !pushes) return;
        std::fprintf(stderr, "strelka_amd pileup push seconds: pushes=%ld check=%.4f enqueue=%.4f wait=%.4f finish=%.4f enq_buffers=%.4f enq_pack=%.4f enq_submit=%.4f\n", pushes, check, enqueue, wait, finish,
                     enq_buffers, enq_pack, enq_submit);
        std::fprintf(stderr, "strelka_amd pileup push laps:");
        for (int i = 0; i < 10; ++i) std::fprintf(stderr, " %.4f", lap[i]);
        std::fprintf(stderr, "\n");
    }
    static double now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
} g_push_seconds;

// adds the time from its construction to the end of its scope to one of g_push_seconds' sums; reads no clock when the diagnostic is off
struct PushLap
{
    double* sum;
    double t0;
    explicit PushLap(double& s) : sum(g_push_seconds.on ? &s : nullptr), t0(sum ? PushSeconds::now() : 0.0) {}
    ~PushLap() { if (sum) *sum += PushSeconds::now() - t0; }
};

// ---- the three blocks of a push (carved below, after the stream they are sized from)
struct InBlock // host -> device, one copy: the carried reads' metadata and the new reads, the window's ploidy, the mask's window
{
    int64_t *read_off, *path_off; sk_path_seg* path; int32_t* pos; uint8_t *is_fwd, *mapq, *level, *ploidy, *code, *qual, *mask;
};
struct WorkBlock // stays on the device
{
    int *begin, *end, *maxend, *minbegin;
    uint32_t* count[3]; // raw tier1, raw tier2, cleaned tier1
    uint32_t *count4, *count4a; int64_t *off2, *off4; uint16_t *calls2, *calls4;
    uint8_t* refbase; float* de; char *gscr, *pods;
};
struct OutBlock // device -> host, one copy: what sk_pileup_window points into
{
    int64_t *off0, *off1; uint32_t *clean_n, *clean4_n, *mq_n, *mq_zero; unsigned long long* mq_sq; uint32_t *spandel, *submapped;
    sk_digt_call* geno; sk_gvcf_site_summary* summary; sk_gvcf_run* runs;
    uint16_t *calls0, *calls1; uint32_t* read_pos; int64_t* evs_off; unsigned long long* evs;
};

// one push of a stream, from stream_enqueue to stream_finish: its counts, its range and its blocks' arrays
struct Push
{
    int n = 0, n_c = 0, n_new = 0, n_loci = 0;     // reads (carried + new), positions of the window
    int64_t n_bases = 0, n_segs = 0;
    int64_t n_bases_tier2 = 0;                     // the bases of the reads that are not tier1-mapped
    int32_t begin = 0, end = 0, F = 0, mask_len = 0;
    size_t in_bytes = 0, out_bytes = 0;            // the input and the output block: what the push's two copies move
    InBlock in = {}; WorkBlock work = {}; OutBlock out = {};
};

} // namespace

struct sk_pileup_stream
{
    sk_pileup_options opt;
    sk_germline_options gopt;
    bool genotype = false;
    bool somatic = false;      // also build the CleanPileupFilter(pi, true) column (kept on the device)
    bool want_read_pos = false; // ... and return each tier1 call's read position / read length
    bool want_evs = false;      // return the germline EVS words of every live call (sk_pileup_stream_enable_evs_words)
    bool want_runs = false;     // return the non-variant block that would start at every plain site (sk_pileup_stream_set_gvcf_block_options)
    sk_gvcf_block_options gvcf_opt;
    bool poisoned = false;      // a push failed after it had begun to change the stream's state: only begin_region is accepted
    bool in_flight = false;     // between sk_pileup_stream_push_begin and _finish: the device is working on the window
    // region
    bool has_region = false;
    int32_t ref_offset = 0, ref_len = 0;
    int32_t region_begin = 0, region_end = 0;
    SkDevBuf d_ref, d_mask, d_spandel, d_submapped;
    // carried reads: metadata on the host, records and spans on the device
    std::vector<int32_t> c_len, c_nseg, c_pos;
    std::vector<uint8_t> c_mapq, c_level;
    std::vector<sk_path_seg> c_path;
    int64_t c_bases = 0;
    int64_t c_tail_base = 0; // where the carried reads' records start in d_rec[cur]
    int64_t c_tail_read = 0; // ... and their spans in d_span[cur]
    int cur = 0;
    SkDevBuf d_rec[2], d_span[2];
    bool has_prev = false;
    int32_t next_begin = 0;
    SkDevBuf d_in2[2], d_work, d_out; // (two input blocks used alternately: with want_evs the carried reads' bases and qualities are copied across)
    int cur_in = 0;
    // the output block of a push: OUT_BLOCKS of them in rotation, so that a window's arrays outlive the next pushes (strelka_amd.h,
    // sk_pileup_window: the caller reads the bulk of a window -- the EVS words -- where the push left it, or not at all)
    SkPinBuf h_in, h_out_blocks[SK_PILEUP_WINDOW_LIFETIME + 1];
    int out_block = 0;
    SkPinBuf& h_out_cur() { return h_out_blocks[out_block]; }
    int64_t pushes = 0, reads_in = 0;
    Push p; // the push in flight (stream_enqueue -> stream_finish)
    template <typename T> T* in_host(T* dev_array) const { return mirror(h_in, d_in2[cur_in], dev_array); }
    template <typename T> T* out_host(T* dev_array) { return mirror(h_out_cur(), d_out, dev_array); }
};

struct sk_somatic_pileup_stream
{
    sk_pileup_stream* sample[2] = { nullptr, nullptr }; // normal, tumor
    sk_somatic_snv_options sopt;
    bool genotype = false;
    bool tier2 = false;
    SkDevBuf d_call; // forced flags, somatic records, the wrapper's scratch
    SkPinBuf h_forced, h_geno;
    bool in_flight = false; // between sk_somatic_pileup_stream_push_begin and _finish
    int p_loci = 0;         // ... the positions of the window in flight
};

namespace
{

InBlock carve_in(SkArena& ar, const Push& p)
{
    const size_t n1 = size_t(std::max(p.n, 1)), nb = size_t(std::max<int64_t>(p.n_bases, 1));
    InBlock b;
    b.read_off = ar.take<int64_t>(size_t(p.n) + 1); b.path_off = ar.take<int64_t>(size_t(p.n) + 1);
    b.path = ar.take<sk_path_seg>(size_t(std::max<int64_t>(p.n_segs, 1)));
    b.pos = ar.take<int32_t>(n1);
    b.is_fwd = ar.take<uint8_t>(n1); b.mapq = ar.take<uint8_t>(n1); b.level = ar.take<uint8_t>(n1);
    b.ploidy = ar.take<uint8_t>(size_t(std::max(p.n_loci, 1)));
    b.code = ar.take<uint8_t>(nb); b.qual = ar.take<uint8_t>(nb);
    b.mask = ar.take<uint8_t>(size_t(std::max(p.mask_len, 1)));
    return b;
}

WorkBlock carve_work(SkArena& ar, const sk_pileup_stream* s)
{
    const Push& p = s->p;
    const size_t n1 = size_t(std::max(p.n, 1)), l1 = size_t(p.n_loci) + 1, lm = size_t(std::max(p.n_loci, 1)), nb = size_t(std::max<int64_t>(p.n_bases, 1));
    const bool som = s->somatic;
    WorkBlock w = {};
    w.begin = ar.take<int>(n1); w.end = ar.take<int>(n1);
    w.maxend = ar.take<int>(n1); w.minbegin = ar.take<int>(n1);
    for (int m = 0; m < 3; ++m) w.count[m] = ar.take<uint32_t>(l1);
    if (som) { w.count4 = ar.take<uint32_t>(l1); w.count4a = ar.take<uint32_t>(l1); }
    w.off2 = ar.take<int64_t>(l1);
    if (som) w.off4 = ar.take<int64_t>(l1);
    w.calls2 = ar.take<uint16_t>(nb);
    if (som) w.calls4 = ar.take<uint16_t>(nb);
    w.refbase = ar.take<uint8_t>(lm);
    if (s->genotype) { w.de = ar.take<float>(nb); w.gscr = ar.take<char>(size_t(4 * (p.n_bases + int64_t(p.n_loci) + 8))); }
    if (s->genotype && s->want_runs) w.pods = ar.take<char>(17 * lm + 512); // (pods, then a tile per 32 of them)
    (void)ar.take<char>(256); // (spare: the block ends 256 bytes past its last array)
    return w;
}

OutBlock carve_out(SkArena& ar, const sk_pileup_stream* s)
{
    const Push& p = s->p;
    const size_t l1 = size_t(p.n_loci) + 1, lm = size_t(std::max(p.n_loci, 1)), nb = size_t(std::max<int64_t>(p.n_bases, 1));
    OutBlock o = {};
    o.off0 = ar.take<int64_t>(l1); o.off1 = ar.take<int64_t>(l1);
    o.clean_n = ar.take<uint32_t>(l1);
    if (s->somatic) o.clean4_n = ar.take<uint32_t>(l1);
    o.mq_n = ar.take<uint32_t>(l1);
    o.mq_zero = ar.take<uint32_t>(lm); o.mq_sq = ar.take<unsigned long long>(lm);
    o.spandel = ar.take<uint32_t>(lm); o.submapped = ar.take<uint32_t>(lm);
    if (s->genotype) { o.geno = ar.take<sk_digt_call>(lm); o.summary = ar.take<sk_gvcf_site_summary>(lm); }
    if (s->genotype && s->want_runs) o.runs = ar.take<sk_gvcf_run>(lm);
    o.calls0 = ar.take<uint16_t>(nb);
    // the tier2 column's room: P1 marks a record REC_TIER2 when its read is not tier1-mapped; a germline run has few such reads, and the
    // block that goes back to the host is that much smaller
    o.calls1 = ar.take<uint16_t>(size_t(std::max<int64_t>(p.n_bases_tier2, 1)));
    if (s->want_read_pos) o.read_pos = ar.take<uint32_t>(nb);
    if (s->want_evs) { o.evs_off = ar.take<int64_t>(l1); o.evs = ar.take<unsigned long long>(nb); }
    return o;
}

// the somatic push's block: the window's forced-output flags, the somatic records, the tier wrapper's scratch
struct CallBlock { uint8_t* forced; sk_somatic_snv_genotype* geno; char* scratch; };
CallBlock carve_call(SkArena& ar, const int n_loci)
{
    return CallBlock{ ar.take<uint8_t>(size_t(n_loci)), ar.take<sk_somatic_snv_genotype>(size_t(std::max(n_loci, 1))),
                      ar.take<char>(sk_somatic_snv_tiers_scratch_bytes(n_loci)) };
}

// what a push refuses before it changes anything: the stream's state, the batch (check_read_batch), the mask's window
int stream_check_reads(const sk_pileup_stream* s, const sk_read_batch* reads, const int32_t mask_begin, const int32_t mask_len,
                       const uint8_t* cand_snv_mask)
{
    if (!s->has_region) return sk_fail("sk_pileup_stream_push: no region (sk_pileup_stream_begin_region)");
    if (reads->n_reads < 0) return sk_fail("sk_pileup_stream_push: negative n_reads");
    bool quality_above_70;
    if (check_read_batch("sk_pileup_stream_push", reads, s->opt.is_mapq_adjust != 0, &quality_above_70)) return 1;
    // (without the MAPQ adjustment the raw quality goes into the calls as it is; the EVS word has seven bits for it, the
    // basecall record six: a quality the reference's own caches would throw on further down the path is refused here)
    if (quality_above_70 && s->want_evs) return sk_fail("sk_pileup_stream_push: basecall quality above 70 with the EVS column on");
    if (mask_len < 0 || (mask_len > 0 && (!cand_snv_mask || mask_begin < s->ref_offset || mask_begin + mask_len > s->ref_offset + s->ref_len)))
        return sk_fail("sk_pileup_stream_push: candidate-SNV mask window outside the reference segment");
    return 0;
}

// lowest start / highest end of the carried and the new reads (INT_MAX / INT_MIN when there are none); fails when a new read
// reaches positions an earlier push declared final
int stream_extent(const sk_pileup_stream* s, const sk_read_batch* reads, int32_t* lowest_out, int32_t* highest_out)
{
    int32_t lowest = INT_MAX, highest = INT_MIN;
    {
        int64_t so = 0;
        for (size_t i = 0; i < s->c_len.size(); ++i) {
            lowest = std::min(lowest, s->c_pos[i]);
            highest = std::max(highest, s->c_pos[i] + path_ref_length(s->c_path.data() + so, s->c_nseg[i]));
            so += s->c_nseg[i];
        }
    }
    for (int r = 0; r < reads->n_reads; ++r) {
        const int nseg = int(reads->path_off[r + 1] - reads->path_off[r]);
        if (nseg == 0) continue;
        const int e = reads->pos[r] + path_ref_length(reads->path + reads->path_off[r], nseg);
        if (s->has_prev && reads->pos[r] < s->next_begin && e > s->region_begin) {
            // (the reference's own guard is validate_new_pos_value, starling_pos_processor_base.cpp:1326: a basecall behind the
            // POST_ALIGN stage throws)
            bool any_match_before = false;
            int ref_head = reads->pos[r];
            for (int64_t i = reads->path_off[r]; i < reads->path_off[r + 1] && !any_match_before; ++i) {
                const uint32_t t = reads->path[i].type;
                if ((seg_match(t) || t == SK_SEG_DELETE) && ref_head < s->next_begin && ref_head >= s->region_begin) any_match_before = true;
                if (seg_ref_len(t)) ref_head += int(reads->path[i].length);
            }
            if (any_match_before) return sk_fail("sk_pileup_stream_push: a read reaches positions that an earlier push declared final");
        }
        lowest = std::min(lowest, reads->pos[r]);
        highest = std::max(highest, e);
    }
    *lowest_out = lowest;
    *highest_out = highest;
    return 0;
}

// the range a push finalises: the not yet final positions below F that the reads (extent lowest..highest) cover
void stream_range(const sk_pileup_stream* s, const int32_t lowest, const int32_t highest, const int32_t F, int32_t* begin_out, int32_t* end_out)
{
    int32_t begin = s->next_begin, end = s->next_begin;
    if (lowest != INT_MAX) {
        begin = std::max(s->region_begin, s->has_prev ? std::max(s->next_begin, lowest) : lowest);
        end = std::max(begin, std::min(F, highest));
    }
    if (begin > F) begin = end = std::max(s->next_begin, std::min(begin, F));
    *begin_out = begin;
    *end_out = end;
}

// ---- the steps of stream_enqueue, in submission order

// the next input block sized and carved (the two device blocks take turns), and its page-locked mirror filled: the carried reads'
// metadata, then the new reads; the window's ploidy; the mask's window
int push_pack_input(sk_pileup_stream* s, const sk_read_batch* reads, const uint8_t* cand_snv_mask, const int32_t ploidy_begin,
                    const int32_t ploidy_len, const uint8_t* ploidy)
{
    Push& p = s->p;
    s->cur_in ^= 1;
    SkDevBuf& d_in = s->d_in2[s->cur_in];
    {
        PushLap lap(g_push_seconds.enq_buffers);
        p.in_bytes = carved_bytes([&](SkArena& ar) { return carve_in(ar, p); });
        if (s->h_in.reserve(p.in_bytes, 2) || d_in.reserve(p.in_bytes, 2)) return sk_fail("sk_pileup_stream_push: out of memory (input block)");
    }
    PushLap lap(g_push_seconds.enq_pack);
    SkArena ar = arena_on(d_in.p);
    p.in = carve_in(ar, p);
    int64_t* ro = s->in_host(p.in.read_off);
    int64_t* po = s->in_host(p.in.path_off);
    sk_path_seg* pa = s->in_host(p.in.path);
    int32_t* ps = s->in_host(p.in.pos);
    uint8_t* fw = s->in_host(p.in.is_fwd);
    uint8_t* mq = s->in_host(p.in.mapq);
    uint8_t* lv = s->in_host(p.in.level);
    const int n_c = p.n_c;
    const int64_t c_segs = int64_t(s->c_path.size()), new_segs = p.n_segs - c_segs, new_bases = p.n_bases - s->c_bases;
    int64_t b = 0, sg = 0;
    for (int i = 0; i < n_c; ++i) {
        ro[i] = b; po[i] = sg;
        b += s->c_len[i]; sg += s->c_nseg[i];
        ps[i] = s->c_pos[i]; fw[i] = 0; mq[i] = s->c_mapq[i]; lv[i] = s->c_level[i]; // (P1 runs over the new reads only: r0)
    }
    if (c_segs) std::memcpy(pa, s->c_path.data(), size_t(8 * c_segs));
    for (int r = 0; r < p.n_new; ++r) {
        ro[n_c + r] = s->c_bases + reads->read_off[r];
        po[n_c + r] = c_segs + reads->path_off[r];
        ps[n_c + r] = reads->pos[r]; fw[n_c + r] = reads->is_fwd[r]; mq[n_c + r] = reads->mapq[r]; lv[n_c + r] = reads->map_level[r];
    }
    ro[p.n] = p.n_bases; po[p.n] = p.n_segs;
    if (new_segs) std::memcpy(pa + c_segs, reads->path, size_t(8 * new_segs));
    if (new_bases) {
        std::memcpy(s->in_host(p.in.code) + s->c_bases, reads->read_code, size_t(new_bases));
        std::memcpy(s->in_host(p.in.qual) + s->c_bases, reads->read_qual, size_t(new_bases));
    }
    uint8_t* pl = s->in_host(p.in.ploidy);
    for (int i = 0; i < p.n_loci; ++i) {
        const int64_t k = int64_t(p.begin) + i - ploidy_begin;
        pl[i] = (ploidy && k >= 0 && k < ploidy_len) ? ploidy[k] : uint8_t(2);
    }
    // (through the pinned block: a copy from the caller's pageable memory would wait for the device)
    if (p.mask_len > 0) std::memcpy(s->in_host(p.in.mask), cand_snv_mask, size_t(p.mask_len));
    return 0;
}

// every device-to-device piece of a push in one launch: with the EVS column on, the carried reads' bases and qualities (`prev`: the
// input block of the push before); the mask's window; and the carried tail of records and spans, which moves to the front of the other
// buffer -- the record / span buffers flip here
int push_carry(sk_pileup_stream* s, const InBlock& prev, const int32_t mask_begin, hipStream_t st)
{
    PushLap lap(g_push_seconds.lap[1]);
    const Push& p = s->p;
    CopyArgs carry;
    carry.n = 0;
    int64_t carry_max = 0;
    auto add_copy = [&](const void* src, void* dst, const int64_t bytes) {
        if (bytes <= 0) return;
        carry.seg[carry.n++] = CopySeg{ static_cast<const char*>(src), static_cast<char*>(dst), bytes };
        carry_max = std::max(carry_max, bytes);
    };
    if (s->want_evs && s->c_bases > 0) { // the EVS words are made in P2 from the reads' bases and qualities
        add_copy(prev.code + s->c_tail_base, p.in.code, s->c_bases);
        add_copy(prev.qual + s->c_tail_base, p.in.qual, s->c_bases);
    }
    if (p.mask_len > 0) add_copy(p.in.mask, s->d_mask.as<char>() + (mask_begin - s->ref_offset), p.mask_len);
    const int nxt = s->cur ^ 1;
    if (s->d_rec[nxt].reserve(size_t(2 * std::max<int64_t>(p.n_bases, 1)), 2) || s->d_span[nxt].reserve(size_t(8 * std::max(p.n, 1)), 2))
        return sk_fail("sk_pileup_stream_push: out of device memory (records)");
    if (s->c_bases > 0) add_copy(s->d_rec[s->cur].as<char>() + 2 * s->c_tail_base, s->d_rec[nxt].p, 2 * s->c_bases);
    if (p.n_c > 0) add_copy(s->d_span[s->cur].as<char>() + 8 * s->c_tail_read, s->d_span[nxt].p, int64_t(8) * p.n_c);
    s->cur = nxt;
    if (carry.n > 0) {
        const int bx = int(std::min<int64_t>((carry_max / 16 + 255) / 256 + 1, 64));
        SK_LAUNCH(copy_segments_kernel, dim3(bx, carry.n), dim3(256), 0, st, carry);
    }
    return 0;
}

// the work block and the output block (the next of the rotation, with its page-locked mirror) sized and carved
int push_carve_blocks(sk_pileup_stream* s)
{
    PushLap lap(g_push_seconds.lap[2]);
    const size_t work_bytes = carved_bytes([&](SkArena& ar) { return carve_work(ar, s); });
    s->p.out_bytes = carved_bytes([&](SkArena& ar) { return carve_out(ar, s); });
    s->out_block = (s->out_block + 1) % (SK_PILEUP_WINDOW_LIFETIME + 1);
    if (s->d_work.reserve(work_bytes, 2) || s->d_out.reserve(s->p.out_bytes, 2) || s->h_out_cur().reserve(s->p.out_bytes, 2))
        return sk_fail("sk_pileup_stream_push: out of memory (work / output blocks)");
    SkArena aw = arena_on(s->d_work.p), ao = arena_on(s->d_out.p);
    s->p.work = carve_work(aw, s);
    s->p.out = carve_out(ao, s);
    return 0;
}

// P1 on the new reads (`a`: its arguments, which P2's start from) and both running bounds of all the reads' spans
int push_read_records(sk_pileup_stream* s, PileupArgs& a, hipStream_t st)
{
    PushLap lap(g_push_seconds.lap[3]);
    const Push& p = s->p;
    std::memset(&a, 0, sizeof(a));
    a.b.n_reads = p.n;
    a.b.read_off = p.in.read_off; a.b.read_code = p.in.code; a.b.read_qual = p.in.qual; a.b.path_off = p.in.path_off; a.b.path = p.in.path;
    a.b.pos = p.in.pos; a.b.is_fwd = p.in.is_fwd; a.b.mapq = p.in.mapq; a.b.map_level = p.in.level;
    a.b.ref_seq = s->d_ref.as<char>(); a.b.ref_offset = s->ref_offset; a.b.ref_len = s->ref_len;
    a.b.cand_snv_mask = s->d_mask.as<uint8_t>();
    a.o = s->opt; // P1: the region's report range, region-wide counters
    a.tab = sk_ctx().dev_tables;
    a.rec = s->d_rec[s->cur].as<uint16_t>(); a.span = s->d_span[s->cur].as<int2>();
    a.spandel = s->d_spandel.as<uint32_t>(); a.submapped = s->d_submapped.as<uint32_t>();
    a.n_loci = s->region_end - s->region_begin;
    a.r0 = p.n_c;
    if (p.n_new > 0) SK_LAUNCH(pileup_read_kernel, dim3((p.n_new + P1_WAVES - 1) / P1_WAVES), dim3(P1_WAVES * WAVE), 0, st, a);
    if (p.n > 0) SK_LAUNCH(span_bounds_kernel, dim3(2), dim3(1024), 0, st, a.span, p.work.maxend, p.work.minbegin, p.n);
    return 0;
}

// The window's columns.  P2's arguments are P1's (`a`), over the window, with the columns where the blocks have them.  P2 counts; one launch
// makes every column's offsets (exclusive sums of n_loci + 1 counts: the last entry is the total) and moves the cleaned columns' sizes, for the
// caller's cache validation, and the region-wide counters' slice into the output block; P2 stores
int push_columns(sk_pileup_stream* s, const PileupArgs& a, hipStream_t st)
{
    PushLap lap(g_push_seconds.lap[4]);
    const Push& p = s->p;
    PileupArgs c = a;
    c.o.report_begin = p.begin; c.o.report_end = p.end; c.n_loci = p.n_loci;
    c.maxend = p.work.maxend; c.minbegin = p.work.minbegin;
    for (int m = 0; m < 3; ++m) c.count3[m] = p.work.count[m];
    c.call_off3[0] = p.out.off0; c.call_off3[1] = p.out.off1; c.call_off3[2] = p.work.off2;
    c.calls3[0] = p.out.calls0; c.calls3[1] = p.out.calls1; c.calls3[2] = p.work.calls2;
    c.mapq_count = p.out.mq_n; c.mapq_zero = p.out.mq_zero; c.mapq_sumsq = p.out.mq_sq;
    const bool som = s->somatic;
    if (som) {
        c.count4 = p.work.count4; c.count4a = p.work.count4a; c.call_off4 = p.work.off4; c.calls4 = p.work.calls4;
        c.read_pos = p.out.read_pos; // (null unless the stream returns read positions)
    }
    if (s->want_evs) { c.evs_off = p.out.evs_off; c.evs_words = p.out.evs; }
    const int n_loci = p.n_loci;
    c.store = 0;
    const int blocks = (n_loci + 1 + WAVE - 1) / WAVE;
    // (a stream's windows are a few thousand loci: the split form; a caller that pushes a whole region at once gets the one-wave form)
    const bool split = blocks < P2_SPLIT_BELOW_BLOCKS;
    const int p2_threads = split ? WAVE * P2_WAVES_MAX : WAVE;
    void (*const p2)(const PileupArgs) =
        split ? (som ? pileup_column_kernel_t<true, true, false> : (s->want_evs ? pileup_column_kernel_t<true, false, true> : pileup_column_kernel_t<true, false, false>))
              : (som ? pileup_column_kernel_t<true, true, false, 1>
                     : (s->want_evs ? pileup_column_kernel_t<true, false, true, 1> : pileup_column_kernel_t<true, false, false, 1>));
    SK_LAUNCH(p2, dim3(blocks), dim3(p2_threads), 0, st, c);
    OffsetsArgs oa;
    std::memset(&oa, 0, sizeof(oa));
    oa.n = n_loci;
    for (int m = 0; m < 3; ++m) {
        oa.count[oa.n_scans] = c.count3[m];
        oa.off[oa.n_scans++] = const_cast<int64_t*>(c.call_off3[m]);
    }
    if (som) {
        oa.count[oa.n_scans] = c.count4;
        oa.off[oa.n_scans++] = const_cast<int64_t*>(c.call_off4);
    }
    if (s->want_evs) { // a locus has mapq_count words
        oa.count[oa.n_scans] = c.mapq_count;
        oa.off[oa.n_scans++] = const_cast<int64_t*>(c.evs_off);
    }
    auto add = [&](const void* src, void* dst, const int64_t bytes) { oa.copy[oa.n_copies++] = CopySeg{ static_cast<const char*>(src), static_cast<char*>(dst), bytes }; };
    add(c.count3[2], p.out.clean_n, 4 * (int64_t(n_loci) + 1));
    if (som) add(c.count4, p.out.clean4_n, 4 * (int64_t(n_loci) + 1));
    if (n_loci > 0) {
        add(s->d_spandel.as<char>() + 4 * size_t(p.begin - s->region_begin), p.out.spandel, 4 * int64_t(n_loci));
        add(s->d_submapped.as<char>() + 4 * size_t(p.begin - s->region_begin), p.out.submapped, 4 * int64_t(n_loci));
    }
    SK_LAUNCH(column_offsets_kernel, dim3(oa.n_scans + oa.n_copies), dim3(1024), 0, st, oa);
    c.store = 1;
    if (p.n > 0 && n_loci > 0) SK_LAUNCH(p2, dim3(blocks), dim3(p2_threads), 0, st, c);
    return 0;
}

// the window's reference base ids, then -- a germline stream -- a9 + a10 on the cleaned column where it is; what the gVCF writer's block
// logic reads of each position, from the same column and the record just written; and, from every plain site, the non-variant block the
// writer would start there
int push_genotypes(sk_pileup_stream* s, hipStream_t st)
{
    PushLap lap(g_push_seconds.lap[5]);
    const Push& p = s->p;
    if (p.n_loci == 0 || !(s->genotype || s->somatic)) return 0;
    SK_LAUNCH(ref_base_id_kernel, dim3((p.n_loci + 255) / 256), dim3(256), 0, st, s->d_ref.as<const char>(), s->ref_offset, s->ref_len, p.begin,
              p.n_loci, p.work.refbase);
    if (!s->genotype) return 0;
    sk_pileup_batch pb;
    std::memset(&pb, 0, sizeof(pb));
    pb.n_loci = p.n_loci;
    pb.call_off = p.work.off2;
    pb.calls = p.work.calls2;
    pb.de = nullptr;
    pb.ref_base = p.work.refbase;
    pb.ploidy = p.in.ploidy;
    if (sk_site_digt_call_fused_dev(&pb, &s->gopt, p.out.geno, p.work.de, 0, p.work.gscr, p.n_bases, st)) return 1;
    if (sk_gvcf_site_summaries_dev(&pb, p.out.geno, p.out.summary, st)) return 1;
    if (s->want_runs && sk_gvcf_plain_runs_dev(p.out.summary, p.work.off2, p.out.off0, p.out.mq_n, &s->gvcf_opt, p.n_loci, p.work.pods, p.out.runs, st))
        return 1;
    return 0;
}

// everything of a push up to and including the copy of its output block to the host, on the context's stream, no wait
int stream_enqueue(sk_pileup_stream* s, const sk_read_batch* reads, const int32_t largest_total_indel_ref_span_per_read,
                   const int32_t mask_begin, const int32_t mask_len, const uint8_t* cand_snv_mask, const int32_t F, const int32_t begin,
                   const int32_t end, const int32_t ploidy_begin, const int32_t ploidy_len, const uint8_t* ploidy)
{
    hipStream_t st = sk_ctx().stream;
    s->opt.largest_total_indel_ref_span_per_read = largest_total_indel_ref_span_per_read;
    const InBlock prev_in = s->p.in; // (the push before: push_carry takes the carried reads' bases from its input block)
    Push& p = s->p;
    p.n_new = reads->n_reads;
    p.n_c = int(s->c_len.size());
    p.n = p.n_c + p.n_new;
    p.n_bases = s->c_bases + (p.n_new ? reads->read_off[p.n_new] : 0);
    p.n_segs = int64_t(s->c_path.size()) + (p.n_new ? reads->path_off[p.n_new] : 0);
    p.n_loci = end - begin;
    p.begin = begin; p.end = end; p.F = F; p.mask_len = mask_len;
    p.n_bases_tier2 = 0;
    for (int i = 0; i < p.n_c; ++i)
        if (s->c_level[i] != SK_MAPLEVEL_TIER1) p.n_bases_tier2 += s->c_len[i];
    for (int r = 0; r < p.n_new; ++r)
        if (reads->map_level[r] != SK_MAPLEVEL_TIER1) p.n_bases_tier2 += reads->read_off[r + 1] - reads->read_off[r];

    if (push_pack_input(s, reads, cand_snv_mask, ploidy_begin, ploidy_len, ploidy)) return 1;
    PushLap submit(g_push_seconds.enq_submit);
    {
        PushLap lap(g_push_seconds.lap[0]);
        SK_HIP(skrt::memcpyAsync(s->d_in2[s->cur_in].p, s->h_in.p, p.in_bytes, hipMemcpyHostToDevice, st));
    }
    if (push_carry(s, prev_in, mask_begin, st)) return 1;
    if (push_carve_blocks(s)) return 1;
    PileupArgs a;
    if (push_read_records(s, a, st)) return 1;
    if (push_columns(s, a, st)) return 1;
    if (push_genotypes(s, st)) return 1;
    PushLap lap(g_push_seconds.lap[6]);
    SK_HIP(skrt::getLastError());
    SK_HIP(skrt::memcpyAsync(s->h_out_cur().p, s->d_out.p, p.out_bytes, hipMemcpyDeviceToHost, st));
    return 0;
}

// after the stream has been waited for: what the next push carries, and the window's pointers
void stream_finish(sk_pileup_stream* s, sk_pileup_window* out)
{
    const Push& p = s->p;
    const int n = p.n;
    const int32_t F = p.F;
    // the reads from the first one that ends past F on
    {
        const int64_t* ro = s->in_host(p.in.read_off);
        const int64_t* po = s->in_host(p.in.path_off);
        const sk_path_seg* pa = s->in_host(p.in.path);
        const int32_t* ps = s->in_host(p.in.pos);
        const uint8_t* mq = s->in_host(p.in.mapq);
        const uint8_t* lv = s->in_host(p.in.level);
        int i0 = n;
        if (F < s->region_end) {
            for (int i = 0; i < n; ++i) {
                const int nseg = int(po[i + 1] - po[i]);
                if (nseg > 0 && ps[i] + path_ref_length(pa + po[i], nseg) > F) {
                    i0 = i;
                    break;
                }
            }
        }
        std::vector<int32_t> nl, ns, np;
        std::vector<uint8_t> nm, nv;
        for (int i = i0; i < n; ++i) {
            nl.push_back(int32_t(ro[i + 1] - ro[i]));
            ns.push_back(int32_t(po[i + 1] - po[i]));
            np.push_back(ps[i]);
            nm.push_back(mq[i]);
            nv.push_back(lv[i]);
        }
        std::vector<sk_path_seg> npath(pa + (i0 < n ? po[i0] : p.n_segs), pa + p.n_segs);
        s->c_tail_base = (i0 < n) ? ro[i0] : p.n_bases;
        s->c_tail_read = i0;
        s->c_bases = p.n_bases - s->c_tail_base;
        s->c_len.swap(nl); s->c_nseg.swap(ns); s->c_pos.swap(np); s->c_mapq.swap(nm); s->c_level.swap(nv); s->c_path.swap(npath);
    }
    s->has_prev = true;
    s->next_begin = std::max(s->next_begin, F);
    s->pushes++;
    s->reads_in += p.n_new;

    out->begin = p.begin; out->end = p.end;
    out->tier1_off = s->out_host(p.out.off0); out->tier1_calls = s->out_host(p.out.calls0);
    out->tier2_off = s->out_host(p.out.off1); out->tier2_calls = s->out_host(p.out.calls1);
    out->spandel_count = s->out_host(p.out.spandel); out->submapped_count = s->out_host(p.out.submapped);
    out->mapq_count = s->out_host(p.out.mq_n); out->mapq_zero_count = s->out_host(p.out.mq_zero);
    out->mapq_sum_square = reinterpret_cast<const uint64_t*>(s->out_host(p.out.mq_sq));
    out->clean_count = s->out_host(p.out.clean_n);
    out->genotype = s->genotype ? s->out_host(p.out.geno) : nullptr;
    out->site_summary = s->genotype ? s->out_host(p.out.summary) : nullptr;
    out->gvcf_runs = (s->genotype && s->want_runs) ? s->out_host(p.out.runs) : nullptr;
    out->evs_off = s->want_evs ? s->out_host(p.out.evs_off) : nullptr;
    out->evs_words = s->want_evs ? reinterpret_cast<const uint64_t*>(s->out_host(p.out.evs)) : nullptr;
}

void stream_drop(sk_pileup_stream* s)
{
    s->d_ref.drop(); s->d_mask.drop(); s->d_spandel.drop(); s->d_submapped.drop();
    s->d_rec[0].drop(); s->d_rec[1].drop(); s->d_span[0].drop(); s->d_span[1].drop();
    s->d_in2[0].drop(); s->d_in2[1].drop(); s->d_work.drop(); s->d_out.drop();
    s->h_in.drop();
    for (SkPinBuf& b : s->h_out_blocks) b.drop();
}

// both samples' windows enqueued and, on the four cleaned columns where they are, a12 + a13.  A failure leaves work in flight and the
// samples' bookkeeping half done: the caller drains and poisons both
int somatic_enqueue(sk_somatic_pileup_stream* p, const sk_read_batch* const reads[2], const int32_t largest_total_indel_ref_span_per_read,
                    const int32_t mask_begin, const int32_t mask_len, const uint8_t* cand_snv_mask, const int32_t F, const int32_t begin,
                    const int32_t end, const int32_t forced_begin, const int32_t forced_len, const uint8_t* is_forced_output,
                    const int is_compute_nonsomatic)
{
    hipStream_t st = sk_ctx().stream;
    for (int i = 0; i < 2; ++i)
        if (stream_enqueue(p->sample[i], reads[i], largest_total_indel_ref_span_per_read, mask_begin, mask_len, cand_snv_mask, F, begin, end, 0, 0, nullptr))
            return 1;
    const int n_loci = end - begin;
    if (!p->genotype || n_loci == 0) return 0;
    if (p->d_call.reserve(carved_bytes([&](SkArena& ar) { return carve_call(ar, n_loci); }), 2) || p->h_forced.reserve(sk_align256(size_t(n_loci)), 2) ||
        p->h_geno.reserve(sizeof(sk_somatic_snv_genotype) * size_t(n_loci), 2))
        return sk_fail("sk_somatic_pileup_stream_push: out of memory (somatic records)");
    uint8_t* hf = p->h_forced.as<uint8_t>();
    for (int i = 0; i < n_loci; ++i) {
        const int64_t k = int64_t(begin) + i - forced_begin;
        hf[i] = (is_forced_output && k >= 0 && k < forced_len) ? is_forced_output[k] : uint8_t(0);
    }
    SkArena ar = arena_on(p->d_call.p);
    const CallBlock d = carve_call(ar, n_loci);
    SK_HIP(skrt::memcpyAsync(d.forced, hf, size_t(n_loci), hipMemcpyHostToDevice, st));
    sk_pileup_batch b[4]; // normal t1, tumor t1, normal t2, tumor t2
    for (int i = 0; i < 2; ++i) {
        const WorkBlock& w = p->sample[i]->p.work;
        std::memset(&b[i], 0, sizeof(sk_pileup_batch));
        b[i].n_loci = n_loci;
        b[i].call_off = w.off2;
        b[i].calls = w.calls2;
        b[i].ref_base = p->sample[0]->p.work.refbase;
        b[2 + i] = b[i];
        b[2 + i].call_off = w.off4;
        b[2 + i].calls = w.calls4;
    }
    if (sk_somatic_snv_call_tiers_dev(&b[0], &b[1], p->tier2 ? &b[2] : nullptr, p->tier2 ? &b[3] : nullptr, &p->sopt, d.forced, is_compute_nonsomatic,
                                      d.geno, d.scratch, st))
        return 1;
    SK_HIP(skrt::memcpyAsync(p->h_geno.p, d.geno, sizeof(sk_somatic_snv_genotype) * size_t(n_loci), hipMemcpyDeviceToHost, st));
    return 0;
}

} // namespace

extern "C" {

sk_pileup_stream* sk_pileup_stream_create(const sk_pileup_options* opt, const sk_germline_options* genotype_opt)
{
    if (!sk_ctx().ready) {
        sk_fail("strelka_amd: sk_init() has not succeeded");
        return nullptr;
    }
    if (!opt) {
        sk_fail("sk_pileup_stream_create: null options");
        return nullptr;
    }
    sk_pileup_stream* s = new sk_pileup_stream();
    s->opt = *opt;
    if (genotype_opt) {
        s->gopt = *genotype_opt;
        s->genotype = true;
    }
    return s;
}

int sk_pileup_stream_set_gvcf_block_options(sk_pileup_stream* s, const sk_gvcf_block_options* opt)
{
    if (!s) return sk_fail("sk_pileup_stream_set_gvcf_block_options: null stream");
    if (s->somatic) return sk_fail("sk_pileup_stream_set_gvcf_block_options: a germline stream's");
    s->want_runs = (opt != nullptr);
    if (opt) s->gvcf_opt = *opt;
    return 0;
}

int sk_pileup_stream_enable_evs_words(sk_pileup_stream* s, const int enable)
{
    if (!s) return sk_fail("sk_pileup_stream_enable_evs_words: null argument");
    if (s->somatic) return sk_fail("sk_pileup_stream_enable_evs_words: a sample of a somatic stream (it returns read positions instead)");
    s->want_evs = (enable != 0);
    return 0;
}

void sk_pileup_stream_destroy(sk_pileup_stream* s)
{
    if (!s) return;
    if (sk_ctx().ready) {
        (void)skrt::setDevice(sk_ctx().device);
        (void)skrt::streamSynchronize(sk_ctx().stream);
    }
    stream_drop(s);
    delete s;
}

int sk_pileup_stream_begin_region(sk_pileup_stream* s, const char* ref_seq, const int32_t ref_offset, const int32_t ref_len,
                                  const int32_t report_begin, const int32_t report_end,
                                  const int32_t largest_total_indel_ref_span_per_read)
{
    SK_REQUIRE_INIT();
    if (!s || (!ref_seq && ref_len > 0)) return sk_fail("sk_pileup_stream_begin_region: null argument");
    if (ref_len < 0 || report_end < report_begin) return sk_fail("sk_pileup_stream_begin_region: bad range");
    if (s->in_flight) return sk_fail("sk_pileup_stream_begin_region: the stream's last push has not been finished");
    SkContext& ctx = sk_ctx();
    SK_HIP(skrt::setDevice(ctx.device));
    hipStream_t st = ctx.stream;
    const size_t n_region = size_t(report_end - report_begin);
    if (s->d_ref.reserve(size_t(ref_len) + 1, 2) || s->d_mask.reserve(size_t(ref_len) + 1, 2) || s->d_spandel.reserve(4 * n_region + 4, 2) ||
        s->d_submapped.reserve(4 * n_region + 4, 2))
        return sk_fail("sk_pileup_stream_begin_region: out of device memory");
    if (ref_len > 0) SK_HIP(skrt::memcpyAsync(s->d_ref.p, ref_seq, size_t(ref_len), hipMemcpyHostToDevice, st));
    SK_HIP(skrt::memsetAsync(s->d_mask.p, 0, size_t(ref_len) + 1, st));
    SK_HIP(skrt::memsetAsync(s->d_spandel.p, 0, 4 * n_region + 4, st));
    SK_HIP(skrt::memsetAsync(s->d_submapped.p, 0, 4 * n_region + 4, st));
    SK_HIP(skrt::streamSynchronize(st)); // ref_seq is the caller's
    s->poisoned = false;
    s->ref_offset = ref_offset;
    s->ref_len = ref_len;
    s->region_begin = report_begin;
    s->region_end = report_end;
    s->opt.report_begin = report_begin;
    s->opt.report_end = report_end;
    s->opt.largest_total_indel_ref_span_per_read = largest_total_indel_ref_span_per_read;
    s->c_len.clear(); s->c_nseg.clear(); s->c_pos.clear(); s->c_mapq.clear(); s->c_level.clear(); s->c_path.clear();
    s->c_bases = 0;
    s->c_tail_base = 0;
    s->c_tail_read = 0;
    s->has_prev = false;
    s->next_begin = report_begin;
    s->has_region = true;
    return 0;
}

// A push in two halves: _begin checks, packs and enqueues everything up to the copy of the window's output block and returns while the
// device works; _finish waits and hands out the window.  A caller with host work between the two (the adapter: the positions POST_ALIGN
// still has to go through before it needs this window) spends the device's ~0.4 ms there instead of asleep.  Between the two the stream
// object takes no other call.
int sk_pileup_stream_push_begin(sk_pileup_stream* s, const sk_read_batch* reads, const int32_t largest_total_indel_ref_span_per_read,
                                const int32_t mask_begin, const int32_t mask_len, const uint8_t* cand_snv_mask, const int32_t final_to,
                                const int32_t ploidy_begin, const int32_t ploidy_len, const uint8_t* ploidy)
{
    SK_REQUIRE_INIT();
    skrt::wakeHint();
    int32_t F, begin, end;
    {
        PushLap lap(g_push_seconds.check);
        if (!s || !reads) return sk_fail("sk_pileup_stream_push: null argument");
        if (s->poisoned) return sk_fail("sk_pileup_stream_push: an earlier push of this stream failed; begin the region again");
        if (s->in_flight) return sk_fail("sk_pileup_stream_push_begin: the stream's last push has not been finished");
        if (stream_check_reads(s, reads, mask_begin, mask_len, cand_snv_mask)) return 1;
        SK_HIP(skrt::setDevice(sk_ctx().device));
        F = std::min(final_to, s->region_end);
        int32_t lowest, highest;
        if (stream_extent(s, reads, &lowest, &highest)) return 1;
        stream_range(s, lowest, highest, F, &begin, &end);
    }
    PushLap lap(g_push_seconds.enqueue);
    // (stream_enqueue flips the record buffers and moves the carried tail as it goes: a failure from here on leaves work in flight and
    // the stream's bookkeeping half done -- the stream is drained and refuses further pushes until begin_region resets it)
    if (stream_enqueue(s, reads, largest_total_indel_ref_span_per_read, mask_begin, mask_len, cand_snv_mask, F, begin, end, ploidy_begin,
                       ploidy_len, ploidy)) {
        (void)skrt::streamSynchronize(sk_ctx().stream);
        s->poisoned = true;
        return 1;
    }
    skrt::kick(); // (a broker client's records start running now, not at the wait)
    s->in_flight = true;
    return 0;
}

int sk_pileup_stream_push_finish(sk_pileup_stream* s, sk_pileup_window* out)
{
    SK_REQUIRE_INIT();
    if (!s || !out) return sk_fail("sk_pileup_stream_push_finish: null argument");
    if (!s->in_flight) return sk_fail("sk_pileup_stream_push_finish: no push of this stream has been begun");
    s->in_flight = false;
    {
        PushLap lap(g_push_seconds.wait);
        if (skrt::streamSynchronize(sk_ctx().stream) != hipSuccess) {
            s->poisoned = true;
            return sk_fail("sk_pileup_stream_push: the device reported an error");
        }
    }
    PushLap lap(g_push_seconds.finish);
    stream_finish(s, out);
    ++g_push_seconds.pushes;
    return 0;
}

int sk_pileup_stream_push(sk_pileup_stream* s, const sk_read_batch* reads, const int32_t largest_total_indel_ref_span_per_read,
                          const int32_t mask_begin, const int32_t mask_len, const uint8_t* cand_snv_mask, const int32_t final_to,
                          const int32_t ploidy_begin, const int32_t ploidy_len, const uint8_t* ploidy, sk_pileup_window* out)
{
    if (!out) return sk_fail("sk_pileup_stream_push: null argument");
    if (sk_pileup_stream_push_begin(s, reads, largest_total_indel_ref_span_per_read, mask_begin, mask_len, cand_snv_mask, final_to, ploidy_begin,
                                    ploidy_len, ploidy))
        return 1;
    return sk_pileup_stream_push_finish(s, out);
}

// ---- the two samples of a somatic run, pushed together and chained into a12+a13 ----------------------------------------------

sk_somatic_pileup_stream* sk_somatic_pileup_stream_create(const sk_pileup_options* opt, const sk_somatic_snv_options* genotype_opt,
                                                          const int with_read_pos)
{
    if (!sk_ctx().ready) {
        sk_fail("strelka_amd: sk_init() has not succeeded");
        return nullptr;
    }
    if (!opt) {
        sk_fail("sk_somatic_pileup_stream_create: null options");
        return nullptr;
    }
    sk_somatic_pileup_stream* p = new sk_somatic_pileup_stream();
    for (int i = 0; i < 2; ++i) {
        p->sample[i] = new sk_pileup_stream();
        p->sample[i]->opt = *opt;
        p->sample[i]->somatic = true;
    }
    p->sample[1]->want_read_pos = (with_read_pos != 0);
    p->tier2 = (opt->use_tier2_evidence != 0);
    if (genotype_opt) {
        p->sopt = *genotype_opt;
        p->genotype = true;
    }
    return p;
}

void sk_somatic_pileup_stream_destroy(sk_somatic_pileup_stream* p)
{
    if (!p) return;
    if (sk_ctx().ready) {
        (void)skrt::setDevice(sk_ctx().device);
        (void)skrt::streamSynchronize(sk_ctx().stream);
    }
    for (int i = 0; i < 2; ++i) {
        stream_drop(p->sample[i]);
        delete p->sample[i];
    }
    p->d_call.drop();
    p->h_forced.drop();
    p->h_geno.drop();
    delete p;
}

int sk_somatic_pileup_stream_begin_region(sk_somatic_pileup_stream* p, const char* ref_seq, const int32_t ref_offset, const int32_t ref_len,
                                          const int32_t report_begin, const int32_t report_end,
                                          const int32_t largest_total_indel_ref_span_per_read)
{
    if (!p) return sk_fail("sk_somatic_pileup_stream_begin_region: null argument");
    for (int i = 0; i < 2; ++i) {
        if (sk_pileup_stream_begin_region(p->sample[i], ref_seq, ref_offset, ref_len, report_begin, report_end, largest_total_indel_ref_span_per_read))
            return 1;
    }
    return 0;
}

int sk_somatic_pileup_stream_push_begin(sk_somatic_pileup_stream* p, const sk_read_batch* normal_reads, const sk_read_batch* tumor_reads,
                                        const int32_t largest_total_indel_ref_span_per_read, const int32_t mask_begin, const int32_t mask_len,
                                        const uint8_t* cand_snv_mask, const int32_t final_to, const int32_t forced_begin, const int32_t forced_len,
                                        const uint8_t* is_forced_output, const int is_compute_nonsomatic)
{
    SK_REQUIRE_INIT();
    skrt::wakeHint();
    if (!p || !normal_reads || !tumor_reads) return sk_fail("sk_somatic_pileup_stream_push: null argument");
    if (p->in_flight) return sk_fail("sk_somatic_pileup_stream_push_begin: the stream's last push has not been finished");
    const sk_read_batch* const reads[2] = { normal_reads, tumor_reads };
    for (int i = 0; i < 2; ++i) {
        if (p->sample[i]->poisoned) return sk_fail("sk_somatic_pileup_stream_push: an earlier push of this stream failed; begin the region again");
        if (stream_check_reads(p->sample[i], reads[i], mask_begin, mask_len, cand_snv_mask)) return 1;
    }
    if (forced_len < 0 || (forced_len > 0 && !is_forced_output)) return sk_fail("sk_somatic_pileup_stream_push: bad forced-output window");
    SK_HIP(skrt::setDevice(sk_ctx().device));
    const int32_t F = std::min(final_to, p->sample[0]->region_end);
    // one range for both samples: the positions either sample's reads cover
    int32_t lowest = INT_MAX, highest = INT_MIN, begin, end;
    for (int i = 0; i < 2; ++i) {
        int32_t lo, hi;
        if (stream_extent(p->sample[i], reads[i], &lo, &hi)) return 1;
        lowest = std::min(lowest, lo);
        highest = std::max(highest, hi);
    }
    stream_range(p->sample[0], lowest, highest, F, &begin, &end);
    // (from the first sample's enqueue on, a failure -- of either sample's push or of the somatic chain -- has one way out: the stream is
    // drained and both samples refuse pushes until begin_region)
    if (somatic_enqueue(p, reads, largest_total_indel_ref_span_per_read, mask_begin, mask_len, cand_snv_mask, F, begin, end, forced_begin, forced_len,
                        is_forced_output, is_compute_nonsomatic)) {
        (void)skrt::streamSynchronize(sk_ctx().stream);
        p->sample[0]->poisoned = p->sample[1]->poisoned = true;
        return 1;
    }
    skrt::kick(); // (a broker client's records start running now, not at the wait)
    p->in_flight = true;
    p->p_loci = end - begin;
    return 0;
}

int sk_somatic_pileup_stream_push_finish(sk_somatic_pileup_stream* p, sk_somatic_pileup_window* out)
{
    SK_REQUIRE_INIT();
    if (!p || !out) return sk_fail("sk_somatic_pileup_stream_push_finish: null argument");
    if (!p->in_flight) return sk_fail("sk_somatic_pileup_stream_push_finish: no push of this stream has been begun");
    p->in_flight = false;
    sk_pileup_stream* sn = p->sample[0];
    sk_pileup_stream* stu = p->sample[1];
    const int n_loci = p->p_loci;
    if (skrt::streamSynchronize(sk_ctx().stream) != hipSuccess) {
        sn->poisoned = stu->poisoned = true;
        return sk_fail("sk_somatic_pileup_stream_push: the device reported an error");
    }
    stream_finish(sn, &out->normal);
    stream_finish(stu, &out->tumor);
    out->tumor_tier1_read_pos = stu->want_read_pos ? stu->out_host(stu->p.out.read_pos) : nullptr;
    out->normal_clean_tier2_count = sn->out_host(sn->p.out.clean4_n);
    out->tumor_clean_tier2_count = stu->out_host(stu->p.out.clean4_n);
    out->genotype = (p->genotype && n_loci > 0) ? p->h_geno.as<const sk_somatic_snv_genotype>() : nullptr;
    return 0;
}

int sk_somatic_pileup_stream_push(sk_somatic_pileup_stream* p, const sk_read_batch* normal_reads, const sk_read_batch* tumor_reads,
                                  const int32_t largest_total_indel_ref_span_per_read, const int32_t mask_begin, const int32_t mask_len,
                                  const uint8_t* cand_snv_mask, const int32_t final_to, const int32_t forced_begin, const int32_t forced_len,
                                  const uint8_t* is_forced_output, const int is_compute_nonsomatic, sk_somatic_pileup_window* out)
{
    if (!out) return sk_fail("sk_somatic_pileup_stream_push: null argument");
    if (sk_somatic_pileup_stream_push_begin(p, normal_reads, tumor_reads, largest_total_indel_ref_span_per_read, mask_begin, mask_len, cand_snv_mask,
                                            final_to, forced_begin, forced_len, is_forced_output, is_compute_nonsomatic))
        return 1;
    return sk_somatic_pileup_stream_push_finish(p, out);
}

} // extern "C"
