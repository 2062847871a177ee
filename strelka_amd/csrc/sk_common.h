// sk_common.h -- internal declarations shared by the HIP translation units of libstrelka_amd.so (gfx950 only).
#pragma once

#include "strelka_amd.h"

#include "sk_rt.h"

#include <atomic>
#include <cstdint>
#include <cstring>
#include <string>

void sk_set_error(const std::string& msg);
int sk_fail(const std::string& msg);

#define SK_HIP(expr)                                                                                          \
    do {                                                                                                      \
        hipError_t _e = (expr);                                                                               \
        if (_e != hipSuccess) return sk_fail(std::string(#expr) + ": " + skrt::errorString(_e));              \
    } while (0)

// ---------------------------------------------------------------------------------------------------------------------
// The library's one grow-on-demand block of device (or page-locked host) memory.  State that outlives a call lives in named members of
// this type and is dropped by its module's reset function at sk_shutdown (below); a host-buffer entry point's per-call arrays come from
// the context arena (SkArena).  Nothing is freed at process exit: the runtime may be gone by then.
// ---------------------------------------------------------------------------------------------------------------------
extern std::atomic<int64_t> sk_grown_bytes[2]; // what the process's SkBufs hold: [0] device, [1] page-locked (sk_debug_grown_bytes)

template <bool PINNED>
struct SkBuf
{
    void* p = nullptr;
    size_t cap = 0;
    /// room for `bytes`; a block that grows is not copied, and grows to bytes + bytes / 4 + 4096 (a pileup stream asks for half: headroom_div 2)
    int reserve(const size_t bytes, const size_t headroom_div = 4)
    {
        if (bytes <= cap) return 0;
        drop();
        const size_t want = bytes + bytes / headroom_div + 4096;
        SK_HIP(PINNED ? skrt::hostMalloc(&p, want) : skrt::malloc_(&p, want));
        cap = want;
        sk_grown_bytes[PINNED] += int64_t(want);
        return 0;
    }
    void drop()
    {
        if (p) (void)(PINNED ? skrt::hostFree(p) : skrt::free_(p));
        sk_grown_bytes[PINNED] -= int64_t(cap);
        p = nullptr;
        cap = 0;
    }
    template <typename T> T* as() const { return static_cast<T*>(p); }
};
using SkDevBuf = SkBuf<false>;
using SkPinBuf = SkBuf<true>;

// what sk_shutdown calls, one per module with state that outlives a call: each drops its buffers and clears what points into them
void sk_enum_reset();         // read_enumerate.hip: the job's buffers; the last run's candidate alignments and scores are forgotten
void sk_feed_reset();         // bam_feed.hip: the feed's buffers and its kept stream
void sk_deflate_reset();      // bgzf_deflate.hip: slots, tokens, slot lengths
void sk_score_extra_reset();  // score_alignments.hip: the legacy batch's extra block
void sk_stage_reset();        // sk_context.hip: SkStage's page-locked mirrors

// ---------------------------------------------------------------------------------------------------------------------
// Device-resident tables.  Every value is computed ON THE HOST with the host libm, using the reference's own
// expressions (file:line on each builder in sk_context.hip), then uploaded: the kernels never evaluate a
// transcendental for a quantity the reference takes from a table or memoises, so those terms are bit-identical.
// ---------------------------------------------------------------------------------------------------------------------
enum { SK_NQ = 71, SK_NQ6 = 64, SK_HET_RES = 9 };

struct SkTables
{
    // hot path A (double): L/blt_util/qscore_cache.cpp:34-50, L/starling_common/starling_read_align_score.cpp:119,133-135
    double q2lncompe[SK_NQ + 1]; // ln(1-e_q)
    double q2mis[SK_NQ + 1];     // ln(e_q) + (-ln 3)
    double ln_quarter;           // std::log(0.25)            (:453)
    double ln_noncand;           // std::log(1e-5)            (:483)

    // hot path B germline (float): L/blt_common/position_snp_call_pprob_digt.cpp:43-46,345-354
    float g_eprob[SK_NQ6];  // (float) error_prob(q)          (adjust_joint_eprob.cpp:210)
    float g_v1[SK_NQ6];     // (float)(log(ce+(1.-ce)/3)+ln 1/2)
    float g_v2[SK_NQ6];     // (float) ln_comp_error_prob(q)
    float g_weight[SK_NQ6]; // (float)(ln0.75 - ln_error_prob(q))  (adjust_joint_eprob.cpp:116,123)
    float g_log_one_third;

    // hot path B somatic (float): L/applications/strelka/position_somatic_snv_strand_grid_lhood_cached.cpp
    float s_v0[SK_NQ6], s_v1[SK_NQ6], s_v2[SK_NQ6];           // :56-64
    float s_c0[SK_HET_RES][SK_NQ6], s_c1[SK_HET_RES][SK_NQ6]; // :104-110  (het grid)
    float t_c0[SK_HET_RES][SK_NQ6], t_c1[SK_HET_RES][SK_NQ6]; // :197-206  (strand states, on-strand)
    float t_off_ref[SK_NQ6];                                  // (float) ln_comp_error_prob(q)            (:213)
    float t_off_alt[SK_NQ6];                                  // (float)(ln_error_prob(q) + ln_one_third) (:221)
    float s_ln_one_half;

    // a8: qphred_cache::mappedq[mapq 0..90][q 0..70] (qscore_cache.cpp:46-49, qscore.hh:104-113)
    uint8_t mappedq[91][SK_NQ + 1];
};

struct SkContext
{
    int device = -1;
    bool ready = false;
    bool libm_restated = false; // the host libm's powf/logf match csrc/libm_flt32.h (checked at sk_init)
    bool blocking_sync = false; // hipDeviceScheduleBlockingSync took effect on this process's device (sk_sync_mode)
    SkTables host_tables;
    SkTables* dev_tables = nullptr;
    hipStream_t stream = nullptr; // used by the host-buffer entry points
    SkDevBuf arena;               // staging arena for the host-buffer entry points (grown on demand, never shrunk; dropped by sk_shutdown)
    // sticky error bits raised by kernels on input the reference would have thrown on (sk_check_device_errors)
    unsigned* dev_error_flags = nullptr;
    // per-kernel attributes raised on this context's device (cleared with the context: another device starts from the defaults)
    size_t global_align_lds_allowed = 0;
    bool inflate_scalar_lds_allowed = false;
};
enum {
    SK_DEVERR_QSCORE = 1u, // a basecall quality above 70 reached a scoring kernel (qscore_cache.cpp:53-75 throws)
    SK_DEVERR_INTAKE = 2u, // sk_read_intake_dev met a read or path its host entry refuses, or ran out of obs_cap
    SK_DEVERR_ACTIVE_REGION = 4u, // sk_active_regions_dev: createActiveRegion's assertion failed; sk_ref_anchors_dev: a span_pos before m
    SK_DEVERR_HAPLOTYPES = 8u, // sk_region_haplotypes_dev met a read or a region its host entry refuses, or ran out of a pool
    SK_DEVERR_ALLELES = 16u, // sk_region_alleles_dev met a haplotype record its host entry refuses, or a capacity below its bound
    SK_DEVERR_SYNC_REGIONS = 32u, // sk_sync_active_regions_dev: createActiveRegion's or closeActiveRegion's assertion failed, or marks its host entry refuses
    SK_DEVERR_INDEL_TABLE = 64u, // sk_indel_table_dev met input its host entry refuses, or a capacity below what the arrays hold
    SK_DEVERR_READ_DEPTH = 128u, // sk_read_depth_dev met an iat above 2 or a path outside path_cap or with a segment type it does not know
    SK_DEVERR_INDEL_CANDIDATES = 256u, // sk_indel_candidates_dev met a rate set, a key count or observations its host entry refuses
    SK_DEVERR_REALIGN_GATE = 512u, // sk_realign_gate_dev met reads, a table or capacities its host entry refuses
    SK_DEVERR_REALIGN_PREAMBLE = 1024u // sk_realign_preamble_dev met reads, gate outputs, keys or a record capacity its host entry refuses
};

SkContext& sk_ctx();
// what sk_read_intake refuses of a read's path (read_intake.hip; nullptr: addAlignmentIndelsToPosProcessor takes it)
const char* sk_intake_path_issue(const sk_path_seg* path, int n_seg, int64_t read_len);
// D1 over problems whose count lies in device memory (global_align.hip): what a device chain launches; only enqueues
size_t sk_ga_ptr_bytes(int64_t grid, int max_query_len, int max_ref_len);
int sk_ga_launch_counted(const sk_global_align_batch& dev_batch, const int32_t* dev_n, int64_t grid, int max_query_len, int max_ref_len, const sk_align_scores& sc,
                         int32_t* dev_out_score, int32_t* dev_out_begin_pos, sk_path_seg* dev_out_path, int32_t* dev_out_n_seg, sk_path_seg* dev_tmp_path,
                         uint8_t* dev_ptr_scratch, hipStream_t st);
#define SK_REQUIRE_INIT()                                                                    \
    do {                                                                                     \
        if (!sk_ctx().ready) return sk_fail("strelka_amd: sk_init() has not succeeded");     \
    } while (0)

// simple bump allocator over the context arena (host-buffer entry points)
struct SkArena
{
    char* base = nullptr;
    size_t cap = 0, used = 0;
    int reserve(size_t bytes);
    template <typename T> T* take(size_t n)
    {
        size_t off = (used + 255) & ~size_t(255);
        used = off + n * sizeof(T);
        return base ? reinterpret_cast<T*>(base + off) : nullptr; // (no base: a dry arena, which only counts -- sk_carve)
    }
    /// take<T>(n + slack_elems) with the first n elements on their way up from `src`; a failed copy leaves its error in rc
    template <typename T> T* up(const T* src, const size_t n, const size_t slack_elems, hipStream_t st, int& rc)
    {
        T* d = take<T>(n + slack_elems);
        if (!d || n == 0 || rc) return d;
        const hipError_t e = skrt::memcpyAsync(d, src, n * sizeof(T), hipMemcpyHostToDevice, st);
        if (e != hipSuccess) rc = sk_fail(std::string("memcpyAsync (host to arena): ") + skrt::errorString(e));
        return d;
    }
};

// An entry point states each of its device arrays once, in a function `carve(SkArena&)` that takes or ups them and returns a struct of
// typed device pointers: run on a dry arena to learn the room, then, with that much reserved, for real.  The caller holds the arena until
// it returns and calls nothing that reserves it again.
template <typename P, typename F> int sk_carve(P& out, F&& carve)
{
    SkArena ar;
    (void)carve(ar);
    if (ar.reserve(ar.used)) return 1;
    out = carve(ar);
    return 0;
}

static inline size_t sk_align256(size_t n) { return (n + 255) & ~size_t(255); }

// The small host-buffer entry points (one indel group, one haplotype, a few loci per call: the adapter's per-unit sites) move their
// arrays as ONE page-locked block in and ONE out, carried by two launches in the process's own queue.  A copy call per array from the
// caller's pageable memory is a synchronous staged copy each (~10 us, ten of them per call), and with several caller processes on a
// device every copy call queues behind the others' (profiles/r05_enum_job_history.txt: the realignment job's way in and out).
//   SkStage st; st.begin(in_bytes, out_bytes);  T* d = st.put(host_array, n); ... U* dout = st.out<U>(n);
//   st.upload(stream); <launch kernels on d..., dout>; st.download_and_wait(stream); st.fetch(host_dst, dout, n);
struct SkStage
{
    SkArena ar;                 // device side: [in block | out block | whatever the caller takes after begin()]
    char* h_in = nullptr;       // page-locked mirrors (the context's, grown on demand)
    char* h_out = nullptr;
    size_t in_cap = 0, out_cap = 0, in_used = 0, out_used = 0;
    char* d_in = nullptr;
    char* d_out = nullptr;
    hipStream_t in_flight = nullptr; // the stream of an upload() that no download_and_wait() has followed yet
    /// An entry point that fails between upload() and download_and_wait() leaves kernels running over the page-locked mirrors, which
    /// the next call refills or frees: the stage waits for them before it goes.
    ~SkStage()
    {
        if (in_flight) (void)skrt::streamSynchronize(in_flight);
    }
    /// room for `in_bytes` of inputs and `out_bytes` of outputs (sums of the arrays' sizes; alignment padding is added here) plus
    /// `extra_bytes` of device scratch the caller takes from `ar` afterwards
    int begin(size_t in_bytes, size_t out_bytes, size_t extra_bytes, int n_arrays);
    template <typename T> T* put(const T* src, const size_t n)
    {
        const size_t off = (in_used + 255) & ~size_t(255);
        in_used = off + n * sizeof(T);
        if (n && in_used <= in_cap) std::memcpy(h_in + off, src, n * sizeof(T)); // (past the room asked for: upload() reports it)
        return reinterpret_cast<T*>(d_in + off);
    }
    template <typename T> T* out(const size_t n)
    {
        const size_t off = (out_used + 255) & ~size_t(255);
        out_used = off + n * sizeof(T);
        return reinterpret_cast<T*>(d_out + off);
    }
    int upload(hipStream_t st);            // in block: page-locked mirror -> device (one launch)
    int download_and_wait(hipStream_t st); // out block: device -> page-locked mirror (one launch), then the wait
    template <typename T> void fetch(T* dst, const T* dev, const size_t n) const
    {
        if (n) std::memcpy(dst, h_out + (reinterpret_cast<const char*>(dev) - d_out), n * sizeof(T));
    }
};

// packed base_call accessors (device + host)
#define SKC_Q(c) ((unsigned)((c) & 0x3f))
#define SKC_BASE(c) ((unsigned)(((c) >> 6) & 0xf))
#define SKC_FWD(c) ((unsigned)(((c) >> 10) & 1))
#define SKC_NMM(c) ((unsigned)(((c) >> 11) & 1))
#define SKC_FILTER(c) ((unsigned)(((c) >> 12) & 1))
