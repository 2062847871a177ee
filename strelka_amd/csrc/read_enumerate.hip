// read_enumerate.hip -- candidate-alignment enumeration, flattening and scoring of a realignment job on the device
// (sk_realign_options.enumeration == 2).
//
//   E1  root_kernel, level_kernel x depth   candidate_alignment_search (csrc/realign_core.h, the statement of
//                          L/starling_common/starling_read_align.cpp:857-1277 shared with the host), level by level: one thread
//                          per call of the reference's recursion, all reads of the job at once
//   E2  group/dedupe/rank  the leaves of each read -> its std::set<CandidateAlignment>: duplicates dropped, set order
//   L1  pool_bounds/layout  reference window and insert sequences of each read's haplotype pool
//   L2  op_count_kernel    one thread per candidate alignment: ops it flattens to
//   F1  pool_fill_kernel   one wave per read: the pool's bytes
//   F2  flatten_kernel     one thread per candidate alignment: the walk of scoreCandidateAlignment
//                          (starling_read_align_score.cpp:286-493) emitting scoring ops (host/align_flatten.cpp holds the host form)
//   F3  entries_kernel     one thread per candidate alignment: the transition entries and event masks kernel A1 reads
//                          (csrc/align_entry.h) -- so neither sk_align_builder nor sk_align_prepare runs on the host for these reads
//   A1  score_wave_per_read (score_alignments.hip) on the batch E3 left in HBM
//
// This file is the host side -- buffers, the process state, the C entry points, the job driver, the rescore entry --; the kernels are
// in sections of this one translation unit, included below in the order of the device object:
//   enum_search.h   E1, E2, the counter slots, the block scan, the job's staging and scan kernels
//   enum_flatten.h  FlatArgs, code_of, L1, flatten_cal, L2, F1, F2
//   enum_f5.h       F5 (flatten_score_kernel: flattening and scoring in one kernel), its grid and launchers, $SK_F5_TIMING's report
//   enum_f5_tail.h  tail_order_kernel: the order of F5's last hand-outs
//   enum_entries.h  gather_cals_kernel, F3
//   enum_stage3.h   S3: stage 3's kernel wrapper
//
// All of this is integer/byte work; it has to reproduce the host stages exactly (tests/test_device_enumeration.py).  A read that
// exceeds a capacity of the core, or that the host code would have thrown on, is reported (status != ST_OK) and redone by the
// container-based host code, which then produces either the result or the reference's error text -- nothing is truncated.

#include "sk_common.h"

#include "align_entry.h"
#include "read_enumerate.h"

#include "enum_search.h"
#include "enum_flatten.h"
#include "enum_f5.h"
#include "enum_f5_tail.h"
#include "enum_entries.h"
#include "enum_stage3.h"

#include <algorithm>
#include <chrono>
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <type_traits>

using namespace skcore;

int sk_score_alignments_launch_hostleg(const sk_align_batch* b, double* dev_out_lnp, void* hip_stream); // score_alignments.hip

namespace
{

// the switches of the environment: set at all / set to this value.  Read where they are asked for: a switch that holds for the process
// is kept in a static by its reader, one that tests flip between jobs ($SK_A5_FUSED, $SK_ENUM_ONE_WAIT, $SK_F3_KERNEL) is read per job
bool env_set(const char* name) { return std::getenv(name) != nullptr; }
bool env_is(const char* name, const char* value)
{
    const char* const e = std::getenv(name);
    return e != nullptr && std::strcmp(e, value) == 0;
}

// ---------------------------------------------------------------------------------------------------------------------
// buffers: grown on demand, kept for the life of the process (one job after the other reuses them)

struct View // a piece of one of the arenas below
{
    void* p = nullptr;
    template <typename T> T* as() const { return static_cast<T*>(p); }
};

// The job's small arrays live in a few arenas so that a job is a handful of copies and fills, not dozens (each one costs 4-5 us on
// the stream whatever its size): everything that goes up before the search in `in_arena` (packed in a pinned mirror, one copy), every
// array that starts at zero in `zero_arena` (one fill; the parts the host reads come back in one copy per synchronisation point)
struct EnumBuffers
{
    SkDevBuf in_arena, zero_arena, minmax_arena, mask_arena;
    SkPinBuf h_in_arena, h_zero_arena;
    View tab, ins, toggle, ref, ref_code, ins_code, reads, read_off, read_code, read_qual, r2i, i2r, orig, map_level;
    View counters, status, warn, n_raw, hap_len, fill, n_uniq, consulted;
    View win_begin, ins_lo, win_end, ins_hi, evmask, addmask;
    View h_counters, h_status, h_warn, h_n_raw, h_hap_len, h_n_uniq, h_consulted;
    View cal_off_z, h_cal_off_z;
    SkDevBuf level_a, level_b, pool, leaf_read, leaf_hash;
    SkDevBuf raw_off, grouped, ghash, gkey, dup, sorted;
    SkDevBuf n_ops, win_len, n_ins, ins_idx, ins_off, n_seg8;
    SkDevBuf cal_off, hap_off, cals, hap_code, op_off, ops, entries, scores, colmat, colmat_off;
    SkDevBuf s3_order, s3_smooth, s3_flag, s3_rm_type, s3_rm_pos, s3_key, s3_sorted_score, s3_sorted_hash, s3_next_same, s3_range_end, s3_removed, s3_out, s3_list;
    SkDevBuf tail_order; // F5's last hand-outs (tail_order_kernel)
    SkPinBuf h_s3_out, h_s3_list;
    SkPinBuf h_raw_off, h_n_ops, h_cal_off, h_hap_off, h_op_off, h_cals, h_scores, h_colmat_off;
    void drop() // every block above, then the views into them
    {
        for (SkDevBuf* b : { &in_arena, &zero_arena, &minmax_arena, &mask_arena, &level_a, &level_b, &pool, &leaf_read, &leaf_hash, &raw_off, &grouped, &ghash,
                             &gkey, &dup, &sorted, &n_ops, &win_len, &n_ins, &ins_idx, &ins_off, &n_seg8, &cal_off, &hap_off, &cals, &hap_code, &op_off, &ops,
                             &entries, &scores, &colmat, &colmat_off, &s3_order, &s3_smooth, &s3_flag, &s3_rm_type, &s3_rm_pos, &s3_key, &s3_sorted_score,
                             &s3_sorted_hash, &s3_next_same, &s3_range_end, &s3_removed, &s3_out, &s3_list, &tail_order })
            b->drop();
        for (SkPinBuf* b : { &h_in_arena, &h_zero_arena, &h_s3_out, &h_s3_list, &h_raw_off, &h_n_ops, &h_cal_off, &h_hap_off, &h_op_off, &h_cals, &h_scores,
                             &h_colmat_off })
            b->drop();
        *this = EnumBuffers();
    }
};
EnumBuffers& bufs()
{
    static EnumBuffers b;
    return b;
}

// a job's reservations, as tables: a device buffer holds at least 256 bytes (an empty array still has an address), a pinned one 64 bytes
// more than asked for (job_stage_out_kernel writes whole 16-byte words)
int reserve_dev(std::initializer_list<std::pair<SkDevBuf&, size_t>> wants) // { buffer, bytes }, ...
{
    for (const auto& w : wants)
        if (w.first.reserve(std::max<size_t>(w.second, 256))) return 1;
    return 0;
}
int reserve_pinned(std::initializer_list<std::pair<SkPinBuf&, size_t>> wants)
{
    for (const auto& w : wants)
        if (w.first.reserve(w.second + 64)) return 1;
    return 0;
}
// copies on the job's stream; nothing is submitted for zero bytes
int copy_up(hipStream_t st, const SkDevBuf& dst, const void* src, const size_t bytes)
{
    if (bytes > 0) SK_HIP(skrt::memcpyAsync(dst.p, src, bytes, hipMemcpyHostToDevice, st));
    return 0;
}
int copy_down(hipStream_t st, const SkPinBuf& dst, const SkDevBuf& src, const size_t bytes)
{
    if (bytes > 0) SK_HIP(skrt::memcpyAsync(dst.p, src.p, bytes, hipMemcpyDeviceToHost, st));
    return 0;
}

} // namespace

extern "C" int sk_enum_device_available(void) { return sk_ctx().ready ? 1 : 0; } // (host stages alone run without a device)

namespace
{
// what sk_enum_device_rescore needs to run F1-F3 + the scoring kernel again on the candidate alignments of the last run
struct LastFlat
{
    bool valid = false;
    bool fused = false; // the last run scored with F5 (fs), else with the staged chain (fa, d)
    FusedScoreArgs fs;
    FlatArgs fa;
    sk_align_batch d;
    int32_t n = 0, n_cals = 0;
    int64_t cells = 0;
    size_t mask_bytes = 0, colmat_bytes = 0;
    double* scores = nullptr;
};

// the state of the process, in one place: the generation, what the last run left on the device, and the process's statistics
struct EnumState
{
    uint64_t generation = 0; // of the run whose candidate alignments the buffers hold
    // ---- what the last run left on the device (forget_run)
    int32_t n_cals = 0;
    bool cals_gathered = false; // bufs().cals holds the run's records in set order (else: pool + list, gathered when the host asks)
    const PCal* cals_pool = nullptr;
    const int32_t* cals_list = nullptr;
    const double* scores = nullptr; // the run's scores, where the scoring kernel left them
    LastFlat last;
    // ---- statistics of the process: jobs run as one fixed sequence (one wait), and those of them the host ran again the staged way because
    // an assumption of the sequence did not hold (deeper levels than launched, a full leaf pool, a read outside F5's form)
    int64_t jobs_one_wait = 0, jobs_one_wait_redone = 0, jobs_staged = 0;
    int64_t tail_launches = 0; // launches of tail_order_kernel by the job drivers (sk_debug_f5_tail_launches)
    int64_t late_turn_downs = 0; // F5's rounds after a read's first that left the read to the staged chain, over the drivers' F5 launches
    int64_t shared_rounds = 0; // F5's rounds scored by a wave other than their read's owner, over the drivers' jobs (sk_debug_f5_shared_rounds)

    // a new job starts, or the buffers go: nothing of the last run is served any more.  The generation and the statistics stay
    void forget_run()
    {
        n_cals = 0;
        cals_gathered = false;
        cals_pool = nullptr;
        cals_list = nullptr;
        scores = nullptr;
        last.valid = false;
    }
};
static_assert(std::is_trivially_destructible<EnumState>::value, "JobSeconds reads the statistics at exit, after the statics of functions are gone");
EnumState& state()
{
    static EnumState s;
    return s;
}
} // namespace

// (the generation counter stays: a caller that kept a generation from before sk_shutdown is refused, not served from another run's memory)
void sk_enum_reset()
{
    bufs().drop();
    state().forget_run();
}

extern "C" uint64_t sk_enum_device_generation(void) { return state().generation; }

extern "C" int sk_enum_device_fetch_scores(const uint64_t generation, const int32_t first, const int32_t count, double* dst)
{
    const EnumState& S = state();
    if (generation != S.generation || first < 0 || count < 0 || first + count > S.n_cals || !S.scores) return 1;
    if (count == 0) return 0;
    SkContext& ctx = sk_ctx();
    SK_HIP(skrt::setDevice(ctx.device));
    SK_HIP(skrt::memcpyAsync(dst, S.scores + first, 8 * size_t(count), hipMemcpyDeviceToHost, ctx.stream));
    SK_HIP(skrt::streamSynchronize(ctx.stream));
    return 0;
}

extern "C" int sk_enum_device_fetch_cals(const uint64_t generation, const int32_t first, const int32_t count, PCal* dst)
{
    EnumState& S = state();
    if (generation != S.generation || first < 0 || count < 0 || first + count > S.n_cals) return 1;
    if (count == 0) return 0;
    SkContext& ctx = sk_ctx();
    SK_HIP(skrt::setDevice(ctx.device));
    if (!S.cals_gathered) { // (F5 left the records where the search put them: in set order on demand, once per run)
        if (bufs().cals.reserve(sizeof(PCal) * size_t(S.n_cals))) return 1;
        SK_LAUNCH(gather_cals_kernel, dim3((S.n_cals + 63) / 64), dim3(64), 0, ctx.stream, S.cals_pool, S.cals_list, S.n_cals, bufs().cals.as<PCal>());
        SK_HIP(skrt::getLastError());
        S.cals_gathered = true;
    }
    SK_HIP(skrt::memcpyAsync(dst, bufs().cals.as<PCal>() + first, sizeof(PCal) * size_t(count), hipMemcpyDeviceToHost, ctx.stream));
    SK_HIP(skrt::streamSynchronize(ctx.stream));
    return 0;
}

namespace
{
// diagnostics ($SK_ENUM_JOB_SECONDS): where a one-sequence job's wall time goes -- buffers + packing, submissions, the wait -- on stderr at exit
struct JobSeconds
{
    double setup = 0, submit = 0, wait = 0, after = 0;
    ~JobSeconds()
    {
        if (env_set("SK_ENUM_JOB_SECONDS"))
            std::fprintf(stderr, "strelka_amd enum job seconds: jobs=%lld setup=%.4f submit=%.4f wait=%.4f after=%.4f\n", (long long)state().jobs_one_wait, setup,
                         submit, wait, after);
    }
} g_job_seconds;
}
extern "C" void sk_enum_device_job_counts(int64_t* one_wait, int64_t* one_wait_redone, int64_t* staged)
{
    const EnumState& S = state();
    if (one_wait) *one_wait = S.jobs_one_wait;
    if (one_wait_redone) *one_wait_redone = S.jobs_one_wait_redone;
    if (staged) *staged = S.jobs_staged;
}

// test hooks (include/strelka_amd.h): the table kernel over a host-given cal_off with the grid's waves and the shift given, in buffers of
// its own (the last job's stay as they are); and how often the job drivers launched it
extern "C" int sk_debug_f5_tail_order(const int32_t* cal_off, const int32_t n_reads, const int32_t waves, const int32_t shift, int32_t* first, int32_t* n,
                                      int32_t* order_out)
{
    SK_REQUIRE_INIT();
    if (!cal_off || n_reads < 0 || waves <= 0 || !first || !n) return sk_fail("sk_debug_f5_tail_order: bad argument");
    const int T = f5_tail_window(n_reads, waves, shift);
    *first = T ? n_reads - T : 0;
    *n = T;
    if (T == 0) return 0; // (no launch: what the drivers do for such a job)
    if (T > F5_TAIL_MAX) return sk_fail("sk_debug_f5_tail_order: a window of more than 65536 hand-outs (the drivers cut the shift down)");
    if (!order_out) return sk_fail("sk_debug_f5_tail_order: no room for the table");
    SkContext& ctx = sk_ctx();
    SK_HIP(skrt::setDevice(ctx.device));
    hipStream_t st = ctx.stream;
    int32_t *d_off = nullptr, *d_order = nullptr;
    int rc = 0;
    auto run = [&]() -> int {
        SK_HIP(skrt::malloc_(&d_off, 4 * (size_t(n_reads) + 1)));
        SK_HIP(skrt::malloc_(&d_order, 4 * size_t(T)));
        SK_HIP(skrt::memcpyAsync(d_off, cal_off, 4 * (size_t(n_reads) + 1), hipMemcpyHostToDevice, st));
        SK_HIP(skrt::memsetAsync(d_order, 0xff, 4 * size_t(T), st)); // (an entry the kernel left out shows as -1)
        launch_tail_order(st, TailArgs{ d_off, n_reads - T, T, shift, d_order });
        SK_HIP(skrt::getLastError());
        SK_HIP(skrt::memcpyAsync(order_out, d_order, 4 * size_t(T), hipMemcpyDeviceToHost, st));
        SK_HIP(skrt::streamSynchronize(st));
        return 0;
    };
    rc = run();
    if (d_off) (void)skrt::free_(d_off);
    if (d_order) (void)skrt::free_(d_order);
    return rc;
}
extern "C" int64_t sk_debug_f5_tail_launches(void) { return state().tail_launches; }
extern "C" int64_t sk_debug_f5_shared_rounds(void) { return state().shared_rounds; }
extern "C" int64_t sk_debug_f5_late_turn_downs(void) { return state().late_turn_downs; }

// ---------------------------------------------------------------------------------------------------------------------
// the job driver.  A job is prepared once (start_job, plan_job: capacities, the arenas' layout, reservations, the packed input on its way up)
// and then run either as ONE fixed sequence of submissions with one host wait (run_one_wait) or the staged way, with a wait after the
// search, one after the sets and one at the end (run_staged).  One builder per kernel argument struct: its parameters are what differs
// between the two runs.
namespace
{
constexpr int ONE_WAIT_MAX_READS = 16384; // reads of a job that runs as one fixed sequence (its buffers are sized by capacities: 256 leaves per read)

struct JobPlan
{
    const SkEnumInput* in = nullptr;
    EnumBuffers& B = bufs();
    hipStream_t st = nullptr;
    bool one_wait = false, with_stage3 = false;
    bool fused = true; // F5 scores the job unless $SK_A5_FUSED = 0 (tests: both chains); read once per job, sk_enum_device_run
    int n = 0;
    int64_t n_bases = 0, frame_cap = 0, pool_cap = 0; // capacities: calls in flight at one depth, leaves found (before duplicates are dropped)
    int W = 0;                                        // words of a read's event mask
    int max_order = 0;                                // the deepest indel order a read of the job arrives with
    size_t in_bytes = 0, zero_bytes = 0, minmax_bytes = 0, mask_bytes = 0; // the arenas
    size_t minmax_split = 0;                                               // win_begin, ins_lo before it; win_end, ins_hi from it on
    PJob dj;
    // stage 3: a read with at most light_cals candidate alignments is the first launch's; a block keeps up to lds_cals of them in LDS
    int light_cals = S3_LIGHT_CALS, lds_cals = S3_LDS_CALS;
    bool timing = false; // $SK_ENUM_TIMING
    std::chrono::steady_clock::time_point t_begin;

    void lap(const char* what) const
    {
        if (!timing) return;
        (void)skrt::streamSynchronize(st);
        std::fprintf(stderr, "[enum-dev] %-28s t=%.3f ms\n", what,
                     std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count());
    }
};

struct Piece // of an arena, at a 256-byte offset
{
    View* view;
    const void* src; // in_arena: where the bytes come from
    size_t bytes, off;
};
size_t lay_out(Piece* pc, const int n_pieces)
{
    size_t at = 0;
    for (int i = 0; i < n_pieces; ++i) {
        pc[i].off = at;
        at += (pc[i].bytes + 255) & ~size_t(255);
    }
    return at;
}

// everything about a job that is known before its first submission.  one_wait: the buffers between the search and stage 3 will be sized
// by the pool's capacity, and cal_off is made on the device (a piece of the zero arena)
int plan_job(const SkEnumInput* in, const bool one_wait, const bool fused, JobPlan& p)
{
    EnumBuffers& B = p.B;
    p.in = in;
    p.st = sk_ctx().stream;
    p.one_wait = one_wait;
    p.fused = fused;
    const int n = p.n = in->n_reads;
    const int64_t n_bases = p.n_bases = n ? in->read_off[n] : 0;
    // capacities: calls in flight at one depth and leaves found (before duplicates are dropped), for the whole job; a job that
    // needs more has the reads that did not fit enumerated on the host
    // (sized by the job; the ceilings -- two level buffers of 2^23 frames, 2^25 leaves: ~21 GB in all -- are a fraction of 288 GB of HBM
    // and let a job of 2^16 reads with ~90 candidate alignments each run whole)
    p.frame_cap = std::min<int64_t>(std::max<int64_t>(int64_t(n) * 128, 1 << 18), 1 << 23);
    p.pool_cap = std::min<int64_t>(std::max<int64_t>(int64_t(n) * 512, 1 << 19), int64_t(32) << 20);
    const char* const test_caps = std::getenv("SK_ENUM_TEST_CAPS"); // tests: small capacities, so that the overflow paths run
    if (test_caps) {
        long long fc = 0, pc = 0;
        if (std::sscanf(test_caps, "%lld,%lld", &fc, &pc) == 2 && fc > 0 && pc > 0) {
            p.frame_cap = std::max<int64_t>(fc, n);
            p.pool_cap = pc;
        }
    }
    // one sequence: the buffers between the search and stage 3 are sized by the pool's capacity instead of by counts the host would have
    // to wait for -- 256 leaves per read (at least 2^17) cover every WGS-like job; one that needs more is run again the staged way
    if (one_wait && !(test_caps && test_caps[0])) p.pool_cap = std::min<int64_t>(p.pool_cap, std::max<int64_t>(int64_t(n) * 256, 1 << 17));
    const bool s3 = p.with_stage3 = in->want_scores && in->want_stage3;
    const int W = p.W = sk_ent_evmask_words(std::max(in->max_read_len, 0));
    for (int r = 0; r < n; ++r) p.max_order = std::max(p.max_order, int(in->reads[r].n_order));
    if (const char* e = std::getenv("SK_STAGE3_TEST_LDS_CALS")) { // tests: small capacities, so that the second launch and the HBM arrays run
        int a = 0, b = 0;
        if (std::sscanf(e, "%d,%d", &a, &b) == 2 && a > 0 && b >= a && b <= S3_LDS_CALS) {
            p.light_cals = a;
            p.lds_cals = b;
        }
    }
    if (reserve_dev({ { B.level_a, sizeof(PFrame) * size_t(p.frame_cap) }, { B.level_b, sizeof(PFrame) * size_t(p.frame_cap) },
                      { B.pool, sizeof(PCal) * size_t(p.pool_cap) }, { B.leaf_read, 4 * size_t(p.pool_cap) }, { B.leaf_hash, 4 * size_t(p.pool_cap) },
                      { B.raw_off, 4 * size_t(n + 1) }, { B.win_len, 4 * size_t(n) }, { B.n_ins, 4 * size_t(n) },
                      { B.ins_idx, 2 * size_t(n) * INS_CAP }, { B.ins_off, 4 * size_t(n) * INS_CAP },
                      { B.cal_off, 4 * size_t(n + 1) }, { B.hap_off, 8 * size_t(n + 1) },
                      { B.tail_order, 4 * size_t(std::min(n, F5_TAIL_MAX)) } }) || // (F5's last hand-outs: a window is at most this, plan_tail)
        reserve_pinned({ { B.h_raw_off, 4 * size_t(n + 1) }, { B.h_cal_off, 4 * size_t(n + 1) }, { B.h_hap_off, 8 * size_t(n + 1) } }))
        return 1;
    // ---- the arenas: pieces at 256-byte offsets
    Piece ins_p[] = {
        { &B.tab, in->tab, sizeof(PIndel) * size_t(in->n_tab), 0 },
        { &B.ins, in->ins_pool, size_t(in->ins_pool_len), 0 },
        { &B.toggle, in->max_toggle, sizeof(uint32_t) * size_t(in->n_max_toggle), 0 },
        { &B.ref, in->ref, size_t(std::max(in->ref_len, 0)), 0 },
        { &B.reads, in->reads, sizeof(PRead) * size_t(n), 0 },
        { &B.read_off, in->read_off, sizeof(int64_t) * size_t(n + 1), 0 },
        { &B.read_code, in->read_code, size_t(n_bases), 0 },
        { &B.read_qual, in->read_qual, size_t(n_bases), 0 },
        { &B.r2i, in->r2i, s3 ? 8 * size_t(in->n_tab) : 0, 0 },
        { &B.i2r, in->i2r, s3 ? 8 * size_t(in->n_tab) : 0, 0 },
        { &B.orig, in->orig, s3 ? 4 * size_t(in->n_tab) : 0, 0 },
        { &B.map_level, in->map_level, s3 ? 4 * size_t(n) : 0, 0 },
        // (no source: the code images are written into the mirror below)
        { &B.ref_code, nullptr, size_t(std::max(in->ref_len, 0)) + 2 * size_t(F5_CODE_PAD), 0 },
        { &B.ins_code, nullptr, size_t(in->ins_pool_len), 0 },
    };
    const int n_ins_p = int(sizeof(ins_p) / sizeof(ins_p[0]));
    p.in_bytes = lay_out(ins_p, n_ins_p);
    // (the order matters: what the host reads after the search is one run, what it reads after the layout another)
    Piece zero_p[] = {
        { &B.counters, nullptr, 4 * size_t(N_COUNTERS), 0 }, { &B.warn, nullptr, 4 * size_t(n), 0 },    { &B.n_raw, nullptr, 4 * size_t(n), 0 },
        { &B.status, nullptr, 4 * size_t(n), 0 },            { &B.hap_len, nullptr, 4 * size_t(n), 0 }, { &B.fill, nullptr, 4 * size_t(n), 0 },
        { &B.n_uniq, nullptr, 4 * size_t(n), 0 },            { &B.consulted, nullptr, size_t(in->n_tab) + 1, 0 },
        { &B.cal_off_z, nullptr, one_wait ? 4 * size_t(n + 1) : 0, 0 }, // (one sequence: cal_off is made on the device and comes back with the arena)
    };
    View* zero_host[] = { &B.h_counters, &B.h_warn, &B.h_n_raw, &B.h_status, &B.h_hap_len, nullptr, &B.h_n_uniq, &B.h_consulted, &B.h_cal_off_z };
    const int n_zero_p = int(sizeof(zero_p) / sizeof(zero_p[0]));
    p.zero_bytes = lay_out(zero_p, n_zero_p);
    Piece minmax_p[] = { { &B.win_begin, nullptr, 4 * size_t(n), 0 }, { &B.ins_lo, nullptr, 4 * size_t(n), 0 },
                         { &B.win_end, nullptr, 4 * size_t(n), 0 },   { &B.ins_hi, nullptr, 4 * size_t(n), 0 } };
    p.minmax_bytes = lay_out(minmax_p, 4);
    p.minmax_split = minmax_p[2].off;
    Piece mask_p[] = { { &B.evmask, nullptr, 4 * (size_t(n) * size_t(W) + 1), 0 }, { &B.addmask, nullptr, 4 * (size_t(n) * size_t(W) + 1), 0 } };
    p.mask_bytes = lay_out(mask_p, 2);
    if (reserve_dev({ { B.in_arena, p.in_bytes }, { B.zero_arena, p.zero_bytes }, { B.minmax_arena, p.minmax_bytes }, { B.mask_arena, p.mask_bytes } })) return 1;
    if (reserve_pinned({ { B.h_in_arena, p.in_bytes }, { B.h_zero_arena, p.zero_bytes } })) return 1;
    for (int i = 0; i < n_ins_p; ++i) {
        ins_p[i].view->p = static_cast<char*>(B.in_arena.p) + ins_p[i].off;
        if (ins_p[i].bytes && ins_p[i].src) std::memcpy(static_cast<char*>(B.h_in_arena.p) + ins_p[i].off, ins_p[i].src, ins_p[i].bytes);
    }
    { // the job's code images, made once where its reference and its insert pool go up
        const CodeLut& lut = code_lut();
        const size_t ref_n = size_t(std::max(in->ref_len, 0));
        uint8_t* rc = static_cast<uint8_t*>(B.h_in_arena.p) + size_t(static_cast<char*>(B.ref_code.p) - static_cast<char*>(B.in_arena.p));
        std::memset(rc, SK_BAM_ANY, size_t(F5_CODE_PAD));
        for (size_t i = 0; i < ref_n; ++i) rc[size_t(F5_CODE_PAD) + i] = lut.code[uint8_t(in->ref[i])];
        std::memset(rc + size_t(F5_CODE_PAD) + ref_n, SK_BAM_ANY, size_t(F5_CODE_PAD));
        uint8_t* ic = static_cast<uint8_t*>(B.h_in_arena.p) + size_t(static_cast<char*>(B.ins_code.p) - static_cast<char*>(B.in_arena.p));
        for (size_t i = 0; i < size_t(in->ins_pool_len); ++i) ic[i] = lut.code[uint8_t(in->ins_pool[i])];
    }
    for (int i = 0; i < n_zero_p; ++i) {
        zero_p[i].view->p = static_cast<char*>(B.zero_arena.p) + zero_p[i].off;
        if (zero_host[i]) zero_host[i]->p = static_cast<char*>(B.h_zero_arena.p) + zero_p[i].off;
    }
    for (int i = 0; i < 4; ++i) minmax_p[i].view->p = static_cast<char*>(B.minmax_arena.p) + minmax_p[i].off;
    for (int i = 0; i < 2; ++i) mask_p[i].view->p = static_cast<char*>(B.mask_arena.p) + mask_p[i].off;

    p.dj.tab = B.tab.as<PIndel>();
    p.dj.n_tab = in->n_tab;
    p.dj.max_toggle = B.toggle.as<uint32_t>();
    p.dj.n_max_toggle = in->n_max_toggle;
    p.dj.sample_count = in->sample_count;
    p.dj.max_read_indel_toggle = in->max_read_indel_toggle;
    p.dj.max_candidate_indel_density = in->max_candidate_indel_density;
    p.dj.is_haplotyping_enabled = in->is_haplotyping_enabled;
    p.dj.max_indel_size = in->max_indel_size;
    p.dj.consulted = B.consulted.as<uint8_t>();
    p.dj.max_nodes = 0;
    return 0;
}

// the copy / fill calls instead of the job_stage_*_kernel launches of a one-sequence run ($SK_ENUM_STAGE_COPIES, for A-B runs)
bool stage_by_kernel()
{
    static const bool by_kernel = !env_set("SK_ENUM_STAGE_COPIES");
    return by_kernel;
}

// the job's way in: the packed input up, the zero arena zeroed
int stage_in(const JobPlan& p)
{
    EnumBuffers& B = p.B;
    if (p.one_wait && stage_by_kernel()) {
        const uint32_t n_in16 = uint32_t(p.in_bytes / 16), n_zero16 = uint32_t(p.zero_bytes / 16); // (pieces sit at 256-byte offsets)
        const int blocks = int(std::min<size_t>(std::max<size_t>((std::max(p.in_bytes, p.zero_bytes) / 16 + 255) / 256, 1), 256));
        SK_LAUNCH(job_stage_in_kernel, dim3(blocks), dim3(256), 0, p.st, static_cast<const uint4*>(B.h_in_arena.p), static_cast<uint4*>(B.in_arena.p), n_in16,
                  static_cast<uint4*>(B.zero_arena.p), n_zero16);
    } else {
        if (copy_up(p.st, B.in_arena, B.h_in_arena.p, p.in_bytes)) return 1;
        SK_HIP(skrt::memsetAsync(B.zero_arena.p, 0, p.zero_bytes, p.st));
    }
    return 0;
}

// a run of the zero arena, device -> its pinned mirror
int fetch_zero(const JobPlan& p, const View& first, const View& last, const size_t last_bytes)
{
    char* const dev = static_cast<char*>(p.B.zero_arena.p);
    const size_t a0 = size_t(static_cast<char*>(first.p) - dev);
    const size_t a1 = size_t(static_cast<char*>(last.p) - dev) + last_bytes;
    SK_HIP(skrt::memcpyAsync(static_cast<char*>(p.B.h_zero_arena.p) + a0, dev + a0, a1 - a0, hipMemcpyDeviceToHost, p.st));
    return 0;
}

// a new generation of results, the plan, the input on its way; a job without reads is complete after this
int start_job(const SkEnumInput* in, SkEnumOutput* out, const bool one_wait, const bool fused, JobPlan& p)
{
    SK_REQUIRE_INIT();
    skrt::wakeHint();
    if (!in || !out) return sk_fail("sk_enum_device_run: null argument");
    std::memset(out, 0, sizeof(*out));
    out->generation = ++state().generation; // (before anything below can fail: a failed job, too, ends the last run's generation)
    state().forget_run();
    if (in->n_reads < 0 || in->n_tab < 0) return sk_fail("sk_enum_device_run: negative count");
    SK_HIP(skrt::setDevice(sk_ctx().device));
    p.timing = env_set("SK_ENUM_TIMING");
    p.t_begin = std::chrono::steady_clock::now();
    if (plan_job(in, one_wait, fused, p) || stage_in(p)) return 1;
    EnumBuffers& B = p.B;
    B.h_cal_off.as<int32_t>()[0] = 0;
    out->status = B.h_status.as<int32_t>();
    out->cal_off = B.h_cal_off.as<int32_t>();
    out->consulted = B.h_consulted.as<uint8_t>();
    if (p.n == 0) {
        std::memset(B.h_consulted.p, 0, size_t(in->n_tab));
        return 0;
    }
    if (p.n > p.frame_cap) return sk_fail("sk_enum_device_run: more reads in one job than the device pipeline holds");
    p.lap("H2D");
    return 0;
}

// ---- the kernels' arguments

// root_sets_minmax: the root launch initialises the four minmax arrays (else they are filled before pool_bounds_kernel)
EnumArgs enum_args(const JobPlan& p, const bool root_sets_minmax)
{
    EnumBuffers& B = p.B;
    int32_t* const counters = B.counters.as<int32_t>();
    EnumArgs ea{}; // (level_in, level_out, depth: launch_search)
    ea.job = p.dj;
    ea.reads = B.reads.as<PRead>();
    ea.n_reads = p.n;
    ea.frame_cap = int32_t(p.frame_cap);
    ea.level_count = counters + CNT_LEVELS;
    ea.pool = B.pool.as<PCal>();
    ea.leaf_read = B.leaf_read.as<int32_t>();
    ea.leaf_hash = B.leaf_hash.as<uint32_t>();
    ea.pool_cap = int32_t(p.pool_cap);
    ea.n_leaves = counters + CNT_LEAVES;
    ea.n_nodes = reinterpret_cast<unsigned long long*>(counters + CNT_NODES);
    ea.n_raw = B.n_raw.as<int32_t>();
    ea.status = B.status.as<int32_t>();
    ea.warn = B.warn.as<int32_t>();
    ea.min_cells_a = root_sets_minmax ? B.win_begin.as<int32_t>() : nullptr;
    ea.min_cells_b = root_sets_minmax ? B.ins_lo.as<int32_t>() : nullptr;
    ea.max_cells_a = root_sets_minmax ? B.win_end.as<int32_t>() : nullptr;
    ea.max_cells_b = root_sets_minmax ? B.ins_hi.as<int32_t>() : nullptr;
    return ea;
}

// E1: the launches of depths [d0, d1) -- depth -1 is the root launch --, the two level buffers taking turns
void launch_search(const JobPlan& p, EnumArgs ea, const int d0, const int d1, const int level_blocks)
{
    PFrame* const buf[2] = { p.B.level_a.as<PFrame>(), p.B.level_b.as<PFrame>() };
    for (int d = d0; d < d1; ++d) {
        ea.level_in = (d < 0) ? nullptr : buf[d & 1];
        ea.level_out = buf[(d + 1) & 1];
        ea.depth = d;
        if (d < 0) SK_LAUNCH(root_kernel, dim3((p.n + 63) / 64), dim3(64), 0, p.st, ea);
        else SK_LAUNCH(level_kernel, dim3(level_blocks), dim3(64), 64 * sizeof(PFrame), p.st, ea);
    }
}

// n_leaves_dev: null, or where the search counted its leaves (n_leaves is then the pool's capacity)
SetArgs set_args(const JobPlan& p, const int32_t n_leaves, const int32_t* n_leaves_dev, const int32_t* cal_off)
{
    EnumBuffers& B = p.B;
    SetArgs sa{};
    sa.pool = B.pool.as<PCal>();
    sa.leaf_read = B.leaf_read.as<int32_t>();
    sa.leaf_hash = B.leaf_hash.as<uint32_t>();
    sa.status = B.status.as<int32_t>();
    sa.n_reads = p.n;
    sa.n_leaves = n_leaves;
    sa.n_leaves_dev = n_leaves_dev;
    sa.raw_off = B.raw_off.as<int32_t>();
    sa.fill = B.fill.as<int32_t>();
    sa.grouped = B.grouped.as<int32_t>();
    sa.ghash = B.ghash.as<uint32_t>();
    sa.gkey = B.gkey.as<ulonglong2>();
    sa.dup = B.dup.as<uint8_t>();
    sa.n_uniq = B.n_uniq.as<int32_t>();
    sa.cal_off = cal_off;
    sa.sorted = B.sorted.as<int32_t>();
    return sa;
}

// n_cals_on_device: the count is cal_off[n] (n_cals is then a capacity); n_ops: null unless L2 runs; chain: with the arrays of the
// staged chain (F1-F3 + A1c), which are reserved once the layout pass has come back
FlatArgs flat_args(const JobPlan& p, const int32_t n_cals, const bool n_cals_on_device, const int32_t* cal_off, int32_t* n_ops, const bool chain)
{
    EnumBuffers& B = p.B;
    FlatArgs fa{};
    fa.job = p.dj;
    fa.ins_pool = B.ins.as<char>();
    fa.ref = B.ref.as<char>();
    fa.ref_code = B.ref_code.as<uint8_t>() + F5_CODE_PAD;
    fa.ins_code = B.ins_code.as<uint8_t>();
    fa.ref_offset = p.in->ref_offset;
    fa.ref_len = p.in->ref_len;
    fa.n_reads = p.n;
    fa.n_cals = n_cals;
    fa.n_cals_on_device = n_cals_on_device ? 1 : 0;
    fa.pool = B.pool.as<PCal>();
    fa.list = B.sorted.as<int32_t>();
    fa.status = B.status.as<int32_t>();
    fa.read_off = B.read_off.as<int64_t>();
    fa.read_code = B.read_code.as<uint8_t>();
    fa.cal_off = cal_off;
    fa.win_begin = B.win_begin.as<int32_t>();
    fa.win_len = B.win_len.as<int32_t>();
    fa.hap_len = B.hap_len.as<int32_t>();
    fa.n_ins = B.n_ins.as<int32_t>();
    fa.ins_idx = B.ins_idx.as<int16_t>();
    fa.ins_off = B.ins_off.as<int32_t>();
    fa.n_ops = n_ops;
    fa.win_end = B.win_end.as<int32_t>();
    fa.ins_lo = B.ins_lo.as<int32_t>();
    fa.ins_hi = B.ins_hi.as<int32_t>();
    fa.n_seg8 = B.n_seg8.as<uint8_t>();
    fa.max_read_len = p.in->max_read_len;
    fa.ref_outside = B.counters.as<int32_t>() + CNT_DYN + DYN_REF_OUTSIDE;
    if (chain) {
        fa.cals = B.cals.as<PCal>();
        fa.hap_off = B.hap_off.as<int64_t>();
        fa.op_off = B.op_off.as<int64_t>();
        fa.hap_code = B.hap_code.as<uint8_t>();
        fa.ops = B.ops.as<sk_score_op>();
        fa.entries = B.entries.as<uint32_t>();
        fa.evmask = B.evmask.as<uint32_t>();
        fa.evmask_words = p.W;
        fa.colmat = B.colmat.as<uint8_t>();
        fa.colmat_off = B.colmat_off.as<int64_t>();
        fa.addmask = B.addmask.as<uint32_t>();
    }
    return fa;
}

FusedScoreArgs fused_args(const JobPlan& p, const FlatArgs& fa)
{
    EnumBuffers& B = p.B;
    FusedScoreArgs fs;
    fs.f = fa;
    fs.read_qual = B.read_qual.as<uint8_t>();
    fs.tab = sk_ctx().dev_tables;
    fs.scores = B.scores.as<double>();
    fs.err = sk_ctx().dev_error_flags;
    fs.n_unhandled = B.counters.as<int32_t>() + CNT_UNHANDLED;
    fs.queue = B.counters.as<unsigned>() + CNT_QUEUE;
    fs.write_cals = 0;
    fs.dbg = nullptr;
    fs.tail_order = nullptr; // (plan_tail)
    fs.tail_first = fs.tail_n = 0;
    // $SK_F5_SHARE = 0: no round sharing (experiments and tests; read once)
    static const bool share = !env_is("SK_F5_SHARE", "0");
    fs.share = share ? 1 : 0;
    fs.shared_rounds = B.counters.as<unsigned>() + CNT_SHARED;
    return fs;
}

// the table of F5's last hand-outs, built on the job's stream from cal_off (after pool_layout_kernel, before F5) and named in the launch's
// arguments.  A job that fits the grid makes no draw and gets no launch here; nor does any job with the shift off.  The table's buffer
// is reserved with the job's others (plan_job): nothing is allocated between the submissions of a sequence.
void plan_tail(const JobPlan& p, FusedScoreArgs& fs)
{
    EnumBuffers& B = p.B;
    const int W = f5_grid(p.n, fs.f.max_read_len).waves();
    const int shift = f5_tail_shift(W), T = f5_tail_window(p.n, W, shift); // (T <= min(n, F5_TAIL_MAX): f5_tail_shift)
    if (T == 0) return;
    launch_tail_order(p.st, TailArgs{ fs.f.cal_off, p.n - T, T, shift, B.tail_order.as<int32_t>() });
    ++state().tail_launches;
    fs.tail_order = B.tail_order.as<int32_t>();
    fs.tail_first = uint32_t(p.n - T);
    fs.tail_n = uint32_t(T);
}

// stage 3's arrays: per candidate alignment (n_cals: the count, or a capacity), per base, a record per read
int reserve_stage3(EnumBuffers& B, const int n, const int64_t n_bases, const int32_t n_cals)
{
    if (reserve_dev({ { B.s3_order, 4 * size_t(n_cals) }, { B.s3_smooth, 8 * size_t(n_cals) }, { B.s3_flag, size_t(n_cals) },
                      { B.s3_rm_type, size_t(n_bases) }, { B.s3_rm_pos, 4 * size_t(n_bases) }, { B.s3_key, 16 * size_t(n_cals) },
                      { B.s3_sorted_score, 8 * size_t(n_cals) }, { B.s3_sorted_hash, 4 * size_t(n_cals) }, { B.s3_next_same, 4 * size_t(n_cals) },
                      { B.s3_removed, size_t(n_cals) }, { B.s3_range_end, 4 * size_t(n_cals) }, { B.s3_out, sizeof(sk3::Out) * size_t(n) } }))
        return 1;
    return reserve_pinned({ { B.h_s3_out, sizeof(sk3::Out) * size_t(n) } });
}

// cals, slot: the records in set order and null -- or the pool the search left its leaves in and each alignment's slot there;
// skip_if: null, or F5's count of the reads it turned down (nothing runs when it is not zero: the scores are incomplete).
// What is a launch's own (its list, the capacity in LDS) is launch_stage3's
Stage3Args stage3_args(const JobPlan& p, const FlatArgs& fa, const PCal* cals, const int32_t* slot, const int32_t* skip_if)
{
    EnumBuffers& B = p.B;
    Stage3Args s3{};
    s3.tab.tab = p.dj.tab;
    s3.tab.r2i = B.r2i.as<double>();
    s3.tab.i2r = B.i2r.as<double>();
    s3.tab.orig = B.orig.as<int32_t>();
    s3.tab.n_tab = p.in->n_tab;
    s3.tab.max_indel_size = p.in->max_indel_size;
    s3.tab.consulted = p.dj.consulted;
    s3.opt = p.in->stage3_opt;
    s3.n_reads = p.n;
    s3.status = fa.status;
    s3.cal_off = fa.cal_off;
    s3.cals = cals;
    s3.slot = slot;
    s3.scores = B.scores.as<double>();
    s3.read_off = fa.read_off;
    s3.read_code = fa.read_code;
    s3.map_level = B.map_level.as<int32_t>();
    s3.order = B.s3_order.as<int32_t>();
    s3.smooth = B.s3_smooth.as<double>();
    s3.flag = B.s3_flag.as<uint8_t>();
    s3.rm_type = B.s3_rm_type.as<uint8_t>();
    s3.rm_pos = B.s3_rm_pos.as<int32_t>();
    s3.key = B.s3_key.as<uint32_t>();
    s3.sorted_score = B.s3_sorted_score.as<double>();
    s3.sorted_hash = B.s3_sorted_hash.as<uint32_t>();
    s3.next_same = B.s3_next_same.as<int32_t>();
    s3.removed = B.s3_removed.as<uint8_t>();
    s3.range_end = B.s3_range_end.as<int32_t>();
    s3.out = B.s3_out.as<sk3::Out>();
    s3.skip_if = skip_if;
    return s3;
}

// one of stage 3's two launches, WAVES wavefronts a read: `blocks` reads of `list` (n_list null), or a block per read of the job with the
// list's length on the device (n_list; list_step -1: the list is filled from the back)
template <int WAVES>
void launch_stage3(hipStream_t st, Stage3Args s3, const int blocks, const int32_t* list, const int32_t* n_list, const int list_step, const int lds_cals)
{
    s3.list = list;
    s3.n_list = n_list;
    s3.list_step = list_step;
    s3.lds_cals = lds_cals;
    SK_LAUNCH(stage3_kernel<WAVES>, dim3(blocks), dim3(64 * WAVES), size_t(lds_cals) * (8 + 8 + 4 + 4 + 4 + 4 + 1 + 1) + 8, st, s3);
}

// warn as the caller reads it: a byte per read, made in place (byte r is written after int r was read)
const uint8_t* narrow_warn(EnumBuffers& B, const int n)
{
    uint8_t* w8 = reinterpret_cast<uint8_t*>(B.h_warn.p);
    const int32_t* w32 = B.h_warn.as<int32_t>();
    for (int r = 0; r < n; ++r) w8[r] = uint8_t(w32[r]);
    return w8;
}

// ---- what sk_enum_device_rescore replays
int64_t job_cells(const SkEnumInput* in, const int32_t* h_cal_off)
{
    int64_t cells = 0;
    for (int r = 0; r < in->n_reads; ++r) cells += (in->read_off[r + 1] - in->read_off[r]) * int64_t(h_cal_off[r + 1] - h_cal_off[r]);
    return cells;
}
void remember_fused(const JobPlan& p, const FusedScoreArgs& fs, const int32_t n_cals)
{
    LastFlat& last = state().last;
    last.fused = true;
    last.fs = fs;
    last.fs.f.n_cals = n_cals;       // (the count, where the run knew a capacity)
    last.fs.f.ref_outside = nullptr; // (a repeat for the clock counts nothing)
    last.n = p.n;
    last.n_cals = n_cals;
    last.scores = fs.scores;
    last.cells = job_cells(p.in, p.B.h_cal_off.as<int32_t>());
    last.valid = true;
}
void remember_staged(const JobPlan& p, const FlatArgs& fa, const sk_align_batch& d, const size_t colmat_bytes)
{
    LastFlat& last = state().last;
    last.fused = false;
    last.fa = fa;
    last.fa.ref_outside = nullptr;
    last.d = d;
    last.mask_bytes = p.mask_bytes;
    last.colmat_bytes = colmat_bytes;
    last.n = p.n;
    last.n_cals = fa.n_cals;
    last.scores = p.B.scores.as<double>();
    last.cells = job_cells(p.in, p.B.h_cal_off.as<int32_t>());
    last.valid = true;
}

// ---- the staged chain's launches, as run_chain and sk_enum_device_rescore both submit them
// what F1-F3 write into: the event and add masks zeroed, the 0.0 column in every word of the column form
int fill_masks_colmat(hipStream_t st, EnumBuffers& B, const size_t mask_bytes, const size_t colmat_bytes)
{
    SK_HIP(skrt::memsetAsync(B.mask_arena.p, 0, mask_bytes, st)); // evmask, addmask
    SK_HIP(skrt::memsetAsync(B.colmat.p, SK_SEL_NONE | (SK_SEL_NONE << 4), colmat_bytes, st));
    return 0;
}
// F1, F2
void launch_fill_flatten(hipStream_t st, const FlatArgs& fa)
{
    SK_LAUNCH(pool_fill_kernel, dim3(fa.n_reads), dim3(64), 0, st, fa);
    SK_LAUNCH(flatten_kernel, dim3((fa.n_cals + 63) / 64), dim3(64), 0, st, fa);
}
// F3: a wave per read ($SK_F3_KERNEL = thread pins the thread-per-alignment form; the tests run both)
void launch_entries(hipStream_t st, const FlatArgs& fa)
{
    if (env_is("SK_F3_KERNEL", "thread")) SK_LAUNCH(entries_kernel, dim3((fa.n_cals + 63) / 64), dim3(64), 0, st, fa);
    else SK_LAUNCH(entries_wave_kernel, dim3(fa.n_reads), dim3(64), 0, st, fa);
}

// ---- the job as one fixed sequence: ~20 submissions, no host decision between them, ONE wait.  Everything the host computes between the
// staged run's waits is computed by job_scan_kernel; every buffer is sized by a capacity known now; launches whose size the host does
// not know cover the capacity with a grid-stride loop (or a block per read of the job that leaves at once).
// *redo is set when the sequence's assumptions did not hold for this job and nothing of `out` is valid: the caller runs it again the staged way
int run_one_wait(const JobPlan& p, SkEnumOutput* out, bool* redo)
{
    const auto t_setup = std::chrono::steady_clock::now();
    EnumBuffers& B = p.B;
    hipStream_t st = p.st;
    const int n = p.n;
    const int32_t n_cap = int32_t(p.pool_cap); // leaves, grouped leaves and candidate alignments are all at most this many
    if (reserve_dev({ { B.grouped, 4 * size_t(n_cap) }, { B.ghash, 4 * size_t(n_cap) }, { B.gkey, 16 * size_t(n_cap) }, { B.dup, size_t(n_cap) },
                      { B.sorted, 4 * size_t(n_cap) }, { B.n_seg8, size_t(n_cap) }, { B.scores, 8 * size_t(n_cap) }, { B.s3_list, 4 * size_t(n) } }) ||
        reserve_stage3(B, n, p.n_bases, n_cap))
        return 1;
    int32_t* const dyn = B.counters.as<int32_t>() + CNT_DYN;

    // E1: root + the levels up to the deepest order of the job (+ 2: indels that join an order on the way); whether calls were left
    // for a deeper level is looked at on the device (scan 1) and reported with the results
    const EnumArgs ea = enum_args(p, true);
    int n_levels = std::min(p.max_order + 3, int(SEARCH_LEVELS));
    if (const char* e = std::getenv("SK_ENUM_TEST_LEVELS")) // tests: too few levels, so that the device reports it and the job runs again
        if (std::atoi(e) > 0) n_levels = std::min(n_levels, std::atoi(e));
    // (a level of this job has at most a few frames per read: blocks beyond that would only read the count and leave)
    launch_search(p, ea, -1, n_levels, int(std::min<int64_t>(std::min<int64_t>((p.frame_cap + 63) / 64, 1024), std::max<int64_t>(n, 16))));
    // scan 1: raw_off
    ScanArgs sc{};
    sc.n_reads = n;
    sc.status = ea.status;
    sc.count = ea.n_raw;
    sc.off = B.raw_off.as<int32_t>();
    sc.dyn = dyn;
    sc.level_count = ea.level_count;
    sc.first_level_not_launched = (n_levels >= SEARCH_LEVELS) ? -1 : n_levels;
    sc.n_leaves = ea.n_leaves;
    sc.pool_cap = n_cap;
    SK_LAUNCH(job_scan_kernel<false>, dim3(1), dim3(1024), 0, st, sc);
    // E2
    const SetArgs sa = set_args(p, n_cap, ea.n_leaves, B.cal_off_z.as<int32_t>());
    // (grids for counts the host has not seen: enough blocks for ~64 leaves per read, the loops cover the rest)
    const int e2_blocks = int(std::min<int64_t>(std::max<int64_t>((int64_t(n) * 64 + 255) / 256, 8), 2048));
    SK_LAUNCH(group_kernel, dim3(e2_blocks), dim3(256), 0, st, sa);
    SK_LAUNCH(dedupe_kernel, dim3(e2_blocks), dim3(256), 0, st, sa);
    // scan 2: cal_off, stage 3's lists
    sc.count = B.n_uniq.as<int32_t>();
    sc.off = B.cal_off_z.as<int32_t>();
    sc.list = B.s3_list.as<int32_t>();
    sc.light_cals = p.light_cals;
    SK_LAUNCH(job_scan_kernel<true>, dim3(1), dim3(1024), 0, st, sc);
    SK_LAUNCH(rank_kernel, dim3(e2_blocks), dim3(256), 0, st, sa);
    // L1
    const FlatArgs fa = flat_args(p, n_cap, true, B.cal_off_z.as<int32_t>(), nullptr, false);
    SK_LAUNCH(pool_bounds_kernel, dim3(e2_blocks), dim3(256), 0, st, fa);
    SK_LAUNCH(pool_layout_kernel, dim3((n + 63) / 64), dim3(64), 0, st, fa);
    // F5, the table of its last hand-outs first
    FusedScoreArgs fs = fused_args(p, fa);
    plan_tail(p, fs);
    launch_flatten_score(n, st, fs);
    // S3: a block per read of the job in either launch; the blocks past a list's length leave at once
    // (the largest read of the heavy list is not known here: LDS for the most a block holds)
    const Stage3Args s3 = stage3_args(p, fa, fa.pool, fa.list, fs.n_unhandled);
    launch_stage3<1>(st, s3, n, B.s3_list.as<int32_t>(), dyn + DYN_N_LIGHT, 1, p.light_cals);
    launch_stage3<4>(st, s3, n, B.s3_list.as<int32_t>() + (n - 1), dyn + DYN_N_HEAVY, -1, p.lds_cals);
    SK_HIP(skrt::getLastError());
    // the results: the zero arena whole (counters + the scans' numbers, warn, n_raw, status, ..., consulted, cal_off) and stage 3's records
    const size_t out_bytes = sizeof(sk3::Out) * size_t(n);
    if (stage_by_kernel()) {
        const uint32_t n_a = uint32_t(p.zero_bytes / 16), n_b = uint32_t((out_bytes + 15) / 16); // (buffers are reserved with slack)
        const int blocks = int(std::min<size_t>(std::max<size_t>((std::max(p.zero_bytes, out_bytes) / 16 + 255) / 256, 1), 256));
        SK_LAUNCH(job_stage_out_kernel, dim3(blocks), dim3(256), 0, st, static_cast<const uint4*>(B.zero_arena.p), static_cast<uint4*>(B.h_zero_arena.p), n_a,
                  static_cast<const uint4*>(B.s3_out.p), static_cast<uint4*>(B.h_s3_out.p), n_b);
        SK_HIP(skrt::getLastError());
    } else {
        if (copy_down(st, B.h_zero_arena, B.zero_arena, p.zero_bytes) || copy_down(st, B.h_s3_out, B.s3_out, out_bytes)) return 1;
    }
    const auto t_submitted = std::chrono::steady_clock::now();
    SK_HIP(skrt::streamSynchronize(st));
    const auto t_waited = std::chrono::steady_clock::now();
    g_job_seconds.setup += std::chrono::duration<double>(t_setup - p.t_begin).count();
    g_job_seconds.submit += std::chrono::duration<double>(t_submitted - t_setup).count();
    g_job_seconds.wait += std::chrono::duration<double>(t_waited - t_submitted).count();
    p.lap("one sequence");
    const int32_t* h_counters = B.h_counters.as<int32_t>();
    const int32_t* const h_dyn = h_counters + CNT_DYN;
    EnumState& S = state();
    S.shared_rounds += h_counters[CNT_SHARED]; // (of this launch, whether the job is run again or not)
    S.late_turn_downs += h_counters[CNT_SHARED + 1];
    if (h_dyn[DYN_FLAGS] != 0 || h_counters[CNT_UNHANDLED] > 0) {
        if (p.timing)
            std::fprintf(stderr, "[enum-dev] one sequence: flags %d, reads outside F5's form %d -> the staged chain\n", h_dyn[DYN_FLAGS], h_counters[CNT_UNHANDLED]);
        *redo = true;
        return 0;
    }
    ++S.jobs_one_wait;
    out->warn = narrow_warn(B, n);
    int32_t* h_cal_off = B.h_cal_off.as<int32_t>();
    std::memcpy(h_cal_off, B.h_cal_off_z.p, 4 * size_t(n + 1));
    const int32_t n_cals = h_cal_off[n];
    S.n_cals = n_cals;
    S.cals_pool = fa.pool;
    S.cals_list = fa.list;
    S.scores = B.scores.as<double>();
    out->cals = nullptr;   // (in the pool: sk_enum_device_fetch_cals)
    out->scores = nullptr; // (on the device: sk_enum_device_fetch_scores -- the host needs them only for a read stage 3 turned down)
    out->stage3 = B.h_s3_out.as<sk3::Out>();
    out->ref_reads_outside = h_dyn[DYN_REF_OUTSIDE];
    remember_fused(p, fs, n_cals);
    if (p.timing)
        std::fprintf(stderr, "[enum-dev] one sequence: %d reads, %d levels launched, %d leaves, %d candidate alignments, stage 3 lists %d + %d\n", n, n_levels,
                     h_counters[CNT_LEAVES], n_cals, h_dyn[DYN_N_LIGHT], h_dyn[DYN_N_HEAVY]);
    return 0;
}

// ---- the staged run

// what follows the scores in either chain: the scores' way back, stage 3 (lists made here: the host has the counts).  cals_in_set_order:
// the staged chain left the records in B.cals (flatten_kernel); else they are where the search put them, and F5 counted the reads it turned
// down: stage 3 then has nothing to work on -- the staged chain scores the job and this runs again
int after_scores(const JobPlan& p, SkEnumOutput* out, const FlatArgs& fa, const bool cals_in_set_order)
{
    EnumBuffers& B = p.B;
    hipStream_t st = p.st;
    const int n = p.n;
    if (copy_down(st, B.h_scores, B.scores, 8 * size_t(fa.n_cals))) return 1;
    out->scores = B.h_scores.as<double>();
    if (!p.in->want_stage3) return 0;
    if (reserve_stage3(B, n, p.n_bases, fa.n_cals)) return 1;
    const Stage3Args s3 = cals_in_set_order ? stage3_args(p, fa, fa.cals, nullptr, nullptr)
                                            : stage3_args(p, fa, fa.pool, fa.list, B.counters.as<int32_t>() + CNT_UNHANDLED);
    // two launches: reads with few candidate alignments (small LDS, many wavefronts per CU) and the others
    if (reserve_dev({ { B.s3_list, 4 * size_t(n) } }) || reserve_pinned({ { B.h_s3_list, 4 * size_t(n) } })) return 1;
    int32_t* h_list = B.h_s3_list.as<int32_t>();
    const int32_t* h_cal_off = B.h_cal_off.as<int32_t>();
    int n_light = 0, n_heavy = 0, max_cals = 0;
    for (int r = 0; r < n; ++r) {
        const int k = h_cal_off[r + 1] - h_cal_off[r];
        if (k <= p.light_cals) h_list[n_light++] = r;
        else {
            h_list[n - 1 - n_heavy++] = r;
            max_cals = std::max(max_cals, k);
        }
    }
    if (copy_up(st, B.s3_list, h_list, 4 * size_t(n))) return 1;
    if (n_light > 0) launch_stage3<1>(st, s3, n_light, B.s3_list.as<int32_t>(), nullptr, 1, p.light_cals);
    if (n_heavy > 0) {
        const int32_t* heavy = B.s3_list.as<int32_t>() + (n - n_heavy);
        const int lds_cals = std::min(max_cals, p.lds_cals); // (a read with more uses the arrays in HBM)
        // four wavefronts per read: the loops over the read's alignments go four times as wide, lane 0's share stays
        static const bool one_wave = env_set("SK_STAGE3_ONE_WAVE"); // (diagnostics)
        if (one_wave) launch_stage3<1>(st, s3, n_heavy, heavy, nullptr, 1, lds_cals);
        else launch_stage3<4>(st, s3, n_heavy, heavy, nullptr, 1, lds_cals);
    }
    if (p.timing)
        std::fprintf(stderr, "[enum-dev] stage 3: %d reads with at most %d candidate alignments, %d with more (up to %d)\n", n_light, p.light_cals, n_heavy, max_cals);
    SK_HIP(skrt::getLastError());
    if (copy_down(st, B.h_s3_out, B.s3_out, sizeof(sk3::Out) * size_t(n))) return 1;
    out->stage3 = B.h_s3_out.as<sk3::Out>();
    p.lap("S3 stage 3");
    return 0;
}

// the staged chain's flattening and scoring (L2, F1-F3, A1c: ops, entries, column words through HBM) and, with scores, what follows them.
// It leaves the records in set order in B.cals.  layout: the job's FlatArgs as L1 ran with them
int run_chain(const JobPlan& p, SkEnumOutput* out, const FlatArgs& layout)
{
    const SkEnumInput* in = p.in;
    EnumBuffers& B = p.B;
    hipStream_t st = p.st;
    const int n = p.n;
    const int32_t n_cals = layout.n_cals;
    const int32_t* h_status = B.h_status.as<int32_t>();
    const int32_t* h_cal_off = B.h_cal_off.as<int32_t>();
    if (reserve_dev({ { B.cals, sizeof(PCal) * size_t(n_cals) } })) return 1;
    state().cals_gathered = true; // (flatten_kernel below writes them)
    if (n_cals > 0) {
        SK_LAUNCH(op_count_kernel, dim3((n_cals + 63) / 64), dim3(64), 0, st, layout);
        SK_HIP(skrt::getLastError());
    }
    if (fetch_zero(p, B.status, B.hap_len, 4 * size_t(n))) return 1; // status, hap_len (the host has made bytes of its copy of warn)
    if (copy_down(st, B.h_n_ops, B.n_ops, 4 * size_t(n_cals))) return 1;
    SK_HIP(skrt::streamSynchronize(st));
    p.lap("L1+L2 layout");

    const int32_t* h_hap_len = B.h_hap_len.as<int32_t>();
    const int32_t* h_n_ops = B.h_n_ops.as<int32_t>();
    int64_t* h_hap_off = B.h_hap_off.as<int64_t>();
    int64_t* h_op_off = B.h_op_off.as<int64_t>();
    h_hap_off[0] = 0;
    h_op_off[0] = 0;
    int32_t max_hap = 1;
    for (int r = 0; r < n; ++r) {
        const int32_t c0 = h_cal_off[r], c1 = h_cal_off[r + 1];
        h_hap_off[r + 1] = h_hap_off[r] + ((c1 > c0) ? h_hap_len[r] : 0);
        if (c1 > c0) max_hap = std::max(max_hap, h_hap_len[r]);
        const bool ok = (h_status[r] == ST_OK); // (a read turned down by L1/L2 keeps its slots in the batch, with no ops)
        for (int32_t c = c0; c < c1; ++c) h_op_off[c + 1] = h_op_off[c] + (ok ? h_n_ops[c] : 0);
    }
    const int64_t n_hap = h_hap_off[n], ops_total = h_op_off[n_cals];

    if (reserve_dev({ { B.hap_code, size_t(n_hap) + 16 }, { B.ops, sizeof(sk_score_op) * size_t(ops_total) }, { B.entries, 4 * (size_t(ops_total) + 2 * size_t(n_cals) + 1) } }) ||
        reserve_pinned({ { B.h_colmat_off, 8 * size_t(n + 1) } }))
        return 1;
    int64_t* h_colmat_off = B.h_colmat_off.as<int64_t>();
    h_colmat_off[0] = 0;
    for (int r = 0; r < n; ++r)
        h_colmat_off[r + 1] = h_colmat_off[r] + ((in->read_off[r + 1] - in->read_off[r] + 7) / 8) * int64_t(h_cal_off[r + 1] - h_cal_off[r]);
    const size_t colmat_bytes = 4 * size_t(h_colmat_off[n]) + 16;
    if (reserve_dev({ { B.colmat, colmat_bytes }, { B.colmat_off, 8 * size_t(n + 1) } })) return 1;
    if (n_cals == 0) return 0;

    if (copy_up(st, B.hap_off, h_hap_off, 8 * size_t(n + 1)) || copy_up(st, B.op_off, h_op_off, 8 * size_t(n_cals + 1))) return 1;
    if (fill_masks_colmat(st, B, p.mask_bytes, colmat_bytes)) return 1;
    if (copy_up(st, B.colmat_off, h_colmat_off, 8 * size_t(n + 1))) return 1;
    const FlatArgs fa = flat_args(p, n_cals, false, layout.cal_off, layout.n_ops, true);
    launch_fill_flatten(st, fa);
    SK_HIP(skrt::getLastError());
    if (p.with_stage3) out->cals = nullptr; // (they stay here: sk_enum_device_fetch_cals)
    else if (copy_down(st, B.h_cals, B.cals, sizeof(PCal) * size_t(n_cals))) return 1;
    if (!in->want_scores) return 0;
    launch_entries(st, fa);
    SK_HIP(skrt::getLastError());
    p.lap("F1-F3 flatten");
    sk_align_batch d{};
    d.n_reads = n;
    d.n_cals = n_cals;
    d.n_ops = ops_total;
    d.read_off = B.read_off.as<int64_t>();
    d.read_code = B.read_code.as<uint8_t>();
    d.read_qual = B.read_qual.as<uint8_t>();
    d.hap_off = fa.hap_off;
    d.hap_code = fa.hap_code;
    d.cal_off = fa.cal_off;
    d.op_off = fa.op_off;
    d.ops = fa.ops;
    d.max_read_len = in->max_read_len;
    d.max_hap_len = max_hap;
    d.entries = fa.entries;
    d.evmask = fa.evmask;
    d.evmask_words = p.W;
    d.colmat = B.colmat.as<uint32_t>();
    d.colmat_off = fa.colmat_off;
    d.addmask = fa.addmask;
    if (sk_score_alignments_launch_hostleg(&d, B.scores.as<double>(), st)) return 1;
    p.lap("A1 score");
    remember_staged(p, fa, d, colmat_bytes);
    return after_scores(p, out, fa, true);
}

// a wait after the search, one after the sets and one at the end; buffers sized by the counts that came back.  The scores come from F5
// or, when the job holds a read F5 turns down, when the host wants the alignments without scores and with $SK_A5_FUSED=0 (tests: both
// chains), from the staged chain
int run_staged(const JobPlan& p, SkEnumOutput* out)
{
    const SkEnumInput* in = p.in;
    EnumBuffers& B = p.B;
    hipStream_t st = p.st;
    const int n = p.n;
    EnumState& S = state();
    ++S.jobs_staged;
    // ---- E1: the search, one launch per depth.  A call at depth d expands indel order[d]; a call at depth n_order is a leaf.  A read's
    // order as it arrives says how deep its search goes unless an alignment reaches indels beyond the read's first range (they join the
    // order): the levels up to the deepest order of the job (+1) go out at once, the level counts that come back with the results say
    // whether more are needed
    const EnumArgs ea = enum_args(p, false);
    const int level_blocks = int(std::min<int64_t>((p.frame_cap + 63) / 64, 1024));
    launch_search(p, ea, -1, 0, level_blocks);
    for (int done = 0, batch = std::min(std::max(p.max_order + 2, 3), int(SEARCH_LEVELS));; batch = 4) {
        const int upto = std::min(done + batch, int(SEARCH_LEVELS));
        launch_search(p, ea, done, upto, level_blocks);
        done = upto;
        SK_HIP(skrt::getLastError());
        if (fetch_zero(p, B.counters, B.status, 4 * size_t(n))) return 1; // counters, warn, n_raw, status
        SK_HIP(skrt::streamSynchronize(st));
        if (done >= SEARCH_LEVELS || B.h_counters.as<int32_t>()[CNT_LEVELS + done] == 0) break;
    }
    p.lap("E1 search (all depths)");
    const int32_t* h_status = B.h_status.as<int32_t>();
    const int32_t* h_counters = B.h_counters.as<int32_t>();
    const int32_t n_leaves = std::min<int32_t>(h_counters[CNT_LEAVES], int32_t(p.pool_cap));
    if (p.timing) {
        long long calls = 0;
        int deepest = 0;
        for (int d = 0; d <= SEARCH_LEVELS; ++d) {
            calls += h_counters[CNT_LEVELS + d];
            if (h_counters[CNT_LEVELS + d]) deepest = d;
        }
        std::fprintf(stderr, "[enum-dev] search calls %lld, deepest level %d, leaves found %d\n", calls, deepest, n_leaves);
    }
    out->warn = narrow_warn(B, n);

    // ---- E2: leaves -> each read's set
    const int32_t* h_n_raw = B.h_n_raw.as<int32_t>();
    int32_t* h_raw_off = B.h_raw_off.as<int32_t>();
    h_raw_off[0] = 0;
    for (int r = 0; r < n; ++r) h_raw_off[r + 1] = h_raw_off[r] + ((h_status[r] == ST_OK) ? h_n_raw[r] : 0);
    const int32_t n_grouped = h_raw_off[n];
    if (reserve_dev({ { B.grouped, 4 * size_t(n_grouped) }, { B.ghash, 4 * size_t(n_grouped) }, { B.gkey, 16 * size_t(n_grouped) }, { B.dup, size_t(n_grouped) },
                      { B.sorted, 4 * size_t(n_grouped) } }))
        return 1;
    const SetArgs sa = set_args(p, n_leaves, nullptr, B.cal_off.as<int32_t>());
    if (copy_up(st, B.raw_off, h_raw_off, 4 * size_t(n + 1))) return 1;
    if (n_grouped > 0) {
        SK_LAUNCH(group_kernel, dim3((n_leaves + 255) / 256), dim3(256), 0, st, sa);
        SK_LAUNCH(dedupe_kernel, dim3((n_grouped + 255) / 256), dim3(256), 0, st, sa);
        SK_HIP(skrt::getLastError());
    }
    if (fetch_zero(p, B.n_uniq, B.n_uniq, 4 * size_t(n))) return 1;
    SK_HIP(skrt::streamSynchronize(st));
    const int32_t* h_n_uniq = B.h_n_uniq.as<int32_t>();
    int32_t* h_cal_off = B.h_cal_off.as<int32_t>();
    for (int r = 0; r < n; ++r) h_cal_off[r + 1] = h_cal_off[r] + ((h_status[r] == ST_OK) ? h_n_uniq[r] : 0);
    const int32_t n_cals = h_cal_off[n];
    if (copy_up(st, B.cal_off, h_cal_off, 4 * size_t(n + 1))) return 1;
    if (n_grouped > 0) {
        SK_LAUNCH(rank_kernel, dim3((n_grouped + 255) / 256), dim3(256), 0, st, sa);
        SK_HIP(skrt::getLastError());
    }
    p.lap("E2 sets");

    // ---- L1: layout of the batch
    if (reserve_dev({ { B.n_ops, 4 * size_t(n_cals) }, { B.op_off, 8 * size_t(n_cals + 1) }, { B.n_seg8, size_t(n_cals) }, { B.scores, 8 * size_t(n_cals) } }) ||
        reserve_pinned({ { B.h_n_ops, 4 * size_t(n_cals) }, { B.h_op_off, 8 * size_t(n_cals + 1) }, { B.h_scores, 8 * size_t(n_cals) } }))
        return 1;
    if (!p.with_stage3 && reserve_pinned({ { B.h_cals, sizeof(PCal) * size_t(n_cals) } })) return 1;
    const FlatArgs fa = flat_args(p, n_cals, false, B.cal_off.as<int32_t>(), B.n_ops.as<int32_t>(), false);
    // (byte patterns: 0x7f7f7f7f is large enough to stand for "no lower bound yet", 0x80808080 is below any position / index)
    SK_HIP(skrt::memsetAsync(B.minmax_arena.p, 0x7f, p.minmax_split, st));                                                                // win_begin, ins_lo
    SK_HIP(skrt::memsetAsync(static_cast<char*>(B.minmax_arena.p) + p.minmax_split, 0x80, p.minmax_bytes - p.minmax_split, st)); // win_end, ins_hi
    if (n_cals > 0) SK_LAUNCH(pool_bounds_kernel, dim3((n_cals + 255) / 256), dim3(256), 0, st, fa);
    SK_LAUNCH(pool_layout_kernel, dim3((n + 63) / 64), dim3(64), 0, st, fa);
    SK_HIP(skrt::getLastError());
    out->cals = B.h_cals.as<PCal>();
    S.n_cals = n_cals;
    S.cals_pool = fa.pool;
    S.cals_list = fa.list;

    // ---- flattening + scoring.  The default is F5 (flatten_score_kernel): one launch from the records to the scores, no layout pass
    // and no host wait before stage 3; it reads the records where the search left them
    bool chain = !(p.fused && in->want_scores && n_cals > 0);
    if (!chain) {
        FusedScoreArgs fs = fused_args(p, fa);
        plan_tail(p, fs); // (the table of F5's last hand-outs)
        launch_flatten_score(n, st, fs);
        SK_HIP(skrt::getLastError());
        p.lap("F5 flatten + score");
        if (in->want_stage3) {
            out->cals = nullptr; // (they stay here, in the pool: sk_enum_device_fetch_cals gathers them when the host asks)
        } else {
            if (reserve_dev({ { B.cals, sizeof(PCal) * size_t(n_cals) } })) return 1;
            SK_LAUNCH(gather_cals_kernel, dim3((n_cals + 63) / 64), dim3(64), 0, st, fa.pool, fa.list, n_cals, B.cals.as<PCal>());
            SK_HIP(skrt::getLastError());
            S.cals_gathered = true;
            if (copy_down(st, B.h_cals, B.cals, sizeof(PCal) * size_t(n_cals))) return 1;
        }
        remember_fused(p, fs, n_cals);
        if (after_scores(p, out, fa, false)) return 1;
        if (fetch_zero(p, B.counters, B.counters, 4 * size_t(N_COUNTERS))) return 1; // (n_unhandled)
        if (fetch_zero(p, B.status, B.status, 4 * size_t(n))) return 1;             // (F5 may have turned reads down: ST_FAIL)
        SK_HIP(skrt::streamSynchronize(st));
        chain = B.h_counters.as<int32_t>()[CNT_UNHANDLED] > 0; // a read outside F5's form: the staged chain over the job
    }
    if (chain && run_chain(p, out, fa)) return 1;
    if (fetch_zero(p, B.consulted, B.consulted, size_t(in->n_tab))) return 1;
    if (fetch_zero(p, B.counters, B.counters, 4 * size_t(N_COUNTERS))) return 1;
    SK_HIP(skrt::streamSynchronize(st));
    // (when F5 turned a read down both chains filled the pools: the count may be double -- what matters to the caller is zero or not)
    out->ref_reads_outside = B.h_counters.as<int32_t>()[CNT_DYN + DYN_REF_OUTSIDE];
    S.shared_rounds += B.h_counters.as<int32_t>()[CNT_SHARED]; // (the job's one F5 launch, if it had one: the counters' last fetch)
    S.late_turn_downs += B.h_counters.as<int32_t>()[CNT_SHARED + 1];
    p.lap("done");
    return 0;
}
} // namespace

// A job with the whole read path on the device (scores + stage 3) and F5 enabled runs as one fixed sequence with one wait; a job for
// which the sequence's assumptions do not hold (reported by the device with the results), one too large for capacity-sized buffers, and
// a caller that wants the alignments or the scores on the host run the staged way (a wait after the search, one after the sets, one at
// the end).  $SK_ENUM_ONE_WAIT = 0 pins the staged way (tests run both).
extern "C" int sk_enum_device_run(const SkEnumInput* in, SkEnumOutput* out)
{
    const bool fused = !env_is("SK_A5_FUSED", "0"); // (both read per job: tests flip them between the jobs of a process)
    if (!env_is("SK_ENUM_ONE_WAIT", "0") && fused && in && in->want_scores && in->want_stage3 && in->n_reads > 0 && in->n_reads <= ONE_WAIT_MAX_READS &&
        in->max_read_len <= F5_MAX_READ) {
        JobPlan p;
        bool redo = false;
        const int rc = start_job(in, out, true, fused, p) || run_one_wait(p, out, &redo);
        if (rc != 0 || !redo) return rc;
        ++state().jobs_one_wait_redone;
    }
    JobPlan p; // (a job run again is prepared again from the start: a new generation, another layout of the zero arena)
    if (start_job(in, out, false, fused, p)) return 1;
    return p.n == 0 ? 0 : run_staged(p, out);
}

// Measurement entry (bench.py's a5 leg): flattening AND scoring of the candidate alignments the last run left on the device, the way
// that run did it -- F5 (one launch from the records to the scores), or, for a job scored by the staged chain, pool bytes, ops,
// transition entries, masks and column words rebuilt from the PCal records (F1-F3), then the scoring kernel over them --
// `reps` times, timed with events on the library's stream.  This is what sk_enum_device_run does between the sets (E2) and stage 3,
// minus the layout pass (L1/L2: per-read pool bounds and op counts, whose results -- offsets -- a steady state already has).
extern "C" int sk_enum_device_rescore(const int32_t reps, float* out_ms, int32_t* out_n_reads, int32_t* out_n_cals, int64_t* out_cells)
{
    SK_REQUIRE_INIT();
    const LastFlat& last = state().last;
    if (!last.valid) return sk_fail("sk_enum_device_rescore: no device run with scores to repeat");
    if (reps <= 0 || !out_ms) return sk_fail("sk_enum_device_rescore: bad argument");
    if (skrt::remote()) return sk_fail("sk_enum_device_rescore: a timing entry point (events); not carried by the broker -- unset STRELKA_AMD_BROKER");
    SkContext& ctx = sk_ctx();
    SK_HIP(skrt::setDevice(ctx.device));
    hipStream_t st = ctx.stream;
    EnumBuffers& B = bufs();
    const FlatArgs& fa = last.fa;
    EventPair ev; // (destroyed on every return below)
    if (ev.create()) return 1;
    SK_HIP(hipEventRecord(ev.a, st));
    if (last.fused && env_set("SK_F5_TIMING") && f5_timing_report(st, last.fs, last.n, B.h_cal_off.as<int32_t>())) return 1;
    for (int i = 0; i < reps; ++i) {
        if (last.fused) { // F5: the records -> the scores in one launch
            launch_flatten_score(last.n, st, last.fs);
            continue;
        }
        if (fill_masks_colmat(st, B, last.mask_bytes, last.colmat_bytes)) return 1;
        launch_fill_flatten(st, fa);
        launch_entries(st, fa);
        if (sk_score_alignments_launch_hostleg(&last.d, last.scores, st)) return 1;
    }
    SK_HIP(hipEventRecord(ev.b, st));
    SK_HIP(hipEventSynchronize(ev.b));
    SK_HIP(skrt::getLastError());
    SK_HIP(hipEventElapsedTime(out_ms, ev.a, ev.b));
    if (out_n_reads) *out_n_reads = last.n;
    if (out_n_cals) *out_n_cals = last.n_cals;
    if (out_cells) *out_cells = last.cells;
    return 0;
}
