// indel_candidates.hip -- what the reference derives from an IndelBuffer entry before anything downstream reads it: the two depth buffers
// per sample, the four error rates per (key, sample), the breakpoint insert size and isCandidateIndel.  The rules are lettered in the
// header's block and restated one function each in tests/indel_candidates_model.py.
//
//   D0  depth_clear_kernel    both arrays and the control word to zero
//   D1  depth_ends_kernel     one thread per read: what the host entry refuses (iat, the path's place and segment types); per alignment-match
//       segment clipped to the window +1 at its first position and -1 behind its last, by integer atomics INTO the output arrays
//       (a segment that ends at the window's end needs no -1): sums of integers, the same whatever the order
//   D2  depth_scan_kernel     per array (blockIdx.y) and chunk of 1 024 positions the inclusive scan in place (block_scan.h), the chunk's
//       total to scratch
//   D3  depth_carry_kernel    per chunk the sum of the totals before it (the carried prefix), added to its positions; after a refusal
//       zeros instead
//   C0  cand_check_kernel     block 0: the rate sets, the key count against key_cap, the observation counts against obs_cap; all blocks:
//       dev_out to zero (rule B's atomicMax starts from 0)
//   C1  cand_bp_kernel        rule B: one thread per observation (blockIdx.y: the sample); a breakpoint observation finds its key by a
//       binary search over (pos, type) and raises bp_insert_size with an integer atomicMax
//   C2  cand_key_kernel       rules E and C: one thread per key, a loop over at most eight samples; totals by integer atomics
//
// Input the host entries refuse raises SK_DEVERR_READ_DEPTH / SK_DEVERR_INDEL_CANDIDATES and leaves zeroed output.
#include "sk_common.h"

#include "block_scan.h"
#include "libm_dbl64.h"

#include <climits>

namespace
{

enum { DEPTH_T = 1024, CAND_T = 256, CAND_GRID = 1024 };

struct DcPlus
{
    __device__ uint32_t operator()(const uint32_t a, const uint32_t b) const { return a + b; }
};

struct DepthArgs
{
    int32_t n_reads;
    const int64_t* path_off;
    const int32_t* n_seg;
    const sk_path_seg* path;
    int64_t path_cap;
    const int32_t* pos;
    const uint8_t* iat;
    int32_t win_begin, n_pos;
    uint32_t* depth[2];
    uint32_t* ctl;    // [0]: refused
    uint32_t* chunk;  // [2][n_chunks] the chunks' totals
    int32_t n_chunks;
    unsigned* err;
};

__global__ __launch_bounds__(DEPTH_T) void depth_clear_kernel(const DepthArgs a)
{
    const int64_t stride = int64_t(gridDim.x) * DEPTH_T;
    for (int64_t i = int64_t(blockIdx.x) * DEPTH_T + threadIdx.x; i < a.n_pos; i += stride) {
        a.depth[0][i] = 0;
        a.depth[1][i] = 0;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) a.ctl[0] = 0;
}

__device__ __forceinline__ bool dc_is_align_match(const uint32_t t) { return t == SK_SEG_MATCH || t == SK_SEG_SEQ_MATCH || t == SK_SEG_SEQ_MISMATCH; } // is_segment_align_match
__device__ __forceinline__ bool dc_is_ref_length(const uint32_t t) { return dc_is_align_match(t) || t == SK_SEG_DELETE || t == SK_SEG_SKIP; }          // is_segment_type_ref_length

// D1 -- rule D
__global__ __launch_bounds__(DEPTH_T) void depth_ends_kernel(const DepthArgs a)
{
    const int64_t stride = int64_t(gridDim.x) * DEPTH_T;
    const int64_t win_end = int64_t(a.win_begin) + a.n_pos;
    for (int64_t r = int64_t(blockIdx.x) * DEPTH_T + threadIdx.x; r < a.n_reads; r += stride) {
        const uint32_t iat = a.iat[r];
        const int64_t off = a.path_off[r];
        const int32_t ns = a.n_seg[r];
        if (iat > uint32_t(SK_IAT_SUBMAP) || ns < 0 || off < 0 || off > a.path_cap || int64_t(ns) > a.path_cap - off) {
            a.ctl[0] = 1; // (every writer writes 1)
            atomicOr(a.err, unsigned(SK_DEVERR_READ_DEPTH));
            continue;
        }
        uint32_t* d = iat == uint32_t(SK_IAT_SUBMAP) ? nullptr : a.depth[iat];
        int64_t head = a.pos[r]; // ref_head_pos
        for (int32_t k = 0; k < ns; ++k) {
            const sk_path_seg ps = a.path[off + k];
            if (ps.type > uint32_t(SK_SEG_SEQ_MISMATCH)) {
                a.ctl[0] = 1;
                atomicOr(a.err, unsigned(SK_DEVERR_READ_DEPTH));
                break;
            }
            if (d && dc_is_align_match(ps.type)) {
                int64_t b = head, e = head + int64_t(ps.length);
                if (b < a.win_begin) b = a.win_begin;
                if (b < e && b < win_end) {
                    atomicAdd(d + (b - a.win_begin), 1u);
                    if (e < win_end) atomicAdd(d + (e - a.win_begin), 0xffffffffu); // - 1 behind the last position
                }
            }
            if (dc_is_ref_length(ps.type)) head += int64_t(ps.length);
        }
    }
}

// D2
__global__ __launch_bounds__(DEPTH_T) void depth_scan_kernel(const DepthArgs a)
{
    __shared__ uint32_t s_wave[16];
    uint32_t* d = a.depth[blockIdx.y];
    for (int32_t c = blockIdx.x; c < a.n_chunks; c += gridDim.x) {
        const int64_t i = int64_t(c) * DEPTH_T + threadIdx.x;
        const uint32_t v = block_scan_1024(i < a.n_pos ? d[i] : 0u, DcPlus(), s_wave);
        if (i < a.n_pos) d[i] = v;
        if (threadIdx.x == DEPTH_T - 1) a.chunk[int64_t(blockIdx.y) * a.n_chunks + c] = v;
    }
}

// D3
__global__ __launch_bounds__(DEPTH_T) void depth_carry_kernel(const DepthArgs a)
{
    __shared__ uint32_t s_wave[16];
    uint32_t* d = a.depth[blockIdx.y];
    const uint32_t* tot = a.chunk + int64_t(blockIdx.y) * a.n_chunks;
    const bool refused = a.ctl[0] != 0;
    for (int32_t c = blockIdx.x; c < a.n_chunks; c += gridDim.x) {
        uint32_t part = 0;
        if (!refused)
            for (int32_t j = threadIdx.x; j < c; j += DEPTH_T) part += tot[j];
        const uint32_t carry = block_scan_1024(part, DcPlus(), s_wave); // (the last thread's is the sum of all)
        __shared__ uint32_t s_carry;
        if (threadIdx.x == DEPTH_T - 1) s_carry = carry;
        __syncthreads();
        const int64_t i = int64_t(c) * DEPTH_T + threadIdx.x;
        if (i < a.n_pos) d[i] = refused ? 0u : d[i] + s_carry;
        __syncthreads();
    }
}

struct DepthLayout
{
    size_t ctl, chunk, total;
    int32_t n_chunks;
};
DepthLayout depth_layout(const int32_t n_pos)
{
    DepthLayout l;
    l.n_chunks = int32_t((int64_t(n_pos) + DEPTH_T - 1) / DEPTH_T);
    l.ctl = 0;
    l.chunk = 256;
    l.total = l.chunk + sk_align256(sizeof(uint32_t) * 2 * size_t(l.n_chunks)) + 256; // (+ 256: the block is aligned here)
    return l;
}

// ---------------------------------------------------------------------------------------------------------------------------------

enum { CC_BAD = 0, CC_KEYS, CC_WORDS = 4 };
enum { RATE_INSERT = 0, RATE_DELETE, RATE_OTHER }; // IndelErrorRateType::index_t as getRateType gives it

struct CandSample
{
    int32_t n_reads;
    const int64_t* obs_off;
    const sk_intake_obs* obs;
    int64_t obs_cap;
    const uint32_t* depth1;
    const uint32_t* depth2;
};

struct CandArgs
{
    int32_t n_samples, n_sets; // the sets after the candidate set
    CandSample s[SK_MAX_SAMPLES];
    int32_t win_begin, n_pos;
    const sk_indel_table_key* keys;
    const sk_indel_table_sample_data* data;
    const int64_t* table_totals;
    int64_t key_cap;
    const sk_indel_rate_set* sets;
    sk_indel_candidate_options opt;
    sk_indel_candidate* out;
    sk_indel_error_rates* rates;
    int64_t* totals;
    int64_t* ctl; // [CC_WORDS]
    int exact_libm;
    unsigned* err;
};

__device__ __forceinline__ bool cc_rate_set_ok(const sk_indel_rate_set& rs)
{
    if (rs.n_sizes < 1 || rs.n_sizes > uint32_t(SK_RATE_MAX_SIZES)) return false;
    for (uint32_t i = 0; i < rs.n_sizes; ++i) {
        if (rs.n_counts[i] < 1 || rs.n_counts[i] > uint32_t(SK_RATE_MAX_COUNTS)) return false;
        for (uint32_t j = 0; j < rs.n_counts[i]; ++j)
            if (!(rs.insertion[i][j] >= 0. && rs.insertion[i][j] <= 1.) || !(rs.deletion[i][j] >= 0. && rs.deletion[i][j] <= 1.)) return false;
    }
    return true;
}

// C0
__global__ __launch_bounds__(CAND_T) void cand_check_kernel(const CandArgs a)
{
    const int64_t stride = int64_t(gridDim.x) * CAND_T;
    for (int64_t k = int64_t(blockIdx.x) * CAND_T + threadIdx.x; k < a.key_cap; k += stride) a.out[k] = sk_indel_candidate{ 0, 0, 0, 0 };
    if (blockIdx.x != 0) return;
    __shared__ int s_bad;
    if (threadIdx.x == 0) s_bad = 0;
    __syncthreads();
    bool bad = false;
    if (int(threadIdx.x) <= a.n_sets) bad = !cc_rate_set_ok(a.sets[threadIdx.x]);
    if (int(threadIdx.x) < a.n_samples) {
        const CandSample& sm = a.s[threadIdx.x];
        const int64_t n = sm.n_reads > 0 ? sm.obs_off[sm.n_reads] : 0;
        if (n < 0 || n > sm.obs_cap) bad = true;
    }
    const int64_t n_keys = a.table_totals[0];
    if (threadIdx.x == 0 && (n_keys < 0 || n_keys > a.key_cap)) bad = true;
    if (bad) s_bad = 1; // (every writer writes 1)
    __syncthreads();
    if (threadIdx.x == 0) {
        a.ctl[CC_BAD] = s_bad;
        a.ctl[CC_KEYS] = s_bad ? 0 : n_keys;
        a.totals[0] = 0;
        a.totals[1] = 0;
        if (s_bad) atomicOr(a.err, unsigned(SK_DEVERR_INDEL_CANDIDATES));
    }
}

// C1 -- rule B
__global__ __launch_bounds__(CAND_T) void cand_bp_kernel(const CandArgs a)
{
    if (a.ctl[CC_BAD]) return;
    const CandSample& sm = a.s[blockIdx.y];
    const int64_t n_obs = sm.n_reads > 0 ? sm.obs_off[sm.n_reads] : 0;
    const int64_t n_keys = a.ctl[CC_KEYS];
    const int64_t stride = int64_t(gridDim.x) * CAND_T;
    for (int64_t j = int64_t(blockIdx.x) * CAND_T + threadIdx.x; j < n_obs; j += stride) {
        const sk_intake_obs o = sm.obs[j];
        if (o.type != SK_INDEL_BP_LEFT && o.type != SK_INDEL_BP_RIGHT) continue;
        int64_t lo = 0, hi = n_keys; // the first key not before (pos, type): all breakpoint observations of one (pos, type) are one key
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            const int32_t kp = a.keys[mid].pos, kt = a.keys[mid].type;
            if (kp < o.pos || (kp == o.pos && kt < int32_t(o.type))) lo = mid + 1;
            else hi = mid;
        }
        if (lo < n_keys && a.keys[lo].pos == o.pos && a.keys[lo].type == int32_t(o.type)) atomicMax(&a.out[lo].bp_insert_size, o.bp_len);
        else atomicOr(a.err, unsigned(SK_DEVERR_INDEL_CANDIDATES)), a.ctl[CC_BAD] = 1; // (C2 runs after this kernel and zeroes everything)
    }
}

// IndelErrorRateSet::getRate
__device__ __forceinline__ double cc_get_rate(const sk_indel_rate_set& rs, uint32_t size, uint32_t count, const int type)
{
    if (size > rs.n_sizes) { // revert back to baseline if the repeating pattern size isn't represented
        size = 1;
        count = 1;
    }
    const uint32_t si = min(size - 1, rs.n_sizes - 1);
    const uint32_t ci = min(count - 1, rs.n_counts[si] - 1);
    return type == RATE_DELETE ? rs.deletion[si][ci] : rs.insertion[si][ci];
}

// IndelErrorModel::getIndelErrorRate
__device__ __forceinline__ void cc_error_rate(const sk_indel_rate_set& rs, const sk_indel_table_key& key, const int type, double& ref_to_indel, double& indel_to_ref)
{
    if (type == RATE_OTHER) {
        const double ins = cc_get_rate(rs, 1, 1, RATE_INSERT), del = cc_get_rate(rs, 1, 1, RATE_DELETE);
        ref_to_indel = ins < del ? del : ins; // std::max(ins, del)
        indel_to_ref = ref_to_indel;
        return;
    }
    const uint32_t size = max(key.repeat_unit_len, 1u), ref_count = max(key.ref_repeat_count, 1u), indel_count = max(key.indel_repeat_count, 1u);
    ref_to_indel = cc_get_rate(rs, size, ref_count, type);
    indel_to_ref = cc_get_rate(rs, size, indel_count, type == RATE_DELETE ? RATE_INSERT : RATE_DELETE);
}

// scaleIndelErrorRate with softMaxInverseTransform and softMaxTransform over [0, 0.5]
__device__ __forceinline__ double cc_scale_rate(double rate, const double log_factor, const int ex, const SkLibmTables& lt)
{
    const double lo = 0.0, hi = 0.5, range = hi - lo;
    rate = hi < rate ? hi : rate; // std::min(rate, maxIndelErrorProb)
    const double ranged = (rate - lo) / range;
    double real;
    if (ranged <= 0.5) real = sk_log(ranged / (1 - ranged), ex, lt);
    else real = -sk_log((1 - ranged) / ranged, ex, lt);
    real += log_factor;
    double t;
    if (real <= 0.) {
        const double er = sk_exp(real, ex, lt);
        t = er / (1. + er);
    } else {
        const double enr = sk_exp(-real, ex, lt);
        t = 1. / (enr + 1.);
    }
    return t * range + lo;
}

__device__ __forceinline__ uint32_t cc_depth(const uint32_t* d, const int64_t at, const CandArgs& a)
{
    const int64_t i = at - a.win_begin;
    return (d && i >= 0 && i < a.n_pos) ? d[i] : 0u;
}

enum { RN_FALSE = 0, RN_TRUE, RN_EXACT };
// min_count_binom_gte_cache::isRejectNull; RN_EXACT where it goes on to min_count_binomial_gte_exact
__device__ __forceinline__ int cc_is_reject_null(const uint32_t n, const double p, const uint32_t n_success, const double* papprox)
{
    if (p <= 0.) return n_success > 0 ? RN_TRUE : RN_FALSE;
    if (n_success == 0) return RN_FALSE;
    if (p / (1 - p) <= 0.01) { // isPoissonApprox
        const double np = n * p;
        if (np < papprox[SK_ICAND_PAPPROX - 1]) return np < papprox[min(n_success, uint32_t(SK_ICAND_PAPPROX)) - 1] ? RN_TRUE : RN_FALSE;
    }
    return RN_EXACT;
}

// rule C -> is_candidate; undecided: the reason
__device__ __forceinline__ bool cc_is_candidate(const CandArgs& a, const sk_indel_table_key& key, const sk_indel_table_sample_data* data, const sk_indel_error_rates* rates,
                                                const uint32_t bp_size, int& undecided)
{
    undecided = SK_ICAND_DECIDED;
    if (key.flags & SK_ITAB_DO_NOT_GENOTYPE) return false; // C1
    if (key.flags & SK_ITAB_AR_PENDING) {
        undecided = SK_ICAND_AR_PENDING;
        return false;
    }
    if (a.opt.is_haplotyping_enabled && key.active_region_id < 0) return false; // C2
    const int64_t depth_pos = int64_t(key.pos) - 1;
    bool signal = false; // C3
    for (int s = 0; s < a.n_samples && !signal; ++s) {
        const uint32_t n1 = data[s].count[SK_ITAB_TIER1];
        if (!a.opt.is_candidate_indel_signal_test) {
            signal = n1 >= 1;
            continue;
        }
        const uint32_t depth = cc_depth(a.s[s].depth1, depth_pos, a);
        const uint32_t total = depth < n1 ? n1 : depth;
        if (total < 2) continue;
        const int r = cc_is_reject_null(total, rates[s].candidate_indel_to_ref, n1, a.opt.papprox);
        if (r == RN_EXACT) {
            undecided = SK_ICAND_EXACT_BINOMIAL;
            return false;
        }
        signal = r == RN_TRUE;
    }
    if (!signal) return false;
    if (key.type == SK_INDEL_BP_LEFT || key.type == SK_INDEL_BP_RIGHT) { // C4
        if (a.opt.min_candidate_indel_open_length > bp_size) return false;
        if (key.n_bp_obs > uint32_t(SK_ICAND_MAX_BP_OBS)) {
            undecided = SK_ICAND_BP_OBS_ORDER;
            return false;
        }
    }
    if (a.opt.max_candidate_depth > 0.) { // C5
        double sum = 0;
        for (int s = 0; s < a.n_samples; ++s) {
            if (!a.opt.is_count_towards_depth_filter[s]) continue;
            const uint32_t d1 = cc_depth(a.s[s].depth1, depth_pos, a), d2 = cc_depth(a.s[s].depth2, depth_pos, a);
            sum += double(d1 + d2); // (unsigned + unsigned, then to double, as the reference adds)
        }
        if (sum > a.opt.max_candidate_depth) return false;
    }
    return true;
}

// C2 -- rules E and C
__global__ __launch_bounds__(CAND_T) void cand_key_kernel(const CandArgs a)
{
    const SkLibmTables lt = sk_libm_tables_default();
    const bool bad = a.ctl[CC_BAD] != 0;
    const int64_t n_keys = bad ? 0 : a.ctl[CC_KEYS];
    const int64_t stride = int64_t(gridDim.x) * CAND_T;
    unsigned n_cand = 0, n_undecided = 0;
    for (int64_t k = int64_t(blockIdx.x) * CAND_T + threadIdx.x; k < a.key_cap; k += stride) {
        sk_indel_error_rates* rates = a.rates + k * a.n_samples;
        if (k >= n_keys) {
            a.out[k] = sk_indel_candidate{ 0, 0, 0, 0 };
            for (int s = 0; s < a.n_samples; ++s) rates[s] = sk_indel_error_rates{ 0., 0., 0., 0. };
            continue;
        }
        const sk_indel_table_key key = a.keys[k];
        const int type = (key.type == SK_INDEL_INDEL && key.ins_len == 0 && key.del_len > 0)   ? RATE_DELETE  // getRateType
                         : (key.type == SK_INDEL_INDEL && key.ins_len > 0 && key.del_len == 0) ? RATE_INSERT
                                                                                               : RATE_OTHER;
        for (int s = 0; s < a.n_samples; ++s) { // rule E
            sk_indel_error_rates r;
            cc_error_rate(a.sets[1 + (a.n_sets > 1 ? s : 0)], key, type, r.ref_to_indel, r.indel_to_ref);
            if (a.opt.is_indel_ref_error_factor) r.indel_to_ref = cc_scale_rate(r.indel_to_ref, a.opt.log_indel_ref_error_factor, a.exact_libm, lt);
            cc_error_rate(a.sets[0], key, type, r.candidate_ref_to_indel, r.candidate_indel_to_ref);
            rates[s] = r;
        }
        const uint32_t bp_size = a.out[k].bp_insert_size;
        int undecided;
        const bool cand = cc_is_candidate(a, key, a.data + k * a.n_samples, rates, bp_size, undecided);
        a.out[k] = sk_indel_candidate{ uint8_t(cand ? 1 : 0), uint8_t(undecided), 0, bp_size };
        n_cand += cand ? 1u : 0u;
        n_undecided += undecided ? 1u : 0u;
    }
    if (n_cand) atomicAdd(reinterpret_cast<unsigned long long*>(a.totals), static_cast<unsigned long long>(n_cand));
    if (n_undecided) atomicAdd(reinterpret_cast<unsigned long long*>(a.totals + 1), static_cast<unsigned long long>(n_undecided));
}

const char* cand_options_issue(const int32_t n_samples, const sk_indel_candidate_options* opt)
{
    if (n_samples < 1 || n_samples > SK_MAX_SAMPLES) return "n_samples must be in 1..SK_MAX_SAMPLES";
    if (!opt) return "null argument";
    for (int i = 0; i + 1 < SK_ICAND_PAPPROX; ++i)
        if (!(opt->papprox[i] < opt->papprox[i + 1])) return "papprox is not ascending";
    return nullptr;
}

const char* cand_rate_set_issue(const sk_indel_rate_set& rs)
{
    if (rs.n_sizes < 1 || rs.n_sizes > uint32_t(SK_RATE_MAX_SIZES)) return "a rate set of no or more than SK_RATE_MAX_SIZES sizes";
    for (uint32_t i = 0; i < rs.n_sizes; ++i) {
        if (rs.n_counts[i] < 1 || rs.n_counts[i] > uint32_t(SK_RATE_MAX_COUNTS)) return "a rate set with a count outside 1..SK_RATE_MAX_COUNTS";
        for (uint32_t j = 0; j < rs.n_counts[i]; ++j)
            if (!(rs.insertion[i][j] >= 0. && rs.insertion[i][j] <= 1.) || !(rs.deletion[i][j] >= 0. && rs.deletion[i][j] <= 1.)) return "a rate outside [0, 1]";
    }
    return nullptr;
}

} // namespace

extern "C" {

void sk_indel_candidate_options_default(sk_indel_candidate_options* o)
{
    if (!o) return;
    std::memset(o, 0, sizeof(*o));
    // (papprox stays zero: caller data, and the entries refuse it until the caller has filled it in)
    o->log_indel_ref_error_factor = 0.0; // std::log(1.)
    o->max_candidate_depth = -1.0;
    o->min_candidate_indel_open_length = 20;
    o->is_candidate_indel_signal_test = 1;
    for (int s = 0; s < SK_MAX_SAMPLES; ++s) o->is_count_towards_depth_filter[s] = 1;
}

size_t sk_read_depth_scratch_bytes(int32_t n_pos)
{
    if (n_pos < 0) return 0;
    return depth_layout(n_pos).total;
}

int sk_read_depth_dev(int32_t n_reads, const int64_t* dev_path_off, const int32_t* dev_n_seg, const sk_path_seg* dev_path, int64_t path_cap,
                      const int32_t* dev_pos, const uint8_t* dev_iat, int32_t win_begin, int32_t n_pos, uint32_t* dev_depth1, uint32_t* dev_depth2,
                      void* dev_scratch, size_t scratch_bytes, void* hip_stream)
{
    if (n_reads < 0 || n_pos < 0 || path_cap < 0) return sk_fail("sk_read_depth_dev: negative size");
    if ((n_reads > 0 && (!dev_path_off || !dev_n_seg || !dev_pos || !dev_iat)) || (path_cap > 0 && !dev_path) || (n_pos > 0 && (!dev_depth1 || !dev_depth2)))
        return sk_fail("sk_read_depth_dev: null argument");
    if (!dev_scratch || scratch_bytes < sk_read_depth_scratch_bytes(n_pos)) return sk_fail("sk_read_depth_dev: scratch is below sk_read_depth_scratch_bytes");
    SK_REQUIRE_INIT();
    skrt::wakeHint();
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    const DepthLayout lay = depth_layout(n_pos);
    char* scratch = static_cast<char*>(dev_scratch);
    scratch += (256 - (reinterpret_cast<uintptr_t>(scratch) & 255)) & 255;
    DepthArgs a;
    std::memset(&a, 0, sizeof(a));
    a.n_reads = n_reads;
    a.path_off = dev_path_off;
    a.n_seg = dev_n_seg;
    a.path = dev_path;
    a.path_cap = path_cap;
    a.pos = dev_pos;
    a.iat = dev_iat;
    a.win_begin = win_begin;
    a.n_pos = n_pos;
    a.depth[0] = dev_depth1;
    a.depth[1] = dev_depth2;
    a.ctl = reinterpret_cast<uint32_t*>(scratch + lay.ctl);
    a.chunk = reinterpret_cast<uint32_t*>(scratch + lay.chunk);
    a.n_chunks = lay.n_chunks;
    a.err = sk_ctx().dev_error_flags;
    const unsigned pos_grid = unsigned(lay.n_chunks < 1 ? 1 : (lay.n_chunks < 1024 ? lay.n_chunks : 1024));
    const int64_t read_blocks = (int64_t(n_reads) + DEPTH_T - 1) / DEPTH_T;
    SK_LAUNCH(depth_clear_kernel, dim3(pos_grid), dim3(DEPTH_T), 0, st, a);
    if (n_reads > 0) SK_LAUNCH(depth_ends_kernel, dim3(unsigned(read_blocks < 1024 ? read_blocks : 1024)), dim3(DEPTH_T), 0, st, a);
    if (n_pos > 0) {
        SK_LAUNCH(depth_scan_kernel, dim3(pos_grid, 2), dim3(DEPTH_T), 0, st, a);
        SK_LAUNCH(depth_carry_kernel, dim3(pos_grid, 2), dim3(DEPTH_T), 0, st, a);
    }
    SK_HIP(skrt::getLastError());
    return 0;
}

int sk_read_depth(int32_t n_reads, const int64_t* path_off, const int32_t* n_seg, const sk_path_seg* path, int64_t path_cap, const int32_t* pos,
                  const uint8_t* iat, int32_t win_begin, int32_t n_pos, uint32_t* depth1, uint32_t* depth2)
{
    if (n_reads < 0 || n_pos < 0 || path_cap < 0) return sk_fail("sk_read_depth: negative size");
    if ((n_reads > 0 && (!path_off || !n_seg || !pos || !iat)) || (path_cap > 0 && !path) || (n_pos > 0 && (!depth1 || !depth2))) return sk_fail("sk_read_depth: null argument");
    for (int32_t r = 0; r < n_reads; ++r) {
        const std::string where = "sk_read_depth: read " + std::to_string(r) + ": ";
        if (iat[r] > SK_IAT_SUBMAP) return sk_fail(where + "an iat above 2");
        if (n_seg[r] < 0) return sk_fail(where + "a negative n_seg");
        if (path_off[r] < 0 || path_off[r] > path_cap || int64_t(n_seg[r]) > path_cap - path_off[r]) return sk_fail(where + "the path lies outside path_cap");
        for (int32_t k = 0; k < n_seg[r]; ++k)
            if (path[path_off[r] + k].type > uint32_t(SK_SEG_SEQ_MISMATCH)) return sk_fail(where + "a segment type above SK_SEG_SEQ_MISMATCH");
    }
    SK_REQUIRE_INIT();
    skrt::wakeHint();
    SkContext& ctx = sk_ctx();
    SK_HIP(skrt::setDevice(ctx.device));
    hipStream_t st = ctx.stream;
    const size_t nr = size_t(n_reads), np = size_t(n_pos);
    const size_t scratch_bytes = sk_read_depth_scratch_bytes(n_pos);
    struct
    {
        int64_t* path_off; int32_t* n_seg; sk_path_seg* path; int32_t* pos; uint8_t* iat; uint32_t* d1; uint32_t* d2; char* scratch;
    } d;
    int rc = 0;
    if (sk_carve(d, [&](SkArena& ar) {
            decltype(d) o{};
            o.path_off = ar.up(path_off, nr, 1, st, rc);
            o.n_seg = ar.up(n_seg, nr, 1, st, rc);
            o.path = ar.up(path, size_t(path_cap), 1, st, rc);
            o.pos = ar.up(pos, nr, 1, st, rc);
            o.iat = ar.up(iat, nr, 16, st, rc);
            o.d1 = ar.take<uint32_t>(np + 1);
            o.d2 = ar.take<uint32_t>(np + 1);
            o.scratch = ar.take<char>(scratch_bytes + 16);
            return o;
        }) || rc)
        return 1;
    if (sk_read_depth_dev(n_reads, d.path_off, d.n_seg, d.path, path_cap, d.pos, d.iat, win_begin, n_pos, d.d1, d.d2, d.scratch, scratch_bytes + 16, st)) return 1;
    if (n_pos > 0) {
        SK_HIP(skrt::memcpyAsync(depth1, d.d1, sizeof(uint32_t) * np, hipMemcpyDeviceToHost, st));
        SK_HIP(skrt::memcpyAsync(depth2, d.d2, sizeof(uint32_t) * np, hipMemcpyDeviceToHost, st));
    }
    SK_HIP(skrt::streamSynchronize(st));
    if (sk_check_device_errors()) return 1;
    return 0;
}

size_t sk_indel_candidates_scratch_bytes(void) { return 512; } // the control words, and room to align them

int sk_indel_candidates_dev(int32_t n_samples, const sk_indel_candidate_sample* samples, int32_t win_begin, int32_t n_pos, const sk_indel_table_key* dev_keys,
                            const sk_indel_table_sample_data* dev_data, const int64_t* dev_table_totals, int64_t key_cap, const sk_indel_rate_set* dev_rate_sets,
                            const sk_indel_candidate_options* opt, sk_indel_candidate* dev_out, sk_indel_error_rates* dev_rates, int64_t* dev_totals,
                            void* dev_scratch, size_t scratch_bytes, void* hip_stream)
{
    if (const char* issue = cand_options_issue(n_samples, opt)) return sk_fail(std::string("sk_indel_candidates_dev: ") + issue);
    if (n_pos < 0 || key_cap < 0) return sk_fail("sk_indel_candidates_dev: negative size");
    if (!samples || !dev_table_totals || !dev_rate_sets || !dev_totals || (key_cap > 0 && (!dev_keys || !dev_data || !dev_out || !dev_rates)))
        return sk_fail("sk_indel_candidates_dev: null argument");
    int64_t obs_cap_max = 0;
    for (int s = 0; s < n_samples; ++s) {
        const sk_indel_candidate_sample& sm = samples[s];
        if (sm.n_reads < 0 || sm.obs_cap < 0) return sk_fail("sk_indel_candidates_dev: negative size");
        if ((sm.n_reads > 0 && !sm.obs_off) || (sm.obs_cap > 0 && !sm.obs) || (n_pos > 0 && (!sm.depth1 || !sm.depth2))) return sk_fail("sk_indel_candidates_dev: null argument");
        if (sm.n_reads > 0 && sm.obs_cap > obs_cap_max) obs_cap_max = sm.obs_cap;
    }
    if (!dev_scratch || scratch_bytes < sk_indel_candidates_scratch_bytes()) return sk_fail("sk_indel_candidates_dev: scratch is below sk_indel_candidates_scratch_bytes");
    SK_REQUIRE_INIT();
    skrt::wakeHint();
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    char* scratch = static_cast<char*>(dev_scratch);
    scratch += (256 - (reinterpret_cast<uintptr_t>(scratch) & 255)) & 255;
    CandArgs a;
    std::memset(&a, 0, sizeof(a));
    a.n_samples = n_samples;
    a.n_sets = opt->is_sample_specific_rates ? n_samples : 1;
    for (int s = 0; s < n_samples; ++s) a.s[s] = CandSample{ samples[s].n_reads, samples[s].obs_off, samples[s].obs, samples[s].obs_cap, samples[s].depth1, samples[s].depth2 };
    a.win_begin = win_begin;
    a.n_pos = n_pos;
    a.keys = dev_keys;
    a.data = dev_data;
    a.table_totals = dev_table_totals;
    a.key_cap = key_cap;
    a.sets = dev_rate_sets;
    a.opt = *opt;
    a.out = dev_out;
    a.rates = dev_rates;
    a.totals = dev_totals;
    a.ctl = reinterpret_cast<int64_t*>(scratch);
    a.exact_libm = sk_ctx().libm_restated ? 1 : 0;
    a.err = sk_ctx().dev_error_flags;
    const int64_t key_blocks = (key_cap + CAND_T - 1) / CAND_T;
    const unsigned key_grid = unsigned(key_blocks < 1 ? 1 : (key_blocks < CAND_GRID ? key_blocks : int64_t(CAND_GRID)));
    SK_LAUNCH(cand_check_kernel, dim3(key_grid), dim3(CAND_T), 0, st, a);
    if (obs_cap_max > 0 && key_cap > 0) {
        const int64_t obs_blocks = (obs_cap_max + CAND_T - 1) / CAND_T;
        SK_LAUNCH(cand_bp_kernel, dim3(unsigned(obs_blocks < CAND_GRID ? obs_blocks : int64_t(CAND_GRID)), unsigned(n_samples)), dim3(CAND_T), 0, st, a);
    }
    if (key_cap > 0) SK_LAUNCH(cand_key_kernel, dim3(key_grid), dim3(CAND_T), 0, st, a);
    SK_HIP(skrt::getLastError());
    return 0;
}

int sk_indel_candidates(int32_t n_samples, const sk_indel_candidate_sample* samples, int32_t win_begin, int32_t n_pos, const sk_indel_table_key* keys,
                        const sk_indel_table_sample_data* data, int64_t n_keys, const sk_indel_rate_set* rate_sets, const sk_indel_candidate_options* opt,
                        sk_indel_candidate* out, sk_indel_error_rates* rates, int64_t* totals)
{
    if (const char* issue = cand_options_issue(n_samples, opt)) return sk_fail(std::string("sk_indel_candidates: ") + issue);
    if (n_pos < 0 || n_keys < 0) return sk_fail("sk_indel_candidates: negative size");
    if (!samples || !rate_sets || !totals || (n_keys > 0 && (!keys || !data || !out || !rates))) return sk_fail("sk_indel_candidates: null argument");
    const int n_sets = 1 + (opt->is_sample_specific_rates ? n_samples : 1);
    for (int i = 0; i < n_sets; ++i)
        if (const char* issue = cand_rate_set_issue(rate_sets[i])) return sk_fail("sk_indel_candidates: rate set " + std::to_string(i) + ": " + issue);
    int64_t n_obs[SK_MAX_SAMPLES];
    for (int s = 0; s < n_samples; ++s) {
        const sk_indel_candidate_sample& sm = samples[s];
        const std::string where = "sk_indel_candidates: sample " + std::to_string(s) + ": ";
        if (sm.n_reads < 0 || sm.obs_cap < 0) return sk_fail(where + "negative size");
        if ((sm.n_reads > 0 && !sm.obs_off) || (n_pos > 0 && (!sm.depth1 || !sm.depth2))) return sk_fail(where + "null argument");
        n_obs[s] = sm.n_reads > 0 ? sm.obs_off[sm.n_reads] : 0;
        if (n_obs[s] < 0 || n_obs[s] > sm.obs_cap) return sk_fail(where + "the observations lie outside obs_cap");
        if (n_obs[s] > 0 && !sm.obs) return sk_fail(where + "null argument");
        for (int64_t j = 0; j < n_obs[s]; ++j) { // rule B's search, for the message
            const sk_intake_obs& o = sm.obs[j];
            if (o.type != SK_INDEL_BP_LEFT && o.type != SK_INDEL_BP_RIGHT) continue;
            int64_t lo = 0, hi = n_keys;
            while (lo < hi) {
                const int64_t mid = (lo + hi) >> 1;
                if (keys[mid].pos < o.pos || (keys[mid].pos == o.pos && keys[mid].type < int32_t(o.type))) lo = mid + 1;
                else hi = mid;
            }
            if (!(lo < n_keys && keys[lo].pos == o.pos && keys[lo].type == int32_t(o.type))) return sk_fail(where + "observation " + std::to_string(j) + ": a breakpoint observation whose key the table lacks");
        }
    }
    SK_REQUIRE_INIT();
    skrt::wakeHint();
    SkContext& ctx = sk_ctx();
    SK_HIP(skrt::setDevice(ctx.device));
    hipStream_t st = ctx.stream;
    const size_t nk = size_t(n_keys), np = size_t(n_pos), ns = size_t(n_samples);
    const size_t scratch_bytes = sk_indel_candidates_scratch_bytes();
    struct
    {
        sk_indel_candidate_sample s[SK_MAX_SAMPLES];
        sk_indel_table_key* keys; sk_indel_table_sample_data* data; int64_t* n_keys; sk_indel_rate_set* sets; sk_indel_candidate* out; sk_indel_error_rates* rates;
        int64_t* totals; char* scratch;
    } d;
    int rc = 0;
    if (sk_carve(d, [&](SkArena& ar) {
            decltype(d) o{};
            for (int s = 0; s < n_samples; ++s) {
                const sk_indel_candidate_sample& sm = samples[s];
                sk_indel_candidate_sample t = sm;
                t.obs_off = ar.up(sm.obs_off, sm.n_reads > 0 ? size_t(sm.n_reads) + 1 : 0, 1, st, rc);
                t.obs = ar.up(sm.obs, size_t(n_obs[s]), 1, st, rc);
                t.obs_cap = n_obs[s];
                t.depth1 = ar.up(sm.depth1, np, 1, st, rc);
                t.depth2 = ar.up(sm.depth2, np, 1, st, rc);
                o.s[s] = t;
            }
            o.keys = ar.up(keys, nk, 1, st, rc);
            o.data = ar.up(data, nk * ns, 1, st, rc);
            o.n_keys = ar.up(&n_keys, 1, 0, st, rc);
            o.sets = ar.up(rate_sets, size_t(n_sets), 0, st, rc);
            o.out = ar.take<sk_indel_candidate>(nk + 1);
            o.rates = ar.take<sk_indel_error_rates>(nk * ns + 1);
            o.totals = ar.take<int64_t>(2);
            o.scratch = ar.take<char>(scratch_bytes + 16);
            return o;
        }) || rc)
        return 1;
    if (sk_indel_candidates_dev(n_samples, d.s, win_begin, n_pos, d.keys, d.data, d.n_keys, n_keys, d.sets, opt, d.out, d.rates, d.totals, d.scratch, scratch_bytes + 16, st)) return 1;
    int64_t t[2] = { 0, 0 };
    SK_HIP(skrt::memcpyAsync(t, d.totals, sizeof(t), hipMemcpyDeviceToHost, st));
    if (n_keys > 0) {
        SK_HIP(skrt::memcpyAsync(out, d.out, sizeof(sk_indel_candidate) * nk, hipMemcpyDeviceToHost, st));
        SK_HIP(skrt::memcpyAsync(rates, d.rates, sizeof(sk_indel_error_rates) * nk * ns, hipMemcpyDeviceToHost, st));
    }
    SK_HIP(skrt::streamSynchronize(st));
    if (sk_check_device_errors()) return 1;
    totals[0] = t[0];
    totals[1] = t[1];
    return 0;
}

} // extern "C"
