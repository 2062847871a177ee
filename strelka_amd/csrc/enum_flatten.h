// enum_flatten.h -- a section of read_enumerate.hip: the flattening both chains share (FlatArgs, code_of and its host table, L1 the
// pools' layout, flatten_cal) and the staged chain's L2, F1 and F2.  F3 follows F5 in the unit: enum_entries.h.
// Part of that one translation unit (after enum_search.h), not a reusable interface.
#pragma once

#include "sk_common.h"

#include "align_entry.h"
#include "enum_search.h"
#include "read_enumerate.h"

#include <cstring>

namespace
{

// ---------------------------------------------------------------------------------------------------------------------
// flattening

__device__ inline uint8_t code_of(const char c) // get_bam_seq_code, L/htsapi/bam_seq.hh:73-92
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
// ---- host (plan_job; F5_CODE_PAD is also what FlatArgs::ref_code and F5's window rely on).  The same on the host, as a table: the job's code images (FlatArgs::ref_code, ins_code) are made with it
constexpr int F5_CODE_PAD = 1024; // bytes of SK_BAM_ANY on either side of the reference's codes
struct CodeLut
{
    uint8_t code[256];
    CodeLut()
    {
        std::memset(code, SK_BAM_ANY, sizeof(code));
        code[uint8_t('=')] = SK_BAM_REF;
        code[uint8_t('A')] = SK_BAM_A;
        code[uint8_t('C')] = SK_BAM_C;
        code[uint8_t('G')] = SK_BAM_G;
        code[uint8_t('T')] = SK_BAM_T;
    }
};
inline const CodeLut& code_lut()
{
    static const CodeLut l;
    return l;
}

struct FlatArgs
{
    PJob job;
    const char* ins_pool;
    const char* ref;
    // the job's code images (F5 reads these; the staged chain keeps reading the characters): code_of() of every reference character
    // with F5_CODE_PAD bytes of SK_BAM_ANY before and after it (ref_code points at the reference's first base: a window that leaves
    // the reference reads pad), and of every character of the insert pool
    const uint8_t* ref_code;
    const uint8_t* ins_code;
    int32_t ref_offset, ref_len;
    int32_t n_reads, n_cals;
    const PCal* pool;
    const int32_t* list; // [n_cals] leaf slots, each read's in set order
    int32_t* status;
    const int64_t* read_off;
    const uint8_t* read_code;
    const int32_t* cal_off;
    // per-read layout of the haplotype pool (L1 out)
    int32_t* win_begin; // (L1a: min over the read's candidate alignments, cells start at INT_MAX)
    int32_t* win_end;   // (cells start at INT_MIN)
    int32_t* ins_lo;    // lowest / highest table index of an indel with an insert sequence
    int32_t* ins_hi;
    uint8_t* n_seg8;    // [n_cals] path segments of each candidate alignment (capped at 255), set order: F5 orders a read's alignments by it
    int32_t* win_len;
    int32_t* hap_len;
    int32_t* n_ins;
    int16_t* ins_idx; // [n_reads][INS_CAP] table indices whose insert sequence is in the pool
    int32_t* ins_off; // [n_reads][INS_CAP] where
    // per candidate alignment
    int32_t* n_ops; // (L2 out)
    const int64_t* hap_off;
    PCal* cals;
    uint8_t* hap_code;
    const int64_t* op_off; // [n_cals + 1]
    sk_score_op* ops;
    uint32_t* entries;
    uint32_t* evmask;
    int32_t evmask_words, max_read_len;
    // the column form (strelka_amd.h, sk_align_batch::colmat)
    uint8_t* colmat; // (bytes of the words; pre-filled with the 0.0 column)
    const int64_t* colmat_off;
    uint32_t* addmask;
    int32_t* ref_outside;     // counts the window bytes that lie outside the job's reference segment (they read as N)
    int32_t n_cals_on_device; // the job runs as one fixed sequence: the number of candidate alignments is cal_off[n_reads], the host has not seen it
};
enum { INS_CAP = Caps::K + 2 };

__device__ inline int read_of_cal(const FlatArgs& a, const int c) // last r with cal_off[r] <= c
{
    int lo = 0, hi = a.n_reads;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (a.cal_off[mid] <= c) lo = mid; else hi = mid;
    }
    return lo;
}

// L1: the layout of each read's haplotype pool -- its reference window (the union of the reference spans of the match segments
// of all its candidate alignments), then the insert sequences of the table indels between the lowest and the highest one any of
// its candidate alignments holds, in table order.  (The host builder appends the insert sequences its ops use in order of first
// use and shares equal sequences; the layout is private to the read's batch entry and the scores do not depend on it.)
//   L1a  one thread per candidate alignment: window and indel-index bounds into the read's cells (atomicMin / atomicMax)
//   L1b  one thread per read: offsets
__global__ __launch_bounds__(256) void pool_bounds_kernel(const FlatArgs a)
{
    const int n_cals = a.n_cals_on_device ? a.cal_off[a.n_reads] : a.n_cals;
    for (int c = blockIdx.x * blockDim.x + threadIdx.x; c < n_cals; c += gridDim.x * blockDim.x) {
    const int r = read_of_cal(a, c);
    const PCal& cal = a.pool[a.list[c]];
    a.n_seg8[c] = uint8_t(min(int(cal.n_seg), 255));
    int32_t wb = INT_MAX, we = INT_MIN, pos = cal.pos;
    for (int i = 0; i < cal.n_seg; ++i) {
        const PSeg s = cal.path[i];
        if (seg_align_match(s.type)) {
            wb = min(wb, pos);
            we = max(we, pos + int32_t(s.length));
            pos += int32_t(s.length);
        } else if (s.type == SK_SEG_DELETE || s.type == SK_SEG_SKIP) {
            pos += int32_t(s.length);
        }
    }
    if (wb <= we) {
        atomicMin(&a.win_begin[r], wb);
        atomicMax(&a.win_end[r], we);
    }
    int lo = INT_MAX, hi = INT_MIN;
    auto add = [&](const int t) {
        if (t < 0 || a.job.tab[t].ins_len == 0) return;
        lo = min(lo, t);
        hi = max(hi, t);
    };
    for (int i = 0; i < cal.n_indels; ++i) add(cal.indels[i]);
    add(cal.lead);
    add(cal.trail);
    if (lo <= hi) {
        atomicMin(&a.ins_lo[r], lo);
        atomicMax(&a.ins_hi[r], hi);
    }
    }
}

__global__ __launch_bounds__(64) void pool_layout_kernel(const FlatArgs a)
{
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= a.n_reads) return;
    const int nc = a.cal_off[r + 1] - a.cal_off[r];
    a.n_ins[r] = 0;
    a.win_len[r] = 0;
    a.hap_len[r] = 0;
    if (nc == 0) return;
    int32_t wb = a.win_begin[r], we = a.win_end[r];
    if (wb > we) wb = we = 0;
    a.win_begin[r] = wb;
    int32_t len = we - wb;
    a.win_len[r] = len;
    int16_t* idx = a.ins_idx + size_t(r) * INS_CAP;
    int32_t* off = a.ins_off + size_t(r) * INS_CAP;
    int n = 0;
    for (int t = a.ins_lo[r]; t <= a.ins_hi[r]; ++t) {
        const uint32_t il = a.job.tab[t].ins_len;
        if (il == 0) continue;
        if (n >= INS_CAP) { // more insert sequences than this form holds: the host flattens this read
            a.status[r] = ST_OVERFLOW;
            n = 0;
            break;
        }
        idx[n] = int16_t(t);
        off[n] = len;
        len += int32_t(il);
        ++n;
    }
    a.n_ins[r] = n;
    a.hap_len[r] = max(len, 1);
}

// getMatchingIndelKey, starling_read_align_score.cpp:177-228: table index, -1 = no key, -2 = inconsistent
__device__ int matching_indel(const PJob& j, const PCal& c, const int32_t ref_head_pos, const unsigned del_len, const unsigned ins_len,
                              const int ends_first, const int ends_second, const int path_index)
{
    if (path_index < ends_first) return c.lead;
    if (path_index > ends_second) return c.trail;
    int found = -1;
    for (int k = 0; k < c.n_indels; ++k) {
        const PIndel& ci = j.tab[c.indels[k]];
        if (ci.pos == ref_head_pos && (ci.type == SK_INDEL_INDEL || ci.type == SK_INDEL_MISMATCH) && ci.del == del_len &&
            ci.ins_len == ins_len) {
            if (found >= 0) return -2;
            found = c.indels[k];
        } else if (ci.pos > ref_head_pos) {
            break;
        }
    }
    return found >= 0 ? found : -2;
}

// one candidate alignment -> ops (the walk of scoreCandidateAlignment :286-493 as host/align_flatten.cpp states it); returns the
// op count, -1 = leave this read to the host (it throws the reference's error, or handles what this form does not hold).
// WRITE = false only counts.
struct NoOpSink
{
    __device__ __forceinline__ void operator()(uint8_t, uint32_t, int32_t, bool) const {}
};

// SINK: called for every op in path order (kind, length, source offset, non-candidate penalty) -- the fused flatten + score kernel
// (F5) scores the op on the spot instead of storing it
template <bool WRITE, typename SINK = NoOpSink>
__device__ int flatten_cal(const FlatArgs& a, const int r, const PCal& c, const int32_t read_len, sk_score_op* ops, SINK&& sink = SINK())
{
    const int aps = c.n_seg;
    const int32_t win_begin = a.win_begin[r];
    const int n_ins = a.n_ins[r];
    const int16_t* ins_idx = a.ins_idx + size_t(r) * INS_CAP;
    const int32_t* ins_off = a.ins_off + size_t(r) * INS_CAP;
    unsigned read_offset = 0;
    int32_t ref_head_pos = c.pos;
    int ends_first = aps, ends_second = aps; // get_match_edge_segments, align_path.cpp:735-752
    {
        bool is_first_match = false;
        for (int i = 0; i < aps; ++i)
            if (seg_align_match(c.path[i].type)) {
                if (!is_first_match) ends_first = i;
                is_first_match = true;
                ends_second = i;
            }
    }
    int n = 0;
    auto emit = [&](const uint8_t kind, const uint32_t len, const int32_t src, const bool penalty) {
        if (kind == SK_OP_NOBASE && !penalty) return;
        sink(kind, len, src, penalty);
        if (WRITE) {
            sk_score_op op;
            op.length = uint16_t(len);
            op.kind = kind;
            op.flags = uint8_t(penalty ? SK_OPFLAG_NONCANDIDATE_PENALTY : 0);
            op.src = src;
            ops[n] = op;
        }
        ++n;
    };
    // offset of insert bases [head, head+len) of table indel `idx` in the pool, -1 = not representable here
    auto insert_src = [&](const int idx, const int32_t head, const uint32_t len) -> int32_t {
        const PIndel& k = a.job.tab[idx];
        if (head < 0 || uint32_t(head) + len > k.ins_len) return -1;
        for (int i = 0; i < n_ins; ++i)
            if (ins_idx[i] == idx) return ins_off[i] + head;
        return -1;
    };
    auto is_cand = [&](const int idx) -> bool { return job_cand(a.job, idx); };

    int path_index = 0;
    while (path_index < aps) {
        bool is_swap_start = false; // is_segment_swap_start, align_path.cpp:868-895
        {
            bool is_insert = false, is_delete = false;
            for (int i = path_index; i < aps; ++i) {
                if (c.path[i].type == SK_SEG_INSERT) is_insert = true;
                else if (c.path[i].type == SK_SEG_DELETE) is_delete = true;
                else break;
            }
            is_swap_start = is_insert && is_delete;
        }
        unsigned n_seg = 1;
        const PSeg ps = c.path[path_index];
        if (is_swap_start || ps.type == SK_SEG_SEQ_MISMATCH) {
            unsigned del_len, ins_len;
            if (ps.type == SK_SEG_SEQ_MISMATCH) {
                del_len = ins_len = ps.length;
            } else { // swap_info, align_path_util.hh:75-106
                int k = path_index;
                del_len = ins_len = 0;
                for (; k < aps && (c.path[k].type == SK_SEG_INSERT || c.path[k].type == SK_SEG_DELETE); ++k) {
                    if (c.path[k].type == SK_SEG_INSERT) ins_len += c.path[k].length;
                    else del_len += c.path[k].length;
                }
                n_seg = unsigned(k - path_index);
            }
            const int key = matching_indel(a.job, c, ref_head_pos, del_len, ins_len, ends_first, ends_second, path_index);
            if (key < 0) return -1;
            int32_t head = 0;
            if (path_index < ends_first) head = int32_t(a.job.tab[key].ins_len) - int32_t(ps.length);
            const bool pen = !is_cand(key);
            if (ins_len > 0) {
                if (ins_len > 0xffffu) return -1;
                const int32_t src = insert_src(key, head, ins_len);
                if (src < 0) return -1;
                emit(SK_OP_BASES, ins_len, src, pen);
            } else {
                emit(SK_OP_NOBASE, 0, 0, pen);
            }
        } else if (seg_align_match(ps.type)) {
            emit(SK_OP_BASES, ps.length, ref_head_pos - win_begin, false);
        } else if (ps.type == SK_SEG_INSERT) {
            const int key = matching_indel(a.job, c, ref_head_pos, 0, ps.length, ends_first, ends_second, path_index);
            if (key < 0) return -1;
            int32_t head = 0;
            if (path_index < ends_first) head = int32_t(a.job.tab[key].ins_len) - int32_t(ps.length);
            const int32_t src = insert_src(key, head, ps.length);
            if (src < 0) return -1;
            emit(SK_OP_BASES, ps.length, src, !is_cand(key));
        } else if (ps.type == SK_SEG_DELETE) {
            const int key = matching_indel(a.job, c, ref_head_pos, ps.length, 0, ends_first, ends_second, path_index);
            if (key < 0) return -1;
            emit(SK_OP_NOBASE, 0, 0, !is_cand(key));
        } else if (ps.type == SK_SEG_SKIP || ps.type == SK_SEG_HARD_CLIP) {
            // nothing
        } else if (ps.type == SK_SEG_SOFT_CLIP) {
            emit(SK_OP_SOFT_CLIP, ps.length, 0, false);
        } else {
            return -1;
        }
        for (unsigned i = 0; i < n_seg; ++i) { // increment_path, align_path_util.hh:38-68
            const PSeg s = c.path[path_index];
            if (seg_align_match(s.type)) {
                read_offset += s.length;
                ref_head_pos += int32_t(s.length);
            } else if (s.type == SK_SEG_DELETE || s.type == SK_SEG_SKIP) {
                ref_head_pos += int32_t(s.length);
            } else if (s.type == SK_SEG_INSERT || s.type == SK_SEG_SOFT_CLIP) {
                read_offset += s.length;
            }
            path_index++;
        }
    }
    if (int64_t(read_offset) != int64_t(read_len)) return -1;
    return n;
}

// L2, one thread per candidate alignment: how many ops it flattens to
__global__ __launch_bounds__(64) void op_count_kernel(const FlatArgs a)
{
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= a.n_cals) return;
    const int r = read_of_cal(a, c);
    const PCal& cal = a.pool[a.list[c]];
    const int n = flatten_cal<false>(a, r, cal, int32_t(a.read_off[r + 1] - a.read_off[r]), nullptr);
    if (n < 0) a.status[r] = ST_FAIL;
    a.n_ops[c] = n < 0 ? 0 : n;
}

// F1, one wave per read: the bytes of its haplotype pool
__global__ __launch_bounds__(64) void pool_fill_kernel(const FlatArgs a)
{
    const int r = blockIdx.x;
    if (a.cal_off[r + 1] == a.cal_off[r]) return;
    uint8_t* hap = a.hap_code + a.hap_off[r];
    const int32_t P = int32_t(a.hap_off[r + 1] - a.hap_off[r]);
    const int32_t wb = a.win_begin[r];
    const int n_ins = a.n_ins[r];
    const int16_t* idx = a.ins_idx + size_t(r) * INS_CAP;
    const int32_t* off = a.ins_off + size_t(r) * INS_CAP;
    const int32_t win_len = a.win_len[r];
    for (int32_t i = threadIdx.x; i < P; i += 64) {
        uint8_t v = SK_BAM_ANY;
        if (i < win_len) {
            const int32_t p = wb + i; // reference_contig_segment::get_base :46-51
            const bool outside = (p < a.ref_offset || p >= a.ref_offset + a.ref_len);
            if (outside && a.ref_outside) atomicAdd(a.ref_outside, 1);
            v = outside ? uint8_t(SK_BAM_ANY) : code_of(a.ref[p - a.ref_offset]);
        }
        for (int k = 0; k < n_ins; ++k) {
            const PIndel& d = a.job.tab[idx[k]];
            if (i >= off[k] && i < off[k] + int32_t(d.ins_len)) v = code_of(a.ins_pool[d.ins_off + uint32_t(i - off[k])]);
        }
        hap[i] = v;
    }
}

// F2, one thread per candidate alignment: the alignment itself (for the host), its ops, and the candidate-status lookups the
// host form performs for every indel of the alignment (cal_to_c)
__global__ __launch_bounds__(64) void flatten_kernel(const FlatArgs a)
{
    // The wave's 64 records travel pool -> LDS -> cals as rows of consecutive dwords: a lane copying its own 288-byte record field
    // by field made every load and store a scatter over 64 records (1.4 GB of traffic for 360 000 candidate alignments,
    // profiles/r03_v20_pmc_traffic.json); the lanes then read their record from LDS (stride 73 dwords: odd, conflict-free).
    constexpr int REC_DW = int(sizeof(PCal) / 4), REC_STRIDE = REC_DW | 1;
    static_assert(sizeof(PCal) % 4 == 0 && REC_DW <= 128, "a record is at most two dwords per lane");
    __shared__ uint32_t s_cal[64 * REC_STRIDE];
    const int lane = threadIdx.x;
    const int c0 = blockIdx.x * blockDim.x;
    const int c = c0 + lane;
    const int nc = min(64, a.n_cals - c0);
    const int src_k = (lane < nc) ? a.list[c0 + lane] : 0;
    for (int k = 0; k < nc; ++k) {
        const uint32_t* __restrict__ src = reinterpret_cast<const uint32_t*>(a.pool + __shfl(src_k, k));
        uint32_t* __restrict__ dst = reinterpret_cast<uint32_t*>(a.cals + (c0 + k));
        for (int j = lane; j < REC_DW; j += 64) {
            const uint32_t v = src[j];
            s_cal[k * REC_STRIDE + j] = v;
            dst[j] = v;
        }
    }
    __syncthreads();
    if (c >= a.n_cals) return;
    const int r = read_of_cal(a, c);
    const PCal& cal = *reinterpret_cast<const PCal*>(s_cal + lane * REC_STRIDE);
    if (a.status[r] != ST_OK) return; // (its op range is empty)
    (void)flatten_cal<true>(a, r, cal, int32_t(a.read_off[r + 1] - a.read_off[r]), a.ops + a.op_off[c]);
    for (int i = 0; i < cal.n_indels; ++i) (void)job_cand(a.job, cal.indels[i]);
    if (cal.lead >= 0) (void)job_cand(a.job, cal.lead);
    if (cal.trail >= 0) (void)job_cand(a.job, cal.trail);
}

} // namespace
