// enum_stage3.h -- a section of read_enumerate.hip: S3, the kernel wrapper of stage 3 (csrc/stage3_core.h): WaveLanes, Stage3Args,
// stage3_kernel.  Part of that one translation unit (its last device section), not a reusable interface.
#pragma once

#include "sk_common.h"

#include "read_enumerate.h"

using namespace skcore;

namespace
{

// ---------------------------------------------------------------------------------------------------------------------
// S3: stage 3 (csrc/stage3_core.h) -- the max / smooth candidate alignment, the realigned alignment clipped where the smooth
// pool disagrees, the late normalisation filter and score_indels -- one wavefront per read over the read's candidate alignments and
// scores where the scoring kernel left them: the loops over alignments are spread over the 64 lanes, lane 0 takes the decisions the
// reference defines by iteration order (see the header).  What leaves the device is a fixed-size record per read.
enum { S3_LIGHT_CALS = 256, S3_LDS_CALS = 1580 }; // (1580 alignments: 53 KB; with the shared state that stays under 64 KB per workgroup)

struct WaveLanes // the lanes of a workgroup: one wavefront for most reads, four for reads with many candidate alignments
{
    int id, width;
    __device__ void sync() const { __syncthreads(); }
    __device__ void max_i64(long long* p, const long long v) const { atomicMax(p, v); }
};

struct Stage3Args
{
    sk3::Tab tab;
    sk3::Opt opt;
    int32_t n_reads;
    const int32_t* status;
    const int32_t* cal_off;
    const PCal* cals;    // the records in set order -- or, with `slot`, the pool the search left its leaves in
    const int32_t* slot; // null, or [n_cals] the pool slot of every alignment in set order
    const double* scores;
    const int64_t* read_off;
    const uint8_t* read_code;
    const int32_t* map_level;
    int32_t* order;
    double* smooth;
    uint8_t* flag;
    uint32_t* key;
    double* sorted_score;
    uint32_t* sorted_hash;
    int32_t* next_same;
    int32_t* range_end;
    uint8_t* removed;
    uint8_t* rm_type;
    int32_t* rm_pos;
    sk3::Out* out;
    const int32_t* list; // the reads of this launch
    int32_t lds_cals;
    // the job as one fixed sequence: the launch has a block per read of the JOB, the number of reads on this launch's list is on the
    // device (n_list; the heavy list is filled from the back: list_step = -1), and nothing runs when F5 turned a read down (skip_if:
    // the scores are then incomplete -- the host runs the job again through the staged chain)
    const int32_t* n_list;
    int32_t list_step;
    const int32_t* skip_if;
};

template <int WAVES>
__global__ __launch_bounds__(64 * WAVES) void stage3_kernel(const Stage3Args a)
{
    constexpr int T = 64 * WAVES;
    __shared__ sk3::Shared sh;
    extern __shared__ double s3_lds[]; // the per-alignment arrays of the selection and the late normalisation filter, for a read with at most a.lds_cals candidate alignments
    if (a.skip_if && *a.skip_if > 0) return;
    if (a.n_list && int(blockIdx.x) >= *a.n_list) return;
    const int r = a.list[int(blockIdx.x) * (a.n_list ? a.list_step : 1)];
    sk3::Out& o = a.out[r];
    const int32_t c0 = a.cal_off[r], c1 = a.cal_off[r + 1];
    if (a.status[r] != ST_OK || c1 == c0) {
        if (threadIdx.x == 0) o.status = sk3::S3_CAPACITY;
        return;
    }
    const int64_t b0 = a.read_off[r], b1 = a.read_off[r + 1];
    sk3::Read rd;
    rd.cals = a.slot ? sk3::CalView{ a.cals, a.slot + c0 } : sk3::CalView{ a.cals + c0, nullptr };
    rd.scores = a.scores + c0;
    rd.scores_select = rd.scores;
    rd.n_cals = c1 - c0;
    rd.map_level = a.map_level[r];
    rd.read_length = int32_t(b1 - b0);
    if (threadIdx.x == 0) sh.ne = 0; // (borrowed as the counter of bases that are not N)
    __syncthreads();
    {
        int na = 0;
        for (int64_t i = b0 + threadIdx.x; i < b1; i += T) na += (a.read_code[i] != SK_BAM_ANY) ? 1 : 0;
        for (int d = 32; d > 0; d >>= 1) na += __shfl_xor(na, d);
        if ((threadIdx.x & 63) == 0) atomicAdd(&sh.ne, na);
    }
    __syncthreads();
    rd.non_ambig = sh.ne;
    __syncthreads();
    sk3::Scratch w;
    w.order = a.order + c0;
    w.smooth = a.smooth + c0;
    w.flag = a.flag + c0;
    w.key = a.key + 4 * size_t(c0);
    w.sorted_score = a.sorted_score + c0;
    w.sorted_hash = a.sorted_hash + c0;
    w.next_same = a.next_same + c0;
    w.range_end = a.range_end + c0;
    w.removed = a.removed + c0;
    w.rm_type = a.rm_type + b0;
    w.rm_pos = a.rm_pos + b0;
    if (rd.n_cals <= a.lds_cals) {
        // what lane 0's scans and the ordering walk over and over sits in LDS (the accesses are chains of dependent loads)
        double* sc = s3_lds; // the scores for the selection, later the smoothed scores by place
        double* ssc = sc + a.lds_cals;
        int32_t* ord = reinterpret_cast<int32_t*>(ssc + a.lds_cals);
        uint32_t* shs = reinterpret_cast<uint32_t*>(ord + a.lds_cals);
        int32_t* nxt = reinterpret_cast<int32_t*>(shs + a.lds_cals);
        int32_t* rend = nxt + a.lds_cals;
        uint8_t* fl = reinterpret_cast<uint8_t*>(rend + a.lds_cals);
        uint8_t* rem = fl + a.lds_cals;
        for (int i = threadIdx.x; i < rd.n_cals; i += T) sc[i] = rd.scores[i];
        __syncthreads();
        rd.scores_select = sc;
        w.smooth = sc;
        w.sorted_score = ssc;
        w.sorted_hash = shs;
        w.next_same = nxt;
        w.range_end = rend;
        w.order = ord;
        w.flag = fl;
        w.removed = rem;
    }
    WaveLanes ln;
    ln.id = int(threadIdx.x);
    ln.width = T;
    sk3::finish_read(ln, a.tab, a.opt, rd, w, sh, o);
}

} // namespace
