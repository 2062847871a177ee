// score_alignments.hip -- hot path A: ln P(read | candidate alignment) for batches of (read, candidate alignment) pairs.
//
// Reproduces scoreCandidateAlignment (L/starling_common/starling_read_align_score.cpp:261-499) bit-for-bit: one running
// double per pair, terms added in path order, every term taken from the host-built tables (SkTables), no FMA
// contraction, no reassociation.
//
// Kernel A1 `score_wave_per_read` (the fast path; needs the batch's prepared form, csrc/align_entry.h)
//   * one 64-lane wavefront per read, one LANE per candidate alignment of that read (up to 64 per pass), 4 waves per block;
//   * per wave, LDS holds (a) the read as a per-position ROW of 6 doubles {term vs hap A, C, G, T, other, 0.0}: M =
//     ln(1-e_q) in the column of the read base, X = ln(e_q)-ln3 elsewhere; all 0.0 for an 'N' read base (the reference's
//     `continue`), all M for '='; (b) the read's haplotype pool as row-column byte offsets, followed by a run of "0.0
//     column" bytes; (c) the pass's TRANSITION ENTRIES, one short list per candidate (read position, hap index base, the
//     first two columns, penalties / soft-clip term to add first), copied from the prepared batch with coalesced loads;
//     (d) the read's event mask: the read positions at which ANY candidate has an entry;
//   * all lanes sweep the read positions together, one uniform scalar loop.  Per cell: one ds_read_b64
//     (row[position][column]; the row address is wave-uniform, so the reads of a row are LDS broadcasts), one
//     ds_read_u8 (the lane's haplotype column two positions ahead), one dependent v_add_f64 one position behind.
//     Soft-clipped and finished lanes read the 0.0 column (x + 0.0 == x exactly): they stay in lock-step without
//     changing a bit of the result;
//   * a scalar bit test per position tells whether any lane has a transition there; only then do the lanes whose next
//     entry starts at that position take the short transition: new hap index base and columns come out of the entry
//     register, the next entry is fetched from LDS, penalties / the soft-clip term are added in path order.
//
// Kernel A2 `score_thread_per_cal` (generic fallback: reads/pools too long for LDS, or unknown bounds)
//   one thread per candidate alignment, straight from global memory.
//
// Roofline: HBM-bound by the algorithmic bytes of SURVEY.md 8d (2L + H*(L_h+8) per read); this layout moves far fewer
// (the haplotypes are never materialised: 2L + pool + 8*ops + 8H per read), so the sweep is LDS/VALU-issue bound.

#include "sk_common.h"

#include "align_entry.h"

#include <algorithm>
#include <cstdlib>
#include <vector>

namespace
{

#ifndef SK_A1_WAVES_PER_BLOCK
#define SK_A1_WAVES_PER_BLOCK 4
#endif
constexpr int WAVES_PER_BLOCK = SK_A1_WAVES_PER_BLOCK;
constexpr int WAVE = 64;
constexpr int ROW_BYTES = 48;                 // per read position: {A, C, G, T, other, 0.0} doubles
constexpr int ZERO_COL = 8 * SK_ENT_ZERO_COL; // byte offset of the 0.0 column
constexpr int ENT_CAP = 576;                  // transition entries per wave per pass (ops of the pass + 2 per candidate)

__device__ __forceinline__ double dadd(double a, double b) { return __dadd_rn(a, b); }

// BAM 4-bit code of a haplotype base -> byte offset of its column in a table row
__device__ __forceinline__ unsigned hap_col_offset(const unsigned code)
{
    return code == SK_BAM_A ? 0u : code == SK_BAM_C ? 8u : code == SK_BAM_G ? 16u : code == SK_BAM_T ? 24u : 32u;
}

struct ScoreArgs
{
    sk_align_batch b;
    const SkTables* tab;
    double* out;
    int lds_tab_bytes; // per wave: ROW_BYTES * maxL
    int lds_hap_bytes; // per wave: align16(maxP + maxL + 8)  (pool columns + the 0.0-column run)
    unsigned* err;     // SkContext::dev_error_flags
    int dbg;           // (diagnostics: phases to skip, see tools/diag)
};

__device__ __forceinline__ void wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// one candidate alignment straight from global memory (kernel A2; also the per-candidate escape of A1)
__device__ double score_one_generic(const ScoreArgs& a, const int r, const int c)
{
    const int64_t ro = a.b.read_off[r];
    const int64_t ho = a.b.hap_off[r];
    const SkTables* __restrict__ T = a.tab;
    double lnp = 0.0;
    int rp = 0;
    for (int64_t k = a.b.op_off[c]; k < a.b.op_off[c + 1]; ++k) {
        const sk_score_op op = a.b.ops[k];
        if (op.kind == SK_OP_BASES) {
            for (int j = 0; j < int(op.length); ++j) {
                const unsigned rc = a.b.read_code[ro + rp + j];
                if (rc == SK_BAM_ANY) continue;
                unsigned q = a.b.read_qual[ro + rp + j];
                if (q > 70u) { // the reference throws (qscore_cache.cpp:53-75): flag it, sk_check_device_errors reports it
                    atomicOr(a.err, unsigned(SK_DEVERR_QSCORE));
                    q = 70u;
                }
                const bool is_ref = (rc == SK_BAM_REF) || (rc == a.b.hap_code[ho + op.src + j]);
                lnp = dadd(lnp, is_ref ? T->q2lncompe[q] : T->q2mis[q]);
            }
            rp += op.length;
        } else if (op.kind == SK_OP_SOFT_CLIP) {
            lnp = dadd(lnp, __dmul_rn(double(unsigned(op.length)), T->ln_quarter));
            rp += op.length;
        }
        if (op.flags & SK_OPFLAG_NONCANDIDATE_PENALTY) lnp = dadd(lnp, T->ln_noncand);
    }
    return lnp;
}

// Kernel A1.  LDS slab per wave: [rows][hap columns + 0.0 run][entries][event mask]
__device__ __forceinline__ void score_wave_per_read_body(const ScoreArgs& a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int lane = threadIdx.x & (WAVE - 1);
    const int wave = __builtin_amdgcn_readfirstlane(int(threadIdx.x) / WAVE); // wave-uniform: L, P, offsets live in SGPRs
    constexpr int ENT_BYTES = (ENT_CAP + 4) * 4;
    const int W = a.b.evmask_words;
    const size_t per_wave = (size_t(a.lds_tab_bytes) + a.lds_hap_bytes + ENT_BYTES + size_t(W) * 4 + 15) & ~size_t(15); // 16-byte aligned slabs
    unsigned char* slab = smem + per_wave * wave;
    unsigned char* tabb = slab;
    unsigned char* hap = slab + a.lds_tab_bytes;
    unsigned* ent = reinterpret_cast<unsigned*>(hap + a.lds_hap_bytes);
    unsigned* mask = ent + (ENT_CAP + 4);

    const int r = blockIdx.x * WAVES_PER_BLOCK + wave;
    if (r >= a.b.n_reads) return; // whole wave; waves never synchronise with each other

    const int64_t ro = a.b.read_off[r];
    const int L = int(a.b.read_off[r + 1] - ro);
    const int64_t ho = a.b.hap_off[r];
    const int P = int(a.b.hap_off[r + 1] - ho);
    const int cal_begin = a.b.cal_off[r], cal_end = a.b.cal_off[r + 1];
    {
        // Global loads are issued in groups, before any of them is consumed, so that their latencies overlap.
        // haplotype pool as column offsets, then the 0.0-column run (soft-clipped / finished lanes index into it)
        const uint8_t* __restrict__ gh = a.b.hap_code + ho;
        for (int j0 = 0; j0 < P; j0 += 8 * WAVE) {
            unsigned t[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int j = j0 + u * WAVE + lane;
                t[u] = (j < P) ? gh[j] : unsigned(SK_BAM_ANY);
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int j = j0 + u * WAVE + lane;
                if (j < P) hap[j] = (unsigned char)hap_col_offset(t[u]);
            }
        }
        for (int j = P + lane; j < a.lds_hap_bytes; j += WAVE) hap[j] = ZERO_COL;
        const uint32_t* __restrict__ gm = a.b.evmask + int64_t(r) * W;
        for (int j = lane; j < W; j += WAVE) mask[j] = gm[j];
        if (lane == 0) { // the entry list of lanes without a candidate: 0.0 column throughout
            ent[ENT_CAP] = unsigned(SK_ENT_ZERO_COL << 15) | unsigned(SK_ENT_ZERO_COL << 18) | (unsigned(P + SK_ENT_HIDX_BIAS) << 21);
            ent[ENT_CAP + 1] = SK_ENT_END;
        }
        // per-position rows: row[col] = the term added when the haplotype base of that column faces read base i
        //   'N' read base -> 0.0 everywhere (the reference `continue`s, :125/:158)
        //   '=' read base -> M everywhere   (always a match, :127/:160)
        const SkTables* __restrict__ T = a.tab;
        double* tab = reinterpret_cast<double*>(tabb);
        for (int j0 = 0; j0 < L; j0 += 4 * WAVE) {
            unsigned rcv[4], rqv[4];
            double Mv[4], Xv[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int j = j0 + u * WAVE + lane;
                rcv[u] = (j < L) ? a.b.read_code[ro + j] : unsigned(SK_BAM_ANY);
                rqv[u] = (j < L) ? a.b.read_qual[ro + j] : 0u;
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                if (rqv[u] > 70u) atomicOr(a.err, unsigned(SK_DEVERR_QSCORE)); // see score_one_generic
                const unsigned q = rqv[u] > 70u ? 70u : rqv[u];
                Mv[u] = T->q2lncompe[q];
                Xv[u] = T->q2mis[q];
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int j = j0 + u * WAVE + lane;
                if (j >= L) continue;
                const unsigned rc = rcv[u];
                const bool any = (rc == SK_BAM_ANY);
                const double M = any ? 0.0 : Mv[u];
                const double X = any ? 0.0 : (rc == SK_BAM_REF ? M : Xv[u]);
                double* row = tab + 6 * j;
                row[0] = (rc == SK_BAM_A) ? M : X;
                row[1] = (rc == SK_BAM_C) ? M : X;
                row[2] = (rc == SK_BAM_G) ? M : X;
                row[3] = (rc == SK_BAM_T) ? M : X;
                row[4] = X; // haplotype 'N'/other never equals a non-N read code
                row[5] = 0.0;
            }
        }
    }

    const double ln_quarter = a.tab->ln_quarter;
    const double ln_noncand = a.tab->ln_noncand;
    const uint32_t* __restrict__ gent = a.b.entries;

    int cbase = cal_begin;
    while (cbase < cal_end) {
        // ---- how many candidates this pass takes: their entry slots (ops + 2 each) must fit the LDS table
        const int c = cbase + lane;
        const bool has = (c < cal_end);
        const int64_t sbase = a.b.op_off[cbase] + 2 * int64_t(cbase); // first entry slot of the pass
        const int s1 = has ? int(a.b.op_off[c + 1] + 2 * int64_t(c + 1) - sbase) : 0x3fffffff; // end slot of the lane's candidate
        const bool fits = has && (s1 <= ENT_CAP);
        const int m = __popcll(__ballot(fits)); // `fits` is monotone in the lane index
        if (m == 0) { // a single candidate with more ops than the table holds
            if (lane == 0) a.out[cbase] = score_one_generic(a, r, cbase);
            cbase += 1;
            continue;
        }
        const bool active = lane < m;
        const int nslots = __builtin_amdgcn_readlane(s1, m - 1);
        const int prev_end = __shfl_up(s1, 1); // the lane's first slot is where the previous lane's candidate ends
        const int ebase = active ? (lane == 0 ? 0 : prev_end) : ENT_CAP;

        wave_sync(); // the previous pass is done with the entry table; rows / hap columns / mask are complete
        for (int j0 = 0; j0 < nslots; j0 += 10 * WAVE) { // the pass's entries are contiguous in the prepared batch
            unsigned t[10];
#pragma unroll
            for (int u = 0; u < 10; ++u) {
                const int j = j0 + u * WAVE + lane;
                t[u] = (j < nslots) ? gent[sbase + j] : SK_ENT_END;
            }
#pragma unroll
            for (int u = 0; u < 10; ++u) {
                const int j = j0 + u * WAVE + lane;
                if (j < nslots) ent[j] = t[u];
            }
        }
        wave_sync();

        // ---- the sweep
        double lnp = 0.0, pend = 0.0; // pend: the term of the previous position, added one step later
        unsigned nxt = ent[ebase];
        const bool complex_cal = (nxt == SK_ENT_COMPLEX);
        if (complex_cal) nxt = ent[ENT_CAP];
        int kp = complex_cal ? ENT_CAP + 1 : ebase + 1;
        int hidx = 0;          // the lane's haplotype column of read position i is hap[hidx + i]
        unsigned cA = 0, cB = 0; // columns of the next even / odd position
        // lanes whose next entry starts at read position i; `first` receives the column of position i, `second` of i+1
        auto transition = [&](const int i, unsigned& first, unsigned& second) {
            const unsigned e = nxt;
            nxt = ent[kp++];
            if (e & SK_ENT_ADD_BITS) {
                lnp = dadd(lnp, pend); // the last base term precedes the penalties
                pend = 0.0;
                const unsigned np = (e >> 10) & 7u;
                for (unsigned t = 0; t < np; ++t) lnp = dadd(lnp, ln_noncand);
                if (e & (1u << 13)) lnp = dadd(lnp, __dmul_rn(double(unsigned(int(nxt & SK_ENT_POS_MASK) - i)), ln_quarter));
            }
            hidx = int(e >> 21) - SK_ENT_HIDX_BIAS;
            first = ((e >> 15) & 7u) << 3;
            second = ((e >> 18) & 7u) << 3;
        };
        transition(0, cA, cB); // every list starts with an entry at read position 0

        const unsigned char* rowp = tabb;
        for (int wb = 0; wb < L; wb += 64) {
            // 64-position window of the event mask, wave-uniform (bit 0 of the read is handled above)
            uint64_t win = uint64_t(uint32_t(__builtin_amdgcn_readfirstlane(mask[wb >> 5]))) |
                           (uint64_t(uint32_t(__builtin_amdgcn_readfirstlane(mask[(wb >> 5) + 1]))) << 32);
            const int wend = (wb + 64 < L) ? wb + 64 : L;
            for (int i = wb; i < wend; i += 2) {
                if (win & 1ull) { // scalar branch: some lane has an entry starting here
                    asm volatile("; event" ::: "memory");
                    if ((nxt & SK_ENT_POS_MASK) == unsigned(i)) transition(i, cA, cB);
                }
                {
                    const double v = *reinterpret_cast<const double*>(rowp + cA);
                    cA = hap[hidx + i + 2];
                    lnp = dadd(lnp, pend);
                    pend = v;
                }
                if (i + 1 < wend) {
                    if (win & 2ull) {
                        asm volatile("; event" ::: "memory");
                        if ((nxt & SK_ENT_POS_MASK) == unsigned(i + 1)) transition(i + 1, cB, cA);
                    }
                    const double v = *reinterpret_cast<const double*>(rowp + ROW_BYTES + cB);
                    cB = hap[hidx + i + 3];
                    lnp = dadd(lnp, pend);
                    pend = v;
                }
                win >>= 2;
                rowp += 2 * ROW_BYTES;
            }
        }
        // entries at the end of the read: trailing penalties
        if ((uint32_t(__builtin_amdgcn_readfirstlane(mask[L >> 5])) >> (L & 31)) & 1u) {
            if ((nxt & SK_ENT_POS_MASK) == unsigned(L)) transition(L, cA, cB);
        }
        lnp = dadd(lnp, pend);
        if (active) a.out[c] = complex_cal ? score_one_generic(a, r, c) : lnp;
        cbase += m;
    }
}

// Kernel A1c `score_wave_per_read_cols`: the column form of the batch (sk_align_batch::colmat).  Same wave-per-read layout, but
// the lanes do not follow transition entries: every lane streams its candidate alignment from HBM -- per read position which of
// the position's terms the haplotype base selects (agree: ln(1-e_q), differ: ln(e_q/3), nothing) -- eight read positions per
// 32-bit word (four bits each), 64 lanes side by side (256-byte
// coalesced loads).  A 150 bp candidate is 19 words, so a lane holds its WHOLE candidate in registers: every global load
// of a read (bases, qualities, add mask, all column words) is issued at the top of the kernel, one round trip after the offsets.
// LDS holds, per wave, the read as one row {ln(1-e_q), ln(e_q/3), 0.0} per position (24 bytes: half of what the six-column rows
// of score_wave_per_read take, so half again as many waves fit a CU).  Per cell: 1.5 VALU to unpack the selector and form the
// row address, one ds_read_b64 and the dependent v_add_f64.  The entries
// are looked at only where the read's add mask says some candidate adds penalty or soft-clip terms -- those words (eight
// positions) take the ordered, branchy form; all others are branch-free.
constexpr uint32_t ZERO_WORD = 0x22222222u; // eight positions that add nothing
constexpr int SEL_ROW_BYTES = 24;             // per read position: {agree, differ, 0.0}

// the eight row-relative byte offsets (8 * selector) of a column word: lo's bytes are positions 0..3, hi's positions 4..7
__device__ __forceinline__ void unpack_cols(const uint32_t w, uint32_t& lo, uint32_t& hi)
{
    lo = (w & 0x03030303u) << 3; // (bit 2 of a nibble is the penalty flag, bit 3 is unused)
    hi = (w & 0x30303030u) >> 1;
}

template <int NW> // column words a lane holds in registers: reads up to 8 * NW positions are swept without a load in the loop
__device__ __forceinline__ void score_cols_body(const ScoreArgs& a)
{
    static_assert(NW % 2 == 0, "words are swept in pairs");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int lane = threadIdx.x & (WAVE - 1);
    const int wave = __builtin_amdgcn_readfirstlane(int(threadIdx.x) / WAVE);
    constexpr int ENT_BYTES = (ENT_CAP + 4) * 4;
    const int W = a.b.evmask_words;
    const size_t per_wave = (size_t(a.lds_tab_bytes) + ENT_BYTES + size_t(W) * 4 + 15) & ~size_t(15);
    unsigned char* tabb = smem + per_wave * wave;
    unsigned* ent = reinterpret_cast<unsigned*>(tabb + a.lds_tab_bytes);
    unsigned* mask = ent + (ENT_CAP + 4);
    // the two quality tables, once per workgroup: a read's row build then depends on one global round trip, not two
    double* qtab = reinterpret_cast<double*>(smem + per_wave * WAVES_PER_BLOCK);
    for (int i = threadIdx.x; i < 2 * (SK_NQ + 1); i += WAVES_PER_BLOCK * WAVE)
        qtab[i] = (i <= SK_NQ) ? a.tab->q2lncompe[i] : a.tab->q2mis[i - (SK_NQ + 1)];
    if (lane == 0) { // the entry list of lanes without a candidate
        ent[ENT_CAP] = SK_ENT_END;
        ent[ENT_CAP + 1] = SK_ENT_END;
        ent[ENT_CAP + 2] = SK_ENT_END;
        ent[ENT_CAP + 3] = SK_ENT_END;
    }
    __syncthreads(); // (the only workgroup-wide step: from here on the waves run on their own)

    const int n_reads = a.b.n_reads;
    const uint32_t* __restrict__ gent = a.b.entries;
    const double ln_quarter = a.tab->ln_quarter;
    const double ln_noncand = a.tab->ln_noncand;

    struct Head
    {
        int64_t ro;
        int L, cal_begin, cal_end;
        const uint32_t* cm;
    };
    // where read r's data is: the offsets are fetched TWO reads ahead, so that the data fetch below never waits for them
    auto fetch_head = [&](const int r, Head& h) {
        h.ro = a.b.read_off[r];
        h.L = int(a.b.read_off[r + 1] - h.ro);
        h.cal_begin = a.b.cal_off[r];
        h.cal_end = a.b.cal_off[r + 1];
        h.cm = a.b.colmat + a.b.colmat_off[r];
    };
    // everything the wave needs of read r, in flight at once
    auto fetch = [&](const int r, const Head& h, unsigned (&rq)[4], uint32_t (&cw)[NW], unsigned& am) {
        const int ncr = h.cal_end - h.cal_begin, nch = (h.L + 7) >> 3;
        const uint32_t* cp = h.cm + ((lane < ncr) ? lane : (ncr > 0 ? ncr - 1 : 0));
#pragma unroll
        for (int t = 0; t < NW; ++t) cw[t] = (t < nch && ncr > 0) ? cp[int64_t(t) * ncr] : ZERO_WORD;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int j = u * WAVE + lane;
            rq[u] = (j < h.L) ? a.b.read_qual[h.ro + j] : 0u;
        }
        am = (lane < W) ? a.b.addmask[int64_t(r) * W + lane] : 0u;
    };

    const int r = int(blockIdx.x) * WAVES_PER_BLOCK + wave;
    if (r >= n_reads) return;
    Head cur;
    unsigned rq[4], am;
    uint32_t cw[NW];
    fetch_head(r, cur);
    fetch(r, cur, rq, cw, am);

    {
        const int64_t ro = cur.ro;
        const int L = cur.L, cal_begin = cur.cal_begin, cal_end = cur.cal_end;
        const int ncr = cal_end - cal_begin, nch = (L + 7) >> 3;
        const uint32_t* __restrict__ cm = cur.cm;

        // ---- the read's add mask and rows into LDS
        const unsigned cx = (lane == W - 1) ? (am >> 31) : 0u;
        const unsigned ne = (lane == W - 1) ? ((am >> 30) & 1u) : 0u;
        const unsigned amw = (lane == W - 1) ? (am & 0x3fffffffu) : am;
        if (lane < W) mask[lane] = amw;
        const bool any_add = __any(amw != 0);
        const bool has_complex = __any(cx != 0);
        // added terms come either from the nibbles' penalty flags (every entry of the read that adds anything adds exactly one
        // penalty) or, for the reads where that does not hold, from the candidates' entry lists
        const bool has_add = any_add && __any(ne != 0);
        const bool has_flags = any_add && !has_add;
        {
            // per-position rows {M, X, 0.0}: the terms of a read base of this quality that agrees / differs; which one a
            // candidate takes (or none: read base N, soft clip, past the end) is in its column word
            double* tab = reinterpret_cast<double*>(tabb);
            const int rows = (a.dbg & 1) ? 0 : 8 * nch;
            for (int j0 = 0; j0 < rows; j0 += 4 * WAVE) {
                unsigned rqv[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int j = j0 + u * WAVE + lane;
                    rqv[u] = (j0 == 0) ? rq[u] : ((j < L) ? a.b.read_qual[ro + j] : 0u);
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int j = j0 + u * WAVE + lane;
                    if (j >= rows) continue;
                    if (rqv[u] > 70u) atomicOr(a.err, unsigned(SK_DEVERR_QSCORE));
                    const unsigned q = rqv[u] > 70u ? 70u : rqv[u];
                    double* row = tab + 3 * j;
                    row[0] = qtab[q];
                    row[1] = qtab[SK_NQ + 1 + q];
                    row[2] = 0.0;
                }
            }
        }

        int cbase = cal_begin;
        bool first_pass = true;
        while (cbase < cal_end) {
            const int c = cbase + lane;
            const bool has = (c < cal_end);
            int m, ebase = ENT_CAP;
            unsigned first_entry = 0;
            if (has_add) { // the pass's entries go to LDS, as in score_wave_per_read
                const int64_t sbase = a.b.op_off[cbase] + 2 * int64_t(cbase);
                const int s1 = has ? int(a.b.op_off[c + 1] + 2 * int64_t(c + 1) - sbase) : 0x3fffffff;
                const bool fits = has && (s1 <= ENT_CAP);
                m = __popcll(__ballot(fits));
                if (m == 0) {
                    if (lane == 0) a.out[cbase] = score_one_generic(a, r, cbase);
                    cbase += 1;
                    first_pass = false;
                    continue;
                }
                const int nslots = __builtin_amdgcn_readlane(s1, m - 1);
                const int prev_end = __shfl_up(s1, 1);
                ebase = (lane < m) ? (lane == 0 ? 0 : prev_end) : ENT_CAP;
                wave_sync();
                for (int j0 = 0; j0 < nslots; j0 += 10 * WAVE) {
                    unsigned t[10];
#pragma unroll
                    for (int u = 0; u < 10; ++u) {
                        const int j = j0 + u * WAVE + lane;
                        t[u] = (j < nslots) ? gent[sbase + j] : SK_ENT_END;
                    }
#pragma unroll
                    for (int u = 0; u < 10; ++u) {
                        const int j = j0 + u * WAVE + lane;
                        if (j < nslots) ent[j] = t[u];
                    }
                }
                wave_sync();
                first_entry = ent[ebase];
            } else {
                m = (cal_end - cbase < WAVE) ? cal_end - cbase : WAVE;
                if (has_complex) first_entry = has ? gent[a.b.op_off[c] + 2 * int64_t(c)] : 0u; // (else no candidate of the read is)
                wave_sync(); // rows / mask complete
            }
            const bool active = lane < m;
            const bool complex_cal = active && (first_entry == SK_ENT_COMPLEX);
            int kp = (active && !complex_cal) ? ebase : ENT_CAP;
            unsigned e1 = SK_ENT_END; // the lane's next entry (looked at only in words the add mask flags)
            if (has_add) e1 = ent[kp++];

            const int j = (has ? c : cal_end - 1) - cal_begin;
            const uint32_t* __restrict__ cp = cm + j;
            if (!first_pass) { // more than 64 candidate alignments: this pass's words were not fetched ahead
#pragma unroll
                for (int t = 0; t < NW; ++t) cw[t] = (t < nch) ? cp[int64_t(t) * ncr] : ZERO_WORD;
            }
            first_pass = false;

            double lnp = 0.0;
            // an entry that adds terms, at read position i: the non-candidate penalties, then the soft-clip term (path order)
            auto at_position = [&](const int i) {
                if ((e1 & SK_ENT_POS_MASK) == unsigned(i)) {
                    const unsigned e = e1;
                    e1 = ent[kp++];
                    if (e & SK_ENT_ADD_BITS) {
                        const unsigned np = (e >> 10) & 7u;
                        for (unsigned t = 0; t < np; ++t) lnp = dadd(lnp, ln_noncand);
                        if (e & (1u << 13)) lnp = dadd(lnp, __dmul_rn(double(unsigned(int(e1 & SK_ENT_POS_MASK) - i)), ln_quarter));
                    }
                }
            };
            // word t (read positions 8t..8t+7) the ordered way: entries that add terms are interleaved with the base terms
            auto ordered_word = [&](const uint32_t w, const int t) {
                uint32_t lo, hi;
                unpack_cols(w, lo, hi);
                const unsigned char* rp = tabb + SEL_ROW_BYTES * 8 * t;
                const int i0 = 8 * t;
                while ((e1 & SK_ENT_POS_MASK) < unsigned(i0)) e1 = ent[kp++]; // entries passed without a look
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    at_position(i0 + u);
                    const uint32_t col8 = (((u < 4) ? lo : hi) >> (8 * (u & 3))) & 0xffu;
                    lnp = dadd(lnp, *reinterpret_cast<const double*>(rp + SEL_ROW_BYTES * u + col8));
                }
            };
            // words t, t+1 (16 read positions).  A word past the read's end holds eight 0.0 columns and is read against row 0
            // (the third term of every row is 0.0), so the pair is processed whole and without a branch.
            auto word_pair = [&](const uint32_t wa, const uint32_t wb, const int t) {
                uint32_t bits = 0;
                if (has_add || has_flags) bits = (uint32_t(__builtin_amdgcn_readfirstlane(mask[t >> 2])) >> (8 * (t & 3))) & 0xffffu; // t is even
                if (bits != 0 && has_flags) { // a flagged position: one penalty, then its term (adding 0.0 elsewhere changes nothing)
                    const uint32_t ww[2] = { wa, wb };
                    const unsigned char* rpa = tabb + SEL_ROW_BYTES * 8 * t;
                    const unsigned char* rpb = (t + 1 < nch) ? rpa + SEL_ROW_BYTES * 8 : tabb;
#pragma unroll
                    for (int h = 0; h < 2; ++h) {
                        uint32_t lo, hi;
                        unpack_cols(ww[h], lo, hi);
                        const unsigned char* rp = h ? rpb : rpa;
                        double v[8];
#pragma unroll
                        for (int u = 0; u < 4; ++u) {
                            v[u] = *reinterpret_cast<const double*>(rp + SEL_ROW_BYTES * u + ((lo >> (8 * u)) & 0xffu));
                            v[4 + u] = *reinterpret_cast<const double*>(rp + SEL_ROW_BYTES * (4 + u) + ((hi >> (8 * u)) & 0xffu));
                        }
#pragma unroll
                        for (int q = 0; q < 8; ++q) {
                            const uint32_t flag = ww[h] & ((q < 4) ? (0x4u << (8 * q)) : (0x40u << (8 * (q - 4))));
                            lnp = dadd(lnp, flag ? ln_noncand : 0.0);
                            lnp = dadd(lnp, v[q]);
                        }
                    }
                    return;
                }
                if (bits == 0) {
                    uint32_t lo[2], hi[2];
                    unpack_cols(wa, lo[0], hi[0]);
                    unpack_cols(wb, lo[1], hi[1]);
                    const unsigned char* rpa = tabb + SEL_ROW_BYTES * 8 * t;
                    const unsigned char* rpb = (t + 1 < nch) ? rpa + SEL_ROW_BYTES * 8 : tabb;
#pragma unroll
                    for (int h = 0; h < 2; ++h) {
                        const unsigned char* rp = h ? rpb : rpa;
                        double v[8];
#pragma unroll
                        for (int u = 0; u < 4; ++u) {
                            v[u] = *reinterpret_cast<const double*>(rp + SEL_ROW_BYTES * u + ((lo[h] >> (8 * u)) & 0xffu));
                            v[4 + u] = *reinterpret_cast<const double*>(rp + SEL_ROW_BYTES * (4 + u) + ((hi[h] >> (8 * u)) & 0xffu));
                        }
#pragma unroll
                        for (int q = 0; q < 8; ++q) lnp = dadd(lnp, v[q]);
                    }
                    return;
                }
                ordered_word(wa, t);
                if (t + 1 < nch) ordered_word(wb, t + 1);
            };
#pragma unroll
            for (int t = 0; t < NW; t += 2)
                if (t < nch && !(a.dbg & 2)) word_pair(cw[t], cw[t + 1], t);
            for (int t = NW; t < nch; t += 2) { // a read longer than 8 * NW positions: the rest straight from memory
                const uint32_t wa = cp[int64_t(t) * ncr];
                const uint32_t wb = (t + 1 < nch) ? cp[int64_t(t + 1) * ncr] : ZERO_WORD;
                word_pair(wa, wb, t);
            }
            // entries at the end of the read (trailing penalties) when the read's length is a multiple of eight
            if (has_add && (L & 7) == 0 && ((uint32_t(__builtin_amdgcn_readfirstlane(mask[L >> 5])) >> (L & 31)) & 1u)) {
                while ((e1 & SK_ENT_POS_MASK) < unsigned(L)) e1 = ent[kp++];
                at_position(L);
            }
            if (active) a.out[c] = complex_cal ? score_one_generic(a, r, c) : lnp;
            cbase += m;
        }

    }
}

__global__ __launch_bounds__(WAVES_PER_BLOCK* WAVE) void score_wave_per_read_cols(const ScoreArgs a) { score_cols_body<20>(a); }
__global__ __launch_bounds__(WAVES_PER_BLOCK* WAVE) void score_wave_per_read_cols_hostbuf(const ScoreArgs a) { score_cols_body<20>(a); }
__global__ __launch_bounds__(WAVES_PER_BLOCK* WAVE) void score_wave_per_read_cols_long(const ScoreArgs a) { score_cols_body<32>(a); }

// The same code under two names: `score_wave_per_read` is what the device-resident entry (sk_score_alignments_dev: the
// adapter's resident pipeline, bench.py's timed leg) launches, `score_wave_per_read_hostbuf` what the host-buffer entry
// (sk_score_alignments: stage 2 of sk_realign_job_run, small per-window batches) launches -- so that a kernel trace keeps
// the per-launch statistics of the two apart.
__global__ __launch_bounds__(WAVES_PER_BLOCK* WAVE) void score_wave_per_read(const ScoreArgs a) { score_wave_per_read_body(a); }
__global__ __launch_bounds__(WAVES_PER_BLOCK* WAVE) void score_wave_per_read_hostbuf(const ScoreArgs a) { score_wave_per_read_body(a); }

__global__ void score_thread_per_cal(const ScoreArgs a)
{
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= a.b.n_cals) return;
    // read index: last r with cal_off[r] <= c
    int lo = 0, hi = a.b.n_reads;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (a.b.cal_off[mid] <= c) lo = mid; else hi = mid;
    }
    a.out[c] = score_one_generic(a, lo, c);
}

inline int align16(int n) { return (n + 15) & ~15; }

} // namespace

static int score_alignments_launch(const sk_align_batch* b, double* dev_out_lnp, void* hip_stream, const bool from_host_entry)
{
    SK_REQUIRE_INIT();
    if (!b || !dev_out_lnp) return sk_fail("sk_score_alignments_dev: null argument");
    if (b->n_reads < 0 || b->n_cals < 0) return sk_fail("sk_score_alignments_dev: negative count");
    if (b->n_reads == 0 || b->n_cals == 0) return 0;
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    ScoreArgs a;
    a.b = *b;
    a.tab = sk_ctx().dev_tables;
    a.out = dev_out_lnp;
    a.err = sk_ctx().dev_error_flags;
    {
        static const int dbg = [] { const char* e = std::getenv("SK_A1_DBG"); return e ? std::atoi(e) : 0; }();
        a.dbg = dbg;
    }
    const int maxL = b->max_read_len, maxP = b->max_hap_len;
    a.lds_tab_bytes = align16(ROW_BYTES * std::max(maxL, 1));
    a.lds_hap_bytes = align16(std::max(maxP, 0) + std::max(maxL, 1) + 8);
    const size_t per_wave = (size_t(a.lds_tab_bytes) + a.lds_hap_bytes + (ENT_CAP + 4) * 4 + size_t(std::max(b->evmask_words, 0)) * 4 + 15) & ~size_t(15);
    const size_t lds = per_wave * WAVES_PER_BLOCK;
    // fast path: prepared batch, bounds known, and 4 waves' slabs leave room for >= 2 workgroups per CU (160 KiB LDS)
    const bool prepared = b->entries && b->evmask && b->evmask_words == sk_ent_evmask_words(maxL);
    if (prepared && b->colmat && b->colmat_off && b->addmask && maxL > 0 && maxL <= SK_ENT_MAX_READ_LEN) { // the column form
        a.lds_tab_bytes = align16(SEL_ROW_BYTES * ((maxL + 7) & ~7));
        a.lds_hap_bytes = 0;
        const size_t pw = (size_t(a.lds_tab_bytes) + (ENT_CAP + 4) * 4 + size_t(b->evmask_words) * 4 + 15) & ~size_t(15);
        const size_t lds_cols = pw * WAVES_PER_BLOCK + 2 * (SK_NQ + 1) * sizeof(double);
        if (lds_cols <= 64 * 1024) {
            const int blocks = (b->n_reads + WAVES_PER_BLOCK - 1) / WAVES_PER_BLOCK;
            if (maxL > 160) SK_LAUNCH(score_wave_per_read_cols_long, dim3(blocks), dim3(WAVES_PER_BLOCK * WAVE), lds_cols, st, a);
            else if (from_host_entry) SK_LAUNCH(score_wave_per_read_cols_hostbuf, dim3(blocks), dim3(WAVES_PER_BLOCK * WAVE), lds_cols, st, a);
            else SK_LAUNCH(score_wave_per_read_cols, dim3(blocks), dim3(WAVES_PER_BLOCK * WAVE), lds_cols, st, a);
            SK_HIP(skrt::getLastError());
            return 0;
        }
        a.lds_tab_bytes = align16(ROW_BYTES * std::max(maxL, 1));
        a.lds_hap_bytes = align16(std::max(maxP, 0) + std::max(maxL, 1) + 8);
    }
    if (prepared && maxL > 0 && maxL <= SK_ENT_MAX_READ_LEN && maxP > 0 && maxP <= SK_ENT_MAX_POOL && lds <= 64 * 1024) {
        const int blocks = (b->n_reads + WAVES_PER_BLOCK - 1) / WAVES_PER_BLOCK;
        if (from_host_entry) SK_LAUNCH(score_wave_per_read_hostbuf, dim3(blocks), dim3(WAVES_PER_BLOCK * WAVE), lds, st, a);
        else SK_LAUNCH(score_wave_per_read, dim3(blocks), dim3(WAVES_PER_BLOCK * WAVE), lds, st, a);
    } else {
        const int threads = 256;
        const int blocks = (b->n_cals + threads - 1) / threads;
        SK_LAUNCH(score_thread_per_cal, dim3(blocks), dim3(threads), 0, st, a);
    }
    SK_HIP(skrt::getLastError());
    return 0;
}

// device batch, but on behalf of a host-buffer entry point (the realignment job's device pipeline, read_enumerate.hip)
int sk_score_alignments_launch_hostleg(const sk_align_batch* b, double* dev_out_lnp, void* hip_stream)
{
    return score_alignments_launch(b, dev_out_lnp, hip_stream, true);
}

extern "C" int sk_score_alignments_dev(const sk_align_batch* b, double* dev_out_lnp, void* hip_stream)
{
    return score_alignments_launch(b, dev_out_lnp, hip_stream, false);
}

// test hook: force the generic kernel regardless of the bounds (parity of the two kernels is tested against each other)
extern "C" int sk_score_alignments_dev_generic(const sk_align_batch* b, double* dev_out_lnp, void* hip_stream)
{
    SK_REQUIRE_INIT();
    if (!b || !dev_out_lnp) return sk_fail("sk_score_alignments_dev_generic: null argument");
    if (b->n_reads <= 0 || b->n_cals <= 0) return 0;
    ScoreArgs a;
    a.b = *b;
    a.tab = sk_ctx().dev_tables;
    a.out = dev_out_lnp;
    a.lds_tab_bytes = a.lds_hap_bytes = 0;
    const int threads = 256;
    SK_LAUNCH(score_thread_per_cal, dim3((b->n_cals + threads - 1) / threads), dim3(threads), 0,
                       static_cast<hipStream_t>(hip_stream), a);
    SK_HIP(skrt::getLastError());
    return 0;
}

static SkDevBuf g_extra; // sk_score_alignments' column form (outside the arena's reservation: sized only after it)
void sk_score_extra_reset() { g_extra.drop(); }

extern "C" int sk_score_alignments(const sk_align_batch* hb, double* out_lnp)
{
    SK_REQUIRE_INIT();
    if (!hb || !out_lnp) return sk_fail("sk_score_alignments: null argument");
    if (hb->n_reads < 0) return sk_fail("sk_score_alignments: negative n_reads");
    if (hb->n_reads == 0) return 0;
    const int n = hb->n_reads;
    if (hb->read_off[0] != 0 || hb->hap_off[0] != 0 || hb->cal_off[0] != 0)
        return sk_fail("sk_score_alignments: CSR offsets must start at 0");
    const int n_cals = hb->cal_off[n];
    if (n_cals != hb->n_cals) return sk_fail("sk_score_alignments: n_cals != cal_off[n_reads]");
    if (n_cals == 0) return 0;
    if (hb->op_off[0] != 0) return sk_fail("sk_score_alignments: op_off must start at 0");
    const int64_t n_ops = hb->op_off[n_cals];
    if (n_ops != hb->n_ops) return sk_fail("sk_score_alignments: n_ops != op_off[n_cals]");
    const int64_t n_bases = hb->read_off[n], n_hap = hb->hap_off[n];

    // validation the reference performs by throwing: q <= 70 (qscore_cache.cpp:53-75); plus structural checks that
    // keep the kernel's LDS indexing in range
    int maxL = 0, maxP = 0;
    for (int r = 0; r < n; ++r) {
        const int64_t L = hb->read_off[r + 1] - hb->read_off[r], P = hb->hap_off[r + 1] - hb->hap_off[r];
        if (L < 0 || P < 0 || L > 0x7fff0000 || P > 0x7fff0000) return sk_fail("sk_score_alignments: bad CSR offsets");
        maxL = std::max<int>(maxL, int(L));
        maxP = std::max<int>(maxP, int(P));
        for (int c = hb->cal_off[r]; c < hb->cal_off[r + 1]; ++c) {
            int64_t covered = 0;
            for (int64_t k = hb->op_off[c]; k < hb->op_off[c + 1]; ++k) {
                const sk_score_op& op = hb->ops[k];
                if (op.kind == SK_OP_BASES) {
                    if (op.src < 0 || int64_t(op.src) + op.length > P)
                        return sk_fail("sk_score_alignments: op source range outside the read's hap pool");
                    covered += op.length;
                } else if (op.kind == SK_OP_SOFT_CLIP) {
                    covered += op.length;
                } else if (op.kind != SK_OP_NOBASE) {
                    return sk_fail("sk_score_alignments: unknown op kind");
                }
            }
            if (covered != L) return sk_fail("sk_score_alignments: candidate alignment does not span its read");
        }
    }
    for (int64_t i = 0; i < n_bases; ++i)
        if (hb->read_qual[i] > 70) return sk_fail("Attempting to lookup basecall quality score which exceeds the maximum cached score of 70");

    SkContext& ctx = sk_ctx();
    SK_HIP(skrt::setDevice(ctx.device));
    SkArena ar;
    const size_t need = sk_align256(sizeof(int64_t) * (n + 1)) * 2 + sk_align256(sizeof(int32_t) * (n + 1)) +
                        sk_align256(sizeof(int64_t) * (n_cals + 1)) + sk_align256(n_bases) * 2 + sk_align256(n_hap) +
                        sk_align256(sizeof(sk_score_op) * n_ops) + sk_align256(sizeof(double) * n_cals) + 16 * 256 +
                        sk_align256(4 * (size_t(n_ops) + 2 * size_t(n_cals) + 1)) +
                        sk_align256(4 * (size_t(n) * size_t(sk_ent_evmask_words(maxL)) + 1));
    if (ar.reserve(need)) return 1;
    sk_align_batch d = *hb;
    d.max_read_len = maxL;
    d.max_hap_len = std::max(maxP, 1);
    // the device-ready form: taken from the caller when it matches these bounds, else prepared here
    std::vector<uint32_t> h_entries, h_evmask;
    const uint32_t* src_entries = hb->entries;
    const uint32_t* src_evmask = hb->evmask;
    d.evmask_words = sk_ent_evmask_words(maxL);
    if (!(hb->entries && hb->evmask && hb->evmask_words == d.evmask_words && hb->max_read_len == maxL)) {
        h_entries.resize(size_t(n_ops) + 2 * size_t(n_cals) + 1);
        h_evmask.resize(size_t(n) * size_t(d.evmask_words) + 1);
        if (sk_align_prepare(&d, h_entries.data(), h_evmask.data())) return sk_fail("sk_score_alignments: sk_align_prepare failed");
        src_entries = h_entries.data();
        src_evmask = h_evmask.data();
    }
    hipStream_t st = ctx.stream;
#define UP(field, T, count)                                                                              \
    {                                                                                                    \
        T* p = ar.take<T>(count);                                                                        \
        if (count) SK_HIP(skrt::memcpyAsync(p, hb->field, sizeof(T) * (count), hipMemcpyHostToDevice, st)); \
        d.field = p;                                                                                     \
    }
    UP(read_off, int64_t, size_t(n + 1));
    UP(read_code, uint8_t, size_t(n_bases));
    UP(read_qual, uint8_t, size_t(n_bases));
    UP(hap_off, int64_t, size_t(n + 1));
    UP(hap_code, uint8_t, size_t(n_hap));
    UP(cal_off, int32_t, size_t(n + 1));
    UP(op_off, int64_t, size_t(n_cals + 1));
    UP(ops, sk_score_op, size_t(n_ops));
#undef UP
    {
        const size_t ne = size_t(n_ops) + 2 * size_t(n_cals), nm = size_t(n) * size_t(d.evmask_words);
        uint32_t* pe = ar.take<uint32_t>(ne + 1);
        uint32_t* pm = ar.take<uint32_t>(nm + 1);
        if (ne) SK_HIP(skrt::memcpyAsync(pe, src_entries, 4 * ne, hipMemcpyHostToDevice, st));
        if (nm) SK_HIP(skrt::memcpyAsync(pm, src_evmask, 4 * nm, hipMemcpyHostToDevice, st));
        d.entries = pe;
        d.evmask = pm;
    }
    { // the column form: the caller's when it comes with the batch, else made here
        std::vector<uint32_t> h_colmat, h_addmask;
        std::vector<int64_t> h_colmat_off;
        const uint32_t* src_colmat = hb->colmat;
        const int64_t* src_off = hb->colmat_off;
        const uint32_t* src_addmask = hb->addmask;
        if (!(src_colmat && src_off && src_addmask && src_entries == hb->entries)) {
            sk_align_batch tmp = *hb;
            tmp.max_read_len = maxL;
            tmp.entries = src_entries;
            tmp.evmask = src_evmask;
            tmp.evmask_words = d.evmask_words;
            h_colmat.resize(size_t(sk_align_colmat_words(&tmp)) + 1);
            h_colmat_off.resize(size_t(n) + 1);
            h_addmask.resize(size_t(n) * size_t(d.evmask_words) + 1);
            if (sk_align_prepare_cols(&tmp, h_colmat.data(), h_colmat_off.data(), h_addmask.data()))
                return sk_fail("sk_score_alignments: sk_align_prepare_cols failed");
            src_colmat = h_colmat.data();
            src_off = h_colmat_off.data();
            src_addmask = h_addmask.data();
        }
        const size_t words = size_t(src_off[n]), nm = size_t(n) * size_t(d.evmask_words);
        // (outside the arena's first reservation: sized only now)
        if (g_extra.reserve(sk_align256(4 * (words + 1)) + sk_align256(8 * size_t(n + 1)) + sk_align256(4 * (nm + 1)))) return 1;
        char* base = g_extra.as<char>();
        uint32_t* pc = reinterpret_cast<uint32_t*>(base);
        int64_t* po = reinterpret_cast<int64_t*>(base + sk_align256(4 * (words + 1)));
        uint32_t* pa = reinterpret_cast<uint32_t*>(base + sk_align256(4 * (words + 1)) + sk_align256(8 * size_t(n + 1)));
        if (words) SK_HIP(skrt::memcpyAsync(pc, src_colmat, 4 * words, hipMemcpyHostToDevice, st));
        SK_HIP(skrt::memcpyAsync(po, src_off, 8 * size_t(n + 1), hipMemcpyHostToDevice, st));
        if (nm) SK_HIP(skrt::memcpyAsync(pa, src_addmask, 4 * nm, hipMemcpyHostToDevice, st));
        SK_HIP(skrt::streamSynchronize(st)); // (the staging vectors above go out of scope)
        d.colmat = pc;
        d.colmat_off = po;
        d.addmask = pa;
    }
    double* dout = ar.take<double>(n_cals);
    if (score_alignments_launch(&d, dout, st, true)) return 1;
    SK_HIP(skrt::memcpyAsync(out_lnp, dout, sizeof(double) * n_cals, hipMemcpyDeviceToHost, st));
    SK_HIP(skrt::streamSynchronize(st));
    return 0;
}
