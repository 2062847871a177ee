// enum_f5.h -- a section of read_enumerate.hip: F5, flattening and scoring in one kernel (flatten_score_kernel with its walk, sums,
// prologue and rounds), the launch's shape (F5Grid) and its launchers, and at the end, next to the stamps it decodes, the host's
// $SK_F5_TIMING report.  The table of the launch's last hand-outs follows in enum_f5_tail.h.
// Part of that one translation unit (after enum_flatten.h), not a reusable interface.
#pragma once

#include "sk_common.h"

#include "enum_flatten.h"
#include "enum_search.h"
#include "read_enumerate.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <utility>
#include <vector>

namespace
{

// ---------------------------------------------------------------------------------------------------------------------
// F5, one wave per read: flattening AND scoring in one kernel -- scoreCandidateAlignment (starling_read_align_score.cpp:261-499) as the
// reference has it, one function from the alignment to its double.  F1-F3 + A1c stage the same work through HBM (the pool's bytes, 8-byte
// ops, transition entries, masks, column words: 6.8 x the algorithmic bytes, profiles/r03_v24_pmc_traffic.json) and wait on dependent
// global loads lane by lane (a wave of entries_wave_kernel took ~200 us per read); here the read (codes, the two terms of every position),
// its haplotype pool and the wave's 64 candidate-alignment records sit in LDS, every lane walks its alignment's path with flatten_cal and
// adds each op's terms as they come -- bases in read order, then the op's penalty, a soft clip's length x ln 0.25: the order of
// score_one_generic (score_alignments.hip), which A1 / A1c reproduce.  Nothing but the scores (and, while stage 3 reads them there, the
// records' copy in set order) goes back to HBM.
// A read this form does not hold (longer than F5_MAX_READ bases, pool over F5_MAX_POOL bytes) is counted in *n_unhandled: the caller
// then runs F1-F3 + A1c over the job.
constexpr int F5_MAX_READ = 256;  // (as F3's wave form; longer reads and larger pools take the staged chain)
constexpr int F5_MAX_POOL = 768;
#ifndef F5_SORT
#define F5_SORT 1 // experiments: 0 = the set's order
#endif
constexpr int F5_TAB = 32;       // span of table indices the indels of one round's candidate alignments may cover (and the width of the
                                 // mask the round's consulted entries are gathered in: 32 bits, a bit an entry of the copy)

static_assert(F5_TAB <= 32, "the table copy is a lane an entry, the consulted mask a bit an entry");

struct FusedScoreArgs
{
    FlatArgs f;
    const uint8_t* read_qual;
    const SkTables* tab;
    double* scores;
    unsigned* err;         // SkContext::dev_error_flags (a quality above 70)
    int32_t* n_unhandled;  // reads left to the staged kernels
    int32_t write_cals;    // the records' copy in set order (stage 3 and sk_enum_device_fetch_cals read it)
    unsigned long long* dbg; // diagnostics ($SK_F5_TIMING): per read F5_STAMPS cycle stamps, or null
    unsigned* queue;       // [2] the launch's read queue: next read, waves that have left (both 0 between launches: the last wave out zeroes them)
    // the order of the launch's last hand-outs (tail_order_kernel): hand-out h in [tail_first, tail_first + tail_n) is read
    // tail_order[h - tail_first], every other hand-out h is read h; tail_n = 0: the job's own order throughout
    const int32_t* tail_order;
    uint32_t tail_first, tail_n;
    // round sharing (flatten_score_kernel): off with 0 ($SK_F5_SHARE); the rounds scored by a wave other than their read's owner
    int32_t share;
    unsigned* shared_rounds; // [2]: the helped rounds that were scored; the rounds after a read's first that turned their read down
                             // (sk_debug_f5_late_turn_downs: what tests look for a case by)
};

// a candidate alignment's slot in LDS: the walk's output -- up to F5_SEGS + 1 transitions, one per op that covers read positions and
// one for the read's end (start position | penalties that precede the op's terms << 9 | soft clip << 15 | (pool offset - position + 256)
// << 16).  The record's header, path and indel indices are in the lane's registers (F5Rec).  17 words a lane instead of round 3's 39:
// with the table entries cut to the five words the walk reads and the rows of terms sized for the job's longest read, a wave's LDS
// goes from 17.8 KB to under 10 KB and a CU holds 16 of them instead of 9 (profiles/r04_a5_history.txt: a wave alone on a CU takes as
// long as nine sharing it; with sixteen the vector unit is ~85 % busy, profiles/r05_f5_history.txt).
constexpr int F5_SEGS = 16, F5_INDELS = 8;
constexpr int F5_STAMPS = 11; // $SK_F5_TIMING: a read's stamps (f5_prologue, f5_round; the ninth is the cycles of the draw that handed
                              // it out, the tenth the 100 MHz counter at the read's start: where the read lies in the launch, the
                              // eleventh the rounds its owner scored itself)
constexpr int F5_SLOT = (F5_SEGS + 1) | 1; // (odd stride: conflict-free)
__device__ __forceinline__ int f5_ent_word(const int k) { return k; }
// doubles per read position: agree, 0.0, differ -- the read's own cases folded in (a '=' base: differ = agree; an N base and the pad
// rows past the read: both +0.0), so that phase B only asks whether the read byte and the pool byte differ, and a position past the
// op's end reads its row's 0.0: byte offset 0 = agree, 8 = past the op, 16 = differ
constexpr int F5_ROW = 3;

struct F5Tab // what the walk reads of a table entry
{
    int32_t pos;
    uint32_t del, ins_len;
    uint32_t type_cand; // type | cand << 8
    int32_t ins_at;     // where the entry's insert sequence starts in the read's pool, -1 = it is not there (ins_idx / ins_off by entry)
};

template <int MAXR>
struct F5Lds
{
    // (phase B fetches a position's eight bytes as the three aligned words that hold them: up to 11 bytes past the last position;
    // the two byte arrays first, where their words' offsets fit the immediate of a two-word LDS read)
    uint8_t read[MAXR + 12];
    uint8_t hap[F5_MAX_POOL + 12];
    double row[(MAXR + 8) * F5_ROW];
    uint32_t slot[64 * F5_SLOT]; // (phase B reads word F5_SLOT of a lane's slot too: the next lane's, or for lane 63 the table copy)
    // what the walk looks up per path segment (a chain of dependent look-ups: from HBM / L2 they cost a wave ~100 us per round)
    F5Tab tab[F5_TAB];
};
// (the CU hands LDS out in 1 280-byte pieces: 10 240 bytes are sixteen waves to a CU, one byte more fourteen; the 256-base form,
// ~12.4 KB, still fits three four-wave blocks)
constexpr int F5_Q_TERMS = 2 * (SK_NQ + 1); // the block's copy of q2lncompe and q2mis
constexpr size_t F5_SHARE_BYTES = 36; // a wave's claim word and descriptor (F5Share), and 8 bytes a block for its count of busy waves
constexpr size_t f5_block_granules(const size_t lds_object, const int waves) // a block's LDS in the CU's 1 280-byte pieces (128 to a CU)
{
    return ((lds_object + F5_SHARE_BYTES) * size_t(waves) + 8 * size_t(F5_Q_TERMS) + 8 + 1279) / 1280;
}
static_assert(sizeof(F5Lds<152>) <= 10240 && 2 * f5_block_granules(sizeof(F5Lds<152>), 8) <= 128, "two eight-wave blocks of the short-read form to a CU");
static_assert(3 * f5_block_granules(sizeof(F5Lds<F5_MAX_READ>), 4) <= 128, "three four-wave blocks of the long-read form to a CU");
static_assert((152 + 12) % 4 == 0 && (F5_MAX_READ + 12) % 4 == 0 && (F5_MAX_POOL + 12) % 4 == 0, "the byte arrays' words stay aligned");
static_assert(INS_CAP <= 64, "a lane an insert");
static_assert(F5_CODE_PAD >= F5_MAX_POOL + 16 && F5_CODE_PAD % 4 == 0, "a window that leaves the reference stays inside the pad");

// A compact record's path in the lane's registers: the walk looks at a segment's type up to a dozen times per turn (the edge
// segments, the look-ahead for swaps, the step to the next segment) and every look from LDS is a round trip on the lane's chain.  The
// sixteen types are 4 bits each in one 64-bit value, the sixteen lengths 16 bits each in four; segment i is a shift by i (the lengths:
// a select among the four values first).  The indel indices are 6 bits each relative to the round's table copy (tab_lo: every index
// of the round lies in [tab_lo, tab_lo + F5_TAB)), the eight of them in one 64-bit value.
struct F5Rec
{
    uint32_t w0, w1, w2;  // pos; lead | trail << 16; fwd | n_seg << 8 | n_indels << 16
    uint64_t types;       // segment i: bits [4i, 4i + 4)
    uint64_t l0, l1, l2, l3; // segment i: bits [16 (i & 3), + 16) of l(i >> 2)  (four values, not an array: an array indexed per lane
                          // goes to scratch memory)
    uint64_t ind;         // indel k: bits [6k, 6k + 6), its table index - ind_lo
    int ind_lo;
    __device__ __forceinline__ int32_t pos() const { return int32_t(w0); }
    __device__ __forceinline__ int lead() const { return int(int16_t(w1 & 0xffffu)); }
    __device__ __forceinline__ int trail() const { return int(int16_t(w1 >> 16)); }
    __device__ __forceinline__ int n_seg() const { return int((w2 >> 8) & 0xffu); }
    __device__ __forceinline__ int n_indels() const { return int((w2 >> 16) & 0xffu); }
    __device__ __forceinline__ int indel(const int k) const { return ind_lo + int(unsigned(ind >> (6 * k)) & 63u); }
};
static_assert(6 * F5_INDELS <= 64, "an indel index in 6 bits, eight in one value");

// flatten_cal over a compact record, every look-up from the block's LDS copies: the walk of scoreCandidateAlignment :286-493 as
// host/align_flatten.cpp states it, as ONE loop of selects.  Written with the reference's four branches (swap, sequence mismatch, insert,
// delete; match; soft clip; skip / hard clip) a turn is ~1 000 instructions, two thirds of them the scalar unit's mask bookkeeping, and
// the lanes of a wave take the branches in turn (round 4's form, profiles/r05_f5_history.txt).  Here what the branches have in common is
// computed once for every lane and selected: the segment kinds as bit sets over the path (one bit per 4-bit type: a run of insert /
// delete segments, the first and last match segment are shifts and bit counts, not loops), getMatchingIndelKey over packed entries
// (position; del << 16 | ins) up to the largest count in the wave, the insert's place in the pool from the table copy (F5Tab::ins_at).
// Only a swap (insert + delete run: rare) keeps a branch of its own.  The walk writes the alignment's transitions into its slot:
// one word per op that covers read positions and one for the read's end; returns their number, -1 = leave the read to the host form.
template <typename LDS>
__device__ __forceinline__ int f5_walk_selects(LDS& S, const F5Rec c, const bool has, const int tab_lo, const int32_t win_begin, uint32_t& consulted,
                                               const int32_t L, const int32_t P, uint32_t* const myslot)
{
    constexpr uint64_t N1 = 0x1111111111111111ull;
    const uint64_t types = c.types, p_l0 = c.l0, p_l1 = c.l1, p_l2 = c.l2, p_l3 = c.l3;
    const int aps = has ? c.n_seg() : 0;
    auto eq4 = [=](const unsigned v) -> uint64_t { // bit 4 i: segment i is of type v
        uint64_t x = types ^ (N1 * v);
        x |= x >> 1;
        x |= x >> 2;
        return ~x & N1;
    };
    auto seg_len = [=](const int i) -> unsigned {
        const uint64_t lo = (i & 4) ? p_l1 : p_l0, hi = (i & 4) ? p_l3 : p_l2;
        return unsigned(((i & 8) ? hi : lo) >> (16 * (i & 3))) & 0xffffu;
    };
    const uint64_t in_path = (aps >= 16) ? N1 : (((1ull << (4 * aps)) - 1ull) & N1);
    const uint64_t M4 = (eq4(SK_SEG_MATCH) | eq4(SK_SEG_SEQ_MATCH) | eq4(SK_SEG_SEQ_MISMATCH)) & in_path;
    const uint64_t I4 = eq4(SK_SEG_INSERT) & in_path, D4 = eq4(SK_SEG_DELETE) & in_path;
    // get_match_edge_segments, align_path.cpp:735-752
    const int ends_first = M4 ? (__builtin_ctzll(M4) >> 2) : aps, ends_second = M4 ? ((63 - __builtin_clzll(M4)) >> 2) : aps;
    // the alignment's indels, read once: position and the two lengths as one word (del << 16 | ins; an entry that is a breakpoint, or no
    // entry, holds a word no segment asks for); lengths of 0xffff and more are left to the host form
    const int ni = c.n_indels();
    int ni_wave = 0; // (the most indels any of the wave's alignments holds: the entries past it are not looked at)
#pragma unroll
    for (int k = 1; k <= F5_INDELS; ++k) ni_wave = __any(ni >= k) ? k : ni_wave;
    int32_t k_pos[F5_INDELS];
    uint32_t k_pack[F5_INDELS];
    bool bad = false;
#pragma unroll
    for (int k = 0; k < F5_INDELS; ++k) {
        k_pos[k] = INT_MIN;
        k_pack[k] = 0xffffffffu;
        if (k < ni_wave) {
            const F5Tab& ci = S.tab[((k < ni) ? c.indel(k) : tab_lo) - tab_lo];
            const unsigned ty = ci.type_cand & 0xffu;
            const bool kind = (ty == SK_INDEL_INDEL || ty == SK_INDEL_MISMATCH);
            if (k < ni) {
                k_pos[k] = ci.pos;
                if (kind) {
                    k_pack[k] = (ci.del << 16) | ci.ins_len;
                    bad = bad || ci.del >= 0xffffu || ci.ins_len >= 0xffffu;
                }
            }
        }
    }
    int pi = 0, n_ent = 0;
    int32_t pos = 0, ref_head_pos = c.pos(); // (read_offset of the reference's walk)
    unsigned npen = 0;
    for (;;) {
        const bool live = pi < aps && !bad;
        if (!__any(live)) break;
        const int sh = 4 * (pi & 15);
        const unsigned ty = unsigned(types >> sh) & 15u, ln = seg_len(pi & 15);
        // the run of insert / delete segments that starts here (is_segment_swap_start, align_path.cpp:868-895: a swap = both kinds in it)
        const uint64_t not_run = ~((I4 | D4) >> sh) & N1;
        const int run4 = not_run ? __builtin_ctzll(not_run) : 64;
        const uint64_t run_set = (run4 >= 64) ? ~0ull : ((1ull << run4) - 1ull);
        const bool is_swap = live && ((I4 >> sh) & run_set) != 0ull && ((D4 >> sh) & run_set) != 0ull;
        const bool is_match = (ty == SK_SEG_MATCH || ty == SK_SEG_SEQ_MATCH), is_clip = (ty == SK_SEG_SOFT_CLIP);
        const bool is_indel_seg = is_swap || ty == SK_SEG_SEQ_MISMATCH || ty == SK_SEG_INSERT || ty == SK_SEG_DELETE;
        unsigned del_len = (ty == SK_SEG_INSERT) ? 0u : ln, ins_len = (ty == SK_SEG_DELETE) ? 0u : ln;
        int n_seg = 1;
        unsigned read_step = (is_match || ty == SK_SEG_SEQ_MISMATCH || ty == SK_SEG_INSERT || is_clip) ? ln : 0u; // increment_path, align_path_util.hh:38-68
        unsigned ref_step = (is_match || ty == SK_SEG_SEQ_MISMATCH || ty == SK_SEG_DELETE || ty == SK_SEG_SKIP) ? ln : 0u;
        if (is_swap) { // swap_info, align_path_util.hh:75-106
            n_seg = run4 >> 2;
            del_len = ins_len = 0;
            for (int k = 0; k < n_seg; ++k) {
                const unsigned l = seg_len((pi + k) & 15);
                if ((I4 >> (4 * ((pi + k) & 15))) & 1ull) ins_len += l;
                else del_len += l;
            }
            read_step = ins_len;
            ref_step = del_len;
        }
        // getMatchingIndelKey, starling_read_align_score.cpp:177-228: the edge indels outside the match segments; between them the one
        // entry of the alignment's that is this indel -- the reference stops at a second match and at the first entry past the position
        const unsigned asked = (del_len << 16) | ins_len;
        const bool askable = del_len < 0xffffu && ins_len < 0xffffu;
        int k_found = 0, n_found = 0;
        bool open = true;
#pragma unroll
        for (int k = 0; k < F5_INDELS; ++k) {
            if (k < ni_wave) {
                const bool m = open && k_pos[k] == ref_head_pos && k_pack[k] == asked;
                k_found = m ? k : k_found;
                n_found += m ? 1 : 0;
                open = open && (m || k_pos[k] <= ref_head_pos);
            }
        }
        int key = (n_found == 1) ? c.indel(k_found) : -2;
        key = (pi < ends_first) ? c.lead() : (pi > ends_second) ? c.trail() : key;
        const bool key_ok = key >= 0;
        const F5Tab te = S.tab[(key_ok ? key : tab_lo) - tab_lo];
        const bool indel_ok = live && is_indel_seg && key_ok;
        consulted |= indel_ok ? (1u << ((key - tab_lo) & 31)) : 0u; // job_cand: bit key - tab_lo (the copy holds F5_TAB <= 32 entries)
        const bool pen = is_indel_seg && (te.type_cand >> 8) == 0u;
        const int32_t head = (pi < ends_first) ? int32_t(te.ins_len) - int32_t(ln) : 0;
        // the op: bases of the pool (a match segment's window bytes, an indel's insert sequence), a soft clip, or a penalty alone
        const bool ins_bases = is_indel_seg && ins_len > 0u;
        const bool ins_ok = ins_len <= 0xffffu && head >= 0 && uint32_t(head) + ins_len <= te.ins_len && te.ins_at >= 0;
        const bool bases = ins_bases || is_match;
        const int32_t src = ins_bases ? te.ins_at + head : ref_head_pos - win_begin;
        const unsigned len = ins_bases ? ins_len : ln;
        const bool known = is_indel_seg || is_match || is_clip || ty == SK_SEG_SKIP || ty == SK_SEG_HARD_CLIP;
        bool fail = !known || (is_indel_seg && (!key_ok || !askable)) || (ins_bases && !ins_ok);
        const bool entry = (bases || (is_clip && !is_indel_seg)) && len > 0u;
        if (entry) {
            fail = fail || pos + int32_t(len) > L || (bases && (src < 0 || int64_t(src) + int64_t(len) > int64_t(P)));
            const int hidx = bases ? int(src) - pos : 0;
            fail = fail || n_ent > F5_SEGS || npen > 4u || hidx < -256 || hidx > 3839;
            if (live && !fail) myslot[f5_ent_word(n_ent)] = unsigned(pos) | (npen << 9) | (bases ? 0u : 1u << 15) | (unsigned(hidx + 256) << 16);
        }
        if (live) {
            bad = fail;
            n_ent += entry ? 1 : 0;
            npen = entry ? (pen ? 1u : 0u) : npen + (pen ? 1u : 0u);
            pos += int32_t(read_step);
            ref_head_pos += int32_t(ref_step);
            pi += n_seg;
        }
    }
    if (!has) return 0;
    if (bad || pos != L || n_ent > F5_SEGS || npen > 4u) return -1;
    myslot[f5_ent_word(n_ent)] = unsigned(L) | (npen << 9) | (256u << 16); // trailing penalties
    return n_ent + 1;
}

// Phase B of F5, a lane its alignment, in path order (the order of score_one_generic): entering an op, the penalties that precede its
// terms, then a soft clip's length x ln 0.25; inside an op of bases, eight positions per turn -- eight read codes against the eight pool
// bytes they face (SWAR), each position's address: its row's agree or differ term, or the row's 0.0 past the op's end (the rows already
// hold what a '=' or an N read base adds) -- eight reads, eight adds.  ONE loop per lane (eight bases and the step to the next op in the
// same turn), so that the turns a wave makes are the longest lane's, not the sum over ops of the longest op.  What is rare for a whole
// wave -- a penalty, a soft clip -- sits behind a vote.
template <typename LDS>
__device__ __forceinline__ double f5_sum(LDS& S, const uint32_t* const myslot, const int n_ent, const double ln_noncand, const double ln_quarter)
{
    double lnp = 0.0;
    const unsigned char* rows = reinterpret_cast<const unsigned char*>(S.row);
    int e = 0, p = 0, stop = 0, hidx = 0;
    // the current op's transition and the next one stay in registers: a turn reads one slot word, the one after them (word e + 1 <=
    // n_ent <= F5_SLOT: past the read's end it is a word of the LDS object that nothing looks at)
    uint32_t cur = myslot[f5_ent_word(0)], nxt = myslot[f5_ent_word(1)];
    // the step to the next op, by selects (the loop has one back edge); true: the read's end
    auto next_op = [&]() -> bool {
        const bool adv = (p >= stop);
        const int start = int(cur & 0x1ffu), next_start = int(nxt & 0x1ffu);
        const unsigned np = adv ? ((cur >> 9) & 63u) : 0u; // (at most 4: the walk hands anything longer to the host form)
        const bool clip = adv && (cur & (1u << 15)) != 0u; // (never the read's end: its word holds no soft clip)
        if (__builtin_amdgcn_ballot_w64(np != 0u || clip) != 0ull) { // (both rare: one vote)
            const double l1 = __dadd_rn(lnp, ln_noncand);
            lnp = (np >= 1u) ? l1 : lnp;
            const double l2 = __dadd_rn(lnp, ln_noncand);
            lnp = (np >= 2u) ? l2 : lnp;
            const double l3 = __dadd_rn(lnp, ln_noncand);
            lnp = (np >= 3u) ? l3 : lnp;
            const double l4 = __dadd_rn(lnp, ln_noncand);
            lnp = (np >= 4u) ? l4 : lnp;
            const double lc = __dadd_rn(lnp, __dmul_rn(double(unsigned(next_start - start)), ln_quarter));
            lnp = clip ? lc : lnp;
        }
        if (adv && e + 1 >= n_ent) return true;
        p = adv ? (clip ? next_start : start) : p;
        stop = adv ? next_start : stop;
        hidx = adv ? int(cur >> 16) - 256 : hidx;
        e = adv ? e + 1 : e;
        cur = adv ? nxt : cur;
        nxt = myslot[f5_ent_word(e + 1)];
        return false;
    };
    if (next_op()) return lnp; // (the first op: no bases before it)
    for (;;) {
        {
            const int m = stop - p;          // bases of the current op still to add (0: a soft clip just stepped over)
            const int mm = (m > 8) ? 8 : m;
            // the eight read codes at p and the eight pool bytes they face, each from the three aligned words that hold them (a byte
            // address read as one 8-byte word is an unaligned LDS access: replayed); 32-bit halves, positions 0-3 and 4-7
            const int ph = p + hidx;
            const uint32_t* const rw = reinterpret_cast<const uint32_t*>(S.read + (p & ~3));
            const uint32_t* const hw = reinterpret_cast<const uint32_t*>(S.hap + (ph & ~3));
            const uint32_t r0 = rw[0], r1 = rw[1], r2 = rw[2], h0 = hw[0], h1 = hw[1], h2 = hw[2];
            const uint32_t R[2] = {__builtin_amdgcn_alignbyte(r1, r0, unsigned(p)), __builtin_amdgcn_alignbyte(r2, r1, unsigned(p))};
            const uint32_t H[2] = {__builtin_amdgcn_alignbyte(h1, h0, unsigned(ph)), __builtin_amdgcn_alignbyte(h2, h1, unsigned(ph))};
            // 0x18 in the bytes of the positions past the op's end (a suffix of the eight)
            const uint64_t past = (mm >= 8) ? 0ull : (0x1818181818181818ull << (8 * mm));
            constexpr uint32_t B0F = 0x0f0f0f0fu, B10 = 0x10101010u;
            uint32_t sel[2]; // per byte the offset in the position's row: 0 agree, 8 past the op's end (0.0), 16 differ
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                // (the codes are 4-bit: x ^ y + 15 sets bit 4 of a byte exactly when the two differ; a byte past the op may carry into
                // the next one, which is past the op too, and the select drops both: bit 4 from the compare where the position is the
                // op's, bit 3 = past the op)
                const uint32_t x = (R[h] ^ H[h]) + B0F;
                uint32_t pm = uint32_t(past >> (32 * h));
                // (no known bits for the compiler to act on: the select stays one three-input bit op, the bytes' extraction below the
                // byte-select operands of the adds)
                __asm__("" : "+v"(pm));
                sel[h] = (B10 & ~pm & x) | (~B10 & pm);
                __asm__("" : "+v"(sel[h]));
            }
            const unsigned base = __umul24(unsigned(8 * F5_ROW), unsigned(p));
            double v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const unsigned at = base + unsigned(8 * F5_ROW * u) + ((sel[u >> 2] >> (8 * (u & 3))) & 0xffu);
                v[u] = *reinterpret_cast<const double*>(rows + at);
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) lnp = __dadd_rn(lnp, v[u]);
            p += mm;
        }
        if (next_op()) break;
    }
    return lnp;
}

// TIMING: the cycle stamps of $SK_F5_TIMING (fa.dbg); without it the stamps are constants and their s_memtime + waits are gone
// a block is F5_WAVES waves, each with a read and an LDS object of its own: what orders a wave's LDS accesses is the wave (its LDS
// instructions complete in order), so the points where the lanes exchange data through LDS need the compiler's and the counters'
// attention, not a workgroup barrier
__device__ __forceinline__ void f5_wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// a record as it is loaded: header + F5_SEGS path segments (five 16-byte loads) + F5_INDELS indel indices, all in flight at once
struct F5Raw
{
    uint4 q0, q1, q2, q3, q4;
    uint32_t i0, i1, i2, i3;
};
__device__ __forceinline__ F5Raw f5_load_raw(const PCal* src)
{
    F5Raw w;
    const uint4* s4 = reinterpret_cast<const uint4*>(src);
    w.q0 = s4[0], w.q1 = s4[1], w.q2 = s4[2], w.q3 = s4[3], w.q4 = s4[4];
    const uint32_t* si = reinterpret_cast<const uint32_t*>(src->indels);
    w.i0 = si[0], w.i1 = si[1], w.i2 = si[2], w.i3 = si[3];
    return w;
}

constexpr int F5_INS_REG = 4;  // inserts of up to 64 bases each whose bytes the prologue holds in registers (a lane a base)

// The prologue's global loads go out as GROUPS, each waited for once (a wave that asks for one value at a time waits ~1 us for each:
// the prologue and the staging were 46k of a read's 122k cycles, nearly all of it such waits -- profiles/r08_f5_history.txt):
//   group 1  what is indexed by the read alone (cal_off, status, read_off, hap_len, win_begin, n_ins, win_len): uniform loads, above
//            the early return -- every index is in range for r < n_reads
//   group 2  what group 1 addresses: list[] of the first round, the job's table (when it fits the copy: one copy per
//            read, tab_lo = 0), ins_idx / ins_off, the window's codes (words of the job's code image: the pad answers for a window
//            that leaves the reference), the read's codes and qualities, n_seg8
//   group 3  what group 2 addresses: the first round's records (where the set's order is kept) and the inserts' bytes (up to
//            F5_INS_REG inserts of up to 64 bases in registers, written in table order; more or longer ones: the loop)
// With the draw from the queue that is four waits for a read of one round (counted in the assembly, profiles/r08_f5_history.txt); a
// later round waits for its records only (its list[] entry is asked for a round ahead).  The two terms of a quality come from the
// block's copy in LDS (q_terms: q2lncompe, then q2mis).  Not built: the read's codes and qualities as words and S.read written with
// word stores -- they are loaded and stored a byte a lane (up to three of each in flight at once, no wait between them).
//
// A read is scored in two parts.  f5_prologue is its owner's alone: everything up to the first round -- the loads above, the read, the
// pool, the rows of terms, the order and (where the job's table fits it) the table copy written into the owner's LDS object, which
// nothing writes again until the owner's next read.  f5_round is one round of up to 64 candidate alignments: staging, walk, sums, the
// consulted marks, the scores' store.  It reads the read's data through a pointer and writes the EXECUTING wave's slots only, so that
// a wave other than the owner can run it (flatten_score_kernel); what it needs of the read beyond the LDS object is in F5Desc.
struct F5Desc // a read's uniforms, as a round needs them
{
    int32_t r, c0, ncr, L, P, win_begin, sorted_order;
};
// what the owner carries from the prologue into its rounds and from a round into its next one
struct F5Own
{
    int32_t slot_next;      // where the lane's record of the owner's coming round is (list[] a round ahead)
    F5Raw raw0;             // round 0's records, asked for in group 3
    int my_ins_idx;         // lane k < n_ins: the read's insert k (a job whose table does not fit the copy places it per round)
    int32_t my_ins_off;
    unsigned long long stamp[F5_STAMPS], wall0; // $SK_F5_TIMING
};
// a wave's published read, in the block's LDS (flatten_score_kernel: round sharing)
struct F5Share
{
    uint32_t claim; // the next round nobody has claimed | the read's rounds << 16; 0: nothing open
    F5Desc d;
    uint32_t dry_at; // the wave has drawn dry: the 100 MHz counter's low word then, | 1 (0: not yet)
};
static_assert(sizeof(F5Share) == F5_SHARE_BYTES, "f5_block_granules counts the claim words and descriptors");

template <int MAXR, bool TIMING>
__device__ __forceinline__ bool f5_prologue(const FusedScoreArgs& fa, const int r, F5Lds<MAXR>& S, const double* const q_terms, F5Desc& desc,
                                            F5Own& own) // false: the read has nothing to score here
{
    auto now = [&]() -> unsigned long long { return TIMING ? (unsigned long long)clock64() : 0ull; };
    const FlatArgs& a = fa.f;
    unsigned long long(&stamp)[F5_STAMPS] = own.stamp;
    // (the lane as a value of this read's: what is computed from it -- addresses of the loads below -- is computed here, not once
    // per kernel and kept in scratch memory, whose reload is one more wait in the middle of a group)
    int lane_of_read = threadIdx.x & 63;
    __asm__ volatile("" : "+v"(lane_of_read));
    const int lane = lane_of_read;
    stamp[0] = now(); // (before group 1: the prologue's figure holds every trip of the read but the draw, as it did)
    own.wall0 = TIMING ? (unsigned long long)wall_clock64() : 0ull; // (the constant 100 MHz counter: the block's life in time)
    // ---- group 1 (the empty statement keeps the loads together above the early return: every value is asked for before the first
    // is looked at; they are the same in every lane)
    int g1_c0 = a.cal_off[r], g1_c1 = a.cal_off[r + 1];
    int32_t g1_status = a.status[r];
    int64_t g1_ro = a.read_off[r], g1_ro1 = a.read_off[r + 1];
    int32_t g1_P = a.hap_len[r], g1_win_begin = a.win_begin[r], g1_n_ins = a.n_ins[r], g1_win_len = a.win_len[r];
    __asm__ volatile("" : "+v"(g1_c0), "+v"(g1_c1), "+v"(g1_status), "+v"(g1_ro), "+v"(g1_ro1), "+v"(g1_P), "+v"(g1_win_begin), "+v"(g1_n_ins), "+v"(g1_win_len));
    auto uniform64 = [](const int64_t v) -> int64_t {
        return int64_t(uint64_t(uint32_t(__builtin_amdgcn_readfirstlane(int(uint32_t(uint64_t(v)))))) |
                       (uint64_t(uint32_t(__builtin_amdgcn_readfirstlane(int(uint32_t(uint64_t(v) >> 32))))) << 32));
    };
    const int c0 = __builtin_amdgcn_readfirstlane(g1_c0), c1 = __builtin_amdgcn_readfirstlane(g1_c1);
    const int32_t status_r = __builtin_amdgcn_readfirstlane(g1_status);
    const int64_t ro = uniform64(g1_ro), ro1 = uniform64(g1_ro1);
    const int32_t P = __builtin_amdgcn_readfirstlane(g1_P);
    const int32_t win_begin = __builtin_amdgcn_readfirstlane(g1_win_begin);
    const int n_ins = __builtin_amdgcn_readfirstlane(g1_n_ins);
    const int32_t win_len = __builtin_amdgcn_readfirstlane(g1_win_len);
    const int ncr = c1 - c0;
    if (ncr == 0 || status_r != ST_OK) return false;
    for (int i = 1; i < F5_STAMPS; ++i) stamp[i] = 0;
    const int32_t L = int32_t(ro1 - ro);
    if (L > MAXR || P > F5_MAX_POOL) {
        if (lane == 0) atomicAdd(fa.n_unhandled, 1);
        return false;
    }
    // the job's table fits the copy: one copy per read, every index relative to entry 0
    const int job_n_tab = a.job.n_tab;
    const bool whole_tab = job_n_tab <= F5_TAB;
    uint8_t* const order = S.hap + ((P + 8 + 3) & ~3);
    const bool sorted_order = (F5_SORT != 0) && ncr > 64 && ncr <= 256 && ((P + 8 + 3) & ~3) + ncr <= int(sizeof(S.hap));
    // ---- group 2, every load issued before the first use
    // where the lane's record of the coming round is: list[] a round ahead (the first round's here, where the lanes take the read's
    // alignments in the set's order, or after the sort; the next round's while this round's sums run), so that a round waits for its
    // records only
    int32_t slot_next = 0;
    if (!sorted_order && lane < ncr) slot_next = a.list[c0 + lane];
    int32_t lst[4]; // (a read whose alignments are put in order first: list[] of all of them)
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        lst[k] = 0;
        if (sorted_order && lane + 64 * k < ncr) lst[k] = a.list[c0 + lane + 64 * k];
    }
    F5Tab g; // lane t: entry t of the job's table (whole_tab)
    g.pos = 0, g.del = 0, g.ins_len = 0, g.type_cand = 0, g.ins_at = -1;
    uint32_t g_ins_off = 0;
    if (whole_tab && lane < job_n_tab) {
        const PIndel& e = a.job.tab[lane];
        g.pos = e.pos;
        g.del = e.del;
        g.ins_len = e.ins_len;
        g.type_cand = unsigned(e.type) | (unsigned(e.cand) << 8);
        g_ins_off = e.ins_off;
    }
    int my_ins_idx = -1;    // lane k < n_ins: the table index of the read's insert k and where its sequence starts in the pool
    int32_t my_ins_off = 0;
    if (lane < n_ins) {
        my_ins_idx = a.ins_idx[size_t(r) * INS_CAP + lane];
        my_ins_off = a.ins_off[size_t(r) * INS_CAP + lane];
    }
    // the window's codes, a lane a word of the pool: bytes [win_len, P + 8) stay SK_BAM_ANY
    constexpr int HAP_WORDS = int(sizeof(S.hap)) / 4, HAP_K = (HAP_WORDS + 63) / 64;
    constexpr uint32_t ANY4 = 0x01010101u * uint32_t(SK_BAM_ANY);
    uint32_t hw[HAP_K];
    {
        // (32-bit from here: a window that begins further out than the pad reads pad all the same)
        const int32_t p_max = int32_t(min(int64_t(a.ref_len) + F5_CODE_PAD - 4, int64_t(INT_MAX - 2 * F5_CODE_PAD)));
        const int32_t wbase = int32_t(min(max(int64_t(win_begin) - int64_t(a.ref_offset), int64_t(-2 * F5_CODE_PAD)), int64_t(p_max) + F5_CODE_PAD));
#pragma unroll
        for (int k = 0; k < HAP_K; ++k) {
            const int w = lane + 64 * k;
            hw[k] = ANY4;
            if (4 * w < win_len) {
                // (a word that lies beyond the pad on either side holds positions outside the reference only, as the pad does)
                const int32_t p = min(max(wbase + 4 * w, -F5_CODE_PAD), p_max);
                uint32_t v;
                __builtin_memcpy(&v, a.ref_code + p, 4);
                hw[k] = v;
            }
        }
    }
    constexpr int READ_K = (MAXR + 12 + 63) / 64;
    uint8_t rc[READ_K], rq[READ_K];
#pragma unroll
    for (int k = 0; k < READ_K; ++k) {
        const int i = lane + 64 * k;
        rc[k] = SK_BAM_ANY;
        rq[k] = 0;
        if (i < L) {
            rc[k] = a.read_code[ro + i];
            rq[k] = fa.read_qual[ro + i];
        }
    }
    uint8_t seg8[4]; // (left by pool_bounds_kernel, which reads every record anyway; looked at after the pool is placed)
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        seg8[k] = 0;
        if (sorted_order && lane + 64 * k < ncr) seg8[k] = a.n_seg8[c0 + lane + 64 * k];
    }
    // The read's candidate alignments in order of path length, longest first (a counting sort over the segment counts, the order in the
    // unused tail of the pool's bytes): a wave's walk lasts as long as its longest path, so a round of like paths wastes fewer turns
    // and the last, partly filled round gets the short ones.  Reads with more than 256 candidate alignments keep the set's order.
    // Done before the pool is placed: the order lies past the pool's bytes, and the first round's records can go out at once.  list[] of
    // all the read's alignments, up to 256, is parked in the slots meanwhile (the first round's walk is the first to write there).
    if (sorted_order) {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (lane + 64 * k < ncr) S.slot[lane + 64 * k] = uint32_t(lst[k]);
        int seg_of[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) seg_of[k] = (lane + 64 * k < ncr) ? min(int(seg8[k]), F5_SEGS + 1) : -1;
        // (only the segment counts that occur: a read's alignments have a handful of distinct ones -- the loop over all eighteen was ~650
        // of a read's ~7 800 instructions)
        unsigned present = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) present |= (seg_of[k] >= 0) ? (1u << seg_of[k]) : 0u;
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) present |= unsigned(__shfl_xor(int(present), d));
        present = unsigned(__builtin_amdgcn_readfirstlane(int(present)));
        int at = 0; // alignments placed so far
        while (present != 0u) { // descending, as the loop over every count was
            const int v = 31 - __builtin_clz(present);
            present &= ~(1u << v);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const uint64_t m = __ballot(seg_of[k] == v);
                if (seg_of[k] == v) order[at + __popcll(m & ((1ull << lane) - 1ull))] = uint8_t(lane + 64 * k);
                at += __popcll(m);
            }
        }
        f5_wave_sync(); // (the order written)
        slot_next = int32_t(S.slot[order[lane]]); // (more than 64 alignments: every lane has one)
    }
    // ---- group 3: the inserts' bytes, then the first round's records -- all issued before either is looked at
    // (insert k's length and source stay in lane k's registers; its table index and offset go into the table copy, F5Tab::ins_at)
    int32_t my_ins_len = 0;
    uint32_t my_ins_src = 0;
    if (whole_tab) {
        const int32_t len_t = __shfl(int32_t(g.ins_len), my_ins_idx & 63);
        const uint32_t src_t = uint32_t(__shfl(int(g_ins_off), my_ins_idx & 63));
        if (lane < n_ins) {
            my_ins_len = len_t;
            my_ins_src = src_t;
        }
    } else if (lane < n_ins) {
        my_ins_len = int32_t(a.job.tab[my_ins_idx].ins_len);
        my_ins_src = a.job.tab[my_ins_idx].ins_off;
    }
    const bool ins_in_regs = n_ins <= F5_INS_REG && !__any(my_ins_len > 64);
    uint32_t ib[F5_INS_REG]; // (a register each: bytes packed into one would be waited for one by one)
    int32_t ib_n[F5_INS_REG];
    uint32_t ib_src[F5_INS_REG];
#pragma unroll
    for (int k = 0; k < F5_INS_REG; ++k) { // (lengths and sources first: the one wait for them stands before the first insert's load)
        ib_n[k] = ins_in_regs ? __builtin_amdgcn_readlane(my_ins_len, k) : 0; // (a lane that is no insert holds 0)
        ib_src[k] = uint32_t(__builtin_amdgcn_readlane(int(my_ins_src), k));
    }
#pragma unroll
    for (int k = 0; k < F5_INS_REG; ++k) {
        ib[k] = SK_BAM_ANY;
        if (lane < ib_n[k]) ib[k] = a.ins_code[ib_src[k] + uint32_t(lane)];
    }
    // (every lane loads -- one without an alignment the record its slot_next names, 0 or a former round's, which nothing looks at:
    // a load that some lanes skip is merged with the registers' former values, and that merge waits for the load where it is issued)
    own.raw0 = f5_load_raw(a.pool + slot_next);
    // ---- the pool's bytes (as pool_fill_kernel), the read, its rows of terms, the pool's layout
    if (a.ref_outside && lane == 0) { // (the window's positions that lie outside the job's reference segment: they read as N)
        const int64_t b = max(int64_t(win_begin), int64_t(a.ref_offset));
        const int64_t e = min(int64_t(win_begin) + int64_t(win_len), int64_t(a.ref_offset) + int64_t(a.ref_len));
        const int32_t outside = win_len - int32_t(max(e - b, int64_t(0)));
        if (outside > 0) atomicAdd(a.ref_outside, outside);
    }
    {
        uint32_t* const hap_w = reinterpret_cast<uint32_t*>(S.hap);
        const int n_words = (P + 8 + 3) >> 2; // (at most HAP_WORDS - 1: the array holds F5_MAX_POOL + 12 bytes)
#pragma unroll
        for (int k = 0; k < HAP_K; ++k) {
            const int w = lane + 64 * k;
            const int keep = win_len - 4 * w; // bytes of the word that are the window's
            const uint32_t m = (keep >= 4) ? 0xffffffffu : (keep <= 0) ? 0u : ((1u << (8 * keep)) - 1u);
            if (w < n_words) hap_w[w] = (hw[k] & m) | (ANY4 & ~m);
        }
    }
    if (whole_tab) {
        if (lane < job_n_tab) S.tab[lane] = g;
        f5_wave_sync();
        // (the read's inserts are distinct table indices, pool_layout_kernel: a lane an insert, no two write the same entry)
        if (lane < n_ins && my_ins_idx < job_n_tab) S.tab[my_ins_idx].ins_at = my_ins_off;
    }
    f5_wave_sync();
    // the insert sequences, in table order (a later one overwrites an earlier one, as pool_fill_kernel)
    if (ins_in_regs) {
#pragma unroll
        for (int k = 0; k < F5_INS_REG; ++k) {
            if (k < n_ins) {
                const int32_t o = __builtin_amdgcn_readlane(my_ins_off, k), n = __builtin_amdgcn_readlane(my_ins_len, k);
                if (lane < n && o + lane < P) S.hap[o + lane] = uint8_t(ib[k]);
            }
        }
    } else {
        for (int k = 0; k < n_ins; ++k) {
            const int32_t o = __builtin_amdgcn_readlane(my_ins_off, k), n = __builtin_amdgcn_readlane(my_ins_len, k);
            const uint32_t src = uint32_t(__builtin_amdgcn_readlane(int(my_ins_src), k));
            for (int32_t i = lane; i < n; i += 64)
                if (o + i < P) S.hap[o + i] = a.ins_code[src + uint32_t(i)];
        }
    }
#pragma unroll
    for (int k = 0; k < READ_K; ++k) {
        const int32_t i = lane + 64 * k;
        if (i < L + 12) {
            unsigned q = rq[k];
            const uint8_t code = rc[k];
            if (q > 70u) { // the reference throws (qscore_cache.cpp:53-75): flagged, sk_check_device_errors reports it
                atomicOr(fa.err, unsigned(SK_DEVERR_QSCORE));
                q = 70u;
            }
            S.read[i] = code & 15u;
            if (i < L + 8) { // (the row of a '=' base adds its agree term either way, an N base and a pad row +0.0)
                const unsigned c = code & 15u;
                const bool adds = i < L && c != 15u;
                const double agree = adds ? q_terms[q] : 0.0;
                S.row[F5_ROW * i] = agree;
                S.row[F5_ROW * i + 1] = 0.0;
                S.row[F5_ROW * i + 2] = !adds ? 0.0 : (c == 0u) ? agree : q_terms[SK_NQ + 1 + q];
            }
        }
    }
    desc.r = r, desc.c0 = c0, desc.ncr = ncr, desc.L = L, desc.P = P, desc.win_begin = win_begin, desc.sorted_order = sorted_order ? 1 : 0;
    own.slot_next = slot_next;
    own.my_ins_idx = my_ins_idx;
    own.my_ins_off = my_ins_off;
    return true;
}

// the place of alignment 64 j + lane of the read in list[] (a round's lanes take the read's alignments in the set's order, or after the
// sort: the order's bytes lie past the pool's in the read's LDS object)
template <typename LDS>
__device__ __forceinline__ int f5_list_index(const LDS& D, const F5Desc& d, const int at)
{
    const uint8_t* const order = D.hap + ((d.P + 8 + 3) & ~3);
    return d.c0 + (d.sorted_order ? int(order[at]) : at);
}

// One round: alignments [64 j, 64 j + 64) of the read d, whose data the prologue left in D.  `mine`: the executing wave is the read's
// owner (D is its own LDS object); else it is a helper -- it reads D, writes its own slots (myslot), and has loaded own.slot_next at the
// round's start.  The owner's round 0 finds its records asked for by the prologue; every other round asks for them here.  `next_j` (the
// owner's): called between the walk and the sums, it names the owner's next round or -1, so that list[] of that round is asked for
// behind the sums.  Returns false where the round ends the read for this form (a record beyond the compact form, an index outside the
// table: counted in *n_unhandled, the staged chain takes the job).
template <int MAXR, bool TIMING, typename NextRound>
__device__ __forceinline__ bool f5_round(const FusedScoreArgs& fa, F5Lds<MAXR>& D, uint32_t* const slots, const F5Desc& d, const int j, const bool mine,
                                         F5Own& own, NextRound next_j, int& j_next)
{
    auto now = [&]() -> unsigned long long { return TIMING ? (unsigned long long)clock64() : 0ull; };
    const FlatArgs& a = fa.f;
    unsigned long long(&stamp)[F5_STAMPS] = own.stamp; // (a helper's rounds are not stamped: the stamps are a read's, stored by its owner)
    F5Lds<MAXR>& S = D;
    F5Raw& raw0 = own.raw0;
    int32_t& slot_next = own.slot_next;
    const int lane = threadIdx.x & 63;
    const int r = d.r, c0 = d.c0, ncr = d.ncr, job_n_tab = a.job.n_tab;
    const int32_t L = d.L, P = d.P, win_begin = d.win_begin;
    const int my_ins_idx = own.my_ins_idx;
    const int32_t my_ins_off = own.my_ins_off;
    const double ln_quarter = fa.tab->ln_quarter, ln_noncand = fa.tab->ln_noncand; // (asked for here, looked at by the sums)
    {
        const int j0 = 64 * j;
        const int nc = min(64, ncr - j0);
        f5_wave_sync(); // (pool and read complete; the previous round's slots read; the order written)
        const unsigned long long ta = now();
        if (mine && j0 == 0) stamp[1] = ta; // prologue done
        // ---- the round's records, a lane its own: header + F5_SEGS path segments (five 16-byte loads) + F5_INDELS indel indices, all in
        // flight at once; a record with more of either is left to the staged chain
        const bool has = lane < nc;
        uint32_t* const myslot = slots + lane * F5_SLOT;
        const bool whole_tab = job_n_tab <= F5_TAB; // (a helper's read is of such a job: only those are published)
        bool fits = true;
        const int my_j = has ? f5_list_index(S, d, j0 + lane) - c0 : 0; // the lane's alignment among the read's
        F5Rec rec;
        rec.w0 = rec.w1 = rec.w2 = 0;
        rec.types = 0;
        rec.l0 = rec.l1 = rec.l2 = rec.l3 = 0;
        rec.ind = 0;
        rec.ind_lo = 0;
        uint64_t ind_raw0 = 0, ind_raw1 = 0; // the record's eight 16-bit indel indices, until the round's table copy is placed
        if (!mine || j0 > 0) raw0 = f5_load_raw(a.pool + slot_next);
        if (has) {
            const F5Raw w = raw0;
            const uint4 q0 = w.q0, q1 = w.q1, q2 = w.q2, q3 = w.q3, q4 = w.q4;
            ind_raw0 = uint64_t(w.i0) | (uint64_t(w.i1) << 32);
            ind_raw1 = uint64_t(w.i2) | (uint64_t(w.i3) << 32);
            rec.w0 = q0.x;
            rec.w1 = q0.y;
            rec.w2 = q0.z;
            const unsigned nseg = (q0.z >> 8) & 0xffu, nind = (q0.z >> 16) & 0xffu;
            fits = (nseg <= unsigned(F5_SEGS) && nind <= unsigned(F5_INDELS));
            uint64_t types = 0;
            bool odd_type = false; // (not a segment type: the staged chain reports it)
            auto pack4 = [&](const uint32_t a0, const uint32_t a1, const uint32_t a2, const uint32_t a3, const int first) -> uint64_t {
                types |= (uint64_t(a0 & 15u) | (uint64_t(a1 & 15u) << 4) | (uint64_t(a2 & 15u) << 8) | (uint64_t(a3 & 15u) << 12)) << (4 * first);
                odd_type = odd_type || (unsigned(first) < nseg && (a0 & 0xffffu) > 15u) || (unsigned(first + 1) < nseg && (a1 & 0xffffu) > 15u) ||
                           (unsigned(first + 2) < nseg && (a2 & 0xffffu) > 15u) || (unsigned(first + 3) < nseg && (a3 & 0xffffu) > 15u);
                return uint64_t(a0 >> 16) | (uint64_t(a1 >> 16) << 16) | (uint64_t(a2 >> 16) << 32) | (uint64_t(a3 >> 16) << 48);
            };
            rec.l0 = pack4(q0.w, q1.x, q1.y, q1.z, 0);
            rec.l1 = pack4(q1.w, q2.x, q2.y, q2.z, 4);
            rec.l2 = pack4(q2.w, q3.x, q3.y, q3.z, 8);
            rec.l3 = pack4(q3.w, q4.x, q4.y, q4.z, 12);
            rec.types = types;
            fits = fits && !odd_type;
        }
        // the table entries this round's alignments name
        auto raw_indel = [&](const int k) -> int { return int(int16_t(((k & 4) ? ind_raw1 : ind_raw0) >> (16 * (k & 3)))); };
        int tab_lo = 0;
        if (whole_tab) {
            // the prologue's copy holds the job's table: tab_lo = 0, nothing to place per round
            bool out_of_table = false;
            if (has && fits) {
                auto check = [&](const int i) { out_of_table = out_of_table || i < 0 || i >= job_n_tab; };
                const int ni = rec.n_indels();
                for (int i = 0; i < ni; ++i) check(raw_indel(i));
                if (rec.lead() >= 0) check(rec.lead());
                if (rec.trail() >= 0) check(rec.trail());
            }
            // (a record beyond the compact form, an index that is none of the table's: the staged chain takes the job)
            if (__any((has && !fits) || out_of_table)) {
                if (lane == 0) {
                    atomicAdd(fa.n_unhandled, 1);
                    if (j > 0) atomicAdd(fa.shared_rounds + 1, 1u); // (diagnostics: a round after the read's first turned it down)
                }
                return false;
            }
            uint64_t ind = 0;
#pragma unroll
            for (int k = 0; k < F5_INDELS; ++k) ind |= uint64_t(unsigned(raw_indel(k)) & 63u) << (6 * k);
            rec.ind = ind;
            rec.ind_lo = 0;
        } else {
            int lo = INT_MAX, hi = INT_MIN;
            if (has && fits) {
                auto add = [&](const int i) {
                    lo = min(lo, i);
                    hi = max(hi, i);
                };
                const int ni = rec.n_indels();
                for (int i = 0; i < ni; ++i) add(raw_indel(i));
                if (rec.lead() >= 0) add(rec.lead());
                if (rec.trail() >= 0) add(rec.trail());
            }
#pragma unroll
            for (int d = 32; d > 0; d >>= 1) {
                lo = min(lo, __shfl_xor(lo, d));
                hi = max(hi, __shfl_xor(hi, d));
            }
            const int n_tab = (lo <= hi) ? hi - lo + 1 : 0;
            // (a record beyond the compact form, indices further apart than the copy holds: the staged chain takes the job)
            if (__any(has && !fits) || (n_tab > 0 && lo < 0) || n_tab > F5_TAB) {
                if (lane == 0) {
                    atomicAdd(fa.n_unhandled, 1);
                    if (j > 0) atomicAdd(fa.shared_rounds + 1, 1u); // (diagnostics: a round after the read's first turned it down)
                }
                return false;
            }
            tab_lo = n_tab ? lo : 0;
            // (every index of the round's records lies in [tab_lo, tab_lo + n_tab), n_tab <= F5_TAB: 6 bits relative to tab_lo)
            uint64_t ind = 0;
#pragma unroll
            for (int k = 0; k < F5_INDELS; ++k) ind |= uint64_t(unsigned(raw_indel(k) - tab_lo) & 63u) << (6 * k);
            rec.ind = ind;
            rec.ind_lo = tab_lo;
            if (lane < n_tab) { // (n_tab <= F5_TAB <= 32: a lane an entry)
                const PIndel& g = a.job.tab[tab_lo + lane];
                F5Tab e;
                e.pos = g.pos;
                e.del = g.del;
                e.ins_len = g.ins_len;
                e.type_cand = unsigned(g.type) | (unsigned(g.cand) << 8);
                e.ins_at = -1;
                S.tab[lane] = e;
            }
            f5_wave_sync();
            // (the read's inserts are distinct table indices, pool_layout_kernel: a lane an insert, no two write the same entry)
            if (my_ins_idx >= tab_lo && my_ins_idx < tab_lo + n_tab) S.tab[my_ins_idx - tab_lo].ins_at = my_ins_off;
        }
        f5_wave_sync();
        const unsigned long long tc = now();
        stamp[2] += tc - ta; // staging + table copy
        // ---- phase A, a lane per candidate alignment: the walk of its path leaves the alignment's TRANSITIONS in its slot: one word per
        // op that covers read positions, and one for the read's end
        int n_ent = 0;
        bool bad = false;
        bool cons_mine = false;
        uint8_t cons_seen = 1;
        {
            const unsigned long long tA0 = now();
            uint32_t cons = 0; // the table entries whose candidate status this lane's alignment consults: bit index - tab_lo
            n_ent = f5_walk_selects(S, rec, has, tab_lo, win_begin, cons, L, P, myslot);
            const unsigned long long tA1 = now();
            stamp[7] += tA1 - tA0; // the walk
            bad = n_ent < 0;
            if (has) {
                // the candidate-status lookups the host form performs for every indel of the alignment (cal_to_c)
                const int ni = rec.n_indels();
                for (int i = 0; i < ni; ++i) cons |= 1u << ((rec.indel(i) - tab_lo) & 31);
                if (rec.lead() >= 0) cons |= 1u << ((rec.lead() - tab_lo) & 31);
                if (rec.trail() >= 0) cons |= 1u << ((rec.trail() - tab_lo) & 31);
                if (bad) a.status[r] = ST_FAIL;
            }
            // the round's entries: one OR over the wave, lane t looks at entry tab_lo + t and marks it where it reads 0 (a stale 0 costs a
            // store of the 1 that is there already) -- a byte store per lane per indel stood in front of the next round's record loads
            if (a.job.consulted) {
#pragma unroll
                for (int d = 32; d > 0; d >>= 1) cons |= uint32_t(__shfl_xor(int(cons), d));
                cons_mine = lane < 32 && ((cons >> lane) & 1u) != 0u;
                if (cons_mine) cons_seen = a.job.consulted[tab_lo + lane];
            }
            (void)tA1;
        }
        // (the owner's next round, named before the sums: its list[] entries travel while they run)
        j_next = mine ? next_j() : -1;
        if (j_next >= 0 && 64 * j_next + lane < ncr) slot_next = a.list[f5_list_index(S, d, 64 * j_next + lane)];
        __builtin_amdgcn_wave_barrier();
        const unsigned long long td = now();
        stamp[4] += td - tc; // phase A
        // ---- phase B, a lane its alignment: the terms in path order (f5_sum)
        if (has && !bad) {
            const double lnp = f5_sum(S, myslot, n_ent, ln_noncand, ln_quarter);
            fa.scores[c0 + my_j] = lnp;
        }
        if (cons_mine && cons_seen == 0) a.job.consulted[tab_lo + lane] = 1;
        // (the record's registers are the next round's to load: nothing of them lives through the walk and the sums)
        raw0.q0 = raw0.q1 = raw0.q2 = raw0.q3 = raw0.q4 = make_uint4(0, 0, 0, 0);
        raw0.i0 = raw0.i1 = raw0.i2 = raw0.i3 = 0;
        stamp[5] += now() - td; // phase B
        if (mine) stamp[10] += 1; // (rounds the owner scored itself)
    }
    return true;
}

// $SK_F5_TIMING: the owner's last rounds are over -- the read's stamps go out (a round a helper still runs ends later: the stamps
// are the owner's time on the read)
template <bool TIMING>
__device__ __forceinline__ void f5_store_stamps(const FusedScoreArgs& fa, const int r, F5Own& own, const unsigned long long draw_cycles)
{
    if (TIMING && fa.dbg && (threadIdx.x & 63) == 0) { // (the build without the stamps has no store of them either)
        unsigned long long(&stamp)[F5_STAMPS] = own.stamp;
        stamp[6] = (unsigned long long)clock64();
        stamp[3] = (unsigned long long)wall_clock64() - own.wall0;
        stamp[8] = draw_cycles; // the draw that handed this read out, from before the atomic to its value in a scalar register (0: the
                                // wave's first read, which is not drawn)
        stamp[9] = own.wall0;
        for (int i = 0; i < F5_STAMPS; ++i) fa.dbg[size_t(r) * F5_STAMPS + i] = stamp[i];
    }
}

// A wave per read, WAVES waves to a block (each wave with an LDS object of its own, which it alone writes; at the launch's end a
// block-mate may read it: ROUND SHARING below).  With a block per
// read the kernel was bound by the rate at which the dispatcher places workgroups (65 536 one-wave blocks went out at ~30 per us, a block
// lives ~58 us: ~7 of a CU's 16 slots filled); eight waves to a block: 2.23 -> 1.67 ms per 65 536 reads (profiles/r05_f5_history.txt).
// The waves TAKE their reads from a queue (one counter, one atomic per read; a grid of the blocks the device holds at a time).  With read r
// bound to wave r a block lived as long as its heaviest read -- a read's work goes with its candidate alignments, a round of the wave per
// 64 -- and its other seven slots stood empty meanwhile: 7.5 waves to a CU on average (SQ_WAVE_CYCLES, profiles/r06_v28_pmc_traffic.json)
// where two such blocks, 16 waves, are resident (tools/diag/lds_residency.hip).  1.67 -> 1.23 ms.  Round 5's persistent grid (reads r, r + 4 096, ... to wave r: slower) had the
// same binding, only longer.  The queue's order is the job's: taking the heavy reads first, or the light ones last (lists by rounds of 64
// candidate alignments, filled by pool_layout_kernel), was tried against the launch's tail and is SLOWER (1.33-1.37 ms: reads of one kind
// side by side keep their waves in step -- all in their prologues, all in their walks -- where the job's own order mixes them;
// profiles/r06_f5_history.txt).  A wave's FIRST read is not drawn: wave g of the grid takes read g, and a draw hands out
// gridDim.x * WAVES + the counter's value.  All the grid's waves used to make their first draw on the one word within the ~15 us it takes
// to place the blocks, and a head word answers ~88 such atomics per us: the last of that burst waited ~45 us for its first read
// (1.025 -> 0.981 ms, profiles/r09_f5_history.txt; a later draw costs a wave 3 700 - 4 600 cycles at this load, the `draw` figure of
// $SK_F5_TIMING).  What is handed out is a number h; it names read h except among the launch's last hand-outs, whose reads are taken
// from a table in which the reads of several rounds stand earlier than in the job (tail_order_kernel, below).  A wave whose number is
// past the last read makes no draw.  The last wave to leave puts the queue back to zero -- every wave counts itself out after
// its last draw, whether it drew or not -- so that the next launch, the same buffers, the same stream, finds it as this one did.
//
// ROUND SHARING.  The launch used to end a heavy read's life after its last hand-out (~135 us of ~0.92 ms, profiles/r10_f5_history.txt): a
// read of three or four rounds drawn late keeps one wave busy while its block-mates have left.  Now a wave that has drawn DRY does not
// leave: it takes whole rounds of reads owned by waves of its own block.  The owner's prologue has left the read, the pool, the order, the
// rows of terms and the table copy in its LDS object, which nothing writes again before the owner's next prologue; the helper reads them
// where they lie and writes its own slots, so no second prologue runs and nothing but the round's own records is read from HBM.
//   publication  A read of more than one round in a job whose table fits the copy (whole_tab: else the table copy is written per round
//                and the read is not shared) is published after the prologue's last LDS write: a workgroup release fence by every
//                lane (each wrote part of the data), then lane 0's descriptor stores, its release fence, and one atomic store of
//                the wave's claim word {next round = 1 | rounds << 16}.
//   claims       A round is claimed by an LDS atomic add of 1 on the claim word; the old value names the round if its low half is below
//                the high half.  The owner claims the same way, between a round's walk and its sums (list[] of its next round
//                travels behind the sums, as before); round 0 is always its own (its records are asked for in the prologue, and the
//                list[] entries parked in its slots die with its first walk).  A helper reads the word first and adds only where a
//                round is open, so a word over-counts by at most the block's waves (rounds < 2^15: the halves do not meet).  After a
//                claim the helper makes an acquire fence, reads the descriptor, asks for list[] of the round and then its records.
//   helpers      `busy` counts the block's waves that have not drawn dry.  A dry wave polls its block-mates' claim words -- never its
//                own -- with s_sleep F5_HELP_NAP between looks, and leaves when busy == 0 (an owner draws dry only after every round
//                of its read is claimed, or its word is closed: nothing is open then) or F5_HELP_CAP ticks of the constant 100 MHz
//                counter (20 ms) after it drew dry.
//   closing      A word is open only while its read is the one in the owner's LDS object.  A read that goes through uses its word
//                up (the owner's last claim finds no round left).  An owner that leaves a published read EARLY -- a round of its
//                own turned the read down -- stores 0 into its word before it draws: left open, the word would outlive a draw
//                that hands out a read, and a wave that drew dry later would score the dead read's rounds over the new read's data.
// NO WAVE EVER WAITS FOR ANOTHER TO DO SOMETHING.  An owner does not wait for helpers: it claims until its word is used up, scores what
// it claimed, and goes on to draw.  A helper may leave at any moment: what nobody claimed the owner scores.  A helper's reads of an
// owner's LDS object are safe without any wait, because the queue's counter only grows: once any wave of the launch has drawn dry
// (n_waves + counter >= n_reads; a wave whose own number is past the last read implies n_waves >= n_reads), every later draw is dry
// too -- the helper's dry draw returned before it claimed, the owner's next draw is issued after its own last claim or after it closed
// its word -- so an owner never runs another prologue while a helper that claimed from its word can be reading its object, and after
// that draw the word gives nothing out; and a block's LDS lives until its last wave leaves, after the helper.  There is no waiting across blocks, no barrier after the first, no spin without the cap.  What ends a round early (a
// record outside the compact form: *n_unhandled, which the drivers test for > 0) or marks the read (ST_FAIL) a helper records as the
// owner would, and goes on polling.  Rounds a helper SCORED (not those it was turned down in) are counted in *shared_rounds, one
// atomic each (the tail pays it).
// $SK_F5_SHARE=0 (FusedScoreArgs::share = 0): nothing is published, a dry wave leaves at once, the kernel runs as it did.
constexpr int F5_HELP_NAP = 64; // s_sleep between a dry wave's looks: ~4 000 cycles, under 2 us -- a fifth of a round
constexpr unsigned F5_HELP_CAP = 2000000u; // ticks of the 100 MHz counter a dry wave stays at most: 20 ms
template <int MAXR, bool TIMING, int WAVES>
__global__ __launch_bounds__(64 * WAVES) __attribute__((amdgpu_waves_per_eu(4, 4))) void flatten_score_kernel(const FusedScoreArgs fa, const int n_reads)
{
    __shared__ __attribute__((aligned(16))) F5Lds<MAXR> S[WAVES];
    // the two terms of every quality, once per block (every wave reaches the barrier: it stands before the first draw)
    __shared__ double q_terms[F5_Q_TERMS];
    __shared__ F5Share share[WAVES];
    __shared__ unsigned busy;
    for (int i = threadIdx.x; i < F5_Q_TERMS; i += 64 * WAVES) q_terms[i] = (i <= SK_NQ) ? fa.tab->q2lncompe[i] : fa.tab->q2mis[i - (SK_NQ + 1)];
    if (threadIdx.x < unsigned(WAVES)) share[threadIdx.x].claim = 0u, share[threadIdx.x].dry_at = 0u; // (nothing open, nobody dry)
    if (threadIdx.x == 0) busy = unsigned(WAVES);
    __syncthreads();
    const int wave = __builtin_amdgcn_readfirstlane(int(threadIdx.x >> 6)), lane = threadIdx.x & 63;
    const unsigned n_waves = gridDim.x * unsigned(WAVES);
    // a read of `ncr` candidate alignments is published: sharing is on, the job's table fits the copy, more than one round
    auto published = [&](const int ncr) -> bool { return WAVES > 1 && fa.share != 0 && fa.f.job.n_tab <= F5_TAB && ncr > 64 && ncr < (0x8000 << 6); };
    // the first hand-out: the wave's own number, no draw
    unsigned h = unsigned(__builtin_amdgcn_readfirstlane(int(blockIdx.x * unsigned(WAVES) + unsigned(wave))));
    unsigned long long draw_cycles = 0;
    auto draw = [&]() {
        f5_wave_sync(); // (the wave's LDS object is the next read's)
        const unsigned long long t0 = TIMING ? (unsigned long long)clock64() : 0ull;
        unsigned got = 0;
        if (lane == 0) got = atomicAdd(&fa.queue[0], 1u);
        int drawn = __builtin_amdgcn_readfirstlane(int(got));
        if (TIMING) __asm__ volatile("" : "+s"(drawn)); // (the second stamp stands after the value has arrived)
        h = n_waves + unsigned(drawn);
        draw_cycles = TIMING ? (unsigned long long)clock64() - t0 : 0ull;
    };
    F5Desc d; // the read whose round comes next: the wave's own, or a block-mate's
    F5Own own;
    d.r = d.c0 = d.ncr = d.L = d.P = d.win_begin = d.sorted_order = 0;
    int j = -1, src = wave; // the round to run (-1: none); the wave whose LDS object holds the read (the wave's own: it is the owner)
    for (;;) {
        if (j < 0 && h < unsigned(n_reads)) { // ---- the owner's next read
            // hand-out h is read h, except among the launch's last tail_n hand-outs, which go through the table (the same for the whole
            // wave; one more dependent load, paid by those hand-outs only)
            unsigned r = h;
            if (h - fa.tail_first < fa.tail_n) r = unsigned(__builtin_amdgcn_readfirstlane(fa.tail_order[h - fa.tail_first]));
            if (!f5_prologue<MAXR, TIMING>(fa, int(r), S[wave], q_terms, d, own)) {
                draw();
                continue;
            }
            j = 0;
            if (published(d.ncr)) {
                // (every lane wrote part of the prologue's data: every lane releases its stores, before lane 0 alone writes the
                // descriptor and, behind a release of its own, the word)
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
                __builtin_amdgcn_wave_barrier();
                if (lane == 0) {
                    share[wave].d = d;
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
                    __hip_atomic_store(&share[wave].claim, 1u | (unsigned((d.ncr + 63) >> 6) << 16), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                }
            }
        } else if (j < 0) { // ---- a dry wave (h is past the last read and stays there: no further draw): a round of a block-mate's read
            // (when it drew dry is kept in LDS, and the lane is taken anew: neither is a register's through the owners' rounds)
            unsigned dry_at = unsigned(__builtin_amdgcn_readfirstlane(int(share[wave].dry_at)));
            if (dry_at == 0u) {
                if (lane == 0) __hip_atomic_fetch_add(&busy, ~0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                if (!(WAVES > 1 && fa.share != 0)) break;
                dry_at = unsigned(wall_clock64()) | 1u;
                if (lane == 0) share[wave].dry_at = dry_at;
            }
            int look = threadIdx.x & 63;
            __asm__ volatile("" : "+v"(look));
            unsigned w = 0;
            if (look < WAVES && look != wave) w = __hip_atomic_load(&share[look].claim, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); // (never its own)
            const unsigned long long open = __ballot((w & 0xffffu) < (w >> 16));
            if (open == 0ull) {
                const unsigned left = __hip_atomic_load(&busy, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                if (__builtin_amdgcn_readfirstlane(int(left)) == 0 || unsigned(wall_clock64()) - dry_at > F5_HELP_CAP) break;
                __builtin_amdgcn_s_sleep(F5_HELP_NAP);
                continue;
            }
            const int o = __builtin_amdgcn_readfirstlane(__builtin_ctzll(open)); // (< WAVES: only those lanes looked)
            unsigned old = 0;
            if (lane == 0) old = __hip_atomic_fetch_add(&share[o].claim, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            old = unsigned(__builtin_amdgcn_readfirstlane(int(old)));
            if ((old & 0xffffu) >= (old >> 16)) continue; // (taken meanwhile: look again)
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
            const F5Desc& p = share[o].d;
            d.r = __builtin_amdgcn_readfirstlane(p.r), d.c0 = __builtin_amdgcn_readfirstlane(p.c0), d.ncr = __builtin_amdgcn_readfirstlane(p.ncr);
            d.L = __builtin_amdgcn_readfirstlane(p.L), d.P = __builtin_amdgcn_readfirstlane(p.P);
            d.win_begin = __builtin_amdgcn_readfirstlane(p.win_begin), d.sorted_order = __builtin_amdgcn_readfirstlane(p.sorted_order);
            j = int(old & 0xffffu), src = o;
            // (what the owner gets a round ahead: list[] of the round; a lane without an alignment names record 0, which nothing looks at)
            own.slot_next = (64 * j + lane < d.ncr) ? fa.f.list[f5_list_index(S[src], d, 64 * j + lane)] : 0;
            own.my_ins_idx = -1, own.my_ins_off = 0;
        }
        const bool mine = src == wave;
        int j_next = -1;
        const bool went = f5_round<MAXR, TIMING>(
            fa, S[src], S[wave].slot, d, j, mine, own,
            [&]() -> int { // the owner's next round: the one after this, or, of a published read, the next that nobody has claimed
                int nj = j + 1;
                if (published(d.ncr)) {
                    unsigned old = 0;
                    if (lane == 0) old = __hip_atomic_fetch_add(&share[wave].claim, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    nj = __builtin_amdgcn_readfirstlane(int(old)) & 0xffff;
                }
                return 64 * nj < d.ncr ? nj : -1;
            },
            j_next);
        if (!mine && went && lane == 0) atomicAdd(fa.shared_rounds, 1u); // (a helped round that was scored)
        j = (mine && went) ? j_next : -1;
        if (mine && j < 0) { // (the owner's last round, or the round that left the read to the staged chain)
            if (went) f5_store_stamps<TIMING>(fa, d.r, own, draw_cycles);
            // The owner leaves a published read EARLY: it closes its word before it draws.  A round claimed before the store is a
            // helper's, and a helper has drawn dry, so the draw below is dry too (the argument above); after the store nothing can be
            // claimed, and if the draw hands out a read, its prologue writes an object that no word points at.  (A read that went
            // through needs no store: its word is used up, the owner's last claim found it so.)
            else if (published(d.ncr) && lane == 0) __hip_atomic_store(&share[wave].claim, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            draw();
        }
    }
    if (lane == 0) {
        __threadfence();
        if (atomicAdd(&fa.queue[1], 1u) == gridDim.x * unsigned(WAVES) - 1u) { // (every wave has made its last draw)
            fa.queue[0] = 0u;
            fa.queue[1] = 0u;
        }
    }
}

// the rows of terms sized for the job's longest read: with 150-base reads a wave's LDS is 10 KB, sixteen waves to a CU (the 256-base
// form: twelve)
// eight waves to a block where their LDS leaves room for two blocks to a CU (the short-read form: 76.7 KB), four with the long form
// the launch's shape, computed in one place for the launch and for the table of its last hand-outs: the waves of a block and the
// blocks of the grid.  waves() is W, the reads handed out without a draw.
struct F5Grid
{
    int wpb, blocks;
    int waves() const { return wpb * blocks; }
};
template <int MAXR>
static F5Grid f5_grid_t(const int n_reads)
{
    static const int waves = [] { const char* e = std::getenv("SK_F5_WAVES"); return e ? std::atoi(e) : 0; }(); // (experiments: 1, 2, 4, 8, 16; 0 = the default)
    constexpr int DEFAULT_WAVES = (sizeof(F5Lds<MAXR>) * 16 <= 160 * 1024) ? 8 : 4;
    const int w = waves > 0 ? waves : DEFAULT_WAVES;
    const int wpb = (w == 16 && MAXR <= 152) ? 16 : w >= 8 ? 8 : w == 4 ? 4 : w == 2 ? 2 : 1; // (the instantiations there are)
    // the blocks the device holds at a time (256 CUs; by LDS: 16 waves of the short-read form to a CU, 14 of the long one; a grid larger
    // than that only queues blocks that find the read queue empty, a smaller one leaves slots unused): $SK_F5_GRID = blocks, experiments
    static const int grid_env = [] { const char* e = std::getenv("SK_F5_GRID"); return e ? std::atoi(e) : 0; }();
    constexpr int WAVES_PER_CU = int((160 * 1024) / sizeof(F5Lds<MAXR>)) >= 16 ? 16 : int((160 * 1024) / sizeof(F5Lds<MAXR>));
    const int resident = grid_env > 0 ? grid_env : 256 * std::max(1, WAVES_PER_CU / wpb);
    return { wpb, std::max(1, std::min(resident, (n_reads + wpb - 1) / wpb)) };
}
static F5Grid f5_grid(const int n_reads, const int max_read_len) // (the form launch_flatten_score takes for the job)
{
    return max_read_len <= 152 ? f5_grid_t<152>(n_reads) : f5_grid_t<F5_MAX_READ>(n_reads);
}

template <int MAXR, bool TIMING>
static void launch_flatten_score_t(const int n_reads, hipStream_t st, const FusedScoreArgs& fs)
{
    const F5Grid g = f5_grid_t<MAXR>(n_reads);
    const dim3 grid(unsigned(g.blocks)), block(unsigned(64 * g.wpb));
    if (g.wpb == 16) SK_LAUNCH((flatten_score_kernel<152, TIMING, 16>), grid, block, 0, st, fs, n_reads);
    else if (g.wpb == 8) SK_LAUNCH((flatten_score_kernel<MAXR, TIMING, 8>), grid, block, 0, st, fs, n_reads);
    else if (g.wpb == 4) SK_LAUNCH((flatten_score_kernel<MAXR, TIMING, 4>), grid, block, 0, st, fs, n_reads);
    else if (g.wpb == 2) SK_LAUNCH((flatten_score_kernel<MAXR, TIMING, 2>), grid, block, 0, st, fs, n_reads);
    else SK_LAUNCH((flatten_score_kernel<MAXR, TIMING, 1>), grid, block, 0, st, fs, n_reads);
}

static void launch_flatten_score(const int n_reads, hipStream_t st, const FusedScoreArgs& fs)
{
    const bool short_reads = fs.f.max_read_len <= 152, timing = fs.dbg != nullptr;
    if (short_reads && !timing) launch_flatten_score_t<152, false>(n_reads, st, fs);
    else if (short_reads) launch_flatten_score_t<152, true>(n_reads, st, fs);
    else if (!timing) launch_flatten_score_t<F5_MAX_READ, false>(n_reads, st, fs);
    else launch_flatten_score_t<F5_MAX_READ, true>(n_reads, st, fs);
}

// ---- host diagnostics
struct EventPair // two events of a timed stretch, destroyed on every way out
{
    hipEvent_t a = nullptr, b = nullptr;
    int create()
    {
        SK_HIP(hipEventCreate(&a));
        SK_HIP(hipEventCreate(&b));
        return 0;
    }
    ~EventPair()
    {
        if (a) (void)hipEventDestroy(a);
        if (b) (void)hipEventDestroy(b);
    }
};

// diagnostics ($SK_F5_TIMING): where a wave of F5 spends its cycles on the last run's job, and how the kernel's time grows with the grid
// (the stamps' indices: F5_STAMPS, f5_store_stamps).  last_fs, n: the launch of the last run's job; cal_off: the job's offsets, on the host
int f5_timing_report(hipStream_t st, const FusedScoreArgs& last_fs, const int n, const int32_t* const cal_off)
{
    FusedScoreArgs fs = last_fs;
    const size_t nb = size_t(n) * F5_STAMPS;
    SkDevBuf dbg; // (this report's own: dropped below)
    if (dbg.reserve(nb * 8)) return 1;
    unsigned long long* d = dbg.as<unsigned long long>();
    SK_HIP(skrt::memsetAsync(d, 0, nb * 8, st));
    fs.dbg = d;
    unsigned helped[2] = { 0, 0 }; // the job's count of helped rounds before and after this launch
    SK_HIP(skrt::memcpyAsync(&helped[0], fs.shared_rounds, 4, hipMemcpyDeviceToHost, st));
    launch_flatten_score(n, st, fs);
    SK_HIP(skrt::memcpyAsync(&helped[1], fs.shared_rounds, 4, hipMemcpyDeviceToHost, st));
    std::vector<unsigned long long> h(nb);
    SK_HIP(skrt::memcpyAsync(h.data(), d, nb * 8, hipMemcpyDeviceToHost, st));
    SK_HIP(skrt::streamSynchronize(st));
    dbg.drop();
    { // the rounds of the reads that were scored (a stamped read: its owner went through all it claimed), by who scored them
        long long by_owner = 0, implied = 0;
        for (int r = 0; r < n; ++r) {
            const unsigned long long* s = &h[size_t(r) * F5_STAMPS];
            if (s[6] == 0) continue;
            by_owner += (long long)s[10];
            implied += (cal_off[r + 1] - cal_off[r] + 63) / 64;
        }
        std::fprintf(stderr, "[f5-timing] rounds: %lld scored by their owners + %u by helpers = %lld; cal_off implies %lld (sharing %s)\n", by_owner,
                     helped[1] - helped[0], by_owner + (long long)(helped[1] - helped[0]), implied, fs.share ? "on" : "off");
    }
    double sum[F5_STAMPS] = { 0 };
    unsigned long long first = ~0ull, last = 0;
    int nblk = 0, ndrawn = 0;
    for (int r = 0; r < n; ++r) {
        const unsigned long long* s = &h[size_t(r) * F5_STAMPS];
        if (s[6] == 0) continue;
        ++nblk;
        first = std::min(first, s[0]);
        last = std::max(last, s[6]);
        sum[0] += double(s[1] - s[0]);
        for (int i = 2; i <= 5; ++i) sum[i] += double(s[i]);
        sum[7] += double(s[7]);
        sum[6] += double(s[6] - s[0]);
        sum[8] += double(s[8]);
        ndrawn += s[8] != 0;
    }
    for (const int grid : { 64, 256, 512, 1024, 1792, 2048, 4096 }) { // how the kernel's time grows with the blocks in flight
        if (grid > n) break;
        EventPair ev;
        if (ev.create()) return 1;
        FusedScoreArgs f2 = last_fs;
        f2.tail_n = 0; // (the table is the whole job's: these launches end before its window)
        launch_flatten_score(grid, st, f2);
        SK_HIP(hipEventRecord(ev.a, st));
        for (int k = 0; k < 5; ++k) launch_flatten_score(grid, st, f2);
        SK_HIP(hipEventRecord(ev.b, st));
        SK_HIP(hipEventSynchronize(ev.b));
        float ms = 0;
        SK_HIP(hipEventElapsedTime(&ms, ev.a, ev.b));
        std::fprintf(stderr, "[f5-timing] grid %d blocks: %.1f us per launch\n", grid, ms * 1000.f / 5.f);
    }
    if (nblk)
        std::fprintf(stderr, "[f5-timing] blocks %d: cycles per block: draw %.0f (%d drawn: %.0f each) prologue %.0f staging %.0f phaseA %.0f (walk %.0f) phaseB %.0f total %.0f = %.1f us by the 100 MHz counter (%.0f MHz); kernel span %llu cycles => %.1f blocks in flight\n",
                     nblk, sum[8] / nblk, ndrawn, sum[8] / std::max(1, ndrawn), sum[0] / nblk, sum[2] / nblk, sum[4] / nblk, sum[7] / nblk, sum[5] / nblk, sum[6] / nblk, sum[3] / nblk / 100.0,
                     sum[6] / std::max(1.0, sum[3]) * 100.0, last - first,
                     sum[6] / double(last - first));
    // the drain, by the 100 MHz counter (a read's start is its tenth stamp, its duration the fourth): when the last read was handed
    // out, when the launch's last read ended, and how long a slot stood empty at the end -- over the W reads that started last (the
    // last read of each of the grid's W waves, or nearly), the mean of (the launch's end - the read's end)
    std::vector<std::pair<unsigned long long, unsigned long long>> span; // (start, end) of every stamped read
    for (int r = 0; r < n; ++r) {
        const unsigned long long* s = &h[size_t(r) * F5_STAMPS];
        if (s[6] != 0) span.emplace_back(s[9], s[9] + s[3]);
    }
    if (!span.empty()) {
        std::sort(span.begin(), span.end());
        const unsigned long long w0 = span.front().first;
        unsigned long long w1 = 0;
        for (const auto& x : span) w1 = std::max(w1, x.second);
        const size_t W = size_t(f5_grid(n, fs.f.max_read_len).waves()), n_last = std::min(W, span.size());
        double idle = 0;
        for (size_t i = span.size() - n_last; i < span.size(); ++i) idle += double(w1 - span[i].second);
        std::fprintf(stderr, "[f5-timing] drain: tail window %u hand-outs; last read handed out at %.1f us, last read ended at %.1f us; over the %zu reads that started last a slot stood empty for %.1f us on average\n",
                     fs.tail_n, double(span.back().first - w0) / 100.0, double(w1 - w0) / 100.0, n_last, idle / double(n_last) / 100.0);
    }
    return 0;
}

} // namespace
