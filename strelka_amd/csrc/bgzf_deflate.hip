// bgzf_deflate.hip -- the feed's way out: BGZF compression on the device (the counterpart of bam_feed.hip's inflate kernels).
//
// What a caller process writes ends up as BGZF: the per-segment VCF / gVCF files the workflow bgzips, the realigned-read BAM.  A BGZF
// file is a chain of independent gzip members of at most 64 KiB (SAM specification v1, section 4.1), each holding at most 65 280 input
// bytes (bgzip's own cut), so the mapping is the one B1s uses for the other direction: a WAVE per block.
//
//   D1  bgzf_deflate_kernel<level>   one wave per block.  level 0 stores; levels 1 and 2 run an LZ77 match finder (one probe of a
//       hash-head table in LDS over 4-byte prefixes, 64 consecutive positions per turn, greedy parse) into a token stream kept in an HBM
//       slot of the block's own, count literal/length and distance symbols, and then price the encodings the level allows from exact bit
//       counts -- stored, the fixed code (RFC 1951 3.2.6), at level 2 a dynamic code built here (3.2.7) -- BEFORE anything is emitted: the
//       smallest is written, so per block level 2 <= level 1 <= level 0 and a block never outgrows its 65 536-byte slot.  The CRC-32 of
//       the block (table in LDS, 64 slices combined as bgzf_inflate_scalar_kernel does) is folded in.
//   D2  bgzf_block_scan_kernel       inclusive scan of the member lengths -> block_end
//   D3  bgzf_pack_kernel             slot -> contiguous stream, plus the 28-byte EOF block
//
// Determinism: where lanes of one turn hash to the same slot, the HIGHEST lane (the latest position) is the one that writes, and a
// lane's candidate is the nearest lower lane of the turn with its slot, else what the table held before the turn.  Both follow from a
// ballot per hash bit; no result depends on the order in which LDS writes land.  Counters are integer LDS atomics (add / or), which
// commute.
#include "sk_common.h"

#include <cstdlib>
#include <vector>

namespace
{

enum {
    BD_IN = SK_BGZF_BLOCK_INPUT,
    BD_SLOT = SK_BGZF_BLOCK_MAX,
    BD_HASH_BITS = 13,
    BD_HASH = 1 << BD_HASH_BITS,
    BD_EMPTY = 0xffff, // (positions in a block stay below 65 280)
    BD_MAX_MATCH = 258,
    BD_WINDOW = 32768,
    BD_NLL = 286,
    BD_ND = 30,
    BD_NCL = 19,
    BD_STAGE = 128,         // words of the emitter's staging row: 31 carried bits + 64 lanes x at most 56 bits
    BD_LAUNCH_BLOCKS = 1024 // blocks per launch: the token slots (255 KiB each) are per launch, not per block of the input
};
enum { BD_STORED = 0, BD_FIXED = 1, BD_DYNAMIC = 2 };

struct DeflateArgs
{
    const uint8_t* data;
    int64_t n_bytes;
    int32_t first_block, n_blocks; // this launch covers blocks [first_block, min(n_blocks, first_block + gridDim.x))
    uint8_t* slots;                // [n_blocks][BD_SLOT]
    uint32_t* tokens;              // [gridDim.x][BD_IN]
    int32_t* slot_len;             // [n_blocks] member length; -1 = the emitted size differs from the priced one (a bug, reported by the host entry)
};

// the code-length code's transmission order (RFC 1951 3.2.7)
__device__ const uint8_t BD_CL_ORDER[BD_NCL] = { 16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15 };

struct HuffWork // lives where the hash heads were: the match finder is done when a code is built
{
    uint32_t key[320];   // (weight << 9 | symbol) of the used symbols, for the rank sort
    uint32_t weight[640]; // leaves in ascending order, then the internal nodes in the order they are made
    uint16_t parent[640];
    uint8_t depth[640];
    uint16_t cl_tok[320]; // run-length symbols of the two length arrays: symbol | extra << 5
    int32_t bl_count[16];
    int32_t n_cl_tok, hlit, hdist, hclen;
};

struct DeflateLds
{
    uint32_t crc_table[256];
    uint32_t ll_freq[320];
    uint32_t d_freq[64];
    uint32_t cl_freq[64];
    uint16_t ll_code[320], d_code[64], cl_code[64]; // bit-reversed: DEFLATE packs Huffman codes from their most significant bit
    uint8_t ll_len[320], d_len[64], cl_len[64];
    uint32_t stage[BD_STAGE];
    union {
        uint16_t head[BD_HASH];
        HuffWork hw;
    } u;
};

__device__ __forceinline__ uint32_t bd_ld32(const uint8_t* p)
{
    uint32_t v;
    __builtin_memcpy(&v, p, 4);
    return v;
}
__device__ __forceinline__ uint64_t bd_ld64(const uint8_t* p)
{
    uint64_t v;
    __builtin_memcpy(&v, p, 8);
    return v;
}
__device__ __forceinline__ uint64_t bd_below(const int k) { return k >= 64 ? ~0ull : ((1ull << k) - 1ull); }

__device__ __forceinline__ int bd_wave_sum(int v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

// length - 3 (0..255) -> length code 0..28 (symbol 257 + code) and its extra bits
__device__ __forceinline__ int bd_len_code(const int l, int* extra_bits)
{
    if (l < 8) { *extra_bits = 0; return l; }
    if (l == 255) { *extra_bits = 0; return 28; }
    const int e = (31 - __clz(l)) - 2;
    *extra_bits = e;
    return 4 + 4 * e + ((l >> e) & 3);
}
// distance - 1 (0..32767) -> distance code 0..29 and its extra bits
__device__ __forceinline__ int bd_dist_code(const int d, int* extra_bits)
{
    if (d < 4) { *extra_bits = 0; return d; }
    const int e = (31 - __clz(d)) - 1;
    *extra_bits = e;
    return 2 * e + 2 + ((d >> e) & 1);
}
__device__ __forceinline__ int bd_ll_extra(const int sym) // extra bits of a literal/length symbol
{
    const int i = sym - 257;
    return (i < 8 || i >= 28) ? 0 : (i >> 2) - 1;
}
__device__ __forceinline__ int bd_d_extra(const int code) { return code < 4 ? 0 : (code >> 1) - 1; }
__device__ __forceinline__ int bd_fixed_ll_len(const int sym) { return sym < 144 ? 8 : sym < 256 ? 9 : sym < 280 ? 7 : 8; }
__device__ __forceinline__ uint32_t bd_rev(const uint32_t code, const int len) { return len ? (__brev(code) >> (32 - len)) : 0u; }

// a * b mod P over GF(2), reflected (zlib crc32.c multmodp), as bam_feed.hip's wave kernel has it
__device__ __forceinline__ uint32_t bd_multmodp(uint32_t a, uint32_t b)
{
    uint32_t m = 1u << 31, p = 0;
    for (;;) {
        if (a & m) {
            p ^= b;
            if ((a & (m - 1u)) == 0) break;
        }
        m >>= 1;
        b = (b & 1u) ? ((b >> 1) ^ 0xedb88320u) : (b >> 1);
    }
    return p;
}

// CRC-32 of in[0, n): 64 slices, slice i shifted by the bytes after it (crc(A || B) = crc(A) * x^(8 |B|) + crc(B))
__device__ uint32_t bd_crc32(const DeflateLds& L, const uint8_t* in, const int n, const int lane)
{
    const int slice = (((n + 63) / 64) + 3) & ~3;
    const int s0 = min(n, lane * slice), s1 = min(n, s0 + slice);
    uint32_t c = 0;
    if (s1 > s0) {
        c = 0xffffffffu;
        int i = s0;
        for (; i + 4 <= s1; i += 4) {
            const uint32_t w = bd_ld32(in + i);
            c = L.crc_table[(c ^ w) & 0xffu] ^ (c >> 8);
            c = L.crc_table[(c ^ (w >> 8)) & 0xffu] ^ (c >> 8);
            c = L.crc_table[(c ^ (w >> 16)) & 0xffu] ^ (c >> 8);
            c = L.crc_table[(c ^ (w >> 24)) & 0xffu] ^ (c >> 8);
        }
        for (; i < s1; ++i) c = L.crc_table[(c ^ in[i]) & 0xffu] ^ (c >> 8);
        c ^= 0xffffffffu;
        uint32_t sq = 1u << 30; // x^1
        uint32_t pw = 1u << 31; // x^0
        uint32_t e = uint32_t(n - s1) * 8u;
        while (e) {
            if (e & 1u) pw = bd_multmodp(sq, pw);
            sq = bd_multmodp(sq, sq);
            e >>= 1;
        }
        c = bd_multmodp(pw, c);
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) c ^= __shfl_xor(c, d, 64);
    return c;
}

// The bit writer.  Every lane hands over up to 56 bits; a wave-wide prefix sum of the lengths tells each lane where its bits start, the
// pieces are or-ed into a row of words in LDS, and the words that are complete leave as 32-bit vector stores.  The unfinished word is
// carried in stage[0].  Every store is bounded by the block's slot.
struct BitWriter
{
    uint32_t* words; // the block's slot
    int wpos;        // next word of the slot to be written
    int fill;        // bits of stage[0] in use (0..31)
};

__device__ void bd_emit(DeflateLds& L, BitWriter& bw, const uint64_t v, const int nb, const int lane)
{
    int incl = nb;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int t = __shfl_up(incl, d, 64);
        if (lane >= d) incl += t;
    }
    const int total = __builtin_amdgcn_readlane(incl, 63);
    if (total == 0) return;
    const int off = bw.fill + incl - nb;
    const int w = off >> 5, sh = off & 31;
    if (nb > 0) {
        atomicOr(&L.stage[w], uint32_t(v << sh));
        const uint64_t hi = sh ? (v >> (32 - sh)) : (v >> 32);
        if (sh + nb > 32) atomicOr(&L.stage[w + 1], uint32_t(hi));
        if (sh + nb > 64) atomicOr(&L.stage[w + 2], uint32_t(hi >> 32));
    }
    __syncthreads();
    const int end = bw.fill + total;
    const int nwords = end >> 5; // < BD_STAGE - 1: at most 31 + 64 * 56 bits
    for (int i = lane; i < nwords; i += 64)
        if (bw.wpos + i < BD_SLOT / 4) bw.words[bw.wpos + i] = L.stage[i];
    const uint32_t carry = L.stage[nwords];
    __syncthreads();
    for (int i = lane; i <= nwords + 1 && i < BD_STAGE; i += 64) L.stage[i] = (i == 0) ? carry : 0u;
    __syncthreads();
    bw.wpos += nwords;
    bw.fill = end & 31;
}

// Code lengths of a prefix code over `freq[0, n_sym)`, at most `max_bits` long, and its canonical codes.  Used symbols are ranked by
// (weight, symbol); one lane merges them with the two-queue method (the leaves are sorted, the internal nodes come out sorted), counts
// the leaves per depth, folds depths past max_bits into max_bits and repairs the Kraft sum one unit at a time (each step moves the
// deepest shorter leaf one level down and gives it a leaf from the last level as its sibling); the lengths then go to the symbols
// longest first in ascending weight, which is optimal for the multiset of lengths.  A code with fewer than two used symbols is padded
// with symbol 0 / 1 at weight 1, as zlib does, so that every code is complete.  CH = ceil(n_sym / 64).
template <int CH> __device__ void bd_build_code(DeflateLds& L, const uint32_t* freq, const int n_sym, const int max_bits, uint8_t* len_out,
                                                uint16_t* code_out, const int lane)
{
    HuffWork& H = L.u.hw;
    uint32_t f[CH];
    int used = 0;
#pragma unroll
    for (int c = 0; c < CH; ++c) {
        const int s = lane + 64 * c;
        f[c] = s < n_sym ? freq[s] : 0u;
        used += __popcll(__ballot(f[c] != 0));
    }
    if (used < 2) {
        const bool has0 = __builtin_amdgcn_readlane(int(f[0]), 0) != 0;
        if (lane == 0 && !has0) f[0] = 1;
        if (lane == 1 && (has0 || used == 0)) f[0] = max(f[0], 1u);
        used = 2;
    }
    const int n = used;
#pragma unroll
    for (int c = 0; c < CH; ++c) {
        const int s = lane + 64 * c;
        if (s < 320) H.key[s] = f[c] ? ((f[c] << 9) | uint32_t(s)) : 0xffffffffu;
    }
    __syncthreads();
    int rank[CH];
#pragma unroll
    for (int c = 0; c < CH; ++c) rank[c] = 0;
    for (int t = 0; t < n_sym; ++t) {
        const uint32_t kt = H.key[t];
#pragma unroll
        for (int c = 0; c < CH; ++c) rank[c] += (kt < ((f[c] << 9) | uint32_t(lane + 64 * c))) ? 1 : 0;
    }
#pragma unroll
    for (int c = 0; c < CH; ++c)
        if (f[c]) H.weight[rank[c]] = f[c];
    __syncthreads();
    if (lane == 0) {
        int i = 0, j = n;
        for (int k = n; k < 2 * n - 1; ++k) {
            int a, b;
            if (i < n && (j >= k || H.weight[i] <= H.weight[j])) a = i++; else a = j++;
            if (i < n && (j >= k || H.weight[i] <= H.weight[j])) b = i++; else b = j++;
            H.weight[k] = H.weight[a] + H.weight[b];
            H.parent[a] = uint16_t(k);
            H.parent[b] = uint16_t(k);
        }
        for (int b = 0; b < 16; ++b) H.bl_count[b] = 0;
        H.depth[2 * n - 2] = 0;
        for (int t = 2 * n - 3; t >= 0; --t) {
            const int d = min(int(H.depth[H.parent[t]]) + 1, 200);
            H.depth[t] = uint8_t(d);
            if (t < n) H.bl_count[min(d, max_bits)] += 1;
        }
        uint32_t total = 0;
        for (int b = 1; b <= max_bits; ++b) total += uint32_t(H.bl_count[b]) << (max_bits - b);
        while (total > (1u << max_bits)) {
            H.bl_count[max_bits] -= 1;
            for (int b = max_bits - 1; b > 0; --b)
                if (H.bl_count[b] > 0) {
                    H.bl_count[b] -= 1;
                    H.bl_count[b + 1] += 2;
                    break;
                }
            total -= 1;
        }
    }
    __syncthreads();
    // lengths: rank 0 (the lightest) takes the longest
    int len[CH];
#pragma unroll
    for (int c = 0; c < CH; ++c) len[c] = 0;
    {
        int cum = 0;
        for (int b = max_bits; b >= 1; --b) {
            const int next = cum + H.bl_count[b];
#pragma unroll
            for (int c = 0; c < CH; ++c)
                if (f[c] && rank[c] >= cum && rank[c] < next) len[c] = b;
            cum = next;
        }
    }
    // canonical codes: within a length, in symbol order
    uint32_t code[CH];
#pragma unroll
    for (int c = 0; c < CH; ++c) code[c] = 0;
    {
        uint32_t next_code = 0;
        for (int b = 1; b <= max_bits; ++b) {
            next_code <<= 1; // (it already stands past the codes of length b - 1)
#pragma unroll
            for (int c = 0; c < CH; ++c) {
                const uint64_t m = __ballot(len[c] == b);
                if (len[c] == b) code[c] = next_code + uint32_t(__popcll(m & bd_below(lane)));
                next_code += uint32_t(__popcll(m));
            }
        }
    }
    __syncthreads();
#pragma unroll
    for (int c = 0; c < CH; ++c) {
        const int s = lane + 64 * c;
        if (s < n_sym) {
            len_out[s] = uint8_t(len[c]);
            code_out[s] = uint16_t(bd_rev(code[c], len[c]));
        }
    }
    __syncthreads();
}

// the fixed code of RFC 1951 3.2.6 into the same tables the dynamic one uses
__device__ void bd_fixed_tables(DeflateLds& L, const int lane)
{
    for (int s = lane; s < 288; s += 64) {
        const int len = bd_fixed_ll_len(s);
        const uint32_t code = s < 144 ? 0x30u + uint32_t(s) : s < 256 ? 0x190u + uint32_t(s - 144) : s < 280 ? uint32_t(s - 256) : 0xc0u + uint32_t(s - 280);
        L.ll_len[s] = uint8_t(len);
        L.ll_code[s] = uint16_t(bd_rev(code, len));
    }
    if (lane < 32) {
        L.d_len[lane] = 5;
        L.d_code[lane] = uint16_t(bd_rev(uint32_t(lane), 5));
    }
    __syncthreads();
}

template <int LEVEL> __global__ __launch_bounds__(64) void bgzf_deflate_kernel(const DeflateArgs a)
{
    __shared__ DeflateLds L;
    const int lane = threadIdx.x;
    const int blk = a.first_block + int(blockIdx.x);
    if (blk >= a.n_blocks) return;
    const int64_t in_off = int64_t(blk) * BD_IN;
    const int64_t left = a.n_bytes - in_off;
    const int n = left < int64_t(BD_IN) ? int(left) : int(BD_IN); // 1..65280
    const uint8_t* in = a.data + in_off;
    uint8_t* slot = a.slots + int64_t(blk) * BD_SLOT;
    uint32_t* slot_w = reinterpret_cast<uint32_t*>(slot);
    uint32_t* tok = a.tokens + int64_t(blockIdx.x) * BD_IN;

    for (int i = lane; i < 256; i += 64) {
        uint32_t c = uint32_t(i);
        for (int k = 0; k < 8; ++k) c = (c & 1u) ? (0xedb88320u ^ (c >> 1)) : (c >> 1);
        L.crc_table[i] = c;
    }
    for (int i = lane; i < 320; i += 64) L.ll_freq[i] = 0;
    L.d_freq[lane] = 0;
    L.cl_freq[lane] = 0;
    for (int i = lane; i < BD_STAGE; i += 64) L.stage[i] = 0;
    if (LEVEL > 0)
        for (int i = lane; i < BD_HASH / 2; i += 64) reinterpret_cast<uint32_t*>(L.u.head)[i] = 0xffffffffu;
    __syncthreads();
    const uint32_t crc = bd_crc32(L, in, n, lane);

    // gzip member header with the BGZF extra field, up to BSIZE: 1f 8b 08 04 | MTIME 0 | XFL 0, OS ff, XLEN 6 | 'B' 'C' 2 0
    if (lane < 4) slot_w[lane] = lane == 0 ? 0x04088b1fu : lane == 1 ? 0u : lane == 2 ? 0x0006ff00u : 0x00024342u;

    int mode = BD_STORED;
    int n_tok = 0;
    int deflate_bits = 0;
    if (LEVEL > 0) {
        // ---- the match finder and the greedy parse: 64 consecutive positions a turn --------------------------------------------------
        int cover = 0; // first position no token covers yet
        for (int base = 0; base < n; base += 64) {
            const int p = base + lane;
            const bool can_hash = p + 4 <= n;
            uint32_t w = 0;
            if (can_hash) w = bd_ld32(in + p);
            else if (p < n) w = in[p];
            const uint32_t h = (w * 2654435761u) >> (32 - BD_HASH_BITS);
            // the lanes of this turn with my slot
            uint64_t same = __ballot(can_hash);
#pragma unroll
            for (int b = 0; b < BD_HASH_BITS; ++b) {
                const bool bit = ((h >> b) & 1u) != 0;
                const uint64_t m = __ballot(bit);
                same &= bit ? m : ~m;
            }
            const bool probe = can_hash && p >= cover;
            int cand = -1;
            if (probe) {
                const uint64_t lower = same & bd_below(lane);
                if (lower) cand = base + 63 - __clzll((long long)lower);
                else {
                    const unsigned hv = L.u.head[h];
                    if (hv != BD_EMPTY) cand = int(hv);
                }
            }
            __syncthreads(); // (every probe of the turn reads the table as the turns before left it)
            if (can_hash && (same >> lane) == 1ull) L.u.head[h] = uint16_t(p); // the highest lane of a slot is its one writer
            int len = 0, dist = 0;
            if (cand >= 0 && p - cand <= BD_WINDOW) {
                const int maxlen = min(int(BD_MAX_MATCH), n - p);
                const uint8_t* x = in + cand;
                const uint8_t* y = in + p;
                int k = 0;
                for (;;) {
                    if (k + 8 <= maxlen) {
                        const uint64_t d = bd_ld64(x + k) ^ bd_ld64(y + k);
                        if (d) {
                            k += __builtin_ctzll(d) >> 3;
                            break;
                        }
                        k += 8;
                    } else {
                        while (k < maxlen && x[k] == y[k]) ++k;
                        break;
                    }
                }
                dist = p - cand;
                if (k >= 4 || (k == 3 && dist <= 4096)) len = k;
            }
            // greedy, left to right: from the first uncovered lane, literals up to the next lane that holds a match, then past the match
            const int lim = min(64, n - base);
            int cur = max(cover - base, 0);
            const uint64_t M = __ballot(len > 0);
            uint64_t sel = 0;
            while (cur < lim) {
                const uint64_t rest = M >> cur;
                const int m = rest ? cur + __builtin_ctzll(rest) : 64;
                const int stop = min(m, lim);
                sel |= bd_below(stop) & ~bd_below(cur);
                cur = stop;
                if (m >= lim) break;
                sel |= 1ull << m;
                cur = m + __builtin_amdgcn_readlane(len, m);
            }
            cover = max(cover, base + cur);
            if ((sel >> lane) & 1ull) {
                const int idx = n_tok + __popcll(sel & bd_below(lane));
                uint32_t t;
                if (len > 0) {
                    int xb;
                    t = 0x80000000u | (uint32_t(len - 3) << 16) | uint32_t(dist - 1);
                    atomicAdd(&L.ll_freq[257 + bd_len_code(len - 3, &xb)], 1u);
                    atomicAdd(&L.d_freq[bd_dist_code(dist - 1, &xb)], 1u);
                } else {
                    t = w & 0xffu;
                    atomicAdd(&L.ll_freq[t], 1u);
                }
                if (idx < BD_IN) tok[idx] = t;
            }
            n_tok += __popcll(sel);
        }
        if (lane == 0) L.ll_freq[256] = 1; // end of block
        __syncthreads();

        // ---- price the encodings -----------------------------------------------------------------------------------------------------
        int part = 0;
        for (int s = lane; s < BD_NLL; s += 64) part += int(L.ll_freq[s]) * (bd_fixed_ll_len(s) + bd_ll_extra(s));
        if (lane < BD_ND) part += int(L.d_freq[lane]) * (5 + bd_d_extra(lane));
        const int fixed_bits = 3 + bd_wave_sum(part);
        const int stored_bytes = n + 5;
        mode = ((fixed_bits + 7) >> 3) < stored_bytes ? BD_FIXED : BD_STORED;
        deflate_bits = fixed_bits;
        if (LEVEL >= 2) {
            HuffWork& H = L.u.hw;
            bd_build_code<5>(L, L.ll_freq, BD_NLL, 15, L.ll_len, L.ll_code, lane);
            bd_build_code<1>(L, L.d_freq, BD_ND, 15, L.d_len, L.d_code, lane);
            if (lane == 0) {
                // HLIT / HDIST and the run-length form (symbols 16, 17, 18) of the two length arrays, each on its own as zlib sends them
                int hlit = BD_NLL, hdist = BD_ND;
                while (hlit > 257 && L.ll_len[hlit - 1] == 0) --hlit;
                while (hdist > 1 && L.d_len[hdist - 1] == 0) --hdist;
                int nt = 0;
                auto put = [&](const int sym, const int extra) {
                    H.cl_tok[nt++] = uint16_t(sym | (extra << 5));
                    L.cl_freq[sym] += 1;
                };
                for (int pass = 0; pass < 2; ++pass) {
                    const uint8_t* lens = pass ? L.d_len : L.ll_len;
                    const int cnt = pass ? hdist : hlit;
                    int i = 0;
                    while (i < cnt) {
                        const int v = lens[i];
                        int r = 1;
                        while (i + r < cnt && lens[i + r] == v) ++r;
                        i += r;
                        if (v == 0) {
                            while (r >= 11) {
                                const int t = min(r, 138);
                                put(18, t - 11);
                                r -= t;
                            }
                            if (r >= 3) {
                                put(17, r - 3);
                                r = 0;
                            }
                            for (; r > 0; --r) put(0, 0);
                        } else {
                            put(v, 0);
                            --r;
                            while (r >= 3) {
                                const int t = min(r, 6);
                                put(16, t - 3);
                                r -= t;
                            }
                            for (; r > 0; --r) put(v, 0);
                        }
                    }
                }
                H.n_cl_tok = nt;
                H.hlit = hlit;
                H.hdist = hdist;
            }
            __syncthreads();
            bd_build_code<1>(L, L.cl_freq, BD_NCL, 7, L.cl_len, L.cl_code, lane);
            int hclen = BD_NCL;
            while (hclen > 4 && L.cl_len[BD_CL_ORDER[hclen - 1]] == 0) --hclen;
            int dpart = 0;
            for (int s = lane; s < BD_NLL; s += 64) dpart += int(L.ll_freq[s]) * (int(L.ll_len[s]) + bd_ll_extra(s));
            if (lane < BD_ND) dpart += int(L.d_freq[lane]) * (int(L.d_len[lane]) + bd_d_extra(lane));
            if (lane < BD_NCL) dpart += int(L.cl_freq[lane]) * (int(L.cl_len[lane]) + (lane == 16 ? 2 : lane == 17 ? 3 : lane == 18 ? 7 : 0));
            const int dyn_bits = 3 + 14 + 3 * hclen + bd_wave_sum(dpart);
            const int best = mode == BD_FIXED ? ((fixed_bits + 7) >> 3) : stored_bytes;
            if (((dyn_bits + 7) >> 3) < best) {
                mode = BD_DYNAMIC;
                deflate_bits = dyn_bits;
            }
            if (lane == 0) H.hclen = hclen;
            __syncthreads();
        }
    }

    if (mode == BD_STORED) {
        // BSIZE, then one stored block: BFINAL 1 BTYPE 00 and padding, LEN, NLEN, the bytes; CRC-32 and ISIZE
        const int member = n + 31;
        if (lane < 7) {
            const uint32_t bsize = uint32_t(member - 1), ln = uint32_t(n), nl = ~uint32_t(n);
            const uint32_t v = lane == 0 ? bsize : lane == 1 ? (bsize >> 8) : lane == 2 ? 1u : lane == 3 ? ln : lane == 4 ? (ln >> 8) : lane == 5 ? nl : (nl >> 8);
            slot[16 + lane] = uint8_t(v);
        }
        if (lane == 0) slot[23] = in[0];
        const int words = (n - 1) / 4; // slot byte 24 is word 6
        for (int w = lane; w < words; w += 64) {
            const uint8_t* s = in + 1 + 4 * w;
            slot_w[6 + w] = uint32_t(s[0]) | (uint32_t(s[1]) << 8) | (uint32_t(s[2]) << 16) | (uint32_t(s[3]) << 24);
        }
        for (int o = 1 + 4 * words + lane; o < n; o += 64) slot[23 + o] = in[o];
        if (lane < 8) slot[23 + n + lane] = uint8_t(lane < 4 ? (crc >> (8 * lane)) : (uint32_t(n) >> (8 * (lane - 4))));
        if (lane == 0) a.slot_len[blk] = member;
        return;
    }

    if (LEVEL > 0) {
        const int member = 18 + ((deflate_bits + 7) >> 3) + 8;
        if (mode == BD_FIXED) bd_fixed_tables(L, lane);
        BitWriter bw;
        bw.words = slot_w;
        bw.wpos = 4;
        bw.fill = 0;
        HuffWork& H = L.u.hw;
        // BSIZE rides in front of the bit stream, which keeps the stream's words aligned with the slot's
        {
            uint64_t v = uint64_t(member - 1);
            int nb = 19;
            if (mode == BD_FIXED) v |= uint64_t(1u | (1u << 1)) << 16;
            else {
                v |= uint64_t(1u | (2u << 1)) << 16;
                v |= uint64_t(H.hlit - 257) << 19;
                v |= uint64_t(H.hdist - 1) << 24;
                v |= uint64_t(H.hclen - 4) << 29;
                nb = 33;
            }
            bd_emit(L, bw, v, lane == 0 ? nb : 0, lane);
        }
        if (LEVEL >= 2 && mode == BD_DYNAMIC) {
            const int hclen = H.hclen;
            bd_emit(L, bw, lane < hclen ? uint64_t(L.cl_len[BD_CL_ORDER[lane < BD_NCL ? lane : 0]]) : 0ull, lane < hclen ? 3 : 0, lane);
            const int nt = H.n_cl_tok;
            for (int t0 = 0; t0 < nt; t0 += 64) {
                uint64_t v = 0;
                int nb = 0;
                if (t0 + lane < nt) {
                    const int t = H.cl_tok[t0 + lane];
                    const int sym = t & 31, ex = t >> 5;
                    const int cl = L.cl_len[sym];
                    v = uint64_t(L.cl_code[sym]) | (uint64_t(ex) << cl);
                    nb = cl + (sym == 16 ? 2 : sym == 17 ? 3 : sym == 18 ? 7 : 0);
                }
                bd_emit(L, bw, v, nb, lane);
            }
        }
        for (int t0 = 0; t0 < n_tok; t0 += 64) {
            uint64_t v = 0;
            int nb = 0;
            if (t0 + lane < n_tok) {
                const uint32_t t = tok[t0 + lane];
                if (t & 0x80000000u) {
                    int lx, dx;
                    const int l = int((t >> 16) & 0xffu), d = int(t & 0x7fffu);
                    const int lsym = 257 + bd_len_code(l, &lx), dc = bd_dist_code(d, &dx);
                    const int ll = L.ll_len[lsym], dl = L.d_len[dc];
                    v = uint64_t(L.ll_code[lsym]);
                    nb = ll;
                    v |= uint64_t(l & ((1 << lx) - 1)) << nb;
                    nb += lx;
                    v |= uint64_t(L.d_code[dc]) << nb;
                    nb += dl;
                    v |= uint64_t(d & ((1 << dx) - 1)) << nb;
                    nb += dx;
                } else {
                    v = uint64_t(L.ll_code[t]);
                    nb = L.ll_len[t];
                }
            }
            bd_emit(L, bw, v, nb, lane);
        }
        // end of block, padding to the byte, CRC-32, ISIZE
        {
            const int pad = (8 - ((deflate_bits + 16) & 7)) & 7;
            const uint64_t v = lane == 0 ? uint64_t(L.ll_code[256]) : lane == 2 ? uint64_t(crc) : lane == 3 ? uint64_t(uint32_t(n)) : 0ull;
            const int nb = lane == 0 ? int(L.ll_len[256]) : lane == 1 ? pad : (lane == 2 || lane == 3) ? 32 : 0;
            bd_emit(L, bw, v, nb, lane);
        }
        if (lane == 0) {
            if (bw.fill > 0 && bw.wpos < BD_SLOT / 4) slot_w[bw.wpos] = L.stage[0];
            const int written = bw.wpos * 4 + (bw.fill >> 3);
            a.slot_len[blk] = (written == member && (bw.fill & 7) == 0) ? member : -1;
        }
    }
}

// D2: block_end[i] = end of member i in the packed stream, block_end[n_blocks] = end of the stream (past the EOF block when there is one)
__global__ __launch_bounds__(256) void bgzf_block_scan_kernel(const int32_t* slot_len, const int32_t n_blocks, const int with_eof, int64_t* block_end)
{
    __shared__ int64_t part[256];
    const int tid = threadIdx.x;
    int64_t carry = 0;
    for (int base = 0; base < n_blocks; base += 256) {
        const int i = base + tid;
        int64_t v = i < n_blocks ? int64_t(max(slot_len[i], 0)) : 0;
        part[tid] = v;
        __syncthreads();
        for (int d = 1; d < 256; d <<= 1) {
            const int64_t t = tid >= d ? part[tid - d] : 0;
            __syncthreads();
            part[tid] += t;
            __syncthreads();
        }
        if (i < n_blocks) block_end[i] = carry + part[tid];
        carry += part[255];
        __syncthreads();
    }
    if (tid == 0) block_end[n_blocks] = carry + (with_eof ? 28 : 0);
}

// D3: slot -> its place in the stream (32-bit stores where the destination allows); workgroup n_blocks writes the EOF block
__global__ __launch_bounds__(256) void bgzf_pack_kernel(const uint8_t* slots, const int32_t* slot_len, const int32_t n_blocks, const int64_t* block_end,
                                                        uint8_t* out, const int64_t out_cap)
{
    const int b = blockIdx.x, tid = threadIdx.x;
    const int64_t start = b ? block_end[b - 1] : 0;
    if (b >= n_blocks) {
        const uint32_t eof[7] = { 0x04088b1fu, 0u, 0x0006ff00u, 0x00024342u, 0x0003001bu, 0u, 0u };
        if (tid < 28 && start + 28 <= out_cap) out[start + tid] = uint8_t(eof[tid >> 2] >> (8 * (tid & 3)));
        return;
    }
    const int len = slot_len[b];
    if (len <= 0 || len > BD_SLOT || start + len > out_cap) return;
    const uint8_t* src = slots + int64_t(b) * BD_SLOT;
    const uint32_t* src_w = reinterpret_cast<const uint32_t*>(src);
    uint8_t* dst = out + start;
    const int head = min(len, int((4u - unsigned(reinterpret_cast<uintptr_t>(dst) & 3u)) & 3u));
    if (tid < head) dst[tid] = src[tid];
    const int words = (len - head) / 4;
    for (int w = tid; w < words; w += 256) { // the source word at byte head + 4 w: two aligned words of the slot, shifted (both inside the slot)
        const int o = head + 4 * w;
        const uint32_t lo = src_w[o >> 2];
        const uint32_t hi = (o & 3) ? src_w[min((o >> 2) + 1, BD_SLOT / 4 - 1)] : 0u;
        const int sh = 8 * (o & 3);
        *reinterpret_cast<uint32_t*>(dst + o) = sh ? ((lo >> sh) | (hi << (32 - sh))) : lo;
    }
    for (int o = head + 4 * words + tid; o < len; o += 256) dst[o] = src[o];
}

// device scratch of the deflate entry points (grown on demand, never shrunk; the library's own: one deflate in flight per process)
struct DeflateBuffers
{
    SkDevBuf slots, tokens, slot_len;
};
DeflateBuffers& deflate_bufs()
{
    static DeflateBuffers b;
    return b;
}

int64_t deflate_blocks(const int64_t n_bytes) { return (n_bytes + BD_IN - 1) / BD_IN; }

} // namespace

void sk_deflate_reset()
{
    DeflateBuffers& B = deflate_bufs();
    B.slots.drop();
    B.tokens.drop();
    B.slot_len.drop();
}

extern "C" {

int64_t sk_bgzf_deflate_bound(int64_t n_bytes, int with_eof)
{
    if (n_bytes < 0) return -1;
    // a block that does not compress is stored: its bytes, 5 of stored-block header, 26 of gzip / BGZF framing
    return deflate_blocks(n_bytes) * int64_t(BD_IN + 5 + 26) + (with_eof ? 28 : 0);
}

int sk_bgzf_deflate_dev(const uint8_t* dev_data, int64_t n_bytes, int level, int with_eof, uint8_t* dev_out, int64_t out_cap, int64_t* dev_block_end,
                        void* hip_stream)
{
    if (n_bytes < 0 || out_cap < 0) return sk_fail("sk_bgzf_deflate_dev: negative size");
    if (level < 0 || level > 2) return sk_fail("sk_bgzf_deflate_dev: level must be 0 (stored), 1 (fixed codes) or 2 (dynamic codes)");
    if ((n_bytes > 0 && !dev_data) || !dev_block_end) return sk_fail("sk_bgzf_deflate_dev: null argument");
    const int64_t bound = sk_bgzf_deflate_bound(n_bytes, with_eof);
    if (out_cap < bound) return sk_fail("sk_bgzf_deflate_dev: out_cap is below sk_bgzf_deflate_bound");
    if (bound > 0 && !dev_out) return sk_fail("sk_bgzf_deflate_dev: null argument");
    const int64_t n_blocks64 = deflate_blocks(n_bytes);
    if (n_blocks64 > (int64_t(1) << 30)) return sk_fail("sk_bgzf_deflate_dev: input too large for one call");
    SK_REQUIRE_INIT();
    const int32_t n_blocks = int32_t(n_blocks64);
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    DeflateBuffers& B = deflate_bufs();
    const int32_t per_launch = n_blocks < BD_LAUNCH_BLOCKS ? n_blocks : int32_t(BD_LAUNCH_BLOCKS);
    if (B.slots.reserve(size_t(n_blocks) * BD_SLOT + 16) || B.slot_len.reserve(4 * size_t(n_blocks) + 16) ||
        (level > 0 && B.tokens.reserve(size_t(per_launch) * BD_IN * 4 + 16)))
        return 1;
    DeflateArgs a;
    a.data = dev_data;
    a.n_bytes = n_bytes;
    a.n_blocks = n_blocks;
    a.slots = B.slots.as<uint8_t>();
    a.tokens = B.tokens.as<uint32_t>();
    a.slot_len = B.slot_len.as<int32_t>();
    for (int32_t first = 0; first < n_blocks; first += per_launch) {
        a.first_block = first;
        const int32_t count = n_blocks - first < per_launch ? n_blocks - first : per_launch;
        if (level == 0) SK_LAUNCH(bgzf_deflate_kernel<0>, dim3(count), dim3(64), 0, st, a);
        else if (level == 1) SK_LAUNCH(bgzf_deflate_kernel<1>, dim3(count), dim3(64), 0, st, a);
        else SK_LAUNCH(bgzf_deflate_kernel<2>, dim3(count), dim3(64), 0, st, a);
    }
    SK_LAUNCH(bgzf_block_scan_kernel, dim3(1), dim3(256), 0, st, a.slot_len, n_blocks, with_eof ? 1 : 0, dev_block_end);
    if (n_blocks + (with_eof ? 1 : 0) > 0)
        SK_LAUNCH(bgzf_pack_kernel, dim3(n_blocks + (with_eof ? 1 : 0)), dim3(256), 0, st, static_cast<const uint8_t*>(a.slots), static_cast<const int32_t*>(a.slot_len),
                  n_blocks, static_cast<const int64_t*>(dev_block_end), dev_out, out_cap);
    SK_HIP(skrt::getLastError());
    return 0;
}

int sk_bgzf_deflate(const uint8_t* data, int64_t n_bytes, int level, int with_eof, uint8_t* out, int64_t out_cap, int64_t* out_bytes)
{
    if (n_bytes < 0 || out_cap < 0) return sk_fail("sk_bgzf_deflate: negative size");
    if (level < 0 || level > 2) return sk_fail("sk_bgzf_deflate: level must be 0 (stored), 1 (fixed codes) or 2 (dynamic codes)");
    if ((n_bytes > 0 && !data) || !out_bytes) return sk_fail("sk_bgzf_deflate: null argument");
    const int64_t bound = sk_bgzf_deflate_bound(n_bytes, with_eof);
    if (out_cap < bound) return sk_fail("sk_bgzf_deflate: out_cap is below sk_bgzf_deflate_bound");
    if (bound > 0 && !out) return sk_fail("sk_bgzf_deflate: null argument");
    SK_REQUIRE_INIT();
    skrt::wakeHint();
    *out_bytes = 0;
    SkContext& ctx = sk_ctx();
    SK_HIP(skrt::setDevice(ctx.device));
    hipStream_t st = ctx.stream;
    const int64_t n_blocks = deflate_blocks(n_bytes);
    // (the arena is this call's until it returns: sk_bgzf_deflate_dev works in the module's own slots, tokens and slot lengths)
    struct { uint8_t* in; uint8_t* out; int64_t* block_end; } d;
    int rc = 0;
    if (sk_carve(d, [&](SkArena& ar) {
            return decltype(d){ ar.up(data, size_t(n_bytes), 16, st, rc), ar.take<uint8_t>(size_t(bound) + 16), ar.take<int64_t>(size_t(n_blocks + 1)) };
        }) || rc)
        return 1;
    if (sk_bgzf_deflate_dev(d.in, n_bytes, level, with_eof, d.out, bound, d.block_end, st)) return 1;
    std::vector<int32_t> slot_len(static_cast<size_t>(n_blocks));
    int64_t total = 0;
    SK_HIP(skrt::memcpyAsync(&total, d.block_end + n_blocks, 8, hipMemcpyDeviceToHost, st));
    if (n_blocks > 0) SK_HIP(skrt::memcpyAsync(slot_len.data(), deflate_bufs().slot_len.p, 4 * size_t(n_blocks), hipMemcpyDeviceToHost, st));
    SK_HIP(skrt::streamSynchronize(st));
    for (int64_t i = 0; i < n_blocks; ++i)
        if (slot_len[size_t(i)] <= 0 || slot_len[size_t(i)] > BD_SLOT)
            return sk_fail("sk_bgzf_deflate: block " + std::to_string(i) + ": the emitted size differs from the priced one");
    if (total < 0 || total > bound) return sk_fail("sk_bgzf_deflate: stream size out of range");
    if (total > 0) {
        SK_HIP(skrt::memcpyAsync(out, d.out, size_t(total), hipMemcpyDeviceToHost, st));
        SK_HIP(skrt::streamSynchronize(st));
    }
    *out_bytes = total;
    return 0;
}

} // extern "C"
