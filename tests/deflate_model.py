"""Two references for csrc/bgzf_deflate.hip, independent of each other (a helper module like tests/e2e_util.py; pytest collects nothing here).

  a. inflate_tokens(raw): a DEFLATE reader written from RFC 1951 alone that records what it reads -- per block the BTYPE, the tokens
     (a literal is an int, a match a (length, distance) pair) and, for a dynamic block, HLIT / HDIST / HCLEN, the three code-length
     arrays and the run-length symbols as sent.  It refuses what the RFC does not allow.  It is the judge of the device's streams and
     shares no function with the model below; the two read the same constants of RFC 1951 (the base / extra-bit tables of 3.2.5, the
     fixed code's lengths of 3.2.6, the order of 3.2.7), which zlib checks for both in tests/test_bgzf_deflate_model.py.

  b. model_member / model_stream: kernel D1 restated rule by rule from DESIGN's D1-D3 paragraph and the kernel's source, so that the
     device's bytes can be compared with it one for one.  The rules that decide a byte:
       hash       (le32(p) * 2654435761 mod 2^32) >> 19; only positions with p + 4 <= n hash, probe or insert
       turn       64 consecutive positions; a lane probes if no token covers it at the START of the turn
       candidate  the nearest lower lane of the turn with the lane's slot (covered or not), else the head the earlier turns left
       insert     after the turn's probes, the highest lane of a slot
       match      dist <= 32768, extended to min(258, n - p); kept if length >= 4, or length 3 and dist <= 4096
       parse      greedy, left to right, carried across turns
       counts     end of block 1
       mode       fixed if ceil(fixed_bits / 8) < n + 5, else stored; dynamic (level 2) only if strictly smaller than that winner
       code       used symbols ranked by (weight, symbol); two-queue merge, the leaf first on a tie; depths past max_bits folded into
                  max_bits; the Kraft sum repaired one unit at a time; lengths longest first in rank order; canonical codes;
                  fewer than two used symbols: padded with symbol 0 / 1 at weight 1 (which costs nothing: the count stays 0)
       run form   each length array on its own; zeros: 18 (up to 138) while 11 or more are left, 17 for 3..10, single zeros;
                  non-zero: the length, then 16 (up to 6) while 3 or more are left, singles
       trimming   HLIT down to 257, HDIST down to 1, HCLEN down to 4, while the last length is zero
       framing    16 header bytes, BSIZE, the deflate bytes padded to a byte, CRC-32, ISIZE
       level 0    the stored member

Speed, one core of a build machine: the model 0.2 s for a 65 280-byte block of text at level 2 and 0.9 s for the 5 blocks of the text
fixture; the inflater 0.25 s for such a block.
"""
import struct
import zlib

import numpy as np

CUT = 65280
HEADER = bytes.fromhex("1f8b08040000000000ff060042430200")
EOF_BLOCK = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
STORED, FIXED, DYNAMIC = 0, 1, 2


# ---- a. the token-recording inflater (RFC 1951) -------------------------------------------------------------------------------------------


class InflateError(ValueError):
    pass


_LEN_BASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
_LEN_EXTRA = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0)
_DIST_BASE = (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289,
              16385, 24577)
_DIST_EXTRA = (0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13)


class _Reader:
    def __init__(self, raw):
        self.raw, self.at, self.acc, self.have = raw, 0, 0, 0

    def need(self, n):
        while self.have < n:
            if self.at >= len(self.raw):
                raise InflateError("the stream ends inside a block")
            self.acc |= self.raw[self.at] << self.have
            self.at += 1
            self.have += 8

    def bits(self, n):
        self.need(n)
        v = self.acc & ((1 << n) - 1)
        self.acc >>= n
        self.have -= n
        return v

    def to_byte(self):
        drop = self.have & 7
        self.acc >>= drop
        self.have -= drop

    def symbol(self, table):
        """one Huffman symbol: codes are packed from their most significant bit, so the bits are taken one at a time"""
        code, n = 0, 0
        while True:
            code = (code << 1) | self.bits(1)
            n += 1
            s = table.get((n, code))
            if s is not None:
                return s
            if n >= 15:
                raise InflateError("a code that no symbol has")


def _decoder(lengths, what, may_be_short):
    """(length, code) -> symbol for the canonical code of `lengths` (3.2.2).  A code has to be complete; `may_be_short` admits what
    3.2.7 admits for the distance code: no code at all (a block of literals) or a single code of one bit."""
    count = [0] * 16
    for n in lengths:
        count[n] += 1
    count[0] = 0
    kraft = sum(c << (15 - n) for n, c in enumerate(count) if n)
    if kraft > 1 << 15:
        raise InflateError("%s: the code lengths are over-subscribed" % what)
    if kraft < 1 << 15:
        used = sum(count)
        if not (may_be_short and (used == 0 or (used == 1 and count[1] == 1))):
            raise InflateError("%s: the code lengths leave the code incomplete" % what)
    nxt, code = [0] * 16, 0
    for n in range(1, 16):
        code = (code + count[n - 1]) << 1
        nxt[n] = code
    table = {}
    for s, n in enumerate(lengths):
        if n:
            table[(n, nxt[n])] = s
            nxt[n] += 1
    return table


_FIXED_LL = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
_FIXED_D = [5] * 32


def inflate_tokens(raw):
    """raw DEFLATE -> (bytes, blocks); a block is a dict: 'btype', 'start' (its first output byte), 'tokens', 'bits' (its size in the
    stream, padding excluded) and for BTYPE 2 'hlit', 'hdist', 'hclen', 'cl_lens' (19, by symbol), 'll_lens', 'd_lens', 'cl_syms'
    [(symbol, extra value)].  Raises InflateError on anything RFC 1951 does not allow.  Bytes after the final block are left alone."""
    r = _Reader(bytes(raw))
    out = bytearray()
    blocks = []
    final = 0
    while not final:
        bit0 = r.at * 8 - r.have
        final = r.bits(1)
        btype = r.bits(2)
        blk = {"btype": btype, "start": len(out), "tokens": []}
        if btype == 0:
            r.to_byte()
            ln, nl = r.bits(16), r.bits(16)
            if ln != (~nl & 0xffff):
                raise InflateError("stored block: LEN is not the complement of NLEN")
            for _ in range(ln):
                b = r.bits(8)
                out.append(b)
                blk["tokens"].append(b)
        elif btype == 3:
            raise InflateError("BTYPE 3")
        else:
            if btype == 1:
                ll_lens, d_lens = _FIXED_LL, _FIXED_D
            else:
                hlit, hdist, hclen = r.bits(5) + 257, r.bits(5) + 1, r.bits(4) + 4
                if hlit > 286 or hdist > 30:
                    raise InflateError("HLIT / HDIST out of range")
                cl_lens = [0] * 19
                for i in range(hclen):
                    cl_lens[CL_ORDER[i]] = r.bits(3)
                cl = _decoder(cl_lens, "code-length code", False)
                lens, syms = [], []
                while len(lens) < hlit + hdist:
                    s = r.symbol(cl)
                    if s < 16:
                        syms.append((s, 0))
                        lens.append(s)
                    elif s == 16:
                        if not lens:
                            raise InflateError("a repeat with nothing before it")
                        e = r.bits(2)
                        syms.append((16, e))
                        lens += [lens[-1]] * (3 + e)
                    elif s == 17:
                        e = r.bits(3)
                        syms.append((17, e))
                        lens += [0] * (3 + e)
                    else:
                        e = r.bits(7)
                        syms.append((18, e))
                        lens += [0] * (11 + e)
                if len(lens) != hlit + hdist:
                    raise InflateError("a run of code lengths passes HLIT + HDIST")
                ll_lens, d_lens = lens[:hlit], lens[hlit:]
                if ll_lens[256] == 0:
                    raise InflateError("no code for the end of the block")
                blk.update(hlit=hlit, hdist=hdist, hclen=hclen, cl_lens=cl_lens, ll_lens=ll_lens, d_lens=d_lens, cl_syms=syms)
            ll = _decoder(ll_lens, "literal/length code", False)
            dd = _decoder(d_lens, "distance code", btype == 2)
            while True:
                s = r.symbol(ll)
                if s < 256:
                    out.append(s)
                    blk["tokens"].append(s)
                elif s == 256:
                    break
                else:
                    if s > 285:
                        raise InflateError("length symbol %d" % s)
                    length = _LEN_BASE[s - 257] + r.bits(_LEN_EXTRA[s - 257])
                    if not dd:
                        raise InflateError("a match in a block without a distance code")
                    c = r.symbol(dd)
                    if c > 29:
                        raise InflateError("distance symbol %d" % c)
                    dist = _DIST_BASE[c] + r.bits(_DIST_EXTRA[c])
                    if dist > len(out):
                        raise InflateError("a distance of %d with %d bytes of output" % (dist, len(out)))
                    for _ in range(length):
                        out.append(out[-dist])
                    blk["tokens"].append((length, dist))
        blk["bits"] = r.at * 8 - r.have - bit0
        blocks.append(blk)
    return bytes(out), blocks


# ---- b. the model of D1 -------------------------------------------------------------------------------------------------------------------


def hash4(w):
    """the slot of a 4-byte prefix read as a little-endian word"""
    return ((w * 2654435761) & 0xffffffff) >> 19


def _hashes(block):
    n = len(block)
    if n < 4:
        return []
    d = np.frombuffer(block, np.uint8).astype(np.uint64)
    w = d[:n - 3] | (d[1:n - 2] << 8) | (d[2:n - 1] << 16) | (d[3:] << 24)
    return (((w * 2654435761) & 0xffffffff) >> 19).tolist()


def _common(block, a, b, limit):
    x, y = block[a:a + limit], block[b:b + limit]
    if x == y:
        return limit
    diff = int.from_bytes(x, "little") ^ int.from_bytes(y, "little")
    return ((diff & -diff).bit_length() - 1) >> 3


def model_parse(block):
    """the token list of one block at levels 1 and 2"""
    n = len(block)
    slot = _hashes(block)
    head = {}
    cover = 0
    tokens = []
    for base in range(0, n, 64):
        found = {}  # position -> (length, distance), for the lanes that probe and hold a match
        turn = {}   # slot -> the highest lane of the turn seen so far
        for p in range(base, min(base + 64, n - 3)):
            s = slot[p]
            if p >= cover:
                cand = turn[s] if s in turn else head.get(s)
                if cand is not None and p - cand <= 32768:
                    k = _common(block, cand, p, min(258, n - p))
                    if k >= 4 or (k == 3 and p - cand <= 4096):
                        found[p] = (k, p - cand)
            turn[s] = p
        head.update(turn)
        cur, end = max(cover, base), min(base + 64, n)
        while cur < end:
            if cur in found:
                tokens.append(found[cur])
                cur += found[cur][0]
            else:
                tokens.append(block[cur])
                cur += 1
        cover = max(cover, cur)
    return tokens


def len_symbol(length):
    """length 3..258 -> (symbol, extra bits, extra value)"""
    for i in range(28, -1, -1):
        if length >= _LEN_BASE[i]:
            return 257 + i, _LEN_EXTRA[i], length - _LEN_BASE[i]


def dist_symbol(dist):
    for i in range(29, -1, -1):
        if dist >= _DIST_BASE[i]:
            return i, _DIST_EXTRA[i], dist - _DIST_BASE[i]


def histograms(tokens):
    ll, dd = [0] * 286, [0] * 30
    for t in tokens:
        if isinstance(t, tuple):
            ll[len_symbol(t[0])[0]] += 1
            dd[dist_symbol(t[1])[0]] += 1
        else:
            ll[t] += 1
    ll[256] = 1
    return ll, dd


def _padded(freq):
    f = list(freq)
    used = [s for s, w in enumerate(f) if w]
    if len(used) < 2:
        if not used:
            f[0] = f[1] = 1
        elif used == [0]:
            f[1] = 1
        else:
            f[0] = 1
    return f


def huffman_depths(freq):
    """the leaves' depths in the kernel's merge before any limit, in rank order: [(symbol, depth)], the lightest first"""
    f = _padded(freq)
    leaves = sorted((w, s) for s, w in enumerate(f) if w)
    n = len(leaves)
    weight = [w for w, _ in leaves] + [0] * (n - 1)
    parent = [0] * (2 * n - 1)
    i, j = 0, n
    for k in range(n, 2 * n - 1):
        pick = []
        for _ in range(2):
            if i < n and (j >= k or weight[i] <= weight[j]):  # on a tie the leaf goes first
                pick.append(i)
                i += 1
            else:
                pick.append(j)
                j += 1
        weight[k] = weight[pick[0]] + weight[pick[1]]
        parent[pick[0]] = parent[pick[1]] = k
    depth = [0] * (2 * n - 1)
    for t in range(2 * n - 3, -1, -1):
        depth[t] = depth[parent[t]] + 1
    return [(leaves[t][1], depth[t]) for t in range(n)]


def limited_lengths(freq, max_bits):
    """code lengths per symbol, at most max_bits"""
    ranked = huffman_depths(freq)
    count = [0] * (max_bits + 1)
    for _, d in ranked:
        count[min(d, max_bits)] += 1
    total = sum(count[b] << (max_bits - b) for b in range(1, max_bits + 1))
    while total > 1 << max_bits:
        count[max_bits] -= 1
        for b in range(max_bits - 1, 0, -1):
            if count[b] > 0:
                count[b] -= 1
                count[b + 1] += 2
                break
        total -= 1
    lens = [0] * len(freq)
    r = 0
    for b in range(max_bits, 0, -1):
        for _ in range(count[b]):
            lens[ranked[r][0]] = b
            r += 1
    return lens


def canonical(lens):
    """symbol -> code, bit-reversed for the stream (which takes Huffman codes from their most significant bit)"""
    codes, code = [0] * len(lens), 0
    for b in range(1, max(lens) + 1):
        code <<= 1
        for s, n in enumerate(lens):
            if n == b:
                codes[s] = int(format(code, "0%db" % b)[::-1], 2)
                code += 1
    return codes


def run_form(lens):
    """[(symbol, extra value)] for one length array"""
    out, i = [], 0
    while i < len(lens):
        v, r = lens[i], 1
        while i + r < len(lens) and lens[i + r] == v:
            r += 1
        i += r
        if v == 0:
            while r >= 11:
                t = min(r, 138)
                out.append((18, t - 11))
                r -= t
            if r >= 3:
                out.append((17, r - 3))
                r = 0
            out += [(0, 0)] * r
        else:
            out.append((v, 0))
            r -= 1
            while r >= 3:
                t = min(r, 6)
                out.append((16, t - 3))
                r -= t
            out += [(v, 0)] * r
    return out


_CL_EXTRA = {16: 2, 17: 3, 18: 7}


def _ll_extra(s):
    return _LEN_EXTRA[s - 257] if s > 256 else 0


def dynamic_plan(ll, dd):
    """everything the dynamic header holds, and the block's size in bits"""
    ll_lens, d_lens = limited_lengths(ll, 15), limited_lengths(dd, 15)
    hlit, hdist = 286, 30
    while hlit > 257 and ll_lens[hlit - 1] == 0:
        hlit -= 1
    while hdist > 1 and d_lens[hdist - 1] == 0:
        hdist -= 1
    syms = run_form(ll_lens[:hlit]) + run_form(d_lens[:hdist])
    cl = [0] * 19
    for s, _ in syms:
        cl[s] += 1
    cl_lens = limited_lengths(cl, 7)
    hclen = 19
    while hclen > 4 and cl_lens[CL_ORDER[hclen - 1]] == 0:
        hclen -= 1
    bits = 3 + 14 + 3 * hclen
    bits += sum(ll[s] * (ll_lens[s] + _ll_extra(s)) for s in range(286))
    bits += sum(dd[c] * (d_lens[c] + _DIST_EXTRA[c]) for c in range(30))
    bits += sum(cl[s] * (cl_lens[s] + _CL_EXTRA.get(s, 0)) for s in range(19))
    return dict(ll_lens=ll_lens, d_lens=d_lens, hlit=hlit, hdist=hdist, cl_syms=syms, cl_freq=cl, cl_lens=cl_lens, hclen=hclen, bits=bits)


def fixed_bits(ll, dd):
    return 3 + sum(ll[s] * (_FIXED_LL[s] + _ll_extra(s)) for s in range(286)) + sum(dd[c] * (5 + _DIST_EXTRA[c]) for c in range(30))


def model_price(block, level):
    """(mode, deflate bytes of the mode, tokens, plan of the dynamic code or None, {mode: bytes} of the forms the level allows)"""
    n = len(block)
    if level == 0:
        return STORED, n + 5, [], None, {STORED: n + 5}
    tokens = model_parse(block)
    ll, dd = histograms(tokens)
    sizes = {STORED: n + 5, FIXED: (fixed_bits(ll, dd) + 7) >> 3}
    mode = FIXED if sizes[FIXED] < sizes[STORED] else STORED
    plan = None
    if level >= 2:
        plan = dynamic_plan(ll, dd)
        sizes[DYNAMIC] = (plan["bits"] + 7) >> 3
        if sizes[DYNAMIC] < sizes[mode]:
            mode = DYNAMIC
    return mode, sizes[mode], tokens, plan, sizes


class _Bits:
    def __init__(self):
        self.out, self.acc, self.have = bytearray(), 0, 0

    def put(self, v, n):
        self.acc |= v << self.have
        self.have += n
        while self.have >= 64:
            self.out += (self.acc & 0xffffffffffffffff).to_bytes(8, "little")
            self.acc >>= 64
            self.have -= 64

    def done(self):
        self.out += self.acc.to_bytes((self.have + 7) >> 3, "little")
        self.acc = self.have = 0
        return bytes(self.out)


def model_member(block, level):
    """one input block (1..65 280 bytes) -> (the BGZF member, the mode, the tokens)"""
    block = bytes(block)
    n = len(block)
    assert 1 <= n <= CUT
    mode, size, tokens, plan, _ = model_price(block, level)
    if mode == STORED:
        deflate = b"\x01" + struct.pack("<HH", n, n ^ 0xffff) + block
    else:
        w = _Bits()
        if mode == FIXED:
            w.put(1 | (1 << 1), 3)
            ll_lens, d_lens = _FIXED_LL, [5] * 30
        else:
            w.put(1 | (2 << 1), 3)
            w.put(plan["hlit"] - 257, 5)
            w.put(plan["hdist"] - 1, 5)
            w.put(plan["hclen"] - 4, 4)
            for i in range(plan["hclen"]):
                w.put(plan["cl_lens"][CL_ORDER[i]], 3)
            cl_codes = canonical(plan["cl_lens"])
            for s, e in plan["cl_syms"]:
                w.put(cl_codes[s], plan["cl_lens"][s])
                w.put(e, _CL_EXTRA.get(s, 0))
            ll_lens, d_lens = plan["ll_lens"], plan["d_lens"]
        ll_codes, d_codes = canonical(ll_lens), canonical(d_lens)
        for t in tokens:
            if isinstance(t, tuple):
                s, xb, xv = len_symbol(t[0])
                w.put(ll_codes[s], ll_lens[s])
                w.put(xv, xb)
                c, xb, xv = dist_symbol(t[1])
                w.put(d_codes[c], d_lens[c])
                w.put(xv, xb)
            else:
                w.put(ll_codes[t], ll_lens[t])
        w.put(ll_codes[256], ll_lens[256])
        deflate = w.done()
    assert len(deflate) == size
    member = HEADER + struct.pack("<H", 18 + len(deflate) + 8 - 1) + deflate + struct.pack("<II", zlib.crc32(block), n)
    return member, mode, tokens


def model_stream(data, level, with_eof):
    data = bytes(data)
    parts = [model_member(data[i:i + CUT], level)[0] for i in range(0, len(data), CUT)]
    return b"".join(parts) + (EOF_BLOCK if with_eof else b"")
