"""BGZF compression on the device against two references of tests/deflate_model.py: a model of kernel D1 that the device has to match
byte for byte, and a token-recording inflater (RFC 1951) that judges the device's streams without the model.

  * -m "not gpu": the references hold without a device -- the inflater against zlib (and refusing what zlib refuses), the model's
    streams read by zlib, the level-2 size of the text fixture (the figure quoted in tests/test_bgzf_deflate.py and DESIGN section 6),
    and, on the model's tokens, the property every new input was built for (short blocks, turn edges, match geometry, an in-turn hash
    collision, the lengths 4 to 258 (3 cannot arise, which is proved here) and all 30 distance codes at both ends, the three length
    limits (15 bits for the literal/length and the distance code, 7 for the code-length code), the stored / fixed and the fixed /
    dynamic tie of the mode choice);
  * -m gpu: device bytes == model bytes for every small input at levels 0, 1, 2 with and without the EOF block; rules checked on the
    device's own tokens (matches fully extended, the 3-byte rule, complete codes within their limits, Huffman-optimal cost, run-length
    form, trimming, the mode choice repriced); 1 025 blocks (the launch split and the scan's carry); unaligned device pointers.

Inputs whose tokens are asserted come from arithmetic or from np.random.Generator(np.random.PCG64(k)), which SK_TEST_SEED_OFFSET does
not shift: a shifted seed could evict a hash head through a collision and fail a coverage assertion for a reason that is no bug.

The model's and the inflater's speed is in the docstring of tests/deflate_model.py; every model-checked input but text_300k (5
blocks) is 2 blocks or fewer."""
import ctypes as C
import functools
import heapq
import zlib

import numpy as np
import pytest

from strelka_amd import capi
from tests import deflate_model as M
from tests import test_bgzf_deflate as T

CUT = T.CUT
LEVELS = T.LEVELS
SHORT_N = (2, 3, 4, 5, 7, 8, 63, 64, 65, 66, 67, 127, 128, 129)
DIST_ENDS = sorted(set(list(M._DIST_BASE) + [b + (1 << e) - 1 for b, e in zip(M._DIST_BASE, M._DIST_EXTRA)]))  # 56 distances
FIB = (1, 1, 2, 3, 5, 8, 13, 21, 34, 55, 89, 144, 233, 377, 610, 987, 1597, 2584)


def _pcg(k):
    return np.random.Generator(np.random.PCG64(k))


def _rnd(k, n, lo=32, hi=127):
    return bytes(_pcg(k).integers(lo, hi, n, dtype=np.uint8))


# ---- the new inputs ---------------------------------------------------------------------------------------------------------------------


def _short(n, repeat):
    """n bytes: all different, or with a repeat in them (from 63 on: the first 20 bytes again as the last 20)"""
    if not repeat:
        return bytes(range(n))
    if n < 63:
        return (b"abcd" * 3)[:n]
    body = _rnd(100 + n, n - 20)
    return body + body[:20]


@functools.lru_cache(maxsize=None)
def _colliding_words():
    """two 4-byte prefixes with different first bytes and one slot"""
    seen = {}
    for i in range(40000):
        word = bytes([65 + i % 26, 97 + (i // 26) % 26, 48 + (i // 676) % 10, 33 + (i // 6760) % 10])
        h = M.hash4(int.from_bytes(word, "little"))
        if h in seen and seen[h][0] != word[0]:
            return seen[h], word
        seen.setdefault(h, word)
    raise AssertionError("no colliding pair")


def _len3(distance):
    """xyz twice, `distance` apart, with different bytes after it and zeros between (which touch one slot of the table)"""
    return b"\x01xyzA" + bytes(distance - 4) + b"xyzB\x02"


def _lane63():
    r, f = _rnd(202, 258), _rnd(203, 61, 1, 32)
    return r + f + r + b"\x01\x02\x03" + r[100:140] + b"\x04"


def _straddle():
    f = bytearray(_rnd(206, CUT + 300, 97, 113))
    s = _rnd(207, 100, 32, 96)
    f[CUT - 350:CUT - 250] = s
    f[CUT - 50:CUT + 50] = s
    return bytes(f)


def _collision(colliding):
    a, b = _colliding_words()
    if not colliding:
        a = b"~~~~"
    return b + _rnd(208, 66, 1, 32) + a + _rnd(209, 12, 1, 32) + b + _rnd(210, 8, 1, 32)


def _cover_len(lengths, k):
    """a source of 259 bytes below 128, then for each length (descending) a byte of its own from 128 up and the source's first
    `length` bytes: the nearest earlier copy is one byte longer, so the match is `length` exactly"""
    s = _rnd(k, 259, 32, 127)
    out = bytearray(s)
    for i, length in enumerate(lengths):
        out.append(128 + i)
        out += s[:length]
    out.append(255)
    return bytes(out)


def _cover_dist(k=1):
    """every distance code at its lowest and its highest distance: up to 64 as a run of that period, from 65 on as a 5-byte marker
    (with a byte of its own before and after each copy) twice in a field of zeros, which touch one slot of the table"""
    g = _pcg(300 + k)
    out = bytearray()
    for d in [x for x in DIST_ENDS if x <= 64]:
        period = bytes(g.permutation(np.arange(1, 128))[:d].astype(np.uint8))
        out += (period * 8)[:2 * d + 4] + b"\x00"
    size = 34400
    field = bytearray(size)
    busy = np.zeros(size, bool)
    field[:len(out)] = out
    busy[:len(out) + 1] = True
    at = len(out) + 1
    for d in [x for x in DIST_ENDS if x > 64]:
        marker = bytes(g.integers(1, 128, 5, dtype=np.uint8))
        pre = g.permutation(np.arange(1, 128))[:4].astype(np.uint8)
        first = bytes(pre[:1]) + marker + bytes(pre[2:3])
        second = bytes(pre[1:2]) + marker + bytes(pre[3:4])
        n = len(first)
        p = at
        while busy[p - 1:p + n + 1].any() or busy[p + d - 1:p + d + n + 1].any():
            p += 1
        field[p:p + n] = first
        field[p + d:p + d + n] = second
        busy[p:p + n] = True
        busy[p + d:p + d + n] = True
    return bytes(field)


def _dist_fold(k=1):
    """18 distance codes (1..18: distances 2 to 513) with the Fibonacci numbers as counts, 6 764 matches of length 4 or so: a unit is a
    period of that many bytes and its first four again; the units are shuffled.  One code more than the 17 that depth 16 needs: a
    unit or two lose their match to a collision in the table, which breaks the chain of sums at that place."""
    g = _pcg(400 + k)
    dists = [M._DIST_BASE[c] for c in range(1, 19)]
    units = np.concatenate([np.full(c, d) for d, c in zip(dists, reversed(FIB))])
    pairs = g.permutation([(a, b) for a in range(1, 128) for b in range(a + 1, 128)])
    out = bytearray()
    for i, d in enumerate(g.permutation(units)):
        period = bytes(pairs[i].astype(np.uint8)) if d == 2 else bytes(g.integers(1, 256, int(d), dtype=np.uint8))
        out += period + (period * 4)[:4]
    return bytes(out)


def _no_repeat(pool):
    """the pool's bytes in an order in which no 4-byte prefix occurs twice, so that nothing matches: the next byte of the pool is
    placed unless it completes a prefix seen before; then it waits until it fits"""
    out, seen, later = bytearray(), set(), []

    def fits(b):
        return len(out) < 3 or bytes(out[-3:]) + bytes([b]) not in seen

    def put(b):
        out.append(b)
        if len(out) >= 4:
            seen.add(bytes(out[-4:]))

    for b in pool:
        i = next((i for i, x in enumerate(later) if fits(x)), None)
        while i is not None:
            put(later.pop(i))
            i = next((i for i, x in enumerate(later) if fits(x)), None)
        if fits(b):
            put(b)
        else:
            later.append(b)
    assert not later
    return bytes(out)


def _ll_fold(k=1):
    """literals only, and a literal/length code deeper than 15.  The end of the block is a leaf of weight 1 itself, so the rare bytes
    0..15 count 1, 2, 3, 5, ... 1 597 (one 1, not two: with two the chain of sums splits into two interleaved ones, which is why
    _skewed() stays at 14); the 23 filler bytes count 2 650 each, more than the chain's sum of 4 180, so they merge among themselves
    and leave the chain alone.  65 129 bytes."""
    counts = list(FIB[1:17]) + [2650] * 23
    pool = np.concatenate([np.full(c, s, np.uint8) for s, c in enumerate(counts)])
    return _no_repeat(_pcg(500 + k).permutation(pool).tolist())


CL_FOLD = {5: 16, 6: 21, 7: 10, 8: 6, 9: 1, 10: 1, 11: 110, 12: 34, 13: 34, 14: 16, 15: 7}  # code length -> literals with it


def _cl_fold(k=1):
    """literals only, and a code-length code deeper than 7.  Byte s occurs 2^(15 - L) times for its length L of CL_FOLD; with the
    end of the block that is 32 768, so every code length is 15 - log2(count) whatever the ties.  CL_FOLD came from a random search
    over counts per length (5 to 15, Kraft sum 1, 257 symbols) for the deepest code over those counts; the lengths are dealt to the
    bytes so that length 11 never runs (a run of four would leave as symbol 16).  32 767 bytes."""
    g = _pcg(520 + k)
    others = g.permutation(np.concatenate([np.full(c, n) for n, c in CL_FOLD.items() if n != 11])).tolist()
    lens = []
    for i, n in enumerate(others):
        lens.append(n)
        if i < CL_FOLD[11]:
            lens.append(11)
    assert len(lens) == 256
    pool = np.concatenate([np.full(1 << (15 - n), s, np.uint8) for s, n in enumerate(lens)])
    return _no_repeat(g.permutation(pool).tolist())


@functools.lru_cache(maxsize=None)
def _new_inputs():
    out = {}
    for n in SHORT_N:
        out["short_%d" % n] = _short(n, False)
        out["short_%d_rep" % n] = _short(n, True)
    out.update({
        "match_to_end": (lambda r: r + r[:30])(_rnd(201, 100)),
        "lane63_258": _lane63(),
        "dist_1": _rnd(204, 10) + b"q" * 40 + b"Z",
        "dist_2": _rnd(204, 10) + b"qr" * 20 + b"Z",
        "dist_63": _rnd(205, 63, 1, 32) * 3 + b"Z",
        "dist_64": _rnd(205, 64, 1, 32) * 3 + b"Z",
        "len3_4096": _len3(4096),
        "len3_4097": _len3(4097),
        "straddle": _straddle(),
        "collision": _collision(True),
        "collision_control": _collision(False),
        "cover_len_a": _cover_len(range(258, 130, -1), 211),
        "cover_len_b": _cover_len(range(130, 3, -1), 212),
        "cover_dist": _cover_dist(),
        "dist_fold": _dist_fold(),
        "ll_fold": _ll_fold(),
        "cl_fold": _cl_fold(),
        "tie_stored_fixed": bytes(range(144, 174)),
        "tie_fixed_dynamic": bytes(_pcg(706).integers(97, 103, 21, dtype=np.uint8)),
    })
    return out


@functools.lru_cache(maxsize=None)
def _all_inputs():
    out = dict(T._inputs())
    out.update(_new_inputs())
    return out


@functools.lru_cache(maxsize=None)
def _deflated(name, level, with_eof):
    """one compression per (input, level, eof); the inputs of tests/test_bgzf_deflate.py share that module's"""
    if name in T._inputs():
        return T._deflated(name, level, with_eof)
    capi.init(0)
    return capi.bgzf_deflate(_all_inputs()[name], level=level, with_eof=with_eof)


@functools.lru_cache(maxsize=None)
def _model(name, level, with_eof):
    return M.model_stream(_all_inputs()[name], level, with_eof)


@functools.lru_cache(maxsize=None)
def _model_blocks(name, level):
    """[(mode, tokens)] per block"""
    data = _all_inputs()[name]
    return [M.model_member(data[i:i + CUT], level)[1:] for i in range(0, len(data), CUT)]


def _tokens(name):
    return _model_blocks(name, 1)[0][1]


def _matches(tokens):
    """[(position, length, distance)]"""
    out, pos = [], 0
    for t in tokens:
        if isinstance(t, tuple):
            out.append((pos, t[0], t[1]))
            pos += t[0]
        else:
            pos += 1
    return out


# ---- without a device: the inflater ---------------------------------------------------------------------------------------------------------


def _zlib_raw(data, level, strategy=zlib.Z_DEFAULT_STRATEGY):
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 8, strategy)
    return c.compress(data) + c.flush()


def _zlib_refuses(raw):
    d = zlib.decompressobj(-15)
    try:
        d.decompress(raw)
    except zlib.error:
        return True
    return not d.eof


def _refuses(raw):
    try:
        M.inflate_tokens(raw)
    except M.InflateError:
        return True
    return False


def _inflater_inputs():
    return {"text": T._inputs()["cut_plus_1"][:40000], "zeros": bytes(70000), "random": T._inputs()["random_70000"][:20000], "skewed": T._skewed()}


@pytest.mark.parametrize("which", ["text", "zeros", "random", "skewed"])
def test_inflater_reads_what_zlib_writes(which):
    data = _inflater_inputs()[which]
    for level, strategy in ((0, zlib.Z_DEFAULT_STRATEGY), (1, zlib.Z_DEFAULT_STRATEGY), (6, zlib.Z_DEFAULT_STRATEGY), (9, zlib.Z_DEFAULT_STRATEGY),
                            (6, zlib.Z_FIXED)):
        raw = _zlib_raw(data, level, strategy)
        got, blocks = M.inflate_tokens(raw)
        assert got == data, (level, strategy)
        if level == 0:
            assert {b["btype"] for b in blocks} == {0}
        if strategy == zlib.Z_FIXED:
            assert {b["btype"] for b in blocks} <= {0, 1}  # (zlib stores what the fixed code would enlarge)
        # the tokens are the bytes, and the recorded sizes add up to the stream
        pos = 0
        for b in blocks:
            assert b["start"] == pos
            for t in b["tokens"]:
                if isinstance(t, tuple):
                    assert data[pos:pos + t[0]] == bytes(data[pos - t[1] + i % t[1]] for i in range(t[0]))
                    pos += t[0]
                else:
                    assert data[pos] == t
                    pos += 1
        assert pos == len(data)


def test_inflater_refuses_where_zlib_refuses():
    data = _inflater_inputs()["text"]
    raw = _zlib_raw(data, 6)
    _, blocks = M.inflate_tokens(raw)
    assert blocks[0]["btype"] == 2
    # 1. every single flipped bit of the code-length header (3 bits for each of HCLEN lengths, from bit 17 of the block on)
    refused = 0
    for bit in range(17, 17 + 3 * blocks[0]["hclen"]):
        bad = bytearray(raw)
        bad[bit >> 3] ^= 1 << (bit & 7)
        z = _zlib_refuses(bytes(bad))
        assert _refuses(bytes(bad)) == z, bit
        refused += z
    assert refused >= blocks[0]["hclen"]  # (a flipped length nearly always breaks the Kraft sum)
    # 2. a distance past the start: fixed block, literal 'a', length 3 at distance 2, end of block
    bits = "1" + "10" + format(0x30 + 97, "08b") + format(1, "07b") + format(1, "05b") + format(0, "07b")
    bad = int(bits[::-1], 2).to_bytes((len(bits) + 7) // 8, "little")
    assert _zlib_refuses(bad) and _refuses(bad)
    good = int(("1" + "10" + format(0x30 + 97, "08b") + format(1, "07b") + format(0, "05b") + format(0, "07b"))[::-1], 2).to_bytes(4, "little")
    assert not _zlib_refuses(good) and M.inflate_tokens(good)[0] == b"aaaa"
    # 3. a bad NLEN
    stored = bytearray(_zlib_raw(b"hello", 0))
    assert not _refuses(bytes(stored))
    stored[3] ^= 0x10
    assert _zlib_refuses(bytes(stored)) and _refuses(bytes(stored))
    # 4. cut short
    assert _zlib_refuses(raw[:len(raw) // 2]) and _refuses(raw[:len(raw) // 2])


# ---- without a device: the model ----------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("name", list(_all_inputs()))
def test_model_stream_is_valid(name):
    data = _all_inputs()[name]
    sizes = {}
    for level in LEVELS:
        for with_eof in (True, False):
            stream = _model(name, level, with_eof)
            assert b"".join(T._zlib_walk(stream)) == data
            members = T._members(stream)
            assert stream[members[-1][0]:] == T.EOF_BLOCK if with_eof else True
        sizes[level] = [length for _, length in T._members(_model(name, level, False))]
    for b in range(-(-len(data) // CUT)):
        assert sizes[0][b] == min(CUT, len(data) - b * CUT) + 31
        assert sizes[2][b] <= sizes[1][b] <= sizes[0][b]


def test_text_fixture_size_at_level_2():
    """the figure the docstring of tests/test_bgzf_deflate.py and DESIGN section 6 quote is this model's, for the unshifted seeds"""
    import os
    size = len(_model("text_300k", 2, False))
    print("model, text_300k at level 2: %d bytes" % size)
    if int(os.environ.get("SK_TEST_SEED_OFFSET", "0")) == 0:
        assert size == 52201


def test_code_builder_follows_its_rules():
    # a tie between a leaf and an internal node of weight 2: the leaf goes first, so the tree is flat
    assert M.limited_lengths([1, 1, 2, 2], 15) == [2, 2, 2, 2]
    # fewer than two used symbols: padded with symbol 0 / 1
    assert M.limited_lengths([0, 0, 0, 0], 15) == [1, 1, 0, 0]
    assert M.limited_lengths([5, 0, 0, 0], 15) == [1, 1, 0, 0]
    assert M.limited_lengths([0, 0, 0, 7], 15) == [1, 0, 0, 1]
    # the fold: Fibonacci weights are as deep as a code gets; limited to 4 bits the Kraft sum is repaired to exactly 1
    lens = M.limited_lengths([1, 1, 2, 3, 5, 8, 13], 4)
    assert max(d for _, d in M.huffman_depths([1, 1, 2, 3, 5, 8, 13])) == 6
    assert max(lens) == 4 and sum(2.0 ** -n for n in lens) == 1.0
    assert lens == sorted(lens, reverse=True)  # the lightest take the longest
    # run-length form
    assert M.run_form([0] * 150) == [(18, 127), (18, 1)]
    assert M.run_form([0] * 148) == [(18, 127), (17, 7)]
    assert M.run_form([0] * 12 + [5] * 10 + [0, 0]) == [(18, 1), (5, 0), (16, 3), (16, 0), (0, 0), (0, 0)]
    assert M.run_form([7] * 9) == [(7, 0), (16, 3), (7, 0), (7, 0)]


@pytest.mark.parametrize("n", SHORT_N)
def test_short_blocks_on_the_model(n):
    assert _tokens("short_%d" % n) == list(range(n))
    tokens = _tokens("short_%d_rep" % n)
    data = _new_inputs()["short_%d_rep" % n]
    if n < 8:
        assert tokens == list(data)  # positions n - 3 .. n - 1 cannot hash: a repeat of fewer than 4 bytes from there on is not found
    elif n == 8:
        assert tokens == [97, 98, 99, 100, (4, 4)]
    else:
        assert tokens == list(data[:n - 20]) + [(20, n - 20)]  # ends at the block's last byte


def test_match_geometry_on_the_model():
    assert _tokens("match_to_end")[-1] == (30, 100)
    # a match of 258 from lane 63 of turn 4; the four turns it covers only insert, and what they insert is found afterwards
    m = _matches(_tokens("lane63_258"))
    assert m == [(319, 258, 319), (580, 40, 161)] and 319 % 64 == 63
    # in-turn candidates (distances 1, 2, 63) and the table's (64)
    assert _matches(_tokens("dist_1")) == [(11, 39, 1)]
    assert _matches(_tokens("dist_2")) == [(12, 38, 2)]
    assert _matches(_tokens("dist_63")) == [(63, 126, 63)]
    assert _matches(_tokens("dist_64")) == [(64, 128, 64)]


def test_three_byte_matches_cannot_arise():
    """The rule `length 3 and dist <= 4096` is never the one that decides.  A candidate shares the position's slot; a match of exactly
    3 has the same first three bytes and another fourth.  The fourth byte b adds b * 2654435761 * 2^24 = (b * 0xb1 mod 256) << 24 to the
    product, and 0xb1 is odd: two different fourth bytes change the product's top 8 bits, so they never share one of the 8 192 slots
    (its top 13 bits).  And a position whose match is cut to 3 by the block's end does not hash.  So no stream holds a length of 3,
    at 4096 or anywhere; the two inputs built for the rule show literals at both distances."""
    for low in (0, 0x7a7978, 0xffffff, 0x123456):
        assert len({M.hash4(low | (b << 24)) >> 5 for b in range(256)}) == 256
    for name, d in (("len3_4096", 4096), ("len3_4097", 4097)):
        data = _new_inputs()[name]
        assert data[1:4] == data[1 + d:4 + d] and data[4] != data[4 + d]
        assert all(dist == 1 for _, _, dist in _matches(_tokens(name))) and _tokens(name)[-5:] == list(data[-5:])
    for name in _all_inputs():
        for mode, tokens in _model_blocks(name, 1):
            assert all(length >= 4 for _, length, _ in _matches(tokens)), name


def test_straddling_repeat_on_the_model():
    data = _new_inputs()["straddle"]
    for level in (1, 2):
        (mode0, tok0), (mode1, tok1) = _model_blocks("straddle", level)
        assert mode0 != M.STORED and mode1 != M.STORED  # (the tokens are in the stream)
        assert tok0[-1] == (50, 300)  # the first half, up to the cut
        assert tok1[:50] == list(data[CUT:CUT + 50])  # the second half has nothing before it in its block
        for tokens in (tok0, tok1):
            assert all(d <= p for p, _, d in _matches(tokens))


def test_in_turn_collision_on_the_model():
    a, b = _colliding_words()
    assert a != b and a[0] != b[0] and M.hash4(int.from_bytes(a, "little")) == M.hash4(int.from_bytes(b, "little"))
    assert _matches(_tokens("collision")) == []  # the in-turn candidate (the other prefix) wins over the table's true occurrence
    assert _matches(_tokens("collision_control")) == [(86, 4, 86)]


def test_coverage_on_the_model():
    lengths, dists = set(), set()
    for name in ("cover_len_a", "cover_len_b", "cover_dist"):
        assert _model_blocks(name, 1)[0][0] == M.FIXED and _model_blocks(name, 2)[0][0] == M.DYNAMIC, name
        assert len(_new_inputs()[name]) <= CUT
        for _, length, d in _matches(_tokens(name)):
            lengths.add(length)
            dists.add(d)
    assert lengths >= set(range(4, 259))  # (3 cannot arise: test_three_byte_matches_cannot_arise)
    assert dists >= set(DIST_ENDS) and len(DIST_ENDS) == 56
    assert {M.dist_symbol(d)[0] for d in DIST_ENDS} == set(range(30))


def _depth(freq):
    return max(d for _, d in M.huffman_depths(freq))


def test_length_limits_on_the_model():
    """Each of the three limits is reached by an input of its own, all of one block: ll_fold the literal/length code's 15 bits
    (unrestricted depth 20), dist_fold the distance code's 15 bits, cl_fold the code-length code's 7 bits (unrestricted depth 8).
    skewed_46k of tests/test_bgzf_deflate.py does NOT reach the first: its byte counts 1, 1, 2, 3, ... and the end of the block make
    three leaves of weight 1, the chain of sums splits in two, the matcher takes frequent letters into matches, and the depth is 14
    for the unshifted seed (printed here; it is kept as an input with a deep code that needs no fold)."""
    mode, tokens = _model_blocks("skewed_46k", 2)[0]
    print("skewed_46k: unrestricted literal/length depth %d" % _depth(M.histograms(tokens)[0]))
    assert mode == M.DYNAMIC
    for name in ("ll_fold", "dist_fold", "cl_fold"):
        assert len(_new_inputs()[name]) <= CUT
        assert _model_blocks(name, 2)[0][0] == M.DYNAMIC, name  # (the folded code is in the stream)
    ll, dd = M.histograms(_model_blocks("ll_fold", 2)[0][1])
    assert _matches(_tokens("ll_fold")) == [] and _model_blocks("ll_fold", 1)[0][0] == M.FIXED
    assert _depth(ll) > 15 and max(M.limited_lengths(ll, 15)) == 15
    ll, dd = M.histograms(_model_blocks("dist_fold", 2)[0][1])
    assert _depth(dd) > 15 and max(M.limited_lengths(dd, 15)) == 15
    assert _matches(_tokens("cl_fold")) == []
    plan = M.model_price(_new_inputs()["cl_fold"], 2)[3]
    assert _depth(plan["cl_freq"]) > 7 and max(plan["cl_lens"]) == 7


def test_mode_ties_on_the_model():
    # 30 literals of 9 bits: the fixed block is 3 + 270 + 7 bits = 35 bytes = 30 + 5: stored is kept
    mode, size, _, _, sizes = M.model_price(_new_inputs()["tie_stored_fixed"], 1)
    assert sizes[M.FIXED] == sizes[M.STORED] == 35 and mode == M.STORED
    assert M.model_price(_new_inputs()["tie_stored_fixed"], 2)[0] == M.STORED
    # 178 bits fixed, 177 bits dynamic, 23 bytes both: fixed is kept, although dynamic has the fewer bits
    mode, size, tokens, plan, sizes = M.model_price(_new_inputs()["tie_fixed_dynamic"], 2)
    assert M.fixed_bits(*M.histograms(tokens)) == 178 and plan["bits"] == 177
    assert sizes[M.DYNAMIC] == sizes[M.FIXED] == 23 < sizes[M.STORED] and mode == M.FIXED


# ---- on the device ----------------------------------------------------------------------------------------------------------------------


def _slices(data):
    return [data[i:i + CUT] for i in range(0, len(data), CUT)]


def _explain(device, model, data):
    """where two streams part: the block, then the first differing token, code length or header field"""
    dm, mm = T._members(device), T._members(model)
    if len(dm) != len(mm):
        return "%d members against the model's %d" % (len(dm), len(mm))
    for b, ((do, dl), (mo, ml)) in enumerate(zip(dm, mm)):
        d, m = device[do:do + dl], model[mo:mo + ml]
        if d == m:
            continue
        if len(d) < 28 or len(m) < 28 or b >= len(_slices(data)):
            return "block %d: the EOF block or the framing differs" % b
        try:
            (_, (db,)), (_, (mb,)) = M.inflate_tokens(d[18:-8]), M.inflate_tokens(m[18:-8])
        except (M.InflateError, ValueError) as e:
            return "block %d: the device's member does not inflate as one block: %s" % (b, e)
        if db["btype"] != mb["btype"]:
            return "block %d: BTYPE %d against the model's %d" % (b, db["btype"], mb["btype"])
        pos = 0
        for i, (x, y) in enumerate(zip(db["tokens"], mb["tokens"])):
            if x != y:
                return "block %d: token %d at byte %d is %r against the model's %r" % (b, i, pos, x, y)
            pos += x[0] if isinstance(x, tuple) else 1
        if len(db["tokens"]) != len(mb["tokens"]):
            return "block %d: %d tokens against the model's %d" % (b, len(db["tokens"]), len(mb["tokens"]))
        for key in ("hlit", "hdist", "hclen", "ll_lens", "d_lens", "cl_lens", "cl_syms"):
            if db.get(key) != mb.get(key):
                if isinstance(db.get(key), list):
                    i = next((i for i, (x, y) in enumerate(zip(db[key], mb[key])) if x != y), min(len(db[key]), len(mb[key])))
                    return "block %d: the tokens agree; %s[%d] is %r against the model's %r" % (
                        b, key, i, db[key][i:i + 1], mb[key][i:i + 1])
                return "block %d: the tokens agree; %s is %r against the model's %r" % (b, key, db.get(key), mb.get(key))
        i = next(i for i, (x, y) in enumerate(zip(d, m)) if x != y) if len(d) == len(m) else min(len(d), len(m))
        return "block %d: tokens and code lengths agree; the members differ from byte %d (lengths %d, %d)" % (b, i, len(d), len(m))
    return "the streams differ past their members"


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(_all_inputs()))
def test_device_bytes_equal_the_model(name):
    for level in LEVELS:
        for with_eof in (True, False):
            device, model = _deflated(name, level, with_eof), _model(name, level, with_eof)
            if device != model:
                pytest.fail("%s, level %d, eof %d: %s" % (name, level, with_eof, _explain(device, model, _all_inputs()[name])))


def _kraft(lens):
    return sum(1 << (15 - n) for n in lens if n)


def _huffman(freq):
    """(cost in bits, longest code) of a plain Huffman code for the non-zero counts; one symbol alone still takes a bit"""
    heap = [(w, 0) for w in freq if w]
    if len(heap) < 2:
        return sum(w for w, _ in heap), 1
    heapq.heapify(heap)
    cost = 0
    while len(heap) > 1:
        (a, x), (b, y) = heapq.heappop(heap), heapq.heappop(heap)
        cost += a + b
        heapq.heappush(heap, (a + b, max(x, y) + 1))
    return cost, heap[0][1]


def _prefix(data, a, b, limit):
    k = 0
    while k < limit and data[a + k] == data[b + k]:
        k += 1
    return k


def _expand(syms):
    out = []
    for s, e in syms:
        out += [s] if s < 16 else [out[-1]] * (3 + e) if s == 16 else [0] * (3 + e) if s == 17 else [0] * (11 + e)
    return out


def _check_member(member, want, level, where):
    """the rules, on the device's own tokens; nothing here comes from the model half of tests/deflate_model.py"""
    n = len(want)
    out, blocks = M.inflate_tokens(member[18:-8])
    assert out == want and len(blocks) == 1, where
    blk = blocks[0]
    assert len(member) == 18 + ((blk["bits"] + 7) >> 3) + 8, where
    if blk["btype"] == 0:
        assert len(member) == n + 31, where
        return 0
    ll, dd, pos = [0] * 286, [0] * 30, 0
    for t in blk["tokens"]:
        if isinstance(t, tuple):
            length, dist = t
            assert dist <= min(pos, 32768), (where, pos, t)
            assert length == _prefix(want, pos - dist, pos, min(258, n - pos)), (where, pos, t)  # fully extended
            assert not (length == 3 and dist > 4096), (where, pos, t)
            ll[257 + max(i for i in range(29) if M._LEN_BASE[i] <= length)] += 1
            dd[max(i for i in range(30) if M._DIST_BASE[i] <= dist)] += 1
            pos += length
        else:
            ll[t] += 1
            pos += 1
    assert pos == n, where
    ll[256] = 1
    extra = sum(ll[257 + i] * M._LEN_EXTRA[i] for i in range(29)) + sum(dd[i] * M._DIST_EXTRA[i] for i in range(30))
    fixed = 3 + sum(ll[s] * M._FIXED_LL[s] for s in range(286)) + 5 * sum(dd) + extra
    sizes = {0: n + 5, 1: (fixed + 7) >> 3}
    if blk["btype"] == 2:
        assert level == 2, where
        cl = [0] * 19
        for s, _ in blk["cl_syms"]:
            cl[s] += 1
        for lens, freq, limit, what in ((blk["ll_lens"], ll, 15, "literal/length"), (blk["d_lens"], dd, 15, "distance"), (blk["cl_lens"], cl, 7, "code-length")):
            assert _kraft(lens) == 1 << 15 and max(lens) <= limit, (where, what)
            lens = lens + [0] * (len(freq) - len(lens))
            assert all(lens[s] for s, w in enumerate(freq) if w), (where, what)
            cost, best = sum(w * lens[s] for s, w in enumerate(freq)), _huffman(freq)
            if best[1] <= limit:
                assert cost == best[0], (where, what, cost, best)
            else:
                assert cost >= best[0], (where, what, cost, best)
        assert _expand(blk["cl_syms"]) == blk["ll_lens"] + blk["d_lens"], where
        assert blk["hlit"] == 257 or blk["ll_lens"][-1], where
        assert blk["hdist"] == 1 or blk["d_lens"][-1], where
        assert blk["hclen"] == 4 or blk["cl_lens"][M.CL_ORDER[blk["hclen"] - 1]], where
        dyn = 3 + 14 + 3 * blk["hclen"] + sum(cl[s] * (blk["cl_lens"][s] + {16: 2, 17: 3, 18: 7}.get(s, 0)) for s in range(19)) + extra \
            + sum(w * blk["ll_lens"][s] for s, w in enumerate(ll) if w) + sum(w * blk["d_lens"][s] for s, w in enumerate(dd) if w)  # (a used symbol has a length: checked above)
        assert dyn == blk["bits"], where
        sizes[2] = (dyn + 7) >> 3
    elif level == 2:
        # the dynamic form was not sent; with Huffman's optimum for the two codes and the shortest header there is, it is no smaller
        low = 3 + 14 + 3 * 4 + _huffman(ll)[0] + _huffman(dd)[0] + extra
        if (low + 7) >> 3 < sizes[1]:
            return -1  # (not decided here: the comparison with the model decides it)
    assert len(member) - 26 == sizes[blk["btype"]] == min(sizes.values()), (where, sizes)
    assert blk["btype"] == min(m for m, s in sizes.items() if s == min(sizes.values())), (where, sizes)  # stored over fixed over dynamic
    return 0


@functools.lru_cache(maxsize=None)
def _undecided_on_the_model():
    """the inputs with a block that is fixed at level 2 while Huffman's optimum with the shortest header there is would be smaller
    in bytes: there the device's own tokens cannot show that fixed was right (the real header is longer than the shortest), and the
    comparison with the model decides; for every other input the repricing in _check_member is complete"""
    out = set()
    for name, data in _all_inputs().items():
        for block in _slices(data):
            mode, _, tokens, _, sizes = M.model_price(block, 2)
            if mode == M.FIXED:
                ll, dd = M.histograms(tokens)
                extra = sum(ll[257 + i] * M._LEN_EXTRA[i] for i in range(29)) + sum(dd[i] * M._DIST_EXTRA[i] for i in range(30))
                if (3 + 14 + 12 + _huffman(ll)[0] + _huffman(dd)[0] + extra + 7) >> 3 < sizes[M.FIXED]:
                    out.add(name)
    return frozenset(out)


def test_only_short_blocks_leave_their_mode_to_the_model():
    """a dynamic header of some 20 bytes decides only where the block is short: every input from 600 bytes on is repriced in full"""
    open_ones = _undecided_on_the_model()
    print("mode left to the model: %s" % ", ".join(sorted(open_ones)))
    assert all(len(_all_inputs()[name]) < 600 for name in open_ones)
    assert "tie_fixed_dynamic" in open_ones  # (a tie in bytes is one of them by nature)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(_all_inputs()))
def test_device_stream_obeys_the_rules(name):
    data = _all_inputs()[name]
    undecided = 0
    for level in (1, 2):
        stream = _deflated(name, level, False)
        members = T._members(stream)
        assert len(members) == len(_slices(data))
        for b, ((off, length), want) in enumerate(zip(members, _slices(data))):
            undecided += _check_member(stream[off:off + length], want, level, (name, level, b))
    print("%s: %d block(s) whose mode the lower bound of the dynamic form leaves open" % (name, -undecided))
    assert (undecided != 0) == (name in _undecided_on_the_model()), name


@functools.lru_cache(maxsize=None)
def _many_blocks():
    """1 024 x 65 280 + 1 000 bytes: block i < 512 is a 4 KB chunk of its own, tiled, its first (41 i mod 3001) bytes random; block
    512 + i equals block i; block 1 024 is the first 1 000 bytes of block 0"""
    g = _pcg(600)
    half = np.tile(g.integers(32, 127, (512, 4096), dtype=np.uint8), (1, 16))[:, :CUT].copy()
    for i in range(512):
        k = 41 * i % 3001
        half[i, :k] = g.integers(0, 256, k, dtype=np.uint8)
    return np.concatenate([half.reshape(-1), half.reshape(-1), half[0, :1000]])


@pytest.mark.gpu
def test_1025_blocks():
    """crosses BD_LAUNCH_BLOCKS (a second launch with first_block = 1 024) and carries the scan through five chunks of 256.
    Not yet timed on an MI355X; on the host side it is three zlib walks of 67 MB and four model members."""
    import torch
    capi.init(0)
    L = capi.lib()
    data = _many_blocks()
    raw = data.tobytes()
    n_blocks = 1025
    assert len(raw) == 1024 * CUT + 1000
    client = bool(L.sk_broker_client())
    for level in LEVELS:
        stream = capi.bgzf_deflate(data, level=level, with_eof=True)
        parts = T._zlib_walk(stream)
        assert len(parts) == n_blocks + 1 and b"".join(parts) == raw, level
        members = T._members(stream)
        ends = np.cumsum([length for _, length in members[:n_blocks]])
        assert stream[members[-1][0]:] == T.EOF_BLOCK
        if level:
            assert {length % 4 for _, length in members[:512]} == {0, 1, 2, 3}
        get = lambda b: stream[members[b][0]:members[b][0] + members[b][1]]
        for i in range(512):
            assert get(i) == get(512 + i), (level, i)  # equal blocks, equal members
        assert get(0) == M.model_member(raw[:CUT], level)[0], level
        assert get(1024) == M.model_member(raw[:1000], level)[0], level
        if not client:
            cap = capi.bgzf_deflate_bound(len(raw), True)
            d_in = torch.from_numpy(data).cuda()
            d_out = torch.zeros(cap, dtype=torch.uint8, device="cuda")
            d_end = torch.full((n_blocks + 1,), -1, dtype=torch.int64, device="cuda")
            torch.cuda.synchronize()
            capi._check(L.sk_bgzf_deflate_dev(C.c_void_p(d_in.data_ptr()), len(raw), level, 1, C.c_void_p(d_out.data_ptr()), cap,
                                              C.c_void_p(d_end.data_ptr()), C.c_void_p(torch.cuda.current_stream().cuda_stream)))
            torch.cuda.synchronize()
            end = d_end.cpu().numpy()
            assert np.array_equal(end[:n_blocks], ends) and int(end[n_blocks]) == int(ends[-1]) + 28 == len(stream)
            assert d_out[:len(stream)].cpu().numpy().tobytes() == stream
            del d_in, d_out, d_end
        # small inputs again, the scratch buffers now large and stale
        for name in ("one_byte", "cut_plus_1"):
            assert capi.bgzf_deflate(_all_inputs()[name], level=level, with_eof=True) == _model(name, level, True), (level, name)


@pytest.mark.gpu
def test_unaligned_device_pointers():
    """dev_out and dev_data at byte offsets 1, 2, 3 (D3 takes its head and tail from the address), out_cap exactly the bound, and
    nothing written outside the stream"""
    import torch
    if capi.lib().sk_broker_client():
        pytest.skip("not available to a broker client: the *_dev entry points need a GPU context of the caller's")
    capi.init(0)
    L = capi.lib()
    guard = 64
    for name in ("cut_plus_1", "cover_len_a", "cover_len_b", "cover_dist"):
        data = _all_inputs()[name]
        n_blocks = len(_slices(data))
        cap = capi.bgzf_deflate_bound(len(data), True)
        for level in (0, 2):
            want = None
            for in_off, out_off in ((0, 0), (0, 1), (0, 2), (0, 3), (1, 0), (2, 0), (3, 0)):
                whole_in = torch.zeros(len(data) + 8, dtype=torch.uint8, device="cuda")
                whole_in[in_off:in_off + len(data)] = torch.from_numpy(np.frombuffer(data, np.uint8).copy()).cuda()
                whole_out = torch.full((guard + 4 + cap + guard,), 0xA5, dtype=torch.uint8, device="cuda")
                d_in, d_out = whole_in[in_off:], whole_out[guard + out_off:]
                assert d_in.data_ptr() % 4 == in_off and d_out.data_ptr() % 4 == out_off
                d_end = torch.full((n_blocks + 1,), -1, dtype=torch.int64, device="cuda")
                torch.cuda.synchronize()
                capi._check(L.sk_bgzf_deflate_dev(C.c_void_p(d_in.data_ptr()), len(data), level, 1, C.c_void_p(d_out.data_ptr()), cap,
                                                  C.c_void_p(d_end.data_ptr()), C.c_void_p(torch.cuda.current_stream().cuda_stream)))
                torch.cuda.synchronize()
                total = int(d_end.cpu().numpy()[n_blocks])
                got = whole_out.cpu().numpy()
                stream = got[guard + out_off:guard + out_off + total].tobytes()
                if want is None:
                    want = stream
                    assert want == _model(name, level, True), (name, level)
                assert stream == want, (name, level, in_off, out_off)
                assert (got[:guard + out_off] == 0xA5).all() and (got[guard + out_off + total:] == 0xA5).all(), (name, level, in_off, out_off)
