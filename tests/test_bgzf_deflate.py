"""The feed's way out: BGZF compression on the device (sk_bgzf_deflate, csrc/bgzf_deflate.hip).

  * -m "not gpu": the bound (host arithmetic), and the refusal to compute without a device;
  * -m gpu: every stream is read back by zlib, by the project's own inflate kernels and, where oracle/_ref holds them, by bgzip and
    samtools; the framing of every block is checked byte by byte; the output is deterministic, the device entry point agrees with
    the host one, and per block level 2 <= level 1 <= level 0.

Compressed size of the text fixture (about 300 KB of gVCF-like lines) against zlib level 1 over the same 65 280-byte slices plus 26
bytes of framing each (56 197 bytes): the model of the kernel in tests/deflate_model.py (same hash, same turns of 64 positions, same
parse, same code construction; tests/test_bgzf_deflate_model.py::test_text_fixture_size_at_level_2 reruns it) gives 52 201 bytes at
level 2, an excess of -0.071.  NOT yet measured on an MI355X: until it is, the
margin asserted below is TEXT_MARGIN = 0.00 over zlib's figure (the restatement's excess rounded up to the next 0.05 is -0.05; zero is
kept until a device run confirms the figure), and test_text_fixture_is_near_zlib_level_1 prints the measured sizes."""
import functools
import gzip
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

from strelka_amd import capi
from tests import e2e_util as E

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TINY = os.path.join(GOLD, "feed_tiny.bam")
BGZIP = os.path.join(E.REF_DIR, "bin", "bgzip")
SAMTOOLS = os.path.join(E.REF_DIR, "bin", "samtools")
CUT = 65280
EOF_BLOCK = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
HEADER = bytes.fromhex("1f8b08040000000000ff060042430200")
LEVELS = (0, 1, 2)
TEXT_MARGIN = 0.00  # over zlib level 1's figure; see the module docstring


def _text(n_bytes, seed):
    """seeded gVCF-like lines: non-variant blocks with the odd variant record between them"""
    rng = np.random.default_rng(seed)
    out, size, pos = [], 0, 10000 + int(rng.integers(0, 1000))
    while size < n_bytes:
        if rng.random() < 0.9:
            span = int(rng.integers(1, 400))
            dp = int(rng.integers(18, 45))
            line = "chr20\t%d\t.\t%s\t.\t.\tPASS\tEND=%d;BLOCKAVG_min30p3a\tGT:GQX:DP:DPF:MIN_DP\t0/0:%d:%d:%d:%d\n" % (
                pos, "ACGT"[int(rng.integers(0, 4))], pos + span, min(3 * dp, 99), dp, int(rng.integers(0, 4)), dp - int(rng.integers(0, 6)))
            pos += span + 1
        else:
            ref, alt = rng.choice(4, 2, replace=False)
            dp = int(rng.integers(18, 45))
            a = int(rng.integers(5, dp - 4))
            line = "chr20\t%d\t.\t%s\t%s\t%d\tPASS\tSNVHPOL=%d;MQ=60\tGT:GQ:GQX:DP:DPF:AD:ADF:ADR:SB:FT:PL\t0/1:%d:%d:%d:%d:%d,%d:%d,%d:%d,%d:%.1f:PASS:%d,0,%d\n" % (
                pos, "ACGT"[ref], "ACGT"[alt], int(rng.integers(20, 400)), int(rng.integers(2, 9)), int(rng.integers(30, 300)),
                int(rng.integers(20, 99)), dp, int(rng.integers(0, 4)), dp - a, a, (dp - a) // 2, a // 2, dp - a - (dp - a) // 2, a - a // 2,
                -float(rng.integers(50, 400)) / 10, int(rng.integers(50, 370)), int(rng.integers(50, 370)))
            pos += 1
        out.append(line)
        size += len(line)
    return "".join(out).encode()[:n_bytes]


def _window_edge(distance):
    """a 40-byte marker of non-zero bytes, zeros, and the marker again `distance` bytes after its first copy: the zeros touch one slot
    of any hash table, so whether the second copy becomes a match is decided by the window alone"""
    marker = bytes(np.random.default_rng(41).integers(1, 256, 40, dtype=np.uint8))
    return marker + bytes(distance - 40) + marker + b"tail"


def _skewed():
    """byte frequencies that follow the Fibonacci numbers: a deep literal/length code.  It does NOT pass 15 bits (the end of the
    block is a third leaf of weight 1 and the matcher takes frequent letters into matches: depth 14); the inputs that reach the
    three length limits are ll_fold, dist_fold and cl_fold of tests/test_bgzf_deflate_model.py"""
    fib = [1, 1]
    while len(fib) < 22:
        fib.append(fib[-1] + fib[-2])
    data = np.concatenate([np.full(f, 65 + i, np.uint8) for i, f in enumerate(fib)])
    return bytes(np.random.default_rng(23).permutation(data))


@functools.lru_cache(maxsize=None)
def _inputs():
    rng = np.random.default_rng(5)
    run258 = bytes(rng.integers(0, 256, 258, dtype=np.uint8))
    return {
        "empty": b"",
        "one_byte": b"x",
        "cut_minus_1": _text(CUT - 1, 11),
        "cut": _text(CUT, 12),
        "cut_plus_1": _text(CUT + 1, 13),
        "zeros_200000": bytes(200000),
        "random_70000": bytes(np.random.default_rng(17).integers(0, 256, 70000, dtype=np.uint8)),
        "all_bytes_twice": bytes(range(256)) * 2,
        "repeat_3": b"abc" + b"-" + b"abc" + b"+" + b"abcabcabc",
        "repeat_258": b"<" + run258 + b"|" + run258 + b">",
        "repeat_259": b"<" + run258 + b"Q" + b"|" + run258 + b"Q" + b">",
        "window_32768": _window_edge(32768),
        "window_32769": _window_edge(32769),
        "text_300k": _text(300000, 19),
        "skewed_46k": _skewed(),
    }


@functools.lru_cache(maxsize=None)
def _deflated(name, level, with_eof):
    """one compression per (input, level, eof), shared by the tests"""
    capi.init(0)
    return capi.bgzf_deflate(_inputs()[name], level=level, with_eof=with_eof)


def _members(stream):
    """[(offset, length)] by walking BSIZE"""
    out, off = [], 0
    while off < len(stream):
        assert len(stream) - off >= 28, "a member is cut short"
        bsize = struct.unpack_from("<H", stream, off + 16)[0]
        out.append((off, bsize + 1))
        off += bsize + 1
    assert off == len(stream)
    return out


def _zlib_walk(stream):
    out, rest = [], stream
    while rest:
        d = zlib.decompressobj(31)
        out.append(d.decompress(rest))
        assert d.eof
        rest = d.unused_data
    return out


def _data_members(name, level, with_eof):
    stream = _deflated(name, level, with_eof)
    m = _members(stream)
    if with_eof:
        assert stream[m[-1][0]:] == EOF_BLOCK
        m = m[:-1]
    return stream, m


# ---- without a device ------------------------------------------------------------------------------------------------------------------


def test_bound_is_host_arithmetic(built):
    assert capi.bgzf_deflate_bound(0, True) == 28 and capi.bgzf_deflate_bound(0, False) == 0
    prev = {True: 28, False: 0}
    for n in (1, 2, 100, CUT - 1, CUT, CUT + 1, 2 * CUT, 2 * CUT + 1, 300000, 30 * 1000 * 1000, 1 << 33):
        for eof in (True, False):
            b = capi.bgzf_deflate_bound(n, eof)
            assert b >= -(-n // CUT) * (CUT + 5 + 26) + (28 if eof else 0)
            assert b >= prev[eof]
            prev[eof] = b
    assert capi.lib().sk_bgzf_deflate_bound(-1, 1) == -1


def test_bound_is_monotone_across_the_cut(built):
    b = [capi.bgzf_deflate_bound(n, True) for n in range(CUT - 3, CUT + 4)] + [capi.bgzf_deflate_bound(n, True) for n in range(2 * CUT - 2, 2 * CUT + 3)]
    assert all(x <= y for x, y in zip(b, b[1:]))


def test_no_cpu_fallback(built):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(capi.StrelkaAmdError):
        capi.bgzf_deflate(b"x")


def test_arguments_are_checked(built):
    """bad arguments are refused with a message, with or without a device"""
    L = capi.lib()
    import ctypes as C
    data = np.frombuffer(b"hello", np.uint8)
    out = np.zeros(capi.bgzf_deflate_bound(5), np.uint8)
    n = C.c_int64(0)
    for args, word in (((None, 5, 2, 1, capi._p(out), len(out), C.byref(n)), "null"),
                       ((capi._p(data), -1, 2, 1, capi._p(out), len(out), C.byref(n)), "negative"),
                       ((capi._p(data), 5, 3, 1, capi._p(out), len(out), C.byref(n)), "level"),
                       ((capi._p(data), 5, -1, 1, capi._p(out), len(out), C.byref(n)), "level"),
                       ((capi._p(data), 5, 2, 1, capi._p(out), len(out) - 1, C.byref(n)), "out_cap"),
                       ((capi._p(data), 5, 2, 1, None, len(out), C.byref(n)), "null"),
                       ((capi._p(data), 5, 2, 1, capi._p(out), len(out), None), "null")):
        assert L.sk_bgzf_deflate(*args) != 0
        assert word in capi.last_error()
    assert L.sk_bgzf_deflate_dev(None, 5, 2, 1, None, 1 << 20, None, None) != 0 and "null" in capi.last_error()
    assert L.sk_bgzf_deflate_dev(None, 0, 7, 1, None, 1 << 20, None, None) != 0 and "level" in capi.last_error()


# ---- on the device ----------------------------------------------------------------------------------------------------------------------


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(_inputs()))
def test_stream_is_bgzf_and_restores_the_input(name):
    data = _inputs()[name]
    slices = [data[i:i + CUT] for i in range(0, len(data), CUT)]
    for level in LEVELS:
        for with_eof in (True, False):
            stream = _deflated(name, level, with_eof)
            # 1. zlib reads every member
            parts = _zlib_walk(stream)
            assert b"".join(parts) == data, (level, with_eof)
            assert len(parts) == len(slices) + (1 if with_eof else 0)
            if not data:
                assert stream == (EOF_BLOCK if with_eof else b"")
            # 2. the framing of every block
            _, members = _data_members(name, level, with_eof)
            assert len(members) == len(slices)
            for (off, length), want in zip(members, slices):
                m = stream[off:off + length]
                assert m[:16] == HEADER
                assert struct.unpack_from("<H", m, 16)[0] == length - 1
                assert length <= 65536
                crc, isize = struct.unpack_from("<II", m, length - 8)
                assert crc == zlib.crc32(want) and isize == len(want) <= CUT
                assert zlib.decompress(m[18:-8], -15) == want
            # 3. the project's own kernels read it
            arr = np.frombuffer(stream, np.uint8)
            block_off, out_off = capi.bgzf_scan(arr)
            assert len(block_off) - 1 == len(members) + (1 if with_eof else 0)
            assert int(out_off[-1]) == len(data)
            if data:
                assert capi.bgzf_inflate(arr).tobytes() == data, (level, with_eof)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(_inputs()))
def test_two_calls_give_identical_bytes(name):
    capi.init(0)
    for level in LEVELS:
        again = capi.bgzf_deflate(_inputs()[name], level=level, with_eof=True)
        assert again == _deflated(name, level, True), level


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(_inputs()))
def test_levels_are_ordered_per_block(name):
    data = _inputs()[name]
    sizes = [[length for _, length in _data_members(name, level, True)[1]] for level in LEVELS]
    n_blocks = -(-len(data) // CUT)
    assert [len(s) for s in sizes] == [n_blocks] * 3
    for b in range(n_blocks):
        n = min(CUT, len(data) - b * CUT)
        assert sizes[0][b] == n + 5 + 26  # stored
        assert sizes[2][b] <= sizes[1][b] <= sizes[0][b], b
    if name == "random_70000":  # nothing to find: every block falls back to stored, at every level
        assert sizes[1] == sizes[0] and sizes[2] == sizes[0]
        stream, members = _data_members(name, 2, True)
        for off, _ in members:
            assert stream[off + 18] & 7 == 1  # BFINAL 1, BTYPE 00
    if name in ("zeros_200000", "text_300k", "cut", "cut_minus_1", "cut_plus_1"):
        assert sum(sizes[1]) < sum(sizes[0]) // 2 and sum(sizes[2]) < sum(sizes[0]) // 2
    if name == "zeros_200000":  # distance 1, length 258, chained: about 1/8 bit a byte, far below what literals alone could reach
        assert sum(sizes[1]) < 200000 // 100 and sum(sizes[2]) < 200000 // 100
    if name in ("repeat_258", "repeat_259"):  # the repeat is found: the second copy costs a few bytes, not its length
        assert sizes[1][0] < sizes[0][0] - 200
    if name == "window_32768":
        # at the window's edge the second marker is one match (at most 15 + 5 + 15 + 13 bits = 6 bytes); one byte further
        # (window_32769) it is 40 literals of an alphabet of 41 symbols, at least 5 bits each = 25 bytes: 10 bytes leaves room for the
        # two code tables to differ
        for level in (1, 2):
            inside = _data_members("window_32768", level, True)[1][0][1]
            outside = _data_members("window_32769", level, True)[1][0][1]
            assert inside + 10 <= outside, level


@pytest.mark.gpu
def test_text_fixture_is_near_zlib_level_1():
    """level 2 against zlib level 1 over the same slices + 26 bytes of framing each (a one-probe greedy matcher with dynamic codes is
    zlib level 1's strategy); the margin is over zlib's figure"""
    data = _inputs()["text_300k"]
    base = 0
    for i in range(0, len(data), CUT):
        c = zlib.compressobj(level=1, wbits=-15)
        base += len(c.compress(data[i:i + CUT]) + c.flush()) + 26
    ours = {level: len(_deflated("text_300k", level, False)) for level in LEVELS}
    print("text fixture: %d bytes; zlib level 1 + framing %d; level 1 %d, level 2 %d; excess %.4f"
          % (len(data), base, ours[1], ours[2], ours[2] / base - 1.0))
    assert ours[2] <= base * (1.0 + TEXT_MARGIN)


@pytest.mark.gpu
def test_device_entry_point_equals_the_host_one():
    import ctypes as C
    import torch
    if capi.lib().sk_broker_client():
        pytest.skip("not available to a broker client: the *_dev entry points need a GPU context of the caller's")
    capi.init(0)
    L = capi.lib()
    for name in ("empty", "one_byte", "cut_plus_1", "zeros_200000", "random_70000", "text_300k"):
        data = _inputs()[name]
        n_blocks = -(-len(data) // CUT)
        for level, with_eof in ((0, True), (1, False), (2, True), (2, False)):
            want = _deflated(name, level, with_eof)
            cap = capi.bgzf_deflate_bound(len(data), with_eof)
            d_in = torch.from_numpy(np.frombuffer(data if data else b"\0", np.uint8).copy()).cuda()
            d_out = torch.zeros(max(cap, 1), dtype=torch.uint8, device="cuda")
            d_end = torch.full((n_blocks + 1,), -1, dtype=torch.int64, device="cuda")
            torch.cuda.synchronize()
            capi._check(L.sk_bgzf_deflate_dev(C.c_void_p(d_in.data_ptr()), len(data), level, int(with_eof), C.c_void_p(d_out.data_ptr()), cap,
                                              C.c_void_p(d_end.data_ptr()), C.c_void_p(torch.cuda.current_stream().cuda_stream)))
            torch.cuda.synchronize()
            end = d_end.cpu().numpy()
            assert int(end[-1]) == len(want)
            assert d_out.cpu().numpy()[:len(want)].tobytes() == want, (name, level, with_eof)
            members = _members(want)
            ends = [off + length for off, length in members]
            assert list(end[:n_blocks]) == ends[:n_blocks]
            assert int(end[n_blocks]) == (ends[-1] if ends else 0)


@pytest.mark.gpu
@pytest.mark.skipif(not os.path.exists(BGZIP), reason="oracle/_ref bgzip not built")
def test_bgzip_reads_it(tmp_path):
    for name, data in _inputs().items():
        for level in LEVELS:
            path = tmp_path / ("%s_%d.gz" % (name, level))
            path.write_bytes(_deflated(name, level, True))
            got = subprocess.run([BGZIP, "-dc", str(path)], stdout=subprocess.PIPE, check=True).stdout
            assert got == data, (name, level)


@functools.lru_cache(maxsize=None)
def _bam_again():
    """the fixture's BAM stream, deflated anew at level 2"""
    capi.init(0)
    with open(TINY, "rb") as f:
        image = np.frombuffer(f.read(), np.uint8)
    stream = capi.bgzf_inflate(image)
    return stream, capi.bgzf_deflate(stream, level=2, with_eof=True)


@pytest.mark.gpu
def test_bam_stream_survives_the_round_trip():
    stream, again = _bam_again()
    assert len(again) < len(stream) // 2
    back = capi.bgzf_inflate(np.frombuffer(again, np.uint8))
    assert back.tobytes() == stream.tobytes()
    a, b = capi.bam_decode(stream), capi.bam_decode(back)
    assert len(a["rec"]) == len(b["rec"]) == 687
    for k in a:
        assert np.array_equal(a[k], b[k]), k


@pytest.mark.gpu
@pytest.mark.skipif(not os.path.exists(SAMTOOLS), reason="oracle/_ref samtools not built")
def test_samtools_views_the_recompressed_bam(tmp_path):
    _, again = _bam_again()
    path = tmp_path / "again.bam"
    path.write_bytes(again)
    got = subprocess.run([SAMTOOLS, "view", str(path)], stdout=subprocess.PIPE, check=True).stdout.decode().splitlines()
    with gzip.open(os.path.join(GOLD, "feed_tiny.sam.txt.gz"), "rt") as f:
        want = [l.rstrip("\n").split("\t") for l in f]
    assert len(got) == len(want) == 687
    for line, w in zip(got, want):
        g = line.split("\t")
        assert [g[1], g[2], g[3], g[4], g[5], g[9], g[10]] == w[:7]
