"""The read intake on the device (sk_read_intake, csrc/read_intake.hip): every field of every output equals the rule-by-rule model
(tests/intake_model.py, itself pinned to vectors recorded from the reference by tests/test_read_intake_model.py)."""
import ctypes as C
import functools
import json
import os
import subprocess
import sys
import uuid

import numpy as np
import pytest

from strelka_amd import capi, synth
from tests import intake_cases as K
from tests import intake_model as M

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TINY = os.path.join(GOLD, "feed_tiny.bam")
OBS_FIELDS = ("read", "pos", "deletion_length", "ins_begin", "ins_len", "bp_begin", "bp_len", "type", "is_noise", "is_low_mapq")


def _opt(max_indel_size=M.MAX_INDEL_SIZE, fraction=None):
    o = capi.intake_options()
    o.max_indel_size = max_indel_size
    if fraction is not None:
        o.min_alt_allele_fraction = fraction
    return o


def _as_model(got):
    """the device's arrays in the model's form"""
    return dict(reads=[(int(r["valid_begin"]), int(r["valid_end"]), int(r["total_indel_ref_span"]), int(r["n_obs"])) for r in got["reads"]],
                obs_off=[int(x) for x in got["obs_off"]], obs=[{k: int(o[k]) for k in OBS_FIELDS} for o in got["obs"]],
                sites=[(int(s["variant_count"]), int(s["depth"])) for s in got["sites"]], is_candidate=[bool(x) for x in got["is_candidate"]])


def _assert_equal(got, want, what=""):
    got = _as_model(got)
    for key in ("reads", "obs_off", "obs", "sites", "is_candidate"):
        if got[key] != want[key]:
            bad = [i for i, (a, b) in enumerate(zip(got[key], want[key])) if a != b]
            first = bad[0] if bad else min(len(got[key]), len(want[key]))
            raise AssertionError("%s %s: %d / %d differ (lengths %d, %d); first at %d: device %r, model %r" % (
                what, key, len(bad), len(want[key]), len(got[key]), len(want[key]), first,
                got[key][first] if first < len(got[key]) else None, want[key][first] if first < len(want[key]) else None))


def _run(ref, ref_offset, reads, low, win_begin, n_pos, max_indel_size=M.MAX_INDEL_SIZE, what=""):
    capi.init(0)
    want = M.read_intake(ref, ref_offset, reads, low, win_begin, n_pos, max_indel_size)
    got = capi.read_intake(ref, ref_offset, reads, low, win_begin, n_pos, _opt(max_indel_size))
    _assert_equal(got, want, what)
    assert not got["obs"]["pad"].any()
    return got, want


def _bytes_of(got):
    return b"".join(np.ascontiguousarray(got[k]).tobytes() for k in ("reads", "obs_off", "obs", "sites", "is_candidate"))


# ---- the recorded reads and the crafted cases --------------------------------------------------------------------------------------------------------


def test_golden_reads_in_one_batch():
    g = K.golden()
    got, want = _run(g["ref"], g["ref_offset"], g["reads"], g["low"], g["win_begin"], g["n_pos"], g["max_indel_size"], "golden")
    # ... and against the recorded numbers themselves
    doc = g["doc"]
    assert [[int(r["valid_begin"]), int(r["valid_end"])] for r in got["reads"]] == [r["valid"] for r in doc["reads"]]
    assert [int(r["total_indel_ref_span"]) for r in got["reads"]] == [r["span"] for r in doc["reads"]]
    assert [(int(s["variant_count"]), int(s["depth"]), int(k)) for s, k in zip(got["sites"], got["is_candidate"])] == [tuple(s) for s in doc["sites"]]
    assert len(got["obs"]) == sum(len(r["obs"]) for r in doc["reads"])


def test_golden_reads_one_per_call():
    g = K.golden()
    for i, (rd, low) in enumerate(zip(g["reads"], g["low"])):
        span = sum(l for t, l in rd["path"] if t in (M.MATCH, M.DELETE))
        _run(g["ref"], g["ref_offset"], [rd], [low], rd["pos"] - 2, span + 4, g["max_indel_size"], "golden read %d" % i)


@pytest.mark.parametrize("case", K.crafted(), ids=lambda c: c["name"])
def test_crafted_case(case):
    got, want = _run(case["ref"], case["ref_offset"], case["reads"], case["low"], case["win_begin"], case["n_pos"], case["max_indel_size"], case["name"])
    for key, value in case["expect"].items():  # the hand-computed values, directly
        assert _as_model(got)[key] == value, key
    for i, (rd, low) in enumerate(zip(case["reads"], case["low"])):  # ... and one read per call
        _run(case["ref"], case["ref_offset"], [rd], [low], case["win_begin"], case["n_pos"], case["max_indel_size"], "%s read %d" % (case["name"], i))


def test_crafted_cases_in_one_batch():
    reads, low = K.crafted_flat()
    assert len(reads) >= 12
    _run(K.REF, K.REF_OFFSET, reads, low, 90, 120, what="crafted, one batch")


# ---- turn edges: read lengths and path lengths -----------------------------------------------------------------------------------------------------


def _long_reference(n, seed):
    return K.repeat_rich_reference(n, np.random.default_rng(seed))


@pytest.mark.parametrize("length", [1, 63, 64, 65, 128, 1023, 1024])
def test_read_lengths_at_the_turn_edges(length):
    """plain reads, reads whose forward minimum / reverse minimum falls on the last base of a turn or the first of the next, reads cut
    from both sides"""
    ref = _long_reference(1400, 41)
    reads, low = [], []
    reads.append(K.make_read(1010, [(M.MATCH, length)], ref=ref, ref_offset=1000))
    edges = {0, 1, 2, length // 2, 62, 63, 64, 127, 128, length - 65, length - 64, length - 63, length - 2, length - 1}
    for edge in sorted(e for e in edges if 0 <= e < length):
        bad_head = tuple(range(0, edge + 1))    # mismatches up to `edge`: the forward sum has its minimum exactly there
        bad_tail = tuple(range(edge, length))   # ... and the reverse sum here
        reads.append(K.make_read(1003, [(M.MATCH, length)], ref=ref, ref_offset=1000, mismatch=bad_head))
        reads.append(K.make_read(1005, [(M.MATCH, length)], ref=ref, ref_offset=1000, mismatch=bad_tail))
        reads.append(K.make_read(1007, [(M.MATCH, length)], ref=ref, ref_offset=1000, mismatch=tuple(range(0, edge // 3 + 1)) + tuple(range(length - edge // 4 - 1, length))))
    if length > 4:
        reads.append(K.make_read(1020, [(M.SOFT_CLIP, 1), (M.MATCH, length - 4), (M.INSERT, 2), (M.MATCH, 1)], ref=ref, ref_offset=1000, mismatch=(length - 1,)))
        reads.append(K.make_read(1020, [(M.MATCH, 1), (M.DELETE, 60), (M.MATCH, length - 2), (M.SOFT_CLIP, 1)], ref=ref, ref_offset=1000, mismatch=(0,)))
    reads.sort(key=lambda r: r["pos"])
    got, want = _run(ref, 1000, reads, [0] * len(reads), 995, 1200, what="length %d" % length)
    assert any(r[:2] not in ((0, length), (0, 0)) for r in want["reads"]) or length < 4


@pytest.mark.parametrize("n_seg", [1, 2, 64, 65, 130])
def test_path_lengths_at_the_turn_edges(n_seg):
    ref = _long_reference(1400, 43)
    rng = np.random.default_rng(4300 + n_seg)
    reads = []
    for k in range(6):
        if n_seg == 1:
            path = [(M.MATCH, 40 + k)]
        elif n_seg == 2:
            path = [[(M.SOFT_CLIP, 3), (M.MATCH, 40)], [(M.MATCH, 40), (M.SOFT_CLIP, 3)], [(M.INSERT, 2), (M.MATCH, 30)], [(M.MATCH, 30), (M.DELETE, 2)],
                    [(M.HARD_CLIP, 2), (M.MATCH, 9)], [(M.MATCH, 9), (M.INSERT, 4)]][k]
        else:  # match, indel, match, ... with a swap here and there (two segments), clipped to n_seg segments, ending in a match
            path = []
            while len(path) < n_seg:
                path.append((M.MATCH, int(rng.integers(1, 8))))
                room = n_seg - len(path)
                if room >= 3 and rng.random() < 0.3:
                    path += [(M.INSERT, int(rng.integers(1, 4))), (M.DELETE, int(rng.integers(1, 4)))][::(1 if rng.random() < 0.5 else -1)]
                elif room >= 2:
                    path.append((M.INSERT, int(rng.integers(1, 4))) if rng.random() < 0.5 else (M.DELETE, int(rng.integers(1, 4))))
                elif room == 1:
                    path.append((M.SOFT_CLIP, 2))
            assert len(path) == n_seg
        reads.append(K.make_read(1005 + 3 * k, path, ref=ref, ref_offset=1000, mismatch=tuple(int(x) for x in rng.integers(0, 30, 3)),
                                 inserted="ACGT"[k % 4]))
    got, want = _run(ref, 1000, reads, [0, 0, 1, 0, 0, 0], 990, 900, what="%d segments" % n_seg)
    if n_seg >= 64:
        assert min(r[3] for r in want["reads"]) > 10


# ---- seeded batches --------------------------------------------------------------------------------------------------------------------------------------


@functools.lru_cache(maxsize=None)
def _normalised_batch(n_reads, read_len, ref_len, seed):
    """the generator's reads through sk_normalize_alignments, as the feed leaves them -> (ref, ref_offset, reads, low)"""
    capi.init(0)
    ref, off, reads, low = K.random_batch(n_reads, read_len, ref_len, seed)
    out = capi.normalize_alignments(ref, off, reads)
    assert sum(ch for ch, _, _ in out) > 10
    reads = [dict(code=r["code"], pos=p, path=path) for r, (_, p, path) in zip(reads, out)]
    reads, low = K.usable(reads, low)
    assert len(reads) > 0.95 * n_reads
    order = sorted(range(len(reads)), key=lambda i: reads[i]["pos"])  # (normalisation moves a few positions)
    return ref, off, [reads[i] for i in order], [low[i] for i in order]


def test_batch_of_3000_reads_over_10_kb():
    ref, off, reads, low = _normalised_batch(3000, 150, 10000, 7001)
    got, want = _run(ref, off, reads, low, off - 60, 10300, what="3000 reads")
    assert len(want["obs"]) > 1000 and sum(want["is_candidate"]) > 500


def test_the_feeds_own_normalisation_cases():
    """strelka_amd.synth.normalize_cases (what tests/test_bam_feed.py normalises), every case on a stretch of its own of one reference"""
    capi.init(0)
    cases = synth.normalize_cases(400, np.random.default_rng(7002))
    ref, reads = "", []
    for c in cases:
        base = 5000 + len(ref)
        reads.append(dict(code=c["code"], pos=base + (c["pos"] - c["ref_offset"]), path=c["path"]))
        ref += c["ref_seq"]
    out = capi.normalize_alignments(ref, 5000, reads)
    reads = [dict(code=r["code"], pos=p, path=path) for r, (_, p, path) in zip(reads, out)]
    reads, low = K.usable(reads, [int(i % 7 == 0) for i in range(len(reads))])
    assert len(reads) > 300
    _run(ref, 5000, reads, low, 4990, len(ref) + 20, what="normalize_cases")


def test_pile_of_4000_reads_at_one_position():
    """contention on one counter: the model runs the read once -- the counters are sums, so 4 000 copies are 4 000 times one copy"""
    capi.init(0)
    ref, off, reads, low = _normalised_batch(3000, 150, 10000, 7001)
    for rd in (r for r, l in zip(reads, low) if not l and any(t == M.INSERT for t, _ in r["path"]) and r["pos"] > off + 100):
        one = M.read_intake(ref, off, [rd], [0], rd["pos"] - 5, 200)
        if any(o["type"] == M.INDEL_INDEL and o["ins_len"] and not o["deletion_length"] for o in one["obs"]):  # a primitive insertion: count 4
            break
    n = 4000
    got = _as_model(capi.read_intake(ref, off, [rd] * n, [0] * n, rd["pos"] - 5, 200))
    assert got["reads"] == one["reads"] * n
    assert got["obs_off"] == [len(one["obs"]) * i for i in range(n + 1)]
    assert got["obs"] == [dict(o, read=i) for i in range(n) for o in one["obs"]]
    assert got["sites"] == [(c * n, d * n) for c, d in one["sites"]]
    assert got["is_candidate"] == [M.is_candidate_variant(M.ref_char(ref, off, rd["pos"] - 5 + i), c * n, d * n) for i, (c, d) in enumerate(one["sites"])]
    assert max(c for c, _ in got["sites"]) >= 4 * n


def test_window_narrower_than_the_reads_and_of_one_position():
    ref, off, reads, low = _normalised_batch(3000, 150, 10000, 7001)
    sub, sub_low = reads[1000:1400], low[1000:1400]
    lo, hi = sub[0]["pos"], sub[-1]["pos"] + 150
    _run(ref, off, sub, sub_low, lo + 200, hi - lo - 400, what="narrow window")  # cut on both sides
    got, want = _run(ref, off, sub, sub_low, (lo + hi) // 2, 1, what="n_pos 1")
    assert want["sites"][0][1] > 10
    _run(ref, off, sub, sub_low, hi + 5000, 50, what="window beside the reads")


def test_no_reads():
    capi.init(0)
    ref = "ACGTNNACGT"
    got = capi.read_intake(ref, 100, [], [], 98, 14)
    assert len(got["reads"]) == 0 and list(got["obs_off"]) == [0] and len(got["obs"]) == 0
    assert [tuple(int(x) for x in s) for s in got["sites"]] == [(0, 0)] * 14
    # the rule at depth 0: count 0 >= 0.35f * 0, so every position whose reference is not N is a candidate
    assert list(got["is_candidate"]) == [False, False, True, True, True, True, False, False, True, True, True, True, False, False]
    got = capi.read_intake(ref, 100, [], [], 98, 0)
    assert len(got["sites"]) == 0 and len(got["is_candidate"]) == 0


def test_min_alt_allele_fraction_is_used():
    capi.init(0)
    g = K.golden()
    for f in (0.05, 0.5):
        want = M.read_intake(g["ref"], g["ref_offset"], g["reads"], g["low"], g["win_begin"], g["n_pos"], g["max_indel_size"], min_alt_allele_fraction=f)
        got = capi.read_intake(g["ref"], g["ref_offset"], g["reads"], g["low"], g["win_begin"], g["n_pos"], _opt(g["max_indel_size"], f))
        _assert_equal(got, want, "fraction %g" % f)


def test_two_calls_give_identical_bytes():
    capi.init(0)
    ref, off, reads, low = _normalised_batch(3000, 150, 10000, 7001)
    a = capi.read_intake(ref, off, reads, low, off - 60, 10300)
    b = capi.read_intake(ref, off, reads, low, off - 60, 10300)
    assert _bytes_of(a) == _bytes_of(b)
    g = K.golden()
    c = [capi.read_intake(g["ref"], g["ref_offset"], g["reads"], g["low"], g["win_begin"], g["n_pos"]) for _ in range(2)]
    assert _bytes_of(c[0]) == _bytes_of(c[1])


# ---- chained on the feed, on one stream ---------------------------------------------------------------------------------------------------------------------


def _consensus_reference(d, first, size):
    """a reference the fixture's reads mostly agree with: the majority base of their match segments per position"""
    votes = np.zeros((size, 16), np.int64)
    for i in range(len(d["rec"])):
        p, q = int(d["rec"]["pos"][i]) - first, int(d["read_off"][i])
        for t, l in d["path"][int(d["path_off"][i]):int(d["path_off"][i + 1])]:
            t, l = int(t), int(l)
            if M.is_match(t):
                for j in range(l):
                    if 0 <= p + j < size:
                        votes[p + j, d["read_code"][q + j]] += 1
                p += l
                q += l
            elif t in (M.INSERT, M.SOFT_CLIP):
                q += l
            elif t == M.DELETE:
                p += l
    best = votes[:, [1, 2, 4, 8]].argmax(axis=1)
    return "".join("ACGT"[b] if votes[k].sum() else "N" for k, b in enumerate(best))


def test_device_chain_equals_the_host_entry_on_the_bam_fixture():
    """sk_bam_decode_dev -> sk_normalize_alignments_dev -> sk_read_intake_dev on one stream, no host copy in between, read_code at an
    unaligned device address (base + 1 element)"""
    import torch
    if capi.lib().sk_broker_client():
        pytest.skip("not available to a broker client: the *_dev entry points need a GPU context of the caller's")
    capi.init(0)
    L = capi.lib()
    with open(TINY, "rb") as f:
        stream = capi.bgzf_inflate(np.frombuffer(f.read(), np.uint8))
    d = capi.bam_decode(stream)
    n_all = len(d["rec"])
    assert n_all == 687
    first = int(d["rec"]["pos"].min()) - 20
    ref = _consensus_reference(d, first, int(d["rec"]["pos"].max()) - first + 400)
    # the host's way: normalise, drop what the intake refuses, sort by position (as the reference's stream delivers them)
    host_reads = [dict(code=d["read_code"][int(d["read_off"][i]):int(d["read_off"][i + 1])], pos=int(d["rec"]["pos"][i]),
                       path=[(int(t), int(l)) for t, l in d["path"][int(d["path_off"][i]):int(d["path_off"][i + 1])]]) for i in range(n_all)]
    norm = capi.normalize_alignments(ref, first, host_reads)
    keep = []
    for i, (_, p, path) in enumerate(norm):
        try:
            M.check_path(path, len(host_reads[i]["code"]))
            keep.append(i)
        except M.PathError:
            pass
    assert len(keep) > 650
    low = [int(d["rec"]["mapq"][i] == 0) for i in keep]
    assert sum(low) > 5
    want = capi.read_intake(ref, first, [dict(code=host_reads[i]["code"], pos=norm[i][1], path=norm[i][2]) for i in keep], low, first, len(ref))
    assert len(want["obs"]) > 10
    _assert_equal(want, M.read_intake(ref, first, [dict(code=host_reads[i]["code"], pos=norm[i][1], path=norm[i][2]) for i in keep], low, first, len(ref)), "host entry")

    # the device's way, on the kept records
    n = len(keep)
    rec_off = np.ascontiguousarray(d["rec_off"][keep])
    read_off = np.zeros(n + 1, np.int64)
    path_off = np.zeros(n + 1, np.int64)
    for k, i in enumerate(keep):
        read_off[k + 1] = read_off[k] + (d["read_off"][i + 1] - d["read_off"][i])
        path_off[k + 1] = path_off[k] + (d["path_off"][i + 1] - d["path_off"][i])
    n_bases, n_segs = int(read_off[-1]), int(path_off[-1])
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    p = lambda t: C.c_void_p(t.data_ptr())
    d_stream, d_rec_off, d_read_off, d_path_off = dev(stream), dev(rec_off), dev(read_off), dev(path_off)
    d_rec = torch.zeros(n * capi.BAM_RECORD_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    d_code = torch.zeros(n_bases + 9, dtype=torch.uint8, device="cuda")[1:]   # base + 1 element
    d_qual = torch.zeros(n_bases + 9, dtype=torch.uint8, device="cuda")[1:]
    d_path = torch.zeros(2 * n_segs + 2, dtype=torch.int32, device="cuda")
    assert d_code.data_ptr() % 4 == 1
    d_ref = dev(np.frombuffer(ref.encode(), np.uint8).copy())
    d_low = dev(np.array(low, np.uint8))
    d_changed = torch.zeros(n, dtype=torch.uint8, device="cuda")
    cap = capi.read_intake_obs_bound(n_segs)
    d_reads = torch.zeros(n * 16, dtype=torch.uint8, device="cuda")
    d_obs_off = torch.full((n + 1,), -1, dtype=torch.int64, device="cuda")
    d_obs = torch.zeros(cap * 32, dtype=torch.uint8, device="cuda")
    d_sites = torch.full((len(ref),), -1, dtype=torch.int64, device="cuda")
    d_cand = torch.full((len(ref),), 7, dtype=torch.uint8, device="cuda")
    scratch_bytes = L.sk_read_intake_scratch_bytes(n, n_segs, len(ref))
    d_scratch = torch.zeros(scratch_bytes, dtype=torch.uint8, device="cuda")
    opt = capi.intake_options()
    torch.cuda.synchronize()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    capi._check(L.sk_bam_decode_dev(p(d_stream), p(d_rec_off), n, p(d_read_off), p(d_path_off), p(d_rec), p(d_code), p(d_qual), p(d_path), st))
    # n_seg and pos of the normalisation come from the decoded records: two small strided copies on the same stream (device to device)
    rec32 = d_rec.view(torch.int32).view(n, capi.BAM_RECORD_DTYPE.itemsize // 4)
    d_pos = rec32[:, 1].contiguous()
    d_nseg = rec32[:, 6].contiguous()
    capi._check(L.sk_normalize_alignments_dev(p(d_ref), first, len(ref), n, p(d_read_off), p(d_code), p(d_path_off), p(d_nseg), p(d_path), p(d_pos), p(d_changed), st))
    capi._check(L.sk_read_intake_dev(p(d_ref), first, len(ref), n, p(d_read_off), p(d_code), p(d_path_off), p(d_nseg), p(d_path), p(d_pos), p(d_low),
                                     C.byref(opt), first, len(ref), p(d_reads), p(d_obs_off), p(d_obs), cap, p(d_sites), p(d_cand), p(d_scratch), scratch_bytes, st))
    torch.cuda.synchronize()
    capi._check(L.sk_check_device_errors())
    assert d_pos.cpu().tolist() == [norm[i][1] for i in keep]
    obs_off = d_obs_off.cpu().numpy()
    got = dict(reads=d_reads.cpu().numpy().view(capi.INTAKE_READ_DTYPE), obs_off=obs_off,
               obs=d_obs.cpu().numpy().view(capi.INTAKE_OBS_DTYPE)[:int(obs_off[-1])], sites=d_sites.cpu().numpy().view(capi.INTAKE_SITE_DTYPE),
               is_candidate=d_cand.cpu().numpy().astype(bool))
    assert _bytes_of(got) == _bytes_of(want)


def test_device_entry_flags_what_the_host_entry_refuses():
    """a path whose read length is not the read's: the host entry says so; the device entry raises the sticky flag and stays in bounds"""
    import torch
    if capi.lib().sk_broker_client():
        pytest.skip("not available to a broker client: the *_dev entry points need a GPU context of the caller's")
    capi.init(0)
    L = capi.lib()
    reads = [K.make_read(110, [(M.MATCH, 20)]), dict(code=M.encode("ACGTACGTAC"), pos=112, path=[(M.MATCH, 30)]), K.make_read(114, [(M.MATCH, 20)])]
    with pytest.raises(capi.StrelkaAmdError, match="read 1"):
        capi.read_intake(K.REF, K.REF_OFFSET, reads, [0, 0, 0], 100, 60)
    read_off, code, path_off, n_seg, path, pos = capi.pack_reads(reads)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    p = lambda t: C.c_void_p(t.data_ptr())
    t = [dev(np.frombuffer(K.REF.encode(), np.uint8).copy()), dev(read_off), dev(code), dev(path_off), dev(n_seg), dev(path.view(np.uint32)), dev(pos), dev(np.zeros(4, np.uint8))]
    d_reads = torch.zeros(3 * 16, dtype=torch.uint8, device="cuda")
    d_obs_off = torch.zeros(4, dtype=torch.int64, device="cuda")
    d_obs = torch.zeros(6 * 32, dtype=torch.uint8, device="cuda")
    d_sites = torch.zeros(60, dtype=torch.int64, device="cuda")
    d_cand = torch.zeros(60, dtype=torch.uint8, device="cuda")
    d_scratch = torch.zeros(512, dtype=torch.uint8, device="cuda")
    opt = capi.intake_options()
    torch.cuda.synchronize()
    capi._check(L.sk_read_intake_dev(p(t[0]), K.REF_OFFSET, len(K.REF), 3, p(t[1]), p(t[2]), p(t[3]), p(t[4]), p(t[5]), p(t[6]), p(t[7]), C.byref(opt), 100, 60,
                                     p(d_reads), p(d_obs_off), p(d_obs), 6, p(d_sites), p(d_cand), p(d_scratch), 512, C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    assert L.sk_check_device_errors() != 0 and "sk_read_intake_dev" in capi.last_error()
    assert L.sk_check_device_errors() == 0  # (cleared)
    rec = d_reads.cpu().numpy().view(capi.INTAKE_READ_DTYPE)
    assert (int(rec[0]["valid_begin"]), int(rec[0]["valid_end"])) == (0, 20) and (int(rec[2]["valid_begin"]), int(rec[2]["valid_end"])) == (0, 20)


# ---- through the broker ------------------------------------------------------------------------------------------------------------------------------------

BROKER_CLIENT = r'''
import hashlib, json, sys
import numpy as np
sys.path.insert(0, %r)
from strelka_amd import capi
from tests import intake_cases as K
capi.init(0)
g = K.golden()
got = capi.read_intake(g["ref"], g["ref_offset"], g["reads"], g["low"], g["win_begin"], g["n_pos"])
h = hashlib.sha256(b"".join(np.ascontiguousarray(got[k]).tobytes() for k in ("reads", "obs_off", "obs", "sites", "is_candidate"))).hexdigest()
print(json.dumps(dict(client=capi.lib().sk_broker_client(), digest=h, n_obs=int(len(got["obs"])))))
'''


def test_through_the_broker(tmp_path):
    import hashlib
    capi.init(0)
    g = K.golden()
    direct = capi.read_intake(g["ref"], g["ref_offset"], g["reads"], g["low"], g["win_begin"], g["n_pos"])
    env = dict(os.environ, STRELKA_AMD_BROKER="1", STRELKA_AMD_BROKER_SOCKET="sktest_" + uuid.uuid4().hex[:12], STRELKA_AMD_BROKER_LOG=str(tmp_path / "broker.log"),
               STRELKA_AMD_BROKER_IDLE_S="2")
    p = subprocess.run([sys.executable, "-c", BROKER_CLIENT % REPO], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert p.returncode == 0, p.stderr.decode()[-3000:]
    res = json.loads(p.stdout.decode().strip().splitlines()[-1])
    assert res["client"] == 1
    assert res["n_obs"] == len(direct["obs"]) > 300
    assert res["digest"] == hashlib.sha256(_bytes_of(direct)).hexdigest()
