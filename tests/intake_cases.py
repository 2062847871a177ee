"""Inputs of the read-intake tests, shared by the model tests (tests/test_read_intake_model.py) and the device tests
(tests/test_read_intake.py): the recorded reference vectors, the crafted cases with their hand-computed values, and the generators of
the seeded batches.  Imports neither the product nor a device."""
import functools
import json
import os

import numpy as np

from tests import intake_model as M

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "read_intake", "intake_golden.json")
MS, IN, DE, SC, HC = M.MATCH, M.INSERT, M.DELETE, M.SOFT_CLIP, M.HARD_CLIP

REF_OFFSET = 100
REF = "ACGTTGCATCAGGATCCTAAGCTTGACCATGGTACGATTCAGGCATTCGAACTGGTCATAGCTAGGATTACAGCTTGCAAGTCCGATAGGCTTAACGTGCAT" * 2  # 100..299


@functools.lru_cache(maxsize=None)
def golden():
    """-> dict(doc, ref, ref_offset, reads, low, win_begin, n_pos): the reads the reference's own intake was recorded on"""
    with open(GOLDEN) as f:
        doc = json.load(f)
    reads = [dict(code=M.encode(r["seq"]), pos=r["pos"], path=[tuple(s) for s in r["path"]]) for r in doc["reads"]]
    return dict(doc=doc, ref=doc["ref"], ref_offset=doc["ref_offset"], reads=reads, low=[r["low_mapq"] for r in doc["reads"]],
                win_begin=doc["site_begin"], n_pos=len(doc["sites"]), max_indel_size=doc["max_indel_size"])


def other(base):
    return {"A": "C", "C": "G", "G": "T", "T": "A", "N": "A"}[base]


def make_read(pos, path, ref=REF, ref_offset=REF_OFFSET, mismatch=(), inserted="T", literal=None):
    """a read that follows `ref` along `path` from `pos`: match bases copy the reference (positions outside it: N), read offsets in
    `mismatch` take another base, inserted and clipped bases are `inserted`; `literal` maps read offsets to given characters"""
    seq, p = [], pos
    for t, l in path:
        if M.is_match(t):
            for j in range(l):
                b = M.ref_char(ref, ref_offset, p + j)
                seq.append(other(b) if len(seq) in mismatch else b)
            p += l
        elif t in (IN, SC):
            seq += [inserted] * l
        elif t == DE:
            p += l
    for k, c in (literal or {}).items():
        seq[k] = c
    return dict(code=M.encode("".join(seq)), pos=pos, path=list(path))


def _case(name, batch, low=None, win=(100, 60), max_indel_size=M.MAX_INDEL_SIZE, ref=REF, ref_offset=REF_OFFSET, **expect):
    return dict(name=name, ref=ref, ref_offset=ref_offset, reads=batch, low=low or [0] * len(batch), win_begin=win[0], n_pos=win[1],
                max_indel_size=max_indel_size, expect=expect)


def _sites(spec, win_begin, n_pos):
    """{pos or (first, last): (count, depth)} -> the window's list, zero elsewhere"""
    out = [(0, 0)] * n_pos
    for k, v in spec.items():
        a, b = k if isinstance(k, tuple) else (k, k)
        for p in range(a, b + 1):
            out[p - win_begin] = v
    return out


def _o(read, pos, otype, noise=0, low=0, dele=0, ins=(0, 0), bp=(0, 0)):
    return dict(read=read, pos=pos, deletion_length=dele, ins_begin=ins[0], ins_len=ins[1], bp_begin=bp[0], bp_len=bp[1], type=otype, is_noise=noise,
                is_low_mapq=low)


@functools.lru_cache(maxsize=None)
def crafted():
    """the crafted cases; `expect` holds values worked out by hand from the reference's rules (the comments say how)"""
    I, L, R = M.INDEL_INDEL, M.INDEL_BP_LEFT, M.INDEL_BP_RIGHT
    c = []
    # leading soft clip: count 4 + depth at al.pos - 1 = 109, count 4 alone at al.pos = 110 (which also has its match's depth);
    # trailing soft clip: count 4 + depth at the reference head 120, count 4 alone at 119
    c.append(_case("soft_clips", [make_read(110, [(SC, 3), (MS, 10), (SC, 2)])],
                   reads=[(0, 15, 0, 0)], obs=[], sites=_sites({109: (4, 1), 110: (4, 1), (111, 118): (0, 1), 119: (4, 1), 120: (4, 1)}, 100, 60)))
    # insertion of 2 at reference position 115: count 4 + depth at 114 and 115, on top of the matches' depth there
    c.append(_case("insertion", [make_read(110, [(MS, 5), (IN, 2), (MS, 5)])],
                   reads=[(0, 12, 0, 1)], obs=[_o(0, 115, I, ins=(5, 2))],
                   sites=_sites({(110, 113): (0, 1), 114: (4, 2), 115: (4, 2), (116, 119): (0, 1)}, 100, 60)))
    # deletion of 1 at 115: count 4 + depth at 114 (on its match) and at 115; the span returned is 1
    c.append(_case("deletion_1", [make_read(110, [(MS, 5), (DE, 1), (MS, 5)])],
                   reads=[(0, 10, 1, 1)], obs=[_o(0, 115, I, dele=1)], sites=_sites({(110, 113): (0, 1), 114: (4, 2), 115: (4, 1), (116, 120): (0, 1)}, 100, 60)))
    # deletion of 3: 114 and 115..117
    c.append(_case("deletion_3", [make_read(110, [(MS, 5), (DE, 3), (MS, 5)])],
                   reads=[(0, 10, 3, 1)], obs=[_o(0, 115, I, dele=3)], sites=_sites({(110, 113): (0, 1), 114: (4, 2), (115, 117): (4, 1), (118, 122): (0, 1)}, 100, 60)))
    # a swap is one observation (both lengths) and adds nothing to the counters; it consumes both segments
    c.append(_case("swap", [make_read(110, [(MS, 5), (IN, 2), (DE, 3), (MS, 5)]), make_read(110, [(MS, 5), (DE, 3), (IN, 2), (MS, 5)])],
                   reads=[(0, 12, 3, 1), (0, 12, 3, 1)], obs=[_o(0, 115, I, dele=3, ins=(5, 2)), _o(1, 115, I, dele=3, ins=(5, 2))],
                   sites=_sites({(110, 114): (0, 2), (118, 122): (0, 2)}, 100, 60)))
    # max_indel_size = 5: an insertion of 5 is an INDEL, of 6 a breakpoint pair with windows of 5 bases after read offset 2 and before
    # read offset 8; a deletion of 6 near the read's end has its left window clipped there (2 bases), near its start its right window
    # (2 bases), and the right breakpoint lies after the deleted bases; breakpoints add nothing, a deletion above the limit no span
    c.append(_case("max_indel_size", [make_read(110, [(MS, 2), (IN, 5), (MS, 2)]), make_read(110, [(MS, 2), (IN, 6), (MS, 2)]),
                                      make_read(110, [(MS, 8), (DE, 6), (MS, 2)]), make_read(110, [(MS, 2), (DE, 6), (MS, 8)]),
                                      make_read(110, [(MS, 2), (DE, 5), (MS, 8)])], max_indel_size=5,
                   reads=[(0, 9, 0, 1), (0, 10, 0, 2), (0, 10, 0, 2), (0, 10, 0, 2), (0, 10, 5, 1)],
                   obs=[_o(0, 112, I, ins=(2, 5)), _o(1, 112, L, bp=(2, 5)), _o(1, 112, R, bp=(3, 5)), _o(2, 118, L, bp=(8, 2)), _o(2, 124, R, bp=(3, 5)),
                        _o(3, 112, L, bp=(2, 5)), _o(3, 118, R, bp=(0, 2)), _o(4, 112, I, dele=5)]))
    # four mismatches, then an insertion: the forward sum is -25 from the insertion's first base to its last, so the valid range begins
    # after the insertion and its read range (3, 15) is outside: noise for 10 bases, cleared for 11 (> max_cand_filter_insert_size)
    c.append(_case("insert_10_invalid", [make_read(110, [(MS, 4), (IN, 10), (MS, 20)], mismatch=(0, 1, 2, 3))],
                   reads=[(14, 34, 0, 1)], obs=[_o(0, 114, I, noise=1, ins=(4, 10))],
                   sites=_sites({(110, 112): (1, 1), 113: (5, 2), 114: (4, 2), (115, 133): (0, 1)}, 100, 60)))
    c.append(_case("insert_11_invalid", [make_read(110, [(MS, 4), (IN, 11), (MS, 20)], mismatch=(0, 1, 2, 3))],
                   reads=[(15, 35, 0, 1)], obs=[_o(0, 114, I, noise=0, ins=(4, 11))]))
    # a low-MAPQ read keeps its observation, flagged, and adds nothing to the counters
    c.append(_case("low_mapq", [make_read(110, [(MS, 5), (IN, 2), (MS, 5)]), make_read(112, [(SC, 2), (MS, 6)])], low=[1, 1],
                   reads=[(0, 12, 0, 1), (0, 8, 0, 0)], obs=[_o(0, 115, I, low=1, ins=(5, 2))], sites=_sites({}, 100, 60)))
    # edge inserts and deletions of genomic reads give no observation and no counts; an edge deletion still adds to the span (:393-399)
    c.append(_case("edge_indels", [make_read(110, [(IN, 2), (MS, 10)]), make_read(110, [(MS, 10), (DE, 2)]), make_read(110, [(DE, 3), (MS, 10)]),
                                   make_read(110, [(MS, 10), (IN, 2)])],
                   reads=[(0, 12, 0, 0), (0, 10, 2, 0), (0, 10, 3, 0), (0, 12, 0, 0)], obs=[],
                   sites=_sites({(110, 112): (0, 3), (113, 119): (0, 4), (120, 122): (0, 1)}, 100, 60)))
    # a read over a short reference segment (100..107), hanging off both ends: outside it the reference reads N; the read's N there is a
    # match (count 0), its A at 108 a mismatch (count 1) -- and no position whose reference is N is a candidate
    c.append(_case("n_against_n", [make_read(97, [(MS, 14)], ref="ACGTACGT", literal={11: "A"})], ref="ACGTACGT", win=(95, 20),
                   reads=[(0, 14, 0, 0)], obs=[], sites=_sites({(97, 107): (0, 1), 108: (1, 1), (109, 110): (0, 1)}, 95, 20),
                   is_candidate=[False] * 5 + [False] * 8 + [False] * 3 + [False] * 4))
    return c


def crafted_flat():
    """every crafted read in one batch over REF (the cases on another reference or another limit left out) -> (reads, low)"""
    reads, low = [], []
    for c in crafted():
        if c["ref"] is REF and c["max_indel_size"] == M.MAX_INDEL_SIZE:
            reads += c["reads"]
            low += c["low"]
    return reads, low


def repeat_rich_reference(n, rng):
    """homopolymers, short tandem repeats and random stretches (as strelka_amd.synth.normalize_cases builds its references)"""
    parts, size = [], 0
    bases = "ACGT"
    while size < n:
        r = rng.random()
        if r < 0.35:
            s = bases[int(rng.integers(0, 4))] * int(rng.integers(3, 12))
        elif r < 0.6:
            s = "".join(bases[i] for i in rng.integers(0, 4, int(rng.integers(2, 5)))) * int(rng.integers(2, 7))
        else:
            s = "".join(bases[i] for i in rng.integers(0, 4, int(rng.integers(4, 20))))
        parts.append(s)
        size += len(s)
    return "".join(parts)[:n]


def random_read(ref, ref_offset, pos, read_len, rng):
    """one read of read_len bases from `pos`: matches with 3 % substitutions (a fifth of them N), now and then a dense tail, indels (often
    copies of the neighbouring reference, so that normalisation has something to shift), swaps, clips, edge indels"""
    bases = "ACGT"
    path, seq, p = [], [], pos
    left = read_len
    if rng.random() < 0.15:
        path.append((HC, int(rng.integers(1, 9))))
    if rng.random() < 0.2 and left > 20:
        k = int(rng.integers(1, 12))
        path.append((SC, k))
        seq += [bases[i] for i in rng.integers(0, 4, k)]
        left -= k
    tail = int(rng.integers(0, 10)) if rng.random() < 0.2 and left > 30 else 0
    left -= tail
    dense = rng.random() < 0.15
    n_ev = int(rng.integers(0, 4))
    for e in range(n_ev + 1):
        m = left if e == n_ev else int(rng.integers(1, max(2, left - 12 * (n_ev - e))))
        m = max(1, min(m, left))
        for j in range(m):
            b = M.ref_char(ref, ref_offset, p + j)
            rate = 0.5 if dense and len(seq) >= read_len - 15 else 0.03
            if rng.random() < rate:
                b = bases[int(rng.integers(0, 4))] if rng.random() < 0.8 else "N"
            seq.append(b)
        path.append((MS, m))
        p += m
        left -= m
        if e == n_ev or left <= 0:
            break
        r = rng.random()
        if r < 0.4:
            k = int(rng.integers(1, 9)) if rng.random() < 0.9 else int(rng.integers(45, 60))
            path.append((DE, k))
            p += k
        elif r < 0.8:
            k = min(left - 1, int(rng.integers(1, 9)) if rng.random() < 0.9 else int(rng.integers(11, 60)))
            if k < 1:
                break
            q = rng.random()
            ins = [M.ref_char(ref, ref_offset, p + j) for j in range(k)] if q < 0.4 else [bases[i] for i in rng.integers(0, 4, k)]
            ins = [b if b != "N" else "A" for b in ins]
            path.append((IN, k))
            seq += ins
            left -= k
        else:
            ki, kd = min(left - 1, int(rng.integers(1, 7))), int(rng.integers(1, 7))
            if ki < 1:
                break
            path += [(IN, ki), (DE, kd)] if rng.random() < 0.5 else [(DE, kd), (IN, ki)]
            seq += [bases[i] for i in rng.integers(0, 4, ki)]
            p += kd
            left -= ki
    if left > 0:  # (an event list cut short)
        t, l = path[-1]
        if M.is_match(t):
            path[-1] = (t, l + left)
        else:
            path.append((MS, left))
        seq += [M.ref_char(ref, ref_offset, p + j) for j in range(left)]
        p += left
    if tail:
        path.append((SC, tail))
        seq += [bases[i] for i in rng.integers(0, 4, tail)]
    if rng.random() < 0.1:
        path.append((HC, int(rng.integers(1, 9))))
    return dict(code=M.encode("".join(seq)), pos=pos, path=path)


def random_batch(n_reads, read_len, ref_len, seed, ref_offset=1000):
    """-> (ref, ref_offset, reads sorted by position, low_mapq): reads start up to 40 positions before the segment and run past its end"""
    rng = np.random.default_rng(seed)
    ref = repeat_rich_reference(ref_len, rng)
    starts = np.sort(rng.integers(ref_offset - 40, ref_offset + ref_len - read_len // 2, n_reads))
    reads = [random_read(ref, ref_offset, int(s), read_len, rng) for s in starts]
    low = [int(x) for x in rng.random(n_reads) < 0.08]
    return ref, ref_offset, reads, low


def usable(reads, low):
    """drop what the reference throws on (normalisation can leave such a path: two deletions side by side stay two segments when
    nothing else changed) -> (reads, low)"""
    keep_r, keep_l = [], []
    for r, l in zip(reads, low):
        try:
            M.check_path([(int(t), int(n)) for t, n in r["path"]], len(r["code"]))
        except M.PathError:
            continue
        keep_r.append(r)
        keep_l.append(l)
    return keep_r, keep_l
