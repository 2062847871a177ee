"""Inputs of the region-haplotype tests, shared by the model tests (tests/test_region_haplotypes_model.py) and the device tests
(tests/test_region_haplotypes.py): the recorded reference vectors, small builders of crafted reads, and the seeded window.  Imports
neither the product nor a device."""
import bisect
import functools
import json
import os

import numpy as np

from tests import anchor_model as A
from tests import haplotype_model as H
from tests import intake_model as M

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "region_haplotypes", "region_haplotypes_golden.json")
MS, IN, DE, SC, HC = M.MATCH, M.INSERT, M.DELETE, M.SOFT_CLIP, M.HARD_CLIP

REF_OFFSET = 100
_rng = np.random.default_rng(4242)
REF = "".join(_rng.choice(list("ACGT"), 400))  # 100..499


@functools.lru_cache(maxsize=None)
def golden():
    """-> [dict(name, ref, ref_offset, reads, low, fwd, max_indel_size, buf_begin, buf_end, regions [recorded dicts])]"""
    with open(GOLDEN) as f:
        doc = json.load(f)
    out = []
    for sc in doc["scenes"]:
        reads = [dict(code=M.encode(r["seq"]), pos=r["pos"], path=[tuple(s) for s in r["path"]]) for r in sc["reads"]]
        out.append(dict(name=sc["name"], ref=sc["ref"], ref_offset=sc["ref_offset"], reads=reads, low=[r["low_mapq"] for r in sc["reads"]],
                        fwd=[r["is_fwd"] for r in sc["reads"]], max_indel_size=sc["max_indel_size"], buf_begin=sc["buf_begin"], buf_end=sc["buf_end"],
                        regions=sc["regions"]))
    return out


def other(base):
    return {"A": "C", "C": "G", "G": "T", "T": "A", "N": "A"}[base]


def read(pos, path, subs=None, ins=None, ref=REF, ref_offset=REF_OFFSET):
    """a read following `ref` along `path` from `pos`; subs: {reference position: character (None: another base)}; ins: inserted strings"""
    subs = subs or {}
    ins = list(ins or [])
    seq, p = [], pos
    for t, l in path:
        if M.is_match(t):
            for j in range(l):
                b = M.ref_char(ref, ref_offset, p + j)
                if p + j in subs:
                    b = other(b) if subs[p + j] is None else subs[p + j]
                seq.append(b)
            p += l
        elif t == IN:
            seq.append(ins.pop(0) if ins else "T" * l)
        elif t == SC:
            seq.append("T" * l)
        elif t == DE:
            p += l
    return dict(code=M.encode("".join(seq)), pos=pos, path=list(path))


def plain(n, subs=None, pos=180, length=60, ref=REF, ref_offset=REF_OFFSET):
    return [read(pos, [(MS, length)], subs=subs, ref=ref, ref_offset=ref_offset) for _ in range(n)]


def case(reads, regions, low=None, fwd=None, buf=(REF_OFFSET, REF_OFFSET + len(REF)), ploidy=2, ref=REF, ref_offset=REF_OFFSET, max_indel_size=M.MAX_INDEL_SIZE):
    n = len(reads)
    return dict(ref=ref, ref_offset=ref_offset, reads=reads, low=low or [0] * n, fwd=fwd if fwd is not None else [i % 2 for i in range(n)],
                regions=[(int(b), int(e)) for b, e in regions], buf_begin=buf[0], buf_end=buf[1], ploidy=ploidy, max_indel_size=max_indel_size)


def model(c):
    return H.region_haplotypes(c["ref"], c["ref_offset"], c["reads"], c["low"], c["fwd"], c["regions"], c["buf_begin"], c["buf_end"], c["ploidy"],
                               c["max_indel_size"])


def groups_case(n_groups, per_group=3, region=(200, 210)):
    """n_groups distinct haplotypes of per_group reads each over `region`: group g differs from the reference at the positions its bits name"""
    reads = []
    for g in range(n_groups):
        subs = {region[0] + 1 + k: None for k in range(6) if (g + 1) >> k & 1}
        reads += plain(per_group, subs=subs)
    return case(reads, [region])


def spread_case(spread, region=(200, 210)):
    """three reads over the region at index 0 and three at index `spread` and before, with reads that lie elsewhere in between"""
    far = read(300, [(MS, 40)])
    reads = plain(3) + [far] * (spread - 5) + plain(3, subs={204: None})
    assert len(reads) == spread + 1
    return case(reads, [region])


@functools.lru_cache(maxsize=None)
def seeded_window(n_reads=2200, seed=9100):
    """a window of about n_reads reads of 100 bases at depth ~40 over a random reference carrying heterozygous variants every ~90
    positions (substitutions, short insertions and deletions, on about half the reads that cross them), sparse sequencing errors, a few
    soft clips and low-MAPQ reads -> a case without regions (they come from the intake -> anchors -> walk chain) with win_begin, n_pos"""
    rng = np.random.default_rng(seed)
    read_len = 100
    span = n_reads * read_len // 40
    ref_offset = 1000
    ref = "".join(rng.choice(list("ACGT"), span + 400))
    # the sample's second haplotype: variants as (position, kind, payload)
    variants = []
    p = ref_offset + 150
    while p < ref_offset + span + 100:
        kind = rng.choice(["snv2", "snv2", "ins", "del"])
        if kind == "snv2":
            variants.append((p, "snv", other(ref[p - ref_offset])))
            variants.append((p + 3, "snv", other(ref[p + 3 - ref_offset])))
        elif kind == "ins":
            variants.append((p, "ins", "".join(rng.choice(list("ACGT"), int(rng.integers(1, 5))))))
            variants.append((p + 4, "snv", other(ref[p + 4 - ref_offset])))
        else:
            variants.append((p, "del", int(rng.integers(1, 5))))
            variants.append((p + 7, "snv", other(ref[p + 7 - ref_offset])))
        p += int(rng.integers(70, 110))
    snv_at = {v[0]: v[2] for v in variants if v[1] == "snv"}
    indels = [v for v in variants if v[1] != "snv"]
    indel_pos = [v[0] for v in indels]
    starts = np.sort(rng.integers(ref_offset + 20, ref_offset + span, n_reads))
    reads, low, fwd = [], [], []
    for s in starts:
        s = int(s)
        alt = rng.random() < 0.5
        path, seq, at, left = [], [], s, read_len
        clip = int(rng.integers(2, 8)) if rng.random() < 0.03 else 0
        if clip:
            path.append((SC, clip))
            seq.append("".join(rng.choice(list("ACGT"), clip)))
            left -= clip

        def match(upto):
            nonlocal at, left
            n = min(upto - at, left)
            if n <= 0:
                return
            bases = list(ref[at - ref_offset:at - ref_offset + n])
            for k in range(n):
                if alt and (at + k) in snv_at:
                    bases[k] = snv_at[at + k]
                elif rng.random() < 0.002:
                    bases[k] = other(bases[k])
            if path and path[-1][0] == MS:
                path[-1] = (MS, path[-1][1] + n)
            else:
                path.append((MS, n))
            seq.append("".join(bases))
            at += n
            left -= n

        for vp, kind, payload in indels[bisect.bisect_right(indel_pos, at + 5):] if alt else ():
            if vp <= at + 5 or left <= 0:
                continue
            if vp >= at + left - 8:
                break
            match(vp)
            if kind == "ins":
                path.append((IN, len(payload)))
                seq.append(payload)
                left -= len(payload)
            else:
                path.append((DE, payload))
                at += payload
        match(at + left)
        reads.append(dict(code=M.encode("".join(seq)), pos=s, path=path))
        low.append(int(rng.random() < 0.02))
        fwd.append(int(rng.random() < 0.5))
    win_begin = ref_offset
    n_pos = span + 300
    c = case(reads, [], low=low, fwd=fwd, buf=(win_begin, win_begin + n_pos), ref=ref, ref_offset=ref_offset)
    c.update(win_begin=win_begin, n_pos=n_pos)
    return c


@functools.lru_cache(maxsize=None)
def seeded_window_model():
    """the model of the whole chain on the seeded window -> (case with its regions filled in, intake, anchors, regions, records)"""
    c = dict(seeded_window())
    intake = M.read_intake(c["ref"], c["ref_offset"], c["reads"], c["low"], c["win_begin"], c["n_pos"], c["max_indel_size"])
    anchor, _ = A.ref_anchors(c["ref"], c["ref_offset"], c["win_begin"] + 1, None, c["win_begin"], c["n_pos"])
    regions, state = A.active_regions(c["win_begin"], [d for _, d in intake["sites"]], intake["is_candidate"], anchor)
    c["regions"] = [(b, e) for b, e, _ in regions]
    return c, intake, anchor, regions, model(c)
