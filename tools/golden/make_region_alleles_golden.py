"""Record tests/golden/region_alleles/region_alleles_golden.json from the reference's own processSelectedHaplotypes.

  python tools/golden/make_region_alleles_golden.py <path of the built tools/golden/region_alleles_driver>

A list of small scenes, each a driver run of its own (fewer than 1 000 reads, every position inside [0, 1000): the reference's store
never aliases).  Every region is recorded at ploidy 1 and 2, with the _prevActiveRegionEnd the scene names, into an IndelBuffer and a
CandidateSnvBuffer of its own.  The scenes are built so that the reference alone meets every rule tests/test_region_alleles_model.py
counts (tests.alleles_model.rule_counts, printed at the end).  Needed only to make the file again; the tests read the file."""
import json
import os
import subprocess
import sys

import numpy as np

M, I, D, S, H = 1, 2, 3, 5, 6
REF_OFFSET = 100


def other(b):
    return {"A": "C", "C": "G", "G": "T", "T": "A"}[b]


def make_ref(seed, n=300):
    rng = np.random.default_rng(seed)
    return "".join(rng.choice(list("ACGT"), n))


def patch(ref, at, s):
    """the reference with s at the positions at .. at + len(s)"""
    k = at - REF_OFFSET
    return ref[:k] + s + ref[k + len(s):]


def mk(ref, pos, path, subs=None, ins=None, low=0, fwd=1):
    """a read following `ref` along `path` from `pos`; subs: {reference position: character (None: another base)}; ins: the inserted strings"""
    subs = subs or {}
    ins = list(ins or [])
    seq, p = [], pos
    for t, l in path:
        if t == M:
            for j in range(l):
                q = p + j
                b = ref[q - REF_OFFSET] if REF_OFFSET <= q < REF_OFFSET + len(ref) else "N"
                seq.append((other(b) if subs[q] is None else subs[q]) if q in subs else b)
            p += l
        elif t == I:
            s = ins.pop(0)
            assert len(s) == l
            seq.append(s)
        elif t == D:
            p += l
    return (pos, low, fwd, "".join(seq), list(path))


def scene(name, ref, groups, regions, pos=180, length=60, max_indel_size=49):
    """groups: [(count, path or None for one match segment, subs, ins)]; regions: [(begin, end, prev_end)]"""
    reads = []
    for count, path, subs, ins in groups:
        reads += [mk(ref, pos, path or [(M, length)], subs=subs, ins=ins, fwd=i % 2) for i in range(count)]
    order = np.random.default_rng(len(name)).permutation(len(reads))
    return dict(name=name, ref=ref, buf=(100, 400), max_indel_size=max_indel_size, reads=[reads[i] for i in order], regions=regions)


def scenes():
    out = []
    ref = make_ref(21)
    a, b = {203: None}, {206: None}
    whole = [(200, 210, -1)]
    out.append(scene("one_alternate", ref, [(10, None, {}, None), (6, None, a, None)], whole))
    out.append(scene("two_alternates_and_the_reference", ref, [(15, None, {}, None), (12, None, a, None), (12, None, b, None)], whole))
    out.append(scene("top_not_reference", ref, [(15, None, a, None), (10, None, {}, None)], whole))
    out.append(scene("only_reference", ref, [(10, None, {}, None), (2, None, a, None)], whole))
    # the same deletion in both alternates, the second with a SNV of its own: haplotypeId 1 + 2, two ratios added; then with 4 and 3 of 7 reads
    ref = patch(make_ref(22), 202, "CAGTC")
    dele = [(M, 24), (D, 2), (M, 34)]
    out.append(scene("same_deletion_in_both", ref, [(10, dele, {}, None), (8, dele, {208: None}, None)], whole))
    out.append(scene("same_deletion_in_both_4_and_3_of_7", ref, [(4, dele, {}, None), (3, dele, {208: None}, None)], whole))
    ref = make_ref(23)
    x = ref[204 - REF_OFFSET]
    out.append(scene("same_position_different_bases", ref, [(10, None, {204: other(x)}, None), (8, None, {204: other(other(x))}, None)], whole))
    # 10 distinct mismatches with a deletion (they go to the indel buffer), 11 over two alternates (they do not)
    ref = patch(make_ref(24), 230, "CAGTC")
    long_del = [(M, 52), (D, 1), (M, 27)]
    ten = {201 + 3 * k: None for k in range(10)}
    out.append(scene("ten_mismatches_and_a_deletion", ref, [(12, None, {}, None), (10, long_del, ten, None)], [(200, 240, -1)], length=80))
    six, five = {201 + 3 * k: None for k in range(6)}, {219 + 2 * k: None for k in range(5)}
    out.append(scene("eleven_mismatches_and_a_deletion", ref, [(10, long_del, six, None), (8, None, five, None)], [(200, 240, -1)], length=80))
    # a run of ten A at 195..204: an indel in it is shifted left of the region's begin, to exactly prev_end and to one below it
    ref = patch(make_ref(25), 194, "C" + "A" * 10 + "GTC")
    shifted = [(200, 210, -1), (200, 210, 195), (200, 210, 196)]
    out.append(scene("deletion_shifted_to_prev_end", ref, [(10, None, {}, None), (8, [(M, 24), (D, 1), (M, 35)], {}, None)], shifted))
    out.append(scene("insertion_shifted_to_prev_end", ref, [(10, None, {}, None), (8, [(M, 25), (I, 1), (M, 35)], {}, ["A"])], shifted))
    # a run of five T from the region's first position: the aligner puts an inserted T before all of them, the path begins with the insertion
    ref = patch(make_ref(30), 199, "G" + "T" * 5 + "CA")
    out.append(scene("insertion_at_the_first_position", ref, [(10, None, {}, None), (8, [(M, 23), (I, 1), (M, 37)], {}, ["T"])], whole))
    # at the region's last position and at its end
    ref = patch(make_ref(26), 207, "GCAGT")
    out.append(scene("insertion_at_the_end", ref, [(10, None, {}, None), (8, [(M, 30), (I, 2), (M, 30)], {}, ["GT"])], [(200, 210, -1), (200, 211, -1)]))
    out.append(scene("deletion_of_the_last_position", ref, [(10, None, {}, None), (8, [(M, 29), (D, 1), (M, 30)], {}, None)], whole))
    # a run of six A at the reference segment's start: shifted to 100, next to the N before the segment
    ref = patch(make_ref(27), 100, "A" * 6 + "CGT")
    at_start = [(102, 110, -1)]
    out.append(scene("deletion_next_to_n", ref, [(10, None, {}, None), (8, [(M, 4), (D, 1), (M, 55)], {}, None)], at_start, pos=100))
    out.append(scene("insertion_next_to_n", ref, [(10, None, {}, None), (8, [(M, 5), (I, 1), (M, 55)], {}, ["A"])], at_start, pos=100))
    # max_indel_size 5: two deletions of a read in a run of twelve A become one of 5 (kept) or of 6 (dropped) for the aligner
    ref = patch(make_ref(28), 204, "C" + "A" * 12 + "GTC")
    for n2, name in ((2, "deletion_of_max_indel_size"), (3, "deletion_above_max_indel_size")):
        out.append(scene(name, ref, [(10, None, {}, None), (8, [(M, 25), (D, 3), (M, 2), (D, n2), (M, 30)], {}, None)], [(200, 225, -1)], length=70, max_indel_size=5))
    # two regions sharing the base 205, the SNV in it: the second region leaves it to the first
    ref = make_ref(29)
    out.append(scene("snv_in_a_shared_base", ref, [(12, None, {}, None), (10, None, {205: None, 209: None}, None)], [(200, 206, -1), (205, 212, 206)]))
    return out


def run_scene(driver, sc, extra=()):
    lines = ["REF %d %s" % (REF_OFFSET, sc["ref"]), "OPT %d" % sc["max_indel_size"], "BUF %d %d" % sc["buf"]]
    for pos, low, fwd, seq, path in sc["reads"]:
        lines.append("READ %d %d %d %s %d %s" % (pos, low, fwd, seq, len(path), " ".join("%d %d" % s for s in path)))
    for b, e, prev_end in sc["regions"]:
        for ploidy in (1, 2):
            lines.append("REGION %d %d %d %d" % (b, e, ploidy, prev_end))
    lines += list(extra)
    out = subprocess.run([driver], input="\n".join(lines) + "\n", stdout=subprocess.PIPE, check=True, universal_newlines=True).stdout
    return json.loads(out)


def main():
    driver = sys.argv[1]
    docs = []
    for sc in scenes():
        assert len(sc["reads"]) < 1000
        doc = run_scene(driver, sc)
        assert len(doc["reads"]) == len(sc["reads"]) and len(doc["regions"]) == 2 * len(sc["regions"])
        doc["name"] = sc["name"]
        docs.append(doc)
    root = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    dst = os.path.join(root, "tests", "golden", "region_alleles", "region_alleles_golden.json")
    os.makedirs(os.path.dirname(dst), exist_ok=True)
    with open(dst, "w") as f:
        json.dump(dict(scenes=docs), f, separators=(",", ":"))
        f.write("\n")
    print("%s: %d scenes, %d reads, %d regions, %d bytes" % (dst, len(docs), sum(len(d["reads"]) for d in docs), sum(len(d["regions"]) for d in docs),
                                                           os.path.getsize(dst)))
    for d in docs:
        print("  %-40s %s" % (d["name"], " | ".join("%s:%dk,%ds" % (",".join(str(len(s["support"])) for s in g["selected"]) or "-", len(g["keys"]), len(g["snvs"]))
                                                    for g in d["regions"])))
    sys.path.insert(0, root)
    from tests import alleles_model
    alleles_model.golden.cache_clear()
    for rule, n in alleles_model.rule_counts(alleles_model.golden()).items():
        print("  %-40s %d%s" % (rule, n, "" if n else "   <-- not covered"))


if __name__ == "__main__":
    main()
