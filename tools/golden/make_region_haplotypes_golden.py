"""Record tests/golden/region_haplotypes/region_haplotypes_golden.json from the reference's own read buffer and haplotype selection.

  python tools/golden/make_region_haplotypes_golden.py <path of the built tools/golden/region_haplotypes_driver>

A list of small scenes, each a driver run of its own (fewer than 1 000 reads, every position inside [0, 1000): the reference's store
never aliases).  Every region is recorded at ploidy 1 and 2.  Needed only to make the file again; the tests read the file."""
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


def mk(ref, pos, path, subs=None, ins=None, clip="T", low=0, fwd=1):
    """a read following `ref` along `path` from `pos`; subs: {reference position: character}; ins: the inserted strings, in path order"""
    subs = subs or {}
    ins = list(ins or [])
    seq, p = [], pos
    for t, l in path:
        if t == M:
            for j in range(l):
                q = p + j
                b = ref[q - REF_OFFSET] if REF_OFFSET <= q < REF_OFFSET + len(ref) else "N"
                seq.append(subs.get(q, b))
            p += l
        elif t == I:
            s = ins.pop(0) if ins else "T" * l
            assert len(s) == l
            seq.append(s)
        elif t == S:
            seq.append(clip * l)
        elif t == D:
            p += l
    return (pos, low, fwd, "".join(seq), list(path))


def plain(ref, n, subs=None, fwd=None, pos=180, length=60):
    """n reads of one match segment; fwd: a list of strands, or None for alternating"""
    return [mk(ref, pos, [(M, length)], subs=subs, fwd=(i % 2 if fwd is None else fwd[i % len(fwd)])) for i in range(n)]


def scene_kinds():
    ref = make_ref(11)
    r = []
    r += plain(ref, 6)
    r += plain(ref, 4, subs={205: other(ref[105])})
    r.append(mk(ref, 206, [(S, 5), (M, 40)]))                       # leading soft clip at 205, inside the region
    r.append(mk(ref, 170, [(M, 35), (S, 4)]))                       # trailing soft clip at 205
    r.append(mk(ref, 180, [(M, 60)], subs={203: "N"}))             # an N base
    r.append(mk(ref, 180, [(M, 60)], subs={204: "="}))             # '=' is a character of its own
    r.append(mk(ref, 180, [(M, 60)], subs={205: other(ref[105])}, low=1))  # low MAPQ: registers nothing
    r.append(mk(ref, 180, [(M, 22), (I, 2), (D, 3), (M, 30)], ins=["GG"]))  # a swap: 202..204 a hole
    r.append(mk(ref, 140, [(M, 62), (D, 50), (M, 20)]))             # above max_indel_size: 202..251 a hole
    r.append(mk(ref, 204, [(M, 40)]))                               # begins inside the region
    r.append(mk(ref, 150, [(M, 55)]))                               # ends inside the region
    r.append(mk(ref, 180, [(H, 3), (M, 60), (H, 2)]))
    r.append(mk(ref, 190, [(I, 2), (M, 40)]))                       # an edge insert
    r.append(mk(ref, 96, [(M, 30)]))                                # hangs off the reference segment's start: N there
    # ... of 1 and 2 positions, inside both holes, 250 and 251 long, cut by the buffer's range at either end, where no read lies
    regions = [(200, 212), (210, 220), (205, 206), (180, 182), (202, 205), (120, 370), (120, 371), (98, 104), (100, 104), (395, 401), (330, 340)]
    return dict(name="kinds", ref=ref, buf=(100, 400), max_indel_size=49, reads=r, regions=regions)


def scene_indels():
    ref = make_ref(12)
    r = []
    r += [mk(ref, 180, [(M, 28), (D, 2), (M, 30)], fwd=i % 2) for i in range(5)]      # a deletion at the region's last two positions
    r += [mk(ref, 180, [(M, 29), (D, 3), (M, 30)], fwd=i % 2) for i in range(3)]      # ... beginning at its last position and running past it
    r += [mk(ref, 180, [(M, 25), (I, 3), (M, 30)], subs={204: other(ref[104])}, ins=["ACA"], fwd=i % 2) for i in range(4)]  # an insertion over a mismatch
    r += [mk(ref, 180, [(M, 25), (I, 3), (M, 30)], ins=["ACA"], fwd=i % 2) for i in range(4)]                             # the same insertion on a match
    r += [mk(ref, 180, [(M, 20), (I, 2), (M, 35)], ins=["GT"], fwd=i % 2) for i in range(4)]                              # an insertion at begin - 1
    r += [mk(ref, 180, [(M, 25), (I, 2), (M, 30)], ins=["NA"], fwd=1) for i in range(3)]                                  # an N in the insert
    r += plain(ref, 3)
    r.append(mk(ref, 180, [(M, 24), (D, 1), (I, 1), (M, 30)], ins=["C"]))  # a swap, deletion first
    r.append(mk(ref, 180, [(M, 24), (D, 60), (M, 10)]))
    r.append(mk(ref, 180, [(M, 24), (I, 50), (M, 10)], ins=["AC" * 25]))   # an insertion above max_indel_size: nothing at 203
    regions = [(200, 210), (199, 210), (208, 210), (204, 205), (203, 206), (200, 205)]
    return dict(name="indels", ref=ref, buf=(100, 400), max_indel_size=49, reads=r, regions=regions)


def scene_ties(name, counts, with_ref=True, region=(200, 208)):
    """counts: [(count, {reference position: base} or path)]"""
    ref = make_ref(13)
    r = []
    for n, what in counts:
        if isinstance(what, dict):
            subs = {p: (other(ref[p - REF_OFFSET]) if b is None else b) for p, b in what.items()}
            r += plain(ref, n, subs=subs)
        else:
            r += [mk(ref, 180, what, fwd=i % 2) for i in range(n)]
    order = np.random.default_rng(len(name)).permutation(len(r))
    r = [r[i] for i in order]
    return dict(name=name, ref=ref, buf=(100, 400), max_indel_size=49, reads=r, regions=[region])


def scene_phasing(name, run, direction, strands, region):
    """a homopolymer of `run` A's at 201.., T before it and C after it; the second haplotype turns the T (direction 'right': the run lies to
    the right of the changed base) or the C ('left') into A, on the given strands"""
    ref = make_ref(14)
    ref = "".join(c if c != "A" else "G" for c in ref[:100]) + "T" + "A" * run + "C" + "GTCGTCCGTG" + ref[112 + run:]
    ref = ref[:300]
    at = 200 if direction == "right" else 201 + run
    r = plain(ref, 12)
    r += plain(ref, len(strands), subs={at: "A"}, fwd=strands)
    return dict(name=name, ref=ref, buf=(100, 400), max_indel_size=49, reads=r, regions=[region])


def scene_coverage(name, covering, total):
    ref = make_ref(15)
    r = plain(ref, covering, length=40)
    r += [mk(ref, 204, [(M, 30)], fwd=i % 2) for i in range(total - covering)]  # registered in the region, not at its first position
    return dict(name=name, ref=ref, buf=(100, 400), max_indel_size=49, reads=r, regions=[(200, 210)])


def scenes():
    out = [scene_kinds(), scene_indels()]
    a, b, c = {202: None}, {204: None}, {206: None}
    out.append(scene_ties("tie_15ref_12_12", [(15, {}), (12, a), (12, b)]))
    out.append(scene_ties("tie_15ref_12_12_12", [(15, {}), (12, a), (12, b), (12, c)]))
    out.append(scene_ties("tie_15alt_12_12", [(15, c), (12, a), (12, b), (2, {})]))
    out.append(scene_ties("tie_15alt_12ref_12", [(15, c), (12, {}), (12, a)]))
    out.append(scene_ties("top_not_reference", [(15, c), (10, {}), (4, a)]))
    out.append(scene_ties("below_min_count", [(2, {}), (2, a), (1, b)]))
    # equal counts, one string a prefix of the other: a deletion of the region's last position against the reference
    out.append(scene_ties("tie_lengths_prefix", [(8, {}), (8, [(M, 27), (D, 1), (M, 30)])]))
    out.append(scene_ties("tie_lengths_insert", [(9, {}), (7, [(M, 24), (I, 2), (M, 30)]), (7, a), (7, [(M, 23), (D, 2), (M, 30)])]))
    for run, tag in ((10, "run11"), (9, "run10")):
        out.append(scene_phasing("phasing_right_%s_reverse_only" % tag, run, "right", [0, 0, 0, 0, 0], (199, 214)))
        out.append(scene_phasing("phasing_left_%s_forward_only" % tag, run, "left", [1, 1, 1, 1], (199, 214)))
    out.append(scene_phasing("phasing_right_run11_mixed_strands", 10, "right", [0, 0, 1, 0], (199, 214)))
    out.append(scene_phasing("phasing_right_run11_forward_only", 10, "right", [1, 1, 1, 1], (199, 214)))  # the walk goes left: a run of one
    out.append(scene_phasing("phasing_left_run11_reverse_only", 10, "left", [0, 0, 0], (199, 214)))       # the walk goes right: a run of one
    out.append(scene_phasing("phasing_left_stops_at_the_strings_start", 10, "left", [1, 1, 1, 1], (201, 214)))  # 10 counted of a run of 11
    out.append(scene_phasing("phasing_left_run12_from_the_strings_start", 11, "left", [1, 1, 1, 1], (201, 215)))
    out.append(scene_coverage("coverage_13_of_20", 13, 20))
    out.append(scene_coverage("coverage_12_of_20", 12, 20))
    out.append(scene_coverage("coverage_65_of_100", 65, 100))
    out.append(scene_coverage("coverage_64_of_100", 64, 100))
    return out


def run_scene(driver, sc, extra=()):
    lines = ["REF %d %s" % (REF_OFFSET, sc["ref"]), "OPT %d" % sc["max_indel_size"], "BUF %d %d" % sc["buf"]]
    for pos, low, fwd, seq, path in sc["reads"]:
        lines.append("READ %d %d %d %s %d %s" % (pos, low, fwd, seq, len(path), " ".join("%d %d" % s for s in path)))
    for b, e in sc["regions"]:
        for ploidy in (1, 2):
            lines.append("REGION %d %d %d" % (b, e, ploidy))
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
    dst = os.path.join(root, "tests", "golden", "region_haplotypes", "region_haplotypes_golden.json")
    os.makedirs(os.path.dirname(dst), exist_ok=True)
    with open(dst, "w") as f:
        json.dump(dict(scenes=docs), f, separators=(",", ":"))
        f.write("\n")
    print("%s: %d scenes, %d reads, %d regions, %d bytes" % (dst, len(docs), sum(len(d["reads"]) for d in docs), sum(len(d["regions"]) for d in docs),
                                                           os.path.getsize(dst)))
    for d in docs:
        print("  %-45s %s" % (d["name"], " | ".join("%d/%d:%s" % (len(g["segments"]), g["n_reads_aligned"], ",".join(str(len(s["support"])) for s in g["selected"]) or "-")
                                                    for g in d["regions"])))


if __name__ == "__main__":
    main()
