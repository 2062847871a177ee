"""Record tests/golden/indel_table/indel_table_golden.json from the reference's own IndelBuffer.

  python tools/golden/make_indel_table_golden.py <path of the built tools/golden/indel_buffer_driver>

A list of small scenes, each a driver run of its own (fewer than 1 000 reads per sample, every position inside [0, 1000): the reference's
store never aliases).  A scene is the input of one sk_indel_table call: S samples' reads with their align ids and INDEL_ALIGN_TYPE, the
shared region list, prev_end_in.  The driver adds every read, then closes the regions in order, sample by sample, then writes the map out.
The first scenes are those of tools/golden/make_region_alleles_golden.py, one region each.  No scene may reach the assembler
("assembled" must be 0): the script refuses one that does.  Needed only to make the file again; the tests read the file.  At the end the
model is run on every scene, compared, and the rule counts (tests.indel_table_model.rule_counts) printed."""
import json
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_region_alleles_golden as RA  # noqa: E402

M, I, D, S, H = RA.M, RA.I, RA.D, RA.S, RA.H
REF_OFFSET = RA.REF_OFFSET
mk, patch, make_ref, other = RA.mk, RA.patch, RA.make_ref, RA.other


def sample(groups, ref, buf=(100, 400), pos=180, length=60, iat=None, id_base=0, id_step=1):
    """groups: [(count, path or None for one match segment, subs, ins[, pos])] -> dict(buf, reads [(id, iat, pos, low, fwd, seq, path)]); iat: a function of
    the read's index (None: tier 1)"""
    reads = []
    for g in groups:
        count, path, subs, ins = g[:4]
        p = g[4] if len(g) > 4 else pos
        for i in range(count):
            reads.append(mk(ref, p, path or [(M, length)], subs=subs, ins=ins, fwd=i % 2))
    order = sorted(range(len(reads)), key=lambda i: (reads[i][0], (i * 7919) % 101))  # by position, the groups interleaved
    out = []
    for k, i in enumerate(order):
        pos_, low, fwd, seq, path = reads[i]
        out.append((id_base + id_step * k, iat(k) if iat else 0, pos_, low, fwd, seq, path))
    return dict(buf=buf, reads=out)


def scenes():
    out = []
    for sc in RA.scenes():  # the region_alleles scenes pushed through, a region at a time
        for k, (b, e, prev_end) in enumerate(sc["regions"]):
            reads = [(i, 0, r[0], r[1], r[2], r[3], r[4]) for i, r in enumerate(sc["reads"])]
            out.append(dict(name="%s_%d" % (sc["name"], k), ref=sc["ref"], max_indel_size=sc["max_indel_size"], samples=[dict(buf=sc["buf"], reads=reads)],
                            regions=[(b, e)], prev_end_in=prev_end, ploidy=[2]))
    # the three alignment types and noise: a deletion in the body of the read, and one in a tail of mismatches (outside the valid range)
    ref = patch(make_ref(41), 200, "GCATCAGT")
    body = [(M, 24), (D, 2), (M, 34)]
    tail = [(M, 50), (D, 1), (M, 7)]
    tail_subs = {232: None, 234: None, 236: None, 237: None}
    out.append(dict(name="tiers_and_noise", ref=ref, max_indel_size=49, regions=[(200, 210)], prev_end_in=-1, ploidy=[2, 2],
                    samples=[sample([(9, None, {}, None), (9, body, {}, None), (4, tail, tail_subs, None)], ref, iat=lambda k: k % 3, id_base=5, id_step=3),
                             sample([(6, None, {}, None), (6, body, {}, None)], ref, iat=lambda k: (k + 1) % 3, id_base=300)]))
    # breakpoints: insertions above max_indel_size 5 with different sequences at one position; a swap; inserts that differ in the last base, an N
    # against a T and a G, (insert 1, delete 2) against (insert 2, delete 1); a MISMATCH key at the same position comes from the region
    ref = patch(make_ref(42), 198, "GCATGCAGTCA")
    groups = [(8, None, {}, None),
              (3, [(M, 24), (I, 7), (M, 36)], {}, ["ACGTACG"]), (3, [(M, 24), (I, 7), (M, 36)], {}, ["TTGTACG"]),
              (3, [(M, 24), (I, 2), (M, 36)], {}, ["CG"]), (3, [(M, 24), (I, 2), (M, 36)], {}, ["CT"]), (3, [(M, 24), (I, 2), (M, 36)], {}, ["CN"]),
              (3, [(M, 24), (I, 1), (D, 2), (M, 34)], {}, ["T"]), (3, [(M, 24), (I, 2), (D, 1), (M, 35)], {}, ["AT"]),
              (3, [(M, 24), (D, 3), (M, 33)], {}, None)]
    out.append(dict(name="key_order_at_one_position", ref=ref, max_indel_size=5, regions=[(198, 212)], prev_end_in=-1, ploidy=[2],
                    samples=[sample(groups, ref, buf=(100, 190))]))  # (the region lies outside the read buffer: bypassed, the keys are the reads')
    # report info: a homopolymer from the segment's first base, an STR deletion with repeats on both sides, an insertion whose unit is the whole
    # insert, one that repeats, a homopolymer running to ref.end(), interrupted homopolymers
    ref = make_ref(43, 300)
    ref = patch(ref, 100, "A" * 7 + "CG")
    ref = patch(ref, 150, "GCACACACACACAGT")
    ref = patch(ref, 200, "GTTTTCTTTTG")
    ref = patch(ref, 250, "CAGCAGCAGT")
    ref = ref[:290] + "C" + "G" * 9
    groups = [(6, [(M, 3), (D, 1), (M, 50)], {}, None, 100), (6, [(M, 6), (I, 2), (M, 50)], {}, ["AA"], 100),
              (6, [(M, 24), (D, 4), (M, 30)], {}, None, 130), (6, [(M, 24), (I, 3), (M, 30)], {}, ["TGA"], 130),
              (6, [(M, 25), (D, 1), (M, 30)], {}, None, 180), (6, [(M, 24), (I, 1), (M, 30)], {}, ["C"], 182),
              (6, [(M, 23), (I, 6), (M, 30)], {}, ["CAGCAG"], 230), (6, [(M, 20), (D, 3), (M, 30)], {}, None, 233),
              (6, [(M, 44), (D, 2), (M, 4)], {}, None, 350), (6, [(M, 46), (I, 2), (M, 4)], {}, ["GG"], 350)]
    out.append(dict(name="report_info", ref=ref, max_indel_size=49, regions=[], prev_end_in=-1, ploidy=[2], samples=[sample(groups, ref, buf=(100, 400))]))
    # the interrupted homopolymer's four probes (pos - 1, pos, right - 1, right), each deciding the maximum alone once: a deletion whose last
    # base ends an interrupted run of A that its first base lies before (right - 1), one that ends just before such a run (right), one that
    # begins just after one (pos - 1), one that takes a whole run from its first base on (pos)
    ref = make_ref(46, 300)
    ref = patch(ref, 148, "CTGAAAATAAAACGT")   # run 151..159: the deletion of 150..159 probes 149, 150, 159, 160
    ref = patch(ref, 198, "CTGCAAAATAAAAGT")   # run 202..210: the deletion of 200..201 probes 199, 200, 201, 202
    ref = patch(ref, 248, "GCCCCTCCCCAGTAC")   # run 249..257: the deletion of 258..260 probes 257, 258, 260, 261
    ref = patch(ref, 298, "GATTTTCTTTTGACA")   # run 300..308: the deletion of 300..309 probes 299, 300, 309, 310
    groups = [(6, [(M, 20), (D, 10), (M, 30)], {}, None, 130), (6, [(M, 20), (D, 2), (M, 30)], {}, None, 180),
              (6, [(M, 28), (D, 3), (M, 30)], {}, None, 230), (6, [(M, 20), (D, 10), (M, 30)], {}, None, 280)]
    out.append(dict(name="interrupted_hpol_probes", ref=ref, max_indel_size=49, regions=[], prev_end_in=-1, ploidy=[2], samples=[sample(groups, ref, buf=(100, 400))]))
    # a deletion the reads write at the right end of a run of six A; the region's aligner shifts it left: a key no read observed.  Sample 0's
    # read buffer does not cover the region (bypassed), sample 1 counts: the shifted key is not marked for sample 0 -- and is, with the samples
    # swapped.  The second region overlaps the first by a base and is bypassed in both samples: the last writer's id.
    ref = patch(make_ref(44), 199, "C" + "A" * 6 + "GTCAGT")
    right_end = [(M, 25), (D, 1), (M, 34)]
    for name, bufs in (("bypassed_then_discovered", ((100, 190), (100, 400))), ("discovered_then_bypassed", ((100, 400), (100, 190)))):
        out.append(dict(name=name, ref=ref, max_indel_size=49, regions=[(198, 209), (208, 215)], prev_end_in=-1, ploidy=[2, 1],
                        samples=[sample([(8, None, {}, None), (7, right_end, {}, None), (3, [(M, 30), (D, 2), (M, 28)], {}, None)], ref, buf=bufs[0], id_base=10),
                                 sample([(7, None, {}, None), (8, right_end, {}, None)], ref, buf=bufs[1], id_base=500, iat=lambda k: 1 if k % 4 == 0 else 0)]))
    # the same deletion found by two samples' regions, one of them with it in both alternates: ids 3 and 1, and a read's own observation of
    # the key the region hands back (the same id twice)
    ref = patch(make_ref(45), 202, "CAGTC")
    dele = [(M, 24), (D, 2), (M, 34)]
    out.append(dict(name="two_samples_one_deletion", ref=ref, max_indel_size=49, regions=[(200, 210), (230, 236)], prev_end_in=150, ploidy=[2, 2],
                    samples=[sample([(4, dele, {}, None), (3, dele, {208: None}, None)], ref, id_base=1),
                             sample([(9, None, {}, None), (6, dele, {}, None), (5, None, {232: None}, None)], ref, id_base=700, iat=lambda k: 2 if k == 3 else 0)]))
    return out


def run_scene(driver, sc, extra=()):
    lines = ["REF %d %s" % (REF_OFFSET, sc["ref"]), "OPT %d" % sc["max_indel_size"], "SAMPLES %d" % len(sc["samples"])]
    reads = []
    for s, sm in enumerate(sc["samples"]):
        lines.append("BUF %d %d %d" % (s, sm["buf"][0], sm["buf"][1]))
        reads += [(r[2], s, r) for r in sm["reads"]]
    for _, s, (rid, iat, pos, low, fwd, seq, path) in sorted(reads, key=lambda x: (x[0], x[1], x[2][0])):
        lines.append("READ %d %d %d %d %d %d %s %d %s" % (s, rid, iat, pos, low, fwd, seq, len(path), " ".join("%d %d" % t for t in path)))
    prev_end = sc["prev_end_in"]
    for b, e in sc["regions"]:
        lines.append("REGION %d %d %d %s" % (b, e, prev_end, " ".join(str(p) for p in sc["ploidy"])))
        prev_end = e
    lines += list(extra)
    out = subprocess.run([driver], input="\n".join(lines) + "\n", stdout=subprocess.PIPE, check=True, universal_newlines=True).stdout
    return json.loads(out)


def document(sc, recorded):
    return dict(name=sc["name"], ref=sc["ref"], ref_offset=REF_OFFSET, max_indel_size=sc["max_indel_size"], prev_end_in=sc["prev_end_in"],
                regions=[list(r) for r in sc["regions"]], ploidy=list(sc["ploidy"]),
                samples=[dict(buf_begin=sm["buf"][0], buf_end=sm["buf"][1],
                              reads=[dict(id=r[0], iat=r[1], pos=r[2], low_mapq=r[3], is_fwd=r[4], seq=r[5], path=[list(t) for t in r[6]]) for r in sm["reads"]])
                         for sm in sc["samples"]],
                assembled=recorded["assembled"], keys=recorded["keys"])


def main():
    driver = sys.argv[1]
    docs = []
    for sc in scenes():
        assert all(len(sm["reads"]) < 1000 for sm in sc["samples"])
        rec = run_scene(driver, sc)
        assert rec["assembled"] == 0, "%s: the reference would run the assembler" % sc["name"]
        docs.append(document(sc, rec))
    root = os.path.dirname(os.path.dirname(HERE))
    dst = os.path.join(root, "tests", "golden", "indel_table", "indel_table_golden.json")
    os.makedirs(os.path.dirname(dst), exist_ok=True)
    with open(dst, "w") as f:
        json.dump(dict(scenes=docs), f, separators=(",", ":"))
        f.write("\n")
    print("%s: %d scenes, %d reads, %d keys, %d bytes" % (dst, len(docs), sum(len(sm["reads"]) for d in docs for sm in d["samples"]), sum(len(d["keys"]) for d in docs),
                                                         os.path.getsize(dst)))
    sys.path.insert(0, root)
    from tests import indel_table_model as T
    T.golden.cache_clear()
    results = []
    for d in T.golden():
        samples, regions = T.scene_samples(d)
        keys, totals = T.indel_table(d["ref"], d["ref_offset"], samples, regions, d["prev_end_in"])
        same = T.as_recorded(keys) == d["keys"]
        print("  %-44s %3d keys%s%s" % (d["name"], len(d["keys"]), "" if same else "   <-- THE MODEL DIFFERS", "   <-- AR_PENDING" if any(k["flags"] & T.AR_PENDING for k in keys) else ""))
        results.append((samples, regions, keys, d["ref"], d["ref_offset"]))
    t = run_scene(driver, scenes()[-1], extra=["TIME 200"])
    print("  TIME %s" % json.dumps(t))
    for rule, n in T.rule_counts(results).items():
        print("  %-44s %d%s" % (rule, n, "" if n else "   <-- not covered"))


if __name__ == "__main__":
    main()
