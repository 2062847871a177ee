"""Record tests/golden/realign_gate/realign_gate_golden.json from the reference's own read-realignment gate over its own IndelBuffer.

  python tools/golden/make_realign_gate_golden.py <path of the built tools/golden/realign_gate_driver> [<path of the built tools/golden/indel_buffer_driver>]

Every scene of tests/golden/indel_candidates recorded under the germline or the somatic configuration runs again (named by reference, not
copied), every read with the widest realign range.  The scenes added here each let one line of the gate decide alone:

  gate_zone_edges       a deletion whose right end is zone_begin (in the range, no breakpoint inside) and one whose right end is zone_begin - 1
                        (the range's skip passes it); a key at pos == zone_end (not returned) and at zone_end - 1; a deletion whose left
                        breakpoint lies before the zone and whose right lies inside; an insertion (pos == right_pos) at either zone edge; a
                        non-candidate intersecting key before the first candidate; two candidates; the realign range exact and short by one
                        position on either side
  gate_mismatch_edges   (germline, one region) a MISMATCH key at zone_begin and at zone_end
  gate_noise_and_support (germline, one region) a read in the noise set and the tier-1 set of one key
  gate_clamped_at_0     a soft-clipped read whose range begins before position 0
  gate_overmax          max_indel_size 5: interior deletions of 5 and 6, edge insertions of 5 and 6 (which is_overmax skips)

A sub-mapped read comes with the reused scenes (tiers_and_noise).  The script refuses a
scene in which the model leaves any key undecided, in which the reference reached the assembler (the second driver, for the scenes added
here that close a region; the reused ones were checked when they were recorded), or in which the model differs from what was recorded.
Needed only to make the file again; the tests read the file."""
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_indel_candidates_golden as IC  # noqa: E402
import make_indel_table_golden as IT  # noqa: E402

M, I, D, S = IT.M, IT.I, IT.D, IT.S
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from tests import indel_candidates_model as CM  # noqa: E402
from tests import realign_gate_model as GM  # noqa: E402


def driver_lines(sc, ranges, time_repeats=0):
    """a scene in tests/golden/indel_candidates' form -> the driver's stdin"""
    doc = CM.scene_document(sc)
    if sc.get("drop_regions"):
        doc = dict(doc, regions=[])
    cfg = IC.CONFIGS[sc["config"]]
    assert "model_file" not in cfg
    lines = ["REF %d %s" % (doc["ref_offset"], doc["ref"]), "OPT %d" % doc["max_indel_size"], "SAMPLES %d" % len(doc["samples"])]
    reads = []
    for s, sm in enumerate(doc["samples"]):
        lines.append("BUF %d %d %d" % (s, sm["buf_begin"], sm["buf_end"]))
        reads += [(r["pos"], s, r["id"], r) for r in sm["reads"]]
    for _, s, _, r in sorted(reads, key=lambda x: x[:3]):
        lines.append("READ %d %d %d %d %d %d %s %d %s" % (s, r["id"], r["iat"], r["pos"], r["low_mapq"], r["is_fwd"], r["seq"], len(r["path"]), " ".join("%d %d" % tuple(t) for t in r["path"])))
    prev_end = doc["prev_end_in"]
    for b, e in doc["regions"]:
        lines.append("REGION %d %d %d %s" % (b, e, prev_end, " ".join(str(p) for p in doc["ploidy"])))
        prev_end = e
    lines += ["MODEL %s %d %r %d %d %d" % (cfg["model"], cfg["is_indel_ref_error_factor"], cfg["factor"], cfg["is_haplotyping_enabled"], cfg["is_candidate_indel_signal_test"],
                                          cfg["min_candidate_indel_open_length"]), "DEPTHFILTER %r" % float(sc["max_candidate_depth"]), "WIN %d %d" % (sc["win_begin"], sc["n_pos"])]
    lines += ["COUNT %d %d" % (s, c) for s, c in enumerate(sc["count_towards_depth"])]
    lines += ["RANGE %d %d %d %d" % tuple(r) for r in ranges]
    if time_repeats:
        lines.append("TIME %d" % time_repeats)
    return lines


def run_driver(driver, lines):
    return json.loads(subprocess.run([driver], input="\n".join(lines) + "\n", stdout=subprocess.PIPE, check=True, universal_newlines=True).stdout)


def candidate_form(sc, config, max_candidate_depth=None):
    """a scene in make_indel_table_golden's form -> one in tests/golden/indel_candidates' form (without what that file records)"""
    cfg = IC.CONFIGS[config]
    n = len(sc["samples"])
    return dict(name=sc["name"], config=config, win_begin=IT.REF_OFFSET, n_pos=len(sc["ref"]), count_towards_depth=[0 if s in cfg["not_counted"] else 1 for s in range(n)],
                max_candidate_depth=cfg["max_candidate_depth"] if max_candidate_depth is None else max_candidate_depth, scene=IT.document(sc, dict(assembled=0, keys=[])))


def read_id(sm, pos, path=None):
    """the id sample() gave the one read at pos (with that path)"""
    hit = [r[0] for r in sm["reads"] if r[2] == pos and (path is None or list(r[6]) == list(path))]
    assert len(hit) == 1, (pos, hit)
    return hit[0]


def _match_spans(pos, path):
    """the reference spans a path of match and deletion segments reads"""
    out = []
    for t, n in path:
        if t == M:
            out.append((pos, n))
        pos += n
    return out


def added_scenes():
    """[(scene in tests/golden/indel_candidates' form, ranges)]"""
    out = []
    ref = IC.plain_ref(61)
    probe = lambda pos, n=30: (1, [(M, n)], {}, None, pos)
    groups = [(12, None, {}, None), (4, IC.DEL2, {}, None), (1, [(M, 20), (D, 1), (M, 39)], {}, None), (4, [(M, 35), (D, 3), (M, 22)], {}, None),
              (4, [(M, 20), (I, 1), (M, 30)], {}, ["C"], 240)] + [probe(p) for p in (206, 207, 174, 175, 176, 177, 205, 260, 230)]
    sm = IT.sample(groups, ref)
    sc = dict(name="gate_zone_edges", ref=ref, max_indel_size=49, regions=[], prev_end_in=-1, ploidy=[2], samples=[sm])
    ranges = [[0, read_id(sm, 175), 175, 205], [0, read_id(sm, 176), 177, 206], [0, read_id(sm, 177), 177, 206]]
    out.append((candidate_form(sc, "somatic"), ranges))
    # a MISMATCH key at either edge: the recorded region scene with one read that begins at the key and one that ends before it
    base = next(x for x in IT.scenes() if x["name"] == "same_deletion_in_both_0")
    reads = list(base["samples"][0]["reads"])
    n = len(reads)
    for k, pos in enumerate((208, 178)):
        p, low, fwd, seq, path = IT.mk(base["ref"], pos, [(M, 30)])
        reads.append((n + k, 0, p, low, fwd, seq, path))
    sc = dict(base, name="gate_mismatch_edges", samples=[dict(base["samples"][0], reads=reads)])
    out.append((candidate_form(sc, "germline"), []))
    # a read in the noise set and the tier-1 set of one key: four reads carry the deletion in a tail of mismatches (a noise observation) and support
    # the region's deletion haplotype
    ref = IC.plain_ref(66)
    tail = [(M, 24), (D, 2), (M, 7)]
    sm = IT.sample([(9, None, {}, None), (9, IC.DEL2, {}, None), (4, tail, {207: None, 209: None, 211: None, 212: None}, None)], ref)
    sc = dict(name="gate_noise_and_support", ref=ref, max_indel_size=49, regions=[(200, 207)], prev_end_in=-1, ploidy=[2], samples=[sm])
    out.append((candidate_form(sc, "germline"), []))
    # the clamp at 0: ten clipped bases before position 4, on a reference segment that begins at 0
    ref = IC.plain_ref(64)
    at = lambda pos, path: "".join(ref[p:p + n] for p, n in _match_spans(pos, path))
    reads = [(4, [(S, 10), (M, 32)], "T" * 10 + ref[4:36])] + [(10, [(M, 60)], None)] * 6 + [(10, [(M, 24), (D, 2), (M, 34)], None)] * 3
    reads = [(i, 0, pos, 0, i % 2, seq or at(pos, path), path) for i, (pos, path, seq) in enumerate(reads)]
    sc = dict(name="gate_clamped_at_0", ref=ref, max_indel_size=49, regions=[], prev_end_in=-1, ploidy=[2], samples=[dict(buf=(0, 300), reads=reads)])
    cf = candidate_form(sc, "somatic")
    cf["win_begin"] = cf["scene"]["ref_offset"] = 0
    out.append((cf, []))
    # max_indel_size 5
    ref = IC.plain_ref(65)
    groups = [(10, None, {}, None), (3, [(M, 24), (D, 5), (M, 31)], {}, None), (3, [(M, 24), (D, 6), (M, 30)], {}, None), (2, [(I, 6), (M, 30)], {}, ["ACGTAC"], 190),
              (2, [(I, 5), (M, 30)], {}, ["ACGTA"], 195)]
    sc = dict(name="gate_overmax", ref=ref, max_indel_size=5, regions=[], prev_end_in=-1, ploidy=[2], samples=[IT.sample(groups, ref)])
    out.append((candidate_form(sc, "somatic"), []))
    return out


def main():
    driver = sys.argv[1]
    table_driver = sys.argv[2] if len(sys.argv) > 2 else None
    jobs = [(dict(candidate_scene=sc["name"]), sc, []) for sc in CM.golden()["scenes"] if sc["config"] in ("germline", "somatic")]
    for sc, ranges in added_scenes():
        if sc["scene"]["regions"]:
            assert table_driver, "%s closes a region: give the indel_buffer_driver too" % sc["name"]
            rec = run_driver(table_driver, [x for x in driver_lines(sc, []) if x.split()[0] in ("REF", "OPT", "SAMPLES", "BUF", "READ", "REGION")])
            assert rec["assembled"] == 0, "%s: the reference would run the assembler" % sc["name"]
        jobs.append((dict(scene=sc), sc, ranges))
    docs, bad = [], 0
    for head, sc, ranges in jobs:
        rec = run_driver(driver, driver_lines(sc, ranges))
        doc = dict(head, name=sc["name"], ranges=ranges, keys=rec["keys"], reads=[{k: v for k, v in r.items() if k != "range"} for r in rec["reads"]])
        keys, cand, samples, out = GM.run_recorded(doc)
        stray = [c for c in cand if c["undecided"] != CM.DECIDED]
        assert not stray, "%s: the model leaves a key undecided" % sc["name"]
        scene_doc = CM.scene_document(sc)
        want_keys, want_reads = GM.as_recorded(scene_doc, out)
        same = want_keys == doc["keys"] and want_reads == doc["reads"]
        bad += not same
        n_pass = sum(r["gate"] for r in doc["reads"])
        print("  %-64s %3d keys %3d reads %3d pass %3d consulted%s" % (sc["name"], len(doc["keys"]), len(doc["reads"]), n_pass, len({k for r in doc["reads"] for k in r["consulted"]}),
                                                                     "" if same else "   <-- THE MODEL DIFFERS"))
        if not same:
            for a, b in zip(want_keys, doc["keys"]):
                if a != b:
                    print("      key  model %s\n           ref   %s" % (a, b))
            for a, b in zip(want_reads, doc["reads"]):
                if a != b:
                    print("      read model %s\n           ref   %s" % (a, b))
        docs.append(doc)
    assert not bad, "%d scenes differ: nothing written" % bad
    dst = os.path.join(ROOT, "tests", "golden", "realign_gate", "realign_gate_golden.json")
    os.makedirs(os.path.dirname(dst), exist_ok=True)
    with open(dst, "w") as f:
        rows = [dict(d, keys=[[k[f] for f in GM.KEY_FIELDS] for k in d["keys"]], reads=[[r[f] for f in GM.READ_FIELDS] for r in d["reads"]]) for d in docs]
        json.dump(dict(scenes=rows), f, separators=(",", ":"))
        f.write("\n")
    print("%s: %d scenes, %d keys, %d reads, %d bytes" % (dst, len(docs), sum(len(d["keys"]) for d in docs), sum(len(d["reads"]) for d in docs), os.path.getsize(dst)))
    big = max((sc for _, sc, _ in jobs), key=lambda sc: sum(len(sm["reads"]) for sm in CM.scene_document(sc)["samples"]))
    print("  TIME %s %s" % (big["name"], json.dumps(run_driver(driver, driver_lines(big, [], time_repeats=200)))))


if __name__ == "__main__":
    main()
