"""Record tests/golden/indel_candidates/indel_candidates_golden.json from the reference's own IndelBuffer, depth buffers, count cache and
error model.

  python tools/golden/make_indel_candidates_golden.py <path of the built tools/golden/indel_candidate_driver>

Every scene of tools/golden/make_indel_table_golden.py runs under both product configurations (named by reference to
tests/golden/indel_table, not copied):

  germline  adaptiveDefault, indelRefErrorFactor 1.8 on, haplotyping on, every sample counted towards depth, depth filter at 200
  somatic   logLinear, no factor, haplotyping off, sample 1 not counted, no depth filter; the scene's regions are dropped (with haplotyping
            off the reference keeps no reads for regions and the product closes none)

and the scenes added here each let one test decide alone.  Two further configurations read a model file, which is the only way to give the
reference rates of 0.5 and above and rate sets per sample.  What could not be recorded, and why:

  n1 above the depth (the "fudge" line) from the depth buffer itself: a read that carries an indel at pos has an alignment match at pos - 1,
      so depth1[pos - 1] >= n1 always.  The window-edge scene takes its place: the window begins at the key, depth1[pos - 1] reads 0 in the
      batch, and only the reads with the deletion cover pos - 1, so the reference's total is n1 too.
  the breakpoint length test deciding: every breakpoint key is doNotGenotype (IndelBuffer.cpp:119-128), which is asked first.  The two
      breakpoint scenes pin getBreakpointInsertSize (19 and 20); the test itself is exercised on crafted tables by the model and device tests.

Every scene keeps the depth under 1 000, and the script refuses a scene in which the model leaves a key undecided for any reason but
AR_PENDING, or where the reference would run the assembler.  Needed only to make the file again; the tests read the file."""
import json
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_indel_table_golden as IT  # noqa: E402

M, I, D = IT.M, IT.I, IT.D
REF_OFFSET = IT.REF_OFFSET
patch, make_ref, sample = IT.patch, IT.make_ref, IT.sample

CONFIGS = dict(
    germline=dict(model="adaptiveDefault", is_indel_ref_error_factor=1, factor=1.8, is_haplotyping_enabled=1, is_candidate_indel_signal_test=1,
                  min_candidate_indel_open_length=20, not_counted=(), max_candidate_depth=200.0),
    somatic=dict(model="logLinear", is_indel_ref_error_factor=0, factor=1.0, is_haplotyping_enabled=0, is_candidate_indel_signal_test=1,
                 min_candidate_indel_open_length=20, not_counted=(1,), max_candidate_depth=-1.0),
    weak_signal=dict(model="logLinear", is_indel_ref_error_factor=0, factor=1.0, is_haplotyping_enabled=0, is_candidate_indel_signal_test=0,
                     min_candidate_indel_open_length=20, not_counted=(), max_candidate_depth=-1.0),
    # model files: [(sample name, [(pattern size, repeat count, rate)])]
    high_rates=dict(model="logLinear", is_indel_ref_error_factor=1, factor=1.8, is_haplotyping_enabled=0, is_candidate_indel_signal_test=1,
                    min_candidate_indel_open_length=20, not_counted=(), max_candidate_depth=-1.0,
                    model_file=[("default", [(1, 1, 0.5), (1, 2, 0.7), (1, 3, 0.2), (2, 1, 0.01), (2, 2, 0.3)])]),
    rates_per_sample=dict(model="logLinear", is_indel_ref_error_factor=1, factor=2.5, is_haplotyping_enabled=0, is_candidate_indel_signal_test=1,
                          min_candidate_indel_open_length=20, not_counted=(), max_candidate_depth=-1.0,
                          model_file=[("sample0.bam", [(1, 1, 1e-3), (1, 2, 2e-3)]), ("sample1.bam", [(1, 1, 0.04), (1, 2, 0.6), (2, 1, 0.25)])]),
)

DEL2 = [(M, 24), (D, 2), (M, 34)]  # from 180: the deletion of 204..205


def plain_ref(seed):
    return patch(make_ref(seed), 200, "GCATCAGT")  # 204..205 is "CA" in no repeat: unit length 2


def added_scenes():
    """[(scene in make_indel_table_golden's form, configuration, dict(win, max_candidate_depth))]"""
    out = []

    def add(name, config, samples, ref, max_indel_size=49, **extra):
        out.append((dict(name=name, ref=ref, max_indel_size=max_indel_size, regions=[], prev_end_in=-1, ploidy=[2] * len(samples), samples=samples), config, extra))

    ref = plain_ref(61)
    # total of 0 (the only reads with the deletion are sub-mapped, nothing else covers), 1 and 2
    add("total_0", "somatic", [sample([(3, DEL2, {}, None)], ref, iat=lambda k: 2)], ref)
    add("total_1", "somatic", [sample([(1, DEL2, {}, None)], ref)], ref)
    add("total_2", "somatic", [sample([(2, DEL2, {}, None)], ref)], ref)
    # n1 of 1, 2, 3 at depth 20: with p = 5e-5, 20 p = 1e-3 lies between papprox[1] and papprox[2]
    for n1 in (1, 2, 3):
        add("n1_%d_at_depth_20" % n1, "somatic", [sample([(20 - n1, None, {}, None), (n1, DEL2, {}, None)], ref)], ref)
    # n1 >= 18: the min(n1, 18) clamp
    add("n1_19_of_25", "somatic", [sample([(6, None, {}, None), (19, DEL2, {}, None)], ref)], ref)
    # the depth sum equal to the limit and one above it: sample 0 has 9 tier-1 and 3 tier-2 reads at 203, sample 1 (not counted) 5 more
    # (which three reads are tier 2 follows the interleaving: at least five of the eight with the deletion stay tier 1, enough at depth 9)
    two = [sample([(4, None, {}, None), (8, DEL2, {}, None)], ref, iat=lambda k: 1 if k >= 9 else 0),
           sample([(5, None, {}, None)], ref, id_base=500)]
    add("depth_sum_equal_to_limit", "somatic", two, ref, max_candidate_depth=12.0)
    add("depth_sum_one_above_limit", "somatic", two, ref, max_candidate_depth=11.0)
    add("depth_sum_counts_every_sample", "germline_no_regions", two, ref, max_candidate_depth=16.0)
    # breakpoints: an insertion of 26 bases above max_indel_size 19 and 20 -- the breakpoint's insert sequence is cut at max_indel_size
    for n in (19, 20):
        ins = ("ACGTTGCATGCAAGCTTGCA" * 2)[:26]
        add("breakpoint_insert_%d" % n, "somatic", [sample([(8, None, {}, None), (6, [(M, 24), (I, 26), (M, 10)], {}, [ins])], ref)], ref, max_indel_size=n)
    # a key at the window's first position: pos - 1 is outside, and only the three reads with the deletion cover it
    add("key_at_window_begin", "somatic", [sample([(3, DEL2, {}, None)], ref)], ref, win=(204, 120))
    # the weak test: one tier-1 read is enough, a tier-2 read is not
    add("weak_signal_one_read", "weak_signal", [sample([(1, DEL2, {}, None)], ref)], ref)
    add("weak_signal_tier2_only", "weak_signal", [sample([(2, DEL2, {}, None)], ref, iat=lambda k: 1)], ref)
    # rates of 0.5 and above through the scaling: one base out of a single C (counts 1, 1: 0.5 both ways), out of CC (ref count 2: 0.7, back 0.5),
    # out of CCC (back: count 2, 0.7, capped), one base into CC (ref count 2, indel count 3)
    ref = make_ref(62)
    ref = patch(ref, 148, "GACGT")      # 150: C
    ref = patch(ref, 198, "GACCGT")     # 200..201: CC
    ref = patch(ref, 248, "GACCCGT")    # 250..252: CCC
    ref = patch(ref, 298, "TGACACAT")   # 300..303: ACAC
    groups = [(4, [(M, 20), (D, 1), (M, 30)], {}, None, 130), (4, [(M, 20), (D, 1), (M, 30)], {}, None, 180), (4, [(M, 20), (D, 1), (M, 30)], {}, None, 230),
              (4, [(M, 20), (I, 1), (M, 30)], {}, ["C"], 180), (4, [(M, 20), (D, 2), (M, 30)], {}, None, 280), (4, [(M, 20), (I, 2), (M, 30)], {}, ["AC"], 280)]
    add("rates_at_and_above_one_half", "high_rates", [sample(groups, ref)], ref)
    add("rates_per_sample", "rates_per_sample", [sample(groups, ref), sample(groups[1:4], ref, id_base=400)], ref)
    # a homopolymer past the table's last repeat count (20 > 16), and a repeat unit longer than the set's sizes (CAG: 3 > 2 and > 1)
    ref = make_ref(63)
    ref = patch(ref, 199, "C" + "A" * 20 + "G")
    ref = patch(ref, 299, "T" + "CAG" * 4 + "T")
    groups = [(5, [(M, 20), (D, 1), (M, 40)], {}, None, 180), (5, [(M, 20), (I, 2), (M, 40)], {}, ["AA"], 180), (5, [(M, 20), (D, 3), (M, 30)], {}, None, 280)]
    for config in ("somatic", "germline_no_regions", "high_rates"):
        add("repeat_counts_and_sizes_past_the_sets_%s" % config, config, [sample(groups, ref)], ref)
    return out


CONFIGS["germline_no_regions"] = dict(CONFIGS["germline"], is_haplotyping_enabled=0)  # the germline rates, for scenes that close no region


def model_file(spec, directory):
    doc = dict(sample=[dict(sampleName=name, isStatic=True,
                            motif=[dict(repeatPatternSize=size, repeatCount=count, indelRate=rate, noisyLocusRate=0.0) for size, count, rate in motifs])
                       for name, motifs in spec])
    path = os.path.join(directory, "model_%d.json" % abs(hash(json.dumps(doc, sort_keys=True))))
    with open(path, "w") as f:
        json.dump(doc, f)
    return path


def record(driver, sc, config, extra, directory, time_repeats=0):
    cfg = CONFIGS[config]
    n_samples = len(sc["samples"])
    win = extra.get("win", (REF_OFFSET, len(sc["ref"])))
    limit = extra.get("max_candidate_depth", cfg["max_candidate_depth"])
    count = [0 if s in cfg["not_counted"] else 1 for s in range(n_samples)]
    lines = ["MODEL %s %d %r %d %d %d" % (cfg["model"], cfg["is_indel_ref_error_factor"], cfg["factor"], cfg["is_haplotyping_enabled"], cfg["is_candidate_indel_signal_test"],
                                          cfg["min_candidate_indel_open_length"]), "DEPTHFILTER %r" % limit, "WIN %d %d" % win]
    lines += ["COUNT %d %d" % (s, c) for s, c in enumerate(count)]
    if "model_file" in cfg:
        lines.append("MODELFILE " + model_file(cfg["model_file"], directory))
    if time_repeats:
        lines.append("TIME %d" % time_repeats)
    return IT.run_scene(driver, sc, extra=lines), win, limit, count


def sparse(values, first):
    """a dense array -> (first covered position, the values up to the last covered one)"""
    nz = [i for i, v in enumerate(values) if v]
    return [first, []] if not nz else [first + nz[0], values[nz[0]:nz[-1] + 1]]


def main():
    driver = sys.argv[1]
    root = os.path.dirname(os.path.dirname(HERE))
    sys.path.insert(0, root)
    from tests import indel_candidates_model as CM
    from tests import indel_table_model as T
    table_names = {d["name"] for d in T.golden()}
    jobs = []
    for sc in IT.scenes():
        assert sc["name"] in table_names
        # (with haplotyping off the reference keeps no reads for its regions, and the product closes none: the somatic runs drop them)
        jobs += [(sc, "germline", {}, True), (dict(sc, regions=[]), "somatic", {}, True)]
    jobs += [(sc, config, extra, False) for sc, config, extra in added_scenes()]
    configs, docs = {}, []
    with tempfile.TemporaryDirectory() as directory:
        for sc, config, extra, is_table_scene in jobs:
            assert all(len(sm["reads"]) < 1000 for sm in sc["samples"])
            rec, win, limit, count = record(driver, sc, config, extra, directory)
            cfg = CONFIGS[config]
            recorded_cfg = dict(papprox=rec["papprox"], log_indel_ref_error_factor=rec["log_indel_ref_error_factor"], is_sample_specific_rates=rec["is_sample_specific"],
                                candidate_rates=rec["candidate_rates"], sample_rates=[r["set"] for r in rec["sample_rates"]],
                                **{k: cfg[k] for k in ("is_indel_ref_error_factor", "is_haplotyping_enabled", "is_candidate_indel_signal_test", "min_candidate_indel_open_length")})
            assert configs.setdefault(config, recorded_cfg) == recorded_cfg
            doc = dict(name="%s@%s" % (sc["name"], config) if is_table_scene else sc["name"], config=config, win_begin=win[0], n_pos=win[1], count_towards_depth=count,
                       max_candidate_depth=limit, depth=[[sparse(d, win[0]) for d in pair] for pair in rec["depth"]], keys=rec["keys"])
            if is_table_scene:
                doc["table_scene"] = sc["name"]
                doc["drop_regions"] = int(not sc["regions"])
            else:
                assert not sc["regions"]  # (no region: nothing the reference would hand to the assembler)
                doc["scene"] = IT.document(sc, dict(assembled=0, keys=[]))
            docs.append(doc)
        timed = [record(driver, sc, config, {}, directory, time_repeats=200)[0] for sc, config in ((IT.scenes()[-1], "germline"), (IT.scenes()[-1], "somatic"))]
    dst = os.path.join(root, "tests", "golden", "indel_candidates", "indel_candidates_golden.json")
    os.makedirs(os.path.dirname(dst), exist_ok=True)
    with open(dst, "w") as f:
        json.dump(dict(configs=configs, scenes=docs), f, separators=(",", ":"))
        f.write("\n")
    print("%s: %d scenes, %d keys, %d bytes" % (dst, len(docs), sum(len(d["keys"]) for d in docs), os.path.getsize(dst)))
    CM.golden.cache_clear()
    g = CM.golden()
    n_cand = n_pending = 0
    for sc in g["scenes"]:
        keys, depth, out, totals = CM.run_recorded(sc)
        same = CM.as_recorded(keys, out) == sc["keys"] and CM.depth_as_recorded(depth, sc) == sc["depth"]
        stray = [o for k, o in zip(keys, out) if o["undecided"] not in (CM.DECIDED, CM.UNDECIDED_AR_PENDING)]
        assert not stray, "%s: a key undecided for a reason other than AR_PENDING" % sc["name"]
        n_cand += totals[0]
        n_pending += totals[1]
        print("  %-64s %3d keys %3d candidates%s" % (sc["name"], len(keys), totals[0], "" if same else "   <-- THE MODEL DIFFERS"))
    print("  candidates %d, AR_PENDING %d" % (n_cand, n_pending))
    for t in timed:
        print("  TIME %s" % json.dumps(t))


if __name__ == "__main__":
    main()
