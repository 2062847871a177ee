"""Record tests/golden/sync_regions/*.json from the reference's own multi-sample ActiveRegionDetector.

  python tools/golden/make_sync_regions_golden.py <path of the built tools/golden/sync_regions_driver>

one_sample.json     S = 1 from position 0, with clear() at the end
two_samples.json    S = 2 inside a segment, in three chained windows: regions shared by both samples, closes put off by the other sample's
                    start, a sample's second region merging into its own first, regions over 250 positions, ploidy marks, clear() with an
                    open synchronised region
three_samples.json  S = 3 from position 0; clear(), then two candidates inside a tandem repeat before any anchor and clear() on an empty
                    read buffer (closeActiveRegionDetector's third branch)
eight_samples.json  S = 8 inside a segment

The counts the issue asks for are printed, and tests/test_sync_regions_model.py asserts them from the files.

Needed only to make the files again; the tests read the files."""
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from tests import sync_cases  # noqa: E402

BASES = "ACGT"
QUIET, CAND, ZERO = (0, 20), (15, 20), (0, 0)


def plain_reference(n, rng):
    """mostly unique sequence with a short tandem repeat now and then: most positions are anchors"""
    parts, size = [], 0
    while size < n:
        r = rng.random()
        if r < 0.08:
            s = BASES[int(rng.integers(0, 4))] * int(rng.integers(3, 9))
        elif r < 0.14:
            s = "".join(BASES[i] for i in rng.integers(0, 4, int(rng.integers(2, 5)))) * int(rng.integers(2, 5))
        else:
            s = "".join(BASES[i] for i in rng.integers(0, 4, int(rng.integers(8, 40))))
        parts.append(s)
        size += len(s)
    return "".join(parts)[:n]


def put(ref, at, s):
    return ref[:at] + s + ref[at + len(s):]


def random_sites(n_samples, n, rng, spacing=(35, 70), join=0.6, long_chain=0.25, tight=False):
    """clusters of candidates at places the samples share, each sample joining with its own shift and its own number of candidates; now
    and then a sample's chain runs on for a hundred positions, which holds the others' regions open; tight: clusters of two to four
    candidates at most five apart, so that neighbouring clusters stay regions of their own"""
    sites = [[QUIET] * n for _ in range(n_samples)]
    at = 20
    while at < n - 40:
        for s in range(n_samples):
            if rng.random() >= join:
                continue
            p = at + int(rng.integers(-5, 6) if tight else rng.integers(-8, 9))
            long = rng.random() < long_chain
            k = int(rng.integers(8, 14)) if long else int(rng.integers(2 if tight else 1, 5))
            for _ in range(k):
                if 0 <= p < n:
                    sites[s][p] = CAND
                p += int(rng.integers(1, 6 if tight and not long else 14))
        if rng.random() < 0.2:
            s, p = int(rng.integers(0, n_samples)), at + int(rng.integers(10, 25))
            for q in range(p, min(n, p + int(rng.integers(2, 20)))):
                sites[s][q] = ZERO
        at += int(rng.integers(*spacing))
    return sites


def chain(sites, s, begin, end, step):
    for p in range(begin, end, step):
        sites[s][p] = CAND


def step_line(win_begin, sites, a, b):
    return "STEP %d %d " % (win_begin + a, b - a) + " ".join("%d %d" % x for row in sites for x in row[a:b])


def run(driver, lines):
    out = subprocess.run([driver], input="\n".join(lines) + "\n", stdout=subprocess.PIPE, check=True, universal_newlines=True).stdout
    return json.loads(out)["items"]


def regions_without_marks(driver, ref_line, begin_line, steps):
    """a first pass, to learn where the regions fall: the marks go on their first and last positions"""
    item = run(driver, [ref_line, begin_line] + steps)[0]
    return sync_cases.replay(item)["regions"]


def main():
    driver = sys.argv[1]
    dst = os.path.join(ROOT, "tests", "golden", "sync_regions")
    os.makedirs(dst, exist_ok=True)
    rng = np.random.default_rng(20261020)
    files = {}

    # S = 1 from position 0
    ref = plain_reference(1300, rng)
    sites = random_sites(1, 400, rng, spacing=(30, 60), join=0.9)
    chain(sites, 0, 390, 400, 4)  # an open pair at the end: clear() makes the region
    files["one_sample"] = ["REF 0 " + ref, "BEGIN one_sample 1 2", step_line(0, sites, 0, 400), "CLEAR"]

    # S = 2 inside a segment, three windows
    ref = plain_reference(2400, rng)
    n, win_begin = 1650, 1050
    sites = random_sites(2, n, rng, spacing=(36, 46), join=0.9, long_chain=0.06, tight=True)
    for p in range(300, 700):
        sites[0][p] = sites[1][p] = QUIET
    # a sample's second region merges into its own first: sample 1's chain holds sample 0's first region open until its second is made
    chain(sites, 1, 310, 420, 9)
    chain(sites, 0, 330, 338, 3)
    chain(sites, 0, 362, 370, 3)
    # regions over 250 positions: one of one sample, one of both, one made of two that overlap
    chain(sites, 0, 450, 730, 11)
    for p in range(760, 1400):
        sites[0][p] = sites[1][p] = QUIET
    chain(sites, 0, 780, 1060, 12)
    chain(sites, 1, 800, 1080, 10)
    chain(sites, 0, 1100, 1290, 12)
    chain(sites, 1, 1240, 1390, 13)
    # at the end: sample 0's region made and held open by sample 1's chain, which runs to the last position: no anchor after it
    for p in range(n - 60, n):
        sites[0][p] = sites[1][p] = QUIET
    chain(sites, 0, n - 40, n - 30, 4)
    chain(sites, 1, n - 43, n, 6)
    ref_line, begin_line = "REF 1000 " + ref, "BEGIN two_samples 2 2"
    # the first cut lies inside the nine positions of padding behind a region that is made, the second inside a region that a sample's
    # start has held open beyond them: both found in a first pass over one window
    rows = run(driver, [ref_line, begin_line, step_line(win_begin, sites, 0, n)])[0]["ops"][0]["calls"]
    last = [None, 0]
    open_at = [(k + 1, sync_cases.decode_row(row, 2, win_begin + k + 1, last)[0]["sync_end"]) for k, row in enumerate(rows)]
    in_padding = [k for k, end in open_at if end and win_begin + k < end + 9]
    held = [k for k, end in open_at if end and win_begin + k >= end + 9 and k > in_padding[0] + 600]
    cuts = [0, in_padding[0], held[0], n]
    steps = [step_line(win_begin, sites, a, b) for a, b in zip(cuts[:-1], cuts[1:])]
    found = regions_without_marks(driver, ref_line, begin_line, steps)
    marks = []
    for k, r in enumerate(found[2::3][:8]):  # sample k % 2 is haploid over every third region; one mark alone changes nothing (the max of the two ends)
        marks += ["PLOIDY %d %d 1" % (k % 2, r["begin"]), "PLOIDY %d %d 1" % (k % 2, r["end"] - 1)]
    marks.append("PLOIDY 0 %d 1" % found[1]["begin"])
    files["two_samples"] = [ref_line, begin_line] + marks + steps + ["CLEAR"]

    # S = 3 from position 0; clear(), then candidates before any anchor and clear() on an empty buffer
    n = 450
    ref = put(plain_reference(1000, rng), n - 4, "AC" * 40)
    sites = random_sites(3, n, rng, spacing=(36, 46), join=0.8, long_chain=0.06, tight=True)
    tail = [[QUIET] * 30 for _ in range(3)]
    for s in (0, 2):
        tail[s][2] = tail[s][6] = CAND
    ref_line, begin_line = "REF 0 " + ref, "BEGIN three_samples 3 2"
    found = regions_without_marks(driver, ref_line, begin_line, [step_line(0, sites, 0, n)])
    marks = ["PLOIDY 1 %d 1" % p for r in found[1::4][:4] for p in (r["begin"], r["end"] - 1)]
    files["three_samples"] = [ref_line, begin_line] + marks + [step_line(0, sites, 0, n), "CLEAR", step_line(n, tail, 0, 30), "CLEARBUF %d %d" % (n - 10, n + 30), "CLEAR"]

    # S = 8 inside a segment
    ref = plain_reference(900, rng)
    sites = random_sites(8, 280, rng, spacing=(36, 46), join=0.4, long_chain=0.05, tight=True)
    files["eight_samples"] = ["REF 500 " + ref, "BEGIN eight_samples 8 2", step_line(560, sites, 0, 280), "CLEAR"]

    total = 0
    for name, lines in files.items():
        items = run(driver, lines)
        path = os.path.join(dst, name + ".json")
        with open(path, "w") as f:
            json.dump(dict(items=items), f, separators=(",", ":"))
            f.write("\n")
        total += os.path.getsize(path)
        print("%s: %d bytes" % (path, os.path.getsize(path)))
    print("total %d bytes" % total)
    for k, v in sorted(sync_cases.coverage().items()):
        print("%-28s %s" % (k, v))


if __name__ == "__main__":
    main()
