"""Record tests/golden/active_region_detect/*.json from the reference's own repeat finder and active-region detector.

  python tools/golden/make_active_region_golden.py <path of the built tools/golden/active_region_driver>

finder.json  anchors and _repeatSpan rows: the reference's unit-test string; a fresh finder at the segment's start (m = ref_offset = 0,
             so the stale slot is (unsigned)(-1) % 1000); a fresh finder followed by a second and a third region on the same, used
             finder, whose first two positions end a tract and whose stale slots hold what the first region left there, inside a tract
             of the same unit: the answer differs from a fresh finder's.
walk.json    region lists and the detector's six coordinates after every call, on seeded counters (mismatches and matches inserted
             per position): a window from position 0 and one inside a segment, both with depth-zero stretches.

Needed only to make the files again; the tests read the files."""
import json
import os
import subprocess
import sys

import numpy as np

BASES = "ACGT"


def repeat_rich(n, rng, max_unit=50):
    parts, size = [], 0
    while size < n:
        r = rng.random()
        if r < 0.25:
            s = BASES[int(rng.integers(0, 4))] * int(rng.integers(2, 14))
        elif r < 0.5:
            s = "".join(BASES[i] for i in rng.integers(0, 4, int(rng.integers(2, 7)))) * int(rng.integers(2, 6))
        elif r < 0.58:
            u = int(rng.integers(7, max_unit + 3))  # units up to 52: 51 and 52 are no repeats
            unit = "".join(BASES[i] for i in rng.integers(0, 4, u))
            s = (unit * 3)[:int(rng.integers(u + 1, 3 * u))]
        elif r < 0.62:
            s = "N" * int(rng.integers(1, 5))
        else:
            s = "".join(BASES[i] for i in rng.integers(0, 4, int(rng.integers(4, 30))))
        parts.append(s)
        size += len(s)
    return "".join(parts)[:n]


def put(ref, at, s):
    return ref[:at] + s + ref[at + len(s):]


def walk_sites(n, rng, candidate_rate):
    """(variant count, depth) per position: mostly quiet, candidates alone and in clusters, depth-zero stretches"""
    sites = []
    while len(sites) < n:
        r = rng.random()
        if r < 0.01:
            sites += [(0, 0)] * int(rng.integers(1, 30))
        elif r < 0.01 + candidate_rate:
            for _ in range(int(rng.integers(1, 4))):  # a cluster: candidates a few positions apart
                depth = int(rng.integers(8, 40))
                sites.append((int(depth * rng.uniform(0.4, 1.0)) + 1, depth + 1))
                for _ in range(int(rng.integers(0, 16))):
                    sites.append((0 if rng.random() < 0.8 else 1, int(rng.integers(10, 40))) if rng.random() < 0.93 else (0, 0))
        else:
            depth = int(rng.integers(10, 40))
            sites.append((int(rng.integers(0, 2)), depth))
    return sites[:n]


def run(driver, lines):
    out = subprocess.run([driver], input="\n".join(lines) + "\n", stdout=subprocess.PIPE, check=True, universal_newlines=True).stdout
    return json.loads(out)["items"]


def main():
    driver = sys.argv[1]
    root = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    dst = os.path.join(root, "tests", "golden", "active_region_detect")
    os.makedirs(dst, exist_ok=True)
    rng = np.random.default_rng(20261019)

    lines = ["REF 0 TATATACCCCCAATGAAAAA", "FINDER unit_test", "REGION 0 21 3 0 5 19"]
    # the segment's start: m = ref_offset = 0 although init_pos - 99 < 0, pos - u < ref_offset, a tract from position 0
    ref0 = put(repeat_rich(900, rng), 0, "CACACACACA")
    lines += ["REF 0 " + ref0, "FINDER segment_start", "REGION 30 700 3 0 1 600"]
    # three regions on one finder, segment 100 .. 3299
    ref = repeat_rich(3200, rng)
    ref = put(ref, 330 - 100, "T" * 40)                    # slot 350 (the third region's stale slot) lies in a homopolymer: span_1 = 21
    ref = put(ref, 388 - 100, "AG" * 12)                   # slot 400 (the second region's stale slot) in a unit-2 tract
    # the second region's first two positions (m = 1401) end a unit-2 tract: spans 1, 2 in a fresh finder, 14, 15 with the stale 13
    ref = put(ref, 1383 - 100, "AG" * 10 + "T")
    # the third's (m = 2351) end a homopolymer of 600: spans 1, 2 in a fresh finder, 22, 23 with the stale 21 -- 2u is stepped over
    ref = put(ref, 1753 - 100, "C" * 600 + "G")
    lines += ["REF 100 " + ref, "FINDER fresh_then_used", "REGION 150 900 3 100 420 1149", "REGION 1500 700 4 1401 1402 2100 2299",
              "REGION 2450 500 4 2351 2352 2499 2900"]
    items = run(driver, lines)
    path = os.path.join(dst, "finder.json")
    with open(path, "w") as f:
        json.dump(dict(items=items), f, separators=(",", ":"))
        f.write("\n")
    print("%s: %d finders, %d bytes" % (path, len(items), os.path.getsize(path)))

    ref_a = put(repeat_rich(2600, rng), 700, "N" * 6)
    ref_b = repeat_rich(1800, rng)
    lines = ["REF 0 " + ref_a, "WALK from_zero 0 2400 " + " ".join("%d %d" % s for s in walk_sites(2400, rng, 0.03)),
             "REF 1000 " + ref_b, "WALK inside 1050 1500 " + " ".join("%d %d" % s for s in walk_sites(1500, rng, 0.05))]
    items = run(driver, lines)
    path = os.path.join(dst, "walk.json")
    with open(path, "w") as f:
        json.dump(dict(items=items), f, separators=(",", ":"))
        f.write("\n")
    for it in items:
        print("%s: %d calls, %d regions" % (it["name"], len(it["calls"]), sum(1 for c in it["calls"] if c[9] >= 0)))
    print("%s: %d bytes" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
