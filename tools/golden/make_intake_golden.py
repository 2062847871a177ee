"""Record tests/golden/read_intake/intake_golden.json from the reference's own read intake.

  python tools/golden/make_intake_golden.py <path of the built tools/golden/intake_driver>

Seeded reads over a region of fewer than 1 000 positions (the detector's ring never wraps): matches with sparse and dense mismatches,
soft and hard clips, insertions, deletions and swaps below and above max_indel_size, edge indels, N and '=' bases, reads hanging off
both ends of the reference segment, low-MAPQ reads.  Needed only to make the file again; the tests read the file."""
import json
import os
import subprocess
import sys

import numpy as np

M, I, D, S, H = 1, 2, 3, 5, 6
REF_OFFSET, REF_LEN = 100, 700
SITES = (1, 999)
N_READS = 210


def make_ref(rng):
    ref = rng.choice(list("ACGT"), REF_LEN)
    ref[300:304] = "N"
    ref[520] = "N"
    return "".join(ref)


def ref_base(ref, p):
    return ref[p - REF_OFFSET] if REF_OFFSET <= p < REF_OFFSET + REF_LEN else "N"


def make_path(rng, kind):
    """-> [(type, length)] with at least one match segment"""
    body = []
    n_match = int(rng.integers(1, 5))
    for k in range(n_match):
        body.append((M, int(rng.integers(1, 70))))
        if k + 1 < n_match:
            what = rng.choice(["ins", "del", "swap_id", "swap_di", "long_ins", "long_del", "long_swap", "ins11"],
                              p=[0.25, 0.25, 0.1, 0.1, 0.08, 0.08, 0.07, 0.07])
            if what == "ins":
                body.append((I, int(rng.integers(1, 11))))
            elif what == "ins11":
                body.append((I, int(rng.integers(11, 30))))
            elif what == "del":
                body.append((D, int(rng.integers(1, 30))))
            elif what == "swap_id":
                body += [(I, int(rng.integers(1, 15))), (D, int(rng.integers(1, 15)))]
            elif what == "swap_di":
                body += [(D, int(rng.integers(1, 15))), (I, int(rng.integers(1, 15)))]
            elif what == "long_ins":
                body.append((I, int(rng.integers(49, 64))))
            elif what == "long_del":
                body.append((D, int(rng.integers(49, 64))))
            else:
                body += [(I, int(rng.integers(1, 60))), (D, int(rng.integers(45, 70)))]
    head, tail = [], []
    if kind == "clipped":
        if rng.random() < 0.7:
            head = [(S, int(rng.integers(1, 20)))]
        if rng.random() < 0.7:
            tail = [(S, int(rng.integers(1, 20)))]
        if rng.random() < 0.3:
            head = [(H, int(rng.integers(1, 9)))] + head
        if rng.random() < 0.3:
            tail = tail + [(H, int(rng.integers(1, 9)))]
    elif kind == "edge_indel":
        which = int(rng.integers(0, 6))
        if which == 0:
            head = [(I, int(rng.integers(1, 8)))]
        elif which == 1:
            head = [(D, int(rng.integers(1, 8)))]
        elif which == 2:
            tail = [(I, int(rng.integers(1, 8)))]
        elif which == 3:
            tail = [(D, int(rng.integers(1, 8)))]
        elif which == 4:
            head = [(S, 3), (I, 2), (D, 4)]  # an edge swap: every segment is visited on its own
        else:
            tail = [(D, 3), (I, 2), (S, 4)]
    return head + body + tail


def make_read(rng, ref, pos, path):
    dense_head = rng.random() < 0.2
    dense_tail = rng.random() < 0.2
    read_len = sum(l for t, l in path if t in (M, I, S))
    seq, p = [], pos
    for t, l in path:
        if t == M:
            for j in range(l):
                at = len(seq)
                rate = 0.02
                if (dense_head and at < 12) or (dense_tail and at >= read_len - 12):
                    rate = 0.6
                b = ref_base(ref, p + j)
                u = rng.random()
                if u < rate:
                    b = str(rng.choice([c for c in "ACGT" if c != b]))
                elif u < rate + 0.01:
                    b = "N"
                elif u < rate + 0.02:
                    b = "="
                seq.append(b)
            p += l
        elif t in (I, S):
            seq += [str(c) for c in rng.choice(list("ACGT"), l)]
        elif t == D:
            p += l
    return "".join(seq)


def main():
    driver = sys.argv[1]
    rng = np.random.default_rng(20261018)
    ref = make_ref(rng)
    lines = ["REF %d %s" % (REF_OFFSET, ref), "OPT 49", "SITES %d %d" % SITES]
    reads = []
    while len(reads) < N_READS:
        kind = str(rng.choice(["plain", "clipped", "edge_indel"], p=[0.5, 0.35, 0.15]))
        path = make_path(rng, kind)
        ref_span = sum(l for t, l in path if t in (M, D))
        pos = int(rng.integers(40, 880))
        if pos - 1 < SITES[0] or pos + ref_span + 1 >= SITES[1]:
            continue
        seq = make_read(rng, ref, pos, path)
        reads.append((pos, int(rng.random() < 0.1), seq, path))
    reads.append((400, 0, "A", [(M, 1)]))
    reads.sort(key=lambda r: r[0])
    for pos, low, seq, path in reads:
        lines.append("READ %d %d %s %d %s" % (pos, low, seq, len(path), " ".join("%d %d" % s for s in path)))
    out = subprocess.run([driver], input="\n".join(lines) + "\n", stdout=subprocess.PIPE, check=True, universal_newlines=True).stdout
    doc = json.loads(out)
    assert len(doc["reads"]) == len(reads)
    root = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    dst = os.path.join(root, "tests", "golden", "read_intake", "intake_golden.json")
    with open(dst, "w") as f:
        json.dump(doc, f, separators=(",", ":"))
        f.write("\n")
    n_obs = sum(len(r["obs"]) for r in doc["reads"])
    print("%s: %d reads, %d observations, %d sites, %d bytes" % (dst, len(doc["reads"]), n_obs, len(doc["sites"]), os.path.getsize(dst)))


if __name__ == "__main__":
    main()
