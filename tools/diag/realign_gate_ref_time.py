"""BUILD CONTAINER, no GPU: the reference's own time for what sk_realign_gate replaces, on the reads of the windows tools/diag/realign_gate_bench.py
uses (seeded windows of about 8 192 and 16 384 positions at 40x, S = 1, 8), from the TIME mode of tools/golden/realign_gate_driver.cpp: per pass, over
a complete IndelBuffer with the cached candidate status cleared, for every read get_alignment_zone, is_realignable, check_for_candidate_indel_overlap
and is_usable_indel over the zone's keys.  One core.  No regions are closed (haplotyping off); every read has the widest realign range.
usage: python tools/diag/realign_gate_ref_time.py <built driver> [repeats]"""
import subprocess
import sys

sys.path.insert(0, ".")
from tests import intake_model as M  # noqa: E402
from tests import region_haplotype_cases as R  # noqa: E402

driver = sys.argv[1]
repeats = int(sys.argv[2]) if len(sys.argv) > 2 else 10
for n_pos in (8192, 16384):
    for n_samples in (1, 8):
        base = R.seeded_window(n_pos * 40 // 100, 9100 + n_pos)
        ref, off, win_begin, n = base["ref"], base["ref_offset"], base["win_begin"], base["n_pos"]
        lines = ["REF %d %s" % (off, ref), "OPT 49", "SAMPLES %d" % n_samples, "MODEL adaptiveDefault 1 1.8 0 1 20", "DEPTHFILTER %r" % (120.0 * n_samples), "WIN %d %d" % (win_begin, n)]
        n_reads = 0
        for s in range(n_samples):
            keep = [k for k in range(len(base["reads"])) if n_samples == 1 or k % 8 != s]
            for j, k in enumerate(keep):
                r = base["reads"][k]
                seq = "".join(M.read_char(r["code"], i) for i in range(len(r["code"])))
                lines.append("READ %d %d %d %d %d %d %s %d %s" % (s, j, 0 if j % 11 else 1, r["pos"], base["low"][k], base["fwd"][k], seq, len(r["path"]), " ".join("%d %d" % tuple(t) for t in r["path"])))
                n_reads += 1
        lines.append("TIME %d" % repeats)
        out = subprocess.run([driver], input="\n".join(lines) + "\n", stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
        print("n_pos_%d_samples_%d" % (n_pos, n_samples), out.stdout.strip() if out.returncode == 0 else out.stderr.strip()[-300:], flush=True)
