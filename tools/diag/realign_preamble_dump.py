"""the crafted preamble scenes (tests/realign_preamble_cases.py) with the model's gate outputs, as one binary file for tools/diag/realign_preamble_sanitize.cpp.
usage: python tools/diag/realign_preamble_dump.py OUT
layout, little endian: int32 n_scenes; per scene int32 n_samples, max_indel_size, ref_offset, ref_len, is_haplotyping_enabled; the reference; int64 n_keys;
sk_realign_gate_key[n_keys]; sk_realign_gate_log_rates[n_keys * n_samples]; int64 insert_len; the insert pool; per sample int32 n_reads; int64 path_cap; pos, path_off,
n_seg, path[path_cap], read_len, realign_begin, realign_end, sk_realign_gate_read[n_reads], observed_off[n_reads + 1], int64 n_observed, observed, read_off[n_reads + 1],
int64 code_cap, the codes, is_fwd_strand[n_reads]"""
import sys

import numpy as np

sys.path.insert(0, ".")
from tests import realign_preamble_cases as P  # noqa: E402

with open(sys.argv[1], "wb") as f:
    i32 = lambda *v: f.write(np.array(v, np.int32).tobytes())
    i64 = lambda *v: f.write(np.array(v, np.int64).tobytes())
    scenes = P.crafted()
    i32(len(scenes))
    for sc in scenes:
        gate, ins, _ = P.model_gate(sc)
        ps, pp = P.packed(sc)
        ref = sc["ref"].encode()
        i32(len(sc["samples"]), sc["max_indel_size"], sc["ref_offset"], len(ref), sc["hap"])
        f.write(ref)
        i64(len(gate["keys"]))
        f.write(gate["keys"].tobytes())
        f.write(gate["logs"].tobytes())
        i64(len(ins))
        f.write(np.ascontiguousarray(ins).tobytes())
        for p, q, g in zip(ps, pp, gate["samples"]):
            n = p["n_reads"]
            i32(n)
            i64(p["path_cap"])
            for name in ("pos", "path_off", "n_seg"):
                f.write(p[name][:n].tobytes())
            f.write(p["path"][:p["path_cap"]].tobytes())
            for name in ("read_len", "realign_begin", "realign_end"):
                f.write(p[name][:n].tobytes())
            f.write(g["reads"][:n].tobytes())
            f.write(g["observed_off"][:n + 1].tobytes())
            i64(g["observed_cap"])
            f.write(g["observed"][:g["observed_cap"]].tobytes())
            f.write(q["read_off"][:n + 1].tobytes())
            i64(q["code_cap"])
            f.write(q["read_code"][:q["code_cap"]].tobytes())
            f.write(q["is_fwd_strand"][:n].tobytes())
