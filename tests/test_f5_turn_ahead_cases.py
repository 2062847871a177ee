"""F5 (flatten_score_kernel) against the staged chain ($SK_A5_FUSED=0) and the host path (enumeration = 0) on small jobs that reach
the cases of a read queue whose first read is not drawn, and the cases at which a sum loop that fetches its byte words a turn ahead
and a walk preamble that reads (position, packed lengths) pairs from the table copy can go wrong (both were built with the queue
change, measured and taken out again, profiles/r09_f5_history.txt: the cases stay for whoever moves those loads next).  The three
give equal results (repr of every result), equal sets of consulted indels and
equal counts of reference reads outside the job's reference; every F5 job is run twice and gives the same; and F5 scored the jobs
itself (device_job_counts: one fixed sequence, nothing run again the staged way) -- a case counts only in such a job.

The cases are counted from the inputs: from the host form's own batch of the same job (RealignJob.batch() at enumeration = 0: every
candidate alignment as its ops -- bases / soft clip / no base, length, pool offset, penalty flag -- which is what F5's walk and sums
restate), from the reads (lengths, codes) and from the indel table.  Each is asserted to occur.

Phase B: ops of 1, 7, 8, 9 and 16 bases; an alignment whose last op of bases ends a multiple of 8 from its start; reads of 1-9 bases;
reads of 150, 151, 152 bases (the pad of the 152-base form), of 153 and 256 (the 256-base form); a leading and a trailing soft clip
(counted in the reads' input alignments, as tests/test_f5_phase_b_cases.py does: the search re-aligns a clipped edge, and the host
batches of these jobs hold no soft-clip op, so the clip terms of the sums are reached only where the search keeps a clip); a
penalty directly before and directly after an op of exactly 8 bases; an N and a '=' among a read's last eight bases; the largest
pool of the scenarios and an alignment whose last op's pool bytes end at its pool's last byte.
Walk: an input alignment over seven table indels, a leading edge insert and six inner ones.  Eight (F5_INDELS) are not reached in a job
F5 scores: between two indels lies a match segment, so eight fit the record's sixteen segments only as six inner indels between two
edge inserts, 15 segments -- that read is run too (the job "walk_eight"), the search toggles all eight (1 900 candidate alignments,
some of 16 ops) and F5 turns the job down: it is compared three ways like the others and counts for nothing.  A lead and a trail
edge insert; a swap (a delete + insert run); a breakpoint-typed table entry; a table over 32
entries whose first 40 lie before every read (the per-round copy with tab_lo > 0); an insert entry far from every read (not in any
pool: ins_at = -1 in the copy).
Not stated: a table entry with a length of 0xffff or more that an alignment names.  synth can put one in the table, but a read over it
has a window of more than F5_MAX_POOL bytes and leaves F5 at the pool gate, before the walk's preamble looks at the entry.
Queue: a few distinct short reads tiled to n reads for n around the number of resident waves W (4 096 for the 152-base form, 3 072
for the 256-base form), one of them a read the gate turns down (no candidate alignments), and sk_realign_job_rescore(2) followed by
reading the results again.  A read whose status is not OK is not stated: the scenarios have none."""
import numpy as np
import pytest

from strelka_amd import capi, synth
from tests import f5_util as U

_BASES = "ACGT"
_CODE = {"A": 1, "C": 2, "G": 4, "T": 8, "N": 15}
_M, _I, _D, _S = synth.SEG["MATCH"], synth.SEG["INSERT"], synth.SEG["DELETE"], synth.SEG["SOFT_CLIP"]
_TAB = 32   # entries of the per-read table copy (F5_TAB)
_W = {152: 4096, 256: 3072}   # waves resident: 256 CUs x 16 (two eight-wave blocks), x 12 (three four-wave blocks)


def _seq(rng, n):
    return "".join(_BASES[int(x)] for x in rng.integers(0, 4, n))


def _indel(pos, del_len=0, ins_seq="", cand=1, type_="INDEL"):
    return dict(pos=pos, type=synth.INDEL[type_], del_len=del_len, ins_seq=ins_seq, is_candidate=int(cand))


def _read_over(sc, start, hap, rl, rng, lead=0, observed=None):
    """a read of up to rl bases that follows the reference from `start` through the table indels `hap` (indices, in position order);
    lead > 0: the read begins with the last `lead` bases of hap[0]'s insert sequence (a leading edge insert at `start`)"""
    off, ref, indels = sc["ref_offset"], sc["ref_seq"], sc["indels"]
    seq, path, p = [], [], start

    def push(t, ln):
        if ln > 0:
            path.append((t, ln))
    for n, i in enumerate(hap):
        d = indels[i]
        if n == 0 and lead:
            assert d["pos"] == start and not d["del_len"]
            seq += list(d["ins_seq"][-lead:])
            push(_I, lead)
            continue
        m = min(d["pos"] - p, rl - len(seq))
        assert m > 0
        seq += list(ref[p - off:p - off + m])
        push(_M, m)
        p += m
        if len(seq) >= rl:
            break
        push(_D, d["del_len"])
        p += d["del_len"]
        k = min(len(d["ins_seq"]), rl - len(seq))
        seq += list(d["ins_seq"][:k])
        push(_I, k)
    m = rl - len(seq)
    seq += list(ref[p - off:p - off + m])
    push(_M, m)
    while path[-1][0] == _D:
        path.pop()
    code = np.array([_CODE[c] for c in seq], np.uint8)
    return dict(code=code, qual=rng.integers(2, 41, len(code)).astype(np.uint8), pos=start, path=path, is_fwd=bool(rng.random() < 0.5),
                map_level=1, observed=list(hap) if observed is None else observed, realign_range=(max(0, off - 60), off + len(ref) + 60))


def _plain(sc, start, rl, rng, path=None):
    rd = _read_over(sc, start, [], rl, rng)
    if path is not None:
        rd["path"] = path
    return rd


def _crafted_ops(rng, lens):
    """ops of 1, 7, 8, 9 and 16 bases, penalties on either side of an 8-base op, soft clips, short reads, reads of the given lengths"""
    off = 1000
    sc = dict(ref_seq=_seq(rng, 460), ref_offset=off, is_haplotyping_enabled=0, min_read_bp_flank=1, kind="ops")
    a = off + 20
    sc["indels"] = [_indel(a + 8, 0, _seq(rng, 1)), _indel(a + 24, 0, _seq(rng, 7), cand=0), _indel(a + 33, 0, _seq(rng, 8)),
                    _indel(a + 41, 2, "", cand=0), _indel(a + 51, 3, "", cand=0), _indel(a + 70, 0, _seq(rng, 9), cand=0),
                    _indel(a + 78, 0, _seq(rng, 16))]
    hap = list(range(7))
    reads = [_read_over(sc, a, hap, rl, rng) for rl in lens]
    reads.append(_read_over(sc, a, hap, 120, rng))  # (ends with the 16 inserted bases and 8 matched ones)
    rl = lens[0]
    reads.append(_plain(sc, a + 5, rl, rng, [(_S, 5), (_M, rl - 5)]))
    reads.append(_plain(sc, a, rl, rng, [(_M, rl - 7), (_S, 7)]))
    for n in range(1, 10):  # reads of 1-9 bases across the first insert
        reads.append(_plain(sc, a + 8 - (n + 1) // 2, n, rng))
    for rd in reads[:len(lens)]:  # an N and a '=' among the last eight bases
        rd["code"][-3] = 15
        rd["code"][-6] = 0
    sc["reads"] = reads
    return sc


def _crafted_walk(rng, rl, which):
    """which = "eight": one read over eight indels, the outer two edge inserts; "seven": one over the leading edge insert and the six
    inner indels; "rest": a lead and a trail edge insert, a swap; a breakpoint entry; 40 table entries before every read (a table over 32 entries, tab_lo > 0); an insert entry
    that lies in no read's window"""
    off = 1000
    sc = dict(ref_seq=_seq(rng, 1100), ref_offset=off, is_haplotyping_enabled=0, min_read_bp_flank=1, kind="walk")
    far = [_indel(off + 20 + 11 * k, 1 + k % 3) for k in range(39)] + [_indel(off + 455, 0, _seq(rng, 5))]
    a = off + 640
    lead_ins, trail_ins = _seq(rng, 6), _seq(rng, 12)
    step = (rl - 30) // 7
    near = [_indel(a, 0, lead_ins)] + [_indel(a + step * (k + 1), 1 + k % 2, "", cand=k == 3) for k in range(6)]
    near.append(_indel(a + step * 7 + 9, 0, trail_ins))
    # (the eight-indel alignment has 15 of the record's 16 segments: what the search may add to it is no candidate)
    near.append(_indel(a + step * 2 + 7, 2, _seq(rng, 3), cand=0))             # a delete + insert entry: a swap in the path
    near.append(_indel(a + step * 3 + 5, 0, "", cand=0, type_="BP_RIGHT"))       # a breakpoint-typed entry among the reads'
    sc["indels"] = far + near
    n0 = len(far)
    eight = list(range(n0, n0 + 8))
    reads = [_read_over(sc, a, eight, rl, rng, lead=4),
             _read_over(sc, a, eight[:4], rl - 20, rng, lead=6),
             _read_over(sc, a + 3, [n0 + 1, n0 + 8, n0 + 3], rl - 10, rng),       # through the swap
             _read_over(sc, a + 3, eight[1:7], rl - 25, rng),
             _read_over(sc, a + step + 4, eight[2:8], 6 * step + 2, rng)]          # ends five bases into the trailing insert
    if which == "eight":
        sc["reads"] = [reads[0]]
    elif which == "seven":
        sc["reads"] = [_read_over(sc, a, eight[:7], rl - 12, rng, lead=4)]
    else:
        sc["reads"] = reads[1:] + [_plain(sc, a + 10, 60, rng), _plain(sc, a + 2 * step, rl - 40, rng)]
    sc["kind"] = "walk_" + which
    return sc


def _decorate(sc, rng):
    """as tests/test_f5_phase_b_cases.py: inserts of every length 1-9 and 16, some of them not candidates; '=' and N bases"""
    off, ref = sc["ref_offset"], sc["ref_seq"]
    used = {(d["pos"], d["del_len"], d["ins_seq"]) for d in sc["indels"]}
    for ln in list(range(1, 10)) + [16]:
        p = off + int(rng.integers(20, len(ref) - 20))
        seq = _seq(rng, ln)
        if (p, 0, seq) not in used:
            used.add((p, 0, seq))
            sc["indels"].append(_indel(p, 0, seq, cand=rng.random() < 0.5))
    for rd in sc["reads"]:
        code = rd["code"].copy()
        code[rng.random(len(code)) < 0.03] = 0
        code[rng.random(len(code)) < 0.02] = 15
        rd["code"] = code
    sc["kind"] = "random"
    return sc


def _scenarios(seed, form):
    rng = np.random.default_rng(seed)
    read_len, window, lens = ((30, 153), (200, 360), (150, 151, 152)) if form == 152 else ((153, 257), (330, 430), (153, 256))
    scs = [_decorate(sc, rng) for sc in synth.realign_scenarios(8, rng, reads_per=10, max_indels=8, min_indels=4, read_len=read_len,
                                                              window=window, haplotyping_rate=0.2)]
    return scs + [_crafted_ops(rng, lens), _crafted_walk(rng, lens[0], "eight"), _crafted_walk(rng, lens[0], "seven"),
                  _crafted_walk(rng, lens[0], "rest"), _crafted_walk(rng, lens[-1], "rest")]


def _count_cases(sc, seen, pools):
    """the cases of one job, from the host form's batch of it (no device work), its reads and its table"""
    job = U.make_job(sc, 0)
    idx = U.add_reads(job, sc["reads"])
    b = job.batch()
    kept = [rd for rd, i in zip(sc["reads"], idx) if i is not None]
    # (the batch holds the reads that passed the gate, in order: each is found among the job's reads by its codes)
    in_batch, at = [], 0
    for r in range(b.n_reads):
        code = b.read_code[int(b.read_off[r]):int(b.read_off[r + 1])]
        while not np.array_equal(kept[at]["code"], code):
            at += 1
        in_batch.append(kept[at])
        at += 1
    for r, rd in enumerate(in_batch):
        c0, c1 = int(b.cal_off[r]), int(b.cal_off[r + 1])
        if c1 == c0:
            continue
        L = len(rd["code"])
        pool = int(b.hap_off[r + 1] - b.hap_off[r])
        pools.append(pool)
        seen["read_len_%d" % L] = seen.get("read_len_%d" % L, 0) + 1
        seen["read_1_to_9"] += 1 <= L <= 9
        seen["N_in_last_8"] += bool((rd["code"][-8:] == 15).any())
        seen["eq_in_last_8"] += bool((rd["code"][-8:] == 0).any())
        for c in range(c0, c1):
            ops = b.ops[int(b.op_off[c]):int(b.op_off[c + 1])]
            kind, ln, flags, src = ops["kind"], ops["length"], ops["flags"], ops["src"]
            bases = kind == capi.OP_BASES
            for n in (1, 7, 8, 9, 16):
                seen["op_of_%d" % n] += bool((bases & (ln == n)).any())
            if bases.any():
                last = int(np.nonzero(bases)[0][-1])
                seen["last_op_multiple_of_8"] += ln[last] % 8 == 0
                seen["ends_at_pool_end"] += int(src[last]) + int(ln[last]) == pool
            for i in np.nonzero(bases & (ln == 8))[0]:
                seen["penalty_before_8"] += bool(i > 0 and flags[i - 1] & 1)
                seen["penalty_after_8"] += bool(flags[i] & 1 or (i + 1 < len(ops) and kind[i + 1] == capi.OP_NOBASE and flags[i + 1] & 1))
        types = [t for t, _ in rd["path"]]
        n_ind = sum(t in (_I, _D) for t in types)
        seen["seven_indels"] += n_ind == 7 and len(rd["observed"]) == 7
        seen["lead_clip"] += types[0] == _S    # (of the input alignment: see the module's docstring)
        seen["trail_clip"] += types[-1] == _S
        seen["lead_edge"] += types[0] == _I
        seen["trail_edge"] += types[-1] == _I
        seen["swap"] += any(x == _D and y == _I for x, y in zip(types, types[1:]))
    lo = min(rd["pos"] for rd in kept)
    hi = max(rd["pos"] + sum(n for t, n in rd["path"] if t in (_M, _D)) for rd in kept)
    seen["breakpoint_entry"] += any(d["type"] != synth.INDEL["INDEL"] and lo <= d["pos"] <= hi for d in sc["indels"])
    seen["table_over_32_tab_lo"] += sum(d["pos"] < lo - 100 for d in sc["indels"]) > _TAB
    seen["insert_in_no_pool"] += any(d["ins_seq"] and (d["pos"] < lo - 150 or d["pos"] > hi + 150) for d in sc["indels"])


_NEEDED = ("op_of_1", "op_of_7", "op_of_8", "op_of_9", "op_of_16", "last_op_multiple_of_8", "read_1_to_9", "lead_clip", "trail_clip",
           "penalty_before_8", "penalty_after_8", "N_in_last_8", "eq_in_last_8", "ends_at_pool_end", "seven_indels", "lead_edge",
           "trail_edge", "swap", "breakpoint_entry", "table_over_32_tab_lo", "insert_in_no_pool")


@pytest.mark.gpu
@pytest.mark.parametrize("seed,form", [(97301, 152), (97302, 256)])
def test_f5_turn_ahead_equals_staged_and_host(seed, form, monkeypatch):
    capi.init(0)
    scs = _scenarios(seed, form)
    seen = dict.fromkeys(_NEEDED, 0)
    pools, pools_all, n_f5_jobs = [], [], 0
    for sc in scs:
        out = {chain: U.run_chain(sc, chain, setenv=monkeypatch.setenv) for chain in ("host", "staged", "f5")}
        out["again"] = U.run_chain(sc, "f5", setenv=monkeypatch.setenv)
        f5 = out["f5"]
        print(sc["kind"], "jobs", f5["jobs"], "outside", [out[c]["outside"] for c in out], "consulted", sum(f5["consulted"]), "of",
              len(sc["indels"]))
        for chain in ("staged", "f5", "again"):
            assert out[chain]["res"] == out["host"]["res"], (sc["kind"], chain)
            assert out[chain]["consulted"] == out["host"]["consulted"], (sc["kind"], chain)
            assert out[chain]["outside"] == out["host"]["outside"], (sc["kind"], chain)
        _count_cases(sc, dict.fromkeys(_NEEDED, 0), pools_all)
        if f5["counts"][1] > 0 and f5["jobs"] == (1, 0, 0):  # F5 scored the job itself
            assert out["again"]["jobs"] == (1, 0, 0)
            n_f5_jobs += 1
            _count_cases(sc, seen, pools)
    lens = (150, 151, 152) if form == 152 else (153, 256)
    print("jobs", len(scs), "scored by F5", n_f5_jobs, "cases", seen, "largest pool", max(pools), "of all jobs", max(pools_all))
    assert n_f5_jobs >= len(scs) - 2
    assert all(seen[k] > 0 for k in _NEEDED), {k: seen[k] for k in _NEEDED}
    assert all(seen.get("read_len_%d" % n, 0) > 0 for n in lens), seen
    assert max(pools) == max(pools_all)   # the largest pool of the scenarios is one F5 scored


def _queue_scenario(rng, long_read):
    """a few distinct short reads over one or two indels (and one that is far from every indel: the gate turns it down); long_read: one
    of them of 160 bases, so that the job takes the 256-base form"""
    off = 1000
    sc = dict(ref_seq=_seq(rng, 700), ref_offset=off, is_haplotyping_enabled=0, min_read_bp_flank=1, kind="queue")
    a = off + 200
    sc["indels"] = [_indel(a + 14, 2), _indel(a + 25, 0, _seq(rng, 3)), _indel(a + 60, 1, "", cand=0)]
    reads = [_read_over(sc, a, [0], 34, rng), _read_over(sc, a + 2, [0, 1], 38, rng), _read_over(sc, a + 18, [1], 30, rng),
             _plain(sc, off + 520, 32, rng),                                    # no indel near it: no candidate alignments
             _read_over(sc, a + 5, [0, 1], 40, rng, observed=[]), _read_over(sc, a + 40, [2], 36, rng),
             _plain(sc, a + 4, 33, rng)]
    if long_read:
        reads[4] = _read_over(sc, a - 60, [0, 1, 2], 160, rng)
    sc["reads"] = reads
    return sc


def _queue_cases():
    out = []
    for form in (152, 256):
        w = _W[form]
        for n in ((1, 7, 8, 9, w - 1, w, w + 1, 2 * w + 5) if form == 152 else (w - 1, w, w + 1, 2 * w + 5)):
            out.append((form, n))
    return out


_queue_reference = {}


def _queue_ref(form, monkeypatch):
    """host and staged results of the distinct reads, once per form"""
    if form not in _queue_reference:
        sc = _queue_scenario(np.random.default_rng(97400 + form), form == 256)
        host, staged = (U.run_chain(sc, chain, setenv=monkeypatch.setenv) for chain in ("host", "staged"))
        assert staged["res"] == host["res"] and staged["consulted"] == host["consulted"] and staged["outside"] == host["outside"] == 0
        assert all(r is not None for r in host["res"])
        n_cals = [eval(r, {"nan": float("nan"), "inf": float("inf")})["n_cals"] for r in host["res"]]
        assert min(n_cals) == 0 and sum(c > 0 for c in n_cals) >= 5   # one read leaves at the gate, the others are scored
        _queue_reference[form] = (sc, host)
    return _queue_reference[form]


@pytest.mark.gpu
@pytest.mark.parametrize("form,n", _queue_cases())
def test_f5_queue_first_read_not_drawn(form, n, monkeypatch):
    capi.init(0)
    sc, host = _queue_ref(form, monkeypatch)
    k = len(sc["reads"])
    reads = [sc["reads"][i % k] for i in range(n)]
    want = [host["res"][i % k] for i in range(n)]
    f5 = U.run_chain(sc, "f5", reads, setenv=monkeypatch.setenv)
    again = U.run_chain(sc, "f5", reads, rescore=2, setenv=monkeypatch.setenv)
    print("form", form, "reads", n, "jobs", f5["jobs"], again["jobs"], "counts", f5["counts"])
    if f5["counts"][1] > 0:   # (a job of reads the gate turns down alone has nothing for the device)
        assert f5["jobs"] == (1, 0, 0) and again["jobs"] == (1, 0, 0)
    else:
        assert n < 4
    for got in (f5, again):
        assert got["res"] == want
        assert got["outside"] == 0
        if n >= k:   # (every distinct read is among them)
            assert got["consulted"] == host["consulted"]
