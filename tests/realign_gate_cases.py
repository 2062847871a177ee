"""Inputs of the realignment-gate tests, shared by the model tests (tests/test_realign_gate_model.py) and the device tests
(tests/test_realign_gate.py, tests/test_realign_gate_job.py): crafted tables, candidacy records and reads in the model's form, and their
conversion to and from the arrays of the entry points.  Imports neither a device nor the library (only the record layouts of
strelka_amd.capi)."""
import numpy as np

from strelka_amd import capi
from tests import indel_candidates_cases as K
from tests import indel_candidates_model as CM
from tests import realign_gate_model as GM

M, I, D, S, H, SKIP = CM.SEG_MATCH, CM.SEG_INSERT, CM.SEG_DELETE, CM.SEG_SOFT_CLIP, CM.SEG_HARD_CLIP, CM.SEG_SKIP
WIDE = (0, 1 << 30)


def key(pos, ktype=CM.INDEL, del_len=0, ins="", ids=None, n_samples=1, active_region_id=-1, haplotype_id=0, bypassed=0, flags=0):
    """a table record in the model's form; ids: per sample [tier1, tier2, submap, noise] lists of align ids (None: all empty)"""
    k = K.key(pos, ktype, del_len, ins, n1=(0,) * n_samples, flags=flags, active_region_id=active_region_id)
    for s, d in enumerate(k["samples"]):
        d["ids"] = [sorted(x) for x in ids[s]] if ids else [[], [], [], []]
        d["haplotype_id"] = haplotype_id[s] if isinstance(haplotype_id, (list, tuple)) else haplotype_id
        d["is_haplotyping_bypassed"] = bypassed[s] if isinstance(bypassed, (list, tuple)) else bypassed
    return k


def cand(is_candidate=0, undecided=CM.DECIDED, rates=(1e-4, 2e-4, 5e-5, 5e-5), n_samples=1):
    """a candidacy record in the model's form; rates: the four doubles of every sample, or one tuple per sample"""
    rows = [rates] * n_samples if not isinstance(rates[0], (list, tuple)) else list(rates)
    return dict(is_candidate=int(is_candidate), undecided=int(undecided), bp_insert_size=0, rates=[[CM.double_bits(x) for x in r] for r in rows])


def read(pos, path, realign=WIDE, read_len=None):
    path = [(int(t), int(n)) for t, n in path]
    return dict(pos=pos, path=path, realign=tuple(realign), read_len=sum(n for t, n in path if t in GM.READ_LENGTH) if read_len is None else read_len)


# ---- to the arrays of the entry points
def table_arrays(keys):
    """model records -> (INDEL_TABLE_KEY_DTYPE[], INDEL_TABLE_SAMPLE_DATA_DTYPE[n_keys * n_samples], id_pool, insert_pool) laid out as sk_indel_table
    leaves them: the id sets tile the pool in (key, sample, set) order"""
    n_samples = len(keys[0]["samples"]) if keys else 1
    ka, da = K.table_arrays(keys)
    ids, ins = [], b""
    for i, k in enumerate(keys):
        ka[i]["ins_off"] = len(ins)
        ins += k["ins"].encode("latin-1")
        for s, d in enumerate(k["samples"]):
            da[i * n_samples + s]["haplotype_id"], da[i * n_samples + s]["is_haplotyping_bypassed"] = d["haplotype_id"], d["is_haplotyping_bypassed"]
            for c in range(4):
                assert int(da[i * n_samples + s]["off"][c]) == len(ids)
                ids += d["ids"][c]
    return ka, da, np.array(ids, np.uint32), np.frombuffer(ins, np.uint8)


def cand_arrays(cand_records):
    """model candidacy records -> (INDEL_CANDIDATE_DTYPE[], INDEL_ERROR_RATES_DTYPE[n_keys * n_samples])"""
    out = np.zeros(len(cand_records), capi.INDEL_CANDIDATE_DTYPE)
    bits = []
    for i, c in enumerate(cand_records):
        out[i]["is_candidate"], out[i]["undecided"], out[i]["bp_insert_size"] = c["is_candidate"], c["undecided"], c["bp_insert_size"]
        bits += [b for row in c["rates"] for b in row]
    return out, np.array(bits, np.uint64).view(capi.INDEL_ERROR_RATES_DTYPE)


def packed_samples(samples):
    return [capi.pack_gate_sample(sm["reads"], sm.get("align_id")) for sm in samples]


def device_results(res, n_samples, insert_pool, slack=0):
    """what sk_realign_gate leaves (capi.realign_gate's result, `slack` canary elements behind every array) -> the model's form; the canaries and
    the padding are checked on the way"""
    def body(a, n):
        assert len(a) == n + slack and (a[n:].view(np.uint8) == 0x5a).all()  # nothing behind the array is written
        return a[:n]
    nk = len(res["keys"]) - slack
    keys = []
    logs = body(res["logs"], nk * n_samples).view(np.uint64).reshape(-1, 2)
    for k, o in enumerate(body(res["keys"], nk)):
        assert int(o["pad"]) == 0
        io, il = int(o["ins_off"]), int(o["ins_len"])
        keys.append(dict(pos=int(o["pos"]), type=int(o["type"]), del_len=int(o["del_len"]), ins=bytes(insert_pool[io:io + il]).decode("latin-1"),
                         active_region_id=int(o["active_region_id"]), is_candidate=int(o["is_candidate"]), undecided=int(o["undecided"]), gate_consulted=int(o["gate_consulted"]),
                         haplotype_id=[int(x) for x in o["haplotype_id"]], is_haplotyping_bypassed=[int(x) for x in o["is_haplotyping_bypassed"]],
                         logs=[[int(x) for x in row] for row in logs[k * n_samples:(k + 1) * n_samples]]))
    samples = []
    for s, so in enumerate(res["samples"]):
        n = len(so["reads"]) - slack
        reads = body(so["reads"], n)
        off = [int(x) for x in body(so["observed_off"], n + 1)]
        observed = so["observed"]
        assert (observed[len(observed) - slack:].view(np.uint8) == 0x5a).all()
        assert off[0] == 0 and off[-1] == res["totals"][2 + s] and not observed[off[-1]:len(observed) - slack].any()  # the room past the lists stays zero
        assert all(int(r["pad"]) == 0 for r in reads)
        samples.append(dict(reads=[dict(zone=[int(r["zone_begin"]), int(r["zone_end"])], status=int(r["status"]), asked_undecided=int(r["asked_undecided"])) for r in reads],
                            observed=[[int(x) for x in observed[off[r]:off[r + 1]]] for r in range(n)]))
    return dict(keys=keys, samples=samples, totals=list(res["totals"]))


# ---- crafted cases
def keys_in_one_range(n_inside, first_candidate, n_before=3, undecided_at=()):
    """one read whose zone holds n_inside keys (three more end before it, inside the reach of max_indel_size: the range's right-end skip passes them); the key
    first_candidate of those inside is the first candidate (None: no candidate), every second key after it is one too; undecided_at: indices
    inside that are undecided -> (keys, cand, samples)"""
    keys = [key(990 + 2 * i, del_len=1) for i in range(n_before)] + [key(1001 + i, del_len=1) if i % 3 else key(1001 + i, ins="AC"[:1 + i % 2]) for i in range(n_inside)]
    cands = [cand(1)] * n_before
    for i in range(n_inside):
        is_cand = first_candidate is not None and (i == first_candidate or (i > first_candidate and i % 2 == 0))
        cands.append(cand(0, CM.UNDECIDED_AR_PENDING + i % 3) if i in undecided_at else cand(is_cand))
    keys = K.sorted_keys(keys)
    return keys, cands, [dict(reads=[read(1000, [(M, n_inside + 2)])], align_id=None)]


def random_case(n_keys, n_samples, n_reads, seed, gaps=False):
    """keys of every kind, candidacy of every kind, reads with clips, insertions, deletions (some over the maximum, some spliced), ranges mostly wide,
    id sets drawn from the reads' ids with a read now and then in the noise set and a support set of one key -> (keys, cand, samples, max_indel_size)"""
    rng = np.random.default_rng(seed)
    max_indel_size = 30
    samples = []
    for s in range(n_samples):
        reads = []
        for r in range(n_reads):
            p = int(rng.integers(0, 400))
            a, b, c = (int(x) for x in rng.integers(1, 40, 3))
            kind = int(rng.integers(0, 9))
            path = [[(M, a + b)], [(M, a), (D, c), (M, b)], [(M, a), (I, c), (M, b)], [(S, c), (M, a), (D, 2), (CM.SEG_SEQ_MATCH, b), (S, 2)], [(I, c), (M, a)], [(M, a), (D, c)],
                    [(H, 3), (S, c), (M, a), (I, 31), (M, b), (H, 2)], [(M, a), (SKIP, 30), (M, b)], [(S, a), (I, b)]][kind]
            rl = None if rng.integers(0, 4) else sum(n for t, n in path if t in GM.READ_LENGTH) + int(rng.integers(0, 5))
            realign = WIDE if rng.integers(0, 5) else (p - int(rng.integers(0, 45)), p + a + b + int(rng.integers(0, 60)))
            reads.append(read(p, path, realign, rl))
        ids = sorted(int(x) for x in rng.choice(5 * n_reads + 7, n_reads, replace=False)) if gaps else None
        samples.append(dict(reads=reads, align_id=ids))
    keys, cands = [], []
    for i in range(n_keys):
        pos = int(rng.integers(0, 480))
        kind = i % 6
        ids = []
        for s in range(n_samples):
            pool = samples[s]["align_id"] if gaps else list(range(n_reads))
            sets = [sorted(int(x) for x in rng.choice(pool, min(len(pool), int(rng.integers(0, 4))), replace=False)) if pool else [] for _ in range(4)]
            if pool and rng.integers(0, 2):
                sets[3] = sorted(set(sets[3]) | set(sets[0][:1]) | set(sets[1][:1]))  # a noise observation plus haplotype support
            ids.append(sets)
        common = dict(ids=ids, n_samples=n_samples, active_region_id=int(rng.integers(-1, 3)) * 100, haplotype_id=[int(x) for x in rng.integers(0, 4, n_samples)],
                      bypassed=[int(x) for x in rng.integers(0, 2, n_samples)])
        if kind in (0, 1):
            keys.append(key(pos, del_len=int(rng.integers(1, 15)), **common))
        elif kind == 2:
            keys.append(key(pos, ins="ACGT"[:1 + i % 4], **common))
        elif kind == 3:
            keys.append(key(pos, CM.MISMATCH, 1, "G", **common))
        elif kind == 4:
            keys.append(key(pos, del_len=2, ins="TT", **common))
        else:
            keys.append(key(pos, CM.BP_LEFT if i % 2 else CM.BP_RIGHT, flags=CM.DO_NOT_GENOTYPE, **common))
    order = sorted(range(n_keys), key=lambda i: (keys[i]["pos"], keys[i]["type"], len(keys[i]["ins"]), keys[i]["del_len"], keys[i]["ins"].encode("latin-1")))
    keys = [keys[i] for i in order]
    seen, kept = set(), []
    for k in keys:  # (one record per key)
        ident = (k["pos"], k["type"]) if k["type"] in (CM.BP_LEFT, CM.BP_RIGHT) else (k["pos"], k["type"], k["del_len"], k["ins"])
        if ident not in seen:
            seen.add(ident)
            kept.append(k)
    for i, k in enumerate(kept):
        u = int(rng.integers(0, 20))
        rates = [tuple(float(x) for x in rng.uniform(0, 0.5, 4)) if rng.integers(0, 6) else (0.0, 0.5, 0.0, 1e-300) for _ in range(n_samples)]
        cands.append(cand(0, u, rates) if 1 <= u <= 3 else cand(int(rng.integers(0, 7) == 0), CM.DECIDED, rates))
    return kept, cands, samples, max_indel_size
