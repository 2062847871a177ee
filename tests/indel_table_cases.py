"""Inputs of the indel-table tests, shared by the model tests (tests/test_indel_table_model.py) and the device tests
(tests/test_indel_table.py): crafted observations and region records in the model's form, and their conversion to the arrays the chain's
entry points leave.  Imports neither a device nor the library (only the record layouts of strelka_amd.capi)."""
import numpy as np

from strelka_amd import capi
from tests import haplotype_model as H
from tests import indel_table_model as T
from tests import intake_model as M

REF_OFFSET = 100
REF = "".join(np.random.default_rng(777).choice(list("ACGT"), 300))  # 100..399
INDEL, MISMATCH, BP_LEFT, BP_RIGHT = T.INDEL, T.MISMATCH, T.BP_LEFT, T.BP_RIGHT


def obs(read, pos, otype=INDEL, del_len=0, ins=(0, 0), noise=0):
    """one sk_intake_obs in the model's form; ins: (begin, length) in the read's bases"""
    return dict(read=read, pos=pos, deletion_length=del_len, ins_begin=ins[0], ins_len=ins[1], bp_begin=0, bp_len=0, type=otype, is_noise=noise, is_low_mapq=0)


def sample(read_seqs, observations, iat=None, align_id=None, hap=(), alleles=()):
    """a sample in the model's form from read strings and observations (sorted here by read: the intake's order)"""
    reads = [dict(code=M.encode(s), pos=0, path=[(M.MATCH, len(s))]) for s in read_seqs]
    return dict(reads=reads, obs=sorted(observations, key=lambda o: o["read"]), align_id=align_id, iat=list(iat) if iat is not None else [0] * len(reads), hap=list(hap),
                alleles=list(alleles))


def hap_rec(status=H.COUNTED, supports=(), n_reads_aligned=None, reason=0):
    """a region's haplotype record in the model's form; supports: the selected haplotypes' support lists (the first is taken as the reference)"""
    n = sum(len(s) for s in supports) if n_reads_aligned is None else n_reads_aligned
    return dict(status=status, reason=reason, n_reads_aligned=n, n_reads_covering=n,
                haps=[dict(seq="ACGT"[:1 + k], support=list(s), is_reference=int(k == 0), count=len(s)) for k, s in enumerate(supports)])


def allele(pos, atype=INDEL, del_len=0, ins="", hap_slot=1, haplotype_id=1, ratio=0.5, to_indel_buffer=1):
    return dict(pos=pos, type=atype, del_len=del_len, ins=ins, hap_slot=hap_slot, haplotype_id=haplotype_id, ratio=T.float_bits(np.float32(ratio)),
                to_indel_buffer=to_indel_buffer, same_as=-1, id_sum=0, ratio_sum=0)


def allele_rec(alleles=(), status=H.COUNTED, reason=0, prev_end=-1):
    return dict(status=status, reason=reason, prev_end=prev_end, n_alt=1 if alleles else 0, alleles=list(alleles))


def obs_arrays(sample_):
    """the model's observations -> (obs_off, INTAKE_OBS_DTYPE[]) as sk_read_intake leaves them"""
    n = len(sample_["reads"])
    obs_off = np.zeros(n + 1, np.int64)
    arr = np.zeros(len(sample_["obs"]), capi.INTAKE_OBS_DTYPE)
    for k, o in enumerate(sample_["obs"]):
        assert k == 0 or int(o["read"]) >= int(sample_["obs"][k - 1]["read"])
        for f in ("read", "pos", "deletion_length", "ins_begin", "ins_len", "bp_begin", "bp_len", "type", "is_noise", "is_low_mapq"):
            arr[k][f] = o[f]
        obs_off[int(o["read"]) + 1:] += 1
    return obs_off, arr


def raw_records(hap, alleles):
    """the model's region records -> (what sk_region_haplotypes leaves: recs, support_pool; what sk_region_alleles leaves: recs, alleles,
    insert_pool) -- the fields sk_indel_table reads"""
    n = len(hap)
    hrecs = np.zeros(n, capi.REGION_HAPLOTYPES_DTYPE)
    support = []
    for i, h in enumerate(hap):
        hrecs[i]["status"], hrecs[i]["reason"], hrecs[i]["n_reads_aligned"], hrecs[i]["n_reads_covering"] = h["status"], h["reason"], h["n_reads_aligned"], h["n_reads_covering"]
        hrecs[i]["n_selected"] = len(h["haps"])
        for k, x in enumerate(h["haps"]):
            hrecs[i]["hap"][k] = (0, len(support), len(x["seq"]), len(x["support"]), x["is_reference"], 0)
            support += list(x["support"])
    arecs = np.zeros(n, capi.REGION_ALLELES_DTYPE)
    flat, ins = [], bytearray()
    for i, r in enumerate(alleles):
        arecs[i]["status"], arecs[i]["reason"], arecs[i]["prev_end"], arecs[i]["n_alt"], arecs[i]["n_alleles"] = r["status"], r["reason"], r["prev_end"], r["n_alt"], len(r["alleles"])
        arecs[i]["allele_off"], arecs[i]["insert_off"] = len(flat), len(ins)
        for a in r["alleles"]:
            flat.append((a["pos"], a["type"], a["del_len"], len(a["ins"]), len(ins), a["hap_slot"], a["haplotype_id"], T.bits_float(a["ratio"]), a["to_indel_buffer"],
                         a["same_as"], a["id_sum"], T.bits_float(a["ratio_sum"]), 0))
            ins += a["ins"].encode("latin-1")
        arecs[i]["n_insert_bytes"] = len(ins) - int(arecs[i]["insert_off"])
    al = np.zeros(len(flat), capi.REGION_ALLELE_DTYPE)
    for k, a in enumerate(flat):
        al[k] = a
    return (dict(recs=hrecs, support_pool=np.array(support, np.int32)), dict(recs=arecs, alleles=al, insert_pool=np.frombuffer(bytes(ins), np.uint8).copy()))


def device_sample(sample_):
    """a sample in the model's form -> the dict strelka_amd.capi.indel_table takes"""
    obs_off, arr = obs_arrays(sample_)
    haplotypes, alleles = raw_records(sample_["hap"], sample_["alleles"])
    return dict(reads=sample_["reads"], intake=dict(obs_off=obs_off, obs=arr), align_id=sample_.get("align_id"), iat=sample_["iat"], haplotypes=haplotypes, alleles=alleles)


def deletions_case(n_reads, pos=210, del_len=2, iat=None, align_id=None):
    """n_reads reads of one sample that each saw the same deletion"""
    return sample(["ACGTACGT"] * n_reads, [obs(r, pos, del_len=del_len) for r in range(n_reads)], iat=iat, align_id=align_id)
