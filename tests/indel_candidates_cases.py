"""Inputs of the indel-candidacy tests, shared by the model tests (tests/test_indel_candidates_model.py) and the device tests
(tests/test_indel_candidates.py): crafted table records, rate sets and options in the model's form, and their conversion to the arrays the
entry points take.  Imports neither a device nor the library (only the record layouts of strelka_amd.capi)."""
import numpy as np

from strelka_amd import capi
from tests import indel_candidates_model as CM

INDEL, MISMATCH, BP_LEFT, BP_RIGHT = CM.INDEL, CM.MISMATCH, CM.BP_LEFT, CM.BP_RIGHT
M, I, D, S, SKIP = CM.SEG_MATCH, CM.SEG_INSERT, CM.SEG_DELETE, CM.SEG_SOFT_CLIP, CM.SEG_SKIP

# gamma_p_inv(k, 1e-9) to a few digits: ascending, of the reference's magnitudes (the tests need no more of it; the recorded scenes carry
# the reference's own bits)
PAPPROX = [1e-9, 4.47e-5, 1.82e-3, 1.25e-2, 4.16e-2, 9.6e-2, 0.179, 0.292, 0.433, 0.602, 0.797, 1.017, 1.259, 1.522, 1.806, 2.107, 2.426, 2.76]


def ramp(n_counts=16, lo=5e-5, hi=3e-4):
    """a log-linear ramp like the candidate set: one pattern size"""
    return [[(lo * (hi / lo) ** (k / max(n_counts - 1, 1)),) * 2 for k in range(n_counts)]]


def flat(rate, n_sizes=1, n_counts=1):
    return [[(rate, rate)] * n_counts for _ in range(n_sizes)]


def options(**fields):
    return CM.default_options(**dict(dict(papprox=list(PAPPROX)), **fields))


def key(pos, ktype=INDEL, del_len=0, ins="", n1=(0,), flags=0, active_region_id=-1, n_bp_obs=0, unit=0, ref_count=0, indel_count=0):
    """a table record in the model's form; n1: per sample the number of tier-1 ids"""
    if ktype == INDEL and not ((del_len > 0) != (len(ins) > 0)):
        flags |= CM.DO_NOT_GENOTYPE  # (what the table gives a key that is not primitive)
    return dict(pos=pos, type=ktype, del_len=del_len, ins=ins, active_region_id=active_region_id, flags=flags, n_bp_obs=n_bp_obs, it=0, repeat_unit_len=unit,
                ref_repeat_count=ref_count, indel_repeat_count=indel_count, interrupted_hpol_len=0,
                samples=[dict(ids=[list(range(n)), [], [], []], haplotype_id=0, is_haplotyping_bypassed=0, ratio=0) for n in n1])


def bp_obs(pos, ktype, bp_len):
    return dict(read=0, pos=pos, deletion_length=0, ins_begin=0, ins_len=0, bp_begin=0, bp_len=bp_len, type=ktype, is_noise=0, is_low_mapq=0)


def sorted_keys(keys):
    return sorted(keys, key=lambda k: (k["pos"], k["type"], len(k["ins"]), k["del_len"], k["ins"].encode("latin-1")))


def ratio_exactly_one_hundredth():
    """a double p with p / (1 - p) == 0.01 exactly: isPoissonApprox's <= at equality"""
    p = 0.01 / 1.01
    for _ in range(64):
        if p / (1 - p) == 0.01:
            return p
        p = np.nextafter(p, 1.0 if p / (1 - p) < 0.01 else 0.0)
    raise AssertionError("no double gives the ratio exactly")


def read(pos, path):
    return dict(pos=pos, path=list(path))


# ---- to the arrays of the entry points
def table_arrays(keys):
    """model records -> (INDEL_TABLE_KEY_DTYPE[], INDEL_TABLE_SAMPLE_DATA_DTYPE[n_keys * n_samples]): the fields sk_indel_candidates reads"""
    n_samples = len(keys[0]["samples"]) if keys else 1
    ka = np.zeros(len(keys), capi.INDEL_TABLE_KEY_DTYPE)
    da = np.zeros(len(keys) * n_samples, capi.INDEL_TABLE_SAMPLE_DATA_DTYPE)
    at = 0
    for i, k in enumerate(keys):
        ka[i]["pos"], ka[i]["type"], ka[i]["del_len"], ka[i]["ins_len"], ka[i]["active_region_id"], ka[i]["flags"] = k["pos"], k["type"], k["del_len"], len(k["ins"]), k["active_region_id"], k["flags"]
        ka[i]["n_bp_obs"], ka[i]["it"], ka[i]["repeat_unit_len"], ka[i]["ref_repeat_count"], ka[i]["indel_repeat_count"] = k["n_bp_obs"], k["it"], k["repeat_unit_len"], k["ref_repeat_count"], k["indel_repeat_count"]
        for s, d in enumerate(k["samples"]):
            for c in range(4):
                da[i * n_samples + s]["off"][c] = at
                da[i * n_samples + s]["count"][c] = len(d["ids"][c])
                at += len(d["ids"][c])
    return ka, da


def rate_set_arrays(rate_sets):
    return np.array([capi.pack_rate_set(rs) for rs in rate_sets], capi.INDEL_RATE_SET_DTYPE)


def obs_arrays(sample_obs):
    """per sample [observation dicts] -> [(n_reads, obs_off, INTAKE_OBS_DTYPE[])]: every observation hangs on read 0"""
    out = []
    for obs in sample_obs:
        arr = np.zeros(len(obs), capi.INTAKE_OBS_DTYPE)
        for j, o in enumerate(obs):
            for f in ("read", "pos", "deletion_length", "ins_begin", "ins_len", "bp_begin", "bp_len", "type", "is_noise", "is_low_mapq"):
                arr[j][f] = o[f]
        out.append((1, np.array([0, len(obs)], np.int64), arr))
    return out


def capi_options(opt):
    return capi.indel_candidate_options(**opt)


def device_results(res, n_samples):
    """what sk_indel_candidates leaves -> the model's form"""
    out = []
    bits = np.ascontiguousarray(res["rates"]).view(np.uint64).reshape(-1, 4)
    for i, o in enumerate(res["out"]):
        assert int(o["pad"]) == 0
        out.append(dict(is_candidate=int(o["is_candidate"]), undecided=int(o["undecided"]), bp_insert_size=int(o["bp_insert_size"]),
                        rates=[[int(x) for x in row] for row in bits[i * n_samples:(i + 1) * n_samples]]))
    return out
