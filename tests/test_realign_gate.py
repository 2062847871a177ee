"""The realignment gate on the device (sk_realign_gate; csrc/realign_gate.hip): the shared key records, every log rate bit for bit, every
read's zone, status and asked_undecided, the consulted marks and the observed lists equal the loop model (tests/realign_gate_model.py,
itself pinned to vectors recorded from the reference by tests/test_realign_gate_model.py) -- through the host entry, the _dev entry, and
behind sk_indel_table_dev -> sk_read_depth_dev -> sk_indel_candidates_dev on one stream.

The shapes are the smallest at which the kernels can go wrong: 0 / 1 / 63 / 64 / 65 / 129 keys inside one read's range (the turns of 64),
the first candidate in lane 0, in lane 63 and in the second turn's lane 0, 0 / 1 / 65 reads, 1 and 8 samples, observed lists of 0 / 1 / 64 /
65 entries (one above SK_RGATE_SORT_CAP), align ids absent and ascending with gaps."""
import ctypes as C

import numpy as np
import pytest

from strelka_amd import capi
from tests import indel_candidates_cases as K
from tests import indel_candidates_model as CM
from tests import realign_gate_cases as G
from tests import realign_gate_model as GM

pytestmark = pytest.mark.gpu

SLACK = 3


def _host(keys, cands, samples, max_indel_size=49):
    """host entry against model -> the model's result"""
    capi.init(0)
    want = GM.realign_gate(keys, cands, samples, max_indel_size)
    ka, da, ids, ins = G.table_arrays(keys)
    ca, ra = G.cand_arrays(cands)
    res = capi.realign_gate(G.packed_samples(samples), ka, da, ids, ca, ra, max_indel_size, slack=SLACK)
    got = G.device_results(res, len(samples), ins, SLACK)
    _same(got, want)
    return want


def _same(got, want):
    assert len(got["keys"]) == len(want["keys"])
    for k, (g, w) in enumerate(zip(got["keys"], want["keys"])):
        assert g == w, k  # (zero bit mismatches on the log rates: they are compared as bit patterns)
    for s, (g, w) in enumerate(zip(got["samples"], want["samples"])):
        for r, (gr, wr) in enumerate(zip(g["reads"], w["reads"])):
            assert gr == wr, (s, r)
        assert len(g["reads"]) == len(w["reads"]) and g["observed"] == w["observed"], s
    assert got["totals"] == want["totals"]


def _dev(keys, cands, samples, max_indel_size=49, key_cap=None, id_cap=None, n_keys=None, n_ids=None, observed_cap=None, mutate=None):
    """sk_realign_gate_dev on uploaded arrays -> (capi.realign_gate's form over all of the rooms, canaries of SLACK elements behind every array, insert pool)"""
    import torch
    L = capi.lib()
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    n_samples = len(samples)
    ka, da, ids, ins = G.table_arrays(keys)
    ca, ra = G.cand_arrays(cands)
    key_cap = len(keys) + 2 if key_cap is None else key_cap
    id_cap = len(ids) + 5 if id_cap is None else id_cap
    packed = G.packed_samples(samples)
    if mutate:
        mutate(packed)
    pad = lambda a: np.concatenate([a, np.zeros(1, a.dtype)]).view(np.uint8)
    t = dict(keys=dev(pad(ka)), data=dev(pad(da)), ids=dev(pad(ids)), cand=dev(pad(ca)), rates=dev(pad(ra)),
             totals=dev(np.array([len(keys) if n_keys is None else n_keys, len(ids) if n_ids is None else n_ids, 0, 0], np.int64)))
    keep, ins_s, outs_s, outs = [], [], [], []
    cap = id_cap if observed_cap is None else observed_cap

    def room(n, itemsize):
        return torch.full(((max(n, 0) + SLACK) * itemsize,), 0x5a, dtype=torch.uint8, device="cuda")
    for p in packed:
        d = {f: dev(p[f].view(np.uint8)) for f in ("pos", "path_off", "n_seg", "path", "read_len", "realign_begin", "realign_end")}
        d["align_id"] = None if p["align_id"] is None else dev(p["align_id"].view(np.uint8))
        keep.append(d)
        ins_s.append(capi.realign_gate_sample_struct(dict(p, **d), ptr=lambda x: x.data_ptr()))
        o = dict(reads=room(p["n_reads"], 12), observed_off=room(p["n_reads"] + 1, 8), observed=room(cap, 4))
        outs.append(o)
        outs_s.append(capi.RealignGateSampleOut(o["reads"].data_ptr(), o["observed_off"].data_ptr(), o["observed"].data_ptr(), cap))
    arr_in = (capi.RealignGateSample * n_samples)(*ins_s)
    arr_out = (capi.RealignGateSampleOut * n_samples)(*outs_s)
    keys_out, logs = room(key_cap, 48), room(key_cap * n_samples, 16)
    totals = torch.full((2 + capi.MAX_SAMPLES,), -1, dtype=torch.int64, device="cuda")
    scratch_bytes = L.sk_realign_gate_scratch_bytes(n_samples, key_cap, id_cap)
    scratch = torch.full((scratch_bytes,), 0xa5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    capi._check(L.sk_realign_gate_dev(n_samples, C.addressof(arr_in), t["keys"].data_ptr(), t["data"].data_ptr(), t["ids"].data_ptr(), t["totals"].data_ptr(), key_cap, id_cap,
                                      t["cand"].data_ptr(), t["rates"].data_ptr(), max_indel_size, keys_out.data_ptr(), logs.data_ptr(), C.addressof(arr_out), totals.data_ptr(),
                                      scratch.data_ptr(), scratch_bytes, torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    res = dict(keys=keys_out.cpu().numpy().view(capi.REALIGN_GATE_KEY_DTYPE), logs=logs.cpu().numpy().view(capi.REALIGN_GATE_LOG_RATES_DTYPE), totals=totals.cpu().numpy().tolist(),
               samples=[dict(reads=o["reads"].cpu().numpy().view(capi.REALIGN_GATE_READ_DTYPE), observed_off=o["observed_off"].cpu().numpy().view(np.int64),
                             observed=o["observed"].cpu().numpy().view(np.int32)) for o in outs])
    return res, ins


def _dev_same(keys, cands, samples, want, max_indel_size=49, **kw):
    """the _dev entry against the model's result; the records past the key count are zero"""
    if capi.lib().sk_broker_client():
        return
    res, ins = _dev(keys, cands, samples, max_indel_size, **kw)
    capi._check(capi.lib().sk_check_device_errors())
    nk, ns = len(keys), len(samples)
    key_cap = len(res["keys"]) - SLACK
    assert not res["keys"][nk:key_cap].view(np.uint8).any() and not res["logs"][nk * ns:key_cap * ns].view(np.uint8).any()
    cut = dict(res, keys=np.concatenate([res["keys"][:nk], res["keys"][key_cap:]]), logs=np.concatenate([res["logs"][:nk * ns], res["logs"][key_cap * ns:]]))
    _same(G.device_results(cut, ns, ins, SLACK), want)


@pytest.mark.parametrize("n_inside,first", [(0, None), (1, 0), (1, None), (63, 62), (64, 63), (64, None), (65, 64), (65, 0), (129, 63), (129, 64), (129, 128), (129, None)])
def test_keys_inside_one_range_and_the_first_candidate(n_inside, first):
    keys, cands, samples = G.keys_in_one_range(n_inside, first)
    want = _host(keys, cands, samples)
    rd = want["samples"][0]["reads"][0]
    assert rd["status"] == (GM.NO_CANDIDATE if first is None else GM.PASS)
    asked = [k["gate_consulted"] for k in want["keys"]]
    assert asked == [0] * 3 + [1] * (n_inside if first is None else first + 1) + [0] * (0 if first is None else n_inside - first - 1)  # up to the FIRST candidate and no further
    _dev_same(keys, cands, samples, want)


def test_every_undecided_reason_and_asked_undecided():
    for reason in (CM.UNDECIDED_AR_PENDING, CM.UNDECIDED_EXACT_BINOMIAL, CM.UNDECIDED_BP_OBS_ORDER):
        keys = [G.key(1001, del_len=1), G.key(1003, ins="A"), G.key(1005, del_len=2), G.key(1070, del_len=2)]
        reads = [G.read(1000, [(G.M, 10)]), G.read(1000, [(G.M, 4)]), G.read(1060, [(G.M, 20)]), G.read(1002, [(G.M, 6)])]
        samples = [dict(reads=reads, align_id=None)]
        # undecided, then a candidate: the read passes, and asked an undecided key on its way
        want = _host(keys, [G.cand(0), G.cand(0, reason), G.cand(1), G.cand(0)], samples)
        assert [(r["status"], r["asked_undecided"]) for r in want["samples"][0]["reads"]] == [(GM.PASS, 1), (GM.UNDECIDED, 1), (GM.NO_CANDIDATE, 0), (GM.PASS, 1)]
        assert [k["gate_consulted"] for k in want["keys"]] == [1, 1, 1, 1] and [k["undecided"] for k in want["keys"]] == [0, reason, 0, 0]
        _dev_same(keys, [G.cand(0), G.cand(0, reason), G.cand(1), G.cand(0)], samples, want)
        # a candidate before the undecided key: it is never asked
        want = _host(keys, [G.cand(1), G.cand(0, reason), G.cand(1), G.cand(0)], [dict(reads=reads[:3], align_id=None)])
        assert [k["gate_consulted"] for k in want["keys"]] == [1, 0, 0, 1] and want["totals"][:2] == [2, 0]
        # no decided candidate among the intersecting keys, one undecided: UNDECIDED
        want = _host(keys, [G.cand(0), G.cand(0, reason), G.cand(0), G.cand(0)], samples)
        assert [(r["status"], r["asked_undecided"]) for r in want["samples"][0]["reads"]] == [(GM.UNDECIDED, 1), (GM.UNDECIDED, 1), (GM.NO_CANDIDATE, 0), (GM.UNDECIDED, 1)]
        assert want["totals"][:2] == [0, 3]
        _dev_same(keys, [G.cand(0), G.cand(0, reason), G.cand(0), G.cand(0)], samples, want)


def test_zone_edges_the_clamp_and_the_cheap_tests():
    keys = [G.key(96, del_len=4), G.key(99, del_len=1), G.key(100, ins="A"), G.key(100, CM.MISMATCH, 1, "G"), G.key(119, del_len=1), G.key(120, CM.MISMATCH, 1, "T"), G.key(120, ins="C")]
    keys = K.sorted_keys(keys)
    one = lambda i: [G.cand(int(j == i)) for j in range(len(keys))]
    rd = [G.read(100, [(G.M, 20)])]  # zone [100, 120)
    status = lambda i, reads=rd, mis=49: _host(keys, one(i), [dict(reads=reads, align_id=None)], mis)["samples"][0]["reads"][0]["status"]
    where = {(k["pos"], k["type"], k["del_len"]): i for i, k in enumerate(keys)}
    assert status(where[(96, CM.INDEL, 4)]) == GM.NO_CANDIDATE        # right end == zone_begin: in the range, no breakpoint inside
    assert status(where[(99, CM.INDEL, 1)]) == GM.NO_CANDIDATE
    assert status(where[(100, CM.INDEL, 0)]) == GM.NO_CANDIDATE       # an insertion at zone_begin
    assert status(where[(100, CM.MISMATCH, 1)]) == GM.PASS            # a mismatch at zone_begin
    assert status(where[(119, CM.INDEL, 1)]) == GM.PASS
    assert status(where[(120, CM.MISMATCH, 1)]) == GM.NO_CANDIDATE    # pos == zone_end: not returned
    assert status(where[(120, CM.INDEL, 0)]) == GM.NO_CANDIDATE
    assert status(where[(96, CM.INDEL, 4)], [G.read(99, [(G.M, 21)])]) == GM.PASS  # the right breakpoint inside, the left before the zone
    # the zone: soft clips and edge insertions widen it, a short path is widened to the read length, the clamp at 0
    want = _host(keys, one(0), [dict(reads=[G.read(100, [(G.S, 5), (G.M, 20), (G.I, 2), (G.S, 3)]), G.read(100, [(G.H, 9), (G.M, 20), (G.D, 7), (G.M, 1)]),
                                            G.read(3, [(G.S, 10), (G.M, 5)]), G.read(100, [(G.M, 5), (G.I, 10), (G.M, 5)]), G.read(50, [(G.I, 4), (G.S, 2)], read_len=6),
                                            G.read(100, [], read_len=0)], align_id=None)])
    assert [r["zone"] for r in want["samples"][0]["reads"]] == [[95, 125], [100, 128], [0, 8], [90, 120], [44, 56], [100, 100]]
    # the realign range short by one position on either side
    tight = lambda b, e: status(where[(119, CM.INDEL, 1)], [G.read(100, [(G.M, 20)], realign=(b, e))])
    assert (tight(100, 120), tight(101, 120), tight(100, 119)) == (GM.PASS, GM.OUTSIDE_RANGE, GM.OUTSIDE_RANGE)
    # max_indel_size: interior segments only
    big = where[(119, CM.INDEL, 1)]
    assert status(big, [G.read(100, [(G.M, 10), (G.D, 8), (G.M, 10)])], 8) == GM.PASS and status(big, [G.read(100, [(G.M, 10), (G.D, 9), (G.M, 10)])], 8) == GM.OVERMAX
    assert status(big, [G.read(100, [(G.M, 10), (G.I, 9), (G.M, 10)])], 8) == GM.OVERMAX and status(big, [G.read(110, [(G.I, 9), (G.M, 10)])], 8) == GM.PASS
    assert status(big, [G.read(110, [(G.M, 10), (G.D, 9)])], 8) == GM.PASS
    assert status(big, [G.read(100, [(G.M, 10), (G.SKIP, 5), (G.M, 10)])]) == GM.SPLICED
    # a deletion as long as max_indel_size reaches back into the range; one longer is not looked for
    far = [G.key(80, del_len=25), G.key(79, del_len=26)]
    far = K.sorted_keys(far)
    for mis, want_status in ((20, GM.PASS), (19, GM.NO_CANDIDATE)):
        got = _host(far, [G.cand(0), G.cand(1)], [dict(reads=[G.read(100, [(G.M, 20)])], align_id=None)], mis)
        assert got["samples"][0]["reads"][0]["status"] == want_status


@pytest.mark.parametrize("n", [0, 1, 64, 65, 130])
def test_observed_lists_across_the_sort_cap(n):
    """read 1 sits in n keys (in the noise set, and for every third key in the tier-1 set too), read 0 in every fifth, read 2 in none"""
    assert capi.RGATE_SORT_CAP == GM.SORT_CAP == 64
    keys = [G.key(10 + i, del_len=1, ids=[[[7] if i % 3 == 0 else [], [2] if i % 5 == 0 else [], [], [2, 7] if i % 5 == 0 else [7]]]) for i in range(n)]
    keys.append(G.key(500, del_len=2))
    samples = [dict(reads=[G.read(0, [(G.M, 30)]), G.read(5, [(G.M, 30)]), G.read(9, [(G.M, 30)])], align_id=[2, 7, 11])]
    cands = [G.cand(i % 2) for i in range(len(keys))]
    want = _host(keys, cands, samples)
    assert want["samples"][0]["observed"] == [list(range(0, n, 5)), list(range(n)), []] and want["totals"][2] == n + len(range(0, n, 5))
    _dev_same(keys, cands, samples, want)


@pytest.mark.parametrize("gaps", [False, True])
@pytest.mark.parametrize("n_keys,n_samples,n_reads", [(0, 1, 5), (40, 1, 0), (40, 1, 1), (150, 1, 65), (150, 8, 65), (90, 8, 9)])
def test_random_tables_reads_and_samples(n_keys, n_samples, n_reads, gaps):
    keys, cands, samples, mis = G.random_case(n_keys, n_samples, n_reads, 131 * n_keys + 17 * n_samples + n_reads + gaps, gaps)
    want = _host(keys, cands, samples, mis)
    if n_keys >= 90 and n_reads >= 9:
        seen = {r["status"] for sm in want["samples"] for r in sm["reads"]}
        assert seen == {GM.PASS, GM.OVERMAX, GM.OUTSIDE_RANGE, GM.NO_CANDIDATE, GM.UNDECIDED, GM.SPLICED} or n_samples * n_reads < 8 * 65
        assert any(r["asked_undecided"] and r["status"] == GM.PASS for sm in want["samples"] for r in sm["reads"])
        assert 0 < sum(k["gate_consulted"] for k in want["keys"]) < len(keys) and want["totals"][2] > 0
        assert any(CM.bits_double(k["logs"][0][0]) == -np.inf for k in want["keys"])  # a rate of 0: the device library's -inf is the host's
    _dev_same(keys, cands, samples, want, mis)


def _bad_seg_type(packed):
    packed[0]["path"][1][0] = 10


def _path_outside(packed):
    packed[0]["n_seg"][packed[0]["n_reads"] - 1] += 1


def _negative_n_seg(packed):
    packed[0]["n_seg"][0] = -1


def _negative_read_len(packed):
    packed[0]["read_len"][1] = -1


def _descending_align_id(packed):
    packed[0]["align_id"][2] = packed[0]["align_id"][1]


def _unowned_id(packed):
    packed[0]["align_id"][1] += 1


REFUSED_READS = ((_bad_seg_type, "segment type"), (_path_outside, "outside path_cap"), (_negative_n_seg, "negative n_seg"), (_negative_read_len, "negative read_len"),
                 (_descending_align_id, "not strictly ascending"), (_unowned_id, "none of the sample's reads"))


def _refusal_case():
    keys = [G.key(10, del_len=1, ids=[[[2], [], [], [7]]]), G.key(14, ins="A", ids=[[[7, 11], [], [], []]])]
    samples = [dict(reads=[G.read(0, [(G.M, 12), (G.D, 1), (G.M, 8)]), G.read(5, [(G.M, 30)]), G.read(9, [(G.M, 30)])], align_id=[2, 7, 11])]
    return keys, [G.cand(1), G.cand(0)], samples


def test_refusals_of_the_host_entry():
    capi.init(0)
    keys, cands, samples = _refusal_case()
    ka, da, ids, ins = G.table_arrays(keys)
    ca, ra = G.cand_arrays(cands)

    def call(mutate=None, ka=ka, da=da, ids=ids, **kw):
        packed = G.packed_samples(samples)
        if mutate:
            mutate(packed)
        try:
            capi.realign_gate(packed, ka, da, ids, ca, ra, kw.pop("max_indel_size", 49), **kw)
        except capi.StrelkaAmdError as e:
            return str(e)
        return ""
    assert call() == ""
    for mutate, which in REFUSED_READS:
        msg = call(mutate)
        assert which in msg and msg.startswith("sk_realign_gate: "), (mutate.__name__, msg)
    assert "SK_MAX_SAMPLES" in call(n_samples=0) and "SK_MAX_SAMPLES" in call(n_samples=9)
    assert "negative size" in call(n_keys=-1) and "negative size" in call(n_ids=-1)
    assert "observed_cap is below" in call(observed_cap=len(ids) - 1)
    assert "max_indel_size" in call(max_indel_size=2**31)
    bad = da.copy()
    bad[1]["off"][0] += 1
    assert "do not tile" in call(da=bad)
    assert "do not tile" in call(n_ids=len(ids) - 1) and "do not tile" in call(ids=np.concatenate([ids, ids[:1]]))
    L = capi.lib()
    assert L.sk_realign_gate_observed_bound(-1) == -1 and L.sk_realign_gate_observed_bound(12) == 12
    assert L.sk_realign_gate_scratch_bytes(0, 1, 1) == 0 and L.sk_realign_gate_scratch_bytes(1, -1, 1) == 0 and L.sk_realign_gate_scratch_bytes(1, 1, 2**31) == 0
    assert call() == ""  # and the library goes on working


def test_device_entry_raises_the_flag_and_leaves_zeroed_output():
    if capi.lib().sk_broker_client():
        pytest.skip("not available to a broker client: the *_dev entry points need a GPU context of the caller's")
    capi.init(0)
    L = capi.lib()
    keys, cands, samples = _refusal_case()
    want = GM.realign_gate(keys, cands, samples, 49)
    n_ids = len(G.table_arrays(keys)[2])

    def refused(**kw):
        res, _ = _dev(keys, cands, samples, **kw)
        assert L.sk_check_device_errors() != 0 and "sk_realign_gate_dev" in capi.last_error() and L.sk_check_device_errors() == 0, kw
        body = lambda a: a[:len(a) - SLACK].view(np.uint8)
        assert not body(res["keys"]).any() and not body(res["logs"]).any() and res["totals"] == [0] * 10, kw
        for so in res["samples"]:
            assert not body(so["reads"]).any() and not body(so["observed_off"]).any() and not body(so["observed"]).any(), kw
            for a in so.values():
                assert (a[len(a) - SLACK:].view(np.uint8) == 0x5a).all(), kw

    for mutate, _ in REFUSED_READS:
        refused(mutate=mutate)
    refused(key_cap=1)               # more keys on the device than the room
    refused(id_cap=n_ids - 1)        # more ids than the room
    refused(observed_cap=n_ids - 1)  # observed_cap below the bound
    refused(n_keys=-1)
    refused(n_ids=n_ids - 1)         # the sets do not tile the pool
    with pytest.raises(capi.StrelkaAmdError, match="SK_MAX_SAMPLES"):
        _dev(keys, cands, samples * 9)
    _dev_same(keys, cands, samples, want, key_cap=2, id_cap=n_ids, observed_cap=n_ids)  # exactly the rooms: enough


def test_recorded_scenes_through_the_host_entry():
    """the reference's scenes: the model's table and candidacy through sk_realign_gate; against the model and against what the reference's
    own gate, zone, sets and logs gave"""
    n_reads = n_pass = 0
    for rec in GM.golden()["scenes"]:
        keys, cands, samples, _ = GM.run_recorded(rec)
        doc = CM.scene_document(GM.candidate_scene(rec))
        want = _host(keys, cands, samples, doc["max_indel_size"])
        n_samples = len(samples)
        assert [[k["pos"], k["type"], k["del_len"], k["ins"], k["is_candidate"], k["active_region_id"], k["logs"], k["haplotype_id"][:n_samples], k["is_haplotyping_bypassed"][:n_samples]]
                for k in want["keys"]] == [[k[f] for f in ("pos", "type", "del_len", "ins", "is_candidate", "active_region_id", "logs", "haplotype_id", "is_haplotyping_bypassed")]
                                           for k in rec["keys"]], rec["name"]
        marks = [0] * len(keys)
        index = [{r["id"]: i for i, r in enumerate(sm["reads"])} for sm in doc["samples"]]
        for rd in rec["reads"]:
            s, r = rd["sample"], index[rd["sample"]][rd["id"]]
            got = want["samples"][s]["reads"][r]
            assert got["zone"] == rd["zone"] and (got["status"] == GM.PASS) == bool(rd["gate"]) and (got["status"] == GM.OVERMAX) == (not rd["realignable"]), (rec["name"], rd)
            assert want["samples"][s]["observed"][r] == rd["member"], (rec["name"], rd)
            for k in rd["consulted"]:
                marks[k] = 1
            n_pass += rd["gate"]
        assert [k["gate_consulted"] for k in want["keys"]] == marks, rec["name"]
        n_reads += len(rec["reads"])
    assert n_reads > 1000 and 0 < n_pass < n_reads


def test_gate_behind_the_device_chain_on_one_stream():
    """per sample sk_read_intake_dev -> sk_region_haplotypes_dev -> sk_region_alleles_dev, then sk_indel_table_dev -> sk_read_depth_dev (per sample) ->
    sk_indel_candidates_dev -> sk_realign_gate_dev, all on one stream with no host copy in between and the key and id counts left on the device: the
    recorded two-sample scene under the germline configuration, against the model and against what the reference gave"""
    import torch
    if capi.lib().sk_broker_client():
        pytest.skip("not available to a broker client: the *_dev entry points need a GPU context of the caller's")
    from tests import indel_table_model as T
    from tests import test_region_haplotypes as RH
    capi.init(0)
    L = capi.lib()
    grec = next(r for r in GM.golden()["scenes"] if r["name"] == "two_samples_one_deletion@germline")
    rec = GM.candidate_scene(grec)
    sc = CM.scene_document(rec)
    samples, regions = T.scene_samples(sc)
    keys, cands, gate_samples, want = GM.run_recorded(grec)
    assert want["totals"][0] > 0 and want["totals"][2] > 0 and want["totals"][3] > 0
    copt, sets = CM.config_options(CM.golden()["configs"]["germline"], rec)
    win_begin, n_pos = rec["win_begin"], rec["n_pos"]
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    region_cap, max_hap_len = len(regions) + 3, 256
    reg = np.zeros(region_cap, capi.ACTIVE_REGION_DTYPE)
    for i, (b, e) in enumerate(regions):
        reg[i] = (b, e, 0)
    d_regions, d_n = dev(reg.view(np.int32)), dev(np.array([len(regions)], np.int32))
    opt = capi.intake_options()
    opt.max_indel_size = sc["max_indel_size"]
    allele_cap, insert_cap = capi.region_alleles_bounds(region_cap, max_hap_len)
    a_scratch_bytes = L.sk_region_alleles_scratch_bytes(region_cap, max_hap_len)
    depth_scratch_bytes = L.sk_read_depth_scratch_bytes(n_pos)
    d_sets = dev(K.rate_set_arrays(sets).view(np.uint8))
    torch.cuda.synchronize()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    keep, structs, n_bases = [], [], 0
    for sm, gs in zip(samples, gate_samples):
        c = dict(ref=sc["ref"], ref_offset=sc["ref_offset"], reads=sm["reads"], low=sm["low"], fwd=sm["fwd"], max_indel_size=sc["max_indel_size"], buf_begin=sm["buf_begin"],
                 buf_end=sm["buf_end"], ploidy=sm["ploidy"])
        n = len(sm["reads"])
        d = RH._dev_upload(c, region_cap)
        t, n_segs = d["t"], d["n_segs"]
        cap = capi.read_intake_obs_bound(n_segs)
        x = dict(reads=torch.zeros(n * 16, dtype=torch.uint8, device="cuda"), obs_off=torch.zeros(n + 1, dtype=torch.int64, device="cuda"),
                 obs=torch.zeros(cap * 32, dtype=torch.uint8, device="cuda"), sites=torch.zeros(1, dtype=torch.int64, device="cuda"), cand=torch.zeros(1, dtype=torch.uint8, device="cuda"),
                 arecs=torch.zeros(region_cap * 72, dtype=torch.uint8, device="cuda"), alleles=torch.zeros(allele_cap * 56, dtype=torch.uint8, device="cuda"),
                 ins=torch.zeros(insert_cap, dtype=torch.uint8, device="cuda"), atotals=torch.zeros(2, dtype=torch.int64, device="cuda"), prev=torch.zeros(1, dtype=torch.int32, device="cuda"),
                 ascratch=torch.zeros(a_scratch_bytes, dtype=torch.uint8, device="cuda"), align_id=dev(np.array(sm["align_id"] + [0], np.uint32).view(np.int32)),
                 iat=dev(np.array(sm["iat"] + [0], np.uint8)), depth1=torch.full((n_pos + 1,), -1, dtype=torch.int32, device="cuda"),
                 depth2=torch.full((n_pos + 1,), -1, dtype=torch.int32, device="cuda"), dscratch=torch.zeros(depth_scratch_bytes, dtype=torch.uint8, device="cuda"),
                 read_len=dev(np.array([r["read_len"] for r in gs["reads"]] + [0], np.int32)), realign_begin=dev(np.array([r["realign"][0] for r in gs["reads"]] + [0], np.int32)),
                 realign_end=dev(np.array([r["realign"][1] for r in gs["reads"]] + [0], np.int32)))
        i_scratch_bytes = L.sk_read_intake_scratch_bytes(n, n_segs, 0)
        x["iscratch"] = torch.zeros(max(i_scratch_bytes, 1), dtype=torch.uint8, device="cuda")
        capi._check(L.sk_read_intake_dev(p(d["ref"]), sc["ref_offset"], len(sc["ref"]), n, p(t[0]), p(t[1]), p(t[2]), p(t[3]), p(t[4]), p(t[5]), p(t[6]), C.byref(opt), 0, 0,
                                         p(x["reads"]), p(x["obs_off"]), p(x["obs"]), cap, p(x["sites"]), p(x["cand"]), p(x["iscratch"]), i_scratch_bytes, st))
        d["obs_off"], d["obs"] = x["obs_off"], x["obs"]
        RH._dev_launch(c, d, d_regions, d_n, st)
        capi._check(L.sk_region_alleles_dev(p(d["ref"]), sc["ref_offset"], len(sc["ref"]), p(d_regions), p(d_n), region_cap, p(d["recs"]), p(d["seq"]), d["seq_cap"],
                                            sc["max_indel_size"], max_hap_len, sc["prev_end_in"], p(x["arecs"]), p(x["alleles"]), allele_cap, p(x["ins"]), insert_cap,
                                            p(x["atotals"]), p(x["prev"]), p(x["ascratch"]), a_scratch_bytes, st))
        keep.append((d, x, n, n_segs, cap))
        q = lambda tensor: tensor.data_ptr()
        structs.append(capi.IndelTableSample(n, 0, q(t[0]), q(t[1]), q(x["obs_off"]), q(x["obs"]), cap, q(x["align_id"]), q(x["iat"]), q(d["recs"]), q(d["support"]),
                                             d["support_cap"], q(x["arecs"]), q(x["alleles"]), allele_cap, q(x["ins"]), insert_cap))
        n_bases += sum(len(r["code"]) for r in sm["reads"])
    n_samples = len(samples)
    arr = (capi.IndelTableSample * n_samples)(*structs)
    expand_cap, key_cap, id_cap, ins_cap = 4096, 512, 4096, n_bases + 1024
    room = lambda n, itemsize: torch.full(((n + SLACK) * itemsize,), 0x5a, dtype=torch.uint8, device="cuda")
    out = dict(keys=torch.zeros(key_cap * 56, dtype=torch.uint8, device="cuda"), data=torch.zeros(key_cap * n_samples * 64, dtype=torch.uint8, device="cuda"),
               ids=torch.zeros(id_cap, dtype=torch.int32, device="cuda"), ins=torch.zeros(ins_cap, dtype=torch.uint8, device="cuda"),
               totals=torch.full((4,), -1, dtype=torch.int64, device="cuda"), cand=torch.full((key_cap * 8,), 0x5a, dtype=torch.uint8, device="cuda"),
               rates=torch.full((key_cap * n_samples * 32,), 0x5a, dtype=torch.uint8, device="cuda"), ctotals=torch.full((2,), -1, dtype=torch.int64, device="cuda"),
               gkeys=room(key_cap, 48), glogs=room(key_cap * n_samples, 16), gtotals=torch.full((2 + capi.MAX_SAMPLES,), -1, dtype=torch.int64, device="cuda"))
    scratch_bytes = L.sk_indel_table_scratch_bytes(n_samples, expand_cap, region_cap)
    scratch = torch.zeros(scratch_bytes, dtype=torch.uint8, device="cuda")
    c_scratch_bytes = L.sk_indel_candidates_scratch_bytes()
    c_scratch = torch.zeros(c_scratch_bytes, dtype=torch.uint8, device="cuda")
    g_scratch_bytes = L.sk_realign_gate_scratch_bytes(n_samples, key_cap, id_cap)
    g_scratch = torch.full((g_scratch_bytes,), 0xa5, dtype=torch.uint8, device="cuda")
    capi._check(L.sk_indel_table_dev(n_samples, C.addressof(arr), keep[0][0]["ref"].data_ptr(), sc["ref_offset"], len(sc["ref"]), d_regions.data_ptr(), d_n.data_ptr(), region_cap,
                                     sc["prev_end_in"], expand_cap, out["keys"].data_ptr(), key_cap, out["data"].data_ptr(), out["ids"].data_ptr(), id_cap, out["ins"].data_ptr(),
                                     ins_cap, out["totals"].data_ptr(), scratch.data_ptr(), scratch_bytes, st))
    cstructs, gin, gout, gouts = [], [], [], []
    for d, x, n, n_segs, cap in keep:
        t = d["t"]
        capi._check(L.sk_read_depth_dev(n, t[2].data_ptr(), t[3].data_ptr(), t[4].data_ptr(), n_segs, t[5].data_ptr(), x["iat"].data_ptr(), win_begin, n_pos,
                                        x["depth1"].data_ptr(), x["depth2"].data_ptr(), x["dscratch"].data_ptr(), depth_scratch_bytes, st))
        cstructs.append(capi.IndelCandidateSample(n, 0, x["obs_off"].data_ptr(), x["obs"].data_ptr(), cap, x["depth1"].data_ptr(), x["depth2"].data_ptr()))
        gin.append(capi.RealignGateSample(n, 0, t[5].data_ptr(), t[2].data_ptr(), t[3].data_ptr(), t[4].data_ptr(), n_segs, x["read_len"].data_ptr(), x["align_id"].data_ptr(),
                                          x["realign_begin"].data_ptr(), x["realign_end"].data_ptr()))
        o = dict(reads=room(n, 12), observed_off=room(n + 1, 8), observed=room(id_cap, 4))
        gouts.append(o)
        gout.append(capi.RealignGateSampleOut(o["reads"].data_ptr(), o["observed_off"].data_ptr(), o["observed"].data_ptr(), id_cap))
    carr = (capi.IndelCandidateSample * n_samples)(*cstructs)
    o = K.capi_options(copt)
    capi._check(L.sk_indel_candidates_dev(n_samples, C.addressof(carr), win_begin, n_pos, out["keys"].data_ptr(), out["data"].data_ptr(), out["totals"].data_ptr(), key_cap,
                                          d_sets.data_ptr(), C.addressof(o), out["cand"].data_ptr(), out["rates"].data_ptr(), out["ctotals"].data_ptr(), c_scratch.data_ptr(),
                                          c_scratch_bytes, st))
    garr_in, garr_out = (capi.RealignGateSample * n_samples)(*gin), (capi.RealignGateSampleOut * n_samples)(*gout)
    capi._check(L.sk_realign_gate_dev(n_samples, C.addressof(garr_in), out["keys"].data_ptr(), out["data"].data_ptr(), out["ids"].data_ptr(), out["totals"].data_ptr(), key_cap, id_cap,
                                      out["cand"].data_ptr(), out["rates"].data_ptr(), sc["max_indel_size"], out["gkeys"].data_ptr(), out["glogs"].data_ptr(), C.addressof(garr_out),
                                      out["gtotals"].data_ptr(), g_scratch.data_ptr(), g_scratch_bytes, st))
    torch.cuda.synchronize()
    capi._check(L.sk_check_device_errors())
    nk = int(out["totals"].cpu().numpy()[0])
    assert nk == len(keys)
    gk, gl = out["gkeys"].cpu().numpy().view(capi.REALIGN_GATE_KEY_DTYPE), out["glogs"].cpu().numpy().view(capi.REALIGN_GATE_LOG_RATES_DTYPE)
    assert not gk[nk:key_cap].view(np.uint8).any() and not gl[nk * n_samples:key_cap * n_samples].view(np.uint8).any()
    res = dict(keys=np.concatenate([gk[:nk], gk[key_cap:]]), logs=np.concatenate([gl[:nk * n_samples], gl[key_cap * n_samples:]]), totals=out["gtotals"].cpu().numpy().tolist(),
               samples=[dict(reads=g["reads"].cpu().numpy().view(capi.REALIGN_GATE_READ_DTYPE), observed_off=g["observed_off"].cpu().numpy().view(np.int64),
                             observed=g["observed"].cpu().numpy().view(np.int32)) for g in gouts])
    _same(G.device_results(res, n_samples, out["ins"].cpu().numpy(), SLACK), want)
