"""Indel candidacy on the device (sk_read_depth, sk_indel_candidates; csrc/indel_candidates.hip): the depth arrays, every rate bit for bit,
the breakpoint insert size, is_candidate and the reason of every undecided key equal the loop model (tests/indel_candidates_model.py,
itself pinned to vectors recorded from the reference by tests/test_indel_candidates_model.py) -- through the host entries, the _dev
entries, and behind sk_indel_table_dev on one stream.

The shapes are the smallest at which the kernels can go wrong: windows of 1 023, 1 024, 1 025 and 2 049 positions (the scan's block of
1 024 and its carried prefix), reads that straddle both window edges, 0 / 1 / 63 / 64 / 65 keys (the wave edge), 1 and 8 samples."""
import ctypes as C
import math
import sys

import numpy as np
import pytest

from strelka_amd import capi
from tests import indel_candidates_cases as K
from tests import indel_candidates_model as CM

pytestmark = pytest.mark.gpu

DBL_MIN = sys.float_info.min
BELOW_HALF = float(np.nextafter(0.5, 0.0))


# ---------------------------------------------------------------------------------------------------------------- rule D
def _depth(reads, iat, win_begin, n_pos):
    """host entry against model -> the model's arrays"""
    capi.init(0)
    want = CM.depth_buffers(reads, iat, win_begin, n_pos)
    got = capi.read_depth(reads, iat, win_begin, n_pos)
    for g, w in zip(got, want):
        assert g.dtype == np.uint32 and g.tolist() == w.tolist()
    return want


def _dev_depth(reads, iat, win_begin, n_pos, path_cap=None, mutate=None):
    """sk_read_depth_dev on uploaded arrays -> (depth1, depth2) as it left them (canaries behind the window included)"""
    import torch
    L = capi.lib()
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    path_off, n_seg, path, pos = capi.pack_paths(reads)
    iat_a = np.array(list(iat) + [0], np.uint8)
    if mutate:
        mutate(path_off, n_seg, path, iat_a)
    t = [dev(path_off), dev(n_seg), dev(path), dev(pos), dev(iat_a)]
    d = [torch.full((n_pos + 4,), 0x5a5a5a5a, dtype=torch.int32, device="cuda") for _ in range(2)]
    scratch_bytes = L.sk_read_depth_scratch_bytes(n_pos)
    scratch = torch.full((scratch_bytes,), 0xa5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    capi._check(L.sk_read_depth_dev(len(reads), t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), len(path) - 1 if path_cap is None else path_cap, t[3].data_ptr(),
                                    t[4].data_ptr(), win_begin, n_pos, d[0].data_ptr(), d[1].data_ptr(), scratch.data_ptr(), scratch_bytes, torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    out = [x.cpu().numpy().view(np.uint32) for x in d]
    for x in out:
        assert x[n_pos:].tolist() == [0x5a5a5a5a] * 4  # nothing behind the window is written
    return out[0][:n_pos], out[1][:n_pos]


def _window_reads(win_begin, n_pos, seed):
    """reads over and around the window: one that straddles both edges, deletions followed by matches, insertions, clips, all three iat"""
    rng = np.random.default_rng(seed)
    reads = [K.read(win_begin - 7, [(K.M, n_pos + 20)]), K.read(win_begin - 5, [(K.S, 3), (K.M, 7), (K.D, 4), (K.M, 6)]),
             K.read(win_begin + n_pos - 6, [(K.M, 3), (K.I, 2), (K.M, 2), (K.D, 3), (K.M, 9)]), K.read(win_begin - 40, [(K.M, 30)]), K.read(win_begin + n_pos, [(K.M, 8)]),
             K.read(win_begin + 1020, [(K.M, 3), (K.D, 2), (K.M, 4)]), K.read(win_begin + n_pos - 1, [(K.M, 1)]), K.read(win_begin, [(K.M, 1)])]
    iat = [0, 1, 0, 0, 1, 0, 1, 0]
    for _ in range(150):
        p = int(rng.integers(win_begin - 60, win_begin + n_pos + 10))
        a, b, c = (int(x) for x in rng.integers(1, 60, 3))
        kind = int(rng.integers(0, 4))
        path = [[(K.M, a + b)], [(K.M, a), (K.D, c), (K.M, b)], [(K.M, a), (K.I, c), (K.M, b)], [(K.S, c), (K.M, a), (K.D, 2), (CM.SEG_SEQ_MATCH, b), (K.S, 2)]][kind]
        reads.append(K.read(p, path))
        iat.append(int(rng.integers(0, 3)))
    return reads, iat


@pytest.mark.parametrize("n_pos", [1023, 1024, 1025, 2049])
def test_depth_windows_across_the_scan_block_and_its_carry(n_pos):
    reads, iat = _window_reads(5000, n_pos, n_pos)
    want = _depth(reads, iat, 5000, n_pos)
    assert want[0][0] > 0 and want[0][-1] > 0 and want[1][0] > 0 and want[1][-1] > 0  # (the inputs reach both edges of both arrays)
    if not capi.lib().sk_broker_client():
        got = _dev_depth(reads, iat, 5000, n_pos)
        assert got[0].tolist() == want[0].tolist() and got[1].tolist() == want[1].tolist()
        capi._check(capi.lib().sk_check_device_errors())


def test_depth_small_cases():
    assert _depth([K.read(10, [(K.M, 3), (K.D, 2), (K.M, 2)])], [0], 8, 12)[0].tolist() == [0, 0, 1, 1, 1, 0, 0, 1, 1, 0, 0, 0]
    path = [(K.S, 4), (K.M, 2), (K.I, 3), (K.M, 1), (K.SKIP, 2), (CM.SEG_SEQ_MATCH, 1), (CM.SEG_SEQ_MISMATCH, 1), (CM.SEG_HARD_CLIP, 5)]
    assert _depth([K.read(0, path)], [1], 0, 8)[1].tolist() == [1, 1, 1, 0, 0, 1, 1, 0]
    reads = [K.read(-3, [(K.M, 5)]), K.read(2, [(K.M, 10)]), K.read(1, [(K.M, 2)]), K.read(0, [(K.M, 4)])]
    d1, d2 = _depth(reads, [0, 0, 1, 2], 0, 4)
    assert d1.tolist() == [1, 1, 1, 1] and d2.tolist() == [0, 1, 1, 0]
    assert [x.tolist() for x in _depth([], [], 0, 5)] == [[0] * 5] * 2 and [len(x) for x in _depth(reads, [0] * 4, 0, 0)] == [0, 0]
    _depth([K.read(2**31 - 10, [(K.M, 100)]), K.read(-2**31, [(K.M, 5), (K.D, 2**31 - 1), (K.D, 2**31 - 1), (K.M, 50)])], [0, 0], 2**31 - 40, 39)  # positions past int32


def _bad_iat(path_off, n_seg, path, iat):
    iat[1] = 3


def _bad_seg_type(path_off, n_seg, path, iat):
    path[1][0] = 10


def _path_outside(path_off, n_seg, path, iat):
    n_seg[2] += 1


def _negative_n_seg(path_off, n_seg, path, iat):
    n_seg[0] = -1


REFUSED_DEPTH = ((_bad_iat, "iat above 2"), (_bad_seg_type, "segment type"), (_path_outside, "outside path_cap"), (_negative_n_seg, "negative n_seg"))


def test_depth_refusals_of_the_host_entry():
    capi.init(0)
    reads = [K.read(3, [(K.M, 4), (K.D, 1), (K.M, 2)]), K.read(5, [(K.M, 6)]), K.read(6, [(K.M, 2)])]
    for mutate, which in REFUSED_DEPTH:
        path_off, n_seg, path, pos = capi.pack_paths(reads)
        iat = np.array([0, 1, 0, 0], np.uint8)
        mutate(path_off, n_seg, path, iat)
        with pytest.raises(capi.StrelkaAmdError, match=which):
            capi.read_depth(None, iat[:3], 0, 16, packed=(path_off, n_seg, path, pos, len(path) - 1))
    with pytest.raises(capi.StrelkaAmdError, match="negative size"):
        capi.read_depth(reads, [0, 0, 0], 0, -1)
    assert capi.lib().sk_read_depth_scratch_bytes(-1) == 0
    _depth(reads, [0, 1, 0], 0, 16)  # and the library goes on working


def test_depth_device_entry_raises_the_flag_and_leaves_zeros():
    if capi.lib().sk_broker_client():
        pytest.skip("not available to a broker client: the *_dev entry points need a GPU context of the caller's")
    capi.init(0)
    L = capi.lib()
    reads = [K.read(3, [(K.M, 4), (K.D, 1), (K.M, 2)]), K.read(5, [(K.M, 6)]), K.read(6, [(K.M, 2)])]
    for mutate, _ in REFUSED_DEPTH:
        d1, d2 = _dev_depth(reads, [0, 1, 0], 0, 16, mutate=mutate)
        assert L.sk_check_device_errors() != 0 and "sk_read_depth_dev" in capi.last_error() and L.sk_check_device_errors() == 0, mutate.__name__
        assert not d1.any() and not d2.any(), mutate.__name__
    want = CM.depth_buffers(reads, [0, 1, 0], 0, 16)
    got = _dev_depth(reads, [0, 1, 0], 0, 16)
    capi._check(L.sk_check_device_errors())
    assert got[0].tolist() == want[0].tolist() and got[1].tolist() == want[1].tolist()


# ---------------------------------------------------------------------------------------------------------------- rules E, B, C
def _zeros(n_samples, n_pos):
    return [np.zeros(n_pos, np.uint32) for _ in range(n_samples)]


def _samples(sample_obs, depth1, depth2):
    return [dict(n_reads=n, obs_off=off, obs=arr, depth1=d1, depth2=d2) for (n, off, arr), d1, d2 in zip(K.obs_arrays(sample_obs), depth1, depth2)]


def _cand(keys, depth1=None, depth2=None, win_begin=0, n_pos=64, sets=None, sample_obs=None, **opt):
    """host entry against model -> the model's (out, totals)"""
    capi.init(0)
    n_samples = len(keys[0]["samples"]) if keys else opt.pop("n_samples", 1)
    opt.pop("n_samples", None)
    depth1, depth2 = depth1 or _zeros(n_samples, n_pos), depth2 or _zeros(n_samples, n_pos)
    sample_obs = sample_obs or [[] for _ in range(n_samples)]
    sets = sets or [K.ramp(), K.ramp()]
    o = K.options(**opt)
    want, totals = CM.indel_candidates(keys, sample_obs, depth1, depth2, win_begin, sets, o)
    ka, da = K.table_arrays(keys)
    res = capi.indel_candidates(_samples(sample_obs, depth1, depth2), win_begin, n_pos, ka, da, K.rate_set_arrays(sets), K.capi_options(o))
    got = K.device_results(res, n_samples)
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        assert g == w, (k, keys[k])  # (zero bit mismatches on the rates: they are compared as bit patterns)
    assert res["totals"] == totals
    return want, totals


def _dev_cand(keys, depth1, depth2, win_begin, n_pos, sets, sample_obs, opt, key_cap=None, n_keys=None, mutate_sets=None, obs_cap=None):
    """sk_indel_candidates_dev on uploaded arrays -> (dict(out, rates, totals) over all of key_cap, n_samples)"""
    import torch
    L = capi.lib()
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    n_samples = len(depth1)
    ka, da = K.table_arrays(keys)
    key_cap = len(keys) + 3 if key_cap is None else key_cap
    d_keys = dev(np.concatenate([ka, np.zeros(1, ka.dtype)]).view(np.uint8))
    d_data = dev(np.concatenate([da, np.zeros(1, da.dtype)]).view(np.uint8))
    d_table_totals = dev(np.array([len(keys) if n_keys is None else n_keys, 0, 0, 0], np.int64))
    sa = K.rate_set_arrays(sets)
    if mutate_sets:
        mutate_sets(sa)
    d_sets = dev(sa.view(np.uint8))
    keep, structs = [], []
    for (n, off, arr), d1, d2 in zip(K.obs_arrays(sample_obs), depth1, depth2):
        t = [dev(off), dev(np.concatenate([arr, np.zeros(1, arr.dtype)]).view(np.uint8)), dev(np.concatenate([d1, [0]]).astype(np.uint32).view(np.int32)),
             dev(np.concatenate([d2, [0]]).astype(np.uint32).view(np.int32))]
        keep.append(t)
        structs.append(capi.IndelCandidateSample(n, 0, t[0].data_ptr(), t[1].data_ptr(), len(arr) if obs_cap is None else obs_cap, t[2].data_ptr(), t[3].data_ptr()))
    arr_s = (capi.IndelCandidateSample * n_samples)(*structs)
    out = torch.full((max(key_cap, 1) * 8,), 0x5a, dtype=torch.uint8, device="cuda")
    rates = torch.full((max(key_cap, 1) * n_samples * 32,), 0x5a, dtype=torch.uint8, device="cuda")
    totals = torch.full((2,), -1, dtype=torch.int64, device="cuda")
    scratch_bytes = L.sk_indel_candidates_scratch_bytes()
    scratch = torch.full((scratch_bytes,), 0xa5, dtype=torch.uint8, device="cuda")
    o = K.capi_options(opt)
    torch.cuda.synchronize()
    capi._check(L.sk_indel_candidates_dev(n_samples, C.addressof(arr_s), win_begin, n_pos, d_keys.data_ptr(), d_data.data_ptr(), d_table_totals.data_ptr(), key_cap,
                                          d_sets.data_ptr(), C.addressof(o), out.data_ptr(), rates.data_ptr(), totals.data_ptr(), scratch.data_ptr(), scratch_bytes,
                                          torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return dict(out=out.cpu().numpy()[:key_cap * 8].view(capi.INDEL_CANDIDATE_DTYPE), rates=rates.cpu().numpy()[:key_cap * n_samples * 32].view(capi.INDEL_ERROR_RATES_DTYPE),
                totals=totals.cpu().numpy().tolist()), n_samples


def _random_case(n_keys, n_samples, seed, n_pos=700):
    """keys of every kind over a window with random depths, rate sets per sample, breakpoint observations"""
    rng = np.random.default_rng(seed)
    keys, sample_obs = [], [[] for _ in range(n_samples)]
    for i in range(n_keys):
        pos = 100 + 9 * i // 2  # (two keys per position now and then; the first at the window's first position)
        n1 = tuple(int(x) for x in rng.integers(0, 25, n_samples))
        kind = i % 7
        common = dict(n1=n1, active_region_id=int(rng.integers(-1, 2)) * pos, unit=int(rng.integers(0, 4)), ref_count=int(rng.integers(0, 30)), indel_count=int(rng.integers(0, 30)),
                      flags=CM.AR_PENDING if rng.integers(0, 9) == 0 else 0)
        if kind in (0, 1):
            keys.append(K.key(pos, del_len=1 + i % 3, **common))
        elif kind in (2, 3):
            keys.append(K.key(pos, ins="ACGT"[:1 + i % 4], **common))
        elif kind == 4:
            keys.append(K.key(pos, K.MISMATCH, 1, "G", **common))
        elif kind == 5:
            keys.append(K.key(pos, del_len=2, ins="T", **common))  # a swap: doNotGenotype
        else:
            n_obs = int(rng.integers(1, 5))
            keys.append(K.key(pos, K.BP_LEFT if i % 2 else K.BP_RIGHT, n_bp_obs=n_obs, **dict(common, flags=common["flags"] | (CM.DO_NOT_GENOTYPE if i % 4 else 0))))
            for _ in range(n_obs):
                sample_obs[int(rng.integers(0, n_samples))].append(K.bp_obs(pos, keys[-1]["type"], int(rng.integers(1, 40))))
    keys = K.sorted_keys(keys)
    depth1 = [rng.integers(0, 60, n_pos).astype(np.uint32) for _ in range(n_samples)]
    depth2 = [rng.integers(0, 9, n_pos).astype(np.uint32) for _ in range(n_samples)]
    sets = [K.ramp()] + [[[(float(x), float(y)) for x, y in rng.uniform(0, 0.6, (int(rng.integers(1, 41)), 2))] for _ in range(int(rng.integers(1, 5)))] for _ in range(n_samples)]
    opt = dict(is_sample_specific_rates=1, is_indel_ref_error_factor=1, log_indel_ref_error_factor=math.log(1.8), is_haplotyping_enabled=seed % 2, max_candidate_depth=40.0 * n_samples,
               is_count_towards_depth_filter=[1, 0, 1, 1, 0, 1, 1, 1], min_candidate_indel_open_length=20)
    return keys, depth1, depth2, sets, sample_obs, opt


@pytest.mark.parametrize("n_samples", [1, 8])
@pytest.mark.parametrize("n_keys", [0, 1, 63, 64, 65])
def test_key_counts_and_samples_host_and_device_entries(n_keys, n_samples):
    keys, depth1, depth2, sets, sample_obs, opt = _random_case(n_keys, n_samples, 31 * n_keys + n_samples)
    want, totals = _cand(keys, depth1, depth2, 100, 700, sets, sample_obs, n_samples=n_samples, **opt)
    if n_keys >= 63:
        assert totals[0] > 0 and totals[1] > 0 and any(w["bp_insert_size"] for w in want) and len({w["undecided"] for w in want}) >= 2
    if capi.lib().sk_broker_client():
        return
    res, _ = _dev_cand(keys, depth1, depth2, 100, 700, sets, sample_obs, K.options(**opt))
    capi._check(capi.lib().sk_check_device_errors())
    assert K.device_results(dict(out=res["out"][:n_keys], rates=res["rates"][:n_keys * n_samples]), n_samples) == want and res["totals"] == totals
    assert not res["out"][n_keys:].view(np.uint8).any() and not res["rates"][n_keys * n_samples:].view(np.uint8).any()  # records past the key count are zero


@pytest.mark.parametrize("config", sorted(CM.golden()["configs"]))
def test_recorded_scenes_through_the_host_entries(config):
    """the reference's scenes: sk_read_depth per sample, then sk_indel_candidates over the model's table; against the model and against what
    the reference's own classes gave"""
    capi.init(0)
    from tests import indel_table_model as T
    cfg = CM.golden()["configs"][config]
    n = 0
    for sc in (s for s in CM.golden()["scenes"] if s["config"] == config):
        doc = CM.scene_document(sc)
        if sc.get("drop_regions"):
            doc = dict(doc, regions=[])
        samples, regions = T.scene_samples(doc)
        keys, _ = T.indel_table(doc["ref"], doc["ref_offset"], samples, regions, doc["prev_end_in"])
        depth = [_depth(sm["reads"], sm["iat"], sc["win_begin"], sc["n_pos"]) for sm in samples]
        assert CM.depth_as_recorded(depth, sc) == sc["depth"]
        opt, sets = CM.config_options(cfg, sc)
        want, _ = _cand(keys, [d[0] for d in depth], [d[1] for d in depth], sc["win_begin"], sc["n_pos"], sets, [sm["obs"] for sm in samples], n_samples=len(samples), **opt)
        assert CM.as_recorded(keys, want) == sc["keys"]
        n += len(keys)
    assert n > 0


def _depth_at(n_pos, at, value):
    d = np.zeros(n_pos, np.uint32)
    d[at] = value
    return d


def test_undecided_by_the_exact_binomial_and_the_ratio_at_equality():
    d = [_depth_at(64, 9, 30)]
    for cand_rate in (0.02, 0.1):  # p = 0.02: the variance ratio is above 0.01; 30 * 0.1 = 3.0 is not below papprox[17]
        want, totals = _cand([K.key(10, del_len=1, n1=(3,))], depth1=d, sets=[K.flat(cand_rate), K.ramp()])
        assert (want[0]["is_candidate"], want[0]["undecided"]) == (0, CM.UNDECIDED_EXACT_BINOMIAL) and totals == [0, 1]
    # p / (1 - p) == 0.01 exactly is still the Poisson branch: decided, and differently for 6 and 7 reads of 18
    p = K.ratio_exactly_one_hundredth()
    d = [_depth_at(64, 9, 18)]
    want, totals = _cand([K.key(10, del_len=1, n1=(6,)), K.key(10, del_len=2, n1=(7,))], depth1=d, sets=[K.flat(p), K.ramp()])
    assert [(w["is_candidate"], w["undecided"]) for w in want] == [(0, 0), (1, 0)] and totals == [1, 0]
    # an exact-binomial sample before the one that says true leaves the key undecided; after it, it is never asked
    d = [_depth_at(64, 9, 5), _depth_at(64, 9, 1000)]
    assert _cand([K.key(10, del_len=1, n1=(5, 5))], depth1=d, sets=[K.flat(3e-3), K.ramp()])[1] == [1, 0]
    assert _cand([K.key(10, del_len=1, n1=(5, 5))], depth1=d[::-1], sets=[K.flat(3e-3), K.ramp()])[1] == [0, 1]


def test_signal_floor_the_fudge_line_and_the_window_edges():
    zero = [K.flat(0.0), K.ramp()]  # p <= 0: any tier-1 read rejects the null, so the floor of 2 decides alone
    assert _cand([K.key(10, del_len=1, n1=(1,))], sets=zero)[1] == [0, 0]
    assert _cand([K.key(10, del_len=1, n1=(2,))], sets=zero)[1] == [1, 0]  # total = max(0, 2): n1 above the depth
    assert _cand([K.key(10, del_len=1, n1=(1,))], depth1=[_depth_at(64, 9, 2)], sets=zero)[1] == [1, 0]
    assert _cand([K.key(10, del_len=1, n1=(1,))], depth1=[_depth_at(64, 10, 2)], sets=zero)[1] == [0, 0]  # pos - 1, not pos
    full = [np.full(64, 7, np.uint32)]
    assert _cand([K.key(100, del_len=1, n1=(1,)), K.key(164, del_len=1, n1=(1,)), K.key(165, del_len=1, n1=(1,))], depth1=full, win_begin=100, sets=zero)[1] == [1, 0]
    assert _cand([K.key(-2**31, del_len=1, n1=(1,)), K.key(2**31 - 1, del_len=1, n1=(1,))], depth1=full, win_begin=2**31 - 64, sets=zero)[1] == [1, 0]  # pos - 1 below int32


def test_order_of_the_tests_and_the_weak_signal():
    d = [_depth_at(64, 9, 20)]
    ok = dict(del_len=1, n1=(3,))
    assert _cand([K.key(10, **ok)], depth1=d)[1] == [1, 0]
    assert _cand([K.key(10, flags=CM.DO_NOT_GENOTYPE | CM.AR_PENDING, **ok)], depth1=d)[1] == [0, 0]
    assert _cand([K.key(10, flags=CM.AR_PENDING, **ok)], depth1=d)[0][0]["undecided"] == CM.UNDECIDED_AR_PENDING
    assert _cand([K.key(10, **ok)], depth1=d, is_haplotyping_enabled=1)[1] == [0, 0]
    assert _cand([K.key(10, active_region_id=0, **ok)], depth1=d, is_haplotyping_enabled=1)[1] == [1, 0]
    assert _cand([K.key(10, del_len=1, n1=(0,))], depth1=d, is_candidate_indel_signal_test=0)[1] == [0, 0]
    assert _cand([K.key(10, del_len=1, n1=(0, 1))], is_candidate_indel_signal_test=0)[1] == [1, 0]


def test_breakpoint_length_and_257_or_258_observations():
    d = [_depth_at(64, 9, 20), _depth_at(64, 9, 0)]
    for n_obs, longest, want in ((3, 19, (0, CM.DECIDED)), (3, 20, (1, CM.DECIDED)), (257, 20, (1, CM.DECIDED)), (258, 19, (0, CM.DECIDED)),
                                 (258, 20, (0, CM.UNDECIDED_BP_OBS_ORDER))):
        obs = [K.bp_obs(10, K.BP_LEFT, 5)] * (n_obs - 1) + [K.bp_obs(10, K.BP_LEFT, longest)]
        keys = [K.key(10, del_len=3, n1=(3, 0)), K.key(10, K.BP_LEFT, n1=(3, 0), n_bp_obs=n_obs), K.key(10, K.BP_RIGHT, n1=(3, 0), n_bp_obs=1), K.key(11, K.BP_LEFT, n1=(0, 0), n_bp_obs=1)]
        out, _ = _cand(keys, depth1=d, sample_obs=[obs[:n_obs // 2] + [K.bp_obs(11, K.BP_LEFT, 33)], obs[n_obs // 2:] + [K.bp_obs(10, K.BP_RIGHT, 27)]])
        assert (out[1]["is_candidate"], out[1]["undecided"], out[1]["bp_insert_size"]) == want + (longest,), (n_obs, longest)
        assert [o["bp_insert_size"] for o in out] == [0, longest, 27, 33]


def test_depth_filter_at_and_above_the_limit():
    d1 = [_depth_at(64, 9, 20), _depth_at(64, 9, 7)]
    d2 = [_depth_at(64, 9, 4), _depth_at(64, 9, 1)]
    k = [K.key(10, del_len=1, n1=(3, 0))]
    assert _cand(k, d1, d2, max_candidate_depth=32.0)[1] == [1, 0]
    assert _cand(k, d1, d2, max_candidate_depth=31.5)[1] == [0, 0]
    assert _cand(k, d1, d2, max_candidate_depth=24.0, is_count_towards_depth_filter=[1, 0] + [1] * 6)[1] == [1, 0]
    assert _cand(k, d1, d2, max_candidate_depth=0.0)[1] == [1, 0]


@pytest.mark.parametrize("log_factor", [math.log(1.8), 0.0, -3.5, 40.0, -800.0])
def test_rule_e_edge_arguments_bit_for_bit(log_factor):
    """what sk_log / sk_exp meet at the ends of rule E: rates of 0, DBL_MIN, 0.5 - 1ulp, 0.5, 1.0 through the scaling.  A rate of 0 and a
    rate of 0.5 or more give log(0), which the restated routine declines: the device library's -inf is the host's.  (A subnormal rate would
    reach the device library's log too -- the restated one declines subnormals -- and is not part of the contract: DESIGN section 3 says so.)"""
    values = [0.0, DBL_MIN, 1e-300, 1e-9, 4.9e-3, 0.25, float(np.nextafter(0.25, 1)), float(np.nextafter(0.25, 0)), 0.4, BELOW_HALF, 0.5, float(np.nextafter(0.5, 1)), 0.7, 1.0]
    sets = [K.ramp(), [[(v, v) for v in values]]]
    keys = [K.key(10 + i, del_len=1, unit=1, ref_count=1, indel_count=i + 1, n1=(0,)) for i in range(len(values))]
    want, _ = _cand(keys, sets=sets, is_indel_ref_error_factor=1, log_indel_ref_error_factor=log_factor)
    assert [CM.bits_double(w["rates"][0][1]) for w in want] == [CM.scale_indel_error_rate(log_factor, v) for v in values]
    assert want[0]["rates"][0][1] == 0 and [CM.bits_double(w["rates"][0][1]) for w in want[-4:]] == [0.5] * 4


def test_sample_specific_sets_and_the_shared_set():
    sets = [K.flat(0.001), K.flat(0.01), K.flat(0.02, n_sizes=2, n_counts=3)]
    k = [K.key(5, del_len=1, n1=(1, 1)), K.key(6, ins="AC", unit=2, ref_count=2, indel_count=3, n1=(1, 1))]
    want, _ = _cand(k, sets=sets, is_sample_specific_rates=1)
    assert [CM.bits_double(r[0]) for r in want[0]["rates"]] == [0.01, 0.02]
    want, _ = _cand(k, sets=sets[:2], is_sample_specific_rates=0)
    assert [CM.bits_double(r[0]) for r in want[0]["rates"]] == [0.01, 0.01]


def _too_many_sizes(sa):
    sa[1]["n_sizes"] = 5


def _no_sizes(sa):
    sa[0]["n_sizes"] = 0


def _count_zero(sa):
    sa[1]["n_counts"][0] = 0


def _count_41(sa):
    sa[1]["n_counts"][0] = 41


def _rate_above_one(sa):
    sa[1]["deletion"][0][0] = 1.5


def _rate_negative(sa):
    sa[0]["insertion"][0][2] = -1e-9


def _rate_nan(sa):
    sa[1]["insertion"][0][0] = np.nan


REFUSED_SETS = (_too_many_sizes, _no_sizes, _count_zero, _count_41, _rate_above_one, _rate_negative, _rate_nan)


def _host_call(keys, sets, opt, n_samples=1, sample_obs=None, mutate_sets=None, obs_cap=None, n_pos=64, n_keys=None):
    try:
        ka, da = K.table_arrays(keys)
        sa = K.rate_set_arrays(sets)
        if mutate_sets:
            mutate_sets(sa)
        samples = _samples(sample_obs or [[] for _ in range(n_samples)], _zeros(n_samples, max(n_pos, 0)), _zeros(n_samples, max(n_pos, 0)))
        if obs_cap is not None:
            samples[0]["obs_cap"] = obs_cap
        capi.indel_candidates(samples, 0, n_pos, ka, da, sa, K.capi_options(opt), n_samples=n_samples, n_keys=n_keys)
    except capi.StrelkaAmdError as e:
        return str(e)
    return ""


def test_refusals_of_the_host_entry():
    capi.init(0)
    keys, sets, opt = [K.key(10, del_len=1, n1=(3,))], [K.ramp(), K.ramp()], K.options()
    assert _host_call(keys, sets, opt) == ""
    for mutate in REFUSED_SETS:
        msg = _host_call(keys, sets, opt, mutate_sets=mutate)
        assert ("rate" in msg or "sizes" in msg or "count" in msg) and msg.startswith("sk_indel_candidates: rate set"), (mutate.__name__, msg)
    assert "papprox" in _host_call(keys, sets, CM.default_options())  # what the defaults leave: caller data
    assert "papprox" in _host_call(keys, sets, K.options(papprox=K.PAPPROX[:5] + [K.PAPPROX[4]] + K.PAPPROX[6:]))
    assert "papprox" in _host_call(keys, sets, K.options(papprox=K.PAPPROX[:17] + [float("nan")]))
    keys8 = [K.key(10, del_len=1, n1=(3,) * 8)]
    assert "SK_MAX_SAMPLES" in _host_call(keys8, sets, opt, n_samples=9, sample_obs=[[]] * 8) and "SK_MAX_SAMPLES" in _host_call(keys, sets, opt, n_samples=0)
    assert "negative size" in _host_call(keys, sets, opt, n_pos=-1) and "negative size" in _host_call(keys, sets, opt, n_keys=-1)
    assert "outside obs_cap" in _host_call([K.key(10, K.BP_LEFT, n1=(3,), n_bp_obs=2)], sets, opt, sample_obs=[[K.bp_obs(10, K.BP_LEFT, 4)] * 2], obs_cap=1)
    assert "key the table lacks" in _host_call(keys, sets, opt, sample_obs=[[K.bp_obs(10, K.BP_LEFT, 4)]])
    assert "key the table lacks" in _host_call([K.key(10, K.BP_LEFT, n1=(3,))], sets, opt, sample_obs=[[K.bp_obs(10, K.BP_RIGHT, 4)]])
    o = capi.indel_candidate_options()
    assert list(o.papprox) == [0.0] * 18 and (o.min_candidate_indel_open_length, o.is_candidate_indel_signal_test, o.max_candidate_depth, o.log_indel_ref_error_factor) == (20, 1, -1.0, 0.0)
    assert (o.is_haplotyping_enabled, o.is_indel_ref_error_factor, o.is_sample_specific_rates, list(o.is_count_towards_depth_filter)) == (0, 0, 0, [1] * 8)
    assert _host_call(keys, sets, opt) == ""  # and the library goes on working


def test_device_entry_raises_the_flag_and_leaves_zeroed_output():
    if capi.lib().sk_broker_client():
        pytest.skip("not available to a broker client: the *_dev entry points need a GPU context of the caller's")
    capi.init(0)
    L = capi.lib()
    keys = K.sorted_keys([K.key(10, del_len=1, n1=(3,)), K.key(10, K.BP_LEFT, n1=(3,), n_bp_obs=2), K.key(12, ins="A", n1=(4,))])
    obs = [[K.bp_obs(10, K.BP_LEFT, 4), K.bp_obs(10, K.BP_LEFT, 22)]]
    d1, d2 = [_depth_at(64, 9, 20)], _zeros(1, 64)
    sets, opt = [K.ramp(), K.ramp()], K.options()
    want, totals = CM.indel_candidates(keys, obs, d1, d2, 0, sets, opt)
    assert totals[0] > 0

    def refused(**kw):
        res, n_samples = _dev_cand(keys, d1, d2, 0, 64, sets, kw.pop("sample_obs", obs), opt, **kw)
        assert L.sk_check_device_errors() != 0 and "sk_indel_candidates_dev" in capi.last_error() and L.sk_check_device_errors() == 0, kw
        assert not res["out"].view(np.uint8).any() and not res["rates"].view(np.uint8).any() and res["totals"] == [0, 0], kw

    for mutate in REFUSED_SETS:
        refused(mutate_sets=mutate)
    refused(key_cap=2)                                      # more keys on the device than the room
    refused(n_keys=-1)
    refused(obs_cap=1)                                      # the observations lie outside obs_cap
    refused(sample_obs=[obs[0] + [K.bp_obs(11, K.BP_LEFT, 9)]])  # a breakpoint observation without its key
    # what the host can read is refused with a message, as by the host entry: nothing is enqueued
    for bad_opt, n in ((CM.default_options(), 1), (K.options(), 9)):
        with pytest.raises(capi.StrelkaAmdError, match="papprox|SK_MAX_SAMPLES"):
            _dev_cand(keys, d1 * n, d2 * n, 0, 64, sets, obs * n, bad_opt)
    res, n_samples = _dev_cand(keys, d1, d2, 0, 64, sets, obs, opt, key_cap=3)  # exactly the room: enough
    capi._check(L.sk_check_device_errors())
    assert K.device_results(res, 1) == want and res["totals"] == totals


def test_candidates_behind_the_device_chain_on_one_stream():
    """per sample sk_read_intake_dev -> sk_region_haplotypes_dev -> sk_region_alleles_dev, then sk_indel_table_dev -> sk_read_depth_dev (per
    sample) -> sk_indel_candidates_dev, all on one stream with no host copy in between and the key count left on the device: the recorded
    two-sample scene under the germline configuration, against the model and against what the reference gave"""
    import torch
    if capi.lib().sk_broker_client():
        pytest.skip("not available to a broker client: the *_dev entry points need a GPU context of the caller's")
    from tests import indel_table_model as T
    from tests import test_region_haplotypes as RH
    capi.init(0)
    L = capi.lib()
    rec = next(s for s in CM.golden()["scenes"] if s["name"] == "two_samples_one_deletion@germline")
    sc = CM.scene_document(rec)
    samples, regions = T.scene_samples(sc)
    keys, depth, want, want_totals = CM.run_recorded(rec)
    assert CM.as_recorded(keys, want) == rec["keys"] and want_totals[0] > 0
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
    for sm in samples:
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
                 depth2=torch.full((n_pos + 1,), -1, dtype=torch.int32, device="cuda"), dscratch=torch.zeros(depth_scratch_bytes, dtype=torch.uint8, device="cuda"))
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
    out = dict(keys=torch.zeros(key_cap * 56, dtype=torch.uint8, device="cuda"), data=torch.zeros(key_cap * n_samples * 64, dtype=torch.uint8, device="cuda"),
               ids=torch.zeros(id_cap, dtype=torch.int32, device="cuda"), ins=torch.zeros(ins_cap, dtype=torch.uint8, device="cuda"),
               totals=torch.full((4,), -1, dtype=torch.int64, device="cuda"), cand=torch.full((key_cap * 8,), 0x5a, dtype=torch.uint8, device="cuda"),
               rates=torch.full((key_cap * n_samples * 32,), 0x5a, dtype=torch.uint8, device="cuda"), ctotals=torch.full((2,), -1, dtype=torch.int64, device="cuda"))
    scratch_bytes = L.sk_indel_table_scratch_bytes(n_samples, expand_cap, region_cap)
    scratch = torch.zeros(scratch_bytes, dtype=torch.uint8, device="cuda")
    c_scratch_bytes = L.sk_indel_candidates_scratch_bytes()
    c_scratch = torch.zeros(c_scratch_bytes, dtype=torch.uint8, device="cuda")
    capi._check(L.sk_indel_table_dev(n_samples, C.addressof(arr), keep[0][0]["ref"].data_ptr(), sc["ref_offset"], len(sc["ref"]), d_regions.data_ptr(), d_n.data_ptr(), region_cap,
                                     sc["prev_end_in"], expand_cap, out["keys"].data_ptr(), key_cap, out["data"].data_ptr(), out["ids"].data_ptr(), id_cap, out["ins"].data_ptr(),
                                     ins_cap, out["totals"].data_ptr(), scratch.data_ptr(), scratch_bytes, st))
    cstructs = []
    for d, x, n, n_segs, cap in keep:
        t = d["t"]
        capi._check(L.sk_read_depth_dev(n, t[2].data_ptr(), t[3].data_ptr(), t[4].data_ptr(), n_segs, t[5].data_ptr(), x["iat"].data_ptr(), win_begin, n_pos,
                                        x["depth1"].data_ptr(), x["depth2"].data_ptr(), x["dscratch"].data_ptr(), depth_scratch_bytes, st))
        cstructs.append(capi.IndelCandidateSample(n, 0, x["obs_off"].data_ptr(), x["obs"].data_ptr(), cap, x["depth1"].data_ptr(), x["depth2"].data_ptr()))
    carr = (capi.IndelCandidateSample * n_samples)(*cstructs)
    o = K.capi_options(copt)
    capi._check(L.sk_indel_candidates_dev(n_samples, C.addressof(carr), win_begin, n_pos, out["keys"].data_ptr(), out["data"].data_ptr(), out["totals"].data_ptr(), key_cap,
                                          d_sets.data_ptr(), C.addressof(o), out["cand"].data_ptr(), out["rates"].data_ptr(), out["ctotals"].data_ptr(), c_scratch.data_ptr(),
                                          c_scratch_bytes, st))
    torch.cuda.synchronize()
    capi._check(L.sk_check_device_errors())
    nk = int(out["totals"].cpu().numpy()[0])
    assert nk == len(keys)
    for (d, x, n, n_segs, cap), (w1, w2) in zip(keep, depth):
        assert x["depth1"].cpu().numpy().view(np.uint32)[:n_pos].tolist() == w1.tolist() and x["depth2"].cpu().numpy().view(np.uint32)[:n_pos].tolist() == w2.tolist()
    res = dict(out=out["cand"].cpu().numpy().view(capi.INDEL_CANDIDATE_DTYPE), rates=out["rates"].cpu().numpy().view(capi.INDEL_ERROR_RATES_DTYPE))
    got = K.device_results(dict(out=res["out"][:nk], rates=res["rates"][:nk * n_samples]), n_samples)
    assert got == want and out["ctotals"].cpu().numpy().tolist() == want_totals
    assert not res["out"][nk:].view(np.uint8).any() and not res["rates"][nk * n_samples:].view(np.uint8).any()
