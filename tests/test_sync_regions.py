"""The synchronised walk on the device (sk_sync_active_regions, csrc/active_region_detect.hip): every byte of every output equals the call
by call model (tests/sync_model.py, itself pinned to vectors recorded from the reference's ActiveRegionDetector by
tests/test_sync_regions_model.py)."""
import ctypes as C
import functools

import numpy as np
import pytest

from strelka_amd import capi
from tests import active_region_cases as R
from tests import anchor_model as A
from tests import sync_cases as K
from tests import sync_model as S

pytestmark = pytest.mark.gpu

CHUNK = 4096  # AR_SYNC_CHUNK: positions the walk takes per turn
N_POS_EDGES = [1, 63, 64, 65, CHUNK - 1, CHUNK, CHUNK + 1]


def _sites(depth):
    a = np.zeros((len(depth), len(depth[0]) if depth else 0), capi.INTAKE_SITE_DTYPE)
    a["depth"] = np.asarray(depth, np.uint32).reshape(a.shape)
    return a


def _region_dicts(regions, n_samples):
    out = []
    for r in regions:
        assert r["ploidy"][n_samples:].tolist() == [0] * (capi.MAX_SAMPLES - n_samples) and int(r["pad"]) == 0
        out.append(dict(begin=int(r["begin"]), end=int(r["end"]), closed_at=int(r["closed_at"]), prev_end=int(r["prev_end"]),
                        ploidy=[int(x) for x in r["ploidy"][:n_samples]], sample_mask=int(r["sample_mask"])))
    return out


def _full_state(state):
    """a model state with fewer than eight samples -> the one the device carries"""
    return dict(state, samples=list(state["samples"]) + [A.initial_state() for _ in range(capi.MAX_SAMPLES - len(state["samples"]))])


def _sync(win_begin, depth, cand, anchor, marks=None, default_ploidy=2, state=None, do_clear=False, buf_begin=None, buf_end=None, what=""):
    """device against model -> (regions, state_out, region_id) of the model; state: a model state"""
    capi.init(0)
    n_samples = len(depth)
    want_regions, want_state, want_id = S.sync_active_regions(win_begin, depth, cand, anchor, marks, default_ploidy, state, do_clear, buf_begin, buf_end)
    got_regions, got_state, got_id = capi.sync_active_regions(win_begin, _sites(depth), cand, anchor, marks, default_ploidy,
                                                              None if state is None else capi.sync_state(_full_state(state)), do_clear, buf_begin, buf_end)
    assert _region_dicts(got_regions, n_samples) == want_regions, what
    assert capi.sync_state_dict(got_state) == _full_state(want_state), what
    assert got_id.tolist() == want_id, what
    return want_regions, want_state, want_id


def _flags(n_samples, n, cand=None, depth=20):
    """n positions, all ring anchors of depth 20, candidates as {sample: window offsets}"""
    c = [[0] * n for _ in range(n_samples)]
    for s, at in (cand or {}).items():
        for i in at:
            c[s][i] = 1
    return [[depth] * n for _ in range(n_samples)], c, [1] * n


# ---- the rules, one by one -----------------------------------------------------------------------------------------------------------------------------


def test_a_region_closes_at_the_first_call_nine_past_its_end():
    # candidates at 120 and 123: the anchor 137, 14 past the last one, makes [119, 125) at call 138 and becomes the start in the same call;
    # call 139 is past end + 9 and finds no start below end - 1
    regions, _, region_id = _sync(100, *_flags(1, 60, {0: (20, 23)}), what="one sample")
    assert regions == [dict(begin=119, end=125, closed_at=139, prev_end=-1, ploidy=[2], sample_mask=1)]
    assert [i for i, v in enumerate(region_id) if v == 119] == list(range(19, 25)) and set(region_id) == {-1, 119}
    # the window ends with the call that makes it: it stays open in the state, and the next window's first call closes it
    regions, state, _ = _sync(100, *_flags(1, 38, {0: (20, 23)}), what="made by the last call")
    assert regions == [] and (state["sync_begin"], state["sync_end"], state["sample_mask"]) == (119, 125, 1)
    regions, _, _ = _sync(138, *_flags(1, 5), state=state, what="the window after")
    assert [(r["begin"], r["end"], r["closed_at"]) for r in regions] == [(119, 125, 139)]
    # a region whose end is less than nine before the call that makes it waits: no anchor from 124 to 139, so the end is 141, made at
    # call 142 and closed by the first call nine past its end
    d, c, a = _flags(1, 80, {0: (20, 23)})
    for i in range(24, 40):
        a[i] = 0
    regions, _, _ = _sync(100, d, c, a, what="a late end")
    assert [(r["begin"], r["end"], r["closed_at"]) for r in regions] == [(119, 141, 150)]
    # the other sample's quiet start does not hold it
    regions, _, _ = _sync(100, *_flags(2, 60, {1: (20, 23)}), what="two samples, one quiet")
    assert [(r["begin"], r["end"], r["closed_at"], r["sample_mask"]) for r in regions] == [(119, 125, 139, 2)]


def test_another_samples_open_start_holds_the_close():
    # sample 1's candidates run from 110 to 170, ten apart: its start 109 lies below sample 0's end - 1 until its own region is made
    d, c, a = _flags(2, 120, {0: (20, 23), 1: tuple(range(10, 71, 10))})
    regions, _, _ = _sync(100, d, c, a, what="held")
    assert [(r["begin"], r["end"], r["sample_mask"]) for r in regions] == [(109, 172, 3)]
    assert regions[0]["closed_at"] > 125 + S.MAX_ASSEMBLY_PADDING + 20


def test_a_samples_second_region_merges_into_its_own_first():
    d, c, a = _flags(2, 160, {0: (20, 23, 50, 53), 1: tuple(range(10, 101, 10))})
    regions, _, _ = _sync(100, d, c, a, what="own merge")
    assert [(r["begin"], r["end"], r["sample_mask"]) for r in regions] == [(109, 202, 3)]


def test_regions_over_250_positions_get_no_ids():
    d, c, a = _flags(1, 400, {0: tuple(range(20, 300, 10)) + (350, 352)})
    regions, _, region_id = _sync(100, d, c, a, what="long")
    assert [(r["end"] - r["begin"] > 250) for r in regions] == [True, False]
    assert set(region_id[:340]) == {-1} and region_id[351] == regions[1]["begin"]


def test_ploidy_is_the_larger_of_the_two_ends():
    d, c, a = _flags(3, 60, {0: (20, 23)})
    marks = [[(119, 1), (124, 1)], [(119, 1)], [(118, 1), (120, 1), (125, 1)]]
    regions, _, _ = _sync(100, d, c, a, marks, what="marks")
    assert regions[0]["ploidy"] == [1, 2, 2]
    regions, _, _ = _sync(100, d, c, a, [[(119, 2)], [(124, 2)], []], default_ploidy=1, what="default 1")
    assert regions[0]["ploidy"] == [2, 2, 1]


def test_clear_through_every_branch():
    # made with both ends known; made with the end from the buffer; made with the start from the buffer; kept (both unknown, empty buffer)
    d, c, a = _flags(4, 40, {0: (30, 33), 1: (36, 39), 2: (30, 33)})
    regions, state, _ = _sync(100, d, c, a, do_clear=True, buf_begin=[100] * 4, buf_end=[141] * 4, what="clear")
    assert [(r["begin"], r["end"], r["closed_at"], r["sample_mask"]) for r in regions] == [(129, 141, capi.SYNC_CLOSED_AT_CLEAR, 7)]
    assert all(sd["active_region_start_pos"] == -1 and sd["is_beginning"] == 0 for sd in state["samples"][:4])
    undetermined = dict(A.initial_state(), is_beginning=0, prev_variant_pos=138, num_variants=2)
    st = dict(S.initial_state(2), samples=[dict(undetermined), dict(undetermined)])
    regions, state, _ = _sync(140, [[], []], [[], []], [], state=st, do_clear=True, buf_begin=[130, 141], buf_end=[141, 141], what="clear, undetermined")
    assert [(r["begin"], r["end"], r["sample_mask"]) for r in regions] == [(130, 141, 1)]
    # a detector that never took a call is left alone
    regions, state, _ = _sync(140, [[]], [[]], [], do_clear=True, buf_begin=[0], buf_end=[0], what="clear at the beginning")
    assert regions == [] and state["samples"][0]["is_beginning"] == 1


# ---- the recorded vectors ------------------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("name", ["one_sample", "two_samples", "three_samples", "eight_samples"])
def test_recorded_vectors(name):
    item = next(it for it in K.golden() if it["name"] == name)
    state = None
    for k, w in enumerate(K.replay(item)["windows"]):
        assert state is None or state == w["state_in"]
        _, state, _ = _sync(w["win_begin"], w["depth"], w["cand"], w["anchor"], w["marks"], w["default_ploidy"], state, w["do_clear"], w["buf_begin"], w["buf_end"],
                            what="%s window %d" % (name, k))
        assert state == w["state_out"]


# ---- sizes, chaining -------------------------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("n_samples", [1, 2, 8])
@pytest.mark.parametrize("n_pos", N_POS_EDGES)
def test_window_sizes_at_the_edges(n_pos, n_samples):
    g = K.seeded(n_samples, n_pos, 40 + n_samples)
    regions, _, _ = _sync(g["win_begin"], g["depth"], g["cand"], g["anchor"], g["marks"], what="n_pos %d, %d samples" % (n_pos, n_samples))
    if n_pos >= CHUNK - 1:
        assert len(regions) >= 8
    b = [g["win_begin"]] * n_samples
    _sync(g["win_begin"], g["depth"], g["cand"], g["anchor"], g["marks"], do_clear=True, buf_begin=b, buf_end=[g["win_begin"] + n_pos + 1] * n_samples, what="with clear()")


@functools.lru_cache(maxsize=None)
def _chained_case():
    """a window of three samples with the calls after which a synchronised region is open: inside its nine positions of padding, and
    past them (held by a sample's start)"""
    g = K.seeded(3, 1500, 77)
    trace = []
    whole = S.sync_active_regions(g["win_begin"], g["depth"], g["cand"], g["anchor"], g["marks"], trace=trace)
    in_padding = [k + 1 for k, (st, _) in enumerate(trace) if st["sync_end"] and g["win_begin"] + k + 1 < st["sync_end"] + S.MAX_ASSEMBLY_PADDING]
    held = [k + 1 for k, (st, _) in enumerate(trace) if st["sync_end"] and g["win_begin"] + k + 1 >= st["sync_end"] + S.MAX_ASSEMBLY_PADDING]
    return g, whole, in_padding, held


def test_one_window_equals_windows_chained_through_the_state():
    g, (whole, whole_state, _), in_padding, held = _chained_case()
    assert len(whole) >= 10 and len(in_padding) >= 3 and len(held) >= 10
    n = len(g["anchor"])
    for cuts in ([in_padding[0]], [held[0]], [held[len(held) // 2], in_padding[-1]], [1, 64, 65], sorted({in_padding[1], held[3], held[-1]})):
        got, state = [], None
        for a, b in zip([0] + cuts, cuts + [n]):
            r, state, _ = _sync(g["win_begin"] + a, [d[a:b] for d in g["depth"]], [c[a:b] for c in g["cand"]], g["anchor"][a:b], g["marks"], state=state,
                                what="cuts %s" % cuts)
            got += r
        assert got == whole and state == whole_state, cuts


def test_host_entry_equals_device_entry_and_the_state_may_be_in_place():
    import torch
    if capi.lib().sk_broker_client():
        pytest.skip("not available to a broker client: the *_dev entry points need a GPU context of the caller's")
    capi.init(0)
    L = capi.lib()
    n_samples, n_pos = 3, 1500
    g = K.seeded(n_samples, n_pos, 77)
    sites = _sites(g["depth"])
    cand, anchor = np.array(g["cand"], np.uint8), np.array(g["anchor"], np.uint8)
    b, e = [g["win_begin"]] * n_samples, [g["win_begin"] + n_pos + 1] * n_samples
    host_regions, host_state, host_id = capi.sync_active_regions(g["win_begin"], sites, cand, anchor, g["marks"], 2, None, True, b, e)
    assert len(host_regions) >= 10
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    p = lambda t: C.c_void_p(t.data_ptr())
    mark_off, marks = capi.pack_ploidy_marks(g["marks"], n_samples)
    cap = capi.sync_regions_bound(n_pos)
    t = [dev(sites.view(np.int64)), dev(cand), dev(anchor), dev(mark_off), dev(marks.view(np.int32))]
    d_state = dev(capi.sync_state_initial().view(np.int32))
    d_regions = torch.full(((cap + 1) * 8,), 0x5a5a5a5a, dtype=torch.int32, device="cuda")
    d_n = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    d_id = torch.full((n_pos + 8,), 7, dtype=torch.int32, device="cuda")
    bb, be = np.array(b, np.int32), np.array(e, np.int32)
    torch.cuda.synchronize()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    capi._check(L.sk_sync_active_regions_dev(n_samples, g["win_begin"], n_pos, p(t[0]), p(t[1]), p(t[2]), p(t[3]), p(t[4]), 2, p(d_state), p(d_state), 1, capi._p(bb), capi._p(be),
                                             p(d_regions), cap, p(d_n), p(d_id), st))
    torch.cuda.synchronize()
    capi._check(L.sk_check_device_errors())
    n = int(d_n.cpu()[0])
    assert n == len(host_regions)
    raw = d_regions.cpu().numpy()
    assert raw[:n * 8].tobytes() == host_regions.tobytes() and (raw[n * 8:] == 0x5a5a5a5a).all()  # (nothing past the count is written)
    assert d_state.cpu().numpy().tobytes() == host_state.tobytes()
    ids = d_id.cpu().numpy()
    assert ids[:n_pos].tobytes() == host_id.tobytes() and (ids[n_pos:] == 7).all()
    # no region_id wanted, an empty window, no clear: the state passes through
    capi._check(L.sk_sync_active_regions_dev(n_samples, g["win_begin"] + n_pos, 0, None, None, None, p(t[3]), p(t[4]), 2, p(d_state), p(d_state), 0, None, None,
                                             p(d_regions), 1, p(d_n), None, st))
    torch.cuda.synchronize()
    assert int(d_n.cpu()[0]) == 0 and d_state.cpu().numpy().tobytes() == host_state.tobytes()


def test_one_sample_with_uniform_ploidy_equals_the_detectors_own_regions():
    """S = 1 where the detector makes no region before the last one is closed: the synchronised list is sk_active_regions' list"""
    capi.init(0)
    g = R.seeded_walk(1500, 32)
    sites = np.zeros(len(g["sites"]), capi.INTAKE_SITE_DTYPE)
    for i, (c, d) in enumerate(g["sites"]):
        sites[i] = (c, d)
    own, own_state = capi.active_regions(g["win_begin"], sites, g["is_candidate"], g["is_anchor"])
    n = len(sites)
    regions, state, _ = capi.sync_active_regions(g["win_begin"], sites.reshape(1, n), [g["is_candidate"]], g["is_anchor"], do_clear=True, buf_begin=[g["win_begin"]],
                                                 buf_end=[g["win_begin"] + n + 1])
    closed_by_call = [r for r in regions if int(r["closed_at"]) != capi.SYNC_CLOSED_AT_CLEAR]
    assert len(own) >= 8 and len(closed_by_call) in (len(own), len(own) - 1)
    assert [(int(r["begin"]), int(r["end"])) for r in closed_by_call] == [(int(r["begin"]), int(r["end"])) for r in own[:len(closed_by_call)]]
    assert all(int(r["closed_at"]) > int(o["made_at"]) for r, o in zip(closed_by_call, own))
    assert all(r["ploidy"].tolist() == [2] + [0] * 7 and int(r["sample_mask"]) == 1 for r in regions)


# ---- refusals and assertions ---------------------------------------------------------------------------------------------------------------------------


def test_refused_inputs():
    capi.init(0)
    L = capi.lib()
    d, c, a = _flags(2, 40, {0: (20, 23)})
    sites = _sites(d)
    ok = lambda **kw: capi.sync_active_regions(100, sites, c, a, **kw)
    assert len(ok()[0]) == 1
    with pytest.raises(capi.StrelkaAmdError, match="n_samples"):
        capi.sync_active_regions(100, np.zeros((9, 4), capi.INTAKE_SITE_DTYPE), np.zeros((9, 4)), np.zeros(4))
    with pytest.raises(capi.StrelkaAmdError, match="region_cap"):
        ok(region_cap=capi.sync_regions_bound(40) - 1)
    with pytest.raises(capi.StrelkaAmdError, match="win_begin"):
        capi.sync_active_regions(-1, sites, c, a)
    with pytest.raises(capi.StrelkaAmdError, match="beyond int32"):
        capi.sync_active_regions(2 ** 31 - 30, sites, c, a)
    with pytest.raises(capi.StrelkaAmdError, match="ascending"):
        ok(marks=[[(120, 1), (119, 1)], []])
    with pytest.raises(capi.StrelkaAmdError, match="ascending"):
        ok(marks=[[], [(119, 1), (119, 2)]])
    for bad in (0, 3):
        with pytest.raises(capi.StrelkaAmdError, match="ploidy other than 1 or 2"):
            ok(marks=[[(119, bad)], []])
        with pytest.raises(capi.StrelkaAmdError, match="default_ploidy"):
            ok(default_ploidy=bad)
    with pytest.raises(capi.StrelkaAmdError, match="null argument"):
        ok(do_clear=True)
    z = np.zeros(64, np.int32)
    for n_samples, n_pos, cap, which in ((0, 4, 8, "n_samples"), (1, -1, 8, "negative size"), (1, 4, -1, "negative size")):
        rc = L.sk_sync_active_regions(n_samples, 100, n_pos, capi._p(z), capi._p(z), capi._p(z), capi._p(z), capi._p(z), 2, capi._p(capi.sync_state_initial()),
                                      capi._p(np.zeros(1, capi.SYNC_STATE_DTYPE)), 0, None, None, capi._p(np.zeros(8, capi.SYNC_REGION_DTYPE)), cap, capi._p(z), None)
        assert rc != 0 and which in capi.last_error()
    assert capi.sync_regions_bound(0) == 1 and capi.sync_regions_bound(16384) == 16385 and L.sk_sync_regions_bound(-1) == -1
    # as many regions as the bound allows for two positions would need more than positions can hold; one carried in and closed at once
    st = dict(S.initial_state(1), sync_begin=50, sync_end=60, sample_mask=1)
    regions, _, _ = _sync(100, [[20]], [[0]], [1], state=st, what="carried in")
    assert [(r["begin"], r["end"], r["closed_at"]) for r in regions] == [(50, 60, 101)]
    assert len(ok()[0]) == 1  # and the library goes on working


def test_assertions_are_an_error_return_not_a_fault():
    """createActiveRegion's assertion in a step and in clear(), closeActiveRegion's size() > 0: the host entry fails with the message and
    leaves its outputs alone; the device entry raises the sticky flag, gives no region and hands the state back"""
    import torch
    capi.init(0)
    L = capi.lib()
    d, c, a = _flags(1, 40)
    in_step = dict(S.initial_state(1), samples=[dict(R.UNREACHABLE_STATE)])
    in_clear = dict(S.initial_state(1), samples=[dict(A.initial_state(), is_beginning=0, active_region_start_pos=190, prev_anchor_pos=44, prev_variant_pos=45, num_variants=2)])
    empty_range = dict(S.initial_state(1), sync_begin=30, sync_end=20)
    cases = [(in_step, False), (in_clear, True), (empty_range, False)]
    for state, do_clear in cases:
        with pytest.raises(S.SyncAssertionFailed):
            S.sync_active_regions(50, d, c, a, state=state, do_clear=do_clear, buf_begin=[50], buf_end=[91])
        with pytest.raises(capi.StrelkaAmdError, match="assertion"):
            capi.sync_active_regions(50, _sites(d), c, a, state=capi.sync_state(_full_state(state)), do_clear=do_clear, buf_begin=[50], buf_end=[91])
        assert L.sk_check_device_errors() == 0  # (the host entry took the flag with it)
    _sync(50, [d[0][:8]], [c[0][:8]], a[:8], state=in_step, what="before the assertion's turn")
    if L.sk_broker_client():
        return
    p = lambda t: C.c_void_p(t.data_ptr())
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    t = [dev(_sites(d).view(np.int64)), dev(np.array(c, np.uint8)), dev(np.array(a, np.uint8)), dev(np.zeros(2, np.int32))]
    bad_marks = dev(np.array([(60, 1), (55, 1)], capi.PLOIDY_MARK_DTYPE).view(np.int32))
    bad_off = dev(np.array([0, 2], np.int32))
    bb, be = np.array([50], np.int32), np.array([91], np.int32)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for (state, do_clear), off, marks in [(cs, t[3], None) for cs in cases] + [((S.initial_state(1), False), bad_off, bad_marks)]:
        d_in = dev(capi.sync_state(_full_state(state)).view(np.int32))
        d_out = torch.full((52,), 77, dtype=torch.int32, device="cuda")
        d_regions = torch.zeros(41 * 8, dtype=torch.int32, device="cuda")
        d_n = torch.full((1,), 77, dtype=torch.int32, device="cuda")
        d_id = torch.full((40,), 77, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        capi._check(L.sk_sync_active_regions_dev(1, 50, 40, p(t[0]), p(t[1]), p(t[2]), p(off), None if marks is None else p(marks), 2, p(d_in), p(d_out), 1 if do_clear else 0,
                                                 capi._p(bb), capi._p(be), p(d_regions), 41, p(d_n), p(d_id), st))
        torch.cuda.synchronize()
        assert L.sk_check_device_errors() != 0 and "sk_sync_active_regions_dev" in capi.last_error()
        assert L.sk_check_device_errors() == 0
        assert int(d_n.cpu()[0]) == 0 and (d_id.cpu().numpy() == -1).all()
        assert d_out.cpu().numpy().tobytes() == d_in.cpu().numpy().tobytes()
