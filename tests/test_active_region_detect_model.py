"""Active regions without a device: the loop model (tests/anchor_model.py) against the vectors recorded from the reference
(tests/golden/active_region_detect/, made by tools/golden/active_region_driver.cpp), the two closed forms of the repeat finder against
the loop model, the inputs the device tests rely on, and the C-ABI's host side (bound, exports, argument checks)."""
import numpy as np
import pytest

from strelka_amd import capi
from tests import active_region_cases as R
from tests import anchor_model as A
from tests import intake_cases as K


# ---- the model against the reference's own numbers ------------------------------------------------------------------------------------------


def test_unit_test_string_of_the_reference():
    """_ref = TATATACCCCCAATGAAAAA (ReferenceRepeatFinder.hh:76-77): anchors 11 to 14, _repeatSpan[5][1] = 6 and [5][2] = 3"""
    anchors, rows = A.ref_anchors("TATATACCCCCAATGAAAAA", 0, 0, None, 0, 20, [5])
    assert [i for i, x in enumerate(anchors) if x] == [11, 12, 13, 14]
    assert rows[0][1] == 6 and rows[0][2] == 3


def test_model_reproduces_the_recorded_finders():
    finders = R.golden()["finders"]
    assert [f["name"] for f in finders] == ["unit_test", "segment_start", "fresh_then_used"]
    assert [len(f["regions"]) for f in finders] == [1, 1, 3]
    n_pos = 0
    for f in finders:
        finder = A.RepeatFinder(f["ref"], f["ref_offset"])  # one object for all its regions, ring and all
        for k, reg in enumerate(f["regions"]):
            m = A.min_pos(reg["init_pos"], f["ref_offset"])
            assert m == reg["m"]
            assert finder.row(m - 1) == reg["init_span"], (f["name"], k)  # the stale slot, before initRepeatSpan
            last = m + len(reg["anchors"]) - 1
            got_m, anchors, rows = A.run_region(finder, reg["init_pos"], last, reg["span_pos"])
            assert anchors == reg["anchors"], (f["name"], k)
            assert rows == reg["span_rows"], (f["name"], k)
            # ... and as a function of the reference and the 50 stale values alone, which is what sk_ref_anchors takes
            anchors2, rows2 = A.ref_anchors(f["ref"], f["ref_offset"], reg["init_pos"], reg["init_span"], m, len(reg["anchors"]), reg["span_pos"])
            assert anchors2 == reg["anchors"] and rows2 == reg["span_rows"], (f["name"], k)
            assert A.closed_form_anchors(f["ref"], f["ref_offset"], reg["init_pos"], reg["init_span"], m, len(reg["anchors"])) == reg["anchors"]
            n_pos += len(reg["anchors"])
    assert n_pos > 2500
    used = finders[2]["regions"]
    assert not any(used[0]["init_span"]) and max(used[1]["init_span"]) > 0 and max(used[2]["init_span"]) > 0
    assert used[2]["init_span"][0] >= 2  # (u = 1: the trigger value 2u is stepped over; the third region begins inside a homopolymer)
    # the stale slot matters: a fresh finder answers differently on the third region
    for reg in used[1:]:
        fresh, _ = A.ref_anchors(finders[2]["ref"], finders[2]["ref_offset"], reg["init_pos"], None, reg["m"], len(reg["anchors"]))
        assert fresh[:2] == [1, 1] and reg["anchors"][:2] == [0, 0] and fresh[2:] == reg["anchors"][2:]


def test_model_reproduces_the_recorded_walks():
    walks = R.golden()["walks"]
    assert [w["name"] for w in walks] == ["from_zero", "inside"] and walks[0]["win_begin"] == 0
    for w in walks:
        g = R.recorded_walk(w)
        trace = []
        regions, state = A.active_regions(g["win_begin"], g["depth"], g["is_candidate"], g["is_anchor"], trace=trace)
        assert regions == g["regions"] and len(regions) >= 8
        assert [s for s, _ in trace] == g["states"]
        assert state == g["states"][-1]
        # the flags the detector saw are the intake's and the finder's
        depth, cand, anchor = R.walk_flags(w["ref"], w["ref_offset"], g["win_begin"], g["sites"])
        assert cand == g["is_candidate"] and anchor == g["is_anchor"]
        assert [int(d == 0) for d in depth] == [c[1] for c in w["calls"]]
        assert sum(1 for c in w["calls"] if c[0] and c[1]) > 20  # depth-zero candidates


# ---- the closed forms ------------------------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("seed", range(8))
def test_closed_forms_equal_the_loop_model(seed):
    rng = np.random.default_rng(9100 + seed)
    ref = K.repeat_rich_reference(1300, rng)
    ref_offset = int(rng.integers(0, 400))
    init_pos = ref_offset + int(rng.integers(0, 300))
    init = None if seed % 2 == 0 else [int(x) for x in rng.integers(0, 130, A.MAX_REPEAT_UNIT)]
    m = A.min_pos(init_pos, ref_offset)
    n = ref_offset + len(ref) + 60 - m
    loop, _ = A.ref_anchors(ref, ref_offset, init_pos, init, m, n)
    assert 0.1 * n < sum(loop) < 0.9 * n
    assert A.closed_form_anchors(ref, ref_offset, init_pos, init, m, n) == loop
    assert A.tract_form_anchors(ref, ref_offset, m + 100, n - 100) == loop[100:]


def test_second_region_on_a_used_finder_equals_the_function_of_its_stale_slot():
    rng = np.random.default_rng(9200)
    ref = K.repeat_rich_reference(2600, rng)
    finder = A.RepeatFinder(ref, 0)
    A.run_region(finder, 40, 700)
    for init_pos in (1300, 2100):
        m = A.min_pos(init_pos, 0)
        stale = finder.row(m - 1)
        _, anchors, rows = A.run_region(finder, init_pos, init_pos + 300, [m, init_pos + 300])
        assert (anchors, rows) == A.ref_anchors(ref, 0, init_pos, stale, m, init_pos + 301 - m, [m, init_pos + 300])
        assert A.closed_form_anchors(ref, 0, init_pos, stale, m, len(anchors)) == anchors


# ---- the inputs of the device tests --------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("u", [1, 2, 3, 7, 49, 50])
def test_tract_of_2u_is_a_repeat_and_of_2u_minus_1_is_not(u):
    at = R.TRACT_AT
    short, _ = A.ref_anchors(R.tract_reference(u, 2 if u == 1 else 2 * u - 1), 0, 0, None, 0, R.TRACT_REF_LEN)
    full, _ = A.ref_anchors(R.tract_reference(u, 3 if u == 1 else 2 * u), 0, 0, None, 0, R.TRACT_REF_LEN)
    assert all(short)
    assert [i for i, x in enumerate(full) if not x] == list(range(at, at + (3 if u == 1 else 2 * u)))


def test_period_51_is_no_repeat():
    assert all(A.ref_anchors(R.tract_reference(51, 153), 0, 0, None, 0, R.TRACT_REF_LEN)[0])


@pytest.mark.parametrize("n,seed", [(200, None), (1500, 32), (4096, 33), (16385, 34)])
def test_seeded_walk_inputs_give_regions_and_depth_zero_candidates(n, seed):
    g = R.dense_walk(n) if seed is None else R.seeded_walk(n, seed)
    trace = []
    regions, _ = A.active_regions(g["win_begin"], g["depth"], g["is_candidate"], g["is_anchor"], trace=trace)
    assert len(regions) >= 8
    assert sum(1 for c, d in zip(g["is_candidate"], g["depth"]) if c and d == 0) >= 1
    # a depth-zero candidate met with a region open (it counts) and one met with none open (it does not)
    before = [A.initial_state()] + [s for s, _ in trace[:-1]]
    zero = [(s["num_variants"] > 0) for s, c, d in zip(before, g["is_candidate"], g["depth"]) if c and d == 0]
    assert any(zero) and not all(zero)


def test_assertion_of_create_active_region_is_modelled():
    with pytest.raises(A.AssertionFailed):
        A.active_regions(50, [10] * 40, [0] * 40, [1] * 40, R.UNREACHABLE_STATE)
    assert A.active_regions(50, [10] * 8, [0] * 8, [1] * 8, R.UNREACHABLE_STATE)[0] == []  # (no event yet more than 13 past the last variant)


# ---- the C-ABI's host side -------------------------------------------------------------------------------------------------------------------------------


def test_new_symbols_are_declared_and_exported(built):
    from tests.test_abi import declared_symbols
    new = {"sk_ar_state_initial", "sk_ref_anchors", "sk_ref_anchors_dev", "sk_active_regions_bound", "sk_active_regions", "sk_active_regions_dev"}
    assert new <= set(declared_symbols())
    assert new <= set(capi.EXPORTS)
    for name in new:
        assert hasattr(capi.lib(), name)
    assert capi.AR_STATE_DTYPE.itemsize == 24 and capi.ACTIVE_REGION_DTYPE.itemsize == 12 and capi.REPEAT_MAX_UNIT == A.MAX_REPEAT_UNIT


def test_bound_and_initial_state_are_host_arithmetic(built):
    assert [capi.active_regions_bound(n) for n in (0, 1, 2, 3, 8192, 2 ** 31 - 1)] == [1, 1, 2, 2, 4097, 2 ** 30]
    assert capi.lib().sk_active_regions_bound(-1) == -1
    s = capi.ar_state_initial()
    assert {k: int(s[k][0]) for k in capi.AR_STATE_DTYPE.names} == A.initial_state()


def test_arguments_are_checked(built):
    """every refusal comes with its message, with or without a device (the checks run before the device is asked for)"""
    L = capi.lib()
    ref = b"ACGT" * 100
    anchor = np.zeros(600, np.uint8)
    rows = np.zeros((4, 50), np.uint32)
    p = capi._p

    def anchors(ref_offset=1000, ref_len=400, init_pos=1200, win_begin=1101, n_pos=100, n_span=0, span=(0, 0)):
        sp = np.array(span, np.int32)
        rc = L.sk_ref_anchors(ref, ref_offset, ref_len, init_pos, None, win_begin, n_pos, p(anchor), n_span, p(sp), p(rows))
        return rc, capi.last_error()

    for kw, word in ((dict(win_begin=1100), "win_begin is before"), (dict(init_pos=1050, win_begin=999), "win_begin is before"), (dict(n_pos=-1), "negative"),
                     (dict(ref_len=-1), "negative"), (dict(n_span=-1), "negative"), (dict(ref_offset=-1), "negative"),
                     (dict(n_span=2, span=(1101, 1100)), "span_pos[1]"), (dict(win_begin=2 ** 31 - 150, n_pos=100), "beyond int32"),
                     (dict(init_pos=2 ** 31 - 50, win_begin=2 ** 31 - 149, n_pos=1), "beyond int32"), (dict(init_pos=-2 ** 31 + 10), "beyond int32"),
                     (dict(ref_offset=2 ** 31 - 100), "beyond int32")):
        rc, msg = anchors(**kw)
        assert rc != 0 and word in msg, (kw, msg)
    assert L.sk_ref_anchors(None, 0, 10, 0, None, 0, 1, p(anchor), 0, None, None) != 0 and "null" in capi.last_error()
    assert L.sk_ref_anchors_dev(ref, 1000, 400, 1200, None, 1100, 10, p(anchor), 0, None, None, None) != 0 and "win_begin is before" in capi.last_error()

    sites = np.zeros(16, capi.INTAKE_SITE_DTYPE)
    flags = np.zeros(16, np.uint8)
    out = np.zeros(1, capi.AR_STATE_DTYPE)
    regions = np.zeros(16, capi.ACTIVE_REGION_DTYPE)
    n_regions = np.zeros(1, np.int32)

    def walk(win_begin=10, n_pos=10, cap=None, state=None):
        state = capi.ar_state_initial() if state is None else state
        cap = capi.active_regions_bound(max(n_pos, 0)) if cap is None else cap
        rc = L.sk_active_regions(win_begin, n_pos, p(sites), p(flags), p(flags), p(state), p(out), p(regions), cap, p(n_regions))
        return rc, capi.last_error()

    unreachable = capi.ar_state(dict(A.initial_state(), is_beginning=0, num_variants=2, active_region_start_pos=30, anchor_pos_following_prev_variant=30))
    for kw, word in ((dict(cap=5), "region_cap"), (dict(win_begin=-1), "win_begin below zero"), (dict(n_pos=-1), "negative"), (dict(cap=-1), "negative"),
                     (dict(win_begin=2 ** 31 - 5, n_pos=10), "beyond int32"), (dict(state=unreachable), "createActiveRegion")):
        rc, msg = walk(**kw)
        assert rc != 0 and word in msg, (kw, msg)
    assert L.sk_active_regions(0, 1, None, None, None, None, None, None, 1, None) != 0 and "null" in capi.last_error()
    assert L.sk_active_regions_dev(0, 4, p(sites), p(flags), p(flags), p(out), p(out), p(regions), 2, p(n_regions), None) != 0 and "region_cap" in capi.last_error()


def test_no_cpu_fallback(built):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(capi.StrelkaAmdError) as e:
        capi.ref_anchors("ACGTACGT", 0, 0, None, 0, 8)
    assert "sk_init" in str(e.value)
    with pytest.raises(capi.StrelkaAmdError) as e:
        capi.active_regions(0, np.zeros(4, capi.INTAKE_SITE_DTYPE), [0] * 4, [1] * 4)
    assert "sk_init" in str(e.value)
