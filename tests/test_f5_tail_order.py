"""The order of F5's last hand-outs (tail_order_kernel, flatten_score_kernel's tail_order / tail_first / tail_n).

1. The table the device builds (sk_debug_f5_tail_order) against its numpy statement, for small grids and shifts:
   first + argsort(arange(T) - (rounds - 1) * s, stable) over the window of the last T = min(n_reads, W + 6 s) hand-outs.  Beside
   equality: it is a permutation of [first, n_reads), every kind of read (by rounds) keeps its own order, and no read of c rounds
   stands in the last L_c places, L_c the lighter reads of the window that the shift puts behind the kind's last read (a read of
   q < c rounds at a position above i_last - (c - q) s).  The bound as first written down for this table -- the last
   min((c - 1) s, lighter reads in the window) places -- does not hold for the order it was written for: a tie goes to the lower
   position, so a heavy read that ends the window stands (c - 1) s - 1 places from the end, not (c - 1) s (with s = 1 a two-round
   read does not move at all), and lighter reads early in the window cannot stand behind a late heavy one ([1 round, 5 rounds,
   3 rounds], s = 1: keys 0, -3, 0, the three-round read stays last).  L_c counts exactly the lighter reads the order puts behind
   the kind's last read; for "only the last read is heavy" that is min((c - 1) s - 1, T - 1), and its place is asserted as well.
2. Scores through the table: a handful of distinct reads -- none, fewer than 64, more than 64 and more than 128 candidate alignments,
   one whose window leaves the reference -- tiled until n of them are the device job's, n around W, W + s and T, under six shapes of ($SK_F5_GRID, $SK_F5_WAVES,
   $SK_F5_TAIL_SHIFT), the shift-off one among them, in both forms of the kernel (152 bases; 256 bases, with one read of 160).  The
   three are read once per process, so each shape is a child process of this file.  F5's results, consulted flags and count of
   reference reads outside equal the host path's and the staged chain's; a rescore of two repeats gives the same again (each F5 job follows a job of another layout: the scores are not cleared in between); the job
   counts say F5 scored the job itself; and the table kernel was launched exactly for the jobs with n > W and s > 0.
3. The one-sequence and the staged driver give the same for such a job, each with one launch of the table kernel, and none for a
   job that fits the grid."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from strelka_amd import capi, synth  # noqa: E402
from tests import f5_util as U  # noqa: E402
from tests import test_f5_turn_ahead_cases as Q  # noqa: E402  (its scenario builders)

_CALS = (0, 1, 63, 64, 65, 128, 129, 256, 257, 400)


def _rounds(ncal):
    return np.clip((np.asarray(ncal) + 63) // 64, 1, 5)


def _model(ncal, waves, shift):
    """(first, order) as the issue states it"""
    n = len(ncal)
    if n <= waves or shift <= 0:
        return 0, np.zeros(0, np.int64)
    t = min(n, waves + 6 * shift)
    first = n - t
    rounds = _rounds(ncal[first:])
    return first, first + np.argsort(np.arange(t) - (rounds - 1) * shift, kind="stable")


def _check_table(ncal, waves, shift):
    ncal = np.asarray(ncal, np.int64)
    n = len(ncal)
    cal_off = np.concatenate([[0], np.cumsum(ncal)]).astype(np.int32)
    first, order = capi.RealignJob.f5_tail_order(cal_off, waves, shift)
    want_first, want = _model(ncal, waves, shift)
    where = "waves %d shift %d reads %d" % (waves, shift, n)
    assert first == want_first and len(order) == len(want), where
    assert np.array_equal(order, want), where
    if len(want) == 0:
        return 0
    t = len(order)
    assert t == min(n, waves + 6 * shift) and first == n - t, where
    assert np.array_equal(np.sort(order), np.arange(first, n)), where          # a permutation of the window
    rounds = _rounds(ncal)
    place = np.empty(n, np.int64)
    place[order] = np.arange(t)                                                   # (of the window's reads)
    win = np.arange(first, n)
    for c in range(1, 6):
        mine = win[rounds[win] == c]
        if len(mine) == 0:
            continue
        assert np.all(np.diff(place[mine]) > 0), (where, c)                       # the kind keeps its own order
        i_last = mine[-1] - first
        behind = sum(int(np.sum((rounds[win] == q) & (np.arange(t) > i_last - (c - q) * shift))) for q in range(1, c))
        if behind:
            assert np.all(rounds[order[t - behind:]] != c), (where, c, behind)
    return 1


@pytest.mark.gpu
@pytest.mark.parametrize("waves", [1, 8, 16])
def test_tail_table_equals_the_model(waves):
    capi.init(0)
    rng = np.random.default_rng(99100 + waves)
    n_tables = n_none = 0
    for shift in sorted({1, 3, waves // 2, waves}):
        t = waves + 6 * shift
        for n in (waves + 1, waves + shift, t - 1, t, t + 1, 3 * t + 7):
            if n < 1:   # (waves 1, shift 0: T - 1)
                continue
            ncal = rng.choice(_CALS, n)
            built = _check_table(ncal, waves, shift)
            n_tables += built
            n_none += not built
            # every read of one kind: the identity
            for one in (0, 64, 65, 400):
                first, order = capi.RealignJob.f5_tail_order(np.arange(n + 1, dtype=np.int32) * one, waves, shift)
                if n > waves and shift > 0:
                    assert np.array_equal(order, np.arange(first, n)) and first == n - min(n, t)
                else:
                    assert len(order) == 0
            # only the last read is heavy: it moves up to the light read with its key (a tie: behind that one), as far as the window goes
            for heavy in (65, 129, 257):
                ncal = np.full(n, 7)
                ncal[-1] = heavy
                if _check_table(ncal, waves, shift):
                    first, order = capi.RealignJob.f5_tail_order(np.concatenate([[0], np.cumsum(ncal)]).astype(np.int32), waves, shift)
                    c = int(_rounds(heavy))
                    assert list(order).index(n - 1) == max(0, len(order) - (c - 1) * shift)
    # a job that fits the grid, a shift of 0: no table
    for n, s in ((waves, 3), (waves - 1, 3), (4 * waves, 0)):
        if n > 0:
            first, order = capi.RealignJob.f5_tail_order(np.arange(n + 1, dtype=np.int32) * 70, waves, s)
            assert len(order) == 0
    print("waves", waves, "tables", n_tables, "without", n_none)
    assert n_tables >= 12 if waves > 1 else n_tables >= 6


# ---- jobs through the table: child processes

_SHAPES = [  # (SK_F5_GRID, SK_F5_WAVES, SK_F5_TAIL_SHIFT, form)
    (1, 1, 0, 152), (1, 1, 1, 152), (2, 8, 3, 152), (3, 1, 3, 152), (3, 8, 1, 256), (1, 8, 3, 256)]


def _tail_scenario(long_read):
    """a dense window (5-7 indels) whose reads have from 3 to some 300 candidate alignments; the reference is cut four bases
    into the leftmost read, so that its window leaves the reference, and extended to the right for a read far from every indel"""
    rng = np.random.default_rng(98107)
    sc = synth.realign_scenarios(2, rng, reads_per=14, max_indels=7, min_indels=5, read_len=(36, 100), window=(200, 260), haplotyping_rate=0.0)[1]
    picked = [sc["reads"][i] for i in (0, 1, 2, 5, 8, 9, 6)]
    cut = min(rd["pos"] for rd in picked) - sc["ref_offset"] + 4
    far = len(sc["ref_seq"]) + 200
    sc["ref_seq"] = sc["ref_seq"][cut:] + Q._seq(rng, 300)
    sc["ref_offset"] += cut
    sc["kind"] = "tail"
    picked.insert(3, Q._plain(sc, sc["ref_offset"] - cut + far, 32, rng))   # no indel near it: no candidate alignments
    if long_read:
        picked[5] = Q._plain(sc, sc["ref_offset"] + 20, 160, rng)
    sc["reads"] = picked
    return sc


def _child(mode, form):
    grid, waves, shift = (int(os.environ[k]) for k in ("SK_F5_GRID", "SK_F5_WAVES", "SK_F5_TAIL_SHIFT"))
    capi.init(0)
    sc = _tail_scenario(form == 256)
    k = len(sc["reads"])
    w = grid * waves
    t = w + 6 * shift
    one = U.run_chain(sc, "host", sc["reads"])
    assert all(r is not None for r in one["res"])
    n_cals = [eval(r, {"nan": float("nan"), "inf": float("inf")})["n_cals"] for r in one["res"]]
    print("candidate alignments of the distinct reads", n_cals, "outside", one["outside"])
    assert min(n_cals) == 0 and any(0 < c < 64 for c in n_cals) and any(64 < c <= 128 for c in n_cals) and any(c > 128 for c in n_cals)
    assert one["outside"] > 0
    longest = max(len(rd["code"]) for rd in sc["reads"])
    assert longest == 160 if form == 256 else longest <= 152

    def tiled(n):
        """the distinct reads in turn until n of them are the device job's (the read without candidate alignments leaves at the gate)"""
        idx = []
        while sum(n_cals[i] > 0 for i in idx) < n:
            idx.append(len(idx) % k)
        return [sc["reads"][i] for i in idx], [one["res"][i] for i in idx]

    if mode == "drivers":
        for n, table in ((2 * t + 5, 1), (w, 0)):
            reads, want = tiled(n)
            a, b = U.fresh_f5(sc, reads, one_wait="1"), U.fresh_f5(sc, reads, one_wait="0")
            print("reads", n, "one sequence", a["jobs"], a["launches"], "staged driver", b["jobs"], b["launches"])
            U.assert_same(a, b, n)
            assert a["res"] == want and a["counts"][1] == b["counts"][1] == n
            assert a["jobs"] == (1, 0, 0) and b["jobs"] == (0, 0, 1)
            assert a["launches"] == table and b["launches"] == table
        print("TAIL-CHILD-OK")
        return
    for n in sorted({w - 1, w, w + 1, w + shift + 1, t, t + 1, 2 * t + 5} - {0}):
        reads, want = tiled(n)
        f5 = U.fresh_f5(sc, reads)
        host, staged = U.run_chain(sc, "host", reads), U.run_chain(sc, "staged", reads)
        again = U.fresh_f5(sc, reads, rescore=2)
        print("reads", n, "jobs", f5["jobs"], again["jobs"], "table launches", f5["launches"], again["launches"], "outside", host["outside"])
        assert host["res"] == want and f5["counts"][1] == again["counts"][1] == n
        for got, what in ((staged, "staged"), (f5, "f5"), (again, "again")):
            U.assert_same(got, host, (n, what))
        assert f5["jobs"] == (1, 0, 0) and again["jobs"] == (1, 0, 0)
        assert staged["launches"] == 0 and host["launches"] == 0
        assert f5["launches"] == again["launches"] == int(n > w and shift > 0)
    print("TAIL-CHILD-OK")


def _spawn(mode, grid, waves, shift, form):
    U.spawn_child(__file__, mode, form, "TAIL-CHILD-OK", SK_F5_GRID=grid, SK_F5_WAVES=waves, SK_F5_TAIL_SHIFT=shift)


@pytest.mark.gpu
@pytest.mark.parametrize("grid,waves,shift,form", _SHAPES)
def test_scores_through_the_table(grid, waves, shift, form):
    _spawn("scores", grid, waves, shift, form)


@pytest.mark.gpu
def test_both_drivers_build_the_table_when_the_job_draws():
    _spawn("drivers", 2, 8, 3, 152)


if __name__ == "__main__":
    _child(sys.argv[1], int(sys.argv[2]))
