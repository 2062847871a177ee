"""Round sharing in F5 (flatten_score_kernel): a wave that has drawn dry scores whole rounds of a multi-round read owned
by a wave of its own block, from the owner's LDS object.  Who scores a round is a matter of timing; what is scored is not.

The scenario is tests/test_f5_tail_order.py's: distinct reads with 0, fewer than 64, 65-128, more than 128 and some 300 candidate
alignments, one whose window leaves the reference.  $SK_F5_GRID, $SK_F5_WAVES, $SK_F5_TAIL_SHIFT and $SK_F5_SHARE are read once per
process, so every shape is a child process of this file.

1. For every shape -- one wave to a block (no helper can exist), 2, 8 and 16 waves, two blocks with a tail table, the 256-base form with
   a 160-base read -- and job sizes 1 (the heaviest read alone in a block: more helpers than rounds), 2, W - 1, W, W + 1, 2 W + 3 (waves
   dry from the start; waves dry only after draws): F5's results (by repr), consulted flags and count of reference reads outside equal
   the host path's and the staged chain's, and a rescore of two repeats gives the same again.  With one wave to a block the counter of
   helped rounds (sk_debug_f5_shared_rounds) does not move; summed over the (1, 8, 0, 152) child's jobs it is at least 1 (the sum, not
   any one launch).
2. With $SK_F5_SHARE=0 the counter does not move on any job, and the results are the same.
3. One-read jobs of the reads nearest to 65, 128 and 129 candidate alignments (the scenario is not trimmed: the existing builders
   give no handle on a read's count; the counts are printed: 68 and 106 are what the scenario has).
4. A job whose indel table has more than 32 entries (tests/test_f5_prologue_cases.py's "big_table"): the table copy is written per
   round, so the read is not shared -- results equal the host's, the counter does not move.
5. A record outside the compact form (more than 16 segments or 8 indels) in a round AFTER a read's first: the long-read scenarios of
   tests/test_f5_phase_b_cases.py (5-9 indels and nine more inserts; four of the 24 hold such a read, as does the crafted eight-indel
   read of tests/test_f5_turn_ahead_cases.py; none of the 152-base scenarios of the two files and of tests/test_f5_prologue_cases.py
   does) are scanned for a job in which sk_debug_f5_late_turn_downs moves, and its reads, one to a job, for the read that does it.  That read then goes FIRST in a job of 3 W + 1 reads on a grid of one block
   ($SK_F5_GRID=1): its owner leaves it early and its next draw hands out a read -- it must have closed its claim word, or a wave that
   draws dry later scores the dead read's rounds over another read's data.  The job falls to the staged chain and equals the host's
   results, consulted flags and count of reference reads outside."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from strelka_amd import capi  # noqa: E402
from tests import f5_util as U  # noqa: E402
from tests import test_f5_prologue_cases as P  # noqa: E402  (scenario builders: here, and test_f5_phase_b_cases below)
from tests import test_f5_tail_order as T  # noqa: E402

_SHAPES = [  # (SK_F5_GRID, SK_F5_WAVES, SK_F5_TAIL_SHIFT, form)
    (1, 1, 0, 152), (1, 2, 0, 152), (1, 8, 0, 152), (2, 8, 3, 152), (1, 16, 0, 152), (1, 4, 1, 256), (3, 4, 0, 256)]


def _distinct(form):
    """the scenario, its distinct reads' host results and their candidate-alignment counts"""
    sc = T._tail_scenario(form == 256)
    one = U.run_chain(sc, "host", sc["reads"])
    assert all(r is not None for r in one["res"])
    n_cals = [eval(r, {"nan": float("nan"), "inf": float("inf")})["n_cals"] for r in one["res"]]
    print("candidate alignments of the distinct reads", n_cals, "outside", one["outside"])
    assert min(n_cals) == 0 and any(0 < c < 64 for c in n_cals) and any(64 < c <= 128 for c in n_cals) and any(c > 128 for c in n_cals)
    assert max(n_cals) > 256   # "about 300": five rounds
    assert one["outside"] > 0
    longest = max(len(rd["code"]) for rd in sc["reads"])
    assert longest == 160 if form == 256 else longest <= 152
    return sc, one, n_cals


def _child(mode, form):
    grid, waves = int(os.environ["SK_F5_GRID"]), int(os.environ["SK_F5_WAVES"])
    share_on = os.environ.get("SK_F5_SHARE", "1") != "0"
    capi.init(0)
    sc, one, n_cals = _distinct(form)
    k = len(sc["reads"])
    w = grid * waves
    total = 0
    if mode == "scores":
        heavy = sorted(range(k), key=lambda i: -n_cals[i])

        def job_of(n):
            if n <= 2:   # the heaviest read alone; the two heaviest
                idx = heavy[:n]
            else:        # the distinct reads in turn until n of them are the device job's (the read without alignments leaves at the gate)
                idx = []
                while sum(n_cals[i] > 0 for i in idx) < n:
                    idx.append(len(idx) % k)
            return [sc["reads"][i] for i in idx], [one["res"][i] for i in idx]

        for n in sorted({1, 2, w - 1, w, w + 1, 2 * w + 3} - {0}):
            reads, want = job_of(n)
            f5 = U.fresh_f5(sc, reads)
            host, staged = U.run_chain(sc, "host", reads), U.run_chain(sc, "staged", reads)
            again = U.fresh_f5(sc, reads, rescore=2)
            print("reads", n, "jobs", f5["jobs"], again["jobs"], "helped rounds", f5["shared"], again["shared"], "outside", host["outside"])
            assert host["res"] == want and f5["counts"][1] == again["counts"][1] == n
            for got, what in ((staged, "staged"), (f5, "f5"), (again, "again")):
                U.assert_same(got, host, (n, what))
            assert f5["jobs"] == (1, 0, 0) and again["jobs"] == (1, 0, 0)
            assert host["shared"] == 0 and staged["shared"] == 0
            total += f5["shared"] + again["shared"]
    elif mode == "edges":
        for target in (65, 128, 129):
            i = min(range(k), key=lambda q: (abs(n_cals[q] - target), q))
            reads = [sc["reads"][i]]
            f5, host, staged = U.fresh_f5(sc, reads), U.run_chain(sc, "host", reads), U.run_chain(sc, "staged", reads)
            print("nearest to", target, "candidate alignments:", n_cals[i], "helped rounds", f5["shared"])
            assert host["res"] == [one["res"][i]]
            U.assert_same(f5, host, target)
            U.assert_same(staged, host, target)
            assert f5["jobs"] == (1, 0, 0)
            total += f5["shared"]
    elif mode == "big_table":
        # the scenario's own job first: sharing works in this process (the counter moves), so that standing still below says something
        reads = [sc["reads"][i] for i in sorted(range(k), key=lambda i: -n_cals[i])[:2]] * 3
        for _ in range(3):
            total += U.fresh_f5(sc, reads)["shared"]
        big = [s for s in P._scenarios(96201, (30, 153), (200, 360), 6) if s["kind"] == "big_table"][0]
        assert len(big["indels"]) > P._TAB
        f5, host = U.fresh_f5(big, big["reads"]), U.run_chain(big, "host", big["reads"])
        print("big table:", len(big["indels"]), "entries,", len(big["reads"]), "reads, jobs", f5["jobs"], "helped rounds", f5["shared"])
        U.assert_same(f5, host, "big table")
        assert f5["shared"] == 0
    elif mode == "turned_down":
        from tests import test_f5_phase_b_cases as B
        late = capi.RealignJob.f5_late_turn_downs
        found = None
        for i, cand in enumerate(B._scenarios(95102, (153, 257), (330, 430), 24)):
            at = late()
            got = U.run_chain(cand, "f5", cand["reads"])
            print("scenario", i, "reads", got["counts"][1], "jobs", got["jobs"], "late turn-downs", late() - at)
            if late() > at and found is None:
                found = cand
        assert found is not None, "no scenario of tests/test_f5_phase_b_cases.py turns a read down in a round after its first"
        bad = []
        for i, rd in enumerate(found["reads"]):
            at = late()
            U.run_chain(found, "f5", [rd])
            if late() > at:
                bad.append(i)
        print("reads turned down in a later round:", bad)
        assert bad
        rest = [rd for i, rd in enumerate(found["reads"]) if i not in bad]
        for first in bad[:2]:
            reads = [found["reads"][first]]
            while len(reads) < 3 * w + 1:
                reads.append(rest[len(reads) % len(rest)])
            at = late()
            f5 = U.run_chain(found, "f5", reads)
            moved = late() - at
            host, staged = U.run_chain(found, "host", reads), U.run_chain(found, "staged", reads)
            print("job of", len(reads), "reads, read", first, "first: jobs", f5["jobs"], "late turn-downs", moved, "helped rounds", f5["shared"])
            assert moved > 0 and f5["jobs"] == (0, 1, 1)
            U.assert_same(f5, host, ("turned down", first))
            U.assert_same(staged, host, ("turned down, staged", first))
            total += f5["shared"]
        total = 0 if not share_on else total
    print("SHARED", total)
    if not share_on or waves == 1:
        assert total == 0
    print("SHARE-CHILD-OK")


def _spawn(mode, grid, waves, shift, form, share=None):
    out = U.spawn_child(__file__, mode, form, "SHARE-CHILD-OK", SK_F5_GRID=grid, SK_F5_WAVES=waves, SK_F5_TAIL_SHIFT=shift, SK_F5_SHARE=share)
    return int([ln for ln in out.splitlines() if ln.startswith("SHARED ")][-1].split()[1])


@pytest.mark.gpu
@pytest.mark.parametrize("grid,waves,shift,form", _SHAPES)
def test_scores_with_helpers(grid, waves, shift, form):
    shared = _spawn("scores", grid, waves, shift, form)
    if (grid, waves, shift, form) == (1, 8, 0, 152):
        assert shared >= 1   # (over the child's jobs: whether a particular round is helped is a matter of timing)
    if waves == 1:
        assert shared == 0


@pytest.mark.gpu
def test_sharing_off_counts_nothing():
    assert _spawn("scores", 1, 8, 0, 152, share="0") == 0


@pytest.mark.gpu
def test_reads_at_the_round_boundaries():
    _spawn("edges", 1, 8, 0, 152)


@pytest.mark.gpu
def test_big_table_is_not_shared():
    _spawn("big_table", 1, 8, 0, 152)


@pytest.mark.gpu
def test_read_turned_down_in_a_later_round_closes_its_word():
    _spawn("turned_down", 1, 4, 0, 256)


if __name__ == "__main__":
    _child(sys.argv[1], int(sys.argv[2]))
