"""The repeat finder and the active-region detector's walk, restated loop by loop: the bit-exact reference for sk_ref_anchors and
sk_active_regions (csrc/active_region_detect.hip).

Two pieces of the reference (L/ = its src/c++/lib), with their loops kept as written:

  * ReferenceRepeatFinder                          L/starling_common/ReferenceRepeatFinder.cpp:26-80 (updateRepeatSpan, initRepeatSpan),
    the ring of 1 000 positions, the set-true-then-unset order, initRepeatSpan's write that updateRepeatSpan(m) overwrites from the
    stale slot (m - 1) % 1000, and the way ActiveRegionReadBuffer::setEndPos (ActiveRegionReadBuffer.cpp:173-189) drives it
  * SampleActiveRegionDetector::updateEndPosition  L/starling_common/ActiveRegionDetector.cpp:336-409 with createActiveRegion :314-328
    and clearCoordinates :296-303, the `not _activeRegionStartPos` test included

and, separately (closed_form_anchors, tract_form_anchors), the two closed forms of the finder that the kernels use.  The loop model
does not use them.

This module does not import the product."""
import numpy as np

MAX_REPEAT_UNIT = 50      # ActiveRegionReadBuffer.hh:72
MAX_BUFFER_SIZE = 1000    # ActiveRegionReadBuffer.hh:61
MIN_REPEAT_SPAN = 3       # ActiveRegionReadBuffer.hh:74
MAX_DISTANCE_BETWEEN_TWO_VARIANTS = 13  # ActiveRegionDetector.hh:141
MIN_NUM_VARIANTS_PER_REGION = 2         # ActiveRegionDetector.hh:144

U32 = 0xFFFFFFFF


def _i32(x):
    """(pos_t) of an unsigned value"""
    x &= U32
    return x - (1 << 32) if x & 0x80000000 else x


def _slot(pos):
    """pos % _maxBufferSize: an int against an unsigned, so the int converts first"""
    return (pos & U32) % MAX_BUFFER_SIZE


def min_pos(init_pos, ref_offset):
    """initRepeatSpan's minPos :62-64"""
    m = init_pos - 2 * MAX_REPEAT_UNIT + 1
    return ref_offset if m < ref_offset else m


class RepeatFinder:
    """ReferenceRepeatFinder over a reference_contig_segment"""

    def __init__(self, ref, ref_offset):
        self.ref, self.ref_offset = ref, ref_offset
        self.repeat_span = [[0] * MAX_REPEAT_UNIT for _ in range(MAX_BUFFER_SIZE)]
        self.anchor = [False] * MAX_BUFFER_SIZE

    def get_base(self, p):
        k = p - self.ref_offset
        return "N" if k < 0 or k >= len(self.ref) else self.ref[k]

    def is_anchor(self, pos):
        return self.anchor[_slot(pos)]

    def row(self, pos):
        return list(self.repeat_span[_slot(pos)])

    def update_repeat_span(self, pos):  # :26-58
        base = self.get_base(pos)
        pos_index = _slot(pos)
        self.anchor[pos_index] = True
        for unit in range(1, MAX_REPEAT_UNIT + 1):
            prev_base = self.get_base(pos - unit)
            unit_index = unit - 1
            if prev_base != "N" and base == prev_base:
                span = (self.repeat_span[_slot(pos - 1)][unit_index] + 1) & U32
            else:
                span = unit
            self.repeat_span[pos_index][unit_index] = span
            if span >= unit * 2 and span >= MIN_REPEAT_SPAN:
                if span == unit * 2 or span == MIN_REPEAT_SPAN:
                    prev_pos = pos - 1
                    stop = _i32(pos - span)
                    while prev_pos > stop:
                        self.anchor[_slot(prev_pos)] = False
                        prev_pos -= 1
                self.anchor[pos_index] = False

    def init_repeat_span(self, pos):  # :60-80
        m = min_pos(pos, self.ref_offset)
        pos_index = _slot(m)
        for unit in range(1, MAX_REPEAT_UNIT + 1):
            self.repeat_span[pos_index][unit - 1] = unit
        for init_pos in range(m, pos + MAX_REPEAT_UNIT * 2):
            self.update_repeat_span(init_pos)


def run_region(finder, init_pos, last_pos, span_pos=()):
    """One region on `finder` as setEndPos drives it: initRepeatSpan(init_pos), then updateRepeatSpan(pos + 100) per head position, until
    every position up to last_pos has been updated through itself + 101.  -> (m, anchors of m .. last_pos as the detector reads them, the
    rows of span_pos)"""
    m = min_pos(init_pos, finder.ref_offset)
    want = set(int(p) for p in span_pos)
    rows = {}
    finder.init_repeat_span(init_pos)
    upto = init_pos + 2 * MAX_REPEAT_UNIT - 1
    for p in want:
        if m <= p <= upto:
            rows[p] = finder.row(p)
    anchors = []
    top = max([last_pos + 2 * MAX_REPEAT_UNIT + 1] + list(want))
    for p in range(m, last_pos + 1):
        while upto < p + 2 * MAX_REPEAT_UNIT + 1:
            upto += 1
            finder.update_repeat_span(upto)
            if upto in want:
                rows[upto] = finder.row(upto)
        anchors.append(1 if finder.is_anchor(p) else 0)
    while upto < top:
        upto += 1
        finder.update_repeat_span(upto)
        if upto in want:
            rows[upto] = finder.row(upto)
    return m, anchors, [rows[int(p)] for p in span_pos]


def ref_anchors(ref, ref_offset, init_pos, init_span, win_begin, n_pos, span_pos=()):
    """What sk_ref_anchors computes, by the loop model: a finder whose ring slot (m - 1) % 1000 holds init_span (None: zeros)
    -> (is_anchor[n_pos], span rows)"""
    m = min_pos(init_pos, ref_offset)
    if win_begin < m or any(p < m for p in span_pos):
        raise ValueError("before the first position initRepeatSpan(init_pos) updates")
    finder = RepeatFinder(ref, ref_offset)
    if init_span is not None:
        finder.repeat_span[_slot(m - 1)] = [int(x) & U32 for x in init_span]
    last = win_begin + n_pos - 1
    _, anchors, rows = run_region(finder, init_pos, max(last, m), span_pos)
    return anchors[win_begin - m:win_begin - m + n_pos], rows


# ---- the closed forms (independent of the class above) ---------------------------------------------------------------------------------------------


def _bases(ref, ref_offset, lo, hi):
    """get_base of lo .. hi - 1 as bytes"""
    out = np.full(hi - lo, ord("N"), np.uint8)
    a, b = max(lo, ref_offset), min(hi, ref_offset + len(ref))
    if b > a:
        out[a - lo:b - lo] = np.frombuffer(ref[a - ref_offset:b - ref_offset].encode(), np.uint8)
    return out


def closed_form_anchors(ref, ref_offset, init_pos, init_span, win_begin, n_pos):
    """The general rule: p is not an anchor <=> some u, q in [p, p + 99] have span_u(q) >= 2u and >= 3, and q == p or (span_u(q) in
    (2u, 3) and q - span_u(q) < p); span_u(m - 1) = init_span[u - 1]"""
    m = min_pos(init_pos, ref_offset)
    last_q = win_begin + n_pos - 1 + 99
    base = _bases(ref, ref_offset, m - MAX_REPEAT_UNIT, last_q + 1)
    non_anchor = np.zeros(last_q + 1 - m, bool)
    for u in range(1, MAX_REPEAT_UNIT + 1):
        cur, prev = base[MAX_REPEAT_UNIT:], base[MAX_REPEAT_UNIT - u:len(base) - u]
        match = (prev != ord("N")) & (cur == prev)
        span = 0 if init_span is None else int(init_span[u - 1]) & U32
        for k in range(len(match)):
            span = (span + 1) & U32 if match[k] else u
            if span >= 2 * u and span >= MIN_REPEAT_SPAN:
                non_anchor[k] = True
                if span == 2 * u or span == MIN_REPEAT_SPAN:
                    non_anchor[max(k - span + 1, 0):k] = True  # q - span < p <= q - 1; span <= 100 here, so q <= p + 99
    return [0 if x else 1 for x in non_anchor[win_begin - m:win_begin - m + n_pos]]


def tract_form_anchors(ref, ref_offset, win_begin, n_pos):
    """Away from m: per u, a maximal run [a, b] of match_u of length >= max(u, 3 - u) makes [a - u, b] non-anchor"""
    lo, hi = win_begin - 2 * MAX_REPEAT_UNIT, win_begin + n_pos + 2 * MAX_REPEAT_UNIT
    base = _bases(ref, ref_offset, lo - MAX_REPEAT_UNIT, hi)
    non_anchor = np.zeros(hi - lo, bool)
    for u in range(1, MAX_REPEAT_UNIT + 1):
        cur, prev = base[MAX_REPEAT_UNIT:], base[MAX_REPEAT_UNIT - u:len(base) - u]
        match = np.concatenate(([False], (prev != ord("N")) & (cur == prev), [False]))
        edges = np.flatnonzero(match[1:] != match[:-1])
        for a, b in zip(edges[0::2], edges[1::2]):  # the run is [a, b - 1] in window coordinates
            if b - a >= max(u, 3 - u):
                non_anchor[max(a - u, 0):b] = True
    # (a run cut by an end of the stretch looked at still shows 100 positions, enough for every u, wherever it reaches the window)
    return [0 if x else 1 for x in non_anchor[win_begin - lo:win_begin - lo + n_pos]]


# ---- the detector's walk ---------------------------------------------------------------------------------------------------------------------------

STATE_FIELDS = ("is_beginning", "active_region_start_pos", "anchor_pos_following_prev_variant", "prev_anchor_pos", "prev_variant_pos", "num_variants")


def initial_state():
    """the constructor's values (ActiveRegionDetector.hh:157-158, clearCoordinates .cpp:296-303)"""
    return dict(is_beginning=1, active_region_start_pos=-1, anchor_pos_following_prev_variant=-1, prev_anchor_pos=-1, prev_variant_pos=-1, num_variants=0)


class AssertionFailed(Exception):
    """createActiveRegion's assert (:318)"""


class SampleDetector:
    """SampleActiveRegionDetector's coordinates and updateEndPosition; the read buffer is three callables of the position"""

    def __init__(self, state, is_candidate_variant, is_depth_zero, is_anchor):
        self.__dict__.update({"_" + k: int(v) for k, v in state.items()})
        self.is_candidate_variant, self.is_depth_zero, self.is_anchor = is_candidate_variant, is_depth_zero, is_anchor

    def state(self):
        return {k: getattr(self, "_" + k) for k in STATE_FIELDS}

    def create_active_region(self):  # :314-328
        if not self._active_region_start_pos < self._anchor_pos_following_prev_variant:
            raise AssertionFailed()
        start, end = self._active_region_start_pos, self._anchor_pos_following_prev_variant
        self._num_variants = 0
        self._active_region_start_pos = 0
        return (start, end + 1)

    def update_end_position(self, pos):  # :336-409
        if self._is_beginning:
            self._active_region_start_pos = pos
            self._anchor_pos_following_prev_variant = pos
            self._prev_anchor_pos = pos
            self._is_beginning = 0
        pos_to_process = pos - 1
        if pos_to_process < 0:
            return None
        is_candidate = self.is_candidate_variant(pos_to_process)
        is_depth_zero = self.is_depth_zero(pos_to_process)
        if is_depth_zero and self._num_variants == 0:
            is_candidate = False
        is_anchor = self.is_anchor(pos_to_process) and not is_candidate
        if not is_candidate and not is_anchor:
            return None
        distance = (pos_to_process - self._prev_variant_pos) & U32
        region = None
        if distance > MAX_DISTANCE_BETWEEN_TWO_VARIANTS and self._anchor_pos_following_prev_variant >= 0:
            if self._num_variants >= MIN_NUM_VARIANTS_PER_REGION:
                region = self.create_active_region()
            else:
                self._num_variants = 0
        if is_anchor:
            if self._num_variants == 0:
                self._active_region_start_pos = pos_to_process
            if self._anchor_pos_following_prev_variant < 0:
                self._anchor_pos_following_prev_variant = pos_to_process
            self._prev_anchor_pos = pos_to_process
        if is_candidate:
            if not self._active_region_start_pos:
                self._active_region_start_pos = self._prev_anchor_pos
            self._num_variants += 1
            self._prev_variant_pos = pos_to_process
            self._anchor_pos_following_prev_variant = -1
        return region


def active_regions(win_begin, depth, is_candidate, is_anchor, state=None, trace=None):
    """What sk_active_regions computes: the calls updateEndPosition(win_begin + 1 .. win_begin + n_pos)
    -> (regions [(begin, end, made_at)], state_out); raises AssertionFailed where the reference's assert would fire.
    `trace`, a list, receives (state after the call, region or None) per call"""
    n = len(is_candidate)
    det = SampleDetector(state or initial_state(), lambda p: bool(is_candidate[p - win_begin]), lambda p: int(depth[p - win_begin]) == 0,
                         lambda p: bool(is_anchor[p - win_begin]))
    regions = []
    for pos in range(win_begin + 1, win_begin + n + 1):
        r = det.update_end_position(pos)
        if r is not None:
            regions.append((r[0], r[1], pos))
        if trace is not None:
            trace.append((det.state(), r))
    return regions, det.state()
