"""The multi-sample synchroniser of the active-region detector, restated call by call: the bit-exact reference for sk_sync_active_regions
(csrc/active_region_detect.hip).

ActiveRegionDetector (L/starling_common/ActiveRegionDetector.cpp, L/ = the reference's src/c++/lib) over tests/anchor_model.SampleDetector,
its statements kept in the order the reference runs them:

  * updateEndPosition            :77-89    the close test first, then sample 0 .. S - 1, each returned region merged as it comes
  * updateActiveRegionRange      :119-131  end_pos() == 0 reads as "no region"; merge_range takes min begin and max end
                                           (L/blt_util/known_pos_range2.hh:166-171)
  * processExistingActiveRegion  :133-154  MaxAssemblyPadding = 9 (ActiveRegionReadBuffer.hh); the raw _activeRegionStartPos of every sample,
                                           whatever its _numVariants
  * closeActiveRegion            :203-250  the assertion size() > 0, a ploidy per sample, the id map, _prevActiveRegionEnd, clear() of the range
                                           (begin = end = 0, known_pos_range2.hh:173-178)
  * getPloidy                    :280-293  max of the ploidies at begin and end - 1; _posToPloidyMap with _defaultPloidy
  * setPosToActiveRegionIdMap    :267-278  nothing for a region of more than MaxRefSpanToBypassAssembly = 250 positions
  * clear                        :98-111   closeActiveRegionDetector per sample, merged as it comes, then the close without a test
  * closeActiveRegionDetector    :413-440  three branches; clearCoordinates leaves _isBeginning alone

What closeActiveRegion does with the region (the processors, filterOutConflictingForcedIndels) is not modelled: it changes none of the
coordinates here.

This module does not import the product."""
from tests import anchor_model as A

MAX_ASSEMBLY_PADDING = 9                  # ActiveRegionReadBuffer.hh: MaxAssemblyPadding
MAX_REF_SPAN_TO_BYPASS_ASSEMBLY = 250     # ActiveRegionProcessor.hh
MAX_SAMPLES = 8                           # SK_MAX_SAMPLES
CLOSED_AT_CLEAR = -1                      # SK_SYNC_CLOSED_AT_CLEAR: the region was closed by clear(), not by a call


class SyncAssertionFailed(Exception):
    """closeActiveRegion's assert (:206), or createActiveRegion's (:318) raised through closeActiveRegionDetector"""


def initial_state(n_samples=MAX_SAMPLES):
    """the constructor's values: every sample's detector new, no synchronised region (end 0), _prevActiveRegionEnd = -1
    (ActiveRegionDetector.hh:117)"""
    return dict(samples=[A.initial_state() for _ in range(n_samples)], sync_begin=0, sync_end=0, prev_end=-1, sample_mask=0)


def copy_state(state):
    return dict(state, samples=[dict(s) for s in state["samples"]])


def ploidy_at(marks, default_ploidy, pos):
    """SampleActiveRegionDetector::getPloidy(pos) :280-284: marks is the sorted [(pos, ploidy)] standing for _posToPloidyMap"""
    for p, v in marks:
        if p == pos:
            return v
    return default_ploidy


class Detector:
    """ActiveRegionDetector's coordinates.  depth, is_candidate: [S][n_pos]; is_anchor: [n_pos] (every sample's finder is given the same
    calls over the same reference); marks: [S][(pos, ploidy)]"""

    def __init__(self, win_begin, depth, is_candidate, is_anchor, marks=None, default_ploidy=2, state=None):
        n_samples = len(depth)
        state = copy_state(state) if state is not None else initial_state(n_samples)
        self.win_begin, self.n_pos = win_begin, len(is_anchor)
        self.samples = []
        for s in range(n_samples):
            self.samples.append(A.SampleDetector(state["samples"][s], lambda p, s=s: bool(is_candidate[s][p - win_begin]),
                                                 lambda p, s=s: int(depth[s][p - win_begin]) == 0, lambda p: bool(is_anchor[p - win_begin])))
        self.rest = state["samples"][n_samples:]  # (carried through untouched)
        self.sync_begin, self.sync_end, self.prev_end, self.sample_mask = state["sync_begin"], state["sync_end"], state["prev_end"], state["sample_mask"]
        self.marks = marks if marks is not None else [[] for _ in range(n_samples)]
        self.default_ploidy = default_ploidy
        self.regions = []
        self.ids = {}          # _posToActiveRegionIdMap, never erased here
        self.new_ids = []      # (begin, end) of the ranges the map gained in the last call
        # what the fixture's coverage is counted from, per closed region (not part of what the product computes): was its close put off
        # past end + 9 by a sample that had no part in it; did a sample's second region merge into its own first
        self.notes = []
        self._blocked_by_other = self._own_merge = False

    def state(self):
        return dict(samples=[d.state() for d in self.samples] + [dict(s) for s in self.rest], sync_begin=self.sync_begin, sync_end=self.sync_end,
                    prev_end=self.prev_end, sample_mask=self.sample_mask)

    def update_active_region_range(self, region, sample):  # :119-131
        if self.sync_end:
            self.sync_begin = min(self.sync_begin, region[0])
            self.sync_end = max(self.sync_end, region[1])
        else:
            self.sync_begin, self.sync_end = region
        if self.sample_mask >> sample & 1:
            self._own_merge = True
        self.sample_mask |= 1 << sample

    def close_active_region(self, closed_at):  # :203-250
        if not max(0, self.sync_end - self.sync_begin) > 0:
            raise SyncAssertionFailed()
        begin, end = self.sync_begin, self.sync_end
        ploidy = [max(ploidy_at(self.marks[s], self.default_ploidy, begin), ploidy_at(self.marks[s], self.default_ploidy, end - 1))
                  for s in range(len(self.samples))]  # :286-293, in the order the processors are made (:212)
        self.regions.append(dict(begin=begin, end=end, closed_at=closed_at, prev_end=self.prev_end, ploidy=ploidy, sample_mask=self.sample_mask))
        if end - begin <= MAX_REF_SPAN_TO_BYPASS_ASSEMBLY:  # :270
            for p in range(begin, end):
                self.ids[p] = begin
            self.new_ids.append((begin, end))
        self.prev_end = end                   # :248
        self.sync_begin = self.sync_end = 0   # :249
        self.sample_mask = 0
        self.notes.append(dict(delayed_by_other=self._blocked_by_other, own_merge=self._own_merge))
        self._blocked_by_other = self._own_merge = False

    def process_existing_active_region(self, pos):  # :133-154
        end = self.sync_end
        if end and end <= pos - MAX_ASSEMBLY_PADDING:
            for s, d in enumerate(self.samples):
                start = d._active_region_start_pos  # getActiveRegionStartPos: the raw coordinate
                if start >= 0 and start < end - 1:
                    if not self.sample_mask >> s & 1:
                        self._blocked_by_other = True
                    return
            self.close_active_region(pos)

    def update_end_position(self, pos):  # :77-89
        self.new_ids = []
        self.process_existing_active_region(pos)
        for s, d in enumerate(self.samples):
            try:
                region = d.update_end_position(pos)
            except A.AssertionFailed:
                raise SyncAssertionFailed()
            if region is not None:
                self.update_active_region_range(region, s)

    def close_sample_detector(self, d, buf_begin, buf_end):  # SampleActiveRegionDetector::closeActiveRegionDetector :413-440
        if d._is_beginning:
            return None
        region = None
        if d._num_variants >= A.MIN_NUM_VARIANTS_PER_REGION:
            start_undetermined = d._active_region_start_pos < 0
            end_undetermined = d._anchor_pos_following_prev_variant < 0
            if not start_undetermined or not end_undetermined or buf_begin < buf_end:
                if start_undetermined:
                    d._active_region_start_pos = buf_begin
                if end_undetermined:
                    d._anchor_pos_following_prev_variant = buf_end - 1
                try:
                    region = d.create_active_region()
                except A.AssertionFailed:
                    raise SyncAssertionFailed()
        # clearCoordinates :296-303
        d._prev_anchor_pos = d._active_region_start_pos = d._anchor_pos_following_prev_variant = d._prev_variant_pos = -1
        d._num_variants = 0
        return region

    def clear(self, buf_begin, buf_end):  # :98-111
        self.new_ids = []
        for s, d in enumerate(self.samples):
            region = self.close_sample_detector(d, buf_begin[s], buf_end[s])
            if region is not None:
                self.update_active_region_range(region, s)
        if self.sync_end:
            self.close_active_region(CLOSED_AT_CLEAR)


def sync_active_regions(win_begin, depth, is_candidate, is_anchor, marks=None, default_ploidy=2, state=None, do_clear=False, buf_begin=None, buf_end=None,
                        trace=None, notes=None):
    """What sk_sync_active_regions computes: ActiveRegionDetector::updateEndPosition(win_begin + 1 .. win_begin + n_pos), then clear() if asked
    -> (regions [dict], state_out, region_id[n_pos]); `notes`, a list, receives the model's note per closed region; raises SyncAssertionFailed where one of the reference's asserts would fire.
    `trace`, a list, receives (state, new id ranges) after every call and after clear()"""
    det = Detector(win_begin, depth, is_candidate, is_anchor, marks, default_ploidy, state)
    n = len(is_anchor)
    for pos in range(win_begin + 1, win_begin + n + 1):
        det.update_end_position(pos)
        if trace is not None:
            trace.append((det.state(), list(det.new_ids)))
    if do_clear:
        det.clear(buf_begin, buf_end)
        if trace is not None:
            trace.append((det.state(), list(det.new_ids)))
    if notes is not None:
        notes.extend(det.notes)
    region_id = [det.ids.get(p, -1) for p in range(win_begin, win_begin + n)]
    return det.regions, det.state(), region_id
