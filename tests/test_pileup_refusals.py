"""Row a8: what the pileup's entry points refuse of a read batch, and that a refusal leaves a stream as it was.

The reference throws or exits on these inputs (starling_read_util.cpp:198-203, bam_seq.hh:145-147, qscore_cache.cpp:53-75); the
library's host check refuses them before anything is changed or sent to the device.  One valid read, and that read with one thing
wrong, through the one-shot entry, the germline stream and the somatic stream (the bad read once as the normal, once as the tumor
sample's).  After every refused push the same stream object takes the valid read, and its window is the window of a fresh stream that
was given nothing else.  The last test pins sk_pileup_scratch_bytes: the device entry stays inside a scratch of exactly that size."""
import numpy as np
import pytest

from strelka_amd import capi, synth

REF = "ACGTTGCA" * 20
OFF = 1000
BEGIN, END = 1000, 1160
CODE = {"A": 1, "C": 2, "G": 4, "T": 8}
M, PAD = capi.SEG["MATCH"], capi.SEG["PAD"]


def _read(pos=1010, n=30, path=None, qual=30):
    code = [CODE[REF[(pos - OFF + i) % len(REF)]] for i in range(n)]
    return dict(code=code, qual=[qual] * n, pos=pos, path=path or [(M, n)], is_fwd=True, mapq=60, map_level=1)


def _batch(r):
    return synth.ReadBatch.from_reads([r], REF, OFF)


def _valid():
    return _batch(_read())


def _with(edit):
    r = _read()
    edit(r)
    return _batch(r)


def _bad_offsets():
    rb = _valid()
    rb.read_off[0] = 1  # (the Python helpers always start at 0: written into the array)
    return rb


# name -> (batch, pileup options, expected text)
BAD = {
    "quality_71_mapq_adjust": (lambda: _with(lambda r: r["qual"].__setitem__(7, 71)), dict(is_mapq_adjust=1),
                               "exceeds the maximum cached basecall quality score of 70"),
    "path_too_short": (lambda: _with(lambda r: r.__setitem__("path", [(M, 29)])), {}, "does not span"),
    "base_code_3": (lambda: _with(lambda r: r["code"].__setitem__(11, 3)), {}, "unsupported BAM base code"),
    "pad_segment": (lambda: _with(lambda r: r.__setitem__("path", [(M, 15), (PAD, 1), (M, 15)])), {}, "Can't handle cigar code"),
    "read_of_1025_bases": (lambda: _batch(_read(n=1025)), {}, "longer than 1024"),
    "offsets_start_at_1": (_bad_offsets, {}, "CSR offsets must start at 0"),
}
KEYS = ("tier1_off", "tier1_calls", "clean_count", "mapq_count")


def _opt(**kw):
    return capi.pileup_options(report_begin=BEGIN, report_end=END, **kw)


def _same_window(got, want):
    assert (got["begin"], got["end"]) == (want["begin"], want["end"]) == (1010, 1040)
    for k in KEYS:
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)
    assert int(want["tier1_off"][-1]) == 30


def _germline(opt, evs_words=False, region=True):
    st = capi.PileupStream(opt, capi.germline_options(), evs_words=evs_words)
    if region:
        st.begin_region(REF, OFF, BEGIN, END)
    return st


def _somatic(opt, region=True):
    st = capi.SomaticPileupStream(opt, capi.somatic_snv_options())
    if region:
        st.begin_region(REF, OFF, BEGIN, END)
    return st


def _fresh_germline(opt, evs_words=False):
    st = _germline(opt, evs_words)
    w = st.push(_valid(), END)
    st.close()
    return w


def _fresh_somatic(opt):
    st = _somatic(opt)
    w = st.push(_valid(), _valid(), END)
    st.close()
    return w


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(BAD))
def test_one_shot_refuses(gpu, case):
    make, kw, text = BAD[case]
    with pytest.raises(RuntimeError, match=text):
        capi.pileup_reads(make(), _opt(**kw), capi.PILEUP_CLEAN_TIER1)
    off, calls, _, _ = capi.pileup_reads(_valid(), _opt(**kw), capi.PILEUP_CLEAN_TIER1)
    assert int(off[-1]) == len(calls) == 30


def _germline_refusal(opt, text, evs_words=False, region=True, bad=None, **push_kw):
    st = _germline(opt, evs_words, region)
    with pytest.raises(RuntimeError, match=text):
        st.push(bad() if bad else _valid(), END, **push_kw)
    if not region:
        st.begin_region(REF, OFF, BEGIN, END)
    got = st.push(_valid(), END)
    st.close()
    _same_window(got, _fresh_germline(opt, evs_words))


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(BAD))
def test_germline_stream_refuses_and_stays_usable(gpu, case):
    make, kw, text = BAD[case]
    _germline_refusal(_opt(**kw), text, bad=make)


@pytest.mark.gpu
def test_germline_stream_refuses_quality_71_with_evs_words(gpu):
    _germline_refusal(_opt(is_mapq_adjust=0), "above 70 with the EVS column on", evs_words=True,
                      bad=lambda: _with(lambda r: r["qual"].__setitem__(7, 71)))


@pytest.mark.gpu
def test_germline_stream_refuses_a_mask_before_the_reference(gpu):
    _germline_refusal(_opt(), "mask window outside", mask=np.zeros(10, np.uint8), mask_begin=OFF - 10)


@pytest.mark.gpu
def test_germline_stream_refuses_a_push_without_a_region(gpu):
    _germline_refusal(_opt(), "no region", region=False)


def _somatic_refusal(opt, text, bad_sample=0, region=True, bad=None, **push_kw):
    st = _somatic(opt, region)
    rbs = [_valid(), _valid()]
    if bad:
        rbs[bad_sample] = bad()
    with pytest.raises(RuntimeError, match=text):
        st.push(rbs[0], rbs[1], END, **push_kw)
    if not region:
        st.begin_region(REF, OFF, BEGIN, END)
    got = st.push(_valid(), _valid(), END)
    st.close()
    want = _fresh_somatic(opt)
    for sample in ("normal", "tumor"):
        _same_window(got[sample], want[sample])


@pytest.mark.gpu
@pytest.mark.parametrize("bad_sample", [0, 1], ids=["normal", "tumor"])
@pytest.mark.parametrize("case", sorted(BAD))
def test_somatic_stream_refuses_and_stays_usable(gpu, case, bad_sample):
    make, kw, text = BAD[case]
    _somatic_refusal(_opt(**kw), text, bad_sample, bad=make)


@pytest.mark.gpu
def test_somatic_stream_refuses_a_mask_before_the_reference(gpu):
    _somatic_refusal(_opt(), "mask window outside", mask=np.zeros(10, np.uint8), mask_begin=OFF - 10)


@pytest.mark.gpu
def test_somatic_stream_refuses_a_push_without_a_region(gpu):
    _somatic_refusal(_opt(), "no region", region=False)


@pytest.mark.gpu
@pytest.mark.parametrize("n_reads,n_loci", [(3, 160), (0, 0)])
def test_device_entry_stays_inside_the_public_scratch_size(gpu, n_reads, n_loci):
    import torch
    from strelka_amd import device
    rb = synth.ReadBatch.from_reads([_read(pos=p) for p in (1010, 1050, 1100)[:n_reads]], REF, OFF)
    d = device.DeviceReadBatch(rb, n_loci, report_begin=BEGIN)
    nbytes = capi.lib().sk_pileup_scratch_bytes(rb.n_reads, rb.n_bases, n_loci)
    assert nbytes >= 0
    GUARD = 4096
    d.scratch = torch.full((nbytes + GUARD,), 0xA5, dtype=torch.uint8, device=d.device)
    call_off, calls = d.pileup(capi.PILEUP_CLEAN_TIER1)
    torch.cuda.synchronize()
    want_off, want_calls, _, _ = capi.pileup_reads(rb, d.opt, capi.PILEUP_CLEAN_TIER1)
    np.testing.assert_array_equal(call_off.cpu().numpy(), want_off)
    np.testing.assert_array_equal(calls.cpu().numpy().view(np.uint16)[:len(want_calls)], want_calls)
    assert len(want_calls) == 30 * n_reads
    assert bool((d.scratch[nbytes:] == 0xA5).all()), "the device entry wrote past sk_pileup_scratch_bytes()"
