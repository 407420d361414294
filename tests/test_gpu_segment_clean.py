"""GPU tests of clean= inside the segmenters.  FrameSegmenter (with and without DenseCRF) and ClipSegmenter with clean= yield exactly
hostutil.clean_mask of what the plain run yields, with equal statistics; with ground_truth the J / F counts are those of the cleaned
masks (scoring runs behind cleaning); with describe= the descriptors and agreement counts are those of a run without clean=; with
clean=None every mask and every byte of every ring slot equals a segmenter constructed without the argument.  Tiny f32 models,
non-square frames of two sizes, three expressions, a short last batch.  The thresholds are medians of the score maps, so the random
weights give fragmented masks: each test asserts that it saw masks of several components."""
import importlib

import numpy as np
import pytest

from tests import test_gpu_clip_segment as TGC
from tests import test_gpu_segment as TG

pytestmark = pytest.mark.gpu

HU = importlib.import_module("cmpc-refseg_amd.hostutil")
EV = importlib.import_module("cmpc-refseg_amd.evaluate")
SG = importlib.import_module("cmpc-refseg_amd.segment")

SIZES = [(48, 80), (100, 64)]
OPTIONS = [{"keep": 1}, {"keep": 2, "min_area": 3, "connectivity": 4}]


def _defaults(opts):
    return dict({"keep": 1, "min_area": 0, "connectivity": 8}, **opts)


def _check(make, frames, exprs, opts, tag):
    """make(**kw) -> a fresh segmenter.  The run with clean=opts against hostutil.clean_mask of the plain run; returns what it yielded
    and the number of masks with more than one component."""
    plain = [(e, f, mk) for e, f, mk in make().run(frames, exprs)]
    seg, log = make(clean=opts), HU.CleanLog()
    got = [(e, f, mk) for e, f, mk in seg.run(iter(frames), exprs, seq=tag, cleaned=log)]
    assert seg.cleaned is log and len(log) == len(plain) == len(got) == len(frames) * len(exprs)
    multi = changed = 0
    for (e, f, mk), (pe, pf, pm) in zip(got, plain):
        assert (e, f) == (pe, pf)
        want, stats = HU.clean_mask(pm, **_defaults(opts))
        assert mk.dtype == np.uint8 and np.array_equal(mk, want), (tag, e, f)
        st, ids = log.stats((tag, e))
        assert np.array_equal(st[ids.index(f)], stats), (tag, e, f, st[ids.index(f)].tolist(), stats.tolist())
        multi += stats[0] > 1
        changed += not np.array_equal(mk, pm)
    print("%s %s: %d of %d masks have several components, %d changed; fragmented: %d" % (tag, opts, multi, len(got), changed, len(log.fragmented())))
    assert multi >= 1 and changed >= 1, "no mask with several components: the comparison is vacuous"
    return got, plain, log


def _frame_case(B=4, n=7, seed=3):
    model, cfg = TG._tiny_model(B, "f32")
    rng = np.random.default_rng(seed)
    frames = [TG._image(rng, *SIZES[(f // 3) % 2]) for f in range(n)]
    exprs = TG._expressions(rng, cfg.num_steps, cfg.vocab_size)
    sig, _ = TG._host_loop(model, frames, exprs)
    thr = float(np.median(np.stack([s.reshape(-1) for s in sig.values()])))
    return model, frames, exprs, thr


def _clip_case(n=8, seed=4):
    model, cfg = TGC._tiny_model("f32")
    rng = np.random.default_rng(seed)
    frames = [TGC._frame(rng, *SIZES[(f // 3) % 2], 3 * f) for f in range(n)]
    T = cfg.num_steps
    exprs = TGC._expressions(rng, T, cfg.vocab_size, [1, T // 2, T])
    thr = TGC._median_threshold([TGC._driver_loop(model, frames[:2], exprs[:1])])
    return model, frames, exprs, thr


@pytest.fixture(scope="module")
def frame_case():
    return _frame_case()


@pytest.fixture(scope="module")
def clip_case():
    return _clip_case()


@pytest.mark.parametrize("opts", OPTIONS)
def test_frame_segmenter_cleans_what_it_yields(frame_case, opts):
    model, frames, exprs, thr = frame_case
    _check(lambda **kw: SG.FrameSegmenter(model, threshold=thr, **kw), frames, exprs, opts, "frame")


@pytest.mark.parametrize("opts", OPTIONS)
def test_clip_segmenter_cleans_what_it_yields(clip_case, opts):
    model, frames, exprs, thr = clip_case
    _check(lambda **kw: SG.ClipSegmenter(model, threshold=thr, **kw), frames, exprs, opts, "clip")


def test_frame_segmenter_cleans_the_dense_crf_mask(frame_case):
    model, frames, exprs, _ = frame_case
    _check(lambda **kw: SG.FrameSegmenter(model, dcrf=True, dcrf_method="lattice", out_size=SG.full_size, **kw), frames[:5], exprs[:2],
           {"keep": 1}, "frame-dcrf")


class Recorder(HU.JFEval):
    """JFEval that also keeps the integers it was given."""

    def __init__(self):
        super().__init__()
        self.counts = {}

    def add(self, seq, frame, counts):
        self.counts[(seq, frame)] = np.array(counts, dtype=np.int64)
        super().add(seq, frame, counts)


def _scored_and_described(make, frames, exprs, tag):
    """Scoring runs behind cleaning: the counts are evaluate.mask_jf's of the yielded (cleaned) masks; describe= reads sigm and the taps:
    its log is bit-identical to a run without clean=."""
    opts = {"keep": 1}
    got, plain, first_log = _check(make, frames, exprs, opts, tag)
    gts = {(e, f): np.roll(pm, (1, 2), (0, 1)) for e, f, pm in plain}        # the uncleaned mask, moved: the speckle counts against J and F
    annotated = lambda e, f: f % 2 == 0
    gt = lambda e, f: gts[(e, f)] if annotated(e, f) else None
    seg, rec, piv, log = make(clean=opts, describe="c4"), Recorder(), HU.PivotLog(), HU.CleanLog()
    both = [(e, f, mk) for e, f, mk in seg.run(frames, exprs, ground_truth=gt, jf=rec, seq=tag, pivots=piv, cleaned=log)]
    for a, b in zip(both, got):
        assert a[:2] == b[:2] and np.array_equal(a[2], b[2])
    keys = [(e, f) for e, f, _ in both if annotated(e, f)]
    want = EV.mask_jf([mk for e, f, mk in both if annotated(e, f)], [gts[k] for k in keys])
    unclean = EV.mask_jf([pm for e, f, pm in plain if annotated(e, f)], [gts[k] for k in keys])
    assert sorted(rec.counts) == sorted(((tag, e), f) for e, f in keys)
    for (e, f), w in zip(keys, want):
        assert np.array_equal(rec.counts[((tag, e), f)], w), (e, f, rec.counts[((tag, e), f)].tolist(), w.tolist())
    assert not np.array_equal(want, unclean)                                   # the scores do tell the two apart
    # the same run without clean=: the describe log is the same, bit for bit; the J / F counts are those of the uncleaned masks
    seg0, rec0, piv0 = make(describe="c4"), Recorder(), HU.PivotLog()
    list(seg0.run(frames, exprs, ground_truth=gt, jf=rec0, seq=tag, pivots=piv0))
    assert sorted(piv.seqs) == sorted(piv0.seqs) and len(piv) == len(both)
    for s in piv.seqs:
        (d, ids), (d0, ids0) = piv.descriptors(s), piv0.descriptors(s)
        assert ids == ids0 and np.array_equal(d.view(np.uint32), d0.view(np.uint32))
        assert np.array_equal(piv.areas(s), piv0.areas(s)) and np.array_equal(piv.consistencies(s), piv0.consistencies(s), equal_nan=True)
    for (e, f), u in zip(keys, unclean):
        assert np.array_equal(rec0.counts[((tag, e), f)], u)
    for e in range(len(exprs)):                                                # the statistics did not move either
        assert np.array_equal(log.stats((tag, e))[0], first_log.stats((tag, e))[0]) and len(log.stats((tag, e))[1]) == len(frames)


def test_frame_segmenter_scores_cleaned_masks_and_describes_as_before(frame_case):
    model, frames, exprs, thr = frame_case
    _scored_and_described(lambda **kw: SG.FrameSegmenter(model, threshold=thr, **kw), frames, exprs, "frame-jf")


def test_clip_segmenter_scores_cleaned_masks_and_describes_as_before(clip_case):
    model, frames, exprs, thr = clip_case
    _scored_and_described(lambda **kw: SG.ClipSegmenter(model, threshold=thr, **kw), frames, exprs, "clip-jf")


def _slots(seg, frames, exprs, gt):
    """Run with every slot and the device buffer pre-filled, so that whole buffers can be compared afterwards."""
    st = seg.stage
    st.reserve(1 << 20)
    st.mask_dev.fill_(0xA5)
    for h in st.host:
        h.fill_(0xA5)
    out = [(e, f, mk) for e, f, mk in seg.run(frames, exprs, ground_truth=gt)]
    st.torch.cuda.synchronize()
    return out, [h.numpy().copy() for h in st.host], st.mask_dev.cpu().numpy()


@pytest.mark.parametrize("which", ["frame", "clip"])
def test_option_off_is_the_segmenter_without_the_argument(which, frame_case, clip_case):
    model, frames, exprs, thr = frame_case if which == "frame" else clip_case
    cls = SG.FrameSegmenter if which == "frame" else SG.ClipSegmenter
    a = cls(model, threshold=thr)
    b = cls(model, threshold=thr, clean=None)
    assert b.clean is None and b.stage.cleaner is None
    gt = lambda e, f: np.ones(SIZES[(f // 3) % 2] if which == "clip" else SG.half_size(*SIZES[(f // 3) % 2]), np.uint8) if f % 2 else None
    (ma, ha, da), (mb, hb, db) = _slots(a, frames, exprs, gt), _slots(b, frames, exprs, gt)
    assert len(ma) == len(mb) == len(frames) * len(exprs)
    for x, y in zip(ma, mb):
        assert x[:2] == y[:2] and np.array_equal(x[2], y[2])
    for x, y in zip(ha, hb):
        assert np.array_equal(x, y)                                            # every byte of every ring slot
    assert np.array_equal(da, db) and b.cleaned is None
    assert list(a.jf.seqs) == list(b.jf.seqs) and a.jf.result() == b.jf.result()
