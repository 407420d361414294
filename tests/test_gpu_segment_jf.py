"""GPU tests of scoring inside the segmenters: FrameSegmenter (with and without DenseCRF) and ClipSegmenter run with ground_truth give
bit-identical masks, and their J / F equal hostutil.JFEval fed with tests/jf_ref.py's counts of the yielded masks -- the counts and the
float64 results with ==.  Tiny f32 models, non-square frames of two sizes, three expressions, every other frame without annotation, a
short last batch."""
import importlib

import numpy as np
import pytest

from tests import jf_ref as R
from tests import test_gpu_clip_segment as TGC
from tests import test_gpu_segment as TG

pytestmark = pytest.mark.gpu

HU = importlib.import_module("cmpc-refseg_amd.hostutil")
SG = importlib.import_module("cmpc-refseg_amd.segment")

SIZES = [(48, 80), (100, 64)]


class Recorder(HU.JFEval):
    """JFEval that also keeps the integers it was given."""

    def __init__(self):
        super().__init__()
        self.counts = {}

    def add(self, seq, frame, counts):
        self.counts[(seq, frame)] = np.array(counts, dtype=np.int64)
        super().add(seq, frame, counts)


def _frames(rng, n):
    return [TG._image(rng, *SIZES[(f // 3) % 2]) for f in range(n)]


def _check(make, frames, exprs, seq, annotated=lambda e, f: f % 2 == 0):
    """make() -> a fresh segmenter.  Runs it without and with ground truths (the unscored run's masks moved by two pixels, so that J and
    F lie strictly between 0 and 1) and compares as the module docstring says."""
    plain = [(e, f, mk) for e, f, mk in make().run(frames, exprs)]
    assert len(plain) == len(frames) * len(exprs)
    gts = {(e, f): np.roll(mk, (1, 2), (0, 1)) for e, f, mk in plain}
    calls = []

    def ground_truth(e, f):
        calls.append((e, f))
        if not annotated(e, f):
            return None
        return gts[(e, f)] if e != 1 else (np.repeat(gts[(e, f)][..., None] // 255 * 9, 3, 2), (9, 0, 0))      # a mask, or an (annotation, key) pair

    seg, rec = make(), Recorder()
    got = [(e, f, mk) for e, f, mk in seg.run(iter(frames), exprs, ground_truth=ground_truth, jf=rec, seq=seq)]
    assert seg.jf is rec
    assert [x[:2] for x in got] == [x[:2] for x in plain] == calls                  # once per pair, pads never
    for a, b in zip(got, plain):
        assert a[2].dtype == np.uint8 and np.array_equal(a[2], b[2]), a[:2]
    want = Recorder()
    for e, f, mk in got:
        if annotated(e, f):
            want.add((seq, e), f, R.counts(mk, gts[(e, f)], HU.jf_radius(*mk.shape)))
    assert sorted(rec.counts) == sorted(want.counts)
    for k in want.counts:
        assert np.array_equal(rec.counts[k], want.counts[k]), (k, rec.counts[k].tolist(), want.counts[k].tolist())
    res = rec.result()
    assert res == want.result()
    print("%s: J %.4f F %.4f J&F %.4f over %d sequences, %d frames" % (seq, res["J_mean"], res["F_mean"], res["J&F"], res["sequences"], res["frames"]))
    return res


@pytest.mark.parametrize("dcrf", [False, True])
def test_frame_segmenter_scores_what_it_yields(dcrf):
    model, cfg = TG._tiny_model(4, "f32")
    rng = np.random.default_rng(3)
    frames, exprs = _frames(rng, 7), TG._expressions(rng, cfg.num_steps, cfg.vocab_size)       # 7 frames in batches of 4: a short last batch
    if dcrf:
        make = lambda: SG.FrameSegmenter(model, dcrf=True, dcrf_method="lattice", out_size=SG.full_size)
    else:
        sig, _ = TG._host_loop(model, frames, exprs)
        thr = float(np.median(np.stack([s.reshape(-1) for s in sig.values()])))
        make = lambda: SG.FrameSegmenter(model, threshold=thr)
    res = _check(make, frames, exprs, "frame-dcrf" if dcrf else "frame")
    assert res["sequences"] == 3 and res["frames"] == 3 * 4
    if not dcrf:
        assert 0.0 < res["J_mean"] < 1.0 and 0.0 < res["F_mean"] <= 1.0


def test_clip_segmenter_scores_what_it_yields():
    model, cfg = TGC._tiny_model("f32")
    rng = np.random.default_rng(4)
    frames = [TGC._frame(rng, *SIZES[(f // 3) % 2], 3 * f) for f in range(8)]
    T = cfg.num_steps
    exprs = TGC._expressions(rng, T, cfg.vocab_size, [1, T // 2, T])
    ups = TGC._driver_loop(model, frames[:2], exprs[:1])
    thr = TGC._median_threshold([ups])
    absent = lambda e, f: f % 2 == 0 and not (e == 2 and f == 4)           # one expression's object is absent from one annotated frame
    res = _check(lambda: SG.ClipSegmenter(model, threshold=thr), frames, exprs, "clip", annotated=absent)
    assert res["sequences"] == 3 and res["frames"] == 3 * 4 - 1
    assert 0.0 < res["J_mean"] < 1.0
