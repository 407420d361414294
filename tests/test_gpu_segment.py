"""GPU tests of cmpc_eval_mask_out (masks without a ground truth, exact against hostutil.resize_and_crop), of predict_masks on it, of
Evaluator(gv_norm="sample") and of segment.FrameSegmenter end to end against the host loop of test.py:250-329 run with the model's own
forward pass."""
import importlib

import numpy as np
import pytest
import torch

from tests import util as U
from tests.test_gpu_eval import _blobs, _image, _samples

pytestmark = pytest.mark.gpu

HU = importlib.import_module("cmpc-refseg_amd.hostutil")
EV = importlib.import_module("cmpc-refseg_amd.evaluate")
SG = importlib.import_module("cmpc-refseg_amd.segment")
CRF = importlib.import_module("cmpc-refseg_amd.crf")
L = importlib.import_module("cmpc-refseg_amd._lib")
pkg = importlib.import_module("cmpc-refseg_amd")

GUARD = 0xA5


def _host_mask(m, t, oh, ow):
    return HU.resize_and_crop((m >= t).astype(np.float32), oh, ow) > 0


def _descs(shapes, HW, aligned):
    """plan_masks' descriptors, or the same geometry packed back to back from byte 1 (offsets that are not 4-byte aligned)."""
    d, nbytes = EV.plan_masks(shapes, HW, HW)
    if aligned:
        return d, nbytes
    off = 1
    for di in d:
        di.offset = off
        off += di.h * di.w + (di.h * di.w) % 2                         # keeps the following offsets odd
    return d, off + 3


@pytest.mark.parametrize("dtype", ["f32", "u8"])
@pytest.mark.parametrize("value", [1, 255])
@pytest.mark.parametrize("aligned", [True, False])
def test_mask_out_exact(dtype, value, aligned):
    """No allowance: every byte equals value * (hostutil.resize_and_crop((m >= t).astype(float32), oh, ow) > 0), every byte outside the
    samples' regions keeps the guard pattern, and the masks equal cmpc_eval_mask_iu(want_masks)'s on the same inputs."""
    rng = np.random.default_rng(7)
    cases = [(320, [(640, 640), (480, 480), (427, 640), (333, 500), (200, 150), (100, 120), (320, 320)]),      # test_mask_iu_exact's
             (64, [(128, 128), (96, 96), (37, 61), (64, 64)]),
             (320, [(166, 250), (213, 320), (360, 640), (240, 427), (20, 30), (1, 500), (500, 1)]),             # half sizes of odd frames, 1 x N
             (64, [(8, 8), (1, 50), (50, 1), (240, 320), (31, 33)])]
    for HW, shapes in cases:
        B = len(shapes)
        maps = np.stack([_blobs(rng, HW, HW) for _ in range(B)])
        if dtype == "f32":
            m = np.where(maps, rng.uniform(1e-9, 1.0, maps.shape), rng.uniform(-1.0, 1e-9, maps.shape)).astype(np.float32)
            t = 1e-9
        else:
            m = maps.astype(np.uint8)
            t = 0.5
        md = torch.from_numpy(m).cuda()
        d, nbytes = _descs(shapes, HW, aligned)
        buf = torch.full((nbytes + 64,), GUARD, dtype=torch.uint8, device="cuda")
        L.call("cmpc_eval_mask_out", md.data_ptr(), L.EVAL_F32 if dtype == "f32" else L.EVAL_U8, B, HW, HW, float(t), d, buf.data_ptr(), nbytes,
               value, torch.cuda.current_stream().cuda_stream)
        host = buf.cpu().numpy()
        inside = np.zeros(host.shape, bool)
        for b, (oh, ow) in enumerate(shapes):
            o = d[b].offset
            assert o % 16 == 0 if aligned else o % 2 == 1
            ref = _host_mask(m[b], np.float32(t) if dtype == "f32" else t, oh, ow).astype(np.uint8) * value
            got = host[o: o + oh * ow].reshape(oh, ow)
            assert np.array_equal(got, ref), (HW, shapes[b], int((got != ref).sum()))
            inside[o: o + oh * ow] = True
        assert np.all(host[~inside] == GUARD), (HW, "bytes outside the samples' regions were written")
        if aligned:
            # the Python wrapper, and cmpc_eval_mask_iu(want_masks) on the same inputs
            b2, d2 = EV.masks_out(md, shapes, t, value=value)
            _, masks = EV.mask_iu(md, [np.zeros(s, np.uint8) for s in shapes], t, want_masks=True)
            for b, mk in enumerate(EV.unpack_masks(b2, d2)):
                assert torch.equal(mk, masks[b] * value), (HW, shapes[b])
                assert np.array_equal(mk.cpu().numpy(), host[d[b].offset: d[b].offset + d[b].h * d[b].w].reshape(d[b].h, d[b].w))


def test_mask_out_thresholds_the_float_itself():
    """sigm >= threshold on the float32 map (test.py:307): values one ulp either side of the threshold fall on their own sides."""
    t = np.float32(0.5)
    m = np.full((1, 32, 32), np.nextafter(t, np.float32(0)), np.float32)
    m[0, 8:16, 8:16] = t
    m[0, 20:24, 4:8] = np.nextafter(t, np.float32(1))
    buf, d = EV.masks_out(torch.from_numpy(m).cuda(), [(32, 32)], float(t), value=255)
    got = EV.unpack_masks(buf, d)[0].cpu().numpy()
    assert np.array_equal(got, (m[0] >= t).astype(np.uint8) * 255) and got.sum() == 255 * (64 + 16)


def _tiny_model(B, dtype="f32"):
    cfg = U.tiny_cfg(B=B)
    return pkg.LSTM_model(**U.model_kwargs(cfg, dtype, mode="eval")), cfg


def test_predict_masks_unchanged_and_option():
    """predict_masks gives the masks of the earlier implementation: cmpc_eval_mask_iu(want_masks) against all-zero ground truths on the same
    `up`.  With gv_norm="sample" they are the masks of the same computation in that mode, and the model's own mode is restored."""
    model, cfg = _tiny_model(3)
    rng = np.random.default_rng(4)
    samples = _samples(rng, 2, cfg.num_steps, cfg.vocab_size, [(48, 80), (100, 64)])
    ids, sl, ims = [s[0] for s in samples], [s[1] for s in samples], [s[2] for s in samples]

    def parents_way():
        feed, _ = EV.prepare_images(ims + [ims[0]], model.H, model.W)
        up = model.forward(np.stack(ids + [ids[0]]), feed, np.array(sl + [sl[0]], np.int32))["up"]
        _, masks = EV.mask_iu(up[:2].float(), [np.zeros(im.shape[:2], np.uint8) for im in ims], 1e-9, want_masks=True)
        return [mk.cpu().numpy() for mk in masks]

    masks = EV.predict_masks(model, ids, sl, ims)
    for a, b, im in zip(masks, parents_way(), ims):
        assert a.dtype == np.uint8 and a.shape == im.shape[:2] and np.array_equal(a, b)
    assert model.gv_norm == "batch"
    got = EV.predict_masks(model, ids, sl, ims, gv_norm="sample")
    assert model.gv_norm == "batch"
    model.set_gv_norm("sample")
    want = parents_way()
    for a, b in zip(got, want):
        assert np.array_equal(a, b)
    assert EV.predict_masks(model, ids, sl, ims, gv_norm="batch")[0].shape == ims[0].shape[:2] and model.gv_norm == "sample"
    with pytest.raises(ValueError):
        EV.predict_masks(model, ids, sl, ims, gv_norm="rows")


def _host_ius(model, batches):
    """(I, U) of the first `n` samples of each given batch ([samples], n) by the host loop, in the model's current mode."""
    out = []
    for pad, n in batches:
        feed, _ = EV.prepare_images([s[2] for s in pad], model.H, model.W)
        up = model.forward(np.stack([s[0] for s in pad]), feed, np.array([s[1] for s in pad], np.int32))["up"].float().cpu().numpy()
        for b in range(n):
            gt = pad[b][3]
            pred = HU.resize_and_crop((up[b, :, :, 0] >= 1e-9).astype(np.float32), gt.shape[0], gt.shape[1])
            out.append(HU.compute_mask_IU(pred > 0, gt))
    return np.array(out)


def test_evaluator_sample_mode_and_pads():
    """Evaluator(gv_norm="sample"): per-sample (I, U) equal the host loop run in the same mode, and the real sample of the padded last batch
    gets the same (I, U) when the pad slots hold other samples.  The model's own mode is left alone."""
    model, cfg = _tiny_model(3)
    rng = np.random.default_rng(1)
    S = _samples(rng, 7, cfg.num_steps, cfg.vocab_size, [(48, 80), (100, 64), (64, 64), (37, 50)])
    ev = EV.Evaluator(model, gv_norm="sample")
    for s in S:
        ev.add(*s)
    per = ev.per_sample()
    assert model.gv_norm == "batch"
    base = EV.Evaluator(model)
    for s in S:
        base.add(*s)
    per_batch_mode = base.per_sample()
    model.set_gv_norm("sample")
    want = _host_ius(model, [(S[0:3], 3), (S[3:6], 3), ([S[6], S[6], S[6]], 1)])
    assert np.array_equal(per, want)
    other = _host_ius(model, [([S[6], S[1], S[4]], 1)])
    assert np.array_equal(other[0], per[6])
    model.set_gv_norm("batch")
    print("samples whose (I, U) differ between the modes: %d of 7" % int((per != per_batch_mode).any(1).sum()))
    with pytest.raises(ValueError):
        EV.Evaluator(model, gv_norm="rows")


FRAME_SIZES = [(480, 640), (360, 640), (240, 427)]


def _video(rng, n):
    return [_image(rng, *FRAME_SIZES[(f // 4) % 3]) for f in range(n)]


def _expressions(rng, T, vocab):
    out = []
    for n in (1, T // 2, T):
        ids = np.zeros(T, np.int32)
        ids[:n] = rng.integers(1, vocab, n)
        out.append((ids, n))
    return out


def _host_loop(model, frames, exprs, dcrf=False):
    """test.py:250-329 with the model's own forward pass: the same frame batches through prepare_images, model.forward per expression in
    mode "sample".  Returns {(e, f): float32 sigm [H, W]}, and with dcrf {(e, f): DenseCRF argmax [H, W]} as well."""
    B, H, W = model.batch_size, model.H, model.W
    sig, crf = {}, {}
    prev = model.gv_norm
    model.set_gv_norm("sample")
    for idx in SG.plan_batches(len(frames), B):
        feed, proc = EV.prepare_images([frames[i] for i in idx], H, W)
        n = len(set(idx))
        for e, (ids, sl) in enumerate(exprs):
            out = model.forward(np.repeat(ids[None], B, 0), feed, np.full(B, sl, np.int32))
            s = out["sigm"].float().reshape(B, H, W)
            if dcrf:
                cm = CRF.dense_crf_batch(s[:n], proc[:n], device=model.device, method="lattice").cpu().numpy()
            s = s.cpu().numpy()
            for b in range(n):
                sig[(e, idx[b])] = s[b]
                if dcrf:
                    crf[(e, idx[b])] = cm[b]
    model.set_gv_norm(prev)
    return sig, crf


@pytest.mark.parametrize("size", ["tiny_f32", "config2_f16"])
def test_frame_segmenter_end_to_end(size):
    """11 frames of three sizes, 3 expressions of different lengths: every yielded mask equals, with no allowance, the host loop's
    resize_and_crop(sigm >= thr) > 0 at (h // 2, w // 2); the order is frame batches, then expressions, then frames; depth 1 and 3 and a
    second run give identical results.  The threshold is the median of the host loop's sigm values, so that the masks are mixed."""
    rng = np.random.default_rng(11)
    if size == "tiny_f32":
        model, cfg = _tiny_model(4, "f32")
        T, vocab = cfg.num_steps, cfg.vocab_size
    else:
        model = pkg.get_segmentation_model("CMPC_model", mode="eval", batch_size=8, num_steps=20, H=320, W=320)
        assert model.dt == L.DT_F16
        T, vocab = 20, model.cfg.vocab_size
    B = model.batch_size
    frames, exprs = _video(rng, 11), _expressions(rng, T, vocab)
    sig, _ = _host_loop(model, frames, exprs)
    thr = float(np.median(np.stack([sig[k] for k in sorted(sig)])))
    want_order = [(e, f) for idx in SG.plan_batches(11, B) for e in range(3) for f in sorted(set(idx))]
    assert sorted(sig) == sorted(want_order)
    ref = {}
    for (e, f), s in sig.items():
        h, w = frames[f].shape[:2]
        ref[(e, f)] = (HU.resize_and_crop((s >= np.float32(thr)).astype(np.float32), h // 2, w // 2) > 0).astype(np.uint8) * 255
    fg = np.mean([r.mean() / 255 for r in ref.values()])
    print("%s: threshold %.6f, foreground share of the reference masks %.3f" % (size, thr, fg))
    assert 0.05 < fg < 0.95
    for depth in (2, 1, 3, 2):
        seg = SG.FrameSegmenter(model, threshold=thr, depth=depth)
        got = [(e, f, mk) for e, f, mk in seg.run(iter(frames), exprs)]
        assert model.gv_norm == "batch"
        assert [(e, f) for e, f, _ in got] == want_order
        for e, f, mk in got:
            assert mk.dtype == np.uint8 and np.array_equal(mk, ref[(e, f)]), (depth, e, f, int((mk != ref[(e, f)]).sum()))
    # one segmenter, run twice (its buffers are reused), and views instead of copies
    seg = SG.FrameSegmenter(model, threshold=thr, copy=False, value=1)
    for _ in range(2):
        n = 0
        for e, f, mk in seg.run(frames, exprs):
            assert np.array_equal(mk * 255, ref[(e, f)])
            n += 1
        assert n == 33


def test_frame_segmenter_dcrf_and_sentences():
    """dcrf=True, dcrf_method="lattice": the masks are the resampled argmax of crf.dense_crf_batch on the same sigm / proc_im.  Sentences go
    through hostutil.preprocess_sentence_lstm; a full-size out_size works as well."""
    rng = np.random.default_rng(12)
    model, cfg = _tiny_model(4, "f32")
    frames = _video(rng, 6)
    vocab = {"<pad>": 0, "<unk>": 1, "the": 2, "dog": 3, "on": 4, "left": 5, "a": 6, "red": 7, "car": 8}
    sentences = ["the dog on the left", "a red car"]
    exprs = [(np.asarray(i, np.int32), n) for i, n in (HU.preprocess_sentence_lstm(s, vocab, cfg.num_steps) for s in sentences)]
    sig, crf = _host_loop(model, frames, exprs, dcrf=True)
    seg = SG.FrameSegmenter(model, vocab=vocab, dcrf=True, dcrf_method="lattice", out_size=lambda h, w: (h, w), value=1)
    n = 0
    for e, f, mk in seg.run(frames, sentences):
        h, w = frames[f].shape[:2]
        want = HU.resize_and_crop(crf[(e, f)].astype(np.float32), h, w) > 0
        assert mk.shape == (h, w) and np.array_equal(mk, want.astype(np.uint8)), (e, f)
        n += 1
    assert n == 12
    with pytest.raises(ValueError, match="video"):
        class Video:
            video, batch_size, H, W, num_steps, device = True, 1, 64, 64, 6, torch.device("cuda:0")
        SG.FrameSegmenter(Video())
