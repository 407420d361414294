"""GPU tests of the evaluation layer: cmpc_eval_prep / cmpc_eval_mask_iu against hostutil's resize_and_pad / resize_and_crop /
compute_mask_IU, and Evaluator end to end against the host loop of trainval_model.test()."""
import importlib

import numpy as np
import pytest
import torch

from tests import util as U

pytestmark = pytest.mark.gpu

HU = importlib.import_module("cmpc-refseg_amd.hostutil")
EV = importlib.import_module("cmpc-refseg_amd.evaluate")
CRF = importlib.import_module("cmpc-refseg_amd.crf")
pkg = importlib.import_module("cmpc-refseg_amd")

SIZES = [(480, 640), (333, 500), (240, 427), (100, 50), (320, 320), (50, 900)]


def _image(rng, h, w, gray=False):
    # smooth content plus noise: realistic gradients and many exact-tie candidates for the rounding
    y, x = np.mgrid[0:h, 0:w]
    base = 127 + 100 * np.sin(x / 17.0)[..., None] * np.cos(y / 23.0)[..., None] * np.array([1.0, 0.7, -0.5])
    im = np.clip(base + rng.normal(0, 25, (h, w, 3)), 0, 255).astype(np.uint8)
    return im[..., 0] if gray else im


def _blobs(rng, h, w, n=4):
    y, x = np.mgrid[0:h, 0:w]
    m = np.zeros((h, w), bool)
    for _ in range(n):
        cy, cx, r = rng.uniform(0, h), rng.uniform(0, w), rng.uniform(0.05, 0.3) * min(h, w)
        m |= (y - cy) ** 2 + (x - cx) ** 2 < r * r
    return m


MU = np.array((104.00698793, 116.66876762, 122.67891434))


@pytest.mark.parametrize("HW", [320, 512])
def test_prepare_images_matches_host(HW):
    rng = np.random.default_rng(HW)
    ims = [_image(rng, h, w) for h, w in SIZES] + [_image(rng, 240, 427, gray=True), _image(rng, HW, HW)]
    feed, proc = EV.prepare_images(ims, HW, HW, "cuda:0")
    feed, proc = feed.cpu().numpy(), proc.cpu().numpy()
    for b, im in enumerate(ims):
        ref = HU.img_as_ubyte(HU.resize_and_pad(im, HW, HW))
        if ref.ndim == 2:
            ref = np.repeat(ref[..., None], 3, 2)
        diff = np.abs(proc[b].astype(int) - ref.astype(int))
        assert diff.max() <= 1 and (diff > 0).mean() <= 1e-3, (im.shape, diff.max(), (diff > 0).mean())
        if im.shape[:2] == (HW, HW):
            assert np.array_equal(proc[b], ref)
        rh, rw, top, left = HU.resize_and_pad_geometry(im.shape[0], im.shape[1], HW, HW)
        pad = np.ones((HW, HW), bool)
        pad[top: top + rh, left: left + rw] = False
        assert not proc[b][pad].any()
        # the reference's feed: proc_im[..., ::-1].astype(float32); proc_im_ -= mu   (trainval_model.py:228-230)
        r = proc[b][..., ::-1].astype(np.float32)
        r -= MU
        assert np.array_equal(feed[b].view(np.uint32), r.view(np.uint32))


def _host_iu(m, gt, t):
    pred = HU.resize_and_crop((m >= t).astype(np.float32), gt.shape[0], gt.shape[1]) > 0
    return HU.compute_mask_IU(pred, gt) + (pred,)


@pytest.mark.parametrize("dtype", ["f32", "u8"])
def test_mask_iu_exact(dtype):
    rng = np.random.default_rng(7)
    cases = [(320, [(640, 640), (480, 480), (427, 640), (333, 500), (200, 150), (100, 120), (320, 320)]),
             (64, [(128, 128), (96, 96), (37, 61), (64, 64)])]
    for HW, shapes in cases:
        B = len(shapes)
        maps = np.stack([_blobs(rng, HW, HW) for _ in range(B)])
        if dtype == "f32":
            m = np.where(maps, rng.uniform(1e-9, 1.0, maps.shape), rng.uniform(-1.0, 1e-9, maps.shape)).astype(np.float32)
            t = 1e-9
        else:
            m = maps.astype(np.uint8)
            t = 0.5
        gts = [_blobs(rng, h, w) for h, w in shapes]
        iu, masks = EV.mask_iu(torch.from_numpy(m).cuda(), gts, t, want_masks=True)
        iu = iu.cpu().numpy()
        for b in range(B):
            I, Un, pred = _host_iu(m[b], gts[b], t)
            assert (iu[b, 0], iu[b, 1]) == (I, Un), (HW, shapes[b])
            assert np.array_equal(masks[b].cpu().numpy(), pred.astype(np.uint8)), (HW, shapes[b])


def _samples(rng, n, T, vocab, sizes):
    out = []
    for i in range(n):
        h, w = sizes[i % len(sizes)]
        L = int(rng.integers(1, T + 1))
        ids = np.zeros(T, np.int32)
        ids[:L] = rng.integers(1, vocab, L)
        out.append((ids, L, _image(rng, h, w), _blobs(rng, h, w, 3)))
    return out


def _host_loop(model, samples, use_gpu_prep):
    """trainval_model.test()'s per-sample loop with the model's forward (batched exactly like the Evaluator)."""
    B, H, W = model.batch_size, model.H, model.W
    seg, ius = HU.SegEval(), []
    for s0 in range(0, len(samples), B):
        chunk = samples[s0: s0 + B]
        pad = chunk + [chunk[0]] * (B - len(chunk))
        if use_gpu_prep:
            feed, _ = EV.prepare_images([s[2] for s in pad], H, W)
        else:
            feed = np.stack([HU.image_feed(HU.img_as_ubyte(HU.resize_and_pad(s[2], H, W))) for s in pad])
        up = model.forward(np.stack([s[0] for s in pad]), feed, np.array([s[1] for s in pad], np.int32))["up"].float().cpu().numpy()
        for b, s in enumerate(chunk):
            pred = HU.resize_and_crop((up[b, :, :, 0] >= 1e-9).astype(np.float32), s[3].shape[0], s[3].shape[1])
            ius.append(seg.add(pred, s[3]))
    return seg, np.array(ius)


def _tiny_model(B):
    cfg = U.tiny_cfg(B=B)
    return pkg.LSTM_model(**U.model_kwargs(cfg, "f32", mode="eval")), cfg


def _check_evaluator(model, samples):
    ev = EV.Evaluator(model)
    for s in samples:
        ev.add(*s)
    res = ev.result()
    per = ev.per_sample()
    seg, ius = _host_loop(model, samples, True)
    assert np.array_equal(per, ius)
    ref = seg.result()
    ref["samples"] = len(samples)
    assert res == ref
    seg2, _ = _host_loop(model, samples, False)
    for k, v in seg2.result().items():
        assert abs(res[k] - v) <= 1e-2, k
    ev2 = EV.Evaluator(model)
    for s in samples:
        ev2.add(*s)
    assert ev2.result() == res and np.array_equal(ev2.per_sample(), per)
    return res


def test_evaluator_tiny_partial_batch():
    model, cfg = _tiny_model(3)
    rng = np.random.default_rng(1)
    samples = _samples(rng, 7, cfg.num_steps, cfg.vocab_size, [(48, 80), (100, 64), (64, 64), (37, 50)])
    res = _check_evaluator(model, samples)
    assert res["samples"] == 7


def test_evaluator_config2_size():
    model = pkg.get_segmentation_model("CMPC_model", mode="eval", batch_size=8, num_steps=20, H=320, W=320)
    rng = np.random.default_rng(2)
    samples = _samples(rng, 21, 20, model.cfg.vocab_size, [(480, 640), (427, 640), (640, 480), (333, 500), (375, 500), (612, 612)])
    _check_evaluator(model, samples)


def test_evaluator_dcrf():
    model, cfg = _tiny_model(3)
    rng = np.random.default_rng(3)
    samples = _samples(rng, 4, cfg.num_steps, cfg.vocab_size, [(48, 80), (100, 64)])
    ev = EV.Evaluator(model, dcrf=True)
    for s in samples:
        ev.add(*s)
    res = ev.result()
    seg = HU.SegEval()
    B = model.batch_size
    for s0 in range(0, 4, B):
        chunk = samples[s0: s0 + B]
        pad = chunk + [chunk[0]] * (B - len(chunk))
        feed, proc = EV.prepare_images([s[2] for s in pad], model.H, model.W)
        out = model.forward(np.stack([s[0] for s in pad]), feed, np.array([s[1] for s in pad], np.int32))
        for b, s in enumerate(chunk):
            m = CRF.dense_crf_mask(out["sigm"][b].float().reshape(model.H, model.W), proc[b]).cpu().numpy()
            pred = HU.resize_and_crop(m.astype(np.float32), s[3].shape[0], s[3].shape[1])
            seg.add(pred, s[3])
    for k, v in seg.result().items():
        assert res["dcrf_" + k] == v, k


def test_predict_masks_and_video_rejected():
    model, cfg = _tiny_model(3)
    rng = np.random.default_rng(4)
    samples = _samples(rng, 2, cfg.num_steps, cfg.vocab_size, [(48, 80), (100, 64)])
    masks = EV.predict_masks(model, [s[0] for s in samples], [s[1] for s in samples], [s[2] for s in samples])
    feed, _ = EV.prepare_images([s[2] for s in samples] + [samples[0][2]], model.H, model.W)
    up = model.forward(np.stack([s[0] for s in samples] + [samples[0][0]]), feed,
                       np.array([s[1] for s in samples] + [samples[0][1]], np.int32))["up"].float().cpu().numpy()
    for b, s in enumerate(samples):
        ref = HU.resize_and_crop((up[b, :, :, 0] >= 1e-9).astype(np.float32), s[2].shape[0], s[2].shape[1]) > 0
        assert masks[b].shape == s[2].shape[:2] and np.array_equal(masks[b], ref.astype(np.uint8))

    class Video:
        video, batch_size, H, W, device = True, 1, 64, 64, torch.device("cuda:0")
    with pytest.raises(ValueError, match="video"):
        EV.Evaluator(Video())


def test_evaluate_batches_script(tmp_path):
    """examples/evaluate_batches.py as a fresh child process on 5 .npz files in build_batches.py's layout: its printed lines equal
    Evaluator.result() on the same snapshot."""
    import os
    import subprocess
    import sys
    CK = importlib.import_module("cmpc-refseg_amd.checkpoint")
    model, cfg = _tiny_model(3)
    snap = CK.Saver(fmt="npz").save(model, str(tmp_path / "snap"))
    rng = np.random.default_rng(6)
    ev = EV.Evaluator(model)
    for n, (ids, L, im, m) in enumerate(_samples(rng, 5, cfg.num_steps, cfg.vocab_size, [(48, 80), (100, 64), (64, 64)])):
        front = np.zeros(cfg.num_steps, np.int64)
        front[cfg.num_steps - L:] = ids[:L]
        np.savez(str(tmp_path / ("val_%d.npz" % n)), text_batch=front, im_batch=im, mask_batch=m, sent_batch=["s"])
        ev.add(ids, L, im, m)
    res = ev.result()
    kw = "vf_h=8,vf_w=8,vf_dim=256,c4_dim=128,c3_dim=64,vocab_size=50,v_emb_dim=40,mlp_dim=24,rnn_size=40,glove_dim=12,parse_dim=20," \
         "backbone_width=8,backbone_blocks=1:1:2:1,dtype=f32"
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    p = subprocess.run([sys.executable, os.path.join(root, "examples", "evaluate_batches.py"), "--folder", str(tmp_path), "--prefix", "val",
                        "--snapshot", snap, "--batch", "3", "--H", "64", "--W", "64", "--T", str(cfg.num_steps), "--model-kwargs", kw],
                       capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = p.stdout.strip().splitlines()
    want = ["samples = 5"] + ["precision@%s = %f" % (t, res["precision@%s" % t]) for t in (.5, .6, .7, .8, .9)] + \
        ["overall IoU = %f; mean IoU = %f" % (res["overall_IoU"], res["mean_IoU"])]
    assert lines[-len(want):] == want
