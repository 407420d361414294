"""GPU tests of the video evaluation path (CMPC_video_mm_tgraph_allvec on an A2D split, trainval_video.py:136-291): forward_video_frames
against forward_video, and VideoEvaluator end to end against the driver's host loop -- prepare_images on all 16 frames, forward_video on
the clip, resize_and_crop(up >= 1e-9) and SegEval at the ten thresholds."""
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import util as U
from oracle import cmpc_torch as O
from oracle import cmpc_video_torch as VD

pytestmark = pytest.mark.gpu

HU = importlib.import_module("cmpc-refseg_amd.hostutil")
EV = importlib.import_module("cmpc-refseg_amd.evaluate")
CRF = importlib.import_module("cmpc-refseg_amd.crf")
MD = importlib.import_module("cmpc-refseg_amd.model")
NAME = "CMPC_video_mm_tgraph_allvec"
THR = EV.VIDEO_THRESHOLDS


def _frame(rng, h, w, phase):
    y, x = np.mgrid[0:h, 0:w]
    base = 127 + 100 * np.sin((x + phase) / 13.0)[..., None] * np.cos(y / 17.0)[..., None] * np.array([1.0, 0.7, -0.5])
    return np.clip(base + rng.normal(0, 25, (h, w, 3)), 0, 255).astype(np.uint8)


def _blobs(rng, h, w, n=3):
    y, x = np.mgrid[0:h, 0:w]
    m = np.zeros((h, w), bool)
    for _ in range(n):
        cy, cx, r = rng.uniform(0, h), rng.uniform(0, w), rng.uniform(0.1, 0.35) * min(h, w)
        m |= (y - cy) ** 2 + (x - cx) ** 2 < r * r
    if not m.any():
        m[h // 2, w // 2] = True
    return m


def _clips(rng, n, T, vocab, sizes, lengths):
    """A2D test samples as build_A2D_batches.py stores them: front-padded text, the key image (clip frame 8), 16 uint8 frames, mask."""
    out = []
    for i in range(n):
        h, w = sizes[i % len(sizes)]
        L = lengths[i % len(lengths)]
        text = np.zeros(T, np.int64)
        text[T - L:] = rng.integers(1, vocab, L)
        frames = np.stack([_frame(rng, h, w, 3 * k) for k in range(16)])
        out.append((text, frames[8].copy(), frames, _blobs(rng, h, w)))
    return out


def _tiny_model(dtype="f32"):
    cfg = VD.tiny_cfg()
    hp, bp = VD.init_head_params(cfg), O.init_backbone_params(cfg)
    g = torch.Generator().manual_seed(3)
    for k in hp:
        if k.endswith(("biases", "beta")):
            hp[k] = (torch.randn(hp[k].shape, generator=g) * 0.05).float()
    m = U.pkg().get_segmentation_model(NAME, head_params=hp, backbone_params=bp, frames=cfg.frames, **U.model_kwargs(cfg, dtype, "eval"))
    return m, cfg


def _host_loop(model, samples, use_gpu_prep, dcrf=False):
    """trainval_video.py:186-253 with the model's forward_video: every frame of the clip prepared, then the graph's own gather."""
    H, W = model.H, model.W
    seg, ius = HU.SegEval(THR), []
    seg_crf = HU.SegEval(THR) if dcrf else None
    for text, im, frames, mask in samples:
        vi = np.array([[HU.first_valid_idx(text)]], np.int32)
        if use_gpu_prep:
            clip, _ = EV.prepare_images(list(frames), H, W)
        else:
            clip = np.stack([HU.image_feed(HU.img_as_ubyte(HU.resize_and_pad(f, H, W))) for f in frames]).astype(np.float32)
        out = model.forward_video(text[None], None, vi, clip[None])
        up = out["up"].float().cpu().numpy()
        pred = HU.resize_and_crop((up[0, :, :, 0] >= 1e-9).astype(np.float32), mask.shape[0], mask.shape[1])
        ius.append(seg.add(pred, mask))
        if dcrf:
            _, proc = EV.prepare_images([im], H, W)
            m = CRF.dense_crf_mask(out["sigm"][0].float().reshape(H, W), proc[0]).cpu().numpy()
            seg_crf.add(HU.resize_and_crop(m.astype(np.float32), mask.shape[0], mask.shape[1]), mask)
    return seg, np.array(ius), seg_crf


def _evaluate(model, samples, **kw):
    ev = EV.VideoEvaluator(model, **kw)
    for s in samples:
        ev.add(*s)
    return ev.result(), ev.per_sample()


@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_forward_video_frames_bit_identical(dtype):
    model, cfg = _tiny_model(dtype)
    g = torch.Generator().manual_seed(11)
    T = cfg.num_steps
    for it in range(4):                 # eager backbone passes first, then both captured-graph slots
        L = (2, T, 1, 4)[it]
        words = torch.zeros(1, T, dtype=torch.int64)
        words[0, T - L:] = torch.randint(1, cfg.vocab_size, (L,), generator=g)
        vi = torch.tensor([[T - L]], dtype=torch.int32)
        clip = (torch.rand(1, 16, cfg.H, cfg.W, 3, generator=g) * 255 - 120).cuda()
        a = model.forward_video(words, None, vi, clip)
        b = model.forward_video_frames(words, vi, clip[0, list(MD.FRAME_IDX)])
        for k in ("pred", "up", "sigm"):
            assert torch.equal(a[k], b[k]), (it, k)
    with pytest.raises(ValueError):
        model.forward_video_frames(words, vi, clip[0, :4])
    with pytest.raises(ValueError):
        model.forward_video_frames(words, vi, clip[0, list(MD.FRAME_IDX)].cpu())


def test_video_evaluator_tiny_exact_against_host_loop():
    model, cfg = _tiny_model()
    rng = np.random.default_rng(1)
    T = cfg.num_steps
    samples = _clips(rng, 8, T, cfg.vocab_size, [(48, 80), (100, 64), (37, 50)], [T, 2, 1, 4, T, 3, 5])
    assert any(HU.first_valid_idx(s[0]) == 0 for s in samples)
    res, per = _evaluate(model, samples)
    seg, ius, _ = _host_loop(model, samples, True)
    assert np.array_equal(per, ius)
    ref = seg.result()
    ref["samples"] = len(samples)
    assert res == ref
    assert sorted(k for k in res if k.startswith("precision@")) == sorted("precision@%s" % t for t in THR)
    seg2, _, _ = _host_loop(model, samples, False)
    for k, v in seg2.result().items():
        assert abs(res[k] - v) <= 1e-2, k
    # reproducible, and the overlapped schedule computes the same bits
    for overlap in (False, True):
        res2, per2 = _evaluate(model, samples, overlap=overlap)
        assert res2 == res and np.array_equal(per2, per), overlap


def test_video_evaluator_dcrf():
    model, cfg = _tiny_model()
    rng = np.random.default_rng(3)
    T = cfg.num_steps
    samples = _clips(rng, 4, T, cfg.vocab_size, [(48, 80), (100, 64)], [3, T])
    _, ius, seg_crf = _host_loop(model, samples, True, dcrf=True)
    for overlap in (False, True):
        ev = EV.VideoEvaluator(model, dcrf=True, overlap=overlap)
        for s in samples:
            ev.add(*s)
        res = ev.result()
        assert np.array_equal(ev.per_sample(), ius)
        for k, v in seg_crf.result().items():
            assert res["dcrf_" + k] == v, (overlap, k)


def test_video_evaluator_config5_full_size():
    """Config 5 at 320x320, L = 20, f16, on clips of A2D-like sizes: exact against the GPU-prep host loop, both schedules."""
    model = U.pkg().get_segmentation_model(NAME, mode="eval", batch_size=1, num_steps=20, H=320, W=320, dtype="f16")
    rng = np.random.default_rng(4)
    samples = _clips(rng, 3, 20, model.cfg.vocab_size, [(480, 640), (360, 640), (240, 320)], [9, 20, 4])
    res, per = _evaluate(model, samples)
    seg, ius, _ = _host_loop(model, samples, True)
    assert np.array_equal(per, ius)
    ref = seg.result()
    ref["samples"] = 3
    assert res == ref
    res2, per2 = _evaluate(model, samples, overlap=not EV.VIDEO_OVERLAP)
    assert res2 == res and np.array_equal(per2, per)


def test_evaluate_a2d_script(tmp_path):
    """examples/evaluate_a2d.py as a fresh child process on 4 .npz files in build_A2D_batches.py's layout: its printed lines equal
    VideoEvaluator.result() on the same snapshot."""
    CK = importlib.import_module("cmpc-refseg_amd.checkpoint")
    model, cfg = _tiny_model()
    snap = CK.Saver(fmt="npz").save(model, str(tmp_path / "snap"))
    rng = np.random.default_rng(6)
    samples = _clips(rng, 4, cfg.num_steps, cfg.vocab_size, [(48, 80), (100, 64)], [2, cfg.num_steps, 4])
    for n, (text, im, frames, mask) in enumerate(samples):
        np.savez(str(tmp_path / ("A2D_test_%d" % n)), text_batch=text, mask_batch=mask, sent_batch=["s"], im_batch=im, frame_id=9,
                 frames=frames)
    res, _ = _evaluate(model, samples)
    kw = "vf_h=8,vf_w=8,vf_dim=256,c4_dim=128,c3_dim=64,vocab_size=50,v_emb_dim=40,mlp_dim=24,rnn_size=40,glove_dim=12,parse_dim=20," \
         "backbone_width=8,backbone_blocks=1:1:2:1,dtype=f32"
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    p = subprocess.run([sys.executable, os.path.join(root, "examples", "evaluate_a2d.py"), "--folder", str(tmp_path), "--prefix", "A2D_test",
                        "--snapshot", snap, "--H", "64", "--W", "64", "--T", str(cfg.num_steps), "--model-kwargs", kw],
                       capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = p.stdout.strip().splitlines()
    want = ["samples = 4", "Segmentation evaluation (without DenseCRF):"] + \
        ["precision@%s = %f" % (t, res["precision@%s" % t]) for t in THR] + \
        ["overall IoU = %f; mean IoU = %f" % (res["overall_IoU"], res["mean_IoU"])]
    assert lines[-len(want):] == want
