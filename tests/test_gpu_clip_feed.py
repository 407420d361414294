"""GPU tests of training the video model from raw clips: cmpc_clip_prep against the two entries whose device code it launches, with no
allowance; train_step_video_frames against train_step_video bit for bit; feed.ClipTrainFeeder end to end against synchronous feeds of
all 16 frames, bit for bit, with the accuracy counts on; and examples/train_video_clips.py as a child process."""
import importlib
import json
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
FD = importlib.import_module("cmpc-refseg_amd.feed")
MD = importlib.import_module("cmpc-refseg_amd.model")
CK = importlib.import_module("cmpc-refseg_amd.checkpoint")
NAME = "CMPC_video_mm_tgraph_allvec"
KEY = FD.REFVOS_OBJECT_COLOR["4"]
HW = 64


def _frame(rng, h, w, phase):
    y, x = np.mgrid[0:h, 0:w]
    base = 127 + 100 * np.sin((x + phase) / 13.0)[..., None] * np.cos(y / 17.0)[..., None] * np.array([1.0, 0.7, -0.5])
    return np.clip(base + rng.normal(0, 25, (h, w, 3)), 0, 255).astype(np.uint8)


def _object(rng, h, w):
    y, x = np.mgrid[0:h, 0:w]
    cy, cx, r = rng.uniform(0.2, 0.8) * h, rng.uniform(0.2, 0.8) * w, rng.uniform(0.15, 0.35) * min(h, w)
    return (y - cy) ** 2 + (x - cx) ** 2 < r * r


def _colour(rng, m):
    a = rng.integers(0, 256, m.shape + (3,), dtype=np.uint8)
    a[..., 0][a[..., 0] == KEY[0]] = KEY[0] ^ 1        # the reference's rule: channel 0 alone decides
    a[m] = KEY
    return a


@pytest.fixture(scope="module")
def params():
    cfg = VD.tiny_cfg()
    hp, bp = VD.init_head_params(cfg), O.init_backbone_params(cfg)
    g = torch.Generator().manual_seed(3)
    for k in hp:
        if k.endswith(("biases", "beta")):
            hp[k] = (torch.randn(hp[k].shape, generator=g) * 0.05).float()
    return cfg, hp, bp


def _tiny_model(params):
    """tests/test_gpu_clip_segment.py's tiny video model, in train mode."""
    cfg, hp, bp = params
    assert (cfg.H, cfg.W) == (HW, HW)
    return U.pkg().get_segmentation_model(NAME, head_params=hp, backbone_params=bp, frames=cfg.frames, **U.model_kwargs(cfg, "f32", "train"))


# ---- 1. cmpc_clip_prep -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.timeout(120)
@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("size", [(37, 53), (64, 64)])
@pytest.mark.parametrize("coded", [True, False])
def test_clip_prep_equals_eval_prep_and_train_prep(size, order, coded):
    rng = np.random.default_rng([size[0], order, coded])
    h, w = size
    frames = [_frame(rng, h, w, 3 * k) for k in range(5)]
    m = _object(rng, h, w)
    ann, key = (_colour(rng, m), KEY) if coded else (m, None)
    feed, tgt, pos = FD.prepare_clip(frames, ann, key, HW, HW, order=order)
    want_feed, _ = EV.prepare_images(frames, HW, HW)
    want_tgt, want_pos = FD.prepare_targets([ann], [key], HW, HW, order=order)
    torch.cuda.synchronize()
    assert feed.dtype == torch.float32 and tuple(feed.shape) == (5, HW, HW, 3) and torch.equal(feed, want_feed)
    assert tuple(tgt.shape) == (1, HW, HW, 1) and torch.equal(tgt, want_tgt)
    assert pos.dtype == torch.int64 and torch.equal(pos, want_pos) and int(pos[0]) == int(tgt.sum()) > 0
    if size == (HW, HW):                               # the identity geometry: a stored train sample passes through unchanged
        assert np.array_equal(tgt[0, :, :, 0].cpu().numpy(), m.astype(np.float32))
        want = (np.stack(frames)[..., ::-1].astype(np.float64) - HU.MU).astype(np.float32)
        assert np.array_equal(feed.cpu().numpy(), want)


@pytest.mark.timeout(120)
def test_prepare_clip_refusals():
    rng = np.random.default_rng(0)
    fr = [_frame(rng, 20, 30, k) for k in range(5)]
    for bad in (lambda: FD.prepare_clip(fr + fr, np.ones((20, 30), bool), None, HW, HW),
                lambda: FD.prepare_clip([], np.ones((20, 30), bool), None, HW, HW),
                lambda: FD.prepare_clip(fr[:4] + [fr[4][:-1]], np.ones((20, 30), bool), None, HW, HW),
                lambda: FD.prepare_clip(fr, np.ones((20, 31), bool), None, HW, HW),
                lambda: FD.prepare_clip(fr, np.ones((20, 30), bool), None, HW, HW, order=2)):
        with pytest.raises(ValueError):
            bad()


# ---- 2. train_step_video_frames ---------------------------------------------------------------------------------------------------------------
def _bits(v):
    return v.cpu().view(torch.int32).item() if torch.is_tensor(v) else float(v)


def _same_scalars(a, b, tag):
    assert set(a) == set(b), tag
    for k in a:
        if k == "accuracy_counts":
            assert torch.equal(a[k], b[k]), (tag, k)
        else:
            assert _bits(a[k]) == _bits(b[k]), (tag, k, a[k], b[k])


def _same_state(ma, mb):
    sa, sb = ma.state_dict(), mb.state_dict()
    assert set(sa) == set(sb)
    for k in sb:
        assert torch.equal(sa[k].cpu(), sb[k].cpu()), k
    va, vb = CK.model_variables(ma), CK.model_variables(mb)      # everything a snapshot holds: weights, Adam slots, the global step
    assert set(va) == set(vb)
    for k in vb:
        assert np.array_equal(np.asarray(va[k]), np.asarray(vb[k])), k


@pytest.mark.timeout(300)
def test_train_step_video_frames_is_train_step_video(params):
    """Two models from the same parameters, 4 steps in f32: one is fed the host clip of 16 frames and front-padded words, the other the 5
    sampled frames on the device and video_words' output.  Scalars bit for bit, the state afterwards with torch.equal."""
    cfg = params[0]
    ma, mb = _tiny_model(params), _tiny_model(params)
    T = cfg.num_steps
    for s in range(4):
        words, clip, tgt = VD.synth_clip(cfg, seed=10 + s)
        vi = torch.tensor([[int((words[0] == 0).sum())]], dtype=torch.int32)
        _, sa = ma.train_step_video(words, None, tgt, vi, clip, accuracy=bool(s % 2))
        we, sl = MD.video_words(words, vi, T)
        fr = torch.as_tensor(np.asarray(clip), dtype=torch.float32)[0, list(MD.FRAME_IDX)].contiguous().cuda()
        tg = torch.as_tensor(np.asarray(tgt), dtype=torch.float32).cuda()
        if s >= 2:                                      # ids and length from the device as well
            we, sl = torch.from_numpy(we).cuda(), torch.from_numpy(sl).cuda()
        _, sb = mb.train_step_video_frames(we, sl, fr, tg, accuracy=bool(s % 2))
        torch.cuda.synchronize()
        assert set(sa) == {"loss_all", "loss_c3", "loss_c4", "loss_c5", "loss_last", "mean_IOU", "learning_rate"} | ({"accuracy_counts"} if s % 2 else set())
        _same_scalars(sa, sb, s)
        if s % 2:
            assert torch.equal(sb["accuracy_counts"], EV.train_accuracy(mb.eng.tap("pred"), tg))
            assert int(sb["accuracy_counts"][0, :2].sum()) == cfg.vf_h * cfg.vf_w
    _same_state(ma, mb)
    fr = torch.zeros(5, HW, HW, 3, device="cuda")
    tg = torch.zeros(1, HW, HW, 1, device="cuda")
    we, sl = np.ones((1, T), np.int32), np.array([T], np.int32)
    for bad in (lambda: mb.train_step_video_frames(we, sl, fr[:4], tg), lambda: mb.train_step_video_frames(we, sl, fr.cpu(), tg),
                lambda: mb.train_step_video_frames(we, sl, fr, tg.cpu()), lambda: mb.train_step_video_frames(we, sl, fr, tg[:, :32]),
                lambda: mb.train_step_video_frames(we[:, :-1], sl, fr, tg), lambda: mb.train_step_video_frames(we, sl.reshape(1, 1), fr, tg)):
        with pytest.raises(ValueError):
            bad()


# ---- 3. ClipTrainFeeder -------------------------------------------------------------------------------------------------------------------------
VOCAB = {w: i for i, w in enumerate(["<pad>", "<unk>", "a", "red", "dog", "on", "the", "left", "car", "small"])}
SENTS = ["a red dog", "the dog on the left.", "dog", "a small red car on the left"]
SIZES = [(37, 53), (64, 64), (48, 80), (90, 70)]


class _Clips:
    """Clip i is a function of i: 16 frames of one of four sizes, a colour-coded or a plain annotation, the three text forms by i % 3."""

    def __init__(self, n, T):
        self.n, self.T = n, T

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        rng = np.random.default_rng(1000 + i)
        h, w = SIZES[i % len(SIZES)]
        frames = [_frame(rng, h, w, 3 * k + i) for k in range(16)]
        m = _object(rng, h, w)
        sent = SENTS[i % len(SENTS)]
        ids, sl = HU.preprocess_sentence_lstm(sent, VOCAB, self.T)
        text = (sent, (np.array(ids), sl), np.array(HU.preprocess_sentence(sent, VOCAB, self.T)))[i % 3]
        if i % 2:
            return frames, m, None, text
        return np.stack(frames), _colour(rng, m), KEY, text


def _sync_step(model, sample, T, accuracy=False):
    """The driver's feeds from one raw clip: all 16 frames resized, a host clip, front-padded words and valid_idx; then a synchronise."""
    frames, ann, key, text = sample
    feed, _ = EV.prepare_images(list(frames), HW, HW)
    tgt, _ = FD.prepare_targets([ann], [key], HW, HW)
    ids, n = FD.encode_text(text, VOCAB, T)
    words = np.zeros((1, T), np.int64)
    words[0, T - n:] = ids[:n]
    _, scal = model.train_step_video(words, None, tgt, np.array([[T - n]], np.int32), feed.cpu()[None], accuracy=accuracy)
    torch.cuda.synchronize()
    return scal, tgt


@pytest.mark.timeout(600)
def test_clip_feeder_trains_bit_identically_to_synchronous_feeds(params):
    """Two models from the same parameters.  One is driven by ClipTrainFeeder (side stream, ring reuse, accuracy counts on) for 14 steps:
    past both backbone-graph captures, 3.5 times round the ring of 4 slots, 14 distinct clips.  The other gets prepare_images of all 16
    frames as a host clip, front-padded words and train_step_video without the accuracy, with a synchronise per step.  Every step's
    scalars and the final state are bit-identical, and the feeder's counts equal the op on the synchronous side's pred and target."""
    cfg = params[0]
    T, steps = cfg.num_steps, 14
    n = steps + 4                                       # the feeder stages ahead of the last step: those clips exist too
    data = _Clips(n, T)
    stream = [int(i) for i in FD.EpochSampler(n, shuffle=True, seed=5).epoch_indices(0)]
    ma = _tiny_model(params)
    fd = FD.ClipTrainFeeder(ma, data, sampler=FD.EpochSampler(n, shuffle=True, seed=5), vocab=VOCAB, depth=2, max_hw=(96, 96))
    assert len(fd.stage.im) == 4 and tuple(fd.stage.im[0].shape) == (5, HW, HW, 3)
    got, fed, slots = [], [], []
    for _ in range(steps):
        step, scal = fd.step(accuracy=True)
        got.append(scal)                                # device scalars: read after the loop, nothing synchronises inside it
        fed.append(list(fd.last_feed["indices"]))
        slots.append(fd.last_feed["slot"])
        f = fd.last_feed
        assert f["words"].dtype == torch.int32 and tuple(f["words"].shape) == (1, T) and tuple(f["seq_len"].shape) == (1,)
        assert tuple(f["frames"].shape) == (5, HW, HW, 3) and tuple(f["target_fine"].shape) == (1, HW, HW, 1) and tuple(f["pos"].shape) == (1,)
    torch.cuda.synchronize()
    fd.close()
    assert fed == [[i] for i in stream[:steps]] and len({i for f in fed for i in f}) == steps
    assert len(set(slots)) == 4 and len(slots) > 3 * 4
    mb = _tiny_model(params)
    for s in range(steps):
        scal, tgt = _sync_step(mb, data[fed[s][0]], T)
        counts = got[s].pop("accuracy_counts")
        _same_scalars(got[s], scal, s)
        assert torch.equal(counts, EV.train_accuracy(mb.eng.tap("pred"), tgt)), s
    _same_state(ma, mb)


# ---- 4. the example script ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.timeout(900)
def test_train_video_clips_script(tmp_path, params):
    """examples/train_video_clips.py as a fresh child process on 6 tiny .npz train samples (build_A2D_batches.py's layout, already at
    H x W): the lines it prints equal TrainLog over the synchronous loop in this process, and it writes its snapshot."""
    cfg = params[0]
    T, n, iters = cfg.num_steps, 6, 8
    data = tmp_path / "train_batch"
    data.mkdir()
    samples = []
    for i in range(n):
        rng = np.random.default_rng(50 + i)
        frames = np.stack([_frame(rng, HW, HW, 3 * k + i) for k in range(16)])
        mask = _object(rng, HW, HW)
        text = np.array(HU.preprocess_sentence(SENTS[i % len(SENTS)], VOCAB, T))
        np.savez(str(data / ("a2d_train_%d.npz" % i)), text_batch=text, mask_batch=mask, sent_batch=[SENTS[i % len(SENTS)]],
                 im_batch=frames[8], frame_id=i, frames=frames)
        samples.append((frames, mask, None, text))
    model = _tiny_model(params)
    snap = CK.Saver(fmt="npz").save(model, str(tmp_path / "init"))
    order = FD.EpochSampler(n, shuffle=True, seed=3)
    log, want = HU.TrainLog(iters_per_log=3), []
    for it in range(iters):
        scal, _ = _sync_step(model, samples[next(order)], T, accuracy=True)
        log.add(it, scal["loss_last"], scal["learning_rate"], scal["accuracy_counts"])
        want += log.lines(it)
    assert len(want) == 9 and sum("accuracy (cur)" in l for l in want) == 3
    kw = json.dumps(dict(vf_h=8, vf_w=8, vf_dim=256, c4_dim=128, c3_dim=64, vocab_size=50, v_emb_dim=40, mlp_dim=24, rnn_size=40, glove_dim=12,
                         parse_dim=20, backbone_width=8, backbone_blocks=[1, 1, 2, 1], dtype="f32"))
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = tmp_path / "ckpt"
    cmd = [sys.executable, os.path.join(root, "examples", "train_video_clips.py"), "--data", str(data), "--iters", str(iters), "--snapshot", "100",
           "--out", str(out), "--restore", snap, "--iters-per-log", "3", "--seed", "3", "--H", str(HW), "--W", str(HW), "--T", str(T),
           "--lr", repr(cfg.start_lr), "--lr-decay-step", str(cfg.lr_decay_step), "--model-kwargs", kw]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = p.stdout.splitlines()
    assert [l for l in lines if l.startswith("iter = ")] == want
    assert any(l.startswith("snapshot saved to ") for l in lines) and lines[-1] == "Optimization done."
    assert CK.latest_checkpoint(str(out / "a2d_iter")) is not None
