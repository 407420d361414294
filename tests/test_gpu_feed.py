"""GPU tests of the training feed (cmpc-refseg_amd/feed.py): cmpc_train_prep against hostutil.train_sample with no allowance on the
targets, the image half against evaluate.prepare_images, and TrainFeeder end to end against synchronous feeds, bit for bit."""
import importlib
import types

import numpy as np
import pytest
import torch

from tests import util as U
from tests.util import O

pytestmark = pytest.mark.gpu

HU = importlib.import_module("cmpc-refseg_amd.hostutil")
EV = importlib.import_module("cmpc-refseg_amd.evaluate")
FD = importlib.import_module("cmpc-refseg_amd.feed")
pkg = importlib.import_module("cmpc-refseg_amd")

SIZES = [(720, 1280), (480, 640), (333, 500), (240, 427), (100, 50), (320, 320), (50, 900), (37, 61), (640, 480), (1, 7), (321, 319)]
KEY = FD.REFVOS_OBJECT_COLOR["3"]


def _blobs(rng, h, w, n=4):
    y, x = np.mgrid[0:h, 0:w]
    m = np.zeros((h, w), bool)
    for _ in range(n):
        cy, cx, r = rng.uniform(0, h), rng.uniform(0, w), rng.uniform(0.05, 0.3) * max(2, min(h, w))
        m |= (y - cy) ** 2 + (x - cx) ** 2 < r * r
    return m


def _mask(rng, h, w, kind):
    m = np.zeros((h, w), bool)
    if kind == "blobs":
        m = _blobs(rng, h, w)
    elif kind == "pixel":
        m[int(rng.integers(h)), int(rng.integers(w))] = True
    elif kind == "corner":
        m[h - 1, w - 1] = True
    elif kind == "border_row":
        m[0, :] = True
    elif kind == "border_col":
        m[:, w - 1] = True
    elif kind == "noise":
        m = rng.random((h, w)) < 0.02
    elif kind != "empty":
        raise ValueError(kind)
    return m


def _colour(rng, m, channels):
    """A colour-coded annotation whose object (the reference's rule: channel 0 equals the key's) is exactly m: other objects and the
    background never carry the key's R; a third of the object's pixels differ from the key in G and B."""
    h, w = m.shape
    a = rng.integers(0, 256, (h, w, channels), dtype=np.uint8)
    a[..., 0][a[..., 0] == KEY[0]] = KEY[0] ^ 1
    a[m, :3] = KEY
    off = m & (rng.random((h, w)) < 1 / 3)
    a[off, 1] = KEY[1] ^ 0x55
    a[off, 2] = KEY[2] ^ 0x0F
    return a


def _image(rng, h, w, gray=False):
    y, x = np.mgrid[0:h, 0:w]
    base = 127 + 100 * np.sin(x / 17.0)[..., None] * np.cos(y / 23.0)[..., None] * np.array([1.0, 0.7, -0.5])
    im = np.clip(base + rng.normal(0, 25, (h, w, 3)), 0, 255).astype(np.uint8)
    return im[..., 0] if gray else im


def _cases(rng, HW):
    """(annotation, key) over the source sizes (already H x W, up- and down-scaling, portrait, 1 pixel high) and the mask kinds, the
    two annotation kinds alternating; plain masks in several dtypes."""
    kinds = ["blobs", "noise", "pixel", "border_row", "border_col", "blobs", "corner", "blobs", "empty", "noise", "blobs"]
    out = []
    sizes = SIZES + [(HW, HW)]
    extra = [((480, 640), k) for k in ("pixel", "corner", "border_row", "border_col", "empty")] + \
            [((37, 61), k) for k in ("pixel", "border_col", "empty")] + [((720, 1280), "pixel"), ((720, 1280), "border_row")]
    for i, ((h, w), k) in enumerate(list(zip(sizes, kinds + ["blobs"])) + extra):
        m = _mask(rng, h, w, k)
        if i % 2 == 0:
            out.append((_colour(rng, m, 3 + (i // 2) % 2), KEY, (h, w, k)))
        else:
            out.append(((m * (1, 255, 3.5)[i % 3]).astype((np.uint8, np.int32, np.float32)[i % 3]), None, (h, w, k)))
    return out


@pytest.mark.parametrize("order", [1, 0])
@pytest.mark.parametrize("HW", [320, 512, 64])
def test_targets_equal_host(HW, order):
    rng = np.random.default_rng(100 * HW + order)
    cases = _cases(rng, HW)
    ref = [HU.train_sample(np.zeros(a.shape[:2], np.uint8), a, k, HW, HW, order=order)[1] for a, k, _ in cases]
    # mixed batches of 8; sample 0 rides again in every later batch at a moving position: a result must not depend on the neighbours
    B = 8
    n_bad = 0
    for s0 in range(0, len(cases), B - 1):
        idx = list(range(s0, min(s0 + B - 1, len(cases))))
        idx.insert((s0 // (B - 1)) % (len(idx) + 1), 0)
        tgt, pos = FD.prepare_targets([cases[i][0] for i in idx], [cases[i][1] for i in idx], HW, HW, order=order)
        assert tgt.shape == (len(idx), HW, HW, 1) and tgt.dtype == torch.float32 and pos.dtype == torch.int64
        tgt, pos = tgt.cpu().numpy(), pos.cpu().numpy()
        for j, i in enumerate(idx):
            diff = int((tgt[j] != ref[i]).sum())
            print("HW %d order %d sample %s: %d differing pixels, pos %d (host %d)" % (HW, order, cases[i][2], diff, pos[j], int(ref[i].sum())))
            n_bad += diff != 0 or int(pos[j]) != int(ref[i].sum())
            assert np.array_equal(tgt[j], ref[i]), (HW, order, cases[i][2], diff)
            assert int(pos[j]) == int(ref[i].sum()), (HW, order, cases[i][2])
    assert n_bad == 0


def test_strict_colour_rule_and_alpha():
    """match=3 demands all of R, G, B; the alpha channel never takes part."""
    rng = np.random.default_rng(5)
    m = _blobs(rng, 240, 427)
    a = _colour(rng, m, 4)
    strict = np.all(a[..., :3] == np.array(KEY, np.uint8), axis=2)
    assert strict.sum() < m.sum() and strict.any()
    for match, obj in ((1, m), (3, strict)):
        tgt, pos = FD.prepare_targets([a, a[..., :3].copy()], [KEY, KEY], 320, 320, match=match)
        ref = HU.train_sample(np.zeros((240, 427), np.uint8), a, KEY, 320, 320, match=match)[1]
        assert np.array_equal(ref, (HU.resize_and_pad(obj, 320, 320) > 0).astype(np.float32)[..., None])
        for b in range(2):
            assert np.array_equal(tgt[b].cpu().numpy(), ref) and int(pos[b]) == int(ref.sum())


@pytest.mark.parametrize("HW", [320, 512])
def test_feed_equals_prepare_images_and_host(HW):
    rng = np.random.default_rng(HW + 1)
    sizes = [(480, 640), (333, 500), (240, 427), (100, 50), (HW, HW), (50, 900), (720, 1280)]
    ims = [_image(rng, h, w) for h, w in sizes] + [_image(rng, 240, 427, gray=True)]
    anns = [_blobs(rng, *im.shape[:2]) for im in ims]
    feed, tgt, pos = FD.prepare_batch(ims, anns, None, HW, HW)
    feed_ev, proc = EV.prepare_images(ims, HW, HW, "cuda:0")
    assert torch.equal(feed.view(torch.int32), feed_ev.view(torch.int32))          # bit-identical to the evaluation feed
    feed, proc = feed.cpu().numpy(), proc.cpu().numpy()
    for b, (im, an) in enumerate(zip(ims, anns)):
        ref_feed, ref_t = HU.train_sample(im, an, None, HW, HW)
        assert np.array_equal(tgt[b].cpu().numpy(), ref_t)
        # tests/test_gpu_eval.py::test_prepare_images_matches_host's criterion: levels differ by <= 1 on <= 1e-3 of the pixels
        ref = HU.img_as_ubyte(HU.resize_and_pad(im, HW, HW))
        if ref.ndim == 2:
            ref = np.repeat(ref[..., None], 3, 2)
        diff = np.abs(proc[b].astype(int) - ref.astype(int))
        assert diff.max() <= 1 and (diff > 0).mean() <= 1e-3, (im.shape, diff.max(), (diff > 0).mean())
        same = diff.max(axis=2) == 0
        assert np.array_equal(feed[b][same].view(np.uint32), ref_feed[same].view(np.uint32))


VOCAB = {w: i for i, w in enumerate(["<pad>", "<unk>", "the", "a", "red", "blue", "left", "right", "dog", "cat", "man", "woman", "car", "on", "of"])}


class _Raw:
    """A synthetic raw data set: random-size images, colour-coded or plain annotations, sentences; sample i is a function of i alone."""

    def __init__(self, n, T, empty_every=0):
        self.n, self.T, self.empty_every = n, T, empty_every

    def __len__(self):
        return self.n

    def is_empty(self, i):
        return bool(self.empty_every) and i % self.empty_every == 1

    def __getitem__(self, i):
        rng = np.random.default_rng(1000 + i)
        h, w = int(rng.integers(20, 128)), int(rng.integers(20, 160))
        im = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        m = _mask(rng, h, w, "empty" if self.is_empty(i) else "blobs")
        if not self.is_empty(i):
            m[h // 2, w // 2] = True
        words = list(VOCAB)[2:]
        sent = " ".join(words[int(k)] for k in rng.integers(0, len(words), int(rng.integers(1, self.T + 1))))
        if i % 2:
            return im, m.astype(np.uint8) * 255, None, sent
        return im, _colour(rng, m, 3), KEY, sent


def _stub_model(B, T, HW):
    return types.SimpleNamespace(batch_size=B, num_steps=T, H=HW, W=HW, device=torch.device("cuda:0"), video=False, MAX_STEPS_IN_FLIGHT=2)


@pytest.mark.parametrize("skip", [False, True])
def test_skip_empty_and_pos_agree_with_host(skip):
    B, T, HW, n = 4, 6, 64, 23
    data = _Raw(n, T, empty_every=3)
    order = [i for e in range(3) for i in FD.EpochSampler(n, seed=4).epoch_indices(e)]
    kept = [i for i in order if not (skip and data.is_empty(i))]
    with FD.TrainFeeder(_stub_model(B, T, HW), data, sampler=FD.EpochSampler(n, seed=4), vocab=VOCAB, skip_empty=skip, max_hw=(128, 160)) as fd:
        k = 0
        for _ in range(9):
            f = next(fd)
            torch.cuda.current_stream().wait_event(f["ready"])
            assert f["indices"] == kept[k: k + B]
            tgt, pos, words, sl = f["target_fine"].cpu().numpy(), f["pos"].cpu().numpy(), f["words"].cpu().numpy(), f["seq_len"].cpu().numpy()
            for b, i in enumerate(f["indices"]):
                im, an, key, sent = data[i]
                ref = HU.train_sample(im, an, key, HW, HW)[1]
                assert np.array_equal(tgt[b], ref) and int(pos[b]) == int(ref.sum())
                assert (int(pos[b]) == 0) == data.is_empty(i)
                ids, sn = HU.preprocess_sentence_lstm(sent, VOCAB, T)
                assert words[b].tolist() == ids and int(sl[b]) == sn and f["sentences"][b] == sent
            k += B
            # the samples dropped in the stream up to this batch's last sample
            upto = _stream_position(order, kept, k, skip, data)
            assert fd.skipped == (sum(data.is_empty(i) for i in order[:upto]) if skip else 0)


def _stream_position(order, kept, k, skip, data):
    """Position in `order` just behind the k-th kept sample."""
    seen = 0
    for p, i in enumerate(order):
        if not (skip and data.is_empty(i)):
            seen += 1
            if seen == k:
                return p + 1
    raise AssertionError("stream too short")


def test_feeder_refuses_the_video_model():
    with pytest.raises(ValueError):
        FD.TrainFeeder(types.SimpleNamespace(video=True), [], vocab=VOCAB)


@pytest.mark.parametrize("lookahead", [True, False])
def test_feeder_trains_bit_identically_to_synchronous_feeds(lookahead):
    """Two models from the same parameters.  One is driven by TrainFeeder (side stream, ring reuse; with lookahead the next batch's
    backbone pass inside the current step, as train_step's next_im places it) for 14 steps --
    past both backbone-graph captures, 3.5 times round the ring of 4 slots, 28 distinct samples; the other gets prepare_batch's feeds on
    the default stream with a synchronise between steps.  Every step's scalars and the final state are bit-identical: a stale or
    early-reused buffer would show as a difference."""
    cfg = U.tiny_cfg()
    hp, bp = O.init_head_params(cfg), O.init_backbone_params(cfg)
    B, T, HW, steps = cfg.batch_size, cfg.num_steps, cfg.H, 14
    n = steps * B + 2 * B * 2                      # the feeder stages ahead of the last step: those samples exist too
    data = _Raw(n, T)
    stream = [i for i in FD.EpochSampler(n, shuffle=True, seed=9).epoch_indices(0)]

    ma = pkg.LSTM_model(head_params=hp, backbone_params=bp, **U.model_kwargs(cfg, "f32"))
    fd = FD.TrainFeeder(ma, data, sampler=FD.EpochSampler(n, shuffle=True, seed=9), vocab=VOCAB, depth=2, max_hw=(128, 160), lookahead=lookahead)
    assert len(fd.stage.im) == 4
    got, fed = [], []
    for _ in range(steps):
        step, scal = fd.step()
        got.append(scal)                            # device scalars: read after the loop, nothing synchronises inside it
        fed.append(list(fd.last_feed["indices"]))
    torch.cuda.synchronize()
    fd.close()
    assert fed == [stream[s * B: (s + 1) * B] for s in range(steps)]
    assert len({i for f in fed for i in f}) == steps * B >= 3 * 4 * B
    state_a = {k: v.clone() for k, v in ma.state_dict().items()}

    mb = pkg.LSTM_model(head_params=hp, backbone_params=bp, **U.model_kwargs(cfg, "f32"))
    for s in range(steps):
        raw = [data[i] for i in fed[s]]
        im, tgt, _ = FD.prepare_batch([r[0] for r in raw], [r[1] for r in raw], [r[2] for r in raw], HW, HW)
        enc = [FD.encode_text(r[3], VOCAB, T) for r in raw]
        words = np.stack([e[0] for e in enc])
        sl = np.array([e[1] for e in enc], np.int32)
        _, scal = mb.train_step(words, im, tgt, sl)
        torch.cuda.synchronize()
        for k in scal:
            a, b = got[s][k], scal[k]
            a, b = (float(a), float(b)) if not torch.is_tensor(a) else (a.cpu().view(torch.int32).item(), b.cpu().view(torch.int32).item())
            assert a == b, (s, k, got[s][k], scal[k])
    state_b = mb.state_dict()
    assert set(state_a) == set(state_b)
    for k in state_b:
        assert torch.equal(state_a[k].cpu(), state_b[k].cpu()), k
