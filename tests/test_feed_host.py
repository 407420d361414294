"""CPU tests of the training feed's host half (cmpc-refseg_amd/feed.py, hostutil.train_sample): the object rules, the order-0 resampler,
descriptor planning, cmpc_train_prep's argument checks before anything is launched (the library loads without a GPU), EpochSampler, and
TrainFeeder's pipeline with a stub in place of the device stage."""
import importlib
import types

import numpy as np
import pytest
from scipy import ndimage as ndi

HU = importlib.import_module("cmpc-refseg_amd.hostutil")
FD = importlib.import_module("cmpc-refseg_amd.feed")
L = importlib.import_module("cmpc-refseg_amd._lib")

KEY = FD.REFVOS_OBJECT_COLOR["1"]


def test_object_colours_are_the_readers():
    assert FD.REFVOS_OBJECT_COLOR == {"1": (236, 95, 103), "2": (249, 145, 87), "3": (250, 200, 99), "4": (153, 199, 148),
                                      "5": (98, 179, 178), "6": (102, 153, 204)}


def test_object_rules_on_hand_worked_pixels():
    # one row: the key itself; R alone equal; G and B equal but not R; another object's colour; black
    ann = np.array([[KEY, (236, 0, 0), (0, 95, 103), FD.REFVOS_OBJECT_COLOR["2"], (0, 0, 0)]], dtype=np.uint8)
    assert HU.object_mask(ann, KEY).tolist() == [[True, True, False, False, False]]              # (mask == color)[:, :, 0]
    assert HU.object_mask(ann, KEY, match=3).tolist() == [[True, False, False, False, False]]
    assert HU.object_mask(ann, KEY, match=2).tolist() == [[True, False, False, False, False]]
    # alpha is ignored, whatever it holds
    rgba = np.concatenate([ann, np.array([[[0], [255], [7], [236], [95]]], np.uint8)], axis=2)
    assert np.array_equal(HU.object_mask(rgba, KEY), HU.object_mask(ann, KEY))
    assert np.array_equal(HU.object_mask(rgba, KEY, match=3), HU.object_mask(ann, KEY, match=3))
    # plain masks: non-zero of any dtype
    assert HU.object_mask(np.array([[0, 2, -1]], np.int32)).tolist() == [[False, True, True]]
    assert HU.object_mask(np.array([[0.0, 0.25]], np.float32)[..., None]).tolist() == [[False, True]]
    for bad in (np.zeros((2, 2, 2), np.uint8), np.zeros((2, 2, 3), np.float32), np.zeros((0, 2, 3), np.uint8)):
        with pytest.raises(ValueError):
            HU.object_mask(bad, KEY)
    with pytest.raises(ValueError):
        HU.object_mask(ann, KEY, match=4)


def test_train_sample_hand_worked():
    # a 2 x 4 sample into 4 x 4: scale 1, resized 2 x 4 centred at rows 1..2, everything else padding
    im = np.arange(24, dtype=np.uint8).reshape(2, 4, 3)
    ann = np.zeros((2, 4, 3), np.uint8)
    ann[0, 1] = KEY
    ann[1, 3] = (236, 1, 2)
    feed, tgt = HU.train_sample(im, ann, KEY, 4, 4)
    assert feed.shape == (4, 4, 3) and feed.dtype == np.float32 and tgt.shape == (4, 4, 1) and tgt.dtype == np.float32
    want = np.zeros((4, 4), np.float32)
    want[1, 1] = want[2, 3] = 1
    assert np.array_equal(tgt[..., 0], want)
    assert np.array_equal(HU.train_sample(im, ann, KEY, 4, 4, match=3)[1][..., 0], np.float32(want * [[0], [1], [0], [0]]))
    mu = np.float32(HU.MU)
    assert np.allclose(feed[0], -mu) and np.allclose(feed[3], -mu)                            # padding: 0 - mu
    assert np.array_equal(feed[1:3], (im[..., ::-1].astype(np.float64) - HU.MU).astype(np.float32))
    # a grey image is tiled to three channels (build_batches.py:67-68); the plain mask of the same object gives the same target
    g, t2 = HU.train_sample(im[..., 0].copy(), HU.object_mask(ann, KEY).astype(np.int64) * 7, None, 4, 4)
    assert np.array_equal(t2, tgt) and g.shape == (4, 4, 3)
    assert np.array_equal(g[1:3], (np.repeat(im[..., :1], 3, 2).astype(np.float64) - HU.MU).astype(np.float32))
    # up-scaling by 2 (order 1): the bilinear taps spread one pixel over the outputs whose taps reach it with non-zero weight
    m = np.zeros((2, 2), bool)
    m[0, 0] = True
    t = HU.train_sample(np.zeros((2, 2), np.uint8), m, None, 4, 4)[1][..., 0]
    assert np.array_equal(t, (HU.resize_and_pad(m, 4, 4) > 0).astype(np.float32)) and t[:3, :3].all()
    t0 = HU.train_sample(np.zeros((2, 2), np.uint8), m, None, 4, 4, order=0)[1][..., 0]
    assert t0.sum() == 4 and t0[:2, :2].all()                                                 # nearest: the pixel's own 2 x 2 block
    with pytest.raises(ValueError):
        HU.train_sample(im, ann, KEY, 4, 4, order=2)
    with pytest.raises(ValueError):
        HU.train_sample(im.astype(np.float32), ann, KEY, 4, 4)


def _or_of_taps(m, H, W):
    """What the mask kernel computes for order 1, restated in NumPy: per axis the zoom's two taps (the second only when its weight
    1 - (1 - t) is non-zero), each widened by the Gaussian radius and clipped to the image; the OR over that rectangle."""
    h, w = m.shape
    rh, rw, top, left = HU.resize_and_pad_geometry(h, w, H, W)

    def taps(n_in, n_out, shrink_any):
        z = n_in / n_out
        r = 0
        if shrink_any:
            s = max(0.0, (z - 1) / 2)
            r = int(4 * s + 0.5) if s > 1e-15 else 0
        out = []
        for o in range(n_out):
            cc = (o + 0.5) * z - 0.5
            cc = 0.0 if n_in == 1 else (-cc if cc < 0 else cc)
            f = int(np.floor(cc))
            t = cc - f
            idx = [f] + ([f + 1] if 1.0 - (1.0 - t) != 0.0 else [])
            p = 2 * (n_in - 1)
            mir = [0 if n_in == 1 else (abs(i) % p if abs(i) % p < n_in else p - abs(i) % p) for i in idx]
            out.append([(max(0, c - r), min(n_in - 1, c + r)) for c in mir])
        return out

    shrink = (h, w) != (rh, rw) and max(h / rh, w / rw) > 1
    ty, tx = taps(h, rh, shrink), taps(w, rw, shrink)
    out = np.zeros((H, W), bool)
    for y in range(rh):
        rows = np.zeros(h, bool)
        for a, b in ty[y]:
            rows[a: b + 1] = True
        sub = m[rows].any(axis=0)
        for x in range(rw):
            out[top + y, left + x] = any(sub[a: b + 1].any() for a, b in tx[x])
    return out


@pytest.mark.parametrize("shape,HW", [((37, 61), 64), ((100, 50), 64), ((1, 7), 64), ((64, 64), 64), ((130, 97), 64), ((50, 300), 64), ((21, 33), 96)])
def test_or_of_taps_equals_float_resampler(shape, HW):
    rng = np.random.default_rng(shape[0])
    for m in (rng.random(shape) < 0.02, rng.random(shape) < 0.5, np.zeros(shape, bool)):
        assert np.array_equal(_or_of_taps(m, HW, HW), HU.resize_and_pad(m, HW, HW) > 0)
    edge = np.zeros(shape, bool)
    edge[-1, :] = True
    assert np.array_equal(_or_of_taps(edge, HW, HW), HU.resize_and_pad(edge.astype(np.float32), HW, HW) > 0)


@pytest.mark.parametrize("shape,HW", [((720, 1280), 320), ((100, 50), 320), ((37, 61), 64), ((1, 7), 64), ((321, 319), 320), ((50, 900), 512), ((64, 64), 64)])
def test_order0_is_ndimage_zoom_order0(shape, HW):
    rng = np.random.default_rng(shape[1])
    m = rng.random(shape) < 0.3
    h, w = shape
    rh, rw, top, left = HU.resize_and_pad_geometry(h, w, HW, HW)
    got = HU.resize_and_pad_order0(m, HW, HW)
    want = np.zeros((HW, HW), bool)
    want[top: top + rh, left: left + rw] = m if (h, w) == (rh, rw) else ndi.zoom(m.astype(np.float64), (rh / h, rw / w), order=0, mode="mirror", grid_mode=True) > 0
    assert np.array_equal(got, want)
    # the source index the kernel uses: the sample nearest (o + 0.5) in / out - 0.5
    iy = np.clip(np.floor(((np.arange(rh) + 0.5) * (h / rh) - 0.5) + 0.5).astype(int), 0, h - 1)
    ix = np.clip(np.floor(((np.arange(rw) + 0.5) * (w / rw) - 0.5) + 0.5).astype(int), 0, w - 1)
    assert np.array_equal(got[top: top + rh, left: left + rw], m[iy][:, ix])
    assert np.array_equal(HU.train_sample(np.zeros(shape, np.uint8), m, None, HW, HW, order=0)[1][..., 0], want.astype(np.float32))


def test_planner():
    shapes = [(480, 640, 3), (333, 500, 4), (100, 50), (64, 64, 3)]
    kinds = [L.ANN_COLOR, L.ANN_COLOR, L.ANN_PLAIN, L.ANN_COLOR]
    keys = [KEY, (1, 2, 3), (0, 0, 0), KEY]
    d, nbytes = FD.plan_targets(shapes, kinds, keys, 64, 64)
    off = 0
    for di, s, kd, ky in zip(d, shapes, kinds, keys):
        c = s[2] if len(s) == 3 else 1
        assert (di.h, di.w, di.c, di.kind) == (s[0], s[1], c, kd)
        assert (di.rh, di.rw, di.top, di.left) == HU.resize_and_pad_geometry(s[0], s[1], 64, 64)
        assert di.match == (1 if kd == L.ANN_COLOR else 0) and tuple(di.key)[:3] == tuple(ky)
        assert di.offset == off and off % 16 == 0
        off += -(-s[0] * s[1] * c // 16) * 16
    assert nbytes == off
    assert FD.plan_targets(shapes[:1], kinds[:1], keys[:1], 64, 64, match=3)[0][0].match == 3
    with pytest.raises(ValueError):
        FD.plan_targets(shapes, kinds, keys, 64, 64, match=0)
    with pytest.raises(ValueError):
        FD.plan_targets([(4, 4, 3)] * (L.EVAL_MAX_BATCH + 1), [0] * 33, [KEY] * 33, 32, 32)
    a, kind, key = FD.annotation_u8(np.array([[0, 3], [0.5, 0]]), None)
    assert a.dtype == np.uint8 and a.tolist() == [[0, 1], [1, 0]] and kind == L.ANN_PLAIN
    for bad, k in ((np.zeros((4, 4, 2), np.uint8), KEY), (np.zeros((4, 4, 3), np.int32), KEY), (np.zeros((4,), np.uint8), None),
                   (np.zeros((4, 4, 3), np.uint8), (1, 2)), (np.zeros((4, 4, 3), np.uint8), (1, 2, 300))):
        with pytest.raises(ValueError):
            FD.annotation_u8(bad, k)


P = 64          # a non-NULL, aligned stand-in for device pointers: every call below must fail before anything is launched


def _call(lib, d, n, e=None, m=0, B=None, H=32, order=1, img=P, ann=P, feed=P, tgt=P, pos=P, proc=None):
    return lib.cmpc_train_prep(img if e is not None else None, m, e, ann, n, d, len(d) if B is None else B, H, H, order, proc,
                               feed if e is not None else None, tgt, pos, None)


def test_train_prep_rejects_invalid_arguments():
    lib = L.load()
    shapes = [(40, 30, 3), (20, 20)]
    d, n = FD.plan_targets(shapes, [L.ANN_COLOR, L.ANN_PLAIN], [KEY, (0, 0, 0)], 32, 32)
    e, m = FD.plan_images([(40, 30, 3), (20, 20)], 32, 32)

    def bad(rc, word=b"train_prep"):
        return rc == -1 and word in lib.cmpc_last_error()

    # NULL pointers (proc_im alone may be NULL); images, their descriptors and the feed go together
    assert bad(_call(lib, d, n, ann=None)) and bad(_call(lib, d, n, tgt=None)) and bad(_call(lib, d, n, pos=None))
    assert bad(lib.cmpc_train_prep(None, 0, None, P, n, None, 2, 32, 32, 1, None, None, P, P, None))
    assert bad(_call(lib, d, n, e, m, img=None)) and bad(_call(lib, d, n, e, m, feed=None))
    assert bad(lib.cmpc_train_prep(P, m, None, P, n, d, 2, 32, 32, 1, None, P, P, P, None))
    assert bad(_call(lib, d, n, ann=P + 2), b"aligned")
    # B out of range, unknown order, bad sizes
    assert bad(_call(lib, d, n, B=0)) and bad(_call(lib, d, n, B=-1))
    big = (L.TrainDesc * (L.EVAL_MAX_BATCH + 1))(*([d[0]] * (L.EVAL_MAX_BATCH + 1)))
    assert bad(_call(lib, big, n), b"outside")
    assert bad(_call(lib, d, n, order=2), b"order") and bad(_call(lib, d, n, order=-1), b"order")
    assert bad(_call(lib, d, n, H=0)) and bad(_call(lib, d, 0))
    # per-sample: unknown kind, channel counts, channels to match, a geometry that is not resize_and_pad_geometry's, empty, beyond the buffer
    for i, field, val in ((0, "kind", 2), (0, "kind", -1), (0, "c", 1), (0, "c", 2), (0, "c", 5), (1, "c", 3), (0, "match", 0), (0, "match", 4),
                          (1, "match", 1), (0, "rh", d[0].rh + 1), (0, "rw", d[0].rw - 1), (0, "top", d[0].top + 1), (1, "left", 5),
                          (0, "h", 0), (1, "w", 0), (0, "offset", -16)):
        t = (L.TrainDesc * 2)(d[0], d[1])
        setattr(t[i], field, val)
        assert bad(_call(lib, t, n)), (i, field, val)
    t = (L.TrainDesc * 2)(d[0], d[1])
    t[1].offset = n - 16
    assert bad(_call(lib, t, n), b"beyond") and bad(_call(lib, d, n - 400), b"beyond")
    # the image half keeps eval_prep's checks
    x = (L.EvalDesc * 2)(e[0], e[1])
    x[0].c = 2
    assert bad(_call(lib, d, n, x, m))
    assert bad(_call(lib, d, n, e, m - 400), b"beyond")
    # shrink factor beyond the Gaussian radius limit: the same message as the evaluation entries
    h, w = 32 * 40, 64
    rh, rw, top, left = HU.resize_and_pad_geometry(h, w, 32, 32)
    far = (L.TrainDesc * 1)(L.TrainDesc(0, h, w, 1, rh, rw, top, left, L.ANN_PLAIN, 0, (L.C.c_ubyte * 4)()))
    assert bad(_call(lib, far, h * w), b"Gaussian radius > 63")
    # the existing entry still refuses a NULL proc_im
    assert lib.cmpc_eval_prep(P, m, e, 2, 32, 32, None, P, None) == -1 and b"eval_prep" in lib.cmpc_last_error()


def test_epoch_sampler():
    n = 23
    a, b = FD.EpochSampler(n, seed=5), FD.EpochSampler(n, seed=5)
    sa = [next(a) for _ in range(3 * n + 4)]
    assert sa == [next(b) for _ in range(3 * n + 4)]                        # same seed, same stream
    epochs = [sa[k * n: (k + 1) * n] for k in range(3)]
    for ep in epochs:
        assert sorted(ep) == list(range(n))                                 # each epoch a permutation
    assert epochs[0] != epochs[1] and epochs[1] != epochs[2]
    assert a.epoch == 3
    assert [next(FD.EpochSampler(n, seed=6)) for _ in range(n)] != epochs[0]
    c = FD.EpochSampler(5, shuffle=False)
    assert [next(c) for _ in range(12)] == [0, 1, 2, 3, 4] * 2 + [0, 1]
    # rank shards: disjoint, equal length, inside the range; the union of an epoch's shards misses at most n % world samples
    world = 4
    for epoch in range(3):
        shards = [FD.EpochSampler(n, seed=5, rank=r, world=world).epoch_indices(epoch) for r in range(world)]
        assert all(len(s) == n // world for s in shards)
        allidx = np.concatenate(shards)
        assert len(set(allidx.tolist())) == len(allidx) and set(allidx.tolist()) <= set(range(n))
        assert set(allidx.tolist()) <= set(FD.EpochSampler(n, seed=5).epoch_indices(epoch).tolist())
    r1 = FD.EpochSampler(n, seed=5, rank=1, world=world)
    s1 = [next(r1) for _ in range(2 * (n // world))]
    assert s1[: n // world] == r1.epoch_indices(0).tolist() and s1[n // world:] == r1.epoch_indices(1).tolist()
    for kw in (dict(n=3, world=4), dict(n=8, rank=2, world=2), dict(n=8, rank=-1, world=2), dict(n=8, world=0)):
        with pytest.raises(ValueError):
            FD.EpochSampler(**kw)


VOCAB = {w: i for i, w in enumerate(["<pad>", "<unk>", "a", "red", "dog", "on", "the", "left"])}
SENTS = ["a red dog", "the dog on the left.", "dog", "a purple dog on the left left left left"]


class _Data:
    """Sample i is a function of i: small images, alternating annotation kinds, the three text forms by i % 3; every 4th object is absent."""

    def __init__(self, n, T):
        self.n, self.T = n, T

    def __len__(self):
        return self.n

    def empty(self, i):
        return i % 4 == 2

    def __getitem__(self, i):
        rng = np.random.default_rng(i)
        h, w = int(rng.integers(4, 20)), int(rng.integers(4, 24))
        im = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        m = np.zeros((h, w), bool)
        if not self.empty(i):
            m[i % h, i % w] = True
        sent = SENTS[i % len(SENTS)]
        ids, sl = HU.preprocess_sentence_lstm(sent, VOCAB, self.T)
        text = (sent, (np.array(ids), sl), np.array(HU.preprocess_sentence(sent, VOCAB, self.T)))[i % 3]
        if i % 2:
            return im, m.astype(np.float32), None, text
        ann = np.zeros((h, w, 4), np.uint8)
        ann[m, :3] = KEY
        return im, ann, KEY, text


class _StubStage:
    """The device stage's interface on plain host memory: stage() copies the slot's bytes out, as the copy to the device would."""

    def __init__(self, nslots, cap):
        self.bufs = [np.zeros(cap, np.uint8) for _ in range(nslots)]
        self.staged, self.released, self.closed = [], [], False

    def buffers(self):
        return self.bufs

    def stage(self, hb):
        self.staged.append(hb.slot)
        return {"slot": hb.slot, "hb": hb, "bytes": self.bufs[hb.slot][: hb.nbytes].copy(), "indices": hb.indices, "sentences": hb.sentences,
                "skipped": hb.skipped}

    def release(self, slot):
        self.released.append(slot)

    def copied_done(self, slot):
        return True

    def close(self):
        self.closed = True


def _feeder(n, B, T, HW, depth=2, **kw):
    model = types.SimpleNamespace(batch_size=B, num_steps=T, H=HW, W=HW, video=False, MAX_STEPS_IN_FLIGHT=2)
    stage = _StubStage(depth + 2, FD.slot_capacity(B, T, 20 * 24))
    return FD.TrainFeeder(model, _Data(n, T), vocab=VOCAB, depth=depth, max_hw=(20, 24), _stage=stage, **kw), stage


def _unpack(f, B, T):
    hb, buf = f["hb"], f["bytes"]
    words = buf[: B * T * 4].view(np.int32).reshape(B, T)
    wb = -(-B * T * 4 // 16) * 16
    sl = buf[wb: wb + B * 4].view(np.int32)
    ims = [buf[hb.img_off + d.offset: hb.img_off + d.offset + d.h * d.w * d.c].reshape(d.h, d.w, d.c) for d in hb.img_descs]
    anns = [buf[hb.ann_off + d.offset: hb.ann_off + d.offset + d.h * d.w * d.c].reshape(d.h, d.w, d.c) for d in hb.ann_descs]
    return words, sl, ims, anns


@pytest.mark.parametrize("skip", [False, True])
def test_feeder_host_half(skip):
    n, B, T, HW = 10, 4, 8, 16
    data = _Data(n, T)
    order = [int(i) for e in range(4) for i in FD.EpochSampler(n, seed=2).epoch_indices(e)]
    kept = [i for i in order if not (skip and data.empty(i))]
    fd, stage = _feeder(n, B, T, HW, sampler=FD.EpochSampler(n, seed=2), skip_empty=skip)
    try:
        for s in range(7):                              # 28 samples: batches straddle the epoch boundaries at 10 and 20
            f = next(fd)
            want = kept[s * B: (s + 1) * B]
            assert f["indices"] == want
            words, sl, ims, anns = _unpack(f, B, T)
            for b, i in enumerate(want):
                im, ann, key, text = data[i]
                ids, n_words = HU.preprocess_sentence_lstm(SENTS[i % len(SENTS)], VOCAB, T)
                assert words[b].tolist() == ids and int(sl[b]) == n_words       # the three text forms give the same words / seq_len
                assert f["sentences"][b] == (text if isinstance(text, str) else None)
                assert np.array_equal(ims[b], im)
                d = f["hb"].ann_descs[b]
                if key is None:
                    assert d.kind == L.ANN_PLAIN and d.c == 1 and np.array_equal(anns[b][..., 0], (ann != 0).astype(np.uint8))
                else:
                    assert d.kind == L.ANN_COLOR and d.c == 4 and tuple(d.key)[:3] == KEY and np.array_equal(anns[b], ann)
                assert (d.rh, d.rw, d.top, d.left) == HU.resize_and_pad_geometry(im.shape[0], im.shape[1], HW, HW)
            # skipped: the empties dropped in the stream up to this batch's last sample
            seen, upto = 0, 0
            for p, i in enumerate(order):
                seen += not (skip and data.empty(i))
                if seen == (s + 1) * B:
                    upto = p + 1
                    break
            assert fd.skipped == (sum(data.empty(i) for i in order[:upto]) if skip else 0)
        assert len(stage.released) == 6 and len(set(stage.staged[:4])) == 4     # a feed is released when the next one is requested
        assert fd.peek()["indices"] == kept[7 * B: 8 * B]
    finally:
        fd.close()
    assert stage.closed and not fd.pipe._thread.is_alive()


def test_feeder_surfaces_worker_errors_and_refuses_bad_setups():
    class Bad(_Data):
        def __getitem__(self, i):
            im, ann, key, text = super().__getitem__(i)
            return (im[:-1] if i == 3 else im), ann, key, text

    model = types.SimpleNamespace(batch_size=2, num_steps=8, H=16, W=16, video=False, MAX_STEPS_IN_FLIGHT=2)
    stage = _StubStage(4, FD.slot_capacity(2, 8, 20 * 24))
    fd = FD.TrainFeeder(model, Bad(6, 8), sampler=FD.EpochSampler(6, shuffle=False), vocab=VOCAB, max_hw=(20, 24), _stage=stage)
    try:
        assert next(fd)["indices"] == [0, 1]
        with pytest.raises(ValueError, match="sample 3"):
            next(fd)
    finally:
        fd.close()
    # a sample larger than the ring's slots
    stage = _StubStage(4, FD.slot_capacity(2, 8, 4 * 4))
    fd = FD.TrainFeeder(model, _Data(6, 8), vocab=VOCAB, max_hw=(4, 4), _stage=stage)
    try:
        with pytest.raises(ValueError, match="max_hw"):
            next(fd)
    finally:
        fd.close()
    with pytest.raises(ValueError):
        FD.TrainFeeder(types.SimpleNamespace(video=True), _Data(6, 8), vocab=VOCAB)
    with pytest.raises(ValueError):
        FD.TrainFeeder(model, _Data(6, 8), vocab=VOCAB, order=3, _stage=stage)
    with pytest.raises(ValueError):
        FD.TrainFeeder(model, _Data(6, 8), vocab=VOCAB, depth=0, _stage=stage)
    with pytest.raises(ValueError):
        FD.TrainFeeder(model, _Data(6, 8), vocab=VOCAB, workers=8, _stage=stage)
    with pytest.raises(ValueError):
        FD.encode_text("a dog", None, 8)
    with pytest.raises(ValueError):
        FD.encode_text(" . ", VOCAB, 8)
    assert FD.WORKERS + 1 <= 4
