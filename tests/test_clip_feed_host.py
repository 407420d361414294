"""CPU tests of the clip feed's host half (cmpc-refseg_amd/feed.py: ClipPipeline, ClipTrainFeeder with a stub in place of the device
stage): which frames are indexed, the packed bytes and descriptors, sampler order, skip_empty accounting, slot recycling, every refusal,
and cmpc_clip_prep's argument checks before anything is launched (the library loads without a GPU)."""
import importlib
import types

import numpy as np
import pytest

HU = importlib.import_module("cmpc-refseg_amd.hostutil")
FD = importlib.import_module("cmpc-refseg_amd.feed")
L = importlib.import_module("cmpc-refseg_amd._lib")

KEY = FD.REFVOS_OBJECT_COLOR["2"]
FRAME_IDX = (0, 4, 8, 12, 15)
FRAMES = 16
VOCAB = {w: i for i, w in enumerate(["<pad>", "<unk>", "a", "red", "dog", "on", "the", "left"])}
SENTS = ["a red dog", "the dog on the left.", "dog", "a purple dog on the left left left left"]


class _Lazy:
    """A clip as a lazy sequence: frame j is made when it is indexed, and every index is recorded."""

    def __init__(self, seed, n, h, w, gray, log):
        self.seed, self.n, self.h, self.w, self.gray, self.log = seed, n, h, w, gray, log

    def __len__(self):
        return self.n

    def __getitem__(self, j):
        self.log.append((self.seed, j))
        rng = np.random.default_rng([self.seed, j])
        return rng.integers(0, 256, (self.h, self.w) if self.gray else (self.h, self.w, 3), dtype=np.uint8)


class _Clips:
    """Clip i is a function of i: small frames (grey every 5th clip), alternating annotation kinds, the three text forms by i % 3, a lazy
    sequence or an array by i % 2; every 4th object is absent."""

    def __init__(self, n, T):
        self.n, self.T, self.log = n, T, []

    def __len__(self):
        return self.n

    def empty(self, i):
        return i % 4 == 2

    def size(self, i):
        rng = np.random.default_rng(i)
        return int(rng.integers(4, 20)), int(rng.integers(4, 24))

    def frames(self, i, log=None):
        h, w = self.size(i)
        return _Lazy(i, FRAMES, h, w, i % 5 == 4, self.log if log is None else log)

    def __getitem__(self, i):
        h, w = self.size(i)
        fr = self.frames(i)
        if i % 2 and i % 5 != 4:
            fr = np.stack([self.frames(i, [])[j] for j in range(FRAMES)])      # an array [frames, h, w, 3]
        m = np.zeros((h, w), bool)
        if not self.empty(i):
            m[i % h, i % w] = True
        sent = SENTS[i % len(SENTS)]
        ids, sl = HU.preprocess_sentence_lstm(sent, VOCAB, self.T)
        text = (sent, (np.array(ids), sl), np.array(HU.preprocess_sentence(sent, VOCAB, self.T)))[i % 3]
        if i % 2:
            return fr, m, None, text                                           # a plain bool mask
        ann = np.zeros((h, w, 3), np.uint8)
        ann[m] = KEY
        return fr, ann, KEY, text


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


def _model(T, HW, **kw):
    d = dict(batch_size=1, num_steps=T, H=HW, W=HW, video=True, frames=FRAMES, FRAME_IDX=FRAME_IDX, MAX_STEPS_IN_FLIGHT=2)
    d.update(kw)
    return types.SimpleNamespace(**d)


def _feeder(data, T, HW, depth=2, max_hw=(20, 24), **kw):
    stage = _StubStage(depth + 2, FD.clip_slot_capacity(T, len(FRAME_IDX), max_hw[0] * max_hw[1]))
    return FD.ClipTrainFeeder(_model(T, HW), data, vocab=VOCAB, depth=depth, max_hw=max_hw, _stage=stage, **kw), stage


def _unpack(f, T):
    hb, buf = f["hb"], f["bytes"]
    words = buf[: T * 4].view(np.int32)
    wb = -(-T * 4 // 16) * 16
    sl = int(buf[wb: wb + 4].view(np.int32)[0])
    ims = [buf[hb.img_off + d.offset: hb.img_off + d.offset + d.h * d.w * d.c].reshape(d.h, d.w, d.c) for d in hb.img_descs]
    d = hb.ann_descs[0]
    ann = buf[hb.ann_off + d.offset: hb.ann_off + d.offset + d.h * d.w * d.c].reshape(d.h, d.w, d.c)
    return words, sl, ims, ann


@pytest.mark.timeout(60)
def test_slot_capacity():
    assert FD.clip_slot_capacity(20, 5, 480 * 640) == 80 + 16 + 5 * 480 * 640 * 3 + 480 * 640 * 4
    assert FD.clip_slot_capacity(6, 5, 3 * 3) == 32 + 16 + 5 * 32 + 48          # every part rounded up to 16 bytes


@pytest.mark.timeout(60)
@pytest.mark.parametrize("skip", [False, True])
def test_clip_feeder_host_half(skip):
    n, T, HW = 10, 8, 16
    data = _Clips(n, T)
    order = [int(i) for e in range(3) for i in FD.EpochSampler(n, seed=2).epoch_indices(e)]
    kept = [i for i in order if not (skip and data.empty(i))]
    fd, stage = _feeder(data, T, HW, sampler=FD.EpochSampler(n, seed=2), skip_empty=skip)
    try:
        for s in range(13):                             # past the epoch boundary at 10; 3 times round the 4-slot ring
            f = next(fd)
            i = kept[s]
            assert f["indices"] == [i]                  # sampler order
            words, sl, ims, ann = _unpack(f, T)
            frames, annotation, key, text = data[i]
            ids, n_words = HU.preprocess_sentence_lstm(SENTS[i % len(SENTS)], VOCAB, T)
            assert words.tolist() == ids and sl == n_words                     # the three text forms give the same words / seq_len
            assert f["sentences"] == [text if isinstance(text, str) else None]
            # packing: the five sampled frames in FRAME_IDX order at 16-byte aligned offsets behind words and seq_len, then the annotation
            hb = f["hb"]
            assert hb.img_off == 32 + 16 and len(hb.img_descs) == len(FRAME_IDX) and len(hb.ann_descs) == 1
            h, w = data.size(i)
            c = 1 if i % 5 == 4 else 3
            off = 0
            for k, (j, d) in enumerate(zip(FRAME_IDX, hb.img_descs)):
                want = data.frames(i, [])[j]
                assert (d.h, d.w, d.c) == (h, w, c) and d.offset == off and off % 16 == 0
                assert (d.rh, d.rw, d.top, d.left) == HU.resize_and_pad_geometry(h, w, HW, HW)
                assert np.array_equal(ims[k].reshape(want.shape), want), (i, j)
                off += -(-h * w * c // 16) * 16
            assert hb.img_bytes == off and hb.ann_off == hb.img_off + off
            d = hb.ann_descs[0]
            assert d.offset == 0 and (d.h, d.w) == (h, w) and (d.rh, d.rw, d.top, d.left) == HU.resize_and_pad_geometry(h, w, HW, HW)
            assert hb.nbytes == hb.ann_off + hb.ann_bytes and hb.ann_bytes == -(-h * w * d.c // 16) * 16
            if key is None:
                assert d.kind == L.ANN_PLAIN and d.c == 1 and d.match == 0 and np.array_equal(ann[..., 0], annotation.astype(np.uint8))
            else:
                assert d.kind == L.ANN_COLOR and d.c == 3 and d.match == 1 and tuple(d.key)[:3] == KEY and np.array_equal(ann, annotation)
            # skipped: the empties dropped in the stream up to this clip
            upto = [p for p, q in enumerate(order) if q == i and sum(not (skip and data.empty(r)) for r in order[:p + 1]) == s + 1][0] + 1
            assert fd.skipped == (sum(data.empty(r) for r in order[:upto]) if skip else 0)
        # slot recycling: a feed is released when the next one is requested, and the ring is reused in the order it was released
        assert stage.released == stage.staged[:12] and len(set(stage.staged[:4])) == 4
        assert fd.peek()["indices"] == [kept[13]]
    finally:
        fd.close()
    assert stage.closed and not fd.pipe._thread.is_alive()
    # only the sampled positions of a lazy clip were ever indexed: 5 frames decoded, not 16
    assert data.log and {j for _, j in data.log} == set(FRAME_IDX)
    per_clip = {}
    for seed, j in data.log:
        per_clip.setdefault(seed, []).append(j)
    assert all(len(v) % len(FRAME_IDX) == 0 for v in per_clip.values())


@pytest.mark.timeout(60)
def test_clip_feeder_surfaces_worker_errors_when_the_clip_is_due():
    class Boom(_Clips):
        def __getitem__(self, i):
            if i == 3:
                raise KeyError("clip 3 is unreadable")
            return super().__getitem__(i)

    fd, stage = _feeder(Boom(6, 8), 8, 16, sampler=FD.EpochSampler(6, shuffle=False))
    try:
        assert [next(fd)["indices"] for _ in range(3)] == [[0], [1], [2]]      # the clips before it are handed out first
        with pytest.raises(KeyError, match="clip 3"):
            next(fd)
        with pytest.raises(KeyError):                                          # and it stays raised
            next(fd)
    finally:
        fd.close()


def _one(frames, ann, key=None, text="a dog"):
    return [(frames, ann, key, text)] * 4


@pytest.mark.timeout(60)
def test_clip_feeder_refusals():
    T, HW = 8, 16
    rng = np.random.default_rng(0)
    good = rng.integers(0, 256, (FRAMES, 6, 7, 3), dtype=np.uint8)
    uneven = [good[j] if j != 12 else good[j][:-1] for j in range(FRAMES)]
    cases = [
        (_one(uneven, np.ones((6, 7), bool)), "sample [0-3]: frame 12"),                        # frames of unequal size
        (_one(good, np.ones((6, 8), bool)), "sample [0-3]: frames .* annotation"),              # an annotation of another size
        (_one(good[:12], np.ones((6, 7), bool)), "sample [0-3]: 12 frames"),                    # not the model's clip length
        (_one(good.astype(np.float32), np.ones((6, 7), bool)), "sample [0-3]: .*uint8"),        # frames must be uint8
        (_one(good, np.ones((6, 7, 3), np.uint8), None), "annotation [0-3]"),                   # a colour-coded annotation needs its key
        (_one(good, np.ones((6, 7), bool), None, " . "), "no word"),
    ]
    for data, pattern in cases:
        fd, _ = _feeder(data, T, HW, sampler=FD.EpochSampler(4, shuffle=False))
        try:
            with pytest.raises(ValueError, match=pattern):
                next(fd)
        finally:
            fd.close()
    # a clip larger than the ring's slots
    fd, _ = _feeder(_one(good, np.ones((6, 7), bool)), T, HW, max_hw=(4, 4))
    try:
        with pytest.raises(ValueError, match="max_hw"):
            next(fd)
    finally:
        fd.close()
    # set-up: an image model, and TrainFeeder's own refusals
    stage = _StubStage(4, FD.clip_slot_capacity(T, 5, 20 * 24))
    data = _one(good, np.ones((6, 7), bool))
    with pytest.raises(ValueError, match="video model"):
        FD.ClipTrainFeeder(_model(T, HW, video=False), data, vocab=VOCAB, _stage=stage)
    with pytest.raises(ValueError, match="ClipTrainFeeder"):
        FD.TrainFeeder(_model(T, HW), data, vocab=VOCAB)                       # and TrainFeeder still refuses the video model
    for kw in (dict(order=3), dict(depth=0), dict(workers=8), dict(match=0)):
        with pytest.raises(ValueError):
            fd = FD.ClipTrainFeeder(_model(T, HW), data, vocab=VOCAB, _stage=stage, **kw)
            try:
                next(fd)                                                       # match is checked when the first clip is planned
            finally:
                fd.close()
    small = _StubStage(4, 64)
    with pytest.raises(ValueError, match="slot buffer"):
        FD.ClipTrainFeeder(_model(T, HW), data, vocab=VOCAB, max_hw=(20, 24), _stage=small)
    with pytest.raises(TypeError):
        FD.ClipTrainFeeder(_model(T, HW), data, vocab=VOCAB, _stage=stage, lookahead=True)     # the video step has no next_im


P = 64          # a non-NULL, aligned stand-in for device pointers: every call below must fail before anything is launched


@pytest.mark.timeout(60)
def test_clip_prep_rejects_invalid_arguments():
    lib = L.load()
    e, m = FD.plan_images([(40, 30, 3)] * 5, 32, 32)
    d, n = FD.plan_targets([(40, 30, 3)], [L.ANN_COLOR], [KEY], 32, 32)

    def call(img=P, m=m, e=e, n_img=5, ann=P, n=n, d=d, H=32, W=32, order=1, feed=P, tgt=P, pos=P):
        return lib.cmpc_clip_prep(img, m, e, n_img, ann, n, d, H, W, order, feed, tgt, pos, None)

    def bad(rc, word=b"clip_prep"):
        return rc == -1 and word in lib.cmpc_last_error()

    for kw in (dict(img=None), dict(e=None), dict(ann=None), dict(d=None), dict(feed=None), dict(tgt=None), dict(pos=None)):
        assert bad(call(**kw), b"NULL"), kw
    big = (L.EvalDesc * 9)(*([e[0]] * 9))
    assert bad(call(n_img=0), b"outside") and bad(call(n_img=-1), b"outside") and bad(call(e=big, n_img=L.TAPS_MAX_FRAMES + 1), b"outside")
    assert bad(call(H=0)) and bad(call(W=-1)) and bad(call(m=0)) and bad(call(n=0))
    assert bad(call(order=2), b"order") and bad(call(ann=P + 2), b"aligned")
    # the annotation's descriptor gets cmpc_train_prep's checks
    for field, val in (("kind", 2), ("c", 1), ("c", 5), ("match", 0), ("match", 4), ("rh", d[0].rh + 1), ("left", d[0].left + 1), ("h", 0),
                       ("offset", -16)):
        t = (L.TrainDesc * 1)(d[0])
        setattr(t[0], field, val)
        assert bad(call(d=t)), (field, val)
    assert bad(call(n=n - 400), b"beyond")
    # the frames' descriptors get cmpc_eval_prep's
    for i, field, val in ((0, "c", 2), (4, "c", 4), (2, "rw", e[2].rw + 1), (1, "top", 1), (3, "w", 0), (4, "offset", -16)):
        x = (L.EvalDesc * 5)(*e)
        setattr(x[i], field, val)
        assert bad(call(e=x)), (i, field, val)
    assert bad(call(m=m - 400), b"beyond")
    h, w = 32 * 40, 64
    rh, rw, top, left = HU.resize_and_pad_geometry(h, w, 32, 32)
    far = (L.EvalDesc * 1)(L.EvalDesc(0, h, w, 3, rh, rw, top, left, 0))
    assert bad(call(e=far, n_img=1, m=h * w * 3), b"Gaussian radius > 63")
