"""Training feed from raw samples: the reference reader's per-sample work (util/data_reader_refvos.py:27-72, build_batches.py:62-75)
with the resampling on the GPU and the host work off the train step's critical path.

    feed, target_fine, pos = prepare_batch(images, annotations, keys, H, W)      # one cmpc_train_prep call, current stream
    target_fine, pos = prepare_targets(annotations, keys, H, W)                   # the mask half alone
    frames, target_fine, pos = prepare_clip(frames5, annotation, key, H, W)       # one clip of the video model: one cmpc_clip_prep call

    feeder = TrainFeeder(model, samples, vocab=vocab)        # samples[i] -> (image, annotation, key_or_None, text)
    for _ in range(iters):
        step, scalars = feeder.step()                        # model.train_step on the staged batch (lookahead=True: next batch as next_im)

    feeder = ClipTrainFeeder(video_model, clips, vocab=vocab)   # clips[i] -> (frames, annotation, key_or_None, text)
    step, scalars = feeder.step(accuracy=True)                  # model.train_step_video_frames on the staged clip (one cmpc_clip_prep call)

A sample is an original-size uint8 image ([h, w, 3] or [h, w]), an annotation at the same size -- colour-coded uint8 [h, w, 3|4] with
a key colour (REFVOS_OBJECT_COLOR), or with key None a plain mask [h, w], non-zero = object -- and a sentence.  Decoding files is the
caller's business: samples are arrays.

Threads: a small pool loads samples (samples[i], tokenising), one packer thread assembles batches in sampler order and copies their
bytes into pinned host buffers.  Only the caller's thread touches the GPU: it issues one host-to-device copy and one cmpc_train_prep
call per batch on the feeder's side stream and records the batch's `ready` event.  The ring of pinned and device buffers is allocated
once; a slot is reused only behind the event recorded after the step that read it, so nothing is allocated and nothing synchronises
in the steady state.
"""
from __future__ import annotations

import queue
import threading
from collections import deque
from concurrent.futures import ThreadPoolExecutor
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import _lib, hostutil as HU

MAX_BATCH = _lib.EVAL_MAX_BATCH
_ALIGN = 16
WORKERS = 2                       # sample-loading threads (plus the packer thread); a small constant, never the machine's CPU count

# the key colours of the Refer-YouTube-VOS annotations by object id (util/data_reader_refvos.py:14-21), R, G, B
REFVOS_OBJECT_COLOR = {
    "1": (236, 95, 103),
    "2": (249, 145, 87),
    "3": (250, 200, 99),
    "4": (153, 199, 148),
    "5": (98, 179, 178),
    "6": (102, 153, 204),
}


def _align(n: int) -> int:
    return -(-n // _ALIGN) * _ALIGN


def _images_u8(images) -> List[np.ndarray]:
    out = []
    for i, im in enumerate(images):
        a = np.asarray(im)
        if a.dtype != np.uint8:
            raise ValueError("image %d: expected uint8, got %s" % (i, a.dtype))
        if a.ndim not in (2, 3) or (a.ndim == 3 and a.shape[2] not in (1, 3)) or a.shape[0] == 0 or a.shape[1] == 0:
            raise ValueError("image %d: expected [h, w] or [h, w, 1|3] with h, w > 0, got %s" % (i, a.shape))
        out.append(np.ascontiguousarray(a))
    return out


def annotation_u8(annotation, key, i: int = 0) -> Tuple[np.ndarray, int, Tuple[int, int, int]]:
    """One annotation as the bytes cmpc_train_prep reads: (contiguous uint8 [h, w, c], kind, key colour).  key None: a plain mask of any
    dtype, non-zero = object, as bytes [h, w] (evaluate._masks_u8's conversion); else the colour-coded uint8 [h, w, 3|4] as it is."""
    a = np.asarray(annotation)
    if key is None:
        if a.ndim == 3 and a.shape[2] == 1:
            a = a[:, :, 0]
        if a.ndim != 2 or a.shape[0] == 0 or a.shape[1] == 0:
            raise ValueError("annotation %d: a plain mask must be [h, w] with h, w > 0, got %s" % (i, a.shape))
        return np.ascontiguousarray(a != 0).view(np.uint8), _lib.ANN_PLAIN, (0, 0, 0)
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] not in (3, 4) or a.shape[0] == 0 or a.shape[1] == 0:
        raise ValueError("annotation %d: a colour-coded annotation must be uint8 [h, w, 3|4] with h, w > 0, got %s %s" % (i, a.dtype, a.shape))
    k = [int(v) for v in np.asarray(key).reshape(-1)[:3]]
    if len(k) != 3 or min(k) < 0 or max(k) > 255:
        raise ValueError("annotation %d: the key colour must hold R, G, B in 0..255, got %r" % (i, key))
    return np.ascontiguousarray(a), _lib.ANN_COLOR, (k[0], k[1], k[2])


def _check_batch(n: int):
    if n <= 0 or n > MAX_BATCH:
        raise ValueError("batch of %d samples: expected 1..%d per call (split larger batches)" % (n, MAX_BATCH))


def plan_images(shapes: Sequence[Tuple[int, ...]], H: int, W: int):
    """evaluate.plan_prep: descriptors (cmpc_eval_desc[B]) and packed length of images of the given shapes."""
    _check_batch(len(shapes))
    d = (_lib.EvalDesc * len(shapes))()
    off = 0
    for i, s in enumerate(shapes):
        h, w = int(s[0]), int(s[1])
        c = int(s[2]) if len(s) == 3 else 1
        rh, rw, top, left = HU.resize_and_pad_geometry(h, w, H, W)
        d[i] = _lib.EvalDesc(off, h, w, c, rh, rw, top, left, 0)
        off += _align(h * w * c)
    return d, off


def plan_targets(shapes: Sequence[Tuple[int, ...]], kinds: Sequence[int], keys: Sequence[Tuple[int, int, int]], H: int, W: int, match: int = 1):
    """Descriptors (cmpc_train_desc[B]) and packed length of annotations of the given shapes ([h, w] or [h, w, c]) for cmpc_train_prep:
    16-byte aligned offsets, resize_and_pad_geometry(h, w, H, W); `match` leading channels of a colour-coded annotation must equal its key."""
    _check_batch(len(shapes))
    if match not in (1, 2, 3):
        raise ValueError("match must be 1 (the reference's rule: channel 0 alone), 2 or 3, got %r" % (match,))
    d = (_lib.TrainDesc * len(shapes))()
    off = 0
    for i, (s, kind, key) in enumerate(zip(shapes, kinds, keys)):
        h, w = int(s[0]), int(s[1])
        c = int(s[2]) if len(s) == 3 else 1
        rh, rw, top, left = HU.resize_and_pad_geometry(h, w, H, W)
        d[i] = _lib.TrainDesc(off, h, w, c, rh, rw, top, left, kind, match if kind == _lib.ANN_COLOR else 0,
                              (_lib.C.c_ubyte * 4)(key[0], key[1], key[2], 0))
        off += _align(h * w * c)
    return d, off


def _check_order(order):
    if order not in (0, 1):
        raise ValueError("order must be 0 (nearest sample, a bool image's default) or 1 (hostutil.resize_and_pad), got %r" % (order,))


def _keys(keys, n):
    if keys is None:
        return [None] * n
    keys = list(keys)
    if len(keys) != n:
        raise ValueError("%d keys for %d annotations" % (len(keys), n))
    return keys


def _prep(images, annotations, keys, H, W, order, match, device):
    import torch
    from .evaluate import _staging
    _check_order(order)
    anns = [annotation_u8(a, k, i) for i, (a, k) in enumerate(zip(annotations, _keys(keys, len(annotations))))]
    B = len(anns)
    adesc, abytes = plan_targets([a[0].shape for a in anns], [a[1] for a in anns], [a[2] for a in anns], H, W, match)
    dev = torch.device(device)
    with torch.cuda.device(dev):
        st = torch.cuda.current_stream(dev).cuda_stream
        feed = isrc = idesc = None
        ibytes = 0
        if images is not None:
            ims = _images_u8(images)
            if len(ims) != B:
                raise ValueError("%d images for %d annotations" % (len(ims), B))
            for i, (im, a) in enumerate(zip(ims, anns)):
                if im.shape[:2] != a[0].shape[:2]:
                    raise ValueError("sample %d: image %s, annotation %s (the annotation is at the image's size)" % (i, im.shape[:2], a[0].shape[:2]))
            idesc, ibytes = plan_images([a.shape for a in ims], H, W)
            isrc = _staging(dev, "im").upload(ims, idesc, ibytes)
            feed = torch.empty(B, H, W, 3, dtype=torch.float32, device=dev)
        asrc = _staging(dev, "ann").upload([a[0] for a in anns], adesc, abytes)
        target = torch.empty(B, H, W, 1, dtype=torch.float32, device=dev)
        pos = torch.empty(B, dtype=torch.int64, device=dev)
        _lib.call("cmpc_train_prep", isrc.data_ptr() if isrc is not None else None, ibytes, idesc, asrc.data_ptr(), abytes, adesc, B, H, W,
                  order, None, feed.data_ptr() if feed is not None else None, target.data_ptr(), pos.data_ptr(), st)
    return feed, target, pos


def prepare_targets(annotations, keys, H: int, W: int, order: int = 1, match: int = 1, device="cuda:0"):
    """(target_fine float32 [B, H, W, 1] in {0, 1}, pos int64 [B]) of original-size annotations on the device: the object cut out of each
    annotation (hostutil.object_mask), resize_and_pad(.) > 0, and the count of foreground pixels.  keys: one key colour or None (plain
    mask) per annotation, or None for all.  Enqueued on the current stream; nothing synchronises."""
    _, target, pos = _prep(None, list(annotations), keys, H, W, order, match, device)
    return target, pos


def prepare_batch(images, annotations, keys, H: int, W: int, order: int = 1, match: int = 1, device="cuda:0"):
    """(im float32 [B, H, W, 3], target_fine, pos): evaluate.prepare_images' feed of the images and prepare_targets of the annotations
    from one cmpc_train_prep call -- hostutil.train_sample per sample, on the device."""
    return _prep(list(images), list(annotations), keys, H, W, order, match, device)


def prepare_clip(frames, annotation, key, H: int, W: int, order: int = 1, match: int = 1, device="cuda:0"):
    """(frames float32 [n, H, W, 3], target_fine float32 [1, H, W, 1], pos int64 [1]) of one clip of the video model from one
    cmpc_clip_prep call on the current stream: evaluate.prepare_images' feed of the n (<= 8) sampled frames -- original-size uint8, all
    one size -- and prepare_targets of the key frame's annotation, bit for bit.  Nothing synchronises."""
    import torch
    from .evaluate import _staging
    _check_order(order)
    ims = _images_u8(list(frames))
    if not 1 <= len(ims) <= _lib.TAPS_MAX_FRAMES:
        raise ValueError("%d frames: expected 1..%d (the clip's sampled frames)" % (len(ims), _lib.TAPS_MAX_FRAMES))
    ann, kind, k = annotation_u8(annotation, key)
    for i, im in enumerate(ims):
        if im.shape != ims[0].shape or im.shape[:2] != ann.shape[:2]:
            raise ValueError("frame %d is %s, frame 0 %s, the annotation %s (one size for all)" % (i, im.shape, ims[0].shape, ann.shape[:2]))
    idesc, ibytes = plan_images([a.shape for a in ims], H, W)
    adesc, abytes = plan_targets([ann.shape], [kind], [k], H, W, match)
    dev = torch.device(device)
    with torch.cuda.device(dev):
        isrc = _staging(dev, "im").upload(ims, idesc, ibytes)
        asrc = _staging(dev, "ann").upload([ann], adesc, abytes)
        feed = torch.empty(len(ims), H, W, 3, dtype=torch.float32, device=dev)
        target = torch.empty(1, H, W, 1, dtype=torch.float32, device=dev)
        pos = torch.empty(1, dtype=torch.int64, device=dev)
        _lib.call("cmpc_clip_prep", isrc.data_ptr(), ibytes, idesc, len(ims), asrc.data_ptr(), abytes, adesc, H, W, order,
                  feed.data_ptr(), target.data_ptr(), pos.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
    return feed, target, pos


class EpochSampler:
    """An endless stream of sample indices like run_prefetch's (data_reader_refvos.py:48-72): a fresh permutation every epoch, seeded
    (default_rng([seed, epoch])) so that a run can be repeated.  With world > 1 every rank takes perm[rank::world] cut to n // world
    entries: equal shards keep the ranks' epochs (and reshuffles) on the same step, and no rank ever runs out of batches for the
    gradient all-reduce."""

    def __init__(self, n: int, shuffle: bool = True, seed: int = 0, rank: int = 0, world: int = 1):
        if world < 1 or not 0 <= rank < world:
            raise ValueError("rank %d outside 0..%d" % (rank, world - 1))
        if n // world < 1:
            raise ValueError("%d samples for %d ranks: every rank needs at least one" % (n, world))
        self.n, self.shuffle, self.seed, self.rank, self.world = int(n), bool(shuffle), int(seed), int(rank), int(world)
        self.per_epoch = self.n // self.world
        self.epoch = 0
        self._order = self.epoch_indices(0)
        self._k = 0

    def epoch_indices(self, epoch: int) -> np.ndarray:
        perm = np.random.default_rng([self.seed, epoch]).permutation(self.n) if self.shuffle else np.arange(self.n)
        return perm[self.rank::self.world][: self.per_epoch]

    def __iter__(self):
        return self

    def __next__(self) -> int:
        if self._k == self.per_epoch:
            self.epoch += 1
            self._order = self.epoch_indices(self.epoch)
            self._k = 0
        i = int(self._order[self._k])
        self._k += 1
        return i


def encode_text(text, vocab, T: int) -> Tuple[np.ndarray, int]:
    """(END-padded int32 ids [T], seq_len) of one sample's text: a sentence (tokenised with hostutil.preprocess_sentence_lstm and
    `vocab`), an (ids, seq_len) pair already in that form, or a FRONT-padded id row as the .npz batches hold (hostutil.end_padded)."""
    if isinstance(text, str):
        if vocab is None:
            raise ValueError("a sentence needs the vocabulary (TrainFeeder(vocab=...))")
        ids, n = HU.preprocess_sentence_lstm(text, vocab, T)
        if n == 0:
            raise ValueError("sentence %r holds no word (the text LSTM needs seq_len >= 1)" % (text,))
        return np.asarray(ids, dtype=np.int32), n
    if isinstance(text, tuple) and len(text) == 2:
        ids, n = np.asarray(text[0]).reshape(-1), int(text[1])
        if ids.shape[0] != T or not np.issubdtype(ids.dtype, np.integer) or not 1 <= n <= T:
            raise ValueError("(ids, seq_len): expected integer ids [%d] and 1 <= seq_len <= %d, got %s %s, %d" % (T, T, ids.dtype, ids.shape, n))
        return ids.astype(np.int32), n
    row = np.asarray(text)
    if row.ndim != 1 or row.shape[0] != T:
        raise ValueError("front-padded ids: expected [%d], got %s" % (T, row.shape))
    ids, n = HU.end_padded(row)
    return ids, int(n)


class _Sample:
    __slots__ = ("index", "image", "ann", "kind", "key", "ids", "seq_len", "text", "empty")


class HostBatch:
    """One batch as the packer leaves it in a slot's host buffer: words ‖ seq_len ‖ images ‖ annotations, with the descriptors."""
    __slots__ = ("slot", "nbytes", "img_off", "img_bytes", "img_descs", "ann_off", "ann_bytes", "ann_descs", "indices", "sentences", "skipped")


class HostPipeline:
    """The feed's host half: sampler -> loader pool -> packer thread -> filled host buffers, in sampler order.  It never touches the GPU:
    `buffers` are uint8 NumPy views (of pinned memory when TrainFeeder builds them).  free(slot) hands a buffer back for refilling;
    get() returns the next HostBatch (blocking), re-raising whatever a worker raised."""

    def __init__(self, samples, sampler, vocab, B, T, H, W, buffers: List[np.ndarray], max_pixels: int, skip_empty=False, match=1, workers=WORKERS):
        if not 1 <= workers <= 3:
            raise ValueError("workers must be 1..3 (plus the packer thread: at most 4 threads), got %d" % workers)
        _check_batch(B)
        self.samples, self.sampler, self.vocab = samples, sampler, vocab
        self.B, self.T, self.H, self.W, self.match = B, T, H, W, match
        self.buffers, self.max_pixels, self.skip_empty = buffers, int(max_pixels), bool(skip_empty)
        self.words_bytes = _align(B * T * 4)
        self.img_off = self.words_bytes + _align(B * 4)
        self.capacity = self._capacity()
        for b in buffers:
            if b.dtype != np.uint8 or b.ndim != 1 or b.shape[0] < self.capacity:
                raise ValueError("a slot buffer must be uint8 [>= %d]" % self.capacity)
        self.skipped = 0
        self._free: "queue.Queue[int]" = queue.Queue()
        self._ready: "queue.Queue" = queue.Queue()
        for k in range(len(buffers)):
            self._free.put(k)
        self._stop = threading.Event()
        self._pool = ThreadPoolExecutor(max_workers=workers, thread_name_prefix="cmpc-feed-load")
        self._window = 2 * B                         # samples loading ahead of the packer
        self._thread = threading.Thread(target=self._run, name="cmpc-feed-pack", daemon=True)
        self._thread.start()

    def _capacity(self) -> int:
        return slot_capacity(self.B, self.T, self.max_pixels)

    # -- loader pool ------------------------------------------------------------------------------------------------------------------
    def _load(self, index: int) -> _Sample:
        image, annotation, key, text = self.samples[index]
        s = _Sample()
        s.index = index
        s.image = _images_u8([image])[0]
        s.ann, s.kind, s.key = annotation_u8(annotation, key, index)
        if s.image.shape[:2] != s.ann.shape[:2]:
            raise ValueError("sample %d: image %s, annotation %s (the annotation is at the image's size)" % (index, s.image.shape[:2], s.ann.shape[:2]))
        if s.image.shape[0] * s.image.shape[1] > self.max_pixels:
            raise ValueError("sample %d: %d x %d pixels exceed the ring's slots (TrainFeeder(max_hw=...) sizes them)" % (index, s.image.shape[0], s.image.shape[1]))
        s.ids, s.seq_len = encode_text(text, self.vocab, self.T)
        s.text = text if isinstance(text, str) else None
        s.empty = self.skip_empty and not HU.object_mask(annotation, key, self.match).any()
        return s

    # -- packer thread ----------------------------------------------------------------------------------------------------------------
    def _take_slot(self) -> Optional[int]:
        while not self._stop.is_set():
            try:
                return self._free.get(timeout=0.05)
            except queue.Empty:
                pass
        return None

    def _run(self):
        try:
            pending = deque()
            it = iter(self.sampler)
            while not self._stop.is_set():
                batch: List[_Sample] = []
                while len(batch) < self.B and not self._stop.is_set():
                    while len(pending) < self._window:
                        pending.append(self._pool.submit(self._load, next(it)))
                    s = pending.popleft().result()
                    if s.empty:                      # build_batches.py:173-175 drops samples whose object is absent
                        self.skipped += 1
                        continue
                    batch.append(s)
                slot = self._take_slot()
                if slot is None:
                    break
                hb = self._pack(slot, batch)
                hb.skipped = self.skipped            # samples dropped in the stream up to this batch's last sample
                self._ready.put(hb)
        except BaseException as e:                   # surfaces in the caller's thread at the next get()
            self._ready.put(e)

    def _pack(self, slot: int, batch: List[_Sample]) -> HostBatch:
        B, T = self.B, self.T
        buf = self.buffers[slot]
        hb = HostBatch()
        hb.slot = slot
        buf[: B * T * 4].view(np.int32).reshape(B, T)[...] = np.stack([s.ids for s in batch])
        buf[self.words_bytes: self.words_bytes + B * 4].view(np.int32)[...] = [s.seq_len for s in batch]
        hb.img_descs, hb.img_bytes = plan_images([s.image.shape for s in batch], self.H, self.W)
        hb.ann_descs, hb.ann_bytes = plan_targets([s.ann.shape for s in batch], [s.kind for s in batch], [s.key for s in batch], self.H, self.W, self.match)
        hb.img_off, hb.ann_off = self.img_off, self.img_off + hb.img_bytes
        hb.nbytes = hb.ann_off + hb.ann_bytes
        for s, di, da in zip(batch, hb.img_descs, hb.ann_descs):
            o = hb.img_off + di.offset
            buf[o: o + s.image.size] = s.image.reshape(-1)
            o = hb.ann_off + da.offset
            buf[o: o + s.ann.size] = s.ann.reshape(-1)
        hb.indices = [s.index for s in batch]
        hb.sentences = [s.text for s in batch]
        return hb

    # -- caller's side ----------------------------------------------------------------------------------------------------------------
    def free(self, slot: int):
        self._free.put(slot)

    def get(self, block: bool = True, timeout: Optional[float] = None) -> HostBatch:
        item = self._ready.get(block, timeout)
        if isinstance(item, BaseException):
            self._ready.put(item)                    # stays raised for every later call
            raise item
        return item

    def close(self):
        self._stop.set()
        self._thread.join(timeout=10)
        self._pool.shutdown(wait=True, cancel_futures=True)


def slot_capacity(B: int, T: int, max_pixels: int) -> int:
    """Bytes of one ring slot: words, seq_len, B images of up to max_pixels x 3 and B annotations of up to max_pixels x 4."""
    return _align(B * T * 4) + _align(B * 4) + B * (_align(max_pixels * 3) + _align(max_pixels * 4))


def clip_slot_capacity(T: int, n_img: int, max_pixels: int) -> int:
    """Bytes of one ring slot of the clip feed: words, seq_len, n_img frames of up to max_pixels x 3 and one annotation of up to
    max_pixels x 4."""
    return _align(T * 4) + _align(4) + n_img * _align(max_pixels * 3) + _align(max_pixels * 4)


class ClipPipeline(HostPipeline):
    """HostPipeline for the video model: a batch is ONE clip -- words ‖ seq_len ‖ the frames at positions `frame_idx` ‖ the annotation.
    samples[i] -> (frames, annotation, key_or_None, text); only frames[j] for j in frame_idx is ever indexed, so a lazy sequence
    decodes those files alone."""

    def __init__(self, samples, sampler, vocab, T, H, W, buffers, max_pixels, frame_idx, n_frames, skip_empty=False, match=1, workers=WORKERS):
        self.frame_idx, self.n_frames = tuple(int(j) for j in frame_idx), int(n_frames)
        super().__init__(samples, sampler, vocab, 1, T, H, W, buffers, max_pixels, skip_empty=skip_empty, match=match, workers=workers)

    def _capacity(self) -> int:
        return clip_slot_capacity(self.T, len(self.frame_idx), self.max_pixels)

    def _load(self, index: int) -> _Sample:
        frames, annotation, key, text = self.samples[index]
        if hasattr(frames, "__len__") and len(frames) != self.n_frames:
            raise ValueError("sample %d: %d frames, the model's clips hold %d" % (index, len(frames), self.n_frames))
        s = _Sample()
        s.index = index
        try:
            s.image = _images_u8([frames[j] for j in self.frame_idx])
        except ValueError as e:
            raise ValueError("sample %d: %s" % (index, e)) from None
        shape = s.image[0].shape
        for j, f in zip(self.frame_idx, s.image):
            if f.shape != shape:
                raise ValueError("sample %d: frame %d is %s, frame %d is %s (a clip's frames are all one size)" % (index, j, f.shape, self.frame_idx[0], shape))
        s.ann, s.kind, s.key = annotation_u8(annotation, key, index)
        if shape[:2] != s.ann.shape[:2]:
            raise ValueError("sample %d: frames %s, annotation %s (the annotation is at the frames' size)" % (index, shape[:2], s.ann.shape[:2]))
        if shape[0] * shape[1] > self.max_pixels:
            raise ValueError("sample %d: %d x %d pixels exceed the ring's slots (ClipTrainFeeder(max_hw=...) sizes them)" % (index, shape[0], shape[1]))
        s.ids, s.seq_len = encode_text(text, self.vocab, self.T)
        s.text = text if isinstance(text, str) else None
        s.empty = self.skip_empty and not HU.object_mask(annotation, key, self.match).any()
        return s

    def _pack(self, slot: int, batch: List[_Sample]) -> HostBatch:
        s, T = batch[0], self.T
        buf = self.buffers[slot]
        hb = HostBatch()
        hb.slot = slot
        buf[: T * 4].view(np.int32)[...] = s.ids
        buf[self.words_bytes: self.words_bytes + 4].view(np.int32)[...] = s.seq_len
        hb.img_descs, hb.img_bytes = plan_images([f.shape for f in s.image], self.H, self.W)
        hb.ann_descs, hb.ann_bytes = plan_targets([s.ann.shape], [s.kind], [s.key], self.H, self.W, self.match)
        hb.img_off, hb.ann_off = self.img_off, self.img_off + hb.img_bytes
        hb.nbytes = hb.ann_off + hb.ann_bytes
        for f, di in zip(s.image, hb.img_descs):
            o = hb.img_off + di.offset
            buf[o: o + f.size] = f.reshape(-1)
        o = hb.ann_off + hb.ann_descs[0].offset
        buf[o: o + s.ann.size] = s.ann.reshape(-1)
        hb.indices = [s.index]
        hb.sentences = [s.text]
        return hb


class _DeviceStage:
    """The feed's device half, run by the caller's thread only: per slot a pinned host buffer, its device twin and the outputs, all
    allocated here once.  stage() enqueues one copy and one cmpc_train_prep call on the side stream behind the event of the slot's last
    reader; release() records that event."""

    def __init__(self, model, nslots: int, capacity: int, order: int, n_img: Optional[int] = None):
        import torch
        self.torch = torch
        self.model, self.order = model, order
        self.dev = model.device
        B, T, H, W = model.batch_size, model.num_steps, model.H, model.W
        self.B, self.T, self.H, self.W = B, T, H, W
        wb = _align(B * T * 4)
        with torch.cuda.device(self.dev):
            self.stream = torch.cuda.Stream(device=self.dev)
            self.host = [torch.empty(capacity, dtype=torch.uint8, pin_memory=True) for _ in range(nslots)]
            self.raw = [torch.empty(capacity, dtype=torch.uint8, device=self.dev) for _ in range(nslots)]
            self.words = [r[: B * T * 4].view(torch.int32).view(B, T) for r in self.raw]
            self.seq_len = [r[wb: wb + B * 4].view(torch.int32) for r in self.raw]
            self.im = [torch.empty(B if n_img is None else n_img, H, W, 3, dtype=torch.float32, device=self.dev) for _ in range(nslots)]
            self.target = [torch.empty(B, H, W, 1, dtype=torch.float32, device=self.dev) for _ in range(nslots)]
            self.pos = [torch.zeros(B, dtype=torch.int64, device=self.dev) for _ in range(nslots)]
            # every event exists before the first step (the backbone's graph capture must see no new HIP object from here)
            self.ready = [torch.cuda.Event() for _ in range(nslots)]
            self.copied = [torch.cuda.Event() for _ in range(nslots)]
            self.read = [torch.cuda.Event() for _ in range(nslots)]
            for e in self.ready + self.copied + self.read:
                e.record(self.stream)
            torch.cuda.synchronize(self.dev)

    def buffers(self) -> List[np.ndarray]:
        return [h.numpy() for h in self.host]

    def stage(self, hb: HostBatch) -> Dict:
        torch, k, fs = self.torch, hb.slot, self.stream
        with torch.cuda.device(self.dev):
            fs.wait_event(self.read[k])              # the step that last read this slot's tensors
            raw = self.raw[k]
            with torch.cuda.stream(fs):
                raw[: hb.nbytes].copy_(self.host[k][: hb.nbytes], non_blocking=True)
                self.copied[k].record(fs)
                self._prep(hb, k, raw.data_ptr(), fs.cuda_stream)
                self.ready[k].record(fs)
        return {"words": self.words[k], self.IM_KEY: self.im[k], "target_fine": self.target[k], "seq_len": self.seq_len[k], "pos": self.pos[k],
                "ready": self.ready[k], "indices": hb.indices, "sentences": hb.sentences, "skipped": hb.skipped, "slot": k}

    IM_KEY = "im"

    def _prep(self, hb: HostBatch, k: int, base: int, st: int):
        _lib.call("cmpc_train_prep", base + hb.img_off, hb.img_bytes, hb.img_descs, base + hb.ann_off, hb.ann_bytes, hb.ann_descs,
                  self.B, self.H, self.W, self.order, None, self.im[k].data_ptr(), self.target[k].data_ptr(), self.pos[k].data_ptr(), st)

    def wait_ready(self, feed: Dict):
        """Order the current stream behind the batch (words, seq_len and target_fine are read there; the backbone waits for `ready` itself)."""
        self.torch.cuda.current_stream(self.dev).wait_event(feed["ready"])

    def release(self, slot: int):
        self.read[slot].record(self.torch.cuda.current_stream(self.dev))

    def copied_done(self, slot: int) -> bool:
        return self.copied[slot].query()

    def close(self):
        self.torch.cuda.synchronize(self.dev)


class _ClipStage(_DeviceStage):
    """_DeviceStage for the video model: the slot's images are the clip's sampled frames, prepared by one cmpc_clip_prep call."""
    IM_KEY = "frames"

    def __init__(self, model, nslots: int, capacity: int, order: int):
        super().__init__(model, nslots, capacity, order, n_img=len(model.FRAME_IDX))

    def _prep(self, hb: HostBatch, k: int, base: int, st: int):
        _lib.call("cmpc_clip_prep", base + hb.img_off, hb.img_bytes, hb.img_descs, len(hb.img_descs), base + hb.ann_off, hb.ann_bytes,
                  hb.ann_descs, self.H, self.W, self.order, self.im[k].data_ptr(), self.target[k].data_ptr(), self.pos[k].data_ptr(), st)


class _RingFeeder:
    """What TrainFeeder and ClipTrainFeeder share: feeds staged ahead through `self.stage` / `self.pipe`, handed out one at a time."""

    def _start(self, depth: int):
        self.depth = depth
        self._staged = deque()                       # feeds staged and not handed out yet
        self._current = None                         # the feed handed out last (released when the next one is requested)
        self._copying: List[int] = []                # released slots whose pinned bytes may still be in flight
        self._closed = False
        self.skipped = 0                             # samples dropped (skip_empty) in the stream up to the feed handed out last

    def _recycle(self):
        """Hand the slots released by the caller back to the packer once their bytes have left the pinned buffer (a query, no wait)."""
        keep = []
        for k in self._copying:
            if self.stage.copied_done(k):
                self.pipe.free(k)
            else:
                keep.append(k)
        self._copying = keep

    def _fill(self, need: int):
        """Stage batches until `need` are waiting (blocking for the packer), then whatever else is ready up to the look-ahead depth."""
        while len(self._staged) < self.depth:
            self._recycle()
            must = len(self._staged) < need
            try:
                hb = self.pipe.get(timeout=0.002) if must else self.pipe.get(block=False)
            except queue.Empty:
                if must:
                    continue
                return
            except BaseException:
                if must:
                    raise
                return                               # a worker's error surfaces when its batch is due, not ahead of the staged ones
            self._staged.append(self.stage.stage(hb))

    def _release_current(self):
        if self._current is not None:
            self.stage.release(self._current["slot"])
            self._copying.append(self._current["slot"])
            self._current = None

    def __iter__(self):
        return self

    def __next__(self) -> Dict:
        if self._closed:
            raise StopIteration
        self._release_current()
        self._fill(1)
        self._current = self._staged.popleft()
        self.skipped = self._current["skipped"]
        return self._current

    def peek(self) -> Dict:
        """The feed after the current one (staged, not handed out): the look-ahead batch."""
        self._fill(1)
        return self._staged[0]

    def close(self):
        if self._closed:
            return
        self._closed = True
        self.pipe.close()
        self.stage.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class TrainFeeder(_RingFeeder):
    """Raw samples -> device-resident train feeds, prepared on a side stream while the previous step runs.

    samples[i] returns (image, annotation, key_or_None, text); `sampler` yields indices endlessly (default EpochSampler(len(samples)));
    text is a sentence (needs `vocab`, hostutil.load_vocab_dict_from_file), an (ids, seq_len) pair, or a front-padded id row.  B, T, H, W
    are the model's.  Iterating yields feeds: dicts of `words` int32 [B, T], `im` float32 [B, H, W, 3], `target_fine` float32 [B, H, W, 1],
    `seq_len` int32 [B], `pos` int64 [B] (foreground pixels of each target: 0 = the object is absent), all device tensors of the ring,
    `ready` (the event recorded once they are complete), and the host-side `indices` and `sentences`.  A feed's tensors stay valid for
    work enqueued on the current stream until the next feed is requested.  step() runs model.train_step on the next feed, its backbone
    waiting for `ready` alone; with lookahead=True it also hands over the look-ahead batch as `next_im`, so that batch's backbone pass
    is enqueued where train_step's docstring says.  Bit-identical either way; the default is the faster one (the
    look-ahead placement costs the step 9 % with resident feeds already, as bench.py --prefetch shows).

    depth: batches staged ahead of the one in use; the ring holds depth + model.MAX_STEPS_IN_FLIGHT slots, each sized for B samples of
    up to max_hw pixels (a larger sample raises ValueError).  skip_empty drops samples whose object is absent at the original size
    (counted in `skipped`); by default they are kept, their target all zero and pos 0.  close() stops the threads."""

    def __init__(self, model, samples, sampler=None, vocab=None, order: int = 1, depth: int = 2, skip_empty: bool = False, match: int = 1,
                 max_hw: Tuple[int, int] = (720, 1280), workers: int = WORKERS, lookahead: bool = False, _stage=None):
        if getattr(model, "video", False):
            raise ValueError("TrainFeeder: the video model (CMPC_video_mm_tgraph_allvec) is not supported here: ClipTrainFeeder feeds it from raw clips")
        _check_order(order)
        if depth < 1:
            raise ValueError("depth must be >= 1 (the look-ahead batch), got %d" % depth)
        self.model, self.order, self.lookahead = model, order, bool(lookahead)
        self.B, self.T, self.H, self.W = model.batch_size, model.num_steps, model.H, model.W
        if self.B > MAX_BATCH:
            raise ValueError("TrainFeeder: model.batch_size %d > %d" % (self.B, MAX_BATCH))
        max_pixels = int(max_hw[0]) * int(max_hw[1])
        nslots = depth + int(getattr(model, "MAX_STEPS_IN_FLIGHT", 2))
        self.stage = _stage if _stage is not None else _DeviceStage(model, nslots, slot_capacity(self.B, self.T, max_pixels), order)
        if sampler is None:
            sampler = EpochSampler(len(samples))
        self.pipe = HostPipeline(samples, sampler, vocab, self.B, self.T, self.H, self.W, self.stage.buffers(), max_pixels,
                                 skip_empty=skip_empty, match=match, workers=workers)
        self._start(depth)

    def step(self):
        """One model.train_step on the next feed; returns train_step's result.  With lookahead the staged batch behind it goes along as
        next_im / next_ready, and the following call passes the very tensor it showed there, so train_step finds its taps ready."""
        feed = next(self)
        nxt = self.peek()
        self.stage.wait_ready(feed)
        self.last_feed = feed
        if not self.lookahead:                       # the batches are staged ahead all the same; each backbone pass starts with its own step
            return self.model.train_step(feed["words"], feed["im"], feed["target_fine"], feed["seq_len"], ready=feed["ready"])
        return self.model.train_step(feed["words"], feed["im"], feed["target_fine"], feed["seq_len"], ready=feed["ready"],
                                     next_im=nxt["im"], next_ready=nxt["ready"])


class ClipTrainFeeder(_RingFeeder):
    """Raw clips -> device-resident train feeds of the video model (CMPC_video_mm_tgraph_allvec), TrainFeeder's machinery per clip.

    samples[i] returns (frames, annotation, key_or_None, text).  frames: a sequence of model.frames items or an array [frames, h, w, 3];
    only positions model.FRAME_IDX are indexed (a lazy sequence decodes 5 files, not 16); those frames are uint8 [h, w, 3] or [h, w], all
    one size.  annotation: at that size, colour-coded with a key colour or (key None) a plain mask, bool accepted; it belongs to clip
    position frames // 2.  text as for TrainFeeder.  A stored train sample of build_A2D_batches.py:137-143 is
    (z["frames"], z["mask_batch"], None, z["text_batch"]): already at H x W, the identity geometry.

    Feeds are dicts of `words` int32 [1, T] (END-padded), `seq_len` int32 [1], `frames` float32 [5, H, W, 3] (BGR - mu),
    `target_fine` float32 [1, H, W, 1], `pos` int64 [1], device tensors of the ring, plus `ready`, `indices`, `sentences`, `skipped`,
    `slot`.  Per clip the caller's thread issues one host-to-device copy and one cmpc_clip_prep call on the feeder's side stream; a slot
    is reused only behind the event recorded after the step that read it; nothing is allocated or synchronised in the steady state.
    step(accuracy=False) runs model.train_step_video_frames on the next feed, its backbone waiting for `ready` alone.  There is no
    look-ahead backbone pass: the video step has no next_im.  sampler, order, depth, skip_empty, match, max_hw, workers, peek(), close()
    and the context manager behave as in TrainFeeder."""

    def __init__(self, model, samples, sampler=None, vocab=None, order: int = 1, depth: int = 2, skip_empty: bool = False, match: int = 1,
                 max_hw: Tuple[int, int] = (720, 1280), workers: int = WORKERS, _stage=None):
        if not getattr(model, "video", False):
            raise ValueError("ClipTrainFeeder feeds the video model (CMPC_video_mm_tgraph_allvec); TrainFeeder feeds the image models")
        _check_order(order)
        if depth < 1:
            raise ValueError("depth must be >= 1 (the clip staged behind the one in use), got %d" % depth)
        self.model, self.order = model, order
        self.T, self.H, self.W = model.num_steps, model.H, model.W
        frame_idx = tuple(model.FRAME_IDX)
        if len(frame_idx) > _lib.TAPS_MAX_FRAMES:
            raise ValueError("ClipTrainFeeder: %d sampled frames > %d" % (len(frame_idx), _lib.TAPS_MAX_FRAMES))
        max_pixels = int(max_hw[0]) * int(max_hw[1])
        nslots = depth + int(getattr(model, "MAX_STEPS_IN_FLIGHT", 2))
        self.stage = _stage if _stage is not None else _ClipStage(model, nslots, clip_slot_capacity(self.T, len(frame_idx), max_pixels), order)
        if sampler is None:
            sampler = EpochSampler(len(samples))
        self.pipe = ClipPipeline(samples, sampler, vocab, self.T, self.H, self.W, self.stage.buffers(), max_pixels, frame_idx, model.frames,
                                 skip_empty=skip_empty, match=match, workers=workers)
        self._start(depth)

    def step(self, accuracy: bool = False):
        """One model.train_step_video_frames on the next feed; returns its result.  The clip behind it is staged first, so its copy and
        prep run beside this step."""
        feed = next(self)
        self.peek()
        self.stage.wait_ready(feed)
        self.last_feed = feed
        return self.model.train_step_video_frames(feed["words"], feed["seq_len"], feed["frames"], feed["target_fine"], ready=feed["ready"],
                                                  accuracy=accuracy)
