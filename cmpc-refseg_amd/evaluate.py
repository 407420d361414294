"""Batched evaluation of a referring-segmentation split on the GPU: the reference's `-m test` loop (trainval_model.py:150-303).

Every sample keeps its ORIGINAL size (build_batches.py:63-66 resizes only the train splits).  Per batch:

    feed, proc_im = prepare_images(images, H, W)      # img_as_ubyte(resize_and_pad(im)) and BGR - mu  (cmpc_eval_prep)
    up = model.forward(ids, feed, seq_len)["up"]      # the forward pass on the device feed
    iu = mask_iu(up, gt_masks, 1e-9)                  # I, U of resize_and_crop(up >= 1e-9) vs the mask  (cmpc_eval_mask_iu)

    ev = Evaluator(model); ev.add(ids, seq_len, image, gt_mask) ...; ev.result()

Host work per batch is packing uint8 bytes and descriptors into a pinned staging buffer (double-buffered behind an event) and one
copy to the device; per-sample (I, U) stay on the device until Evaluator.result().  The resampled pixels follow hostutil's
restatement of skimage.transform.resize (parity-unpinned against scikit-image itself).
"""
from __future__ import annotations

from typing import Dict, List, Sequence, Tuple

import numpy as np
import torch

from . import _lib, hostutil as HU

MAX_BATCH = _lib.EVAL_MAX_BATCH
_ALIGN = 16


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


def _masks_u8(masks) -> List[np.ndarray]:
    out = []
    for i, m in enumerate(masks):
        a = np.asarray(m)
        if a.ndim == 3 and a.shape[2] == 1:
            a = a[:, :, 0]
        if a.ndim != 2 or a.shape[0] == 0 or a.shape[1] == 0:
            raise ValueError("mask %d: expected [h, w] with h, w > 0, got %s" % (i, a.shape))
        out.append(np.ascontiguousarray(a != 0).view(np.uint8))
    return out


def _check_batch(n: int):
    if n <= 0 or n > MAX_BATCH:
        raise ValueError("batch of %d samples: expected 1..%d per call (split larger batches)" % (n, MAX_BATCH))


def plan_prep(shapes: Sequence[Tuple[int, ...]], H: int, W: int):
    """Descriptors (cmpc_eval_desc[B]) and packed length of images of the given shapes ([h, w] or [h, w, c]) for cmpc_eval_prep:
    16-byte aligned offsets, resize_and_pad_geometry(h, w, H, W)."""
    _check_batch(len(shapes))
    d = (_lib.EvalDesc * len(shapes))()
    off = 0
    for i, s in enumerate(shapes):
        h, w = int(s[0]), int(s[1])
        c = int(s[2]) if len(s) == 3 else 1
        rh, rw, top, left = HU.resize_and_pad_geometry(h, w, H, W)
        d[i] = _lib.EvalDesc(off, h, w, c, rh, rw, top, left, 0)
        off += -(-h * w * c // _ALIGN) * _ALIGN
    return d, off


def plan_masks(shapes: Sequence[Tuple[int, ...]], H: int, W: int):
    """Descriptors and packed length of ground-truth masks [mh, mw] for cmpc_eval_mask_iu against an [H, W] map:
    resize_and_crop_geometry(H, W, mh, mw)."""
    _check_batch(len(shapes))
    d = (_lib.EvalDesc * len(shapes))()
    off = 0
    for i, s in enumerate(shapes):
        h, w = int(s[0]), int(s[1])
        rh, rw, top, left = HU.resize_and_crop_geometry(H, W, h, w)
        d[i] = _lib.EvalDesc(off, h, w, 1, rh, rw, top, left, 0)
        off += -(-h * w // _ALIGN) * _ALIGN
    return d, off


class _Staging:
    """Two pinned host buffers and their device twins: packing batch n+1 waits (on the event of the copy that last used the slot)
    only until the bytes of batch n-1 have left, never for the device work behind them."""

    def __init__(self, device):
        self.device = torch.device(device)
        self.host: List[torch.Tensor] = [None, None]
        self.dev: List[torch.Tensor] = [None, None]
        self.ev = [None, None]
        self.k = 0

    def upload(self, arrays: Sequence[np.ndarray], descs, nbytes: int) -> torch.Tensor:
        k = self.k
        self.k = 1 - k
        if self.ev[k] is not None:
            self.ev[k].synchronize()
        if self.host[k] is None or self.host[k].numel() < nbytes:
            cap = max(nbytes, 1 << 20)
            self.host[k] = torch.empty(cap, dtype=torch.uint8, pin_memory=True)
            self.dev[k] = torch.empty(cap, dtype=torch.uint8, device=self.device)
        hv = self.host[k].numpy()
        for a, d in zip(arrays, descs):
            n = a.size
            hv[d.offset: d.offset + n] = a.reshape(-1)
        dev = self.dev[k][:nbytes]
        dev.copy_(self.host[k][:nbytes], non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(self.device))
        self.ev[k] = ev
        return dev


_STAGING: Dict[Tuple[str, str], _Staging] = {}


def _staging(device, kind: str) -> _Staging:
    key = (str(torch.device(device)), kind)
    if key not in _STAGING:
        _STAGING[key] = _Staging(device)
    return _STAGING[key]


def prepare_images(images, H: int, W: int, device="cuda:0") -> Tuple[torch.Tensor, torch.Tensor]:
    """resize_and_pad + img_as_ubyte + BGR - mu of original-size uint8 images ([h, w, 3] or [h, w]) on the device:
    (feed float32 [B, H, W, 3], proc_im uint8 [B, H, W, 3]).  Enqueued on the current stream; nothing synchronises."""
    ims = _images_u8(images)
    descs, nbytes = plan_prep([a.shape for a in ims], H, W)
    dev = torch.device(device)
    with torch.cuda.device(dev):
        src = _staging(dev, "im").upload(ims, descs, nbytes)
        B = len(ims)
        proc = torch.empty(B, H, W, 3, dtype=torch.uint8, device=dev)
        feed = torch.empty(B, H, W, 3, dtype=torch.float32, device=dev)
        _lib.call("cmpc_eval_prep", src.data_ptr(), nbytes, descs, B, H, W, proc.data_ptr(), feed.data_ptr(),
                  torch.cuda.current_stream(dev).cuda_stream)
    return feed, proc


def _upload_masks(masks, H, W, device):
    ms = _masks_u8(masks)
    descs, nbytes = plan_masks([m.shape for m in ms], H, W)
    return ms, descs, nbytes, _staging(device, "gt").upload(ms, descs, nbytes)


def mask_iu(score_map, gt_masks, thresh: float = 1e-9, want_masks: bool = False, out: torch.Tensor = None):
    """(I, U) per sample of compute_mask_IU(resize_and_crop(score_map >= thresh, mh, mw), gt) on the device.
    score_map: device tensor [B, H, W] (or [B, H, W, 1]) float32 (`up`) or uint8 (the DenseCRF argmax); gt_masks: B host arrays [mh, mw].
    Returns an int64 device tensor [B, 2] (written into `out` when given), plus with want_masks the predicted masks at the original
    sizes (list of uint8 {0, 1} device tensors)."""
    m = score_map
    if not torch.is_tensor(m) or m.device.type != "cuda":
        raise ValueError("score_map must be a device tensor")
    if m.dim() == 4 and m.shape[3] == 1:
        m = m[..., 0]
    if m.dim() != 3 or m.dtype not in (torch.float32, torch.uint8):
        raise ValueError("score_map must be [B, H, W] float32 or uint8, got %s %s" % (m.dtype, tuple(m.shape)))
    m = m.contiguous()
    B, H, W = m.shape
    if len(gt_masks) != B:
        raise ValueError("%d masks for a batch of %d maps" % (len(gt_masks), B))
    dev = m.device
    with torch.cuda.device(dev):
        ms, descs, nbytes, gt = _upload_masks(gt_masks, H, W, dev)
        iu = out if out is not None else torch.empty(B, 2, dtype=torch.int64, device=dev)
        if tuple(iu.shape) != (B, 2) or iu.dtype != torch.int64 or not iu.is_contiguous():
            raise ValueError("out must be a contiguous int64 [B, 2] tensor")
        mo = torch.empty(nbytes, dtype=torch.uint8, device=dev) if want_masks else None
        dt = _lib.EVAL_F32 if m.dtype == torch.float32 else _lib.EVAL_U8
        _lib.call("cmpc_eval_mask_iu", m.data_ptr(), dt, B, H, W, float(thresh), gt.data_ptr(), nbytes, descs, iu.data_ptr(),
                  mo.data_ptr() if mo is not None else None, torch.cuda.current_stream(dev).cuda_stream)
    if not want_masks:
        return iu
    return iu, [mo[d.offset: d.offset + d.h * d.w].view(d.h, d.w) for d in descs]


def _check_model(model):
    if getattr(model, "video", False):
        raise ValueError("Evaluator: the video model (CMPC_video_mm_tgraph_allvec) is not supported; its A2D evaluation is out of scope")


def _pad_to(items: list, B: int) -> list:
    return list(items) + [items[0]] * (B - len(items))


def predict_masks(model, ids, seq_len, images) -> List[np.ndarray]:
    """Inference only: the reference's `predicts` (resize_and_crop(up >= 1e-9) at each image's original size) for up to
    model.batch_size samples, as host uint8 {0, 1} arrays."""
    _check_model(model)
    images = list(images)
    n, B = len(images), model.batch_size
    if n == 0 or n > B:
        raise ValueError("predict_masks: 1..%d samples per call, got %d" % (B, n))
    ids, seq_len = np.asarray(ids, dtype=np.int32).reshape(n, -1), np.asarray(seq_len, dtype=np.int32).reshape(n)
    feed, _ = prepare_images(_pad_to(images, B), model.H, model.W, model.device)
    up = model.forward(np.concatenate([ids, np.repeat(ids[:1], B - n, 0)]), feed, np.concatenate([seq_len, np.repeat(seq_len[:1], B - n)]))["up"]
    zeros = [np.zeros(np.asarray(im).shape[:2], dtype=np.uint8) for im in images]
    _, masks = mask_iu(up[:n].float(), zeros, 1e-9, want_masks=True)
    return [mk.cpu().numpy() for mk in masks]


class Evaluator:
    """The `-m test` loop (trainval_model.py:198-303) batched on the GPU.  add() queues one sample (end-padded ids [T], seq_len,
    original-size uint8 image, original-size mask); a batch of model.batch_size samples runs prep -> forward -> mask_iu (and with
    dcrf, DenseCRF on each sample's sigm / proc_im -> mask_iu on the argmax).  result() flushes a partial last batch (padded by
    repeating a sample; pads are never counted) and returns hostutil.SegEval.result()'s keys plus `samples` (and `dcrf_`-prefixed
    metrics with dcrf)."""

    def __init__(self, model, thresholds: Sequence[float] = (.5, .6, .7, .8, .9), dcrf: bool = False, score_thresh: float = 1e-9):
        _check_model(model)
        self.model, self.thresholds, self.dcrf, self.score_thresh = model, tuple(thresholds), bool(dcrf), float(score_thresh)
        self.B, self.H, self.W = model.batch_size, model.H, model.W
        if self.B > MAX_BATCH:
            raise ValueError("Evaluator: model.batch_size %d > %d" % (self.B, MAX_BATCH))
        self.queue = []
        self.n = 0
        self.iu = torch.zeros(64, 2, dtype=torch.int64, device=model.device)
        self.iu_crf = torch.zeros(64, 2, dtype=torch.int64, device=model.device) if self.dcrf else None

    def add(self, ids, seq_len, image, gt_mask):
        self.queue.append((np.asarray(ids, dtype=np.int32).reshape(-1), int(seq_len), image, gt_mask))
        if len(self.queue) == self.B:
            self._run()

    def _grow(self, need: int):
        if need > self.iu.shape[0]:
            cap = max(need, 2 * self.iu.shape[0])
            self.iu = torch.cat([self.iu, torch.zeros(cap - self.iu.shape[0], 2, dtype=torch.int64, device=self.iu.device)])
            if self.dcrf:
                self.iu_crf = torch.cat([self.iu_crf, torch.zeros(cap - self.iu_crf.shape[0], 2, dtype=torch.int64, device=self.iu.device)])

    def _run(self):
        q, self.queue = self.queue, []
        n = len(q)
        if n == 0:
            return
        q = _pad_to(q, self.B)
        m = self.model
        ids = np.stack([s[0] for s in q])
        sl = np.array([s[1] for s in q], dtype=np.int32)
        with torch.cuda.device(m.device):
            feed, proc = prepare_images([s[2] for s in q], self.H, self.W, m.device)
            out = m.forward(ids, feed, sl)
            gts = [s[3] for s in q[:n]]
            self._grow(self.n + n)
            mask_iu(out["up"][:n].float(), gts, self.score_thresh, out=self.iu[self.n: self.n + n])
            if self.dcrf:
                from . import crf
                sigm = out["sigm"].float()
                crf_masks = torch.stack([crf.dense_crf_mask(sigm[b].reshape(self.H, self.W), proc[b], device=m.device) for b in range(n)])
                mask_iu(crf_masks, gts, 0.5, out=self.iu_crf[self.n: self.n + n])
        self.n += n

    def _metrics(self, iu: np.ndarray) -> Dict[str, float]:
        # hostutil.SegEval's arithmetic, in sample order
        cum_I = cum_U = 0
        sum_iou = 0.0
        correct = np.zeros(len(self.thresholds), dtype=np.int64)
        for I, U in iu.tolist():
            iou = float(I) / U
            cum_I += I
            cum_U += U
            sum_iou += iou
            correct += np.array([iou >= t for t in self.thresholds])
        total = len(iu)
        out = {"precision@%s" % t: float(c) / total for t, c in zip(self.thresholds, correct)}
        out["overall_IoU"] = cum_I / cum_U
        out["mean_IoU"] = sum_iou / total
        return out

    def per_sample(self) -> np.ndarray:
        """(I, U) of every sample added so far (flushes the partial batch), int64 [n, 2]."""
        self._run()
        return self.iu[: self.n].cpu().numpy()

    def result(self) -> Dict[str, float]:
        self._run()
        if self.n == 0:
            raise ValueError("Evaluator.result: no samples")
        iu = self.iu[: self.n].cpu().numpy()
        out = self._metrics(iu)
        out["samples"] = self.n
        if self.dcrf:
            out.update({"dcrf_" + k: v for k, v in self._metrics(self.iu_crf[: self.n].cpu().numpy()).items()})
        return out
