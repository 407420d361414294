"""Batched evaluation of a referring-segmentation split on the GPU: the reference's `-m test` loop (trainval_model.py:150-303).

Every sample keeps its ORIGINAL size (build_batches.py:63-66 resizes only the train splits).  Per batch:

    feed, proc_im = prepare_images(images, H, W)      # img_as_ubyte(resize_and_pad(im)) and BGR - mu  (cmpc_eval_prep)
    up = model.forward(ids, feed, seq_len)["up"]      # the forward pass on the device feed
    iu = mask_iu(up, gt_masks, 1e-9)                  # I, U of resize_and_crop(up >= 1e-9) vs the mask  (cmpc_eval_mask_iu)

    ev = Evaluator(model); ev.add(ids, seq_len, image, gt_mask) ...; ev.result()

The video model (CMPC_video_mm_tgraph_allvec, batch 1) on an A2D split (CMPC_video/trainval_video.py:136-291) goes through VideoEvaluator:
one clip per forward pass, the 5 sampled frames (plus the key image for DenseCRF) resized by one cmpc_eval_prep launch, the forward pass on
that device feed (LSTM_model.forward_video_frames), I / U by cmpc_eval_mask_iu at the mask's size, precision at the driver's ten thresholds:

    ev = VideoEvaluator(model); ev.add(text_batch, im_batch, frames, mask_batch) ...; ev.result()

Host work per batch is packing uint8 bytes and descriptors into a pinned staging buffer (double-buffered behind an event) and one
copy to the device; per-sample (I, U) stay on the device until Evaluator.result().  The resampled pixels follow hostutil's
restatement of skimage.transform.resize (parity-unpinned against scikit-image itself).
"""
from __future__ import annotations

import contextlib
from typing import Dict, List, Optional, Sequence, Tuple

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


def _prepare_images(images, H: int, W: int, device):
    """prepare_images' work: (feed, proc_im, the packed source images on the device, their descriptors, the packed length).  The source
    buffer is a staging slot: it holds these bytes until the second call after this one enqueues its upload on the same stream."""
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
    return feed, proc, src, descs, nbytes


def prepare_images(images, H: int, W: int, device="cuda:0") -> Tuple[torch.Tensor, torch.Tensor]:
    """resize_and_pad + img_as_ubyte + BGR - mu of original-size uint8 images ([h, w, 3] or [h, w]) on the device:
    (feed float32 [B, H, W, 3], proc_im uint8 [B, H, W, 3]).  Enqueued on the current stream; nothing synchronises."""
    feed, proc, _, _, _ = _prepare_images(images, H, W, device)
    return feed, proc


def _upload_masks(masks, H, W, device):
    ms = _masks_u8(masks)
    descs, nbytes = plan_masks([m.shape for m in ms], H, W)
    return ms, descs, nbytes, _staging(device, "gt").upload(ms, descs, nbytes)


def _mask_iu(score_map, gt_masks, thresh: float, want_masks: bool, out: torch.Tensor):
    """mask_iu's work: (iu, packed predicted masks or None, descriptors, packed length, the uploaded ground truths on the device)."""
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
    return iu, mo, descs, nbytes, gt


def mask_iu(score_map, gt_masks, thresh: float = 1e-9, want_masks: bool = False, out: torch.Tensor = None):
    """(I, U) per sample of compute_mask_IU(resize_and_crop(score_map >= thresh, mh, mw), gt) on the device.
    score_map: device tensor [B, H, W] (or [B, H, W, 1]) float32 (`up`) or uint8 (the DenseCRF argmax); gt_masks: B host arrays [mh, mw].
    Returns an int64 device tensor [B, 2] (written into `out` when given), plus with want_masks the predicted masks at the original
    sizes (list of uint8 {0, 1} device tensors)."""
    iu, mo, descs, _, _ = _mask_iu(score_map, gt_masks, thresh, want_masks, out)
    if not want_masks:
        return iu
    return iu, [mo[d.offset: d.offset + d.h * d.w].view(d.h, d.w) for d in descs]


def masks_out(score_map, sizes: Sequence[Tuple[int, int]], thresh: float = 1e-9, value: int = 1, out: torch.Tensor = None):
    """value * (resize_and_crop(score_map[b] >= thresh, oh, ow) > 0) per sample on the device, with no ground truth (cmpc_eval_mask_out):
    mask_iu's decision at any output size.  score_map as for mask_iu; sizes: one (oh, ow) per sample; value 1 or 255.  Returns
    (buf, descs): a flat uint8 device buffer (`out` when given: it must hold the packed length) and the descriptors whose 16-byte
    aligned offsets locate sample b's [oh, ow] mask in it (unpack_masks).  Bytes between the masks are not written.

    The rule is "resampled value > 0" (trainval_model.py:245 with compute_mask_IU), as everywhere in this package.  test.py:308 casts the
    resampled float map with .astype('uint8') instead, which keeps only values that are exactly >= 1.0: with this resampler an all-ones
    320 x 320 map comes out 98.4 % foreground at (240, 427) and 0.19 % at (166, 250).  That is an accident of rounding, not reproduced."""
    m = score_map
    if not torch.is_tensor(m) or m.device.type != "cuda":
        raise ValueError("score_map must be a device tensor")
    if m.dim() == 4 and m.shape[3] == 1:
        m = m[..., 0]
    if m.dim() != 3 or m.dtype not in (torch.float32, torch.uint8):
        raise ValueError("score_map must be [B, H, W] float32 or uint8, got %s %s" % (m.dtype, tuple(m.shape)))
    m = m.contiguous()
    B, H, W = m.shape
    if len(sizes) != B:
        raise ValueError("%d sizes for a batch of %d maps" % (len(sizes), B))
    descs, nbytes = plan_masks(sizes, H, W)
    dev = m.device
    with torch.cuda.device(dev):
        buf = out if out is not None else torch.empty(nbytes, dtype=torch.uint8, device=dev)
        if buf.dtype != torch.uint8 or buf.dim() != 1 or buf.numel() < nbytes or not buf.is_contiguous() or buf.device != dev:
            raise ValueError("out must be a contiguous uint8 device buffer of at least %d bytes" % nbytes)
        dt = _lib.EVAL_F32 if m.dtype == torch.float32 else _lib.EVAL_U8
        _lib.call("cmpc_eval_mask_out", m.data_ptr(), dt, B, H, W, float(thresh), descs, buf.data_ptr(), buf.numel(), int(value),
                  torch.cuda.current_stream(dev).cuda_stream)
    return buf, descs


def train_accuracy(pred, target_fine, out: torch.Tensor = None) -> torch.Tensor:
    """Per sample (n_pos, n_neg, correct_pos, correct_neg) of compute_accuracy(pred[b], resize_bilinear(target_fine, pred's size)[b])
    (util/processing_tools.py:24-35 on model.pred / model.target) on the device: one cmpc_train_accuracy launch on the current stream,
    nothing synchronises.  pred: float32 device tensor [B, h, w] or [B, h, w, 1]; target_fine: float32 [B, H, W] or [B, H, W, 1] on
    the same device, h <= H, w <= W.  Returns an int64 device tensor [B, 4] (`out` when given); hostutil.accuracy_from_counts turns it
    into the three fractions."""
    ts = []
    for name, t in (("pred", pred), ("target_fine", target_fine)):
        if not torch.is_tensor(t) or t.device.type != "cuda" or t.dtype != torch.float32:
            raise ValueError("%s must be a float32 device tensor" % name)
        if t.dim() == 4 and t.shape[3] == 1:
            t = t[..., 0]
        if t.dim() != 3:
            raise ValueError("%s must be [B, h, w] or [B, h, w, 1], got %s" % (name, tuple(t.shape)))
        ts.append(t.contiguous())
    p, f = ts
    if p.device != f.device or p.shape[0] != f.shape[0]:
        raise ValueError("pred %s on %s and target_fine %s on %s: one device and one batch size" % (tuple(p.shape), p.device, tuple(f.shape), f.device))
    B, h, w = p.shape
    H, W = f.shape[1:]
    if B > MAX_BATCH or h > H or w > W:
        raise ValueError("pred [%d, %d, %d] against target_fine [%d, %d]: at most %d samples, and pred no larger than the target" % (B, h, w, H, W, MAX_BATCH))
    dev = p.device
    with torch.cuda.device(dev):
        counts = out if out is not None else torch.empty(B, 4, dtype=torch.int64, device=dev)
        if tuple(counts.shape) != (B, 4) or counts.dtype != torch.int64 or not counts.is_contiguous() or counts.device != dev:
            raise ValueError("out must be a contiguous int64 [B, 4] tensor on %s" % dev)
        _lib.call("cmpc_train_accuracy", p.data_ptr(), f.data_ptr(), B, h, w, H, W, counts.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
    return counts


# ---- J and F of video object segmentation: cmpc_mask_jf (include/cmpc.h; hostutil.jf_from_counts / JFEval turn the counts into scores) --
JF_COUNTS = 6                  # I, U, n_pred, n_gt, pred_match, gt_match


class JfPlan:
    """One cmpc_mask_jf call: `n` samples and their descriptors.  Prediction offsets are as given.  With `gts` (host uint8 arrays) the
    ground truths are packed at 16-byte aligned offsets for one upload (gt_offs, gt_bytes); with `gt_offs` they are where the caller
    says.  ws_bytes: the workspace the call needs; idx: which of the caller's results each sample scores; counts_off: where the
    caller keeps the counts."""
    __slots__ = ("n", "descs", "gts", "gt_offs", "gt_bytes", "ws_bytes", "idx", "counts_off")

    def __init__(self, sizes: Sequence[Tuple[int, int]], pred_offs: Sequence[int], gts: Optional[Sequence[np.ndarray]] = None,
                 gt_offs: Optional[Sequence[int]] = None, bound_th: float = 0.008, idx: Optional[Sequence[int]] = None, counts_off: int = 0):
        _check_batch(len(sizes))
        self.n = len(sizes)
        self.descs = (_lib.JfDesc * self.n)()
        self.gts, self.gt_offs, off = (None if gts is None else list(gts)), [], 0
        for i, ((h, w), po) in enumerate(zip(sizes, pred_offs)):
            h, w = int(h), int(w)
            r = HU.jf_radius(h, w, bound_th)
            if r > _lib.JF_MAX_RADIUS:
                raise ValueError("sample %d: radius %d at %d x %d exceeds %d" % (i, r, h, w, _lib.JF_MAX_RADIUS))
            go = off if gt_offs is None else int(gt_offs[i])
            self.descs[i] = _lib.JfDesc(int(po), go, h, w, r, 0)
            self.gt_offs.append(_Offset(go))
            off = max(off, go + -(-h * w // _ALIGN) * _ALIGN) if gt_offs is not None else off + -(-h * w // _ALIGN) * _ALIGN
        self.gt_bytes = off
        self.ws_bytes = jf_workspace(self.descs, self.n)
        self.idx = list(range(self.n)) if idx is None else list(idx)
        self.counts_off = int(counts_off)


def jf_workspace(descs, n: int) -> int:
    """cmpc_mask_jf_workspace: 2 * h * ceil(w / 64) 64-bit words per sample, in bytes."""
    import ctypes
    out = ctypes.c_int64()
    _lib.call("cmpc_mask_jf_workspace", descs, n, ctypes.byref(out))
    return out.value


class _JfDevice:
    """The device half of scoring, shared by mask_jf and the two segmenters: the plan's ground truths go up through a pinned _Staging
    of their own (or are read where they lie, gt_ptr), cmpc_mask_jf reads the predictions where they lie and writes the counts where
    it is told, all on the current stream.  The workspace grows only when a call needs more than any before it."""

    def __init__(self, device):
        self.device = torch.device(device)
        self.staging = _Staging(self.device)
        self.ws = None

    def score(self, pred_ptr: int, pred_bytes: int, plan: JfPlan, counts_ptr: int, gt_ptr: Optional[int] = None, gt_bytes: int = 0):
        with torch.cuda.device(self.device):
            if self.ws is None or self.ws.numel() * 8 < plan.ws_bytes:
                self.ws = torch.empty(max(plan.ws_bytes // 8, 1 << 15), dtype=torch.int64, device=self.device)
            if gt_ptr is None:
                gt_ptr, gt_bytes = self.staging.upload(plan.gts, plan.gt_offs, plan.gt_bytes).data_ptr(), plan.gt_bytes
            _lib.call("cmpc_mask_jf", pred_ptr, pred_bytes, gt_ptr, gt_bytes, plan.descs, plan.n, counts_ptr,
                      self.ws.data_ptr(), self.ws.numel() * 8, torch.cuda.current_stream(self.device).cuda_stream)


_JF_DEVICE: Dict[str, _JfDevice] = {}


def _mask_addresses(masks, first: int, dev, kind: str):
    """(sizes, device addresses) of a chunk of [h, w] masks: contiguous uint8 tensors on `dev` where they lie, host arrays packed
    into one upload through the `kind` staging."""
    sizes, addr, host = [], [], []
    for i, m in enumerate(masks):
        if torch.is_tensor(m):
            if m.device != dev or m.dtype != torch.uint8 or m.dim() != 2 or not m.is_contiguous() or m.numel() == 0:
                raise ValueError("mask %d: a tensor must be a contiguous uint8 [h, w] on %s, got %s %s on %s"
                                 % (first + i, dev, m.dtype, tuple(m.shape), m.device))
            sizes.append((int(m.shape[0]), int(m.shape[1])))
            addr.append(m.data_ptr())
        else:
            try:
                a = _masks_u8([m])[0]
            except ValueError as e:
                raise ValueError("mask %d: %s" % (first + i, str(e).split(": ", 1)[-1])) from None
            sizes.append(a.shape)
            addr.append(None)
            host.append((i, a))
    if host:
        offs, off = [], 0
        for _, a in host:
            offs.append(_Offset(off))
            off += -(-a.size // _ALIGN) * _ALIGN
        up = _staging(dev, kind).upload([a for _, a in host], offs, off)
        for (i, _), o in zip(host, offs):
            addr[i] = up.data_ptr() + o.offset
    return sizes, addr


def mask_jf(preds, gts, bound_th: float = 0.008, device="cuda:0") -> np.ndarray:
    """The six integers of cmpc_mask_jf (I, U, n_pred, n_gt, pred_match, gt_match) for every (prediction, ground truth) pair: two lists
    of [h, w] masks, non-zero = foreground, each pair of one size and the pairs of any sizes.  Host arrays are packed and uploaded;
    contiguous uint8 device tensors are read in place.  The dilation radius is hostutil.jf_radius(h, w, bound_th).  Runs in chunks of
    MAX_BATCH on the current stream and synchronises once, at the end: returns int64 [n, 6] (hostutil.jf_from_counts, JFEval)."""
    preds, gts = list(preds), list(gts)
    if len(preds) != len(gts) or not preds:
        raise ValueError("mask_jf: %d predictions and %d ground truths" % (len(preds), len(gts)))
    dev = torch.device(device)
    if dev.index is None:
        dev = torch.device(dev.type, torch.cuda.current_device())
    key = str(dev)
    if key not in _JF_DEVICE:
        _JF_DEVICE[key] = _JfDevice(dev)
    jd = _JF_DEVICE[key]
    n = len(preds)
    with torch.cuda.device(dev):
        counts = torch.empty(n, JF_COUNTS, dtype=torch.int64, device=dev)
        for s in range(0, n, MAX_BATCH):
            sizes, pa = _mask_addresses(preds[s: s + MAX_BATCH], s, dev, "jf_pred")
            gsizes, ga = _mask_addresses(gts[s: s + MAX_BATCH], s, dev, "jf_gt")
            for i, (a, b) in enumerate(zip(sizes, gsizes)):
                if a != b:
                    raise ValueError("mask_jf: pair %d: prediction %s, ground truth %s" % (s + i, a, b))
            pb, gb = min(pa), min(ga)
            plan = JfPlan(sizes, [a - pb for a in pa], gt_offs=[a - gb for a in ga], bound_th=bound_th)
            jd.score(pb, max(a + h * w for a, (h, w) in zip(pa, sizes)) - pb, plan, counts[s: s + len(sizes)].data_ptr(),
                     gt_ptr=gb, gt_bytes=max(a + h * w for a, (h, w) in zip(ga, sizes)) - gb)
        return counts.cpu().numpy()


# ---- connected components and mask cleaning: cmpc_mask_components (include/cmpc.h; hostutil.clean_mask is the host twin) ---------------
CC_STATS = 4                   # n_components, area, area_largest, area_kept


def cc_descs(sizes: Sequence[Tuple[int, int]], offs: Sequence[int]):
    """cmpc_cc_desc[n] of [h, w] masks at byte offsets `offs`."""
    _check_batch(len(sizes))
    d = (_lib.CcDesc * len(sizes))()
    for i, ((h, w), o) in enumerate(zip(sizes, offs)):
        if int(h) * int(w) > _lib.CC_MAX_PIXELS:
            raise ValueError("mask %d: %d x %d exceeds %d pixels" % (i, h, w, _lib.CC_MAX_PIXELS))
        d[i] = _lib.CcDesc(int(o), int(h), int(w))
    return d


def cc_workspace(descs, n: int) -> int:
    """cmpc_mask_components_workspace: 64 + 64 n + 8 * sum roundup(h w, 4) bytes."""
    import ctypes
    out = ctypes.c_int64()
    _lib.call("cmpc_mask_components_workspace", descs, n, ctypes.byref(out))
    return out.value


class _CcDevice:
    """The device half of cleaning, shared by mask_components / mask_clean and the two segmenters: cmpc_mask_components works on the
    masks where they lie and writes the statistics (and labels) where it is told, on the current stream.  The workspace grows only
    when a call needs more than any before it (reserve() ahead of the steady state)."""

    def __init__(self, device):
        self.device = torch.device(device)
        self.ws = None

    def reserve(self, nbytes: int):
        if self.ws is None or self.ws.numel() * 4 < nbytes:
            with torch.cuda.device(self.device):
                self.ws = torch.empty(max(-(-nbytes // 4), 1 << 16), dtype=torch.int32, device=self.device)

    def run(self, mask_ptr: int, mask_bytes: int, descs, n: int, connectivity: int, keep: int, min_area: int, stats_ptr: int,
            labels_ptr: Optional[int] = None, ws_bytes: Optional[int] = None):
        with torch.cuda.device(self.device):
            self.reserve(cc_workspace(descs, n) if ws_bytes is None else ws_bytes)
            _lib.call("cmpc_mask_components", mask_ptr, mask_bytes, descs, n, int(connectivity), int(keep), int(min_area), labels_ptr,
                      stats_ptr, self.ws.data_ptr(), self.ws.numel() * 4, torch.cuda.current_stream(self.device).cuda_stream)

    def status(self) -> torch.Tensor:
        """The status word of the last call, as a one-element view of the workspace (read it behind a synchronisation)."""
        return self.ws[:1]


_CC_DEVICE: Dict[str, _CcDevice] = {}


def _components(masks, connectivity: int, keep: int, min_area: int, device, want_labels: bool, who: str):
    keep, min_area, connectivity = HU.check_clean(keep, min_area, connectivity)
    masks = list(masks)
    if not masks:
        raise ValueError("%s: no masks" % who)
    dev = torch.device(device)
    if dev.index is None:
        dev = torch.device(dev.type, torch.cuda.current_device())
    # everything is validated on the host before the first device call
    host = {}
    for i, m in enumerate(masks):
        if torch.is_tensor(m):
            if m.device != dev or m.dtype != torch.uint8 or m.dim() != 2 or not m.is_contiguous() or m.numel() == 0:
                raise ValueError("mask %d: a tensor must be a contiguous uint8 [h, w] on %s, got %s %s on %s"
                                 % (i, dev, m.dtype, tuple(m.shape), m.device))
            hw = int(m.shape[0]) * int(m.shape[1])
        else:
            try:
                host[i] = _masks_u8([m])[0]
            except ValueError as e:
                raise ValueError("mask %d: %s" % (i, str(e).split(": ", 1)[-1])) from None
            hw = host[i].size
        if hw > _lib.CC_MAX_PIXELS:
            raise ValueError("mask %d: %d pixels, at most %d" % (i, hw, _lib.CC_MAX_PIXELS))
    key = str(dev)
    if key not in _CC_DEVICE:
        _CC_DEVICE[key] = _CcDevice(dev)
    cd = _CC_DEVICE[key]
    n = len(masks)
    out: list = [None] * n
    later = []                                     # (device copy of a chunk's results, [(mask index, first element, h, w)])
    with torch.cuda.device(dev):
        stats = torch.empty(n, CC_STATS, dtype=torch.int64, device=dev)
        status = torch.zeros(-(-n // MAX_BATCH), dtype=torch.int32, device=dev)
        for c, s in enumerate(range(0, n, MAX_BATCH)):
            idx = list(range(s, min(s + MAX_BATCH, n)))
            sizes = [tuple(int(v) for v in (host[i].shape if i in host else masks[i].shape)) for i in idx]
            offs, off = {}, 0
            for i in idx:
                if i in host:
                    offs[i] = _Offset(off)
                    off += -(-host[i].size // _ALIGN) * _ALIGN
            up = _staging(dev, "cc").upload([host[i] for i in idx if i in host], [offs[i] for i in idx if i in host], off) if offs else None
            addr = [up.data_ptr() + offs[i].offset if i in host else masks[i].data_ptr() for i in idx]
            base = min(addr)
            nbytes = max(a + h * w for a, (h, w) in zip(addr, sizes)) - base
            descs = cc_descs(sizes, [a - base for a in addr])
            lab = torch.empty(sum(h * w for h, w in sizes), dtype=torch.int32, device=dev) if want_labels else None
            cd.run(base, nbytes, descs, len(idx), connectivity, keep, min_area, stats[s: s + len(idx)].data_ptr(),
                   labels_ptr=None if lab is None else lab.data_ptr())
            status[c: c + 1].copy_(cd.status())
            first, back = 0, []
            for i, (h, w) in zip(idx, sizes):
                if want_labels:
                    if i in host:
                        back.append((i, first, h, w))
                    else:
                        out[i] = lab[first: first + h * w].view(h, w)
                    first += h * w
                elif i in host:
                    back.append((i, offs[i].offset, h, w))
                else:
                    out[i] = masks[i]
            if back:                               # the staging slot is reused two uploads from now: keep a copy of what it holds
                later.append((lab if want_labels else up.clone(), back))
        out_stats = stats.cpu().numpy()            # the one synchronisation
        if int(status.max().item()) != 0:
            raise _lib.CmpcError("%s: cmpc_mask_components reported a loop that reached its bound (status %s): the result is not valid"
                                 % (who, status.cpu().tolist()))
        for t, back in later:
            flat = t.cpu().numpy()
            for i, o, h, w in back:
                got = flat[o: o + h * w].reshape(h, w)
                if want_labels:
                    out[i] = got.copy()
                else:                              # the uploaded copy was {0, 1}: kept pixels keep the caller's values
                    src = np.asarray(masks[i])
                    src = src[:, :, 0] if src.ndim == 3 else src
                    out[i] = np.where(got != 0, src, 0).astype(src.dtype)
    return out, out_stats


def mask_components(masks, connectivity: int = 8, device="cuda:0") -> Tuple[list, np.ndarray]:
    """The connected components of every [h, w] mask (non-zero = foreground; cmpc_mask_components, label-only): (labels, stats).
    labels[i]: int32 [h, w], 0 for background and 1 + the raster index of the component's first pixel for foreground -- a NumPy array
    for a host mask, a device tensor for a device mask; stats: int64 [n, 4] = (n_components, area, area_largest, area_kept = area).
    Host arrays are packed and uploaded; contiguous uint8 device tensors are read in place and not written.  Arguments are validated
    on the host before any device call.  Chunks of MAX_BATCH on the current stream, one synchronisation at the end; raises CmpcError
    if the kernels' status word is set."""
    return _components(masks, connectivity, 0, 0, device, True, "mask_components")


def mask_clean(masks, keep: int = 1, min_area: int = 0, connectivity: int = 8, device="cuda:0") -> Tuple[list, np.ndarray]:
    """Keep the `keep` largest components (0: all) of at least `min_area` pixels of every mask, as hostutil.clean_mask does on the host:
    (cleaned masks, stats int64 [n, 4]).  A host array comes back as a new array (kept pixels keep their value); a contiguous uint8
    device tensor is cleaned IN PLACE and returned.  Validation, chunks and synchronisation as for mask_components."""
    return _components(masks, connectivity, keep, min_area, device, False, "mask_clean")


# ---- pivot frames: cmpc_mask_pool and cmpc_level_agree (include/cmpc.h; hostutil.find_pivot_frames / PivotLog use what they give) ------
_POOL_DT = {torch.float32: _lib.DT_F32, torch.bfloat16: _lib.DT_BF16, torch.float16: _lib.DT_F16}


def check_pool_mode(mode: str) -> str:
    if mode not in _lib.POOL_MODES:
        raise ValueError("describe weights must be 'soft' or 'hard', got %r" % (mode,))
    return mode


def agree_logit(threshold: float) -> float:
    """The logit of a probability threshold, log(t / (1 - t)) in float64 rounded to float32: sigmoid(x) > t as x > logit."""
    t = float(threshold)
    if not 0.0 < t < 1.0:
        raise ValueError("threshold must be a probability in (0, 1), got %r" % (threshold,))
    return float(np.float32(np.log(t / (1.0 - t))))


def pool_workspace(n: int, h: int, w: int, C: int) -> int:
    """cmpc_mask_pool_workspace: n * ceil(h * w / POOL_CHUNK) partial rows of C + 8 floats, in bytes."""
    import ctypes
    out = ctypes.c_int64()
    _lib.call("cmpc_mask_pool_workspace", int(n), int(h), int(w), int(C), ctypes.byref(out))
    return out.value


class _PoolDevice:
    """The device half of describing, shared by mask_pool / level_agree and the two segmenters: both kernels read their inputs where
    they lie and write where they are told, on the current stream.  The workspace grows only when a call needs more than any before
    it (reserve() ahead of the steady state)."""

    def __init__(self, device):
        self.device = torch.device(device)
        self.ws = None
        self._need: Dict[Tuple[int, int, int, int], int] = {}     # sizes asked for so far -> workspace bytes (one library call per size)

    def reserve(self, n: int, h: int, w: int, C: int) -> int:
        key = (int(n), int(h), int(w), int(C))
        need = self._need.get(key)
        if need is None:
            need = self._need[key] = pool_workspace(*key)
        if self.ws is None or self.ws.numel() * 4 < need:
            with torch.cuda.device(self.device):
                self.ws = torch.empty(max(need // 4, 1 << 16), dtype=torch.float32, device=self.device)
        return need

    def pool(self, feat: torch.Tensor, n: int, score_ptr: int, sH: int, sW: int, mode: str, threshold: float, desc_ptr: int, area_ptr: int):
        """feat: [>= n, h, w, C] whose results are contiguous taps (any stride between them); score: float32 [n, sH, sW] at score_ptr."""
        h, w, C = (int(x) for x in feat.shape[1:])
        self.reserve(n, h, w, C)
        stride = int(feat.stride(0)) if feat.shape[0] > 1 else h * w * C
        _lib.call("cmpc_mask_pool", _POOL_DT[feat.dtype], feat.data_ptr(), stride, score_ptr, int(sH), int(sW), int(n), h, w, C,
                  _lib.POOL_MODES[mode], float(threshold), desc_ptr, area_ptr, self.ws.data_ptr(), self.ws.numel() * 4,
                  torch.cuda.current_stream(self.device).cuda_stream)

    def agree(self, a_ptr: int, b_ptr: int, n: int, h: int, w: int, logit: float, counts_ptr: int):
        _lib.call("cmpc_level_agree", a_ptr, b_ptr, int(n), int(h), int(w), float(logit), counts_ptr,
                  torch.cuda.current_stream(self.device).cuda_stream)


_POOL_DEVICE: Dict[str, _PoolDevice] = {}


def _pool_device(dev) -> _PoolDevice:
    key = str(dev)
    if key not in _POOL_DEVICE:
        _POOL_DEVICE[key] = _PoolDevice(dev)
    return _POOL_DEVICE[key]


def _check_tap(feat):
    if not torch.is_tensor(feat) or feat.device.type != "cuda" or feat.dtype not in _POOL_DT or feat.dim() != 4 or feat.numel() == 0:
        raise ValueError("feat must be a float32, float16 or bfloat16 device tensor [n, h, w, C]")
    n, h, w, C = feat.shape
    if C % 8:
        raise ValueError("feat: C = %d is not a multiple of 8" % C)
    if feat.stride()[1:] != (w * C, C, 1) or (n > 1 and (feat.stride(0) < h * w * C or feat.stride(0) % 8)) or feat.data_ptr() % 16:
        raise ValueError("feat: each result must be a contiguous, 16-byte aligned [h, w, C] tap (strides %s)" % (tuple(feat.stride()),))


def mask_pool(feat, score, mode: str = "soft", threshold: float = 0.5) -> Tuple[torch.Tensor, torch.Tensor]:
    """cmpc_mask_pool on device tensors: desc[i, c] = sum_{y, x} wgt_i[y, x] * feat[i, y, x, c] and area[i] = sum wgt_i, with wgt_i the
    point sample score[i, y * (sH / h), x * (sW / w)] (mode "soft") or that float32 >= threshold ? 1 : 0 ("hard").  feat: [n, h, w, C]
    float32 / float16 / bfloat16, each result a contiguous tap (a slice or a strided selection of a batch is read in place); score:
    float32 [n, sH, sW] or [n, sH, sW, 1] on the same device, sH % h == 0 and sW % w == 0.  Runs in chunks of MAX_BATCH on the current
    stream, nothing synchronises.  Returns float32 device tensors (desc [n, C], area [n]).  The partial rows live in ONE workspace per
    device, shared by every call of this function on that device: calls must follow one another on one stream; calls from several host
    threads, or on several streams that may run side by side, would share the rows and must be serialised by the caller (the segmenters
    own a workspace each)."""
    check_pool_mode(mode)
    _check_tap(feat)
    if not torch.is_tensor(score) or score.device != feat.device or score.dtype != torch.float32:
        raise ValueError("score must be a float32 tensor on feat's device")
    if score.dim() == 4 and score.shape[3] == 1:
        score = score[..., 0]
    n, h, w, C = feat.shape
    if score.dim() != 3 or score.shape[0] != n or score.shape[1] % h or score.shape[2] % w or score.shape[1] < h or score.shape[2] < w:
        raise ValueError("score %s against feat %s: [n, sH, sW] with sH, sW multiples of the tap grid" % (tuple(score.shape), tuple(feat.shape)))
    score = score.contiguous()
    dev = feat.device
    pd = _pool_device(dev)
    with torch.cuda.device(dev):
        desc = torch.empty(n, C, dtype=torch.float32, device=dev)
        area = torch.empty(n, dtype=torch.float32, device=dev)
        for s in range(0, n, MAX_BATCH):
            k = min(MAX_BATCH, n - s)
            pd.pool(feat[s: s + k], k, score[s: s + k].data_ptr(), score.shape[1], score.shape[2], mode, threshold,
                    desc[s: s + k].data_ptr(), area[s: s + k].data_ptr())
    return desc, area


def level_agree(a, b, threshold: float = 0.2) -> torch.Tensor:
    """cmpc_level_agree on device tensors: int64 [n, 2] = (I, U), the sizes of (sigmoid(a) > threshold) & (sigmoid(b) > threshold) and of
    their union -- loss.iou_with_threshold (util/loss.py:51-68) as exact integers; hostutil.consistency gives I / U.  a, b: float32 logit
    maps [n, h, w] or [n, h, w, 1] of one shape on one device.  The probability threshold becomes the logit agree_logit(threshold) and
    the maps are compared with it as they are (no exp).  Chunks of MAX_BATCH on the current stream, nothing synchronises."""
    logit = agree_logit(threshold)
    ts = []
    for name, t in (("a", a), ("b", b)):
        if not torch.is_tensor(t) or t.device.type != "cuda" or t.dtype != torch.float32:
            raise ValueError("%s must be a float32 device tensor" % name)
        if t.dim() == 4 and t.shape[3] == 1:
            t = t[..., 0]
        if t.dim() != 3 or t.numel() == 0:
            raise ValueError("%s must be [n, h, w] or [n, h, w, 1], got %s" % (name, tuple(t.shape)))
        ts.append(t.contiguous())
    a, b = ts
    if a.shape != b.shape or a.device != b.device:
        raise ValueError("a %s on %s and b %s on %s: one shape and one device" % (tuple(a.shape), a.device, tuple(b.shape), b.device))
    n, h, w = a.shape
    dev = a.device
    pd = _pool_device(dev)
    with torch.cuda.device(dev):
        counts = torch.empty(n, 2, dtype=torch.int64, device=dev)
        for s in range(0, n, MAX_BATCH):
            k = min(MAX_BATCH, n - s)
            pd.agree(a[s: s + k].data_ptr(), b[s: s + k].data_ptr(), k, h, w, logit, counts[s: s + k].data_ptr())
    return counts


# ---- mask propagation: cmpc_label_propagate and cmpc_prop_fuse (include/cmpc.h; hostutil.propagation_plan says who receives from whom) ----
def prop_workspace(n: int, h: int, w: int) -> int:
    """cmpc_label_propagate_workspace: the inverse norms, n * (1 + PROP_MAX_SOURCES) * h * w floats, in bytes."""
    import ctypes
    out = ctypes.c_int64()
    _lib.call("cmpc_label_propagate_workspace", int(n), int(h), int(w), ctypes.byref(out))
    return out.value


def prop_items(items) -> list:
    """[(target frame, [(source frame, label index), ...]), ...] -> a list of _lib.PropItem.  ValueError for an item without sources
    or with more than PROP_MAX_SOURCES; the indices themselves are checked by the library against the banks."""
    out = []
    for i, it in enumerate(items):
        try:
            tgt, srcs = it
            srcs = [(int(f), int(l)) for f, l in srcs]
        except (TypeError, ValueError):
            raise ValueError("item %d: expected (target frame, [(source frame, label index), ...]), got %r" % (i, it)) from None
        if not 1 <= len(srcs) <= _lib.PROP_MAX_SOURCES:
            raise ValueError("item %d: %d sources, 1..%d are allowed" % (i, len(srcs), _lib.PROP_MAX_SOURCES))
        p = _lib.PropItem()
        p.tgt, p.nsrc = int(tgt), len(srcs)
        for k, (f, l) in enumerate(srcs):
            p.src[k], p.label[k] = f, l
        out.append(p)
    return out


class _PropDevice:
    """The device half of propagating, shared by label_propagate / prop_fuse and FrameSegmenter: both kernels read their inputs where
    they lie and write where they are told, on the current stream.  The workspace grows only when a call needs more than any before
    it (reserve() ahead of the steady state)."""

    def __init__(self, device):
        self.device = torch.device(device)
        self.ws = None

    def reserve(self, n: int, h: int, w: int) -> int:
        need = prop_workspace(n, h, w)
        if self.ws is None or self.ws.numel() * 4 < need:
            with torch.cuda.device(self.device):
                self.ws = torch.empty(max(need // 4, 1 << 16), dtype=torch.float32, device=self.device)
        return need

    def propagate(self, feats: torch.Tensor, labels: torch.Tensor, items: list, radius: int, temperature: float, out_ptr: int, peak_ptr: int):
        """feats: a bank [frames, h, w, C] of contiguous taps (any stride between frames); labels: contiguous float32 [L, h, w];
        items: at most MAX_BATCH _lib.PropItem; out / peak: float32 [len(items), h, w] at out_ptr / peak_ptr (0: no peak)."""
        frames, h, w, C = (int(x) for x in feats.shape)
        n = len(items)
        self.reserve(n, h, w)
        stride = int(feats.stride(0)) if frames > 1 else h * w * C
        arr = (_lib.PropItem * n)(*items)
        _lib.call("cmpc_label_propagate", _POOL_DT[feats.dtype], feats.data_ptr(), stride, frames, labels.data_ptr(), int(labels.shape[0]),
                  arr, n, h, w, C, int(radius), float(temperature), out_ptr, peak_ptr or None, self.ws.data_ptr(), self.ws.numel() * 4,
                  torch.cuda.current_stream(self.device).cuda_stream)

    def fuse(self, own_ptr: int, prop_ptr: int, n: int, h: int, w: int, H: int, W: int, alpha: float, fused_ptr: int):
        _lib.call("cmpc_prop_fuse", own_ptr, prop_ptr, int(n), int(h), int(w), int(H), int(W), float(alpha), fused_ptr,
                  torch.cuda.current_stream(self.device).cuda_stream)


_PROP_DEVICE: Dict[str, _PropDevice] = {}


def _prop_device(dev) -> _PropDevice:
    key = str(dev)
    if key not in _PROP_DEVICE:
        _PROP_DEVICE[key] = _PropDevice(dev)
    return _PROP_DEVICE[key]


def label_propagate(feats, labels, items, radius: int = 12, temperature: float = 0.07, want_peak: bool = False):
    """cmpc_label_propagate on device tensors: every item (target frame, [(source frame, label index), ...]) receives the labels of its
    sources along cosine affinities between the taps, out[i, q] = sum_{s, p} softmax_{s, p}(<a_q, b_p> / temperature) * labels[l_s][p]
    over the positions p within `radius` of q in both directions (radius < 0: the whole grid), a and b the L2-normalised vectors of
    the target and source taps.  feats: a bank [frames, h, w, C] float32 / float16 / bfloat16, each frame a contiguous tap (a strided
    selection is read in place); labels: float32 [L, h, w] on the same device.  Runs in chunks of MAX_BATCH items on the current
    stream, nothing synchronises.  Returns float32 out [n, h, w], or (out, peak) with want_peak: peak[i, q] = the largest cosine among
    q's candidates.  One workspace per device is shared by every call of this function on that device, as in mask_pool."""
    _check_tap(feats)
    if not torch.is_tensor(labels) or labels.device != feats.device or labels.dtype != torch.float32:
        raise ValueError("labels must be a float32 tensor on feats' device")
    frames, h, w, C = feats.shape
    if labels.dim() != 3 or tuple(labels.shape[1:]) != (h, w) or labels.shape[0] < 1:
        raise ValueError("labels %s against feats %s: [L, h, w] at the taps' grid" % (tuple(labels.shape), tuple(feats.shape)))
    items = prop_items(items)
    if not items:
        raise ValueError("label_propagate: no items")
    labels = labels.contiguous()
    dev = feats.device
    pd = _prop_device(dev)
    n = len(items)
    with torch.cuda.device(dev):
        out = torch.empty(n, h, w, dtype=torch.float32, device=dev)
        peak = torch.empty(n, h, w, dtype=torch.float32, device=dev) if want_peak else None
        for s in range(0, n, MAX_BATCH):
            k = min(MAX_BATCH, n - s)
            pd.propagate(feats, labels, items[s: s + k], radius, temperature, out[s: s + k].data_ptr(), peak[s: s + k].data_ptr() if want_peak else 0)
    return (out, peak) if want_peak else out


def prop_fuse(own, prop, alpha: float) -> torch.Tensor:
    """cmpc_prop_fuse on device tensors: (1 - alpha) * own + alpha * U(prop) for own float32 [n, H, W] and prop float32 [n, h, w], U the
    model's legacy bilinear rule (the one that makes `up` from `pred`); alpha in [0, 1], alpha == 0 returns own's bits.  Chunks of
    MAX_BATCH on the current stream, nothing synchronises.  Returns a new float32 tensor [n, H, W]."""
    for name, t in (("own", own), ("prop", prop)):
        if not torch.is_tensor(t) or t.device.type != "cuda" or t.dtype != torch.float32 or t.dim() != 3 or t.numel() == 0:
            raise ValueError("%s must be a float32 device tensor [n, rows, cols]" % name)
    if own.device != prop.device or own.shape[0] != prop.shape[0]:
        raise ValueError("own %s on %s and prop %s on %s: one n and one device" % (tuple(own.shape), own.device, tuple(prop.shape), prop.device))
    own, prop = own.contiguous(), prop.contiguous()
    n, H, W = own.shape
    h, w = prop.shape[1:]
    dev = own.device
    pd = _prop_device(dev)
    with torch.cuda.device(dev):
        fused = torch.empty_like(own)
        for s in range(0, n, MAX_BATCH):
            k = min(MAX_BATCH, n - s)
            pd.fuse(own[s: s + k].data_ptr(), prop[s: s + k].data_ptr(), k, h, w, H, W, alpha, fused[s: s + k].data_ptr())
    return fused


def unpack_masks(buf, descs) -> list:
    """The [h, w] views of a packed mask buffer (device tensor or NumPy array) at its descriptors' offsets."""
    if torch.is_tensor(buf):
        return [buf[d.offset: d.offset + d.h * d.w].view(d.h, d.w) for d in descs]
    return [buf[d.offset: d.offset + d.h * d.w].reshape(d.h, d.w) for d in descs]


def check_gv_norm(mode: Optional[str], allow_none: bool = True) -> Optional[str]:
    if (mode is None and allow_none) or mode in _lib.GV_NORMS:
        return mode
    raise ValueError("gv_norm must be %s'batch' or 'sample', got %r" % ("None, " if allow_none else "", mode))


@contextlib.contextmanager
def gv_norm_scope(model, mode: Optional[str]):
    """The model's gv_lang norm set to `mode` for the forward passes inside, restored afterwards; None leaves the model as it is."""
    if mode is None:
        yield
        return
    prev = model.gv_norm
    model.set_gv_norm(mode)
    try:
        yield
    finally:
        model.set_gv_norm(prev)


def _metrics(iu: np.ndarray, thresholds: Sequence[float]) -> Dict[str, float]:
    # hostutil.SegEval's arithmetic, in sample order
    cum_I = cum_U = 0
    sum_iou = 0.0
    correct = np.zeros(len(thresholds), dtype=np.int64)
    for I, U in iu.tolist():
        iou = float(I) / U
        cum_I += I
        cum_U += U
        sum_iou += iou
        correct += np.array([iou >= t for t in thresholds])
    total = len(iu)
    out = {"precision@%s" % t: float(c) / total for t, c in zip(thresholds, correct)}
    out["overall_IoU"] = cum_I / cum_U
    out["mean_IoU"] = sum_iou / total
    return out


def _check_model(model):
    if getattr(model, "video", False):
        raise ValueError("Evaluator: the video model (CMPC_video_mm_tgraph_allvec) is not supported; its A2D evaluation is out of scope")


def _pad_to(items: list, B: int) -> list:
    return list(items) + [items[0]] * (B - len(items))


def predict_masks(model, ids, seq_len, images, gv_norm: Optional[str] = None) -> List[np.ndarray]:
    """Inference only: the reference's `predicts` (resize_and_crop(up >= 1e-9) at each image's original size) for up to
    model.batch_size samples, as host uint8 {0, 1} arrays.  gv_norm: None leaves the model's gv_lang norm as it is; "sample" / "batch" set
    it for this call and restore it (LSTM_model.set_gv_norm: with "sample" the masks are those of the reference's batch-1 loop, whatever
    the batch holds; with "batch" a sample's mask depends on its batch mates and on the pads of a short batch)."""
    _check_model(model)
    check_gv_norm(gv_norm)
    images = list(images)
    n, B = len(images), model.batch_size
    if n == 0 or n > B:
        raise ValueError("predict_masks: 1..%d samples per call, got %d" % (B, n))
    ids, seq_len = np.asarray(ids, dtype=np.int32).reshape(n, -1), np.asarray(seq_len, dtype=np.int32).reshape(n)
    feed, _ = prepare_images(_pad_to(images, B), model.H, model.W, model.device)
    with gv_norm_scope(model, gv_norm):
        up = model.forward(np.concatenate([ids, np.repeat(ids[:1], B - n, 0)]), feed, np.concatenate([seq_len, np.repeat(seq_len[:1], B - n)]))["up"]
    buf, descs = masks_out(up[:n].float(), [np.asarray(im).shape[:2] for im in images], 1e-9)
    host = buf.cpu().numpy()
    return [mk.copy() for mk in unpack_masks(host, descs)]


def _check_dcrf_method(method: str) -> str:
    if method not in ("exact", "lattice"):
        raise ValueError("dcrf_method must be 'exact' or 'lattice', got %r" % (method,))
    return method


class Evaluator:
    """The `-m test` loop (trainval_model.py:198-303) batched on the GPU.  add() queues one sample (end-padded ids [T], seq_len,
    original-size uint8 image, original-size mask); a batch of model.batch_size samples runs prep -> forward -> mask_iu (and with
    dcrf, DenseCRF on each sample's sigm / proc_im -> mask_iu on the argmax).  result() flushes a partial last batch (padded by
    repeating a sample; pads are never counted) and returns hostutil.SegEval.result()'s keys plus `samples` (and `dcrf_`-prefixed
    metrics with dcrf).  dcrf_method: "exact" (one cmpc_dense_crf call per sample) or "lattice" (the batch's masks from one
    cmpc_dense_crf_lattice call, crf.py).  gv_norm: None leaves the model's gv_lang norm as it is (by default the batch-wide norm of the
    training graph: a sample's (I, U) then depends on its batch mates and on the pads of the last batch); "sample" gives every sample the
    result of the reference's batch-1 `-m test` loop; either value is set around each forward pass and the model's own mode restored.
    visualize: None, or a callable fn(i, pics) -- the driver's `-v` switch (visualize_seg, trainval_model.py:306-330).  Every real sample
    (never a pad) calls it exactly once, in sample order, with pics = {"im", "gt", "pred"} (and "pred_dcrf" with dcrf): uint8 [h, w, 3]
    host arrays, valid during the call; gt and pred are cmpc_vis_overlay's pictures of the ground truth and of the masks
    cmpc_eval_mask_iu writes, on the frames cmpc_eval_prep was given (visualize.EvaluatorPictures).  A batch's pictures are delivered
    once the next batch is enqueued, or by result() / per_sample(); the metrics are the same integers with and without the hook."""

    def __init__(self, model, thresholds: Sequence[float] = (.5, .6, .7, .8, .9), dcrf: bool = False, score_thresh: float = 1e-9,
                 dcrf_method: str = "exact", gv_norm: Optional[str] = None, visualize=None):
        _check_model(model)
        self.gv_norm = check_gv_norm(gv_norm)
        self.model, self.thresholds, self.dcrf, self.score_thresh = model, tuple(thresholds), bool(dcrf), float(score_thresh)
        self.dcrf_method = _check_dcrf_method(dcrf_method)
        self.B, self.H, self.W = model.batch_size, model.H, model.W
        if self.B > MAX_BATCH:
            raise ValueError("Evaluator: model.batch_size %d > %d" % (self.B, MAX_BATCH))
        self.queue = []
        self.n = 0
        self.iu = torch.zeros(64, 2, dtype=torch.int64, device=model.device)
        self.iu_crf = torch.zeros(64, 2, dtype=torch.int64, device=model.device) if self.dcrf else None
        self.pictures = None
        if visualize is not None:
            if not callable(visualize):
                raise ValueError("Evaluator: visualize must be None or a callable fn(i, pics)")
            from . import visualize as VIS
            self.pictures = VIS.EvaluatorPictures(visualize, model.device)

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
            feed, proc, src, src_descs, src_bytes = _prepare_images([s[2] for s in q], self.H, self.W, m.device)
            with gv_norm_scope(m, self.gv_norm):
                out = m.forward(ids, feed, sl)
            gts = [s[3] for s in q[:n]]
            self._grow(self.n + n)
            pic = self.pictures
            if pic is None:
                mask_iu(out["up"][:n].float(), gts, self.score_thresh, out=self.iu[self.n: self.n + n])
            else:
                _, mo, descs, nbytes, gt_dev = _mask_iu(out["up"][:n].float(), gts, self.score_thresh, True, self.iu[self.n: self.n + n])
                pic.begin(self.n, [s[2] for s in q[:n]], src, src_descs, src_bytes, descs, nbytes)
                pic.overlay("gt", gt_dev)
                pic.overlay("pred", mo)
            if self.dcrf:
                from . import crf
                sigm = out["sigm"].float()
                if self.dcrf_method == "lattice":
                    crf_masks = crf.dense_crf_batch(sigm[:n].reshape(n, self.H, self.W), proc[:n], device=m.device, method="lattice")
                else:
                    crf_masks = torch.stack([crf.dense_crf_mask(sigm[b].reshape(self.H, self.W), proc[b], device=m.device) for b in range(n)])
                if pic is None:
                    mask_iu(crf_masks, gts, 0.5, out=self.iu_crf[self.n: self.n + n])
                else:
                    pic.overlay("pred_dcrf", _mask_iu(crf_masks, gts, 0.5, True, self.iu_crf[self.n: self.n + n])[1])
            if pic is not None:
                pic.end()
        self.n += n

    def _metrics(self, iu: np.ndarray) -> Dict[str, float]:
        return _metrics(iu, self.thresholds)

    def _flush(self):
        self._run()
        if self.pictures is not None:
            self.pictures.flush()

    def per_sample(self) -> np.ndarray:
        """(I, U) of every sample added so far (flushes the partial batch), int64 [n, 2]."""
        self._flush()
        return self.iu[: self.n].cpu().numpy()

    def result(self) -> Dict[str, float]:
        self._flush()
        if self.n == 0:
            raise ValueError("Evaluator.result: no samples")
        iu = self.iu[: self.n].cpu().numpy()
        out = self._metrics(iu)
        out["samples"] = self.n
        if self.dcrf:
            out.update({"dcrf_" + k: v for k, v in self._metrics(self.iu_crf[: self.n].cpu().numpy()).items()})
        return out


# ---- CMPC_video_mm_tgraph_allvec on an A2D split (CMPC_video/trainval_video.py:136-291) --------------------------------------------------
VIDEO_THRESHOLDS = (.5, .55, .6, .65, .7, .75, .8, .85, .9, .95)        # trainval_video.py:147
VIDEO_OVERLAP = False          # VideoEvaluator(overlap=None): on one MI355X the overlap was 2-4 % slower


def check_video_sample(i: int, text, image, frames, gt_mask, T: int, n_frames: int):
    """add()'s validation of one A2D test sample as build_A2D_batches.py:137-143 stores it (text_batch, im_batch, frames, mask_batch).
    Raises ValueError naming sample `i`; returns (END-padded ids int32 [1, T], seq_len int32 [1], the FRAME_IDX frames, the key image,
    the mask as uint8 {0, 1})."""
    from .model import FRAME_IDX, video_words
    t = np.asarray(text)
    if t.ndim != 1 or t.shape[0] != T or not np.issubdtype(t.dtype, np.integer):
        raise ValueError("sample %d: text must be integer ids [%d], got %s %s" % (i, T, t.dtype, t.shape))
    if not np.any(t != 0):
        raise ValueError("sample %d: the sentence holds only pad ids (the model needs at least one word)" % i)
    try:
        we, sl = video_words(t, HU.first_valid_idx(t), T)
    except ValueError as e:
        raise ValueError("sample %d: %s" % (i, e)) from None
    fr = list(frames) if isinstance(frames, (list, tuple)) or (isinstance(frames, np.ndarray) and frames.dtype == object) else None
    if fr is None:
        fa = np.asarray(frames)
        if fa.ndim != 4:
            raise ValueError("sample %d: frames must be [%d, h, w, 3], got %s" % (i, n_frames, fa.shape))
        fr = list(fa)
    if len(fr) != n_frames:
        raise ValueError("sample %d: %d frames, the model takes %d" % (i, len(fr), n_frames))
    fr = [np.asarray(f) for f in fr]
    for k, f in enumerate(fr):
        if f.dtype != np.uint8:
            raise ValueError("sample %d: frame %d is %s, expected uint8" % (i, k, f.dtype))
        if f.shape != fr[0].shape:
            raise ValueError("sample %d: frame %d is %s, frame 0 %s (a clip's frames share one size)" % (i, k, f.shape, fr[0].shape))
    if fr[0].ndim != 3 or fr[0].shape[2] != 3 or fr[0].shape[0] == 0 or fr[0].shape[1] == 0:
        raise ValueError("sample %d: frames must be [h, w, 3] with h, w > 0, got %s" % (i, fr[0].shape))
    im = np.asarray(image)
    if im.dtype != np.uint8:
        raise ValueError("sample %d: the key image is %s, expected uint8" % (i, im.dtype))
    if im.ndim not in (2, 3) or (im.ndim == 3 and im.shape[2] not in (1, 3)) or im.shape[0] == 0 or im.shape[1] == 0:
        raise ValueError("sample %d: the key image must be [h, w] or [h, w, 1|3] with h, w > 0, got %s" % (i, im.shape))
    m = np.asarray(gt_mask)
    if m.ndim == 3 and m.shape[2] == 1:
        m = m[:, :, 0]
    if m.shape != im.shape[:2]:
        raise ValueError("sample %d: mask %s, key image %s (the mask is at the key image's size)" % (i, m.shape, im.shape[:2]))
    m = np.ascontiguousarray(m != 0).view(np.uint8)
    if not m.any():
        raise ValueError("sample %d: empty mask (U would be 0; build_A2D_batches.py:98 drops these)" % i)
    return we, sl, [np.ascontiguousarray(fr[k]) for k in FRAME_IDX], np.ascontiguousarray(im), m


class VideoEvaluator:
    """The video driver's `-m test` loop (trainval_video.py:186-291) on the GPU, one clip per forward pass (the graph is batch 1).
    add(text, image, frames, gt_mask) takes one sample of build_A2D_batches.py's .npz files as it is stored: FRONT-padded ids [T], the
    key image, the [frames, h, w, 3] uint8 clip and the mask at the key image's size.  Per clip, one pinned upload carries the 5 sampled
    frames (plus the key image with dcrf) and the END-padded ids; one cmpc_eval_prep launch resizes them, forward_video_frames' path runs
    the model on the device feed, cmpc_eval_mask_iu counts I and U of resize_and_crop(up >= score_thresh) at the mask's size (with dcrf,
    also of DenseCRF on sigm with the key image's proc_im, :227-240).  (I, U) stay on the device until result() / per_sample(); nothing
    synchronises between clips.  overlap=True enqueues clip n+1's upload, prep and backbone on the backbone stream before clip n's
    head (off by default: DESIGN.md §13b); results are bit-identical either way.  dcrf_method as in Evaluator (one key image per
    clip: one call either way)."""

    def __init__(self, model, thresholds: Sequence[float] = VIDEO_THRESHOLDS, dcrf: bool = False, score_thresh: float = 1e-9,
                 overlap: bool = None, dcrf_method: str = "exact"):
        if not getattr(model, "video", False):
            raise ValueError("VideoEvaluator: expects the video model (CMPC_video_mm_tgraph_allvec); use Evaluator for the image models")
        self.model, self.thresholds, self.dcrf, self.score_thresh = model, tuple(thresholds), bool(dcrf), float(score_thresh)
        self.dcrf_method = _check_dcrf_method(dcrf_method)
        self.overlap = VIDEO_OVERLAP if overlap is None else bool(overlap)
        self.T, self.H, self.W = model.num_steps, model.H, model.W
        self.n = 0
        self.iu = torch.zeros(64, 2, dtype=torch.int64, device=model.device)
        self.iu_crf = torch.zeros(64, 2, dtype=torch.int64, device=model.device) if self.dcrf else None
        self.staging = None
        self.pending = None            # overlap: the clip whose head is enqueued by the next add() or the flush

    def _grow(self, need: int):
        if need > self.iu.shape[0]:
            cap = max(need, 2 * self.iu.shape[0])
            dev = self.iu.device
            self.iu = torch.cat([self.iu, torch.zeros(cap - self.iu.shape[0], 2, dtype=torch.int64, device=dev)])
            if self.dcrf:
                self.iu_crf = torch.cat([self.iu_crf, torch.zeros(cap - self.iu_crf.shape[0], 2, dtype=torch.int64, device=dev)])

    def _stage(self, we, sl, frames, image):
        """One upload of [5 frames (+ key image)] ‖ ids ‖ seq_len and one cmpc_eval_prep launch over the images, on the current stream.
        Returns (feed [5|6, H, W, 3] f32, proc_im [5|6, H, W, 3] u8, ids [1, T] i32, seq_len [1] i32), all on the device."""
        m = self.model
        ims = _images_u8(frames + ([image] if self.dcrf else []))
        descs, img_bytes = plan_prep([a.shape for a in ims], self.H, self.W)
        ids_off = img_bytes
        sl_off = ids_off + -(-we.nbytes // _ALIGN) * _ALIGN
        nbytes = sl_off + _ALIGN
        offs = list(descs) + [_Offset(ids_off), _Offset(sl_off)]
        if self.staging is None:
            self.staging = _Staging(m.device)
        dev = self.staging.upload(ims + [we.view(np.uint8), sl.view(np.uint8)], offs, nbytes)
        B = len(ims)
        proc = torch.empty(B, self.H, self.W, 3, dtype=torch.uint8, device=m.device)
        feed = torch.empty(B, self.H, self.W, 3, dtype=torch.float32, device=m.device)
        _lib.call("cmpc_eval_prep", dev.data_ptr(), img_bytes, descs, B, self.H, self.W, proc.data_ptr(), feed.data_ptr(),
                  torch.cuda.current_stream(m.device).cuda_stream)
        ids = dev[ids_off: ids_off + we.nbytes].view(torch.int32).view(1, self.T)
        seq = dev[sl_off: sl_off + 4].view(torch.int32)
        return feed, proc, ids, seq

    def add(self, text, image, frames, gt_mask):
        m = self.model
        we, sl, fr, im, gt = check_video_sample(self.n, text, image, frames, gt_mask, self.T, m.frames)
        with torch.no_grad(), torch.cuda.device(m.device):
            main = torch.cuda.current_stream(m.device)
            if self.overlap and m.bb_stream is not None:
                bb = m.bb_stream
                bb.wait_stream(main)              # the head that last read this staging slot's ids, and the taps of this backbone slot
                with torch.cuda.stream(bb):
                    feed, proc, ids, seq = self._stage(we, sl, fr, im)
                    ready = torch.cuda.Event()
                    ready.record(bb)
                proc.record_stream(main)
                feats, done = m.features_async(feed[:len(fr)], ready=ready)
                clip = (feats, done, ids, seq, proc, gt, self.n)
                self._head(self.pending)
                self.pending = clip
            else:
                feed, proc, ids, seq = self._stage(we, sl, fr, im)
                feats, done = m.features_async(feed[:len(fr)])
                self._head((feats, done, ids, seq, proc, gt, self.n))
        self.n += 1

    def _head(self, clip):
        if clip is None:
            return
        feats, done, ids, seq, proc, gt, i = clip
        m = self.model
        out = m._video_fetch(feats, done, ids, seq)
        self._grow(i + 1)
        mask_iu(out["up"].float(), [gt], self.score_thresh, out=self.iu[i: i + 1])
        if self.dcrf:
            from . import crf
            key = crf.dense_crf_mask(out["sigm"].float().reshape(self.H, self.W), proc[-1], device=m.device, method=self.dcrf_method)
            mask_iu(key[None], [gt], 0.5, out=self.iu_crf[i: i + 1])

    def _flush(self):
        clip, self.pending = self.pending, None
        with torch.no_grad(), torch.cuda.device(self.model.device):
            self._head(clip)

    def per_sample(self) -> np.ndarray:
        """(I, U) of every clip added so far, int64 [n, 2]."""
        self._flush()
        return self.iu[: self.n].cpu().numpy()

    def result(self) -> Dict[str, float]:
        """Evaluator.result()'s keys (precision@t for the ten thresholds, overall_IoU, mean_IoU, samples, dcrf_* with dcrf)."""
        self._flush()
        if self.n == 0:
            raise ValueError("VideoEvaluator.result: no samples")
        out = _metrics(self.iu[: self.n].cpu().numpy(), self.thresholds)
        out["samples"] = self.n
        if self.dcrf:
            out.update({"dcrf_" + k: v for k, v in _metrics(self.iu_crf[: self.n].cpu().numpy(), self.thresholds).items()})
        return out


class _Offset:
    """A staging entry that is not an image (the ids, the length): only its offset."""
    __slots__ = ("offset",)

    def __init__(self, offset: int):
        self.offset = offset
