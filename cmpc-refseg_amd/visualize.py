"""The drivers' pictures on the GPU: what `-v` (visualize_seg, trainval_model.py:306-330; CMPC_video/trainval_video.py), the figure scripts
test_visualize_fusion*.py (:283-304) and test_visualize_graph.py (:267-274) draw, from tensors that are already on the device.

    buf, descs = overlays(frames, masks, "pred")              # (im0 >> 1) + 100 m, im1 >> 1, im2 >> 1      (cmpc_vis_overlay)
    buf, descs = overlays(None, gt_masks, "gt")               # (170 m, 0, 170 (1 - m))
    buf, descs = heat_maps(out["up_c3"], sizes, sigmoid=True) # lut[idx] of resize_and_crop(sigmoid(map)) at each frame's size (cmpc_vis_heat)
    sheets = word_sheets(out["gw_v_c5"], seq_len, (h, w))     # one panel per word                           (cmpc_vis_words)
    pictures = unpack_pictures(buf.cpu().numpy(), descs)

Everything is enqueued on the current stream and nothing synchronises: the caller decides when to read back.  Masks are 0 / non-zero
masks (m = mask != 0), the package's "resampled value > 0" decision (evaluate.masks_out's docstring), not the driver's
.astype('uint8') of a fractional map.  The colour index is idx = clip(floor((v - lo) / (hi - lo) * 256), 0, 255) in float64 (0 when
hi == lo) on the array's own pixels; matplotlib's imshow resamples to screen pixels and lays out a figure, so parity with its image
pipeline is UNPINNED.  Text on pictures, figure layout and writing files are left to the caller (examples/visualize_split.py).
"""
from __future__ import annotations

import ctypes
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib, evaluate as EV

MAX_BATCH = _lib.EVAL_MAX_BATCH
_ALIGN = 16
KINDS = {"pred": _lib.VIS_PRED, "gt": _lib.VIS_GT}

# matplotlib's `jet` as (x, y) knots of its piecewise-linear channels (_cm.py's _jet_data, y0 == y1 at every knot)
_JET = {"red": ((0., 0.), (0.35, 0.), (0.66, 1.), (0.89, 1.), (1., 0.5)),
        "green": ((0., 0.), (0.125, 0.), (0.375, 1.), (0.64, 1.), (0.91, 0.), (1., 0.)),
        "blue": ((0., 0.5), (0.11, 1.), (0.34, 1.), (0.65, 0.), (1., 0.))}


def jet_lut() -> np.ndarray:
    """uint8 [256, 3]: `jet` sampled at linspace(0, 1, 256), times 255 and TRUNCATED -- matplotlib 3.10's jet(arange(256), bytes=True)."""
    x = np.linspace(0.0, 1.0, 256)
    out = np.empty((256, 3), np.uint8)
    for c, name in enumerate(("red", "green", "blue")):
        k = np.array(_JET[name])
        out[:, c] = (np.interp(x, k[:, 0], k[:, 1]) * 255).astype(np.uint8)
    return out


def gray_lut() -> np.ndarray:
    """uint8 [256, 3]: index i -> (i, i, i)."""
    return np.repeat(np.arange(256, dtype=np.uint8)[:, None], 3, 1)


_LUTS: Dict[Tuple[str, str], torch.Tensor] = {}


def _lut_on(lut, dev) -> torch.Tensor:
    if lut is None:
        key = (str(dev), "jet")
        if key not in _LUTS:
            _LUTS[key] = torch.from_numpy(jet_lut()).to(dev)
        return _LUTS[key]
    if torch.is_tensor(lut):
        t = lut
    else:
        a = np.asarray(lut)
        if a.dtype != np.uint8:
            raise ValueError("lut must be uint8 [256, 3], got %s" % a.dtype)
        t = torch.from_numpy(np.ascontiguousarray(a))
    if t.dtype != torch.uint8 or tuple(t.shape) != (256, 3):
        raise ValueError("lut must be uint8 [256, 3], got %s %s" % (t.dtype, tuple(t.shape)))
    return t.to(dev).contiguous()


def plan_pictures(sizes: Sequence[Tuple[int, int]], channels: int = 3):
    """Descriptors (offset, h, w, c at 16-byte aligned offsets) and packed length of [h, w, channels] uint8 pictures."""
    EV._check_batch(len(sizes))
    d = (_lib.EvalDesc * len(sizes))()
    off = 0
    for i, s in enumerate(sizes):
        h, w = int(s[0]), int(s[1])
        d[i] = _lib.EvalDesc(off, h, w, channels, 0, 0, 0, 0, 0)
        off += -(-h * w * channels // _ALIGN) * _ALIGN
    return d, off


def _plan_frames(shapes):
    EV._check_batch(len(shapes))
    d = (_lib.EvalDesc * len(shapes))()
    off = 0
    for i, s in enumerate(shapes):
        h, w = int(s[0]), int(s[1])
        c = int(s[2]) if len(s) == 3 else 1
        d[i] = _lib.EvalDesc(off, h, w, c, 0, 0, 0, 0, 0)
        off += -(-h * w * c // _ALIGN) * _ALIGN
    return d, off


def unpack_pictures(buf, descs) -> list:
    """The [h, w, c] (c > 1) or [h, w] views of a packed picture buffer (device tensor or NumPy array) at its descriptors' offsets."""
    out = []
    for d in descs:
        shape = (d.h, d.w, d.c) if d.c > 1 else (d.h, d.w)
        flat = buf[d.offset: d.offset + d.h * d.w * d.c]
        out.append(flat.view(*shape) if torch.is_tensor(buf) else flat.reshape(shape))
    return out


def _device(device) -> torch.device:
    dev = torch.device(device)
    return torch.device(dev.type, torch.cuda.current_device()) if dev.index is None else dev


def _overlay_call(kind: int, frames_ptr, frame_bytes: int, fdescs, masks_ptr: int, mask_bytes: int, mdescs, n: int, out_ptr: int,
                  out_bytes: int, odescs, dev):
    _lib.call("cmpc_vis_overlay", kind, frames_ptr, frame_bytes, fdescs, masks_ptr, mask_bytes, mdescs, n, out_ptr, out_bytes, odescs,
              torch.cuda.current_stream(dev).cuda_stream)


def overlays(frames, masks, kind: str = "pred", device="cuda:0", out: torch.Tensor = None):
    """The `-v` pictures of up to MAX_BATCH samples (cmpc_vis_overlay).  kind "pred": (im0 >> 1) + 100 m, im1 >> 1, im2 >> 1 of host uint8
    frames [h, w, 3] or [h, w] (grey: tiled to three channels); kind "gt": (170 m, 0, 170 (1 - m)), frames are not read and may be None.
    masks, m = mask != 0, each of its frame's size: host arrays, contiguous uint8 device tensors (what mask_iu(want_masks=True) and the
    segmenters yield), or a (buf, descs) pair from masks_out.  Returns (buf, descs): a flat uint8 device buffer (`out` when given) and
    the descriptors that locate sample b's [h, w, 3] picture in it (unpack_pictures).  Bytes between the pictures are not written."""
    if kind not in KINDS:
        raise ValueError("kind must be 'pred' or 'gt', got %r" % (kind,))
    dev = _device(device)
    with torch.cuda.device(dev):
        if isinstance(masks, tuple) and len(masks) == 2 and torch.is_tensor(masks[0]):
            mbuf, md = masks
            if mbuf.device != dev or mbuf.dtype != torch.uint8 or mbuf.dim() != 1 or not mbuf.is_contiguous():
                raise ValueError("masks: a (buf, descs) pair needs a flat contiguous uint8 buffer on %s" % dev)
            n = len(md)
            EV._check_batch(n)
            mdescs = (_lib.EvalDesc * n)(*[_lib.EvalDesc(d.offset, d.h, d.w, 1, 0, 0, 0, 0, 0) for d in md])
            mptr, mbytes = mbuf.data_ptr(), mbuf.numel()
        else:
            masks = list(masks)
            n = len(masks)
            EV._check_batch(n)
            sizes, addr = EV._mask_addresses(masks, 0, dev, "vis_mask")
            mptr = min(addr)
            mdescs = (_lib.EvalDesc * n)(*[_lib.EvalDesc(a - mptr, h, w, 1, 0, 0, 0, 0, 0) for a, (h, w) in zip(addr, sizes)])
            mbytes = max(a + h * w for a, (h, w) in zip(addr, sizes)) - mptr
        sizes = [(d.h, d.w) for d in mdescs]
        fptr, fbytes, fdescs = None, 0, None
        if kind == "pred":
            if frames is None or len(frames) != n:
                raise ValueError("overlays: %d masks for %s frames" % (n, "no" if frames is None else len(frames)))
            ims = EV._images_u8(frames)
            for i, (a, s) in enumerate(zip(ims, sizes)):
                if a.shape[:2] != s:
                    raise ValueError("overlays: sample %d: frame %s, mask %s" % (i, a.shape[:2], s))
            fdescs, fbytes = _plan_frames([a.shape for a in ims])
            fptr = EV._staging(dev, "vis_im").upload(ims, fdescs, fbytes).data_ptr()
        odescs, obytes = plan_pictures(sizes)
        buf = out if out is not None else torch.empty(obytes, dtype=torch.uint8, device=dev)
        if buf.dtype != torch.uint8 or buf.dim() != 1 or buf.numel() < obytes or not buf.is_contiguous() or buf.device != dev:
            raise ValueError("out must be a contiguous uint8 device buffer of at least %d bytes" % obytes)
        _overlay_call(KINDS[kind], fptr, fbytes, fdescs, mptr, mbytes, mdescs, n, buf.data_ptr(), buf.numel(), odescs, dev)
    return buf, odescs


def heat_workspace(B: int, flags: int) -> int:
    """cmpc_vis_heat_workspace: 16 bytes per sample with the AUTO flag, else 0."""
    out = ctypes.c_int64()
    _lib.call("cmpc_vis_heat_workspace", B, flags, ctypes.byref(out))
    return out.value


def heat_maps(score_map, sizes: Sequence[Tuple[int, int]], sigmoid: bool = False, vrange: Optional[Tuple[float, float]] = (0.0, 1.0),
              lut=None, want: str = "rgb", range_out: torch.Tensor = None):
    """Colour-mapped maps at any output sizes (cmpc_vis_heat): v = resize_and_crop(s, oh, ow) in float64 for s = score_map[b] (float32
    device tensor [B, H, W] or [B, H, W, 1]; with sigmoid its float32 sigmoid -- the figure scripts' sigmoid(up_c3 | up_c4 | up_c5 | sigm)),
    idx by the module's rule with (lo, hi) = vrange, or with vrange None each sample's own min and max (imshow's autoscale).  lut: uint8
    [256, 3] (host array or device tensor), default jet_lut().  want "rgb": (buf, descs) of packed [oh, ow, 3] pictures lut[idx];
    "index": (buf, descs) of packed [oh, ow] index planes; "both": the two pairs, rgb first.  range_out: a float64 [B, 2] device tensor
    that receives the (lo, hi) used.  unpack_pictures gives the views."""
    if want not in ("rgb", "index", "both"):
        raise ValueError("want must be 'rgb', 'index' or 'both', got %r" % (want,))
    m = score_map
    if not torch.is_tensor(m) or m.device.type != "cuda" or m.dtype != torch.float32:
        raise ValueError("score_map must be a float32 device tensor")
    if m.dim() == 4 and m.shape[3] == 1:
        m = m[..., 0]
    if m.dim() != 3:
        raise ValueError("score_map must be [B, H, W] or [B, H, W, 1], got %s" % (tuple(m.shape),))
    m = m.contiguous()
    B, H, W = m.shape
    if len(sizes) != B:
        raise ValueError("%d sizes for a batch of %d maps" % (len(sizes), B))
    flags = (_lib.VIS_SIGMOID if sigmoid else 0) | (_lib.VIS_AUTO if vrange is None else 0)
    lo, hi = (0.0, 1.0) if vrange is None else (float(vrange[0]), float(vrange[1]))
    if not lo < hi:
        raise ValueError("vrange must be (vmin, vmax) with vmin < vmax, or None; got %r" % (vrange,))
    idescs, ibytes = EV.plan_masks(sizes, H, W)
    dev = m.device
    with torch.cuda.device(dev):
        rdescs = rgb = idx = None
        rbytes = 0
        if want in ("rgb", "both"):
            rdescs, rbytes = plan_pictures(sizes)
            rgb = torch.empty(rbytes, dtype=torch.uint8, device=dev)
        if want in ("index", "both"):
            idx = torch.empty(ibytes, dtype=torch.uint8, device=dev)
        table = _lut_on(lut, dev) if rgb is not None else None
        if range_out is not None and (tuple(range_out.shape) != (B, 2) or range_out.dtype != torch.float64 or not range_out.is_contiguous()
                                      or range_out.device != dev):
            raise ValueError("range_out must be a contiguous float64 [B, 2] tensor on %s" % dev)
        wsb = heat_workspace(B, flags)
        ws = torch.empty(wsb // 8, dtype=torch.int64, device=dev) if wsb else None
        _lib.call("cmpc_vis_heat", m.data_ptr(), B, H, W, idescs, flags, lo, hi, table.data_ptr() if table is not None else None,
                  idx.data_ptr() if idx is not None else None, ibytes, rgb.data_ptr() if rgb is not None else None, rbytes, rdescs,
                  range_out.data_ptr() if range_out is not None else None, ws.data_ptr() if ws is not None else None, wsb,
                  torch.cuda.current_stream(dev).cuda_stream)
    if want == "rgb":
        return rgb, rdescs
    if want == "index":
        return idx, idescs
    return (rgb, rdescs), (idx, idescs)


def sheet_size(grid: Tuple[int, int], max_words: int, zoom: int = 4, cols: int = 5, gap: int = 2) -> Tuple[int, int]:
    """(height, width) of a word sheet: ceil(max_words / cols) rows of cols panels of grid * zoom pixels, `gap` pixels between panels."""
    rows = -(-int(max_words) // int(cols))
    return rows * grid[0] * zoom + (rows - 1) * gap, cols * grid[1] * zoom + (cols - 1) * gap


def word_sheets(gw_v, n_words, grid: Tuple[int, int], zoom: int = 4, cols: int = 5, gap: int = 2, lut=None, max_words: Optional[int] = None):
    """test_visualize_graph.py's panels (cmpc_vis_words): gw_v float32 device tensor [B, N, ld] (the gw_v_<level> fetch, N = grid[0] *
    grid[1], ld = the padded sentence length), n_words[b] panels per sample (its seq_len; at most min(ld, 32)).  Panel t is
    gw_v[b, :, t] as `grid`, indexed with its own min and max and drawn zoom x zoom pixels per cell; the sheet holds
    ceil(max_words / cols) rows of cols panels `gap` pixels apart (max_words: default max(n_words), so all sheets share one size);
    gaps and unused panels are white.  Returns a uint8 device tensor [B, sheet_h, sheet_w, 3]."""
    g = gw_v
    if not torch.is_tensor(g) or g.device.type != "cuda" or g.dim() != 3:
        raise ValueError("gw_v must be a device tensor [B, N, ld]")
    g = g.float().contiguous()
    B, N, ld = g.shape
    gh, gw = int(grid[0]), int(grid[1])
    nw = [int(v) for v in np.asarray(n_words).reshape(-1)]
    if B < 1 or B > MAX_BATCH or len(nw) != B or gh < 1 or gw < 1 or gh * gw != N:
        raise ValueError("word_sheets: gw_v %s, %d word counts, grid %s (1..%d samples, N = grid[0] * grid[1])" % (tuple(g.shape), len(nw), (gh, gw), MAX_BATCH))
    mw = max(max(nw), 1) if max_words is None else int(max_words)
    if mw < 1 or mw > 32 or any(v < 0 or v > min(ld, mw) for v in nw):
        raise ValueError("word_sheets: n_words %s must lie in 0..min(ld = %d, max_words = %d), max_words in 1..32" % (nw, ld, mw))
    if zoom < 1 or cols < 1 or gap < 0:
        raise ValueError("word_sheets: zoom %r >= 1, cols %r >= 1, gap %r >= 0" % (zoom, cols, gap))
    sh, sw = sheet_size((gh, gw), mw, zoom, cols, gap)
    dev = g.device
    with torch.cuda.device(dev):
        out = torch.empty(B, sh, sw, 3, dtype=torch.uint8, device=dev)
        _lib.call("cmpc_vis_words", g.data_ptr(), B, gh, gw, ld, (ctypes.c_int * B)(*nw), mw, int(zoom), int(cols), int(gap),
                  _lut_on(lut, dev).data_ptr(), out.data_ptr(), out.numel(), torch.cuda.current_stream(dev).cuda_stream)
    return out


def _rgb_frame(a: np.ndarray) -> np.ndarray:
    return a if a.ndim == 3 and a.shape[2] == 3 else np.repeat(a.reshape(a.shape[0], a.shape[1], 1), 3, 2)       # build_batches.py:67-68


class EvaluatorPictures:
    """Evaluator(visualize=fn)'s device half.  Per batch cmpc_vis_overlay draws "gt" and "pred" (and "pred_dcrf") from the ground truths
    cmpc_eval_mask_iu was given, the masks it wrote and the frames cmpc_eval_prep read -- the packed source images are still in their
    staging slot, so nothing goes up a second time -- and one copy per picture plane brings them to one of two pinned host buffers
    (3 h w bytes per picture: 2.7 MB at 720 x 1280) on a copy stream of the hook's own.  Nothing waits for those copies when they are
    enqueued: batch n's pictures are handed to fn after batch n + 1 has been enqueued, or by flush()."""

    def __init__(self, fn, device):
        self.fn, self.device = fn, torch.device(device)
        self.host: List[Optional[torch.Tensor]] = [None, None]
        self.k = 0
        self.copy_stream = None
        self.cur = None
        self.pending = None
        self.bytes_read_back = 0

    def begin(self, first: int, frames, src: torch.Tensor, src_descs, src_bytes: int, mask_descs, mask_bytes: int):
        """frames: the n real samples' host images (handed to fn as "im"); src / src_descs / src_bytes: evaluate._prepare_images' packed
        device copy of the batch (pads behind the real samples); mask_descs / mask_bytes: cmpc_eval_mask_iu's descriptors."""
        ims = EV._images_u8(frames)
        n = len(ims)
        for i, (a, d) in enumerate(zip(ims, mask_descs)):
            if a.shape[:2] != (d.h, d.w):
                raise ValueError("Evaluator(visualize=...): sample %d: image %s, mask %s" % (first + i, a.shape[:2], (d.h, d.w)))
        fdescs = (_lib.EvalDesc * n)(*[_lib.EvalDesc(d.offset, d.h, d.w, d.c, 0, 0, 0, 0, 0) for d in list(src_descs)[:n]])
        odescs, obytes = plan_pictures([(d.h, d.w) for d in mask_descs][:n])
        mdescs = (_lib.EvalDesc * n)(*[_lib.EvalDesc(d.offset, d.h, d.w, 1, 0, 0, 0, 0, 0) for d in list(mask_descs)[:n]])
        self.cur = dict(first=first, ims=ims, n=n, fdescs=fdescs, fbytes=src_bytes, src=src, odescs=odescs, obytes=obytes, mdescs=mdescs,
                        mbytes=mask_bytes, names=[], planes=[])

    def overlay(self, name: str, masks: torch.Tensor):
        c = self.cur
        plane = torch.empty(c["obytes"], dtype=torch.uint8, device=self.device)
        pred = name != "gt"
        _overlay_call(_lib.VIS_PRED if pred else _lib.VIS_GT, c["src"].data_ptr() if pred else None, c["fbytes"] if pred else 0,
                      c["fdescs"] if pred else None, masks.data_ptr(), c["mbytes"], c["mdescs"], c["n"], plane.data_ptr(), c["obytes"],
                      c["odescs"], self.device)
        c["names"].append(name)
        c["planes"].append(plane)

    def end(self):
        c, self.cur = self.cur, None
        k, self.k = self.k, 1 - self.k
        total = c["obytes"] * len(c["planes"])
        if self.host[k] is None or self.host[k].numel() < total:
            self.host[k] = torch.empty(max(total, 1 << 20), dtype=torch.uint8, pin_memory=True)
        # the copies run on a stream of their own behind this batch's overlays, beside the next batch's forward pass
        main = torch.cuda.current_stream(self.device)
        if self.copy_stream is None:
            self.copy_stream = torch.cuda.Stream(self.device)
        self.copy_stream.wait_stream(main)
        with torch.cuda.stream(self.copy_stream):
            for j, plane in enumerate(c["planes"]):
                self.host[k][j * c["obytes"]: (j + 1) * c["obytes"]].copy_(plane, non_blocking=True)
                plane.record_stream(self.copy_stream)
            ev = torch.cuda.Event()
            ev.record(self.copy_stream)
        self.bytes_read_back += total
        prev, self.pending = self.pending, (ev, self.host[k], c)
        self._deliver(prev)

    def _deliver(self, item):
        if item is None:
            return
        ev, host, c = item
        ev.synchronize()
        hv = host.numpy()
        ob = c["obytes"]
        planes = [unpack_pictures(hv[j * ob: (j + 1) * ob], c["odescs"]) for j in range(len(c["names"]))]
        for b in range(c["n"]):
            pics = {"im": _rgb_frame(c["ims"][b])}
            for name, pl in zip(c["names"], planes):
                pics[name] = pl[b]
            self.fn(c["first"] + b, pics)

    def flush(self):
        item, self.pending = self.pending, None
        self._deliver(item)
