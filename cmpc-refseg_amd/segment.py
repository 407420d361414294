"""Segment a video per referring expression: the reference's Refer-YouTube-VOS prediction loop (test.py:250-329) on the GPU, and, for the
video model, the video driver's per-clip prediction over every frame of a video (ClipSegmenter, at the end of this file).

For every video test.py runs every expression over every frame, one sample per sess.run on a batch-1 graph, and writes one mask per
(expression, frame) at half the frame's size.  Here

    seg = FrameSegmenter(model, vocab)
    for e, f, mask in seg.run(frames, expressions):        # mask: host uint8 [oh, ow] in {0, value}

does the same work in batches of model.batch_size frames:

    upload + cmpc_eval_prep + backbone      once per frame batch (the backbone does not see the sentence: 69 GMAC per frame saved per
                                            further expression)
    model.head on those taps                once per (frame batch, expression)
    cmpc_eval_mask_out + one copy           the batch's masks, sigm >= threshold resized and cropped to out_size(h, w), into a ring of
                                            pinned host buffers behind an event
    (cmpc_mask_components, clean=)          between the two: the masks' largest connected components kept in place on the device

with gv_norm="sample" by default (LSTM_model.set_gv_norm), so that every (expression, frame) pair gets what the batch-1 loop computes,
whatever else shares its batch -- the pads of a short last batch included.

The mask is "resampled value > 0" of the binarised map, the rule of trainval_model.py:245 and of every path in this package.
test.py:308 casts the resampled float map with .astype('uint8') instead, which keeps only values that are exactly >= 1.0 -- an accident
of rounding (an all-ones 320 x 320 map comes out 98.4 % foreground at (240, 427) and 0.19 % at (166, 250)); it is not reproduced.

Order on the device.  The graphed backbone alternates two static output slots (LSTM_model._backbone_graphed), and features_async makes
the backbone stream wait for everything enqueued on the caller's stream so far.  run() enqueues frame batch n + 1's upload, prep and
backbone BEFORE batch n's heads: that pass runs beside batch n's heads, and it rewrites the slot of batch n - 1, whose heads were all
enqueued before it.  The pass after it is enqueued behind batch n's heads in the same way, so no tap is rewritten while a head may still
read it.  Only the caller's thread talks to HIP; nothing allocates and nothing synchronises the device in the
steady state: the host waits only on the event of the ring slot it is about to hand out or reuse.
"""
from __future__ import annotations

from collections import deque
from typing import Callable, Iterable, Iterator, List, Optional, Sequence, Tuple

import numpy as np

from . import _lib, hostutil as HU
from .evaluate import (CC_STATS, JF_COUNTS, MAX_BATCH, JfPlan, _check_dcrf_method, _images_u8, agree_logit, cc_descs, cc_workspace, check_gv_norm,
                       check_pool_mode, gv_norm_scope, plan_masks, plan_prep)


def half_size(h: int, w: int) -> Tuple[int, int]:
    """test.py:308: masks are written at (h // 2, w // 2)."""
    return h // 2, w // 2


def plan_batches(n: int, B: int) -> List[List[int]]:
    """Frame indices of each batch of B: consecutive frames; a short last batch is padded by repeating its first frame."""
    if n <= 0 or B <= 0:
        raise ValueError("plan_batches: %d frames in batches of %d" % (n, B))
    out = []
    for s in range(0, n, B):
        idx = list(range(s, min(s + B, n)))
        out.append(idx + [idx[0]] * (B - len(idx)))
    return out


def check_expression(i: int, ex, vocab, T: int) -> Tuple[np.ndarray, int]:
    """A sentence (tokenised as test.py:267 does, hostutil.preprocess_sentence_lstm) or an (ids, seq_len) pair -> (END-padded int32 ids
    [T], seq_len).  Raises ValueError naming expression `i`."""
    if isinstance(ex, str):
        if vocab is None:
            raise ValueError("expression %d: a sentence needs the vocabulary (FrameSegmenter(vocab=...)); pass (ids, seq_len) otherwise" % i)
        ids, n = HU.preprocess_sentence_lstm(ex, vocab, T)
        if n == 0:
            raise ValueError("expression %d: empty sentence (the model needs at least one word)" % i)
        return np.asarray(ids, dtype=np.int32), n
    try:
        ids, n = ex
    except (TypeError, ValueError):
        raise ValueError("expression %d: expected a sentence or an (ids, seq_len) pair, got %r" % (i, type(ex).__name__)) from None
    ids = np.asarray(ids)
    if ids.ndim != 1 or ids.shape[0] != T or not np.issubdtype(ids.dtype, np.integer):
        raise ValueError("expression %d: ids must be integers [%d], got %s %s" % (i, T, ids.dtype, ids.shape))
    n = int(n)
    if not 1 <= n <= T:
        raise ValueError("expression %d: seq_len %d outside 1..%d" % (i, n, T))
    return ids.astype(np.int32), n


def check_ground_truth(e: int, f: int, gt, size: Tuple[int, int]) -> np.ndarray:
    """What run(ground_truth=...) returned for expression e and frame f -- a mask [oh, ow] (non-zero = object) or an (annotation, key)
    pair cut with hostutil.object_mask -- as uint8 {0, 1} at the size of the yielded mask.  Raises ValueError naming (e, f)."""
    try:
        obj = HU.object_mask(gt[0], gt[1]) if isinstance(gt, tuple) and len(gt) == 2 else HU.object_mask(gt)
    except ValueError as err:
        raise ValueError("ground truth of (expression %d, frame %d): %s" % (e, f, err)) from None
    if obj.shape != tuple(size):
        raise ValueError("ground truth of (expression %d, frame %d): %s, the mask is %s (out_size of the frame)" % (e, f, obj.shape, tuple(size)))
    return np.ascontiguousarray(obj).view(np.uint8)


def plan_scoring(descs, pairs: Sequence[Tuple[int, np.ndarray]], nbytes: int, bound_th: float) -> Optional[JfPlan]:
    """The cmpc_mask_jf call that scores results `i` of `descs` (the packed masks of one ring slot) against the ground truths of
    `pairs` [(i, uint8 mask)]; None when the slot holds no annotated frame.  The counts ride at the 8-aligned tail of the slot."""
    if not pairs:
        return None
    ds = [descs[i] for i, _ in pairs]
    return JfPlan([(d.h, d.w) for d in ds], [d.offset for d in ds], gts=[g for _, g in pairs], bound_th=bound_th,
                  idx=[i for i, _ in pairs], counts_off=scored_bytes(nbytes, 0))


def scored_bytes(nbytes: int, n: int) -> int:
    """Bytes of a ring slot that holds `nbytes` of packed masks and the counts of n of them behind, 8-byte aligned."""
    return -(-nbytes // 8) * 8 + 8 * JF_COUNTS * n


def slot_counts(host: np.ndarray, plan: JfPlan) -> np.ndarray:
    """The int64 [n, 6] counts at the tail of a pinned slot."""
    return host[plan.counts_off: plan.counts_off + 8 * JF_COUNTS * plan.n].view(np.int64).reshape(plan.n, JF_COUNTS)


def _enqueue_scoring(stage, plan: JfPlan, nbytes: int) -> int:
    """The device half both stages share: cmpc_mask_jf on the `nbytes` of masks cmpc_eval_mask_out left in stage.mask_dev, the counts
    into the same buffer behind them.  Returns the bytes the slot's one copy now carries."""
    base = stage.mask_dev.data_ptr()
    stage.scorer.score(base, nbytes, plan, base + plan.counts_off)
    return scored_bytes(nbytes, plan.n)


# ---- describe=: a descriptor, its area and the agreement of two levels per result, for hostutil.PivotLog --------------------------------
DESCRIBE_LEVELS = ("c3", "c4", "c5")           # the backbone taps in the order model.features returns them
AGREE_THRESHOLD = 0.2                          # CMPCv4_model.py:146: iou_with_threshold(sigmoid(score_c4), sigmoid(score_c5), 0.2)


def check_describe(model, describe: Optional[str], weights: str) -> Optional[int]:
    """describe -> the index of that tap in model.features' result (None: no describing).  Raises ValueError for an unknown level or
    weights, and for "c3" on the CMPCv5 models, whose first tap is c2 at another grid."""
    check_pool_mode(weights)
    if describe is None:
        return None
    if describe not in DESCRIBE_LEVELS:
        raise ValueError("describe must be None, 'c3', 'c4' or 'c5', got %r" % (describe,))
    if describe == "c3" and getattr(model, "v5", False):
        raise ValueError("describe='c3': the CMPCv5 models' first tap is c2, at another grid than c4 and c5; use 'c4' or 'c5'")
    return DESCRIBE_LEVELS.index(describe)


class DescribePlan:
    """Where the describe tail of a ring slot with n results lies, every part 4-byte and the counts 8-byte aligned: int64 counts
    [n, 2] (I, U) at `off` (8-aligned: behind the masks, and behind the J / F counts when the slot is scored), float32 descriptors
    [n, C] behind them, float32 areas [n] behind those; `end`: the bytes the slot's one copy then carries."""
    __slots__ = ("n", "C", "off", "desc_off", "area_off", "end")

    def __init__(self, n: int, C: int, off: int):
        if off % 8:
            raise ValueError("DescribePlan: offset %d is not 8-byte aligned" % off)
        self.n, self.C, self.off = int(n), int(C), int(off)
        self.desc_off = self.off + 16 * self.n
        self.area_off = self.desc_off + 4 * self.n * self.C
        self.end = self.area_off + 4 * self.n


def plan_describe(nbytes: int, n_scored: int, n: int, C: int) -> DescribePlan:
    """The tail of a slot that holds `nbytes` of packed masks, the J / F counts of n_scored of them and n described results."""
    return DescribePlan(n, C, scored_bytes(nbytes, n_scored))


def slot_describe(host: np.ndarray, plan: DescribePlan) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(int64 counts [n, 2], float32 descriptors [n, C], float32 areas [n]) at the tail of a pinned slot (views)."""
    return (host[plan.off: plan.desc_off].view(np.int64).reshape(plan.n, 2),
            host[plan.desc_off: plan.area_off].view(np.float32).reshape(plan.n, plan.C),
            host[plan.area_off: plan.end].view(np.float32))


def _tap_channels(model, level: int) -> int:
    cfg = model.cfg
    return int((cfg.c3_dim, cfg.c4_dim, cfg.vf_dim)[level])


def _check_describe_grid(model, level: int):
    cfg = model.cfg
    if model.H % cfg.vf_h or model.W % cfg.vf_w or _tap_channels(model, level) % 8:
        raise ValueError("describe: a %d x %d score map over a %d x %d tap of %d channels: the map must be a multiple of the tap grid and "
                         "the channels a multiple of 8" % (model.H, model.W, cfg.vf_h, cfg.vf_w, _tap_channels(model, level)))


def _enqueue_describe(stage, tap, i0: int, sigm_ptr: int, a, b, plan: DescribePlan, row: int, n: int):
    """The device half both stages share: cmpc_mask_pool on results i0 .. i0 + n - 1 of `tap` weighted by the n float32 [H, W] maps at
    sigm_ptr, cmpc_level_agree on the n logit maps a and b, into rows row .. row + n - 1 of the plan's tail in stage.mask_dev."""
    m, base = stage.model, stage.mask_dev.data_ptr()
    mode, level = stage.describe
    stage.pooler.pool(tap[i0:], n, sigm_ptr, m.H, m.W, mode, stage.threshold_pool, base + plan.desc_off + 4 * plan.C * row,
                      base + plan.area_off + 4 * row)
    stage.pooler.agree(a.data_ptr(), b.data_ptr(), n, int(a.shape[1]), int(a.shape[2]), stage.agree_logit, base + plan.off + 16 * row)


# ---- clean=: keep the largest connected components of every mask on the device (cmpc_mask_components), for hostutil.CleanLog ------------
def check_clean(clean) -> Optional[Tuple[int, int, int]]:
    """clean -> (keep, min_area, connectivity), None when the option is off.  A dict or an object with some of the attributes keep
    (default 1), min_area (0), connectivity (8); ValueError for anything else or for values hostutil.check_clean rejects."""
    if clean is None:
        return None
    names = ("keep", "min_area", "connectivity")
    if isinstance(clean, dict):
        unknown = sorted(set(clean) - set(names))
        if unknown:
            raise ValueError("clean: unknown keys %s (expected some of %s)" % (unknown, list(names)))
        get = clean.get
    elif any(hasattr(clean, k) for k in names):
        get = lambda k, dflt: getattr(clean, k, dflt)
    else:
        raise ValueError("clean must be None, a dict or an object with keep / min_area / connectivity, got %r" % (clean,))
    return HU.check_clean(get("keep", 1), get("min_area", 0), get("connectivity", 8))


class CleanPlan:
    """One cmpc_mask_components call on the n packed masks of a ring slot, and where its statistics lie: int64 [n, 4] at `off`, the next
    8-byte boundary behind whatever the slot already carries (the masks, the J / F counts, the describe tail); `end`: the bytes the
    slot's one copy then carries."""
    __slots__ = ("n", "descs", "keep", "min_area", "connectivity", "off", "end", "ws_bytes")

    def __init__(self, descs, opts: Tuple[int, int, int], tail: int):
        self.n = len(descs)
        self.descs = cc_descs([(d.h, d.w) for d in descs], [d.offset for d in descs])
        self.keep, self.min_area, self.connectivity = opts
        self.off = clean_offset(tail)
        self.end = self.off + 8 * CC_STATS * self.n
        self.ws_bytes = cc_workspace(self.descs, self.n)


def clean_offset(tail: int) -> int:
    return -(-int(tail) // 8) * 8


def cleaned_bytes(tail: int, n: int) -> int:
    """Bytes of a ring slot that carries `tail` bytes and the statistics of n cleaned masks behind them."""
    return clean_offset(tail) + 8 * CC_STATS * n


def slot_clean(host: np.ndarray, plan: CleanPlan) -> np.ndarray:
    """The int64 [n, 4] statistics at the tail of a pinned slot."""
    return host[plan.off: plan.end].view(np.int64).reshape(plan.n, CC_STATS)


def _enqueue_clean(stage, plan: CleanPlan, nbytes: int):
    """The device half both stages share: cmpc_mask_components in place on the `nbytes` of masks cmpc_eval_mask_out left in
    stage.mask_dev, the statistics into the same buffer at the plan's offset."""
    base = stage.mask_dev.data_ptr()
    stage.cleaner.run(base, nbytes, plan.descs, plan.n, plan.connectivity, plan.keep, plan.min_area, base + plan.off, ws_bytes=plan.ws_bytes)


# ---- propagate=: keep what a mask propagator needs while run() goes, then carry the pivot frames' answers to their neighbours ------------
PROPAGATE_LEVELS = ("c4", "c5")                # taps at the head's own grid (vf_h x vf_w) on every model


class PropOptions:
    """FrameSegmenter(propagate=...) checked and completed: level, radius, temperature, alpha, num_propagate, bank, results."""
    __slots__ = ("level", "radius", "temperature", "alpha", "num_propagate", "bank", "results")
    DEFAULTS = {"level": None, "radius": 12, "temperature": 0.07, "alpha": 0.5, "num_propagate": 2, "bank": 128, "results": 512}

    def tap(self) -> int:
        return DESCRIBE_LEVELS.index(self.level)


def check_propagate(model, propagate, describe: Optional[str]) -> Optional[PropOptions]:
    """propagate -> PropOptions, None when the option is off.  A dict or an object with some of the attributes level ("c4" or "c5";
    default: the describe level when that is one of the two, else "c4"), radius (12; negative: the whole grid), temperature (0.07),
    alpha (0.5), num_propagate (2), bank (128 frames), results (512 (expression, frame) pairs); ValueError for anything else."""
    if propagate is None:
        return None
    names = tuple(PropOptions.DEFAULTS)
    if isinstance(propagate, dict):
        unknown = sorted(set(propagate) - set(names))
        if unknown:
            raise ValueError("propagate: unknown keys %s (expected some of %s)" % (unknown, list(names)))
        get = propagate.get
    elif not isinstance(propagate, (str, int, float)) and any(hasattr(propagate, k) for k in names):
        get = lambda k, dflt: getattr(propagate, k, dflt)
    else:
        raise ValueError("propagate must be None, a dict or an object with some of %s, got %r" % (list(names), propagate))
    o = PropOptions()
    for k, dflt in PropOptions.DEFAULTS.items():
        setattr(o, k, get(k, dflt))
    if o.level is None:
        o.level = describe if describe in PROPAGATE_LEVELS else "c4"
    if o.level not in PROPAGATE_LEVELS:
        raise ValueError("propagate: level must be 'c4' or 'c5', got %r" % (o.level,))
    for k in ("radius", "num_propagate", "bank", "results"):
        v = getattr(o, k)
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise ValueError("propagate: %s must be an integer, got %r" % (k, v))
        setattr(o, k, int(v))
    if o.num_propagate < 0 or o.bank < 1 or o.results < 1:
        raise ValueError("propagate: num_propagate %d must be >= 0, bank %d and results %d >= 1" % (o.num_propagate, o.bank, o.results))
    try:
        o.temperature, o.alpha = float(o.temperature), float(o.alpha)
    except (TypeError, ValueError):
        raise ValueError("propagate: temperature and alpha must be numbers, got %r and %r" % (o.temperature, o.alpha)) from None
    if not (_lib.PROP_MIN_TEMPERATURE <= o.temperature < float("inf")):
        raise ValueError("propagate: temperature must be finite and >= %g, got %r" % (_lib.PROP_MIN_TEMPERATURE, o.temperature))
    if not 0.0 <= o.alpha <= 1.0:
        raise ValueError("propagate: alpha must lie in [0, 1], got %r" % (o.alpha,))
    return o


def _consecutive_runs(idx: Sequence[int]) -> List[Tuple[int, int]]:
    """(first position, length) of every run of consecutive values in idx."""
    runs, s = [], 0
    for i in range(1, len(idx) + 1):
        if i == len(idx) or idx[i] != idx[i - 1] + 1:
            runs.append((s, i - s))
            s = i
    return runs


def _slot_tail(nbytes: int, scored: Optional[int], described: Optional[Tuple[int, int]]) -> int:
    """The bytes a slot carries before any clean tail: `nbytes` of masks, the counts of `scored` results (None: no scoring), the
    describe tail of described = (n, C) results."""
    if described is not None:
        return plan_describe(nbytes, scored or 0, described[0], described[1]).end
    return nbytes if scored is None else scored_bytes(nbytes, scored)


class _DeviceStage:
    """The device half of FrameSegmenter.  All buffers are allocated once (the pinned ring and the device mask buffer grow only when a
    batch needs more bytes than any before it): two feed / proc_im sets that alternate with the frame batches, one device mask buffer,
    `nslots` pinned host buffers with an event each.  Everything is enqueued on the caller's current stream."""

    def __init__(self, model, nslots: int, threshold: float, value: int, dcrf: bool, dcrf_method: str, describe=None, clean: bool = False,
                 propagate: Optional[PropOptions] = None):
        import torch
        from .evaluate import _CcDevice, _JfDevice, _PoolDevice, _PropDevice, _Staging
        self.torch = torch
        self.model, self.threshold, self.value, self.dcrf, self.dcrf_method = model, threshold, value, dcrf, dcrf_method
        self.dev = model.device
        self.cleaner = _CcDevice(self.dev) if clean else None
        B, H, W = model.batch_size, model.H, model.W
        self.describe = describe                       # (weights, index of the tap) or None
        if describe is not None:
            _check_describe_grid(model, describe[1])
            self.pooler, self.threshold_pool, self.agree_logit = _PoolDevice(self.dev), threshold, agree_logit(AGREE_THRESHOLD)
            self.pooler.reserve(B, model.cfg.vf_h, model.cfg.vf_w, self.describe_channels())
        with torch.cuda.device(self.dev):
            self.staging = _Staging(self.dev)
            self.feed = [torch.empty(B, H, W, 3, dtype=torch.float32, device=self.dev) for _ in range(2)]
            self.proc = [torch.empty(B, H, W, 3, dtype=torch.uint8, device=self.dev) for _ in range(2)]
            self.events = [torch.cuda.Event() for _ in range(nslots)]
        self.scorer = _JfDevice(self.dev)
        self.nslots = nslots
        self.host: List = [None] * nslots
        self.mask_dev = None
        self.k = 0
        self.words = []
        self.prop = propagate
        if propagate is not None:                      # the banks, once: taps per frame, sigm and its point samples per (expression, frame)
            cfg = model.cfg
            h, w, C = cfg.vf_h, cfg.vf_w, _tap_channels(model, propagate.tap())
            if H % h or W % w or C % 8:
                raise ValueError("propagate: a %d x %d score map over a %d x %d tap of %d channels: the map must be a multiple of the tap "
                                 "grid and the channels a multiple of 8" % (H, W, h, w, C))
            tdt = {_lib.DT_F32: torch.float32, _lib.DT_BF16: torch.bfloat16, _lib.DT_F16: torch.float16}[model.dt]
            with torch.cuda.device(self.dev):
                self.tap_bank = torch.empty(propagate.bank, h, w, C, dtype=tdt, device=self.dev)
                self.sigm_bank = torch.empty(propagate.results, H, W, dtype=torch.float32, device=self.dev)
                self.label_bank = torch.empty(propagate.results, h, w, dtype=torch.float32, device=self.dev)
                self.prop_out = torch.empty(B, h, w, dtype=torch.float32, device=self.dev)
                self.fused = torch.empty(B, H, W, dtype=torch.float32, device=self.dev)
            self.propagator = _PropDevice(self.dev)
            self.propagator.reserve(B, h, w)

    def bank(self, feats, sigm, e: int, n: int, where: Tuple[int, int]):
        """Keep what propagate_batch() reads: the chosen tap of the batch's n real frames (once per frame batch, with expression 0) at
        their frame ids, and expression e's sigm and its point samples at results e * F + frame.  where = (first frame, F)."""
        first, F = where
        fy, fx = self.model.H // self.tap_bank.shape[1], self.model.W // self.tap_bank.shape[2]
        if e == 0:
            self.tap_bank[first: first + n].copy_(feats[self.prop.tap()].reshape((-1,) + tuple(self.tap_bank.shape[1:]))[:n])
        r = e * F + first
        self.sigm_bank[r: r + n].copy_(sigm[:n])
        self.label_bank[r: r + n].copy_(sigm[:n, ::fy, ::fx])

    def propagate_batch(self, e: int, frames: Sequence[int], sources: Sequence[Sequence[int]], F: int, descs, nbytes: int, slot: int,
                        jf: Optional[JfPlan] = None, clean: Optional[CleanPlan] = None):
        """Frames `frames` (ascending, at most a batch) of expression e receive from their pivots `sources`: cmpc_label_propagate on the
        banks, cmpc_prop_fuse with each frame's own sigm, then cmpc_eval_mask_out, clean= and scoring as segment() enqueues them, into
        ring slot `slot` behind its event."""
        from .evaluate import prop_items
        torch, m, o = self.torch, self.model, self.prop
        n = len(frames)
        h, w = int(self.tap_bank.shape[1]), int(self.tap_bank.shape[2])
        items = prop_items([(f, [(p, e * F + p) for p in src]) for f, src in zip(frames, sources)])
        with torch.no_grad(), torch.cuda.device(self.dev):
            self.propagator.propagate(self.tap_bank, self.label_bank, items, o.radius, o.temperature, self.prop_out.data_ptr(), 0)
            for i0, k in _consecutive_runs(list(frames)):          # a frame's own sigm is read where it lies: one call per run of frames
                self.propagator.fuse(self.sigm_bank[e * F + frames[i0]].data_ptr(), self.prop_out[i0].data_ptr(), k, h, w, m.H, m.W, o.alpha,
                                     self.fused[i0].data_ptr())
            _lib.call("cmpc_eval_mask_out", self.fused.data_ptr(), _lib.EVAL_F32, n, m.H, m.W, float(self.threshold), descs,
                      self.mask_dev.data_ptr(), self.mask_dev.numel(), self.value, torch.cuda.current_stream(self.dev).cuda_stream)
            if clean is not None:
                _enqueue_clean(self, clean, nbytes)
            if jf is not None:
                nbytes = _enqueue_scoring(self, jf, nbytes)
            if clean is not None:
                nbytes = clean.end
            self.host[slot][:nbytes].copy_(self.mask_dev[:nbytes], non_blocking=True)
            self.events[slot].record(torch.cuda.current_stream(self.dev))

    def reserve(self, nbytes: int):
        """Room for `nbytes` of packed masks in every ring slot and in the device buffer."""
        torch = self.torch
        if self.mask_dev is not None and self.mask_dev.numel() >= nbytes:
            return
        cap = max(nbytes, 1 << 20)
        torch.cuda.synchronize(self.dev)               # a copy into the old buffers may be in flight (growth only: not the steady state)
        with torch.cuda.device(self.dev):
            self.mask_dev = torch.empty(cap, dtype=torch.uint8, device=self.dev)
            old, self.host = self.host, [torch.empty(cap, dtype=torch.uint8, pin_memory=True) for _ in range(self.nslots)]
        for o, h in zip(old, self.host):               # results not handed out yet move with their slot
            if o is not None:
                h[: o.numel()].copy_(o)

    def describe_channels(self) -> int:
        return _tap_channels(self.model, self.describe[1])

    def set_expressions(self, exprs: Sequence[Tuple[np.ndarray, int]]):
        torch, B = self.torch, self.model.batch_size
        with torch.cuda.device(self.dev):
            self.words = [(torch.from_numpy(np.repeat(ids[None], B, 0)).to(self.dev), torch.full((B,), n, dtype=torch.int32).to(self.dev))
                          for ids, n in exprs]

    def begin(self, images: List[np.ndarray]):
        """Upload, cmpc_eval_prep and the backbone pass of one (padded) frame batch; returns the token segment() takes."""
        torch, m = self.torch, self.model
        k, self.k = self.k, 1 - self.k
        descs, nbytes = plan_prep([a.shape for a in images], m.H, m.W)
        with torch.no_grad(), torch.cuda.device(self.dev):
            src = self.staging.upload(images, descs, nbytes)
            feed, proc = self.feed[k], self.proc[k]
            _lib.call("cmpc_eval_prep", src.data_ptr(), nbytes, descs, len(images), m.H, m.W, proc.data_ptr(), feed.data_ptr(),
                      torch.cuda.current_stream(self.dev).cuda_stream)
            feats, done = m.features_async(feed)
        return feats, done, feed, proc

    def segment(self, token, e: int, descs, nbytes: int, slot: int, jf: Optional[JfPlan] = None, describe: Optional[DescribePlan] = None,
                clean: Optional[CleanPlan] = None, propagate: Optional[Tuple[int, int]] = None):
        """Head of expression e on the batch's taps, the masks of its first len(descs) frames into ring slot `slot`; with `jf`, their
        J / F counts behind them; with `describe`, their descriptors (the batch's tap weighted by the head's sigm, with DenseCRF too:
        the descriptor describes the network's own answer), areas and level-agreement counts behind those; with `clean`, the masks
        are cleaned in place before they are scored, and their component statistics ride at the end."""
        torch, m = self.torch, self.model
        feats, done, feed, proc = token
        n = len(descs)
        words, sl = self.words[e]
        with torch.no_grad(), torch.cuda.device(self.dev):
            o = m.head(feats, words, sl, after=done, im=feed)
            sigm = o["sigm"].float().reshape(m.batch_size, m.H, m.W)
            if propagate is not None:
                self.bank(feats, sigm, e, n, propagate)
            if self.dcrf:
                from . import crf
                score, thr = crf.dense_crf_batch(sigm[:n], proc[:n], device=self.dev, method=self.dcrf_method), 0.5
            else:
                score, thr = sigm, self.threshold
            dt = _lib.EVAL_F32 if score.dtype == torch.float32 else _lib.EVAL_U8
            _lib.call("cmpc_eval_mask_out", score.data_ptr(), dt, n, m.H, m.W, float(thr), descs, self.mask_dev.data_ptr(),
                      self.mask_dev.numel(), self.value, torch.cuda.current_stream(self.dev).cuda_stream)
            if clean is not None:
                _enqueue_clean(self, clean, nbytes)
            if jf is not None:
                nbytes = _enqueue_scoring(self, jf, nbytes)
            if describe is not None:
                _enqueue_describe(self, feats[self.describe[1]], 0, sigm.data_ptr(), o["score_c4"], o["score_c5"], describe, 0, n)
                nbytes = describe.end
            if clean is not None:
                nbytes = clean.end
            self.host[slot][:nbytes].copy_(self.mask_dev[:nbytes], non_blocking=True)
            self.events[slot].record(torch.cuda.current_stream(self.dev))

    def done(self, slot: int) -> bool:
        return self.events[slot].query()

    def wait(self, slot: int):
        self.events[slot].synchronize()

    def view(self, slot: int) -> np.ndarray:
        return self.host[slot].numpy()


class FrameSegmenter:
    """test.py:250-329 batched on the GPU (module docstring).  run(frames, expressions) yields (e, f, mask) for every expression index e
    and frame index f: frame batches in order, within a batch expressions in order, within those frames in order.

    frames: original-size uint8 arrays [h, w, 3] or [h, w] (any iterable: decoded lazily, one batch ahead); expressions: sentences
    (needs `vocab`) or (END-padded ids [T], seq_len) pairs.  mask = value * (resize_and_crop(sigm >= threshold, *out_size(h, w)) > 0),
    thresholding the float32 sigm itself (test.py:307); with dcrf, the same resampling of the DenseCRF argmax on sigm / proc_im
    (test.py:309-322, crf.dense_crf_batch).  gv_norm: "sample" (default: the loop this replaces is batch 1) or "batch"; set for the
    run, the model's own mode restored when the generator ends or is closed.  depth: (frame batch, expression) results in flight behind
    the one being handed out (depth + 1 pinned slots).  copy=False yields views of the pinned slot, valid until the next iteration.

    run(..., ground_truth=fn) also scores the masks on the device (J and F, cmpc_mask_jf): fn(e, f) returns None for a frame without
    annotation, a mask at out_size(h, w), or an (annotation, key) pair for hostutil.object_mask; it is called once per pair, on the
    caller's thread, when that result is enqueued.  The counts travel with the masks and are added to `jf` (a hostutil.JFEval, kept
    as self.jf; a fresh one when none is passed) under sequence (seq, e) and frame f as the masks are handed out; the yielded
    triples are the same with and without it.

    describe="c3" | "c4" | "c5" also describes every result for the reference's pivot-frame step (test.py:150-181): behind each head
    call cmpc_mask_pool pools that backbone tap weighted by the head's sigm (describe_weights="soft") or by sigm >= threshold
    ("hard"), and cmpc_level_agree counts where the score_c4 and score_c5 levels agree at probability 0.2 (test.py:289).  Descriptor,
    area and counts travel with the masks and reach `pivots` (run(..., pivots=), a hostutil.PivotLog kept as self.pivots; a fresh one
    when none is passed) under sequence (seq, e) and frame f before the masks are yielded; the yielded triples are the same.  A log
    holds a (sequence, frame) once: a second run() with the same `pivots` and the same `seq` raises ValueError from PivotLog.add when
    its first result is handed out -- pass a fresh log or another seq.

    clean={"keep": 1, "min_area": 0, "connectivity": 8} (a dict or an object with some of these attributes; None, the default: off)
    cleans every mask on the device before anything else sees it: behind cmpc_eval_mask_out, cmpc_mask_components keeps the `keep`
    largest connected components (0: all) of at least `min_area` pixels in place -- hostutil.clean_mask's rule -- so the yielded
    masks and, with ground_truth, the J / F counts are those of the cleaned masks; describe= reads sigm and is unaffected; with dcrf
    the DenseCRF mask is cleaned.  The statistics (n_components, area, area_largest, area_kept) of the mask BEFORE cleaning travel
    with the masks and reach `cleaned` (run(..., cleaned=), a hostutil.CleanLog kept as self.cleaned; a fresh one when none is
    passed) under sequence (seq, e) and frame f.  With clean=None no code path changes.

    propagate={"level": "c4", "radius": 12, "temperature": 0.07, "alpha": 0.5, "num_propagate": 2, "bank": 128, "results": 512} (a dict
    or an object with some of these attributes; None, the default: off) keeps what a mask propagator needs while run() goes -- run()
    yields exactly what it yields without it.  In device banks allocated once: per frame the chosen tap (level: "c4" or "c5", default
    the describe level, else "c4"), per (expression, frame) the head's float32 sigm [H, W] and its label, the point sample
    sigm[y * (H / h), x * (W / w)] that cmpc_mask_pool uses (H % h == 0 and W % w == 0 as there).  The video's length must be known
    before any work: a `frames` without len() is read into a list first, and run() raises ValueError when the video exceeds `bank`
    frames or expressions x frames exceed `results`.  Afterwards seg.propagate(pivots) carries the pivot frames' answers to their
    neighbours (see there).  Not with dcrf=True (ValueError): fusing happens before a CRF, and that is not built.  With propagate=None
    no code path changes."""

    def __init__(self, model, vocab=None, threshold: float = 0.5, out_size: Callable[[int, int], Tuple[int, int]] = half_size, value: int = 255,
                 dcrf: bool = False, dcrf_method: str = "lattice", gv_norm: str = "sample", depth: int = 2, copy: bool = True, _stage=None,
                 describe: Optional[str] = None, describe_weights: str = "soft", clean=None, propagate=None):
        if getattr(model, "video", False):
            raise ValueError("FrameSegmenter: the video model (CMPC_video_mm_tgraph_allvec) is not supported: it takes a clip per forward pass")
        if model.batch_size > MAX_BATCH:
            raise ValueError("FrameSegmenter: model.batch_size %d > %d" % (model.batch_size, MAX_BATCH))
        if value not in (1, 255):
            raise ValueError("value must be 1 or 255, got %r" % (value,))
        if int(depth) < 1:
            raise ValueError("depth must be >= 1, got %r" % (depth,))
        self.model, self.vocab, self.threshold, self.out_size, self.value = model, vocab, float(threshold), out_size, int(value)
        self.dcrf, self.dcrf_method = bool(dcrf), _check_dcrf_method(dcrf_method)
        self.gv_norm = check_gv_norm(gv_norm, allow_none=False)
        self.depth, self.copy = int(depth), bool(copy)
        self.B, self.T, self.H, self.W = model.batch_size, model.num_steps, model.H, model.W
        self.nslots = self.depth + 1
        self.jf, self.bound_th = None, 0.008
        self.describe, self.describe_weights, self.pivots = describe, describe_weights, None
        level = check_describe(model, describe, describe_weights)
        self.clean, self.cleaned = check_clean(clean), None
        kw = {} if level is None else {"describe": (describe_weights, level)}
        if self.clean is not None:
            kw["clean"] = True
        self.prop, self._prop_run, self.prop_jf, self.prop_cleaned = check_propagate(model, propagate, describe), None, None, None
        if self.prop is not None:
            if self.dcrf:
                raise ValueError("FrameSegmenter(propagate=..., dcrf=True): fusing happens before a CRF, which is not built; use dcrf=False")
            kw["propagate"] = self.prop
        self.stage = _stage if _stage is not None else _DeviceStage(model, self.nslots, self.threshold, self.value, self.dcrf, self.dcrf_method, **kw)

    def _batches(self, frames: Iterable) -> Iterator[Tuple[int, List[np.ndarray]]]:
        """(index of the first frame, the validated frames) of every batch of B, read lazily."""
        first, cur = 0, []
        for f, im in enumerate(frames):
            a = np.asarray(im)
            try:
                cur.extend(_images_u8([a]))
            except ValueError as e:
                raise ValueError("frame %d: %s" % (f, str(e).split(": ", 1)[-1])) from None
            if len(cur) == self.B:
                yield first, cur
                first, cur = f + 1, []
        if cur:
            yield first, cur

    def _plan(self, first: int, ims: List[np.ndarray]):
        sizes = []
        for i, a in enumerate(ims):
            oh, ow = self.out_size(int(a.shape[0]), int(a.shape[1]))
            if int(oh) < 1 or int(ow) < 1:
                raise ValueError("frame %d: out_size(%d, %d) = (%d, %d) is empty" % (first + i, a.shape[0], a.shape[1], oh, ow))
            sizes.append((int(oh), int(ow)))
        descs, nbytes = plan_masks(sizes, self.H, self.W)
        return descs, nbytes

    def run(self, frames: Iterable, expressions: Sequence, ground_truth: Optional[Callable] = None, jf: Optional[HU.JFEval] = None,
            seq=None, pivots: Optional[HU.PivotLog] = None, cleaned: Optional[HU.CleanLog] = None) -> Iterator[Tuple[int, int, np.ndarray]]:
        exprs = [check_expression(i, ex, self.vocab, self.T) for i, ex in enumerate(expressions)]
        if not exprs:
            raise ValueError("FrameSegmenter.run: no expressions")
        if self.clean is not None:
            self.cleaned = cleaned if cleaned is not None else HU.CleanLog()
        if ground_truth is not None:
            self.jf = jf if jf is not None else HU.JFEval()
        st = self.stage
        F = None                                   # frames of the video: known ahead only when the banks of propagate= must hold them
        if self.prop is not None:
            frames = frames if hasattr(frames, "__len__") else list(frames)
            F = len(frames)
            if F > self.prop.bank or len(exprs) * F > self.prop.results:
                raise ValueError("FrameSegmenter.run: %d frames x %d expressions exceed the banks of propagate= (bank = %d frames, results = %d)"
                                 % (F, len(exprs), self.prop.bank, self.prop.results))
            self._prop_run = {"F": F, "E": len(exprs), "seq": seq, "sizes": []}
        C = None                                   # channels of the described tap
        if self.describe is not None:
            self.pivots = pivots if pivots is not None else HU.PivotLog()
            C = st.describe_channels()
        free = deque(range(self.nslots))
        pending = deque()                          # (slot, e, first frame, descs, scoring plan, describe plan) in enqueue order = yield order

        def hand_out(block: bool):
            """Yield the masks of the oldest result(s) whose event has completed (waiting for the oldest one if `block`)."""
            while pending and (block or st.done(pending[0][0])):
                slot, e, first, descs, plan, dplan, cplan = pending.popleft()
                st.wait(slot)
                host = st.view(slot)
                if cplan is not None:
                    for i, c in enumerate(slot_clean(host, cplan)):
                        self.cleaned.add((seq, e), first + i, c)
                if plan is not None:
                    for i, c in zip(plan.idx, slot_counts(host, plan)):
                        self.jf.add((seq, e), first + i, c)
                if dplan is not None:
                    for i, (iu, d, a) in enumerate(zip(*slot_describe(host, dplan))):
                        self.pivots.add((seq, e), first + i, d, a, iu)
                for i, d in enumerate(descs):
                    mk = host[d.offset: d.offset + d.h * d.w].reshape(d.h, d.w)
                    yield e, first + i, (mk.copy() if self.copy else mk)
                free.append(slot)                  # only now: the caller has moved past the slot's last mask
                block = False

        with gv_norm_scope(self.model, self.gv_norm):
            st.set_expressions(exprs)
            it = self._batches(frames)

            def begin_next():
                nxt = next(it, None)
                if nxt is None:
                    return None
                first, ims = nxt
                descs, nbytes = self._plan(first, ims)
                if F is not None:
                    self._prop_run["sizes"].extend((d.h, d.w) for d in descs)
                tail = _slot_tail(nbytes, None if ground_truth is None else len(descs), None if C is None else (len(descs), C))
                st.reserve(tail if self.clean is None else cleaned_bytes(tail, len(descs)))
                return first, descs, nbytes, st.begin(ims + [ims[0]] * (self.B - len(ims)))

            cur = begin_next()
            if cur is None:
                raise ValueError("FrameSegmenter.run: no frames")
            while cur is not None:
                nxt = begin_next()                 # the next batch's backbone pass goes in ahead of this batch's heads (module docstring)
                first, descs, nbytes, token = cur
                for e in range(len(exprs)):
                    if not free:
                        yield from hand_out(True)
                    slot = free.popleft()
                    # several call shapes on purpose: a stage written before jf=, describe= or clean= existed (the fake stages of the older host
                    # tests, a caller's own _stage) keeps working as long as the options it does not know stay off
                    plan = dplan = None
                    if ground_truth is not None:
                        gts = [(i, ground_truth(e, first + i)) for i in range(len(descs))]
                        plan = plan_scoring(descs, [(i, check_ground_truth(e, first + i, g, (descs[i].h, descs[i].w)))
                                                    for i, g in gts if g is not None], nbytes, self.bound_th)
                    kw = {}
                    if C is not None:
                        dplan = plan_describe(nbytes, 0 if plan is None else plan.n, len(descs), C)
                        kw = {"jf": plan, "describe": dplan}
                    elif ground_truth is not None:
                        kw = {"jf": plan}
                    cplan = None
                    if self.clean is not None:     # the fourth shape: `clean` reaches the stage only when the option is on
                        tail = dplan.end if dplan is not None else nbytes if plan is None else scored_bytes(nbytes, plan.n)
                        cplan = kw["clean"] = CleanPlan(descs, self.clean, tail)
                    if F is not None:              # the fifth: the stage keeps the taps, sigm and labels of (e, first .. first + n - 1)
                        kw["propagate"] = (first, F)
                    st.segment(token, e, descs, nbytes, slot, **kw)
                    pending.append((slot, e, first, descs, plan, dplan, cplan))
                    yield from hand_out(False)
                cur = nxt
            while pending:
                yield from hand_out(True)

    def propagate(self, pivots, ground_truth: Optional[Callable] = None, jf: Optional[HU.JFEval] = None, cleaned: Optional[HU.CleanLog] = None,
                  seq=None) -> Iterator[Tuple[int, int, np.ndarray]]:
        """Carry the pivot frames' answers of the last run() to their neighbours (needs FrameSegmenter(propagate=...), and run()
        consumed to its end).  pivots: a hostutil.PivotLog that holds the sequences (seq, e) as run() logs them (seq: this call's, or
        the run's when None) -- its pivots(.., num_propagate) are taken -- or a dict {e: [frame, ...]}.  For every expression e and
        every frame f of hostutil.propagation_plan(range(F), pivots of e, num_propagate, 4), in batches of model.batch_size frames of
        one expression: cmpc_label_propagate carries the pivots' labels (the point samples of their sigm) to f along the banked taps,
        cmpc_prop_fuse blends the result with f's own sigm (alpha), and the fused map goes through cmpc_eval_mask_out with f's own
        descriptor, threshold and out_size, then clean= and scoring exactly as run() enqueues them, into the same pinned ring behind
        events.  Yields (e, f, mask) for those frames only, expressions in order and frames ascending; pivot frames and frames out of
        reach keep the masks run() gave.  ground_truth / jf / cleaned as in run(); the counts and statistics go to `jf` / `cleaned`
        (fresh logs when None: a log holds a (sequence, frame) once) kept as self.prop_jf / self.prop_cleaned."""
        if self.prop is None or self._prop_run is None:
            raise RuntimeError("FrameSegmenter.propagate: run() has not been called with propagate= (FrameSegmenter(..., propagate={...}))")
        o, st, run = self.prop, self.stage, self._prop_run
        F, E, sizes = run["F"], run["E"], run["sizes"]
        if len(sizes) != F:
            raise RuntimeError("FrameSegmenter.propagate: run() saw %d of its %d frames: consume it to its end first" % (len(sizes), F))
        seq = run["seq"] if seq is None else seq
        plans = []
        for e in range(E):
            if isinstance(pivots, HU.PivotLog):
                piv = pivots.pivots((seq, e), o.num_propagate)
            else:
                try:
                    piv = [int(f) for f in pivots[e]]
                except (KeyError, IndexError, TypeError):
                    raise ValueError("FrameSegmenter.propagate: no pivots for expression %d" % e) from None
            plans.append(HU.propagation_plan(range(F), piv, o.num_propagate, _lib.PROP_MAX_SOURCES))
        if self.clean is not None:
            self.prop_cleaned = cleaned if cleaned is not None else HU.CleanLog()
        if ground_truth is not None:
            self.prop_jf = jf if jf is not None else HU.JFEval()
        free = deque(range(self.nslots))
        pending = deque()                          # (slot, e, frames, descs, scoring plan, clean plan) in enqueue order = yield order

        def hand_out(block: bool):
            while pending and (block or st.done(pending[0][0])):
                slot, e, fr, descs, plan, cplan = pending.popleft()
                st.wait(slot)
                host = st.view(slot)
                if cplan is not None:
                    for f, c in zip(fr, slot_clean(host, cplan)):
                        self.prop_cleaned.add((seq, e), f, c)
                if plan is not None:
                    for i, c in zip(plan.idx, slot_counts(host, plan)):
                        self.prop_jf.add((seq, e), fr[i], c)
                for f, d in zip(fr, descs):
                    mk = host[d.offset: d.offset + d.h * d.w].reshape(d.h, d.w)
                    yield e, f, (mk.copy() if self.copy else mk)
                free.append(slot)
                block = False

        for e, plan_e in enumerate(plans):
            todo = sorted(plan_e)
            for s in range(0, len(todo), self.B):
                fr = todo[s: s + self.B]
                descs, nbytes = plan_masks([sizes[f] for f in fr], self.H, self.W)
                plan = None
                if ground_truth is not None:
                    gts = [(i, ground_truth(e, f)) for i, f in enumerate(fr)]
                    plan = plan_scoring(descs, [(i, check_ground_truth(e, fr[i], g, (descs[i].h, descs[i].w))) for i, g in gts if g is not None],
                                        nbytes, self.bound_th)
                tail = nbytes if plan is None else scored_bytes(nbytes, plan.n)
                cplan = None if self.clean is None else CleanPlan(descs, self.clean, tail)
                st.reserve(tail if cplan is None else cplan.end)
                if not free:
                    yield from hand_out(True)
                slot = free.popleft()
                st.propagate_batch(e, fr, [plan_e[f] for f in fr], F, descs, nbytes, slot, jf=plan, clean=cplan)
                pending.append((slot, e, fr, descs, plan, cplan))
                yield from hand_out(False)
        while pending:
            yield from hand_out(True)


# ---- CMPC_video_mm_tgraph_allvec over whole videos (CMPC_video/trainval_video.py:186-253 applied to every frame) --------------------------
CLIP_LOOKAHEAD = 1             # ClipSegmenter(lookahead=None): backbone batches enqueued ahead of the heads that need them


def full_size(h: int, w: int) -> Tuple[int, int]:
    """trainval_video.py:225: the video driver resamples to the frame's own size."""
    return h, w


def clip_window(f: int, n_frames: int, frames: int = 16) -> List[int]:
    """The clip of frame f (0-based) of a video of n_frames as build_A2D_batches.py:150-167 forms it: positions f - frames // 2 + k,
    k = 0..frames-1, each clamped to the video.  Position frames // 2 is f itself."""
    if not 0 <= f < n_frames:
        raise ValueError("clip_window: frame %d outside a video of %d frames" % (f, n_frames))
    return [min(max(f - frames // 2 + k, 0), n_frames - 1) for k in range(frames)]


def sampled_frames(f: int, n_frames: int, frames: int = 16) -> List[int]:
    """The frames of clip_window(f) that the graph reads (model.FRAME_IDX; vid:70): f-8, f-4, f, f+4, f+7 for 16 frames, clamped."""
    from .model import FRAME_IDX
    w = clip_window(f, n_frames, frames)
    return [w[k] for k in FRAME_IDX]


def _reach(frames: int) -> Tuple[int, int]:
    """How far a clip reaches behind and ahead of its own frame."""
    return frames // 2, frames - 1 - frames // 2


def min_ring(frames: int = 16, lookahead: int = CLIP_LOOKAHEAD) -> int:
    """The smallest ring of cached frames ClipSegmenter can run with.  The backbone takes frames in batches of B = len(FRAME_IDX).  With
    f the oldest frame whose heads are not all enqueued, run() enqueues batches up to the one that holds frame f + ahead (ahead =
    frames - 1 - frames // 2, the newest frame f's clip reads) plus `lookahead` more: a batch's first frame s is at most
    f + ahead + B * lookahead.  The batch writes slots s .. s + B - 1 and so evicts frames up to s + B - 1 - ring, which must all be older
    than f - frames // 2, the oldest frame a head not yet enqueued reads: ring >= ahead + B * lookahead + B + frames // 2 =
    frames - 1 + B * (lookahead + 1): 20, 25, 30 for 16-frame clips and a lookahead of 0, 1, 2."""
    from .model import FRAME_IDX
    if frames <= max(FRAME_IDX) or int(lookahead) < 0:
        raise ValueError("min_ring: frames = %r (the graph reads clip position %d), lookahead = %r" % (frames, max(FRAME_IDX), lookahead))
    return frames - 1 + len(FRAME_IDX) * (int(lookahead) + 1)


class _ClipStage:
    """The device half of ClipSegmenter; everything that touches HIP.  Allocated once: one feed / proc_im set, the ring of cached taps
    (three levels, `ring` frames each; a proc_im ring with dcrf), the head's contiguous [5, h, w, C] inputs, one event per backbone batch
    in flight, one device mask buffer and `nslots` pinned host buffers with an event each (these two grow only when a frame needs more
    bytes than any before it).

    Streams.  Upload, cmpc_eval_prep, the graphed backbone and the scatter into the ring run on the model's backbone stream;
    features_async makes that stream wait for everything enqueued on the caller's stream so far (the gathers that read the slots this
    batch evicts among it), and the batch's event is recorded behind the scatter.  Gathers, heads, cmpc_eval_mask_out and the copies to
    the pinned ring run on the caller's stream; a gather waits for the event of the newest batch its clip reads."""

    def __init__(self, model, ring: int, nslots: int, score: str, threshold: float, value: int, dcrf: bool, dcrf_method: str, describe=None,
                 clean: bool = False):
        import ctypes
        import torch
        from .evaluate import _CcDevice, _JfDevice, _PoolDevice, _Staging
        from .model import FRAME_IDX
        self.torch, self.C = torch, ctypes
        self.model, self.score, self.threshold, self.value, self.dcrf, self.dcrf_method = model, score, threshold, value, dcrf, dcrf_method
        self.dev = model.device
        self.ring, self.nslots, self.B = ring, nslots, len(FRAME_IDX)
        B, H, W = self.B, model.H, model.W
        if dcrf and (H * W * 3) % 16:
            raise ValueError("ClipSegmenter(dcrf=True): H * W * 3 = %d bytes of proc_im per frame is not a multiple of 16" % (H * W * 3))
        with torch.no_grad(), torch.cuda.device(self.dev):
            self.staging = _Staging(self.dev)
            self.feed = torch.empty(B, H, W, 3, dtype=torch.float32, device=self.dev)
            self.proc = torch.empty(B, H, W, 3, dtype=torch.uint8, device=self.dev)
            taps = model.features(torch.zeros(B, H, W, 3, dtype=torch.float32, device=self.dev))       # shapes and dtype of the three levels
            self.cache = [torch.empty((ring,) + tuple(t.shape[1:]), dtype=t.dtype, device=self.dev) for t in taps]
            self.gathered = [torch.empty_like(t) for t in taps]
            self.proc_ring = torch.empty(ring, H, W, 3, dtype=torch.uint8, device=self.dev) if dcrf else None
            self.batch_ev = [torch.cuda.Event() for _ in range(ring // B + 2)]
            self.events = [torch.cuda.Event() for _ in range(nslots)]
        self.scorer = _JfDevice(self.dev)
        self.cleaner = _CcDevice(self.dev) if clean else None
        self.describe = describe                       # (weights, index of the tap) or None
        if describe is not None:
            _check_describe_grid(model, describe[1])
            if model.frames // 2 not in FRAME_IDX:
                raise ValueError("describe: clip position %d (the frame itself) is not among the sampled positions %s" % (model.frames // 2, FRAME_IDX))
            self.own = FRAME_IDX.index(model.frames // 2)      # where frame f itself lies among its gathered taps
            # "hard" weights are sigm >= threshold: the run's own threshold when it thresholds sigm, else 0.5 (up >= 1e-9 is a logit >= 0)
            self.pooler, self.threshold_pool = _PoolDevice(self.dev), (threshold if score == "sigm" else 0.5)
            self.agree_logit = agree_logit(AGREE_THRESHOLD)
            self.pooler.reserve(1, model.cfg.vf_h, model.cfg.vf_w, self.describe_channels())
        self.bytes = [t[0].numel() * t.element_size() for t in taps]
        for b in self.bytes:
            if b % 16:
                raise ValueError("ClipSegmenter: a frame's tap block of %d bytes is not a multiple of 16" % b)
        self.host: List = [None] * nslots
        self.mask_dev = None
        self.words = []
        # argument arrays of cmpc_taps_copy, built once
        vp, i64 = ctypes.c_void_p * 3, ctypes.c_int64 * 3
        self._cache_p = vp(*[t.data_ptr() for t in self.cache])
        self._gath_p = vp(*[t.data_ptr() for t in self.gathered])
        self._bytes = i64(*self.bytes)
        self._idx_a, self._idx_b = (ctypes.c_int * _lib.TAPS_MAX_FRAMES)(), (ctypes.c_int * _lib.TAPS_MAX_FRAMES)()
        self._seq = (ctypes.c_int * _lib.TAPS_MAX_FRAMES)(*range(_lib.TAPS_MAX_FRAMES))
        self._proc_bytes = (ctypes.c_int64 * 1)(H * W * 3)

    def reserve(self, nbytes: int):
        """Room for `nbytes` of packed masks (one frame, every expression) in every ring slot and in the device buffer."""
        torch = self.torch
        if self.mask_dev is not None and self.mask_dev.numel() >= nbytes:
            return
        cap = max(nbytes, 1 << 20)
        torch.cuda.synchronize(self.dev)               # a copy into the old buffers may be in flight (growth only: not the steady state)
        with torch.cuda.device(self.dev):
            self.mask_dev = torch.empty(cap, dtype=torch.uint8, device=self.dev)
            old, self.host = self.host, [torch.empty(cap, dtype=torch.uint8, pin_memory=True) for _ in range(self.nslots)]
        for o, h in zip(old, self.host):               # results not handed out yet move with their slot
            if o is not None:
                h[: o.numel()].copy_(o)

    def describe_channels(self) -> int:
        return _tap_channels(self.model, self.describe[1])

    def set_expressions(self, exprs: Sequence[Tuple[np.ndarray, int]]):
        torch = self.torch
        with torch.cuda.device(self.dev):
            self.words = [(torch.from_numpy(np.ascontiguousarray(ids[None])).to(self.dev), torch.full((1,), n, dtype=torch.int32).to(self.dev))
                          for ids, n in exprs]

    def _copy(self, levels, dst, src, nbytes, n, dst_idx, src_idx, dst_cap, src_cap, stream):
        _lib.call("cmpc_taps_copy", levels, dst, src, nbytes, n, dst_idx, src_idx, dst_cap, src_cap, stream.cuda_stream)

    def backbone(self, first: int, images: List[np.ndarray], n: int):
        """Upload, cmpc_eval_prep and one backbone pass of the B frames `images` (frames first .. first + n - 1 and the pads of a short
        last batch), then the taps of the n real frames into ring slots frame % ring; the batch's event behind them."""
        torch, m, C = self.torch, self.model, self.C
        descs, nbytes = plan_prep([a.shape for a in images], m.H, m.W)
        main = torch.cuda.current_stream(self.dev)
        bb = m.bb_stream if m.bb_stream is not None else main
        with torch.no_grad(), torch.cuda.device(self.dev):
            with torch.cuda.stream(bb):
                src = self.staging.upload(images, descs, nbytes)
                _lib.call("cmpc_eval_prep", src.data_ptr(), nbytes, descs, len(images), m.H, m.W, self.proc.data_ptr(), self.feed.data_ptr(),
                          bb.cuda_stream)
            feats, _ = m.features_async(self.feed)         # the backbone stream waits for the caller's stream here
            with torch.cuda.stream(bb):
                for j in range(n):
                    self._idx_a[j] = (first + j) % self.ring
                src_p = (C.c_void_p * 3)(*[t.data_ptr() for t in feats])
                self._copy(3, self._cache_p, src_p, self._bytes, n, self._idx_a, self._seq, self.ring, self.B, bb)
                if self.dcrf:
                    self._copy(1, (C.c_void_p * 1)(self.proc_ring.data_ptr()), (C.c_void_p * 1)(self.proc.data_ptr()), self._proc_bytes, n,
                               self._idx_a, self._seq, self.ring, self.B, bb)
                self.batch_ev[(first // self.B) % len(self.batch_ev)].record(bb)

    def gather(self, f: int, idx: Sequence[int]):
        """The cached taps of frames `idx` (sampled_frames(f)) into the head's inputs, once the newest batch among them is complete."""
        torch = self.torch
        main = torch.cuda.current_stream(self.dev)
        with torch.cuda.device(self.dev):
            main.wait_event(self.batch_ev[(max(idx) // self.B) % len(self.batch_ev)])
            for j, g in enumerate(idx):
                self._idx_b[j] = g % self.ring
            self._copy(3, self._gath_p, self._cache_p, self._bytes, len(idx), self._seq, self._idx_b, self.B, self.ring, main)

    def head(self, f: int, e: int, descs, slot: int, describe: Optional[DescribePlan] = None):
        """Head of expression e on the gathered taps of frame f; its mask into the device buffer at the offset of descs[e]; with
        `describe`, row e of the frame's describe tail: frame f's own tap among the gathered ones weighted by the head's sigm."""
        torch, m = self.torch, self.model
        words, sl = self.words[e]
        with torch.no_grad(), torch.cuda.device(self.dev):
            o = m.head_video(self.gathered, words, sl)
            if describe is not None:
                _enqueue_describe(self, self.gathered[self.describe[1]], self.own, o["sigm"].float().reshape(1, m.H, m.W).data_ptr(),
                                  o["score_c4"], o["score_c5"], describe, e, 1)
            if self.dcrf:
                from . import crf
                sigm = o["sigm"].float().reshape(1, m.H, m.W)
                k = f % self.ring
                score, thr = crf.dense_crf_batch(sigm, self.proc_ring[k: k + 1], device=self.dev, method=self.dcrf_method), 0.5
            else:
                score, thr = o[self.score].float().reshape(1, m.H, m.W), self.threshold
            dt = _lib.EVAL_F32 if score.dtype == torch.float32 else _lib.EVAL_U8
            _lib.call("cmpc_eval_mask_out", score.data_ptr(), dt, 1, m.H, m.W, float(thr), self.C.byref(descs[e]), self.mask_dev.data_ptr(),
                      self.mask_dev.numel(), self.value, torch.cuda.current_stream(self.dev).cuda_stream)

    def finish(self, f: int, slot: int, nbytes: int, jf: Optional[JfPlan] = None, describe: Optional[DescribePlan] = None,
               clean: Optional[CleanPlan] = None):
        """Frame f's masks (every expression) into pinned slot `slot`, its event behind the copy; with `jf`, their J / F counts
        behind them; with `describe`, the tail the frame's heads wrote behind those; with `clean`, the masks are cleaned in place
        first (so the counts score the cleaned masks) and their component statistics ride at the end."""
        torch = self.torch
        with torch.cuda.device(self.dev):
            if clean is not None:
                _enqueue_clean(self, clean, nbytes)
            if jf is not None:
                nbytes = _enqueue_scoring(self, jf, nbytes)
            if describe is not None:
                nbytes = describe.end
            if clean is not None:
                nbytes = clean.end
            self.host[slot][:nbytes].copy_(self.mask_dev[:nbytes], non_blocking=True)
            self.events[slot].record(torch.cuda.current_stream(self.dev))

    def done(self, slot: int) -> bool:
        return self.events[slot].query()

    def wait(self, slot: int):
        self.events[slot].synchronize()

    def view(self, slot: int) -> np.ndarray:
        return self.host[slot].numpy()


class ClipSegmenter:
    """The video model over a whole video: for every frame f and expression e what the video driver computes on f's clip
    (trainval_video.py:214-226 on the 16 frames of clip_window(f)), with each frame through the backbone once.

        seg = ClipSegmenter(model, vocab)
        for e, f, mask in seg.run(frames, expressions):        # frame by frame in order, within a frame the expressions in order

    frames: original-size uint8 arrays [h, w, 3] or [h, w], any iterable, read lazily (the video's length need not be known: frame f's
    heads go out once frame f + 7 was read or the video ended).  expressions: sentences (needs `vocab`) or (END-padded ids [T], seq_len)
    pairs -- the form head_video takes after model.video_words.  mask = value * (resize_and_crop(score >= threshold, *out_size(h, w)) > 0)
    with score = "up" (default, threshold 1e-9: trainval_video.py:225-226) or "sigm"; with dcrf the same resampling of the DenseCRF
    argmax on sigm and frame f's proc_im (trainval_video.py:227-240).

    Frames pass the backbone in consecutive batches of len(FRAME_IDX) = 5 (a short last batch padded with its first frame); their taps
    are kept in a ring of `ring` frames (slot = frame % ring) and each frame's clip is gathered from it by one cmpc_taps_copy.  A batch
    is enqueued `lookahead` batches ahead of the first head that needs it and only when every frame it evicts is older than
    f - frames // 2 for the oldest frame f whose heads are not all enqueued (min_ring).  depth: frames whose masks are in flight behind
    the one being handed out (depth + 1 pinned slots); copy=False yields views of the pinned slot, valid until the next iteration.
    stats after a run: {"frames": N, "backbone_passes": ceil(N / 5), "gathers": N, "heads": N * E}.

    run(..., ground_truth=fn, jf=None, seq=None) scores the masks on the device as FrameSegmenter.run does: fn(e, f) is called for
    e = 0 .. E - 1 when frame f's heads are enqueued, one cmpc_mask_jf call per frame scores its annotated expressions, and the counts
    reach `jf` (self.jf) under sequence (seq, e) and frame f.

    describe= / describe_weights= / run(..., pivots=) describe every (frame, expression) as FrameSegmenter does: behind each head
    cmpc_mask_pool pools frame f's own tap (position FRAME_IDX.index(frames // 2) of the gathered set) weighted by the head's sigm,
    "hard" weights being sigm >= threshold with score="sigm" and sigm >= 0.5 otherwise, and cmpc_level_agree counts the agreement of
    score_c4 and score_c5; they reach self.pivots under sequence (seq, e) and frame f (a second run() into the same log under the same
    seq raises, as in FrameSegmenter).

    clean= / run(..., cleaned=) clean every mask on the device as FrameSegmenter does: one cmpc_mask_components call per frame on its
    E masks, behind the heads' cmpc_eval_mask_out and before cmpc_mask_jf; the statistics reach self.cleaned under (seq, e), f.

    Mask propagation from pivot frames (FrameSegmenter's propagate= and propagate()) is out of scope here: the video model already
    sees five frames of a clip per answer, and its ring of cached taps evicts frames that a propagator would still read."""

    def __init__(self, model, vocab=None, score: str = "up", threshold: float = 1e-9, out_size: Callable[[int, int], Tuple[int, int]] = full_size,
                 value: int = 255, dcrf: bool = False, dcrf_method: str = "lattice", ring: int = 32, depth: int = 2, copy: bool = True,
                 _stage=None, lookahead: Optional[int] = None, describe: Optional[str] = None, describe_weights: str = "soft", clean=None):
        from .model import FRAME_IDX
        if not getattr(model, "video", False):
            raise ValueError("ClipSegmenter: expects the video model (CMPC_video_mm_tgraph_allvec); use FrameSegmenter for the image models")
        if score not in ("up", "sigm"):
            raise ValueError("score must be 'up' or 'sigm', got %r" % (score,))
        if value not in (1, 255):
            raise ValueError("value must be 1 or 255, got %r" % (value,))
        if int(depth) < 1:
            raise ValueError("depth must be >= 1, got %r" % (depth,))
        self.lookahead = CLIP_LOOKAHEAD if lookahead is None else int(lookahead)
        if self.lookahead < 0:
            raise ValueError("lookahead must be >= 0, got %r" % (lookahead,))
        self.frames, self.B = int(model.frames), len(FRAME_IDX)
        self.behind, self.ahead = _reach(self.frames)
        need = min_ring(self.frames, self.lookahead)
        if int(ring) < need:
            raise ValueError("ring = %r is smaller than min_ring(%d, %d) = %d" % (ring, self.frames, self.lookahead, need))
        self.model, self.vocab, self.score, self.threshold, self.out_size, self.value = model, vocab, score, float(threshold), out_size, int(value)
        self.dcrf, self.dcrf_method = bool(dcrf), _check_dcrf_method(dcrf_method)
        self.ring, self.depth, self.copy = int(ring), int(depth), bool(copy)
        self.T, self.H, self.W = model.num_steps, model.H, model.W
        self.nslots = self.depth + 1
        self.stats = {"frames": 0, "backbone_passes": 0, "gathers": 0, "heads": 0}
        self.jf, self.bound_th = None, 0.008
        self.describe, self.describe_weights, self.pivots = describe, describe_weights, None
        level = check_describe(model, describe, describe_weights)
        self.clean, self.cleaned = check_clean(clean), None
        kw = {} if level is None else {"describe": (describe_weights, level)}
        if self.clean is not None:
            kw["clean"] = True
        self.stage = _stage if _stage is not None else _ClipStage(model, self.ring, self.nslots, self.score, self.threshold, self.value, self.dcrf,
                                                                   self.dcrf_method, **kw)

    def _frame(self, f: int, im) -> Tuple[np.ndarray, Tuple[int, int]]:
        try:
            a = _images_u8([np.asarray(im)])[0]
        except ValueError as e:
            raise ValueError("frame %d: %s" % (f, str(e).split(": ", 1)[-1])) from None
        oh, ow = self.out_size(int(a.shape[0]), int(a.shape[1]))
        if int(oh) < 1 or int(ow) < 1:
            raise ValueError("frame %d: out_size(%d, %d) = (%d, %d) is empty" % (f, a.shape[0], a.shape[1], oh, ow))
        return a, (int(oh), int(ow))

    def run(self, frames: Iterable, expressions: Sequence, ground_truth: Optional[Callable] = None, jf: Optional[HU.JFEval] = None,
            seq=None, pivots: Optional[HU.PivotLog] = None, cleaned: Optional[HU.CleanLog] = None) -> Iterator[Tuple[int, int, np.ndarray]]:
        exprs = [check_expression(i, ex, self.vocab, self.T) for i, ex in enumerate(expressions)]
        if not exprs:
            raise ValueError("ClipSegmenter.run: no expressions")
        if self.clean is not None:
            self.cleaned = cleaned if cleaned is not None else HU.CleanLog()
        if ground_truth is not None:
            self.jf = jf if jf is not None else HU.JFEval()
        if len(exprs) > MAX_BATCH:
            raise ValueError("ClipSegmenter.run: %d expressions, at most %d per run" % (len(exprs), MAX_BATCH))
        st, B, E = self.stage, self.B, len(exprs)
        C = None                                   # channels of the described tap
        if self.describe is not None:
            self.pivots = pivots if pivots is not None else HU.PivotLog()
            C = st.describe_channels()
        stats = self.stats = {"frames": 0, "backbone_passes": 0, "gathers": 0, "heads": 0}
        free = deque(range(self.nslots))
        pending = deque()                          # (slot, frame, descs, scoring plan, describe plan) in enqueue order = yield order
        sizes = deque()                            # out sizes of the frames read whose heads are not enqueued yet
        it = iter(frames)
        st.set_expressions(exprs)
        read, ended, f = 0, False, 0               # frames handed to the backbone; the iterator ran out; oldest frame without its heads

        def hand_out(block: bool):
            while pending and (block or st.done(pending[0][0])):
                slot, fr, descs, plan, dplan, cplan = pending.popleft()
                st.wait(slot)
                host = st.view(slot)
                if cplan is not None:
                    for e, c in enumerate(slot_clean(host, cplan)):
                        self.cleaned.add((seq, e), fr, c)
                if plan is not None:
                    for e, c in zip(plan.idx, slot_counts(host, plan)):
                        self.jf.add((seq, e), fr, c)
                if dplan is not None:
                    for e, (iu, d, a) in enumerate(zip(*slot_describe(host, dplan))):
                        self.pivots.add((seq, e), fr, d, a, iu)
                for e, d in enumerate(descs):
                    mk = host[d.offset: d.offset + d.h * d.w].reshape(d.h, d.w)
                    yield e, fr, (mk.copy() if self.copy else mk)
                free.append(slot)                  # only now: the caller has moved past the slot's last mask
                block = False

        def next_batch():
            """Read up to B frames and enqueue their backbone pass; False once the video has ended."""
            nonlocal read, ended
            ims = []
            while len(ims) < B:
                im = next(it, it)
                if im is it:
                    ended = True
                    break
                a, size = self._frame(read + len(ims), im)
                ims.append(a)
                sizes.append(size)
            if not ims:
                return False
            # ring safety: every frame this batch evicts is older than anything a head not yet enqueued reads (min_ring)
            assert read + len(ims) - 1 - self.ring < f - self.behind, (read, f, self.ring)
            st.backbone(read, ims + [ims[0]] * (B - len(ims)), len(ims))
            read += len(ims)
            stats["backbone_passes"] += 1
            return True

        while True:
            # the batch that holds the newest frame of f's clip, and `lookahead` more
            want = (f + self.ahead) // B * B + B * (self.lookahead + 1)
            while not ended and read < want:
                next_batch()
            if read == 0:
                raise ValueError("ClipSegmenter.run: no frames")
            if f >= read:
                break
            # frame f + ahead was read, or the video ended and `read` is its length
            idx = sampled_frames(f, read, self.frames)
            descs, nbytes = plan_masks([sizes.popleft()] * E, self.H, self.W)
            tail = _slot_tail(nbytes, None if ground_truth is None else E, None if C is None else (E, C))
            st.reserve(tail if self.clean is None else cleaned_bytes(tail, E))
            if not free:
                yield from hand_out(True)
            slot = free.popleft()
            plan = None
            if ground_truth is not None:
                gts = [(e, ground_truth(e, f)) for e in range(E)]
                plan = plan_scoring(descs, [(e, check_ground_truth(e, f, g, (descs[e].h, descs[e].w))) for e, g in gts if g is not None],
                                    nbytes, self.bound_th)
            # head() and finish() keep their older call shapes while describe= (and ground_truth=) are off, as in FrameSegmenter.run
            dplan = None if C is None else plan_describe(nbytes, 0 if plan is None else plan.n, E, C)
            st.gather(f, idx)
            stats["gathers"] += 1
            for e in range(E):
                if dplan is None:
                    st.head(f, e, descs, slot)
                else:
                    st.head(f, e, descs, slot, describe=dplan)
                stats["heads"] += 1
            kw = {}
            if dplan is not None:
                kw = {"jf": plan, "describe": dplan}
            elif ground_truth is not None:
                kw = {"jf": plan}
            cplan = None
            if self.clean is not None:             # `clean` reaches the stage only when the option is on
                tail = dplan.end if dplan is not None else nbytes if plan is None else scored_bytes(nbytes, plan.n)
                cplan = kw["clean"] = CleanPlan(descs, self.clean, tail)
            st.finish(f, slot, nbytes, **kw)
            pending.append((slot, f, descs, plan, dplan, cplan))
            f += 1
            stats["frames"] = f
            yield from hand_out(False)
        while pending:
            yield from hand_out(True)
