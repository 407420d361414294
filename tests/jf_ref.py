"""NumPy restatement of the six integers cmpc_mask_jf returns (include/cmpc.h): the J and F measures of video object segmentation as the
DAVIS-2017 evaluation code defines them (db_eval_iou; f_measure with seg2bmap at the mask's own size and a disc of radius r).  That code
is not available to this project, so parity against it is unpinned; the window rule of `dilate` was checked once against
scipy.ndimage.binary_dilation with skimage's disk(r) footprint (identical counts on 24 cases).  TEST SCAFFOLDING, not product code."""
import math

import numpy as np


def bmap(seg) -> np.ndarray:
    """The boundary map of a mask [h, w] (non-zero = foreground) as bool [h, w]."""
    seg = np.asarray(seg) != 0
    e, s, se = np.zeros_like(seg), np.zeros_like(seg), np.zeros_like(seg)
    e[:, :-1] = seg[:, 1:]
    s[:-1, :] = seg[1:, :]
    se[:-1, :-1] = seg[1:, 1:]
    b = (seg ^ e) | (seg ^ s) | (seg ^ se)
    b[-1, :] = seg[-1, :] ^ e[-1, :]
    b[:, -1] = seg[:, -1] ^ s[:, -1]
    b[-1, -1] = False
    return b


def disc_offsets(r: int):
    return [(dy, dx) for dy in range(-r, r + 1) for dx in range(-r, r + 1) if dx * dx + dy * dy <= r * r]


def dilate(b: np.ndarray, r: int) -> np.ndarray:
    """Binary dilation by the disc dx^2 + dy^2 <= r^2: the OR of shifted copies, nothing entering from outside the image."""
    h, w = b.shape
    out = np.zeros_like(b)
    for dy in range(-min(r, h - 1), min(r, h - 1) + 1):
        hw = min(math.isqrt(r * r - dy * dy), w - 1)
        rows = b[max(dy, 0): h + min(dy, 0)]                       # out[y] |= b[y + dy]
        dst = out[max(-dy, 0): h + min(-dy, 0)]
        for dx in range(-hw, hw + 1):
            dst[:, max(-dx, 0): w + min(-dx, 0)] |= rows[:, max(dx, 0): w + min(dx, 0)]
    return out


def counts(pred, gt, r: int) -> np.ndarray:
    """int64 [6] = (I, U, n_pred, n_gt, pred_match, gt_match)."""
    p, g = np.asarray(pred) != 0, np.asarray(gt) != 0
    if p.shape != g.shape or p.ndim != 2:
        raise ValueError("counts: masks %s and %s" % (p.shape, g.shape))
    bp, bg = bmap(p), bmap(g)
    return np.array([(p & g).sum(), (p | g).sum(), bp.sum(), bg.sum(), (bp & dilate(bg, r)).sum(), (bg & dilate(bp, r)).sum()], dtype=np.int64)
