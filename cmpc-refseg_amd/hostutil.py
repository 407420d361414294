"""Host-side helpers around the hot path: what the reference's drivers do to a sample before
`sess.run` and to a mask after it.  Pure Python / NumPy, no GPU.

  tokeniser + padding   util/text_processing.py:9-67   (vocabulary file: one word per line, '<pad>' = line 0 and
                                                         '<unk>' present, e.g. data/vocabulary_Gref.txt)
  image feed            trainval_model.py:90-91,229-230,371   (RGB -> BGR, minus the channel means)
  mask IoU bookkeeping  util/eval_tools.py:31-35, trainval_model.py:267-296   (I/U, cumulative IoU, precision@X)
  video valid_idx       CMPC_video/trainval_video.py:191-197   (first non-pad position of the front-padded ids)

Resizing (util/im_processing.py:7-41) goes through scikit-image in the reference (third-party, not installed here, and its
`resize` defaults changed between releases).  `resize_and_pad_geometry` / `resize_and_crop_geometry` return the geometry those
functions compute (pinned by hand-worked cases); `resize_and_pad` / `resize_and_crop` fill it with a restatement of
`skimage.transform.resize` as scikit-image >= 0.19 documents it (order 1, mode "reflect", anti-aliasing Gaussian when shrinking,
uint8 scaled to [0, 1]) on scipy.ndimage -- the resampled pixel values are PARITY-UNPINNED (no scikit-image to compare with).
`skimage_like_resize` resamples a bool image like a float one (order 1); `resize_and_pad_order0` is the order-0 rule scikit-image >= 0.19
documents for bool input, equally parity-unpinned.  `train_sample` is the training reader's per-sample work on both
(util/data_reader_refvos.py:27-46).
"""
from __future__ import annotations

import re
from typing import Dict, List, Sequence, Tuple

import numpy as np

MU = np.array((104.00698793, 116.66876762, 122.67891434))          # trainval_model.py:371 (B, G, R)
UNK, PAD = "<unk>", "<pad>"
_SPLIT = re.compile(r"(\W+)")


def load_vocab_dict_from_file(path: str) -> Dict[str, int]:
    """word -> line number (util/text_processing.py:9-13)."""
    with open(path) as f:
        return {w.strip(): i for i, w in enumerate(f.readlines())}


def sentence2vocab_indices(sentence: str, vocab: Dict[str, int]) -> List[int]:
    """Split on runs of non-word characters (the separators are kept as tokens unless blank), lower-case, drop one
    trailing '.', map unknown tokens to '<unk>' (util/text_processing.py:17-25)."""
    toks = [t.lower() for t in _SPLIT.split(sentence.strip()) if t.strip()]
    if toks and toks[-1] == ".":
        toks = toks[:-1]
    unk = vocab[UNK]
    return [vocab.get(t, unk) for t in toks]


def preprocess_sentence_lstm(sentence: str, vocab: Dict[str, int], T: int) -> Tuple[List[int], int]:
    """The form CMPC_model is fed with (test.py:267): truncate to T, pad AT THE END with '<pad>', return the ids and the
    unpadded length = `seq_len` (util/text_processing.py:55-67)."""
    ids = sentence2vocab_indices(sentence, vocab)[:T]
    n = len(ids)
    return ids + [vocab[PAD]] * (T - n), n


def preprocess_sentence(sentence: str, vocab: Dict[str, int], T: int) -> List[int]:
    """Front-padded variant used by the non-LSTM readers (util/text_processing.py:42-53)."""
    ids = sentence2vocab_indices(sentence, vocab)[:T]
    return [vocab[PAD]] * (T - len(ids)) + ids


def image_feed(rgb: np.ndarray, mu: Sequence[float] = MU) -> np.ndarray:
    """uint8/float RGB [H,W,3] (or [B,H,W,3]) -> float32 BGR minus the per-channel means (trainval_model.py:90-91)."""
    return (np.asarray(rgb, dtype=np.float32)[..., ::-1] - np.asarray(mu, dtype=np.float32)).astype(np.float32)


def resize_and_pad_geometry(im_h: int, im_w: int, out_h: int, out_w: int) -> Tuple[int, int, int, int]:
    """(resized_h, resized_w, pad_top, pad_left) of im_processing.resize_and_pad (util/im_processing.py:7-23)."""
    scale = min(out_h / im_h, out_w / im_w)
    rh, rw = int(np.round(im_h * scale)), int(np.round(im_w * scale))
    return rh, rw, int(np.floor(out_h - rh) / 2), int(np.floor(out_w - rw) / 2)


def resize_and_crop_geometry(im_h: int, im_w: int, out_h: int, out_w: int) -> Tuple[int, int, int, int]:
    """(resized_h, resized_w, crop_top, crop_left) of im_processing.resize_and_crop (util/im_processing.py:25-41)."""
    scale = max(out_h / im_h, out_w / im_w)
    rh, rw = int(np.round(im_h * scale)), int(np.round(im_w * scale))
    return rh, rw, int(np.floor(rh - out_h) / 2), int(np.floor(rw - out_w) / 2)


def skimage_like_resize(im: np.ndarray, out_h: int, out_w: int) -> np.ndarray:
    """skimage.transform.resize(im, [out_h, out_w]) as scikit-image >= 0.19 documents its defaults: integer images become floats in
    [0, 1] (img_as_float), bilinear (order=1), mode="reflect" (numpy.pad's: ndimage "mirror"), anti_aliasing on when an axis shrinks
    (Gaussian, sigma = (scale - 1) / 2 per shrinking axis), pixel-area grid (ndimage.zoom grid_mode=True); channels are not resized.
    Parity-unpinned (module header)."""
    from scipy import ndimage as ndi
    a = np.asarray(im)
    if a.dtype == np.bool_:
        a = a.astype(np.float64)
    elif np.issubdtype(a.dtype, np.integer):
        a = a.astype(np.float64) / float(np.iinfo(a.dtype).max)
    else:
        a = a.astype(np.float64)
    h, w = a.shape[:2]
    if (h, w) == (out_h, out_w):
        return a
    factors = (h / out_h, w / out_w)
    extra = (1,) * (a.ndim - 2)
    if max(factors) > 1:
        sigma = tuple(max(0.0, (f - 1) / 2) for f in factors) + (0,) * (a.ndim - 2)
        a = ndi.gaussian_filter(a, sigma, mode="mirror")
    return ndi.zoom(a, (out_h / h, out_w / w) + extra, order=1, mode="mirror", grid_mode=True)


def resize_and_pad(im: np.ndarray, input_h: int, input_w: int) -> np.ndarray:
    """im_processing.resize_and_pad (util/im_processing.py:7-23): aspect-preserving resize to fit, centred on a zero canvas."""
    rh, rw, top, left = resize_and_pad_geometry(im.shape[0], im.shape[1], input_h, input_w)
    r = skimage_like_resize(im, rh, rw)
    out = np.zeros((input_h, input_w) + r.shape[2:], dtype=r.dtype)
    out[top: top + rh, left: left + rw, ...] = r
    return out


def resize_and_crop(im: np.ndarray, input_h: int, input_w: int) -> np.ndarray:
    """im_processing.resize_and_crop (util/im_processing.py:25-41): aspect-preserving resize to cover, centre crop."""
    rh, rw, top, left = resize_and_crop_geometry(im.shape[0], im.shape[1], input_h, input_w)
    r = skimage_like_resize(im, rh, rw)
    return np.ascontiguousarray(r[top: top + input_h, left: left + input_w, ...])


def compute_mask_IU(masks: np.ndarray, target: np.ndarray) -> Tuple[int, int]:
    """|masks AND target|, |masks OR target| (util/eval_tools.py:31-35)."""
    if masks.shape[-2:] != target.shape[-2:]:
        raise ValueError("mask and target sizes differ: %s vs %s" % (masks.shape, target.shape))
    return int(np.logical_and(masks, target).sum()), int(np.logical_or(masks, target).sum())


class SegEval:
    """The evaluation loop's running numbers (trainval_model.py:198-203,267-296): cumulative I and U, per-sample IoU
    mean, and precision@{.5,.6,.7,.8,.9}."""

    def __init__(self, thresholds: Sequence[float] = (.5, .6, .7, .8, .9)):
        self.thresholds = tuple(thresholds)
        self.cum_I = self.cum_U = 0
        self.sum_iou, self.total = 0.0, 0
        self.correct = np.zeros(len(self.thresholds), dtype=np.int64)

    def add(self, pred_mask: np.ndarray, gt_mask: np.ndarray) -> Tuple[int, int]:
        I, U = compute_mask_IU(pred_mask, gt_mask)
        iou = float(I) / U
        self.cum_I += I
        self.cum_U += U
        self.sum_iou += iou
        self.correct += np.array([iou >= t for t in self.thresholds])
        self.total += 1
        return I, U

    def result(self) -> Dict[str, float]:
        out = {"precision@%s" % t: float(c) / self.total for t, c in zip(self.thresholds, self.correct)}
        out["overall_IoU"] = self.cum_I / self.cum_U
        out["mean_IoU"] = self.sum_iou / self.total
        return out


def img_as_ubyte(x: np.ndarray) -> np.ndarray:
    """skimage.img_as_ubyte of a float image as scikit-image >= 0.19 documents it: values must lie in [-1, 1]; x * 255 in float64,
    rounded half to even, clipped to [0, 255] (negative values become 0).  Parity-unpinned like the resize restatement above."""
    a = np.asarray(x)
    if not np.issubdtype(a.dtype, np.floating):
        raise ValueError("img_as_ubyte: expected a float image, got %s" % a.dtype)
    if a.size and (np.min(a) < -1.0 or np.max(a) > 1.0):
        raise ValueError("img_as_ubyte: images of type float must be between -1 and 1")
    out = np.multiply(a, 255, dtype=np.float64)
    np.rint(out, out=out)
    np.clip(out, 0, 255, out=out)
    return out.astype(np.uint8)


def end_padded(text_front_padded, pad: int = 0) -> Tuple[np.ndarray, np.ndarray]:
    """The batches' `text_batch` (front-padded by preprocess_sentence, build_batches.py:70) -> the form CMPC_model is fed with
    (test.py:267): END-padded int32 ids and int32 `seq_len`.  Accepts [T] or [B, T]; the leading run of `pad` ids is the padding.
    An all-pad row (an empty sentence) raises ValueError: the text LSTM needs at least one word (seq_len >= 1)."""
    a = np.asarray(text_front_padded)
    if a.ndim not in (1, 2) or not np.issubdtype(a.dtype, np.integer) or a.shape[-1] == 0:
        raise ValueError("end_padded: expected integer ids [T] or [B, T], got %s %s" % (a.dtype, a.shape))
    rows = a.reshape(-1, a.shape[-1])
    T = rows.shape[1]
    ids = np.full(rows.shape, pad, dtype=np.int32)
    seq_len = np.zeros(rows.shape[0], dtype=np.int32)
    for i, r in enumerate(rows):
        nz = np.flatnonzero(r != pad)
        if nz.size == 0:
            raise ValueError("end_padded: row %d holds only pad ids (empty sentence)" % i)
        n = T - int(nz[0])
        ids[i, :n] = r[nz[0]:]
        seq_len[i] = n
    if a.ndim == 1:
        return ids[0], seq_len[0]
    return ids, seq_len


def first_valid_idx(text_front_padded, pad: int = 0) -> int:
    """The video driver's `valid_idx` (trainval_video.py:191-197): the index of the first non-pad id of a front-padded sentence [T],
    0 when every id is a pad (the driver's loop then never assigns it)."""
    a = np.asarray(text_front_padded)
    if a.ndim != 1 or not np.issubdtype(a.dtype, np.integer):
        raise ValueError("first_valid_idx: expected integer ids [T], got %s %s" % (a.dtype, a.shape))
    nz = np.flatnonzero(a != pad)
    return int(nz[0]) if nz.size else 0


# ---- the training reader's per-sample work (util/data_reader_refvos.py:27-46, build_batches.py:62-75) -----------------------------------
def object_mask(annotation, key=None, match: int = 1) -> np.ndarray:
    """The object of one annotation as bool [h, w].  key given: a colour-coded annotation uint8 [h, w, 3|4] (alpha ignored,
    data_reader_refvos.py:64); the object is where the first `match` channels equal the key's.  match=1 is the reference's rule,
    `(mask == mask_color)[:, :, 0]` (data_reader_refvos.py:30): channel 0 alone decides; match=3 asks for all of R, G, B.
    key None: a plain mask [h, w] (or [h, w, 1]) of any dtype, non-zero = object."""
    a = np.asarray(annotation)
    if key is None:
        if a.ndim == 3 and a.shape[2] == 1:
            a = a[:, :, 0]
        if a.ndim != 2 or a.shape[0] == 0 or a.shape[1] == 0:
            raise ValueError("plain mask: expected [h, w] with h, w > 0, got %s" % (a.shape,))
        return a != 0
    k = np.asarray(key).reshape(-1)
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] not in (3, 4) or a.shape[0] == 0 or a.shape[1] == 0:
        raise ValueError("colour-coded annotation: expected uint8 [h, w, 3|4] with h, w > 0, got %s %s" % (a.dtype, a.shape))
    if k.size < 3 or match not in (1, 2, 3) or np.any(k[:3] < 0) or np.any(k[:3] > 255):
        raise ValueError("key colour must hold R, G, B in 0..255 and match must be 1, 2 or 3, got %s, %s" % (key, match))
    return np.all(a[:, :, :match] == k[:match].astype(np.uint8), axis=2)


def resize_and_pad_order0(mask: np.ndarray, input_h: int, input_w: int) -> np.ndarray:
    """resize_and_pad of a BOOL image as scikit-image >= 0.19 documents resize for that dtype: order 0, no anti-aliasing, i.e. the source
    sample nearest each pixel-area grid coordinate (ndimage.zoom order 0, mode "mirror", grid_mode).  skimage_like_resize above keeps
    resampling a bool like a float (order 1); both are parity-unpinned against scikit-image itself (module header)."""
    from scipy import ndimage as ndi
    m = np.asarray(mask, dtype=bool)
    h, w = m.shape
    rh, rw, top, left = resize_and_pad_geometry(h, w, input_h, input_w)
    r = m if (h, w) == (rh, rw) else ndi.zoom(m.astype(np.uint8), (rh / h, rw / w), order=0, mode="mirror", grid_mode=True) != 0
    if r.shape != (rh, rw):
        raise ValueError("resize_and_pad_order0: zoom gave %s for (%d, %d)" % (r.shape, rh, rw))
    out = np.zeros((input_h, input_w), dtype=bool)
    out[top: top + rh, left: left + rw] = r
    return out


def train_sample(image, annotation, key, H: int, W: int, order: int = 1, match: int = 1) -> Tuple[np.ndarray, np.ndarray]:
    """preprocess_data's two tensors for one raw sample (data_reader_refvos.py:27-46) as the train step is fed with them
    (trainval_model.py:90-91): im float32 [H, W, 3] = img_as_ubyte(resize_and_pad(image))[..., ::-1] - mu (a grey image tiled to three
    channels, build_batches.py:67-68) and target_fine float32 [H, W, 1] in {0, 1} = resize_and_pad(mask_obj) > 0.  order 1 resamples the
    object mask like a float image (resize_and_pad above), order 0 as a bool image (resize_and_pad_order0)."""
    if order not in (0, 1):
        raise ValueError("order must be 0 or 1, got %r" % (order,))
    im = np.asarray(image)
    if im.dtype != np.uint8:
        raise ValueError("image: expected uint8, got %s" % im.dtype)
    proc = img_as_ubyte(resize_and_pad(im, H, W))
    if proc.ndim == 2 or proc.shape[2] == 1:
        proc = np.repeat(proc.reshape(H, W, 1), 3, 2)
    feed = proc[..., ::-1].astype(np.float32)
    feed -= MU
    obj = object_mask(annotation, key, match)
    tgt = resize_and_pad(obj, H, W) > 0 if order == 1 else resize_and_pad_order0(obj, H, W)
    return feed, tgt.astype(np.float32)[..., None]


# ---- the train loops' accuracy lines (test.py:94-127, CMPC_video/trainval_video.py:93-123) ---------------------------------------------
def accuracy_counts(scores, labels) -> np.ndarray:
    """int64 [4] = (n_pos, n_neg, correct_pos, correct_neg): the integer sums compute_accuracy divides (what cmpc_train_accuracy
    returns per sample)."""
    s, l = np.asarray(scores), np.asarray(labels)
    if s.shape != l.shape:
        raise ValueError("scores %s and labels %s differ in shape" % (s.shape, l.shape))
    is_pos = l != 0
    is_neg = np.logical_not(is_pos)
    is_correct = np.logical_xor(s < 0, is_pos)
    return np.array([is_pos.sum(), is_neg.sum(), is_correct[is_pos].sum(), is_correct[is_neg].sum()], dtype=np.int64)


def _accuracy(n_pos: int, n_neg: int, c_pos: int, c_neg: int) -> Tuple[float, float, float]:
    n_all = n_pos + n_neg
    return ((c_pos + c_neg) / n_all if n_all else float("nan"), c_pos / (n_pos + 1), c_neg / n_neg if n_neg else float("nan"))


def compute_accuracy(scores, labels) -> Tuple[float, float, float]:
    """(accuracy_all, accuracy_pos, accuracy_neg) of processing_tools.compute_accuracy (util/processing_tools.py:24-35): a pixel is
    positive where labels != 0 and right where (scores < 0) XOR positive.  accuracy_pos keeps the reference's / (num_pos + 1);
    accuracy_neg is nan when there is no negative pixel (the reference's 0 / 0)."""
    return _accuracy(*(int(v) for v in accuracy_counts(scores, labels)))


def accuracy_from_counts(counts) -> Tuple[float, float, float]:
    """compute_accuracy's three fractions from integer counts [B, 4] (or [4]) of (n_pos, n_neg, correct_pos, correct_neg), summed over
    the batch: compute_accuracy over the whole batch's pixels, the same integer sums and one float64 division each."""
    c = np.asarray(counts.cpu() if hasattr(counts, "cpu") else counts)
    if c.ndim not in (1, 2) or c.shape[-1] != 4 or not np.issubdtype(c.dtype, np.integer):
        raise ValueError("counts: expected integers [B, 4] or [4], got %s %s" % (c.dtype, c.shape))
    return _accuracy(*(int(v) for v in c.reshape(-1, 4).sum(axis=0)))


class TrainLog:
    """The train loops' running numbers and log lines (CMPC_video/trainval_video.py:102-121; test.py:107-127 prints the same):

        log = TrainLog(iters_per_log=100)
        for n_iter in range(max_iter):
            step, scal = feeder.step(accuracy=True)
            log.add(n_iter, scal["loss_last"], scal["learning_rate"], scal["accuracy_counts"])
            for line in log.lines(n_iter): print(line)

    add() only stores what it is given: device tensors are not read, so nothing synchronises per step.  lines(n_iter) returns the three
    lines when n_iter % iters_per_log == 0 (else none); the stored values are read then, or on flush(), and the 0.99-decay averages
    (cls_loss_avg, avg_accuracy_all / pos / neg, all starting at 0) are replayed on the host in float64 in step order -- the per-step
    loop's result.  `loss` stands for model.cls_loss (the `loss_last` scalar), `counts` for compute_accuracy's integer sums [B, 4]."""

    def __init__(self, iters_per_log: int = 100, decay: float = 0.99):
        if iters_per_log < 1:
            raise ValueError("iters_per_log must be >= 1, got %r" % (iters_per_log,))
        self.iters_per_log, self.decay = int(iters_per_log), float(decay)
        self.cls_loss_avg = 0.0
        self.avg_accuracy_all = self.avg_accuracy_pos = self.avg_accuracy_neg = 0.0
        self.last = None                             # (n_iter, loss, lr, accuracy_all, accuracy_pos, accuracy_neg) of the last step replayed
        self._pending: List[tuple] = []

    def add(self, n_iter: int, loss, lr, counts):
        self._pending.append((n_iter, loss, lr, counts))

    def flush(self):
        """Read every stored step (this is where device values cross to the host) and fold it into the averages, in step order."""
        d = self.decay
        for n_iter, loss, lr, counts in self._pending:
            loss, lr = float(loss), float(lr)
            a, p, n = accuracy_from_counts(counts)
            self.cls_loss_avg = d * self.cls_loss_avg + (1 - d) * loss
            self.avg_accuracy_all = d * self.avg_accuracy_all + (1 - d) * a
            self.avg_accuracy_pos = d * self.avg_accuracy_pos + (1 - d) * p
            self.avg_accuracy_neg = d * self.avg_accuracy_neg + (1 - d) * n
            self.last = (n_iter, loss, lr, a, p, n)
        self._pending = []

    def lines(self, n_iter: int) -> List[str]:
        if n_iter % self.iters_per_log != 0:
            return []
        self.flush()
        if self.last is None or self.last[0] != n_iter:
            raise ValueError("TrainLog.lines(%d): that step was not added" % n_iter)
        _, loss, lr, a, p, n = self.last
        return ['iter = %d, loss (cur) = %f, loss (avg) = %f, lr = %f' % (n_iter, loss, self.cls_loss_avg, lr),
                'iter = %d, accuracy (cur) = %f (all), %f (pos), %f (neg)' % (n_iter, a, p, n),
                'iter = %d, accuracy (avg) = %f (all), %f (pos), %f (neg)' % (n_iter, self.avg_accuracy_all, self.avg_accuracy_pos, self.avg_accuracy_neg)]


# ---- J and F of video object segmentation (the ranking of Refer-YouTube-VOS and Refer-DAVIS) -------------------------------------------
# Restated from the DAVIS-2017 evaluation code (db_eval_iou, f_measure, db_statistics), which neither the reference nor this project
# holds a copy of: parity against it is UNPINNED.  The integer counts come from cmpc_mask_jf (evaluate.mask_jf, the segmenters).
JF_KEYS = ("J_mean", "J_recall", "J_decay", "F_mean", "F_recall", "F_decay")


def jf_radius(h: int, w: int, bound_th: float = 0.008) -> int:
    """f_measure's dilation radius in pixels: bound_th itself when it is >= 1 (a whole number of pixels), else
    ceil(bound_th * sqrt(h^2 + w^2)) in float64 -- 12 at 720 x 1280."""
    if h < 1 or w < 1 or not bound_th > 0:
        raise ValueError("jf_radius: mask %r x %r, bound_th %r" % (h, w, bound_th))
    if bound_th >= 1:
        if bound_th != int(bound_th):
            raise ValueError("jf_radius: bound_th %r >= 1 must be a whole number of pixels" % (bound_th,))
        return int(bound_th)
    return int(np.ceil(np.float64(bound_th) * np.sqrt(np.float64(h) * h + np.float64(w) * w)))


def jf_from_counts(c) -> Tuple[float, float]:
    """(J, F) in float64 from one sample's (I, U, n_pred, n_gt, pred_match, gt_match).  J = I / U, 1 when both masks are empty.
    Precision = pred_match / n_pred and recall = gt_match / n_gt, with f_measure's rules for an empty boundary map: (1, 0) when only
    the prediction's is empty, (0, 1) when only the ground truth's, (1, 1) when both; F = 2 P R / (P + R), 0 when P + R = 0."""
    I, U, n_pred, n_gt, pm, gm = (int(v) for v in np.asarray(c).reshape(6))
    J = 1.0 if U == 0 else I / U
    if n_pred == 0 and n_gt > 0:
        P, R = 1.0, 0.0
    elif n_gt == 0 and n_pred > 0:
        P, R = 0.0, 1.0
    elif n_pred == 0 and n_gt == 0:
        P, R = 1.0, 1.0
    else:
        P, R = pm / n_pred, gm / n_gt
    return J, (0.0 if P + R == 0 else 2 * P * R / (P + R))


def jf_decay_bins(n: int) -> List[Tuple[int, int]]:
    """db_statistics' four bins of a sequence of n frames as (first, last) frame positions, both inclusive: the edges are
    round(linspace(1, n, 5) + 1e-10) - 1 and bin i runs from edge i to edge i + 1."""
    ids = (np.round(np.linspace(1, n, 5) + 1e-10) - 1).astype(np.int64)
    return [(int(ids[i]), int(ids[i + 1])) for i in range(4)]


def _jf_stats(v: np.ndarray) -> Tuple[float, float, float]:
    """db_statistics: mean, recall (share of frames > 0.5) and decay (first bin's mean minus the last bin's) of per-frame values."""
    bins = jf_decay_bins(len(v))
    (a0, a1), (b0, b1) = bins[0], bins[3]
    return float(np.mean(v)), float(np.mean(v > 0.5)), float(np.mean(v[a0: a1 + 1]) - np.mean(v[b0: b1 + 1]))


class JFEval:
    """Per-sequence J and F, as the benchmarks average them: a sequence is one (video, expression) pair.

        jf = JFEval(); jf.add(seq, frame, counts) ...; jf.result()

    counts: the six integers of cmpc_mask_jf for that frame.  result() -> {"J_mean", "J_recall", "J_decay", "F_mean", "F_recall",
    "F_decay"} averaged over the sequences (each sequence's statistics over its frames in frame order, _jf_stats), "J&F" =
    (J_mean + F_mean) / 2, "sequences", "frames", and "per_sequence": {seq: the six statistics and "frames"}."""

    def __init__(self):
        self.seqs: Dict[object, Dict[int, Tuple[float, float]]] = {}

    def add(self, seq, frame: int, counts):
        frames = self.seqs.setdefault(seq, {})
        if frame in frames:
            raise ValueError("JFEval.add: sequence %r already holds frame %r" % (seq, frame))
        frames[frame] = jf_from_counts(counts)

    def result(self) -> Dict[str, object]:
        if not self.seqs:
            raise ValueError("JFEval.result: no frames")
        per = {}
        for seq, frames in self.seqs.items():
            jf = np.array([frames[f] for f in sorted(frames)], dtype=np.float64)
            per[seq] = dict(zip(JF_KEYS, _jf_stats(jf[:, 0]) + _jf_stats(jf[:, 1])), frames=len(frames))
        out: Dict[str, object] = {k: float(np.mean([p[k] for p in per.values()])) for k in JF_KEYS}
        out["J&F"] = (out["J_mean"] + out["F_mean"]) / 2
        out["sequences"], out["frames"], out["per_sequence"] = len(per), sum(p["frames"] for p in per.values()), per
        return out


# ---- pivot frames (test.py:150-181) and the per-frame consistency of two levels (test.py:289,301-302; util/loss.py:51-68) ---------------
# find_pivot_frames restates the reference's function with its two crashes repaired -- its row normalisation broadcasts [F, C] / [F],
# and `avail_frame[a:b] = False` assigns a scalar to a list slice -- and nothing else changed.  The reference's function cannot run, so
# parity against it is UNPINNED.  The descriptors and counts come from cmpc_mask_pool / cmpc_level_agree (evaluate.mask_pool,
# evaluate.level_agree, the segmenters' describe=).
def find_pivot_frames(descriptors, num_propagate: int = 2, nearest_first: bool = False) -> List[int]:
    """The frames a mask propagator would start from, as 0-based row indices of `descriptors` [F, C] (one global feature per frame).
    Rows are normalised in float64 (a zero row stays zero: its similarity to everything is 0); S = the cosine similarities;
    first = argmax of S.sum(0) (first occurrence); the frames are tried in the order of a stable argsort of S[first] -- ascending as the
    reference writes it, so the frame LEAST like `first` is tried first and `first` itself last; nearest_first=True tries them in
    the descending order (a stable argsort of -S[first]) -- and a frame is taken if it is still available, after which the frames
    [f - num_propagate, f + num_propagate] are not.  No two pivots lie within num_propagate of each other and every frame lies
    within num_propagate of a pivot."""
    d = np.asarray(descriptors, dtype=np.float64)
    if d.ndim != 2 or d.shape[0] < 1:
        raise ValueError("find_pivot_frames: descriptors must be [F, C] with F >= 1, got %s" % (d.shape,))
    p = int(num_propagate)
    if p < 0:
        raise ValueError("find_pivot_frames: num_propagate %r < 0" % (num_propagate,))
    F = d.shape[0]
    norm = np.linalg.norm(d, axis=1, keepdims=True)
    dn = np.divide(d, norm, out=np.zeros_like(d), where=norm > 0)
    S = dn @ dn.T
    first = int(np.argmax(S.sum(0)))
    to_first = S[first]
    order = np.argsort(-to_first if nearest_first else to_first, kind="stable")
    avail, out = [True] * F, []
    for f in order:
        f = int(f)
        if avail[f]:
            out.append(f)
            lo, hi = max(f - p, 0), min(f + p + 1, F)
            avail[lo:hi] = [False] * (hi - lo)
    return out


def consistency(I, U) -> float:
    """loss.iou_with_threshold from its two counts: I / U, NaN when U == 0 (0 / 0 there; test.py:301 guards with math.isnan)."""
    I, U = int(I), int(U)
    return float("nan") if U == 0 else I / U


class PivotLog:
    """What the segmenters' describe= collects, per sequence (one (video, expression) pair):

        log = PivotLog(); log.add(seq, frame, desc, area, (I, U)) ...; log.pivots(seq); log.inconsistent(); log.meta()

    desc: the frame's float32 descriptor [C] (cmpc_mask_pool); area: the sum of its weights; (I, U): cmpc_level_agree's counts."""

    def __init__(self):
        self.seqs: Dict[object, Dict[int, Tuple[np.ndarray, float, float]]] = {}

    def add(self, seq, frame: int, desc, area, iu):
        frames = self.seqs.setdefault(seq, {})
        if frame in frames:
            raise ValueError("PivotLog.add: sequence %r already holds frame %r" % (seq, frame))
        I, U = (int(v) for v in np.asarray(iu).reshape(2))
        frames[frame] = (np.array(desc, dtype=np.float32).reshape(-1), float(area), consistency(I, U))

    def __len__(self) -> int:
        return sum(len(f) for f in self.seqs.values())

    def _frames(self, seq) -> Dict[int, Tuple[np.ndarray, float, float]]:
        if seq not in self.seqs:
            raise KeyError("PivotLog: no sequence %r" % (seq,))
        return self.seqs[seq]

    def descriptors(self, seq) -> Tuple[np.ndarray, List[int]]:
        """([F, C] float32 in frame order, the frame ids)."""
        frames = self._frames(seq)
        ids = sorted(frames)
        return np.stack([frames[f][0] for f in ids]), ids

    def areas(self, seq) -> np.ndarray:
        frames = self._frames(seq)
        return np.array([frames[f][1] for f in sorted(frames)], dtype=np.float64)

    def consistencies(self, seq) -> np.ndarray:
        """I / U per frame in frame order, NaN where both levels are empty."""
        frames = self._frames(seq)
        return np.array([frames[f][2] for f in sorted(frames)], dtype=np.float64)

    def pivots(self, seq, num_propagate: int = 2, nearest_first: bool = False) -> List[int]:
        """find_pivot_frames on the sequence's descriptors, as frame ids."""
        d, ids = self.descriptors(seq)
        return [ids[i] for i in find_pivot_frames(d, num_propagate, nearest_first)]

    def inconsistent(self, below: float = 0.3) -> List[Tuple[object, int]]:
        """(seq, frame) of every frame whose consistency is below `below` (test.py:301-302); never a NaN one."""
        return [(seq, f) for seq, frames in self.seqs.items() for f in sorted(frames) if frames[f][2] < below]

    def meta(self, num_propagate: int = 2, nearest_first: bool = False) -> Dict[object, List[int]]:
        """{seq: pivots}: the content of test.py's meta_pivot_frames."""
        return {seq: self.pivots(seq, num_propagate, nearest_first) for seq in self.seqs}


def propagation_plan(frame_ids: Sequence[int], pivots: Sequence[int], num_propagate: int = 2, max_sources: int = 4) -> Dict[int, List[int]]:
    """Who receives from whom when masks are propagated from pivot frames: {frame: [pivot, ...]} for every frame of `frame_ids` that
    is no pivot and has a pivot within num_propagate positions of it IN frame_ids (the list's order is the video's; the ids need not
    be consecutive).  A frame's pivots come nearest first, a tie going to the lower frame id, at most max_sources of them; a frame
    out of reach of every pivot is left out (find_pivot_frames leaves none when it ran with the same num_propagate).  ValueError for
    a pivot that is not in frame_ids, a repeated frame id, num_propagate < 0 or max_sources < 1."""
    ids = [int(f) for f in frame_ids]
    p, k = int(num_propagate), int(max_sources)
    if p < 0 or k < 1:
        raise ValueError("propagation_plan: num_propagate %r must be >= 0 and max_sources %r >= 1" % (num_propagate, max_sources))
    pos = {f: i for i, f in enumerate(ids)}
    if len(pos) != len(ids):
        raise ValueError("propagation_plan: frame_ids holds a frame twice")
    piv = sorted(set(int(f) for f in pivots))
    for f in piv:
        if f not in pos:
            raise ValueError("propagation_plan: pivot %r is not among the %d frame ids" % (f, len(ids)))
    is_pivot = set(piv)
    plan: Dict[int, List[int]] = {}
    for f in ids:
        if f in is_pivot:
            continue
        near = sorted((abs(pos[g] - pos[f]), g) for g in piv if abs(pos[g] - pos[f]) <= p)
        if near:
            plan[f] = [g for _, g in near[:k]]
    return plan


# ---- cleaning masks by their connected components (the host twin of cmpc_mask_components: evaluate.mask_clean, the segmenters' clean=) --
CLEAN_MAX_KEEP = 8             # CMPC_CC_MAX_KEEP
CLEAN_STATS = ("n_components", "area", "area_largest", "area_kept")


def check_clean(keep, min_area, connectivity) -> Tuple[int, int, int]:
    """(keep, min_area, connectivity) as integers; ValueError outside keep 0..8, min_area >= 0, connectivity 4 | 8."""
    for name, v in (("keep", keep), ("min_area", min_area), ("connectivity", connectivity)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise ValueError("%s must be an integer, got %r" % (name, v))
    if not 0 <= keep <= CLEAN_MAX_KEEP:
        raise ValueError("keep = %r outside 0..%d" % (keep, CLEAN_MAX_KEEP))
    if min_area < 0:
        raise ValueError("min_area = %r is negative" % (min_area,))
    if connectivity not in (4, 8):
        raise ValueError("connectivity must be 4 or 8, got %r" % (connectivity,))
    return int(keep), int(min_area), int(connectivity)


def clean_mask(mask, keep: int = 1, min_area: int = 0, connectivity: int = 8) -> Tuple[np.ndarray, np.ndarray]:
    """cmpc_mask_components' rule on scipy.ndimage.label: components of the non-zero pixels of `mask` [h, w], ranked by area
    descending with ties to the component whose first pixel comes first in raster order (SciPy numbers components in that order, so
    a stable sort by area keeps it); one is kept iff (keep == 0 or rank < keep) and area >= min_area.  Returns (a new mask: kept
    pixels keep their value, the rest 0; int64 stats {n_components, area, area_largest, area_kept})."""
    from scipy import ndimage
    keep, min_area, connectivity = check_clean(keep, min_area, connectivity)
    a = np.asarray(mask)
    if a.ndim != 2:
        raise ValueError("clean_mask: expected [h, w], got %s" % (a.shape,))
    lab, n = ndimage.label(a != 0, structure=ndimage.generate_binary_structure(2, 1 if connectivity == 4 else 2))
    if n == 0:
        return a.copy(), np.zeros(4, np.int64)
    areas = np.bincount(lab.reshape(-1), minlength=n + 1)[1:]
    order = np.argsort(-areas, kind="stable")
    ok = np.zeros(n + 1, bool)
    ranked = order if keep == 0 else order[:keep]
    ok[1 + ranked[areas[ranked] >= min_area]] = True
    kept = ok[lab]
    return np.where(kept, a, 0).astype(a.dtype), np.array([n, areas.sum(), areas.max(), np.count_nonzero(kept)], np.int64)


class CleanLog:
    """What the segmenters' clean= collects, per sequence (one (video, expression) pair):

        log = CleanLog(); log.add(seq, frame, stats) ...; log.fragmented(); log.dump()

    stats: the four integers of cmpc_mask_components for that frame (CLEAN_STATS)."""

    def __init__(self):
        self.seqs: Dict[object, Dict[int, Tuple[int, int, int, int]]] = {}

    def add(self, seq, frame: int, stats):
        frames = self.seqs.setdefault(seq, {})
        if frame in frames:
            raise ValueError("CleanLog.add: sequence %r already holds frame %r" % (seq, frame))
        s = tuple(int(v) for v in np.asarray(stats).reshape(4))
        if min(s) < 0 or s[2] > s[1] or s[3] > s[1] or (s[0] == 0) != (s[1] == 0):
            raise ValueError("CleanLog.add: impossible statistics %r" % (s,))
        frames[frame] = s

    def __len__(self) -> int:
        return sum(len(f) for f in self.seqs.values())

    def stats(self, seq) -> Tuple[np.ndarray, List[int]]:
        """(int64 [F, 4] in frame order, the frame ids)."""
        if seq not in self.seqs:
            raise KeyError("CleanLog: no sequence %r" % (seq,))
        ids = sorted(self.seqs[seq])
        return np.array([self.seqs[seq][f] for f in ids], dtype=np.int64).reshape(len(ids), 4), ids

    def fragmented(self, min_share: float = 0.9) -> List[Tuple[object, int]]:
        """(seq, frame) of every frame whose largest component holds less than `min_share` of the foreground; never an empty frame."""
        return [(seq, f) for seq, frames in self.seqs.items() for f in sorted(frames)
                if frames[f][1] > 0 and frames[f][2] < min_share * frames[f][1]]

    def dump(self) -> List[Dict[str, object]]:
        """JSON-able: one {"seq", "frame", and the four statistics} per frame, sequences in insertion order, frames in order."""
        return [dict(zip(CLEAN_STATS, frames[f]), seq=list(seq) if isinstance(seq, tuple) else seq, frame=int(f))
                for seq, frames in self.seqs.items() for f in sorted(frames)]
