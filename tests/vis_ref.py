"""NumPy restatement of the pictures cmpc_vis_overlay / cmpc_vis_heat / cmpc_vis_words render (csrc/ops_vis.hip), the oracle of
tests/test_vis_host.py and tests/test_gpu_vis.py.

  overlay_pred / overlay_gt   written as the reference writes them (trainval_model.py:306-330): float `/ 2`, `+=`, `.astype('uint8')`.
                              The mask is a 0/1 mask (`mask != 0`): the package's "resampled value > 0" decision.
  heat_value                  hostutil.resize_and_crop of the float32 map (or of its float32 sigmoid, 1 / (1 + exp(-x)) evaluated in
                              float32 in that order: test_visualize_fusion.py:150-151 on a float32 fetch), in float64.
  index_of                    idx = clip(floor((v - lo) / (hi - lo) * 256), 0, 255) in float64; hi == lo gives 0.
  heat                        (idx, (lo, hi)): fixed range, or with vrange None the min and max of v over the output (imshow's autoscale).
  word_sheet                  panel t = gw[:, t] as (gh, gw), indexed with its own min and max (float32 widened to float64), every pixel
                              repeated zoom x zoom; rows = ceil(max_words / cols) rows of cols panels, `gap` pixels between panels;
                              gaps and panels t >= n_words are (255, 255, 255).
"""
import importlib

import numpy as np

HU = importlib.import_module("cmpc-refseg_amd.hostutil")


def _rgb(im):
    im = np.asarray(im)
    if im.ndim == 2 or im.shape[2] == 1:
        im = np.repeat(im.reshape(im.shape[0], im.shape[1], 1), 3, 2)          # build_batches.py:67-68
    return im


def overlay_pred(im, mask):
    predicts = (np.asarray(mask) != 0)
    out = _rgb(im) / 2                                                          # float64
    out[:, :, 0] += predicts.astype('uint8') * 100
    return out.astype('uint8')


def overlay_gt(mask):
    m = (np.asarray(mask) != 0)
    out = np.zeros(m.shape + (3,))
    out[:, :, 0] = 170 * m
    out[:, :, 2] = 170 * (1 - m)
    return out.astype('uint8')


def sigmoid32(x):
    x = np.asarray(x, dtype=np.float32)
    one = np.float32(1.0)
    s = one / (one + np.exp(-x))
    assert s.dtype == np.float32
    return s


def heat_value(m, h, w, sigmoid=False):
    s = np.asarray(m, dtype=np.float32)
    if sigmoid:
        s = sigmoid32(s)
    v = HU.resize_and_crop(s, h, w)
    assert v.dtype == np.float64 and v.shape == (h, w)
    return v


def index_of(v, lo, hi):
    v = np.asarray(v, dtype=np.float64)
    lo, hi = np.float64(lo), np.float64(hi)
    if hi == lo:
        return np.zeros(v.shape, np.uint8)
    return np.clip(np.floor((v - lo) / (hi - lo) * 256), 0, 255).astype(np.uint8)


def heat(m, h, w, sigmoid=False, vrange=(0.0, 1.0)):
    v = heat_value(m, h, w, sigmoid)
    lo, hi = (v.min(), v.max()) if vrange is None else vrange
    return index_of(v, lo, hi), (float(lo), float(hi))


def sheet_size(gh, gw, max_words, zoom, cols, gap):
    rows = -(-max_words // cols)
    return rows * gh * zoom + (rows - 1) * gap, cols * gw * zoom + (cols - 1) * gap


def word_sheet(gw_v, n_words, grid, max_words, zoom, cols, gap, lut):
    """gw_v: float32 [N, ld] of one sample."""
    gh, gw = grid
    g = np.asarray(gw_v, dtype=np.float32)
    sh, sw = sheet_size(gh, gw, max_words, zoom, cols, gap)
    out = np.full((sh, sw, 3), 255, np.uint8)
    for t in range(n_words):
        panel = g[:, t].reshape(gh, gw).astype(np.float64)
        idx = index_of(panel, panel.min(), panel.max())
        pic = np.repeat(np.repeat(np.asarray(lut)[idx], zoom, 0), zoom, 1)
        r, c = divmod(t, cols)
        y0, x0 = r * (gh * zoom + gap), c * (gw * zoom + gap)
        out[y0: y0 + gh * zoom, x0: x0 + gw * zoom] = pic
    return out
