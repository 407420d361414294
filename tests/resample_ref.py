"""A dense float64 reference of the resampling csrc/ops_eval.hip does, independent of hostutil's restatement on scipy.ndimage: every
axis of a resize is ONE explicit matrix (the mirror-mode Gaussian folded into the pixel-area bilinear zoom), a resize is two matrix
products per channel.  Pure NumPy: no scipy, no separable filtering, no shared helper with the kernels or with hostutil except the
pad / crop geometry functions, which tests/test_hostutil.py pins by hand-worked cases.

    dense_resize(a, oh, ow)      skimage.transform.resize as scikit-image >= 0.19 documents it (float64 [oh, ow(, c)])
    dense_pad / dense_crop       resize_and_pad / resize_and_crop on it
    nearest_pad                  resize_and_pad of a bool image, order 0
    tile_choice                  which LDS tile launch_prep / plan_target pick (a restatement of the host code, for coverage guards only)

The case lists of tests/test_resample_ref_host.py and tests/test_gpu_resample_edges.py live here, so both walk the same cases.
"""
import functools
import importlib
import math

import numpy as np

HU = importlib.import_module("cmpc-refseg_amd.hostutil")

MAXR = 63                                   # eval_resample.h
LDS_CAP = 64 * 1024 - 2 * (MAXR + 1) * 8    # ops_eval.hip: 64 KB less the two Gaussian weight tables
SHAPES = ((8, 32), (4, 32), (2, 32), (1, 32), (1, 16), (1, 8), (1, 4), (1, 1))


# ---- per-axis matrices ---------------------------------------------------------------------------------------------------------------
def mirror(i: int, n: int) -> int:
    """numpy.pad "reflect" / ndimage "mirror": period 2 (n - 1), the edge sample is not repeated."""
    if n == 1:
        return 0
    p = 2 * (n - 1)
    i = abs(i) % p
    return p - i if i >= n else i


def gauss_radius(sigma: float) -> int:
    return int(4.0 * sigma + 0.5)


@functools.lru_cache(maxsize=None)
def gauss_matrix(n: int, sigma: float) -> np.ndarray:
    """[n, n] (cached: treat as read-only): row i holds the normalised Gaussian of radius int(4 sigma + 0.5) centred on i, folded back into 0..n-1 by mirroring."""
    G = np.zeros((n, n), np.float64)
    if sigma <= 1e-15:
        G[np.arange(n), np.arange(n)] = 1.0
        return G
    r = gauss_radius(sigma)
    x = np.arange(-r, r + 1, dtype=np.float64)
    w = np.exp(-(x * x) / (2.0 * sigma * sigma))
    w = w / w.sum()
    for i in range(n):
        for d in range(-r, r + 1):
            G[i, mirror(i + d, n)] += w[d + r]
    return G


@functools.lru_cache(maxsize=None)
def zoom_matrix(n: int, m: int) -> np.ndarray:
    """[m, n] (cached: treat as read-only): output o samples the source at cc = (o + 0.5) (n / m) - 0.5 (pixel-area grid), linearly between floor(cc) and floor(cc) + 1."""
    Z = np.zeros((m, n), np.float64)
    for o in range(m):
        cc = (o + 0.5) * (n / m) - 0.5
        if n == 1:
            cc = 0.0
        elif cc < 0.0:
            cc = -cc
        f = math.floor(cc)
        t = cc - f
        Z[o, mirror(f, n)] += 1.0 - t
        Z[o, mirror(f + 1, n)] += 1.0 - (1.0 - t)
    return Z


def axis_matrices(h: int, w: int, oh: int, ow: int):
    fy, fx = h / oh, w / ow
    My, Mx = zoom_matrix(h, oh), zoom_matrix(w, ow)
    if max(fy, fx) > 1:
        My = My @ gauss_matrix(h, max(0.0, (fy - 1) / 2))
        Mx = Mx @ gauss_matrix(w, max(0.0, (fx - 1) / 2))
    return My, Mx


def dense_resize(a, oh: int, ow: int) -> np.ndarray:
    a = np.asarray(a)
    a = a.astype(np.float64) / 255.0 if a.dtype == np.uint8 else a.astype(np.float64)
    h, w = a.shape[:2]
    if (h, w) == (oh, ow):
        return a
    My, Mx = axis_matrices(h, w, oh, ow)
    if a.ndim == 2:
        return (My @ a) @ Mx.T
    return np.stack([(My @ a[:, :, c]) @ Mx.T for c in range(a.shape[2])], axis=2)


# ---- pad, crop, order 0 --------------------------------------------------------------------------------------------------------------
def dense_pad(im, H: int, W: int) -> np.ndarray:
    im = np.asarray(im)
    rh, rw, top, left = HU.resize_and_pad_geometry(im.shape[0], im.shape[1], H, W)
    r = dense_resize(im, rh, rw)
    out = np.zeros((H, W) + r.shape[2:], np.float64)
    out[top: top + rh, left: left + rw] = r
    return out


def dense_crop(m, h: int, w: int) -> np.ndarray:
    m = np.asarray(m)
    rh, rw, top, left = HU.resize_and_crop_geometry(m.shape[0], m.shape[1], h, w)
    return dense_resize(m, rh, rw)[top: top + h, left: left + w]


def nearest_pad(mask, H: int, W: int) -> np.ndarray:
    """Order 0: the source sample at floor(cc + 0.5), clipped to the image."""
    m = np.asarray(mask) != 0
    h, w = m.shape
    rh, rw, top, left = HU.resize_and_pad_geometry(h, w, H, W)
    ys = [min(max(math.floor(((o + 0.5) * (h / rh) - 0.5) + 0.5), 0), h - 1) for o in range(rh)]
    xs = [min(max(math.floor(((o + 0.5) * (w / rw) - 0.5) + 0.5), 0), w - 1) for o in range(rw)]
    out = np.zeros((H, W), bool)
    out[top: top + rh, left: left + rw] = m[np.ix_(ys, xs)]
    return out


# ---- the kernels' tile selection, restated -------------------------------------------------------------------------------------------
def radii(sh: int, sw: int, dh: int, dw: int):
    """(zy, zx, ry, rx) of a sh x sw -> dh x dw resize: sample_geo of eval_resample.h."""
    zy, zx = sh / dh, sw / dw
    ry = rx = 0
    if max(zy, zx) > 1.0:
        sy, sx = max(0.0, (zy - 1.0) / 2.0), max(0.0, (zx - 1.0) / 2.0)
        ry = gauss_radius(sy) if sy > 1e-15 else 0
        rx = gauss_radius(sx) if sx > 1e-15 else 0
    return zy, zx, ry, rx


def _extent(z, t, r, n):
    span = min(int(math.ceil((t - 1) * z)) + 6, n + 2)
    return span, span + 2 * r


def tile_choice(kernel: str, samples, H: int, W: int, order: int = 1):
    """The output tile (ty, tx) one launch over `samples` ([(h, w, c), ...], padded into H x W) stages its source footprints with, or the
    refusal the host code answers with: "empty" (a resized side of 0), "radius" (Gaussian radius above MAXR) or "lds" (not even the
    1 x 1 tile fits).  kernel "prep": eval_prep_kernel (launch_prep: tile_extent, prep_lds); "target": train_target_kernel (plan_target:
    tile_lds, tile_lds_bytes; order 0 drops the Gaussian).  The maximum over the samples decides, as on the device.

    This RESTATES host code of csrc/ops_eval.hip and must follow it whenever the staging changes.  It exists only so that the tests can
    assert that their case lists reach the tile shapes they claim to cover; no expected value comes from it."""
    geo = []
    for h, w, c in samples:
        rh, rw, _, _ = HU.resize_and_pad_geometry(h, w, H, W)
        if rh <= 0 or rw <= 0:
            return "empty"
        zy, zx, ry, rx = radii(h, w, rh, rw)
        if ry > MAXR or rx > MAXR:
            return "radius"
        if kernel == "target" and order == 0:
            ry = rx = 0
        geo.append((h, w, c, zy, zx, ry, rx))
    for ty, tx in SHAPES:
        need = 0
        for h, w, c, zy, zx, ry, rx in geo:
            nyb, nyr = _extent(zy, ty, ry, h)
            nxb, nxr = _extent(zx, tx, rx, w)
            if kernel == "prep":
                b = ((nyr * nxr * c + 15) & ~15) + nyb * nxr * c * 8
            else:
                wn = (nxb + 3) // 4
                wr = wn + (2 * rx) // 4 + 2
                b = 4 * (nyr * wr + nyr * wn + nyb * wn)
            need = max(need, b)
        if need <= LDS_CAP:
            return ty, tx
    return "lds"


# ---- the cases ------------------------------------------------------------------------------------------------------------------------
OUTS = ((23, 41), (41, 23), (32, 32))
# source sizes at output (23, 41); (41, 23) takes them mirrored (w, h), (32, 32) as they are
SOURCES = ((1, 1), (1, 7), (7, 1), (2, 2), (5, 3), (23, 41), (12, 20), (24, 40), (37, 61), (3, 50), (50, 3), (2, 60), (46, 82), (96, 96),
           (128, 128), (160, 160), (256, 256), (320, 320), (40, 700), (50, 900))
BIG = (720, 1280)                            # grey images and plain masks only: a colour source of this size is refused (LDS)
REFUSALS = (((700, 40, 3), "radius"), ((720, 1280, 3), "lds"), ((1, 100, 3), "empty"))       # at output (23, 41)


TARGET_EXTRA = (10, 739)                     # plain masks only: the source that takes train_target_kernel to its {1, 32} tile


def sources(out):
    """The source sizes of output `out`: (41, 23) takes them mirrored; the large grey-only one comes last, where its radius allows it
    ((32, 32) would need radius 78)."""
    flip = out == (41, 23)
    big = () if out == (32, 32) else (BIG,)
    return [(w, h) if flip else (h, w) for h, w in SOURCES + big]


def prep_cases(out):
    """(h, w, c) of every image of output `out`: each source as colour [h, w, 3] and grey, the grey ones alternating between [h, w]
    (c = 0) and [h, w, 1]; the large source grey only."""
    cases = []
    for i, (h, w) in enumerate(sources(out)):
        if (h, w) not in (BIG, BIG[::-1]):
            cases.append((h, w, 3))
        cases.append((h, w, i % 2))
    return cases


def image(h: int, w: int, c: int, seed: int = 0) -> np.ndarray:
    """A uint8 test image: smooth waves plus noise, full range, the channels different (c = 0: [h, w]; 1: [h, w, 1]; 3: [h, w, 3])."""
    rng = np.random.default_rng(1000003 * h + 1009 * w + 7 * c + seed)
    y, x = np.mgrid[0:h, 0:w]
    base = 127 + 110 * np.sin(x / 5.0 + 0.3)[..., None] * np.cos(y / 7.0)[..., None] * np.array([1.0, 0.7, -0.5])
    im = np.clip(base + rng.normal(0, 30, (h, w, 3)), 0, 255).astype(np.uint8)
    if c == 3:
        return im
    return np.ascontiguousarray(im[..., 1] if c == 0 else im[..., 1:2])


MASK_KINDS = ("c00", "c01", "c10", "c11", "interior", "row", "col", "pair", "empty", "noise")


def mask(h: int, w: int, kind: str, gap=(1, 1)) -> np.ndarray:
    """A bool [h, w] object mask whose misses show: one pixel in a corner (c00 .. c11) or inside, a full border row / column, two pixels
    `gap` = (2 ry + 1, 2 rx + 1) apart (their Gaussian windows just do not meet), nothing, or 2 % noise."""
    m = np.zeros((h, w), bool)
    if kind in ("c00", "c01", "c10", "c11"):
        m[(h - 1) * int(kind[1]), (w - 1) * int(kind[2])] = True
    elif kind == "interior":
        m[h // 3, (2 * w) // 3] = True
    elif kind == "row":
        m[h - 1, :] = True
    elif kind == "col":
        m[:, 0] = True
    elif kind == "pair":
        y, x = h // 4, w // 4
        m[y, x] = True
        m[min(y + gap[0], h - 1), min(x + gap[1], w - 1)] = True
    elif kind == "noise":
        m = np.random.default_rng(31 * h + w).random((h, w)) < 0.02
        m[h // 2, w // 2] = True
    elif kind != "empty":
        raise ValueError(kind)
    return m


@functools.lru_cache(maxsize=None)
def target_cases(out):
    """[(mask, name, dense_pad(mask) > 0)] for prepare_targets at output `out`: every source size (and TARGET_EXTRA) with two kinds
    rotating through MASK_KINDS, every kind on the degenerate and the strongly shrinking sources, noise only where no radius exceeds 1,
    one empty mask.  A kind whose reference target comes out empty or full over the resized rectangle is dropped (a border row under a
    radius as large as the image fills everything): an all-true or all-false kernel must not pass.  The 1 x 1 and 2 x 2 sources stay:
    upscaled, every output pixel mixes all of their samples, so any object fills the rectangle."""
    H, W = out
    cases = []
    kinds = [k for k in MASK_KINDS if k not in ("noise", "empty")]
    extra = TARGET_EXTRA[::-1] if out == (41, 23) else TARGET_EXTRA
    for i, (h, w) in enumerate(sources(out) + ([] if out == (32, 32) else [extra])):         # at (32, 32) its resized height is 0
        rh, rw, _, _ = HU.resize_and_pad_geometry(h, w, H, W)
        _, _, ry, rx = radii(h, w, rh, rw)
        ks = [kinds[i % len(kinds)], kinds[(i + 3) % len(kinds)]]
        if h * w <= 15 or (h, w) in ((50, 900), (900, 50), (160, 160), (37, 61), (61, 37), BIG, BIG[::-1]):
            ks = list(kinds)
        if max(ry, rx) <= 1:
            ks.append("noise")
        if i == 0:
            ks.append("empty")
        for k in dict.fromkeys(ks):
            m = mask(h, w, k, (2 * ry + 1, 2 * rx + 1))
            ref = dense_pad(m, H, W) > 0
            if k == "empty" or h * w <= 4 or 0 < int(ref.sum()) < rh * rw:
                cases.append((m, "%dx%d %s" % (h, w, k), ref))
    return cases


# ---- resize-and-crop: score maps against target sizes -------------------------------------------------------------------------------
MAPS = ((24, 40), (40, 24), (8, 8), (1, 5))
CROP_SIZES = ((1, 1), (1, 9), (9, 1), (2, 2), (5, 7), (7, 5), None, (37, 61), (61, 37), (200, 150), (3, 250), (2, 90))      # None: the map's own size
MAP_KINDS = ("c00", "c11", "interior", "half", "noise", "empty")


def crop_sizes(shape):
    return [shape if s is None else s for s in CROP_SIZES]


def binary_map(h: int, w: int, kind: str) -> np.ndarray:
    """A bool [h, w] binarised score map: mask()'s kinds, or the lower-right part below a diagonal ("half")."""
    if kind == "half":
        y, x = np.mgrid[0:h, 0:w]
        return (y + 1) * w + (x + 1) * h > int(1.2 * h * w)
    return mask(h, w, kind)


@functools.lru_cache(maxsize=None)
def crop_cases(shape):
    """[(kind, (oh, ow), dense_crop(map) > 0)] over MAP_KINDS x crop_sizes(shape) for a map of `shape`, in an order that mixes kinds and
    sizes within a batch."""
    out = []
    for j, size in enumerate(crop_sizes(shape)):
        for kind in MAP_KINDS:
            out.append((kind, size, dense_crop(binary_map(shape[0], shape[1], kind), size[0], size[1]) > 0))
    return out
