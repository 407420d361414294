"""Inputs, float64 references and the shared assertions of the DenseCRF edge tests (tests/test_gpu_crf_lattice_edges.py,
tests/test_gpu_crf_exact_edges.py and their CPU companions in tests/test_crf_refs_host.py).  A case is built once per process and its
reference is computed once; the GPU test and the companion that asserts the case's structural premise read the same objects.

Both sides get the same numbers: every map is rounded to float32 before the reference sees it, and every real-valued parameter is
rounded to float32 (`f32`), which is what the C entry points receive.  Without that, srgb = 0.57 would reach the kernel as
float32(0.57) and the reference as the double 0.57: 1 / srgb then rounds to neighbouring float32 values, and at colour keys near
+-2000 one ulp of a feature moves a barycentric weight by 4e-5 -- a difference of the inputs, not of the kernel."""
import functools
from collections import namedtuple

import numpy as np

from oracle import dense_crf_numpy as OC
from tests import crf_exact_ref as X
from tests import crf_lattice_ref as R
from tests.test_dense_crf_lattice import _case

Q_TOL = 2e-4            # the project's bar on |Q - float64 reference| for both paths
SURE = 1e-3             # a pixel is "sure" when |ref Q1 - ref Q0| exceeds this: only there is the mask compared
SURE_SHARE = 0.95       # every case keeps at least this share of its pixels sure (asserted in the companions)
SUM_TOL = 1e-5
CHUNK = 1024            # entries per block of the lattice's leader scan (kChunk)

Case = namedtuple("Case", "p rgb kw")          # p [H, W] float32, rgb [H, W, 3] uint8, kw: parameters as Python floats of float32 value


def f32(x):
    return float(np.float32(x))


def params(**kw):
    return {k: (v if k == "iters" else f32(v)) for k, v in kw.items()}


def disc(seed, H, W, noise=6):
    """tests/test_dense_crf_lattice.py's noisy disc; noise = 0 replaces the image by its exact two tones."""
    p, rgb = _case(np.random.default_rng(seed), H, W)
    if noise == 0:
        rgb = np.where(p[..., None] > 0.5, 150, 60).astype(np.uint8) * np.ones((1, 1, 3), np.uint8)
    return p.astype(np.float32), rgb


def bits_image(seed, H, W):
    """Every channel 0 or 255; the corners black and white, one pure blue and one pure red pixel."""
    rgb = (np.random.default_rng(1000 + seed).integers(0, 2, (H, W, 3)) * 255).astype(np.uint8)
    rgb[0, 0] = (0, 0, 0)
    rgb[H - 1, W - 1] = (255, 255, 255)
    if H * W > 3:
        rgb.reshape(-1, 3)[1] = (0, 0, 255)
        rgb.reshape(-1, 3)[H * W - 2] = (255, 0, 0)
    return rgb


SATURATED = np.array([0.0, 1.0, 0.5, 1e-8, 1.0 - 1e-8])


def saturated(seed, H, W):
    """A map drawn from {0, 1, 0.5, 1e-8, 1 - 1e-8} (every value at least once) on the {0, 255} image."""
    rng = np.random.default_rng(2000 + seed)
    idx = rng.integers(0, 5, H * W)
    idx[:5] = np.arange(5)
    return SATURATED[rng.permutation(idx)].reshape(H, W).astype(np.float32), bits_image(seed, H, W)


# The noisy disc under the default weights (compat 3 / 10, 5 iterations) ends with Q within 1e-7 of 0 or 1 almost everywhere, and there
# a wrong pairwise term moves Q by far less than the bar.  Every geometric case therefore runs a second time with weak weights and two
# iterations ("name~soft"): Q stays undecided (|Q1 - Q0| < 0.99 on 97 % of the pixels and more) and an error e of a pairwise sum shows
# as about e / 4 in Q.  Measured on the float64 references: a bilateral lattice whose neighbour keys are read with 11 instead of 12 bits
# moves key_bilateral by 1.3e-5 and key_bilateral~soft by 1.2e-2; a window table without its entries beyond 255 moves table_300 by
# 9e-7 and table_300~soft by 1.1e-3.
SOFT = dict(compat_g=1.0, compat_b=1.0, iters=2)


def _soften(make):
    def made(name):
        if not name.endswith("~soft"):
            return make(name)
        c = make(name[:-5])
        return Case(c.p, c.rgb, {**c.kw, **SOFT})
    return made


def with_soft(names, hard_only=()):
    return tuple(names) + tuple(n + "~soft" for n in names if n not in hard_only)


def all_tie(H, W, iters):
    return Case(np.full((H, W), 0.5, np.float32), np.full((H, W, 3), 90, np.uint8), params(iters=iters))


# ---- lattice ---------------------------------------------------------------------------------------------------------------------------

VH, VW = 24, 28                                 # the vertex-count extremes
V_BATCH = ("uniform_rgb@0.9", "const0@0.9", "const255")          # one call, one srgb: the three images at srgb 0.9
SMALL_B = 40


def _uniform_rgb(seed):
    return np.random.default_rng(3000 + seed).integers(0, 256, (VH, VW, 3), dtype=np.uint8)


@_soften
def _lattice_case(name):
    if name == "key_bilateral":
        return Case(disc(0, 12, 13)[0], bits_image(0, 12, 13), params(sxy_b=20.0, srgb=0.57))
    if name == "key_gauss_1e-3":
        return Case(*disc(0, 12, 13), params(sxy_g=1e-3))
    if name == "key_gauss_1e-4":
        return Case(*disc(0, 12, 13), params(sxy_g=1e-4))
    if name in ("uniform_rgb", "uniform_rgb@0.9"):
        return Case(disc(0, VH, VW)[0], _uniform_rgb(0), params(srgb=0.9) if "@" in name else {})
    if name in ("const0", "const0@0.9"):
        return Case(disc(0, VH, VW)[0], np.zeros((VH, VW, 3), np.uint8), params(srgb=0.9) if "@" in name else {})
    if name == "const255":
        return Case(disc(0, VH, VW)[0], np.full((VH, VW, 3), 255, np.uint8), params(srgb=0.9))
    if name == "scan_d5":
        return Case(*disc(0, 210, 209), params(iters=2))
    if name == "scan_d2":
        return Case(*disc(0, 296, 296, noise=0), params(iters=2))
    if name.startswith("shape_"):
        H, W = (int(v) for v in name[6:].split("x"))
        return Case(*disc(0, H, W), {})
    if name.startswith("small_"):
        return Case(*disc(100 + int(name[6:]), 5, 7), {})
    if name == "saturated":
        return Case(*saturated(0, 9, 11), params(sxy_b=20.0, srgb=0.57))
    raise KeyError(name)


SHAPES = ("shape_11x31", "shape_18x19", "shape_10x17", "shape_9x19", "shape_1x1", "shape_1x2", "shape_2x1")
LATTICE_SINGLE = with_soft(("key_bilateral", "key_gauss_1e-3", "key_gauss_1e-4", "uniform_rgb", "const0", "const255", "scan_d5", "scan_d2") + SHAPES +
                           ("saturated",), hard_only=("saturated",))
LATTICE_ALL = LATTICE_SINGLE + V_BATCH[:2] + tuple("small_%d" % b for b in range(SMALL_B))


@functools.lru_cache(maxsize=None)
def lattice_case(name):
    return _lattice_case(name)


@functools.lru_cache(maxsize=None)
def lattice_pair(name):
    """The (Gaussian, bilateral) lattices of the reference for the case (the ~soft variant shares them: same image, same sigmas)."""
    if name.endswith("~soft"):
        return lattice_pair(name[:-5])
    c = lattice_case(name)
    kw = {k: v for k, v in c.kw.items() if k in ("sxy_g", "sxy_b", "srgb")}
    return R.lattices(c.p.shape, c.rgb, fast=c.p.size > 5000, **kw)      # the two scan cases: without the Python loops


@functools.lru_cache(maxsize=None)
def lattice_ref(name):
    c = lattice_case(name)
    q = R.dense_crf(c.p.astype(np.float64), c.rgb, lats=lattice_pair(name), **c.kw)
    q.setflags(write=False)
    return q


# ---- the host bound on the lattice keys, restated ------------------------------------------------------------------------------------

def key_bound(fmax, d):
    """key_bound<D> of ops_crf_lattice.hip: double arithmetic on the float32 feature maxima and scale factors."""
    cf = [float(fmax[i]) * float(s) for i, s in enumerate(R.scale_factors(d))]
    worst = 0.0
    for j in range(d + 1):
        worst = max(worst, sum(cf[j:]), j * cf[j - 1] if j > 0 else 0.0)
    return worst * (1.0 + 1e-5) + 1.5 * (d + 1) + d + 1


def gaussian_bound(H, W, sxy_g):
    inv = np.float32(1.0 / f32(sxy_g))
    return key_bound([np.float32(W - 1) * inv, np.float32(H - 1) * inv], 2)


def bilateral_bound(H, W, sxy_b, srgb):
    inv, ic = np.float32(1.0 / f32(sxy_b)), np.float32(1.0 / f32(srgb))
    return key_bound([np.float32(W - 1) * inv, np.float32(H - 1) * inv] + [np.float32(255) * ic] * 3, 5)


KEY_MAX = {2: 2 ** 30 - 1, 5: 2047}


def smallest_accepted_srgb(H=12, W=13, sxy_b=20.0):
    """Bisection on the restated bound: the smallest float32 srgb (to 1e-6 relative) the entry point accepts at this size."""
    lo, hi = 0.1, 3.0
    assert bilateral_bound(H, W, sxy_b, lo) > KEY_MAX[5] >= bilateral_bound(H, W, sxy_b, hi)
    while hi - lo > 1e-6 * hi:
        mid = 0.5 * (lo + hi)
        if bilateral_bound(H, W, sxy_b, mid) <= KEY_MAX[5]:
            hi = mid
        else:
            lo = mid
    return hi


# ---- exact window ----------------------------------------------------------------------------------------------------------------------

@_soften
def _exact_case(name):
    if name == "table_300":
        return Case(*disc(0, 3, 300), params(sxy_b=120.0))
    if name == "table_512":
        return Case(*disc(0, 2, 512), params(sxy_b=127.75))
    if name == "window_12x100":
        return Case(*disc(0, 12, 100), {})
    if name == "window_40x45":
        return Case(*disc(0, 40, 45), params(sxy_g=1.0, sxy_b=4.0))
    if name == "shape_9x9_iters0":
        return Case(*disc(0, 9, 9), params(iters=0))
    if name.startswith("shape_"):
        H, W = (int(v) for v in name[6:].split("x"))
        return Case(*disc(0, H, W), {})
    if name == "bits":
        return Case(disc(0, 12, 13)[0], bits_image(0, 12, 13), params(srgb=0.57))
    if name == "saturated":
        return Case(*saturated(0, 9, 11), params(srgb=0.57))
    raise KeyError(name)


EXACT_ALL = with_soft(("table_300", "table_512", "window_12x100", "window_40x45", "shape_1x1", "shape_1x29", "shape_31x1", "shape_33x65",
                       "shape_9x9_iters0", "bits", "saturated"), hard_only=("shape_9x9_iters0", "saturated"))


@functools.lru_cache(maxsize=None)
def exact_case(name):
    return _exact_case(name)


def radii(name):
    c = exact_case(name)
    H, W = c.p.shape
    return X.window_radius(H, W, c.kw.get("sxy_g", 3.0)), X.window_radius(H, W, c.kw.get("sxy_b", 20.0))


def truncated(name):
    H, W = exact_case(name).p.shape
    return min(radii(name)) < max(H, W) - 1


@functools.lru_cache(maxsize=None)
def exact_ref(name):
    c = exact_case(name)
    q = X.dense_crf(c.p.astype(np.float64), c.rgb, **c.kw)
    q.setflags(write=False)
    return q


def exact_oracle(name):
    c = exact_case(name)
    return OC.dense_crf(c.p.astype(np.float64), c.rgb, **c.kw)


# ---- the assertions every comparison makes ---------------------------------------------------------------------------------------------

def sure_share(ref):
    return float((np.abs(ref[1] - ref[0]) > SURE).mean())


def check(tag, q, mask, ref):
    """q [2, H, W] and mask [H, W] from the device against ref [2, H, W] float64; prints the measured error before asserting."""
    q, mask = np.asarray(q, np.float64), np.asarray(mask)
    err = float(np.abs(q - ref).max()) if np.isfinite(q).all() else float("inf")
    print("crf-edge %-28s %4d x %-4d max|Q - ref| = %.3e" % (tag, ref.shape[1], ref.shape[2], err))
    assert np.isfinite(q).all(), tag
    assert err < Q_TOL, (tag, err)
    sure = np.abs(ref[1] - ref[0]) > SURE
    assert np.array_equal(mask[sure], ref.argmax(0)[sure].astype(np.uint8)), tag
    assert np.abs(q.sum(0) - 1).max() < SUM_TOL, tag
    return err
