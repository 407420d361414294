"""Float64 restatement of cmpc_label_propagate and cmpc_prop_fuse (csrc/ops_propagate.hip), and the bounds the tests hold them to.

propagate() materialises every candidate of every target and takes a plain softmax; nothing of the kernel's tiling, masking or online
rescaling is repeated here.

bound(C, n_candidates, temperature, max_label).  The kernel's vectors are unit vectors up to rounding, so sum |a b| <= 1 and any
summation order of the C products gives |c - exact| <= delta = (C + 8) 2^-24; the 8 covers the two inverse norms (a tree sum of
squares, a correctly rounded square root and division each), the two scalings and the division by the temperature.  The logits are
therefore off by at most Delta = delta / temperature, every weight exp(logit - max) by a factor within e^{+-Delta}, and a ratio of two
sums of such weights by a factor within e^{+-2 Delta}.  The sums themselves: a target's candidates are spread over 16 partial states
(4 waves x 4 lane groups), each a chain of at most n_candidates / 16 + 1 additions, merged by 15 more, and every weight passes at
most n_candidates / 64 + 2 rescalings -- together fewer than (n_candidates + 8) roundings of 2^-24.  eps_exp = 2^-22: expf is
documented at 1 ulp (HIP math API), 2^-23 relative, once in the numerator and once in the denominator.  Hence

    |out - ref| <= (e^{2 Delta} - 1 + (n_candidates + 8) 2^-24 + eps_exp) max |label|          |peak - ref| <= delta

fuse_bound.  The interpolation coefficients are float32 in the kernel and here (the same three operations: product, floor, difference),
so they are equal; what differs is the arithmetic on the values.  With M = the largest |prop| among the four taps: top and bot are a
difference (2 M), a product (2 M) and a sum (M), 5 M 2^-24 each; u = top + (bot - top) fy inherits 10 M and adds a difference (2 M), a
product (2 M) and a sum (M): 20 M 2^-24 (M bounds every intermediate: each is a convex combination).  The blend rounds 1 - alpha, two
products and a sum: |fused - ref| <= (3 (1 - alpha) |own| + alpha 22 M + |own| + M) 2^-24."""
import numpy as np

U = 2.0 ** -24
EPS_EXP = 2.0 ** -22


def l2_normalize(f):
    """f * rsqrt(max(sum f^2, 1e-12)) over the last axis: a zero vector stays zero."""
    f = np.asarray(f, dtype=np.float64)
    return f / np.sqrt(np.maximum((f * f).sum(-1, keepdims=True), 1e-12))


def window(h, w, radius):
    """bool [h w, h w]: candidate p (column) lies within `radius` of target q (row) in both directions; radius < 0: everywhere."""
    ys, xs = np.divmod(np.arange(h * w), w)
    if radius < 0:
        return np.ones((h * w, h * w), bool)
    return (np.abs(ys[:, None] - ys[None]) <= radius) & (np.abs(xs[:, None] - xs[None]) <= radius)


def propagate(feat, labels, items, radius, temperature):
    """feat: the STORED tap values [frames, h, w, C]; labels [L, h, w]; items [(tgt, [(src, label), ...])].
    Returns float64 (out [n, h, w], peak [n, h, w]) and the candidate counts int [n, h, w]."""
    feat = np.asarray(feat, dtype=np.float64)
    labels = np.asarray(labels, dtype=np.float64)
    frames, h, w, C = feat.shape
    N = h * w
    a = l2_normalize(feat).reshape(frames, N, C)
    win = window(h, w, radius)
    out, peak, cnt = [], [], []
    for tgt, srcs in items:
        c = np.concatenate([a[tgt] @ a[sf].T for sf, _ in srcs], axis=1)              # [N targets, nsrc * N candidates]
        lab = np.concatenate([labels[l].reshape(N) for _, l in srcs])
        mask = np.tile(win, (1, len(srcs)))
        logit = np.where(mask, c / float(temperature), -np.inf)
        e = np.exp(logit - logit.max(1, keepdims=True))
        wgt = e / e.sum(1, keepdims=True)
        out.append((wgt @ lab).reshape(h, w))
        peak.append(np.where(mask, c, -np.inf).max(1).reshape(h, w))
        cnt.append(mask.sum(1).reshape(h, w))
    return np.stack(out), np.stack(peak), np.stack(cnt)


def delta(C):
    return (C + 8) * U


def bound(C, n_candidates, temperature, max_label):
    D = delta(C) / float(temperature)
    return (np.expm1(2.0 * D) + (np.asarray(n_candidates, dtype=np.float64) + 8) * U + EPS_EXP) * float(max_label)


def _coef(n_out, n_in):
    """The legacy bilinear rule in float32: src = dst * (n_in / n_out), lo = floor(src), hi = min(lo + 1, n_in - 1), lerp = src - lo."""
    scale = np.float32(n_in) / np.float32(n_out)
    src = np.arange(n_out, dtype=np.float32) * scale
    lo = np.floor(src)
    lerp = (src - lo).astype(np.float64)
    lo = lo.astype(np.int64)
    return lo, np.minimum(lo + 1, n_in - 1), lerp


def upsample(prop, H, W):
    """U(prop) [n, H, W] in float64 on float32 coefficients, and M [n, H, W]: the largest |tap| each output reads."""
    prop = np.asarray(prop, dtype=np.float64)
    n, h, w = prop.shape
    y0, y1, fy = _coef(H, h)
    x0, x1, fx = _coef(W, w)
    tl, tr = prop[:, y0][:, :, x0], prop[:, y0][:, :, x1]
    bl, br = prop[:, y1][:, :, x0], prop[:, y1][:, :, x1]
    top = tl + (tr - tl) * fx[None, None]
    bot = bl + (br - bl) * fx[None, None]
    u = top + (bot - top) * fy[None, :, None]
    M = np.maximum(np.maximum(np.abs(tl), np.abs(tr)), np.maximum(np.abs(bl), np.abs(br)))
    return u, M


def fuse(own, prop, alpha):
    """(1 - alpha) own + alpha U(prop) in float64 with alpha the float32 the kernel receives, and its bound [n, H, W]."""
    own = np.asarray(own, dtype=np.float64)
    al = float(np.float32(alpha))
    u, M = upsample(prop, own.shape[1], own.shape[2])
    ref = (1.0 - al) * own + al * u
    if al == 0.0:
        return ref, np.zeros_like(ref)
    return ref, (3.0 * (1.0 - al) * np.abs(own) + al * 22.0 * M + np.abs(own) + M) * U


def fuse_prop_bound(own, prop_bound, alpha):
    """What an error of at most prop_bound [n, h, w] in prop adds to the fused map: alpha * U(prop_bound) (U is a convex combination)."""
    u, _ = upsample(prop_bound, own.shape[1], own.shape[2])
    return float(np.float32(alpha)) * u


# ---- seeded inputs shared by the host and the GPU tests ---------------------------------------------------------------------------------
DTYPES = ("f32", "f16", "bf16")


def stored(x, dtype):
    """float32 values as the storage type keeps them (round to nearest even), as float32."""
    x = np.asarray(x, dtype=np.float32)
    if dtype == "f32":
        return x
    if dtype == "f16":
        return x.astype(np.float16).astype(np.float32)
    b = x.view(np.uint32).astype(np.uint64)
    b = ((b + 0x7FFF + ((b >> 16) & 1)) >> 16) << 16
    return b.astype(np.uint32).view(np.float32).reshape(x.shape)


def make_items(n, frames, n_labels, nsrc, rng):
    """n items over a bank of `frames`: sources repeat between items, and item 0 uses its own target as its first source."""
    items = []
    for i in range(n):
        tgt = i % frames
        srcs = [((i + 1 + k) % frames, (i + k) % n_labels) for k in range(nsrc)]
        if i == 0:
            srcs[0] = (tgt, 0)
        items.append((tgt, srcs))
    return items


def case(shape, dtype):
    """(feat float32 as stored [frames, h, w, C], labels float32 [L, h, w] of exact 0 and 1, items) of one (n, h, w, C, radius, nsrc):
    a tenth of the vectors all zero, the first half of the channels post-ReLU; frames = min(n, 3) + 1, L = 3."""
    n, h, w, C, radius, nsrc = shape
    rng = np.random.default_rng([n, h, w, C, radius + 1, nsrc, DTYPES.index(dtype)])
    frames, L = min(n, 3) + 1, 3
    x = rng.normal(0, 1, (frames, h, w, C)).astype(np.float32)
    x[..., : C // 2] = np.maximum(x[..., : C // 2], 0)
    x[rng.uniform(0, 1, (frames, h, w)) < 0.1] = 0.0
    labels = (rng.uniform(0, 1, (L, h, w)) < 0.5).astype(np.float32)
    return stored(x, dtype), labels, make_items(n, frames, L, nsrc, rng)


# The mask test: a small video of smooth taps (so that the correspondences mean something), per-frame sigm maps, one expression.
MASK_SEEDS = (11, 12)
MASK_SHAPE = dict(frames=5, h=8, w=10, C=32, H=64, W=80, radius=3, temperature=0.07, alpha=0.5, threshold=0.5)


def mask_case(seed):
    """Seeded inputs of the mask test: f16-stored taps [frames, h, w, C], sigm float32 [frames, H, W] (a smooth blob that moves with the
    taps' content), pivots (0, 4) and the plan's items: frames 1, 2, 3 receive from their pivots within two frames."""
    s = MASK_SHAPE
    rng = np.random.default_rng(seed)
    F, h, w, C, H, W = s["frames"], s["h"], s["w"], s["C"], s["H"], s["W"]
    base = rng.normal(0, 1, (h + F, w + F, C)).astype(np.float32)
    feat = np.stack([base[f: f + h, f // 2: f // 2 + w] for f in range(F)]) + 0.1 * rng.normal(0, 1, (F, h, w, C)).astype(np.float32)
    feat = stored(np.maximum(feat, 0), "f16")
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    sig = []
    for f in range(F):
        cy, cx = 0.6 * H - (H // h) * f, 0.55 * W - (W // w) * (f // 2)          # the blob moves with the taps' content
        d2 = ((yy - cy) / (0.3 * H)) ** 2 + ((xx - cx) / (0.35 * W)) ** 2
        sig.append(1.0 / (1.0 + np.exp(4.0 * (d2 - 1.0))) + 0.02 * rng.normal(0, 1, (H, W)))
    sigm = np.clip(np.stack(sig), 0, 1).astype(np.float32)
    return feat, sigm


def mask_reference(feat, sigm, plan, radius, temperature, alpha, threshold):
    """The float64 chain on one expression's banks: labels = the point samples of sigm, propagate, fuse.  plan: {frame: [pivot, ...]}
    (frame == index into the banks).  Returns {frame: (fused float64 [H, W], bound [H, W], mask bool, unsure bool)}: `unsure` marks the
    pixels whose fused value lies within the bound of the threshold."""
    F, h, w, C = feat.shape
    H, W = sigm.shape[1:]
    labels = sigm[:, :: H // h, :: W // w][:, :h, :w]
    frames = sorted(plan)
    items = [(f, [(p, p) for p in plan[f]]) for f in frames]
    out, _, cnt = propagate(feat, labels, items, radius, temperature)
    pb = bound(C, cnt, temperature, float(np.abs(labels).max()))
    res = {}
    for k, f in enumerate(frames):
        ref, fb = fuse(sigm[f: f + 1], out[k: k + 1], alpha)
        lim = fb + fuse_prop_bound(sigm[f: f + 1], pb[k: k + 1], alpha)
        res[f] = (ref[0], lim[0], ref[0] >= threshold, np.abs(ref[0] - threshold) <= lim[0])
    return res
