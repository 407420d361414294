"""Op-level tests of csrc/ops_decoder.hip against float64 references: slim batch_norm (bn_stats, bn_from_moving, bn_update_moving,
bn_apply_fwd, bn_bwd), legacy-bilinear resize_bilinear_fwd / bwd, hsv_map / hsv_grid, reverse_sequence / reverse_words_tb, rows_nonzero2
and conv_to1_fwd / bwd, in every storage type the entry point takes."""
import pytest
import torch

from tests import opref as R

pytestmark = pytest.mark.gpu

BN_EPS = 1e-5
MEAN_BGR = (104.00698793, 116.66876762, 122.67891434)      # the kernels' mean, BGR (hsv:120-126)
# (C, Cpad, ld): tiny; one column group; the product shape; two column blocks with a pad tail; Cpad at its 2048 limit (128 KiB of LDS)
BN_SHAPES = [(3, 8, 8), (48, 64, 64), (256, 256, 256), (1000, 1024, 1032), (2047, 2048, 2048)]


def _bn_x(Rr, C, ld, dt, g, scale=1.0, offset=0.0):
    x = torch.zeros(Rr, ld, dtype=torch.float64)
    x[:, :C] = torch.randn(Rr, C, generator=g, dtype=torch.float64) * scale + offset + torch.randn(C, generator=g, dtype=torch.float64) * 0.5
    return x.to(R.TDT[dt])


def _stats_ref(x, C):
    x = x.double()[:, :C]
    Rr = x.shape[0]
    m = x.mean(0)
    var = ((x - m) ** 2).mean(0)
    return x.sum(0), (x * x).sum(0), m, 1.0 / torch.sqrt(var + BN_EPS), var, Rr


def _run_stats(x, dt, Rr, C, Cpad, ld):
    sums = R.guarded(2, Cpad, torch.float64)
    mr = R.guarded(2, Cpad, torch.float32)
    R.call("cmpc_bn_stats", dt, x, ld, Rr, C, Cpad, BN_EPS, sums, mr)
    return {"sums": sums, "mr": mr}


def _check_stats(o, x, Rr, C, Cpad, what, dt):
    s1, s2, m, rstd, var, _ = _stats_ref(x, C)
    xc = x.double()[:, :C]
    R.assert_guard(o["sums"], 2, what + " sums")
    R.assert_guard(o["mr"], 2, what + " mean_rstd")
    sums, mr = o["sums"][:2].cpu(), o["mr"][:2].cpu()
    # float32 partial sums over <= 32 rows per lane of the shifted values (x - x[0]), then float64: 32 roundings of 6e-8 of the
    # shifted magnitudes, carried into sum x / sum x^2 exactly (float64)
    d = (xc - xc[0]).abs()
    R.assert_close(sums[0, :C], s1, K=Rr, what=what + " sum x", atol=2e-6 * d.sum(0))
    R.assert_close(sums[1, :C], s2, K=Rr, what=what + " sum x^2", atol=2e-6 * (d * d + 2 * d * xc[0].abs()).sum(0))
    R.assert_zero(sums[:, C:], what + " sums pad channels")
    # mean and rstd are derived from those sums (K = 1: their rounding is the atol).  A stable variance is correct to the float32 rounding
    # of the shifted second moment, times d rstd / d var; E[x^2] - E[x]^2 on unshifted sums is not once |mean| >> std, nor at R = 1
    R.assert_close(mr[0, :C], m, what=what + " mean", atol=2e-6 * d.mean(0))
    dvar = 2e-6 * (d * d).mean(0)
    R.assert_close(mr[1, :C], rstd, what=what + " rstd", atol=0.5 * rstd ** 3 * dvar)
    R.assert_zero(mr[:, C:], what + " mean_rstd pad channels")


@pytest.mark.parametrize("dt", R.DTS, ids=R.DT_IDS)
@pytest.mark.parametrize("shape", BN_SHAPES, ids=lambda s: "C%d-Cpad%d-ld%d" % s)
def test_bn_stats(dt, shape):
    """sums = {sum x, sum x^2} (float64), mean_rstd = {mean, 1/sqrt(biased var + eps)}; R = 1 (variance 0), 127 / 128 / 129 (the 128-row
    partials); pad channels C..Cpad are 0"""
    C, Cpad, ld = shape
    g = R.gen(31)
    for Rr in (1, 127, 128, 129):
        x = _bn_x(Rr, C, ld, dt, g)
        xd = x.to(R.DEV)
        o = R.run_twice(lambda: _run_stats(xd, dt, Rr, C, Cpad, ld))
        _check_stats(o, x, Rr, C, Cpad, f"bn_stats R={Rr}", dt)
    if C <= 48:
        # more than 1000 partial rows, and a mean far from 0 (|mean| >= 30 std): the one-pass E[x^2] - E[x]^2 in float32 cancels there
        for Rr, off in ((130001, 0.0), (20000, 40.0)):
            x = _bn_x(Rr, C, ld, dt, g, scale=1.0, offset=off)
            o = _run_stats(x.to(R.DEV), dt, Rr, C, Cpad, ld)
            torch.cuda.synchronize()
            _check_stats(o, x, Rr, C, Cpad, f"bn_stats R={Rr} offset={off}", dt)


def test_bn_moving():
    """bn_from_moving: mean_rstd = {moving_mean, 1/sqrt(moving_var + eps)}; bn_update_moving: moving = d moving + (1 - d) batch with the
    batch variance Bessel-corrected (R / (R - 1); R = 1 keeps the biased 0); decay 0.9997"""
    g = R.gen(32)
    for C, Cpad in ((3, 8), (1000, 1024), (2047, 2048)):
        mm = torch.randn(C, generator=g).float()
        mv = (torch.rand(C, generator=g) * 2).float()
        mr = R.guarded(2, Cpad, torch.float32)
        R.call("cmpc_bn_from_moving", mm.to(R.DEV), mv.to(R.DEV), C, Cpad, BN_EPS, mr)
        R.assert_guard(mr, 2, "bn_from_moving")
        assert torch.equal(mr[0, :C].cpu(), mm), "bn_from_moving mean"
        R.assert_close(mr[1, :C], 1.0 / torch.sqrt(mv.double() + BN_EPS), what="bn_from_moving rstd")
        R.assert_zero(mr[:2, C:], "bn_from_moving pad")
        for Rr in (1, 129):
            x = torch.randn(Rr, C, generator=g, dtype=torch.float64) + 3.0
            sums = torch.zeros(2, Cpad, dtype=torch.float64)
            sums[0, :C], sums[1, :C] = x.sum(0), (x * x).sum(0)
            m = x.mean(0)
            var = ((x - m) ** 2).mean(0) * (Rr / (Rr - 1) if Rr > 1 else 1.0)
            dec = 0.9997
            mmd, mvd = R.guarded(1, C, torch.float32, mm), R.guarded(1, C, torch.float32, mv)
            R.call("cmpc_bn_update_moving", sums.to(R.DEV), Rr, dec, mmd, mvd, C, Cpad)
            R.assert_guard(mmd, 1, "bn_update_moving mean")
            R.assert_guard(mvd, 1, "bn_update_moving var")
            d = float(torch.tensor(dec, dtype=torch.float32))
            R.assert_close(mmd[0], mm.double() * d + m * (1 - d), what=f"bn_update_moving mean R={Rr}")
            # E[x^2] - m^2 in float64 on sums of x ~ 3 +- 1: 1e-15 relative of E[x^2], far below float32
            R.assert_close(mvd[0], mv.double() * d + var * (1 - d), what=f"bn_update_moving var R={Rr}")


def _affine(C, g):
    return (1 + 0.3 * torch.randn(C, generator=g)).float(), (0.3 * torch.randn(C, generator=g)).float()


@pytest.mark.parametrize("dt", R.DTS, ids=R.DT_IDS)
@pytest.mark.parametrize("shape", BN_SHAPES, ids=lambda s: "C%d-Cpad%d-ld%d" % s)
def test_bn_apply_fwd(dt, shape):
    """y = relu?(gamma (x - mean) rstd + beta) for c < C, 0 for C <= c < Cy; y a column block of a wider map (ldy > Cy): the columns past
    Cy stay untouched"""
    C, Cpad, ld = shape
    g = R.gen(33)
    Rr = 300
    x = _bn_x(Rr, C, ld, dt, g)
    _, _, m, rstd, _, _ = _stats_ref(x, C)
    mr = torch.zeros(2, Cpad)
    mr[0, :C], mr[1, :C] = m.float(), rstd.float()
    gam, bet = _affine(C, g)
    Cy = (C + 7) // 8 * 8 + 8 if C + 8 <= 2048 else Cpad
    ldy = Cy + 16
    xd, mrd, gd, bd = x.to(R.DEV), mr.to(R.DEV), gam.to(R.DEV), bet.to(R.DEV)
    mf = mr.double()
    xh = (x.double()[:, :C] - mf[0, :C]) * mf[1, :C]
    for relu in (0, 1):
        def run():
            y = R.guarded(Rr, ldy, dt)
            R.call("cmpc_bn_apply_fwd", dt, xd, ld, mrd, Cpad, gd, bd, y, ldy, Cy, Rr, C, relu)
            return {"y": y}
        y = R.run_twice(run)["y"]
        what = f"bn_apply_fwd relu={relu}"
        R.assert_guard(y, Rr, what)
        ref = xh * gam.double() + bet.double()
        if relu:
            ref = ref.clamp_min(0)
        # (x - mean) * rstd * gamma + beta in float32: the subtraction cancels, so its rounding scales with |x| + |mean|
        mag = (x.double()[:, :C].abs() + mf[0, :C].abs()) * mf[1, :C] * gam.double().abs() + bet.double().abs()
        R.assert_close(y[:Rr, :C], ref, dt, what=what, atol=3e-7 * mag)
        R.assert_zero(y[:Rr, C:Cy], what + " pad channels C..Cy")
        R.assert_sentinel(y[:Rr, Cy:], what + " columns past Cy")


@pytest.mark.parametrize("dt", R.DTS, ids=R.DT_IDS)
@pytest.mark.parametrize("shape", BN_SHAPES, ids=lambda s: "C%d-Cpad%d-ld%d" % s)
def test_bn_bwd(dt, shape):
    """g = dy [y > 0] (relu) or dy (y NULL); dbeta += sum g, dgamma += sum g xhat; dx = gamma rstd (g - mean g - xhat mean(g xhat)), pad
    channels C..roundup(C, 8) of dx are 0"""
    C, Cpad, ld = shape
    g = R.gen(34)
    Rr = 300
    x = _bn_x(Rr, C, ld, dt, g)
    _, _, m, rstd, _, _ = _stats_ref(x, C)
    mr = torch.zeros(2, Cpad)
    mr[0, :C], mr[1, :C] = m.float(), rstd.float()
    gam, bet = _affine(C, g)
    mf = mr.double()
    xh = (x.double()[:, :C] - mf[0, :C]) * mf[1, :C]
    y = torch.zeros(Rr, ld, dtype=torch.float64)
    y[:, :C] = (xh * gam.double() + bet.double()).clamp_min(0)
    y = y.to(R.TDT[dt])
    dy = R.map_input(1, Rr, C, ld, dt, g)
    dg0, db0 = torch.randn(C, generator=g).float(), torch.randn(C, generator=g).float()
    xd, yd, dyd, mrd, gd = x.to(R.DEV), y.to(R.DEV), dy.to(R.DEV), mr.to(R.DEV), gam.to(R.DEV)
    cin = (C + 7) // 8 * 8
    for relu in (0, 1):
        def run():
            dx = R.guarded(Rr, ld, dt)
            dgm, dbt = R.guarded(1, C, torch.float32, dg0), R.guarded(1, C, torch.float32, db0)
            R.call("cmpc_bn_bwd", dt, dyd, ld, yd if relu else None, ld, xd, ld, mrd, Cpad, gd, dx, ld, dgm, dbt,
                   torch.empty(2, Cpad, device=R.DEV), Rr, C, relu)
            return {"dx": dx, "dg": dgm, "db": dbt}
        o = R.run_twice(run)
        what = f"bn_bwd relu={relu}"
        for k, n in (("dx", Rr), ("dg", 1), ("db", 1)):
            R.assert_guard(o[k], n, what + " " + k)
        gg = dy.double()[:, :C] * ((y.double()[:, :C] > 0).double() if relu else 1.0)
        m0, m1 = gg.mean(0), (gg * xh).mean(0)
        dx = gam.double() * mf[1, :C] * (gg - m0 - xh * m1)
        # column sums over R rows: rounding bounded by the sum of |terms|
        R.assert_close(o["db"][0], db0.double() + gg.sum(0), K=Rr, what=what + " dbeta", atol=R.sum_atol(gg, 0) + 1e-7 * db0.double().abs())
        # ... and each term's xhat = (x - mean) rstd in float32 carries a rounding of (|x| + |mean|) rstd
        xmag = (x.double()[:, :C].abs() + mf[0, :C].abs()) * mf[1, :C]
        R.assert_close(o["dg"][0], dg0.double() + (gg * xh).sum(0), K=Rr, what=what + " dgamma",
                       atol=R.sum_atol(gg * xh, 0) + 3e-7 * (gg.abs() * xmag).sum(0) + 1e-7 * dg0.double().abs())
        # g - mean(g) - xhat mean(g xhat) cancels: rounding of |g| + |mean g| + |xhat mean(g xhat)| (and of xhat's own (x - mean))
        mag = gam.double().abs() * mf[1, :C] * (gg.abs() + m0.abs() + (xh.abs() + (x.double()[:, :C].abs() + mf[0, :C].abs()) * mf[1, :C]) * m1.abs()
                                                 + gg.abs().mean(0) + (gg * xh).abs().mean(0))
        R.assert_close(o["dx"][:Rr, :C], dx, dt, what=what + " dx", atol=4e-7 * mag)
        R.assert_zero(o["dx"][:Rr, C:cin], what + " dx pad channels")


# ----------------------------------------------------------------------------------------------------------------------------
# resize
# ----------------------------------------------------------------------------------------------------------------------------
# (B, h, w, H, W): integer 20 -> 80; non-integer 7 -> 50 and 10x30 -> 57x211; down 50 -> 7; non-square; 1x1 -> up and up -> 1x1;
# the shipped 64 -> 128 and 512 -> 64 ratios
RESIZE_SHAPES = [(2, 20, 20, 80, 80), (1, 7, 7, 50, 50), (2, 10, 30, 57, 211), (2, 50, 50, 7, 7), (1, 13, 6, 40, 9), (2, 1, 1, 5, 3),
                 (1, 6, 4, 1, 1), (1, 8, 8, 16, 16)]


def _resize_ref(x, H, W):
    """[B, h, w, C] float64 -> [B, H, W, C]: TF's float32 coefficients (opref.bilinear_axis), float64 lerps in the kernel's order"""
    B, h, w, C = x.shape
    ylo, yhi, yl = R.bilinear_axis(h, H)
    xlo, xhi, xl = R.bilinear_axis(w, W)
    top, bot = x[:, ylo], x[:, yhi]
    xl = xl[:, None]
    t = top[:, :, xlo] + (top[:, :, xhi] - top[:, :, xlo]) * xl
    b = bot[:, :, xlo] + (bot[:, :, xhi] - bot[:, :, xlo]) * xl
    return t + (b - t) * yl[:, None, None]


@pytest.mark.parametrize("dt", R.DTS, ids=R.DT_IDS)
@pytest.mark.parametrize("shape", RESIZE_SHAPES, ids=lambda s: "B%d-%dx%d-to-%dx%d" % s)
def test_resize_bilinear(dt, shape):
    """forward into a column block (ldy > C: the columns past C stay untouched); backward = the adjoint of the same resize, from float64
    autograd, into dx with lddx > C"""
    B, h, w, H, W = shape
    C, ldx, ldy = 16, 24, 40
    g = R.gen(35)
    x = R.map_input(B, h * w, C, ldx, dt, g, pad="nan")
    xd = x.to(R.DEV)
    nin, nout = B * h * w, B * H * W

    def run():
        y = R.guarded(nout, ldy, dt)
        R.call("cmpc_resize_bilinear_fwd", dt, xd, ldx, y, ldy, B, h, w, H, W, C)
        return {"y": y}
    y = R.run_twice(run)["y"]
    R.assert_guard(y, nout, "resize_fwd")
    R.assert_sentinel(y[:nout, C:], "resize_fwd columns past C")
    xa = x.double()[:, :C].reshape(B, h, w, C).clone().requires_grad_(True)
    ref = _resize_ref(xa, H, W)
    # two float32 lerps: rounding of the corner values' magnitude
    R.assert_close(y[:nout, :C].reshape(B, H, W, C), ref.detach(), dt, what="resize_fwd", atol=1e-7 * float(x.double()[:, :C].abs().max()))
    dy = R.map_input(B, H * W, C, ldy, dt, g, pad="nan")
    dyd = dy.to(R.DEV)
    ref.backward(dy.double()[:, :C].reshape(B, H, W, C))
    xb = torch.zeros(B, h, w, C, dtype=torch.float64, requires_grad=True)
    _resize_ref(xb, H, W).backward(dy.double()[:, :C].abs().reshape(B, H, W, C))

    def runb():
        dx = R.guarded(nin, ldx, dt)
        R.call("cmpc_resize_bilinear_bwd", dt, dyd, ldy, dx, ldx, B, h, w, H, W, C)
        return {"dx": dx}
    dx = R.run_twice(runb)["dx"]
    R.assert_guard(dx, nin, "resize_bwd")
    R.assert_sentinel(dx[:nin, C:], "resize_bwd columns past C")
    K = max(1, (H * W) // (h * w))
    # a footprint sum of signed terms: rounding bounded by the sum of |terms|
    R.assert_close(dx[:nin, :C].reshape(B, h, w, C), xa.grad, dt, K=K, what="resize_bwd", atol=1e-7 * xb.grad)


# ----------------------------------------------------------------------------------------------------------------------------
# HSV
# ----------------------------------------------------------------------------------------------------------------------------
def _rgb_to_hsv(rgb):
    """tf.image.rgb_to_hsv in float64 on [..., 3] RGB.  The kernel forms the hue as (g - b) * (1 / (6 range)); TF's kernel
    (core/kernels/colorspace_op.h) could not be consulted here, so that float32 ordering is a parity point nobody has checked -- the
    reference uses the exact quotient and the tolerance allows the two float32 roundings"""
    r, g, b = rgb.unbind(-1)
    v = torch.maximum(r, torch.maximum(g, b))
    rng = v - torch.minimum(r, torch.minimum(g, b))
    s = torch.where(v > 0, rng / torch.where(v > 0, v, torch.ones_like(v)), torch.zeros_like(v))
    safe = torch.where(rng > 0, rng, torch.ones_like(rng))
    h = torch.where(r == v, (g - b) / (6 * safe), torch.where(g == v, (b - r) / (6 * safe) + 2.0 / 6, (r - g) / (6 * safe) + 4.0 / 6))
    h = torch.where(rng > 0, h, torch.zeros_like(h))
    h = torch.where(h < 0, h + 1, h)
    return torch.stack([h, s, v], -1)


def _hsv_ref(im, h, w):
    """im [B, H, W, 3] float32 BGR minus mean: + mean in float32 (as the kernel adds it), reversed to RGB, rgb_to_hsv, legacy bilinear"""
    mean = torch.tensor(MEAN_BGR, dtype=torch.float32)
    bgr = (im + mean).double()
    return _resize_ref(_rgb_to_hsv(bgr.flip(-1)), h, w)


def _image(B, H, W, g):
    """random pixels in 0..255, then the edge pixels at the start of sample 0: grey, black, r == g == max, r == b == max, g == b == max,
    a negative hue (r max, g < b), pure colours, white"""
    rgb = torch.rand(B, H, W, 3, generator=g, dtype=torch.float64) * 255
    edges = torch.tensor([[128, 128, 128], [0, 0, 0], [200, 200, 50], [200, 50, 200], [50, 200, 200], [220, 10, 90], [255, 0, 0],
                          [0, 255, 0], [0, 0, 255], [255, 255, 255], [1, 0, 0], [30, 20, 29.99]], dtype=torch.float64)
    flat = rgb.reshape(-1, 3)
    flat[:edges.shape[0]] = edges
    rgb = flat.reshape(B, H, W, 3)
    return (rgb.flip(-1) - torch.tensor(MEAN_BGR, dtype=torch.float64)).float()


# (B, H, W, h, w): identity size (every edge pixel lands on an output unmixed), the shipped 512 -> 64, a non-integer ratio
HSV_SHAPES = [(2, 8, 6, 8, 6), (1, 512, 512, 64, 64), (2, 30, 41, 7, 9)]


def _hsv_tol(ref):
    # the hue's (x - y) * (1 / (6 range)) and + 2/6 in float32, s = range / v, and the float32 lerps: a few roundings of values <= 255
    return 1e-6 * (1 + ref.abs())


@pytest.mark.parametrize("dt", R.DTS, ids=R.DT_IDS)
@pytest.mark.parametrize("shape", HSV_SHAPES, ids=lambda s: "B%d-%dx%d-to-%dx%d" % s)
def test_hsv_map(dt, shape):
    B, H, W, h, w = shape
    g = R.gen(36)
    im = _image(B, H, W, g)
    imd = im.to(R.DEV)
    ld = 16
    P = B * h * w

    def run():
        out = R.guarded(P, ld, dt)
        R.call("cmpc_hsv_map", dt, imd, out, ld, B, H, W, h, w)
        return {"out": out}
    out = R.run_twice(run)["out"]
    R.assert_guard(out, P, "hsv_map")
    ref = _hsv_ref(im, h, w).reshape(P, 3)
    R.assert_close(out[:P, :3], ref, dt, what="hsv_map", atol=_hsv_tol(ref))
    R.assert_zero(out[:P, 3:], "hsv_map channels 3..ld")


@pytest.mark.parametrize("dt", R.DTS, ids=R.DT_IDS)
@pytest.mark.parametrize("shape", HSV_SHAPES, ids=lambda s: "B%d-%dx%d-to-%dx%d" % s)
def test_hsv_grid(dt, shape):
    """channels 8..10 = HSV, 11 = 1 in grid1 only, 12..15 = 0; channels 0..7 (the position grid) and 16..63 are never touched"""
    B, H, W, h, w = shape
    g = R.gen(37)
    im = _image(B, H, W, g)
    imd = im.to(R.DEV)
    P = B * h * w
    ref = _hsv_ref(im, h, w).reshape(P, 3)
    for with1 in (False, True):
        def run():
            g0, g1 = R.guarded(P, 64, dt), R.guarded(P, 64, dt)
            R.call("cmpc_hsv_grid", dt, imd, g0, g1 if with1 else None, B, H, W, h, w)
            return {"g0": g0, "g1": g1}
        o = R.run_twice(run)
        for k, one in (("g0", 0.0), ("g1", 1.0)):
            if k == "g1" and not with1:
                R.assert_sentinel(o[k], "hsv_grid grid1 (NULL)")
                continue
            what = f"hsv_grid {k}"
            t = o[k]
            R.assert_guard(t, P, what)
            R.assert_sentinel(t[:P, :8], what + " channels 0..7")
            R.assert_sentinel(t[:P, 16:], what + " channels 16..63")
            R.assert_close(t[:P, 8:11], ref, dt, what=what, atol=_hsv_tol(ref))
            assert bool((t[:P, 11].cpu() == one).all()), what + " channel 11"
            R.assert_zero(t[:P, 12:16], what + " channels 12..15")


# ----------------------------------------------------------------------------------------------------------------------------
# sequence helpers, conv_to1
# ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [1, 5, 25])
def test_reverse_sequence(T):
    """out[b, t] = in[b, t < n ? n - 1 - t : t], n = seq_len clamped to [0, T]: seq_len 0, 1, T, T + 3 and -1 (exact)"""
    g = R.gen(38)
    lens = [0, 1, T, T + 3, -1]
    B, ld = len(lens), 24
    x = torch.randn(B, T, ld, generator=g)
    words = torch.randint(0, 1000, (B, T), generator=g, dtype=torch.int32)
    sl = torch.tensor(lens, dtype=torch.int32)
    ref = x.clone()
    wref = words.clone()
    for b, n in enumerate(lens):
        n = min(max(n, 0), T)
        ref[b, :n] = x[b, :n].flip(0)
        wref[b, :n] = words[b, :n].flip(0)
    out = R.guarded(B * T, ld, torch.float32)
    otb = R.guarded(B * T, 1, torch.int32)
    R.call("cmpc_reverse_sequence", x.to(R.DEV), out, sl.to(R.DEV), B, T, ld)
    R.call("cmpc_reverse_words_tb", words.to(R.DEV), sl.to(R.DEV), otb, B, T)
    torch.cuda.synchronize()
    R.assert_guard(out, B * T, "reverse_sequence")
    R.assert_guard(otb, B * T, "reverse_words_tb")
    assert torch.equal(out[:B * T].cpu().reshape(B, T, ld), ref), "reverse_sequence"
    assert torch.equal(otb[:B * T, 0].cpu().reshape(T, B), wref.t()), "reverse_words_tb"


def test_rows_nonzero2():
    """mask[r] = (sum |a| + |b| over C columns) != 0: all-zero rows, -0.0 only, one subnormal, NaN, inf, and NaN in the pad columns C..ld
    (never read)"""
    C, ld = 20, 32
    rows = []
    for va, vb in ((0.0, 0.0), (-0.0, -0.0), (1e-45, 0.0), (0.0, 1e-40), (float("nan"), 0.0), (0.0, float("inf")), (float("-inf"), 0.0),
                   (0.0, -3.0), (2.5, 0.0)):
        for col in (0, C - 1):
            a = torch.zeros(ld)
            b = torch.zeros(ld)
            a[C:] = float("nan")
            b[C:] = float("nan")
            a[col], b[col] = va, vb
            if str(va) == "-0.0":
                a[:C], b[:C] = -0.0, -0.0
            rows.append((a, b))
    a = torch.stack([r[0] for r in rows])
    b = torch.stack([r[1] for r in rows])
    n = a.shape[0]
    ref = ((a[:, :C].double().abs() + b[:, :C].double().abs()).sum(1) != 0).float()
    mask = R.guarded(n, 1, torch.float32)
    R.call("cmpc_rows_nonzero2", a.to(R.DEV), b.to(R.DEV), mask, n, ld, C)
    torch.cuda.synchronize()
    R.assert_guard(mask, n, "rows_nonzero2")
    assert torch.equal(mask[:n, 0].cpu(), ref), (mask[:n, 0].cpu(), ref)


# (R, C, ld): R > 4 x 512 (the backward's grid cap: its loop strides), R > 4 x 8192 (the forward's), C in {1, 250, 256, 2048}
CONV1_SHAPES = [(2100, 1, 8), (5000, 250, 256), (2049, 256, 264), (2500, 2048, 2048), (33000, 24, 64)]


@pytest.mark.parametrize("dt", R.DTS, ids=R.DT_IDS)
@pytest.mark.parametrize("shape", CONV1_SHAPES, ids=lambda s: "R%d-C%d-ld%d" % s)
def test_conv_to1(dt, shape):
    """out[r] = x[r, :C] . w + bias; backward dx[r, :] = d[r] w (pad columns 0), dw += sum_r d[r] x[r, :], dbias += sum_r d[r]"""
    Rr, C, ld = shape
    g = R.gen(39)
    x = R.map_input(1, Rr, C, ld, dt, g)
    wv = (torch.randn(C, generator=g) * 0.1).float()
    bias = torch.randn(1, generator=g).float()
    xd, wd, bd = x.to(R.DEV), wv.to(R.DEV), bias.to(R.DEV)

    def run():
        out = R.guarded(Rr, 1, torch.float32)
        R.call("cmpc_conv_to1_fwd", dt, xd, ld, wd, bd, out, Rr, C)
        return {"out": out}
    out = R.run_twice(run)["out"]
    R.assert_guard(out, Rr, "conv_to1_fwd")
    xc = x.double()[:, :C]
    ref = xc @ wv.double() + bias.double()
    # a dot product of C signed terms: rounding bounded by the sum of |terms|
    R.assert_close(out[:Rr, 0], ref, K=C, what="conv_to1_fwd", atol=1e-7 * (xc.abs() @ wv.double().abs() + abs(float(bias))))
    d = torch.randn(Rr, generator=g).float()
    dw0, db0 = torch.randn(C, generator=g).float(), torch.randn(1, generator=g).float()
    dd = d.to(R.DEV)

    def runb():
        dx = R.guarded(Rr, ld, dt)
        dw, db = R.guarded(1, C, torch.float32, dw0), R.guarded(1, 1, torch.float32, db0)
        R.call("cmpc_conv_to1_bwd", dt, dd, xd, ld, wd, dx, dw, db, Rr, C)
        return {"dx": dx, "dw": dw, "db": db}
    o = R.run_twice(runb)
    for k, n in (("dx", Rr), ("dw", 1), ("db", 1)):
        R.assert_guard(o[k], n, "conv_to1_bwd " + k)
    R.assert_close(o["dx"][:Rr, :C], d.double()[:, None] * wv.double(), dt, what="conv_to1_bwd dx")
    R.assert_zero(o["dx"][:Rr, C:], "conv_to1_bwd dx pad")
    # column sums over R rows: rounding bounded by the sum of |terms|
    R.assert_close(o["dw"][0], dw0.double() + d.double() @ xc, K=Rr, what="conv_to1_bwd dw",
                   atol=R.sum_atol(d.double()[:, None] * xc, 0) + 1e-7 * dw0.double().abs())
    R.assert_close(o["db"][0], db0.double() + d.double().sum(), K=Rr, what="conv_to1_bwd dbias",
                   atol=R.sum_atol(d.double(), 0) + 1e-7 * db0.double().abs())
