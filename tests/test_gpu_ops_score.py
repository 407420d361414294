"""Op-level tests of csrc/ops_score.hip against float64 references: score_conv_fwd/bwd (the 3x3 SAME M->1 convolution), upsample_fwd
(legacy bilinear, sigmoid, per-sample BCE, inter / uni counters) and upsample_loss_bwd, in every storage type the entry point takes."""
import pytest
import torch
import torch.nn.functional as F

from tests import opref as R
from tests.util import O

pytestmark = pytest.mark.gpu

# (B, h, w, M, ld): ld <= 512 takes the row kernels, ld > 512 the per-pixel ones; h or w = 1; M not a multiple of 8
CONV_SHAPES = [(1, 1, 1, 24, 64), (3, 7, 7, 72, 136), (2, 5, 1, 1000, 1024), (1, 1, 9, 500, 512), (2, 40, 40, 513, 520),
               (8, 9, 13, 20, 24), (1, 64, 80, 1024, 1024)]


def _conv_ref(feat, Wk, bias, B, h, w, M):
    x = feat.reshape(B, h, w, -1)[..., :M].permute(0, 3, 1, 2)
    k = Wk.reshape(3, 3, M).permute(2, 0, 1)[None].contiguous()                  # Wk[t * M + c], t = ky * 3 + kx
    return F.conv2d(x, k, padding=1)[:, 0] + bias


@pytest.mark.parametrize("dt", R.DTS, ids=R.DT_IDS)
@pytest.mark.parametrize("shape", CONV_SHAPES, ids=lambda s: "B%d-%dx%d-M%d-ld%d" % s)
def test_score_conv(dt, shape):
    """score = conv3x3(feat, Wk) + bias; backward dfeat (+)=, dWk += , dbias += (cmpc.h:215-218).  feat's pad columns are 0 (every
    producer's contract); dfeat's pad columns come back 0 (plain) or unchanged (accumulate)."""
    B, h, w, M, ld = shape
    g = R.gen(11)
    P = B * h * w
    feat = R.map_input(B, h * w, M, ld, dt, g)
    Wk = (torch.randn(9 * M, generator=g, dtype=torch.float64) * 0.1).float()
    bias = torch.randn(1, generator=g).float()
    fd, Wd, bd = feat.to(R.DEV), Wk.to(R.DEV), bias.to(R.DEV)

    def run():
        s = R.guarded(P, 1, torch.float32)
        R.call("cmpc_score_conv_fwd", dt, fd, Wd, bd, s, B, h, w, ld, M)
        return {"s": s}
    s = R.run_twice(run)["s"]
    R.assert_guard(s, P, "score_conv_fwd")
    fa = feat.double().clone().requires_grad_(True)
    wa = Wk.double().clone().requires_grad_(True)
    ba = bias.double().clone().requires_grad_(True)
    ref = _conv_ref(fa, wa, ba, B, h, w, M)
    terms = _conv_ref(feat.double().abs(), Wk.double().abs(), 0, B, h, w, M)
    # a dot product of 9 M signed terms: rounding bounded by the sum of |terms|
    R.assert_close(s[:P, 0], ref.detach().reshape(-1), K=9 * M, what="score_conv_fwd", atol=1e-7 * terms.reshape(-1))

    ds = torch.randn(B, h, w, generator=g, dtype=torch.float64).float()
    ref.backward(ds.double())
    dfeat0 = R.map_input(B, h * w, M, ld, dt, g)
    dW0 = torch.randn(9 * M, generator=g).float()
    db0 = torch.randn(1, generator=g).float()
    dsd = ds.to(R.DEV)
    wabs = torch.zeros(9 * M, dtype=torch.float64, requires_grad=True)
    _conv_ref(feat.double().abs(), wabs, 0, B, h, w, M).backward(ds.double().abs())
    dW_abs = wabs.grad
    fabs = torch.zeros(P, ld, dtype=torch.float64, requires_grad=True)
    _conv_ref(fabs, Wk.double().abs(), 0, B, h, w, M).backward(ds.double().abs())
    df_abs = fabs.grad[:, :M]
    for acc in (0, 1):
        def run():
            df = R.guarded(P, ld, dt, dfeat0)
            dW = R.guarded(9 * M, 1, torch.float32, dW0)
            db = R.guarded(1, 1, torch.float32, db0)
            R.call("cmpc_score_conv_bwd", dt, dsd, fd, Wd, df, acc, dW, db, B, h, w, ld, M)
            return {"df": df, "dW": dW, "db": db}
        o = R.run_twice(run)
        what = f"score_conv_bwd acc={acc}"
        for k, n in (("df", P), ("dW", 9 * M), ("db", 1)):
            R.assert_guard(o[k], n, what + " " + k)
        dfr = fa.grad.reshape(P, ld)[:, :M] + (dfeat0.double()[:, :M] if acc else 0)
        # a 9-tap sum of signed terms: rounding bounded by the per-element sum of |terms|
        R.assert_close(o["df"][:P, :M], dfr, dt, K=9, what=what + " dfeat", atol=1e-7 * df_abs)
        if acc:
            assert torch.equal(o["df"][:P, M:].cpu(), dfeat0[:, M:]), what + " dfeat pad changed"
        else:
            R.assert_zero(o["df"][:P, M:], what + " dfeat pad")
        # sums over the pixels of signed terms: rounding bounded by the sum of |terms|
        R.assert_close(o["dW"][:9 * M, 0], dW0.double() + wa.grad, K=P, what=what + " dWk", atol=1e-7 * dW_abs)
        R.assert_close(o["db"][0, 0:1], db0.double() + ba.grad, K=P, what=what + " dbias", atol=R.sum_atol(ds.double().reshape(1, -1), 1))


# (B, h, w, H, W): the product's ratio 8, non-integer up-ratios, a down-ratio, non-square sizes, h = H
UP_SHAPES = [(2, 40, 40, 320, 320), (1, 7, 7, 50, 50), (3, 40, 40, 321, 321), (2, 20, 10, 8, 5), (2, 10, 30, 57, 211),
             (1, 13, 17, 104, 136), (8, 5, 5, 5, 5)]


def _up_ref(score, H, W):
    """O.resize_bilinear's lerp order, in float64 on the float32 coefficients (O.resize_bilinear takes float64 lerps for float64 input)"""
    B, h, w = score.shape
    ylo, yhi, yl = R.bilinear_axis(h, H)
    xlo, xhi, xl = R.bilinear_axis(w, W)
    top, bot = score[:, ylo], score[:, yhi]
    t = top[:, :, xlo] + (top[:, :, xhi] - top[:, :, xlo]) * xl
    b = bot[:, :, xlo] + (bot[:, :, xhi] - bot[:, :, xlo]) * xl
    return t + (b - t) * yl[:, None]


@pytest.mark.parametrize("shape", UP_SHAPES, ids=lambda s: "B%d-%dx%d-to-%dx%d" % s)
def test_upsample_fwd(shape):
    """up = legacy bilinear(score), sigm = sigmoid(up), loss[b] += sum BCE, inter / uni += |pred & gt|, |pred | gt| (cmpc.h:219-222).
    The counters are checked EXACTLY against the kernel's own `up` (pred = up > 0); sigm / target / loss may be NULL."""
    B, h, w, H, W = shape
    g = R.gen(12)
    score = (torch.randn(B, h, w, generator=g, dtype=torch.float64) * 3).float()
    tgt = (torch.rand(B, H, W, generator=g) > 0.6).float()
    loss0 = torch.randn(B, generator=g).float()
    iu0 = torch.randint(0, 1000, (2, B), generator=g, dtype=torch.int32)
    sd, td = score.to(R.DEV), tgt.to(R.DEV)
    ref = _up_ref(score.double(), H, W)
    for with_sigm, with_t in ((True, True), (False, True), (True, False), (False, False)):
        def run():
            up, sg = R.guarded(B * H * W, 1, torch.float32), R.guarded(B * H * W, 1, torch.float32)
            loss = R.guarded(B, 1, torch.float32, loss0)
            iu = R.guarded(2 * B, 1, torch.int32, iu0)
            R.call("cmpc_upsample_fwd", sd, up, sg if with_sigm else None, td if with_t else None, loss if with_t else None,
                   iu[:B] if with_t else None, iu[B:] if with_t else None, B, h, w, H, W)
            return {"up": up, "sg": sg, "loss": loss, "iu": iu}
        o = R.run_twice(run)
        what = f"upsample_fwd(sigm={with_sigm}, target={with_t})"
        for k, n in (("up", B * H * W), ("sg", B * H * W), ("loss", B), ("iu", 2 * B)):
            R.assert_guard(o[k], n, what + " " + k)
        up = o["up"][:B * H * W, 0].reshape(B, H, W).cpu()
        R.assert_close(up, ref, what=what + " up", atol=1e-7 * float(score.abs().max()))
        if with_sigm:
            R.assert_close(o["sg"][:B * H * W, 0].reshape(B, H, W), torch.sigmoid(up.double()), what=what + " sigm")
        else:
            R.assert_sentinel(o["sg"], what + " sigm (NULL)")
        if with_t:
            bce = O.sigmoid_xent(up.double(), tgt.double()).reshape(B, -1).sum(1)
            R.assert_close(o["loss"][:B, 0], loss0.double() + bce, K=H * W, what=what + " loss")
            pr, gt = up > 0, tgt != 0
            inter = (pr & gt).reshape(B, -1).sum(1).int() + iu0[0]
            uni = (pr | gt).reshape(B, -1).sum(1).int() + iu0[1]
            assert torch.equal(o["iu"][:B, 0].cpu(), inter), what + " inter"
            assert torch.equal(o["iu"][B:2 * B, 0].cpu(), uni), what + " uni"
        else:
            assert torch.equal(o["loss"][:B, 0].cpu(), loss0) and torch.equal(o["iu"][:2 * B, 0].cpu(), iu0.reshape(-1))


@pytest.mark.parametrize("shape", UP_SHAPES, ids=lambda s: "B%d-%dx%d-to-%dx%d" % s)
def test_upsample_loss_bwd(shape):
    """dscore = sum over the bilinear footprint of wscale (sigmoid(up) - target) (cmpc.h:223-225): the adjoint of the legacy resize,
    from torch.autograd on the float64 forward with the same upstream gradient"""
    B, h, w, H, W = shape
    g = R.gen(13)
    up = (torch.randn(B, H, W, generator=g, dtype=torch.float64) * 3).float()
    tgt = (torch.rand(B, H, W, generator=g) > 0.5).float()
    wscale = 0.37
    sa = torch.zeros(B, h, w, dtype=torch.float64, requires_grad=True)
    d = wscale * (torch.sigmoid(up.double()) - tgt.double())
    _up_ref(sa, H, W).backward(d)
    sb = torch.zeros(B, h, w, dtype=torch.float64, requires_grad=True)
    _up_ref(sb, H, W).backward(d.abs())              # the same footprint sums over |terms|
    ud, td = up.to(R.DEV), tgt.to(R.DEV)

    def run():
        ds = R.guarded(B * h * w, 1, torch.float32)
        R.call("cmpc_upsample_loss_bwd", ud, td, ds, wscale, B, h, w, H, W)
        return {"ds": ds}
    ds = R.run_twice(run)["ds"]
    R.assert_guard(ds, B * h * w, "upsample_loss_bwd")
    K = max(1, (H * W) // (h * w))
    # a footprint sum of signed terms: rounding bounded by the sum of |terms|
    R.assert_close(ds[:B * h * w, 0].reshape(B, h, w), sa.grad, K=K, what="upsample_loss_bwd", atol=1e-7 * sb.grad)
