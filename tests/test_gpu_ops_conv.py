"""Op-level tests of cmpc_conv_nhwc (csrc/gemm.hip conv_v3_kernel, include/cmpc.h:80-96) against a float64 convolution with TF 'SAME'
padding built here from its definition (not from backbone._same_pad), in f32, bf16 and f16 at 128- and 256-row tiles: k 1 and 3, stride 1
and 2, dilation 1, 2, 4 and >= H, odd / even non-square maps, B 1 and > 1, Cin 64 / 192, Cout 8 / 72, padded row strides ldx / ldw / ldy,
residual (read with stride ldy) with and without ReLU.  Y has sentinel guard rows and sentinel pad columns [Cout, ldy); X and Wt carry NaN
in their pad columns.  Also the backbone's own 3x3 operands (BackboneTrainer.refold) in the forward and in the dX of _conv_dx3."""
import importlib
import types

import pytest
import torch

from tests import opref as R
from tests import opwrap as W

pytestmark = pytest.mark.gpu
F32 = R.F32
BT = importlib.import_module("cmpc-refseg_amd.backbone_train")


def same_pads(n, k, s, d):
    """TF 'SAME': out = ceil(n / s); total pad = max((out - 1) s + (k - 1) d + 1 - n, 0), the smaller half before"""
    out = -(-n // s)
    tot = max((out - 1) * s + (k - 1) * d + 1 - n, 0)
    return out, tot // 2, tot - tot // 2


def conv_ref(X, Wt, k, s, d, dev):
    """X [B, H, W, Cin] float64, Wt [Cout, k, k, Cin] float64 -> (Y [B, Ho, Wo, Cout], norm): explicit zero padding, one product per tap"""
    B, H, Wd, Cin = X.shape
    Ho, pt, pb = same_pads(H, k, s, d)
    Wo, pl, pr = same_pads(Wd, k, s, d)
    Xp = torch.zeros(B, H + pt + pb, Wd + pl + pr, Cin, dtype=torch.float64, device=dev)
    Xp[:, pt:pt + H, pl:pl + Wd] = X.to(dev)
    Wt = Wt.to(dev)
    Y = torch.zeros(B, Ho, Wo, Wt.shape[0], dtype=torch.float64, device=dev)
    N2 = torch.zeros_like(Y)
    for ky in range(k):
        for kx in range(k):
            xt = Xp[:, ky * d:ky * d + (Ho - 1) * s + 1:s, kx * d:kx * d + (Wo - 1) * s + 1:s]
            w = Wt[:, ky, kx]
            Y += xt @ w.t()
            N2 += (xt * xt) @ (w * w).t()
    return Y.cpu(), N2.sqrt().cpu()


# (B, H, W, Cin, Cout, k, stride, dil, ldx_pad, ldw_pad, ldy_pad, res, relu)
CASES = [
    (2, 9, 7, 64, 72, 3, 1, 1, 8, 8, 8, True, True),
    (1, 8, 10, 64, 8, 3, 2, 1, 0, 0, 0, False, True),        # 3x3 stride 2, even map: asymmetric padding (0 before, 1 after)
    (3, 7, 9, 192, 72, 3, 2, 2, 16, 0, 8, True, False),       # odd map at stride 2, residual without ReLU
    (2, 11, 6, 64, 72, 3, 1, 4, 0, 8, 0, False, False),
    (2, 6, 5, 64, 8, 3, 1, 8, 8, 0, 8, True, True),           # dilation >= H, W: only the centre tap sees the image
    (2, 13, 12, 192, 8, 1, 2, 1, 8, 8, 0, False, True),       # 1x1 stride 2
    (1, 5, 5, 64, 72, 1, 1, 1, 0, 0, 8, True, False),
    (2, 160, 160, 64, 72, 1, 1, 1, 8, 8, 8, True, False),     # 51 200 rows: 256-row tiles, residual without ReLU
    (2, 158, 161, 64, 72, 3, 1, 2, 0, 8, 8, True, True),      # 256-row tiles, 3x3 dilated, odd W
    (2, 320, 310, 64, 8, 3, 2, 1, 8, 0, 0, False, True),      # 256-row tiles at stride 2 (160 x 155 out)
]


def _case_seed(case, dt):
    return (sum((i + 1) * v for i, v in enumerate(case)) * 7 + dt) % 100003


def cid(c):
    return "B%d-%dx%d-ci%d-co%d-k%d-s%d-d%d-pad%d.%d.%d-res%d-relu%d" % c


@pytest.mark.parametrize("dt", R.DTS, ids=R.DT_IDS)
@pytest.mark.parametrize("case", CASES, ids=cid)
def test_conv_nhwc(dt, case):
    B, H, Wd, Cin, Cout, k, s, d, px, pw, py, use_res, relu = case
    g = R.gen(_case_seed(case, dt))
    ldx, ldw, ldy = Cin + px, k * k * Cin + pw, Cout + py
    Ho, Wo = -(-H // s), -(-Wd // s)
    M = B * Ho * Wo
    X = torch.randn(B * H * Wd, ldx, generator=g, dtype=torch.float64)
    X[:, Cin:] = float("nan")
    Wt = torch.randn(Cout, ldw, generator=g, dtype=torch.float64) / (k * Cin ** 0.5)
    Wt[:, k * k * Cin:] = float("nan")
    Xs, Ws = X.to(R.TDT[dt]), Wt.to(R.TDT[dt])
    bias = (torch.randn(Cout, generator=g, dtype=torch.float64) * 0.5).float()
    res = torch.randn(M, ldy, generator=g, dtype=torch.float64)
    res[:, Cout:] = float("nan")                     # a residual read past Cout would show
    res = res.to(R.TDT[dt])
    dX, dW, db, dres = Xs.to(R.DEV), Ws.to(R.DEV), bias.to(R.DEV), res.to(R.DEV)

    def run():
        Y = R.guarded(M, ldy, dt)
        with W.LaunchTrace() as t:
            W.conv_nhwc(dt, dX, ldx, dW, ldw, db, Y, ldy, B, H, Wd, Cin, Cout, k, s, d, relu, dres if use_res else None)
        torch.cuda.synchronize()
        assert t.names == ["conv_nhwc"]
        return {"Y": Y}
    Y = R.run_twice(run)["Y"]
    R.assert_guard(Y, M, "conv_nhwc")
    R.assert_sentinel(Y[:M, Cout:], "conv_nhwc pad columns [Cout, ldy)")
    Xr = Xs[:, :Cin].double().reshape(B, H, Wd, Cin)
    Wr = Ws[:, :k * k * Cin].double().reshape(Cout, k, k, Cin)
    acc, nrm = conv_ref(Xr, Wr, k, s, d, R.DEV if M * Cout * k * k * Cin > 1e8 else "cpu")
    acc, nrm = acc.reshape(M, Cout), nrm.reshape(M, Cout)
    pre = acc + bias.double()
    mag = acc.abs() + bias.double().abs()
    if use_res:
        r = res[:, :Cout].double()
        pre, mag = pre + r, mag + r.abs()
    ref = torch.relu(pre) if relu else pre
    R.assert_prod(Y[:M, :Cout].cpu(), ref, dt, k * k * Cin, nrm, 1.0, 4 * R.U24 * mag, f"conv_nhwc {cid(case)} {R.DT_IDS[dt]}",
                  old_tol=2e-2 if dt == R.BF16 else None)


def _refold_3x3(w_hwio, dt):
    """the operands BackboneTrainer.refold (backbone_train.py) makes of one 3x3 layer's fp32 master: (w_ohwi [cout][kh kw cin] for the
    forward, wn [cin][kh kw cout] with the taps reversed for dX), through the project's own code on a one-layer stand-in of the trainer"""
    k, _, cin, cout = w_hwio.shape
    L = dict(off=0, count=w_hwio.numel(), k=k, cin=cin, cout=cout,
             mod=types.SimpleNamespace(w_ohwi=torch.empty(cout, k * k * cin, dtype=torch.float32, device=R.DEV)))
    tr = types.SimpleNamespace(params=w_hwio.reshape(-1).float().to(R.DEV), scale=torch.ones(w_hwio.numel(), device=R.DEV), layers=[L],
                               tdt=R.TDT[dt])
    tr.view = lambda buf, L: BT.BackboneTrainer.view(tr, buf, L)
    BT.BackboneTrainer.refold(tr)
    return L["mod"].w_ohwi.to(R.TDT[dt]), L["wn"]


@pytest.mark.parametrize("dt", R.DTS, ids=R.DT_IDS)
@pytest.mark.parametrize("geo", [(2, 9, 7, 1), (1, 12, 10, 2), (2, 6, 5, 8)], ids=lambda g: "B%d-%dx%d-d%d" % g)
def test_conv_dx3(dt, geo):
    """The backbone's 3x3 forward and dX (backbone_train: refold builds w_ohwi and the flipped, transposed taps wn; _conv_dx3 runs the
    stride-1 atrous convolution of dY with wn): both operands come from BackboneTrainer.refold, the forward Y and dX are checked against
    float64 conv2d and its autograd"""
    B, H, Wd, d = geo
    Cin, Cout = 64, 128                # dX reads the Cout channels of dY: both a multiple of 64, and different so a transposition shows
    g = R.gen(600 + d + dt)
    x = torch.randn(B, H, Wd, Cin, generator=g, dtype=torch.float64).to(R.TDT[dt])
    w_hwio = torch.randn(3, 3, Cin, Cout, generator=g, dtype=torch.float64).float() / (3 * Cin ** 0.5)
    w_ohwi, wn = _refold_3x3(w_hwio, dt)
    w = w_hwio.to(R.TDT[dt]).double()                                   # the values the kernels read, HWIO
    wk = w.permute(3, 2, 0, 1)                                          # OIHW
    dy = torch.randn(B, H, Wd, Cout, generator=g, dtype=torch.float64).to(R.TDT[dt])
    xv = x.double().permute(0, 3, 1, 2).clone().requires_grad_(True)
    y = torch.nn.functional.conv2d(xv, wk, padding=d, dilation=d)
    y.backward(dy.double().permute(0, 3, 1, 2))
    R_ = B * H * Wd
    zb = torch.zeros(max(Cin, Cout), dtype=torch.float32, device=R.DEV)
    # forward through w_ohwi
    Y = R.guarded(R_, Cout, dt)
    W.conv_nhwc(dt, x.reshape(-1, Cin).to(R.DEV), Cin, w_ohwi, 9 * Cin, zb, Y, Cout, B, H, Wd, Cin, Cout, 3, 1, d, False)
    # dX through wn, as _conv_dx3 launches it
    DX = R.guarded(R_, Cin, dt)
    W.conv_nhwc(dt, dy.reshape(-1, Cout).to(R.DEV), Cout, wn, 9 * Cout, zb, DX, Cin, B, H, Wd, Cout, Cin, 3, 1, d, False)
    torch.cuda.synchronize()
    R.assert_guard(Y, R_, "conv forward")
    R.assert_guard(DX, R_, "conv dX")
    ynrm = torch.nn.functional.conv2d(x.double().permute(0, 3, 1, 2) ** 2, wk ** 2, padding=d, dilation=d).permute(0, 2, 3, 1).reshape(-1, Cout)
    yref = y.detach().permute(0, 2, 3, 1).reshape(-1, Cout)
    R.assert_prod(Y[:R_].cpu(), yref, dt, 9 * Cin, ynrm.sqrt(), 1.0, 4 * R.U24 * yref.abs(), f"conv forward (refold w_ohwi) {geo}")
    # the norm of the dX product: the transposed convolution of dY^2 with w^2
    xnrm = torch.nn.functional.conv_transpose2d((dy.double() ** 2).permute(0, 3, 1, 2), wk ** 2, padding=d, dilation=d)
    xref = xv.grad.permute(0, 2, 3, 1).reshape(-1, Cin)
    R.assert_prod(DX[:R_].cpu(), xref, dt, 9 * Cout, xnrm.permute(0, 2, 3, 1).reshape(-1, Cin).sqrt(), 1.0, 4 * R.U24 * xref.abs(),
                  f"conv dX (refold wn) {geo}")
