"""Op-level tests of csrc/ops_norm.hip against float64 references: cast, axpy, bias_act_res, act_bwd, wcolsum, rowdot1, rank1_update,
l2norm_rows_fwd/bwd, sample_stats, gconv_pre_fwd/bwd, gconv_post_fwd/bwd -- in f32, bf16 and f16 storage, at the shapes of
tests/opref.MAP_SHAPES.  Input maps carry zero pad columns [C, ld) (what every producer writes, include/cmpc.h conventions); per-channel
vectors (v, gamma, beta) carry garbage past C ("values beyond C are never used", ops_norm.hip).  Outputs have sentinel guard rows."""
import pytest
import torch

from tests import opref as R
from tests.util import O

pytestmark = pytest.mark.gpu

DTS = pytest.mark.parametrize("dt", R.DTS, ids=R.DT_IDS)
SHAPES = pytest.mark.parametrize("shape", R.MAP_SHAPES, ids=R.shape_id)


def _vec(rows, ld, C, g, scale=1.0, offset=0.0, pad=3.0):
    """per-channel vectors with finite garbage past C (NaN would vanish inside fmaxf / relu and hide a pad column used as valid)"""
    v = torch.randn(rows, ld, generator=g, dtype=torch.float64) * scale + offset
    v[:, C:] = pad
    return v.float()


# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("src", R.DTS, ids=R.DT_IDS)
@pytest.mark.parametrize("dst", R.DTS, ids=R.DT_IDS)
def test_cast(src, dst):
    """cmpc_cast (cmpc.h:99): round to nearest even at ties, f16 overflow to inf, NaN / inf / signed zero / subnormals kept"""
    g = R.gen(1)
    n = 100003
    x = torch.randn(n, generator=g, dtype=torch.float64) * 3
    x[:12] = torch.tensor([0.0, -0.0, float("inf"), -float("inf"), 70000.0, -65520.0, 65504.0, 1e-6, 3e-8, 1e-40, float("nan"), 65519.0])
    # exact ties of the 16-bit grids: 1 + 2^-8 + k 2^-7 (bf16) and 1 + 2^-11 + k 2^-10 (f16), both rounding directions
    k = torch.arange(1000, dtype=torch.float64)
    x[100:1100] = 1 + 2.0 ** -8 + k * 2.0 ** -7
    x[1100:2100] = -(1 + 2.0 ** -11 + k * 2.0 ** -10)
    xs = x.to(R.TDT[src])
    ref = xs.float().to(R.TDT[dst]) if dst != R.F32 else xs.float()   # torch's CPU conversions round to nearest even
    s = xs.to(R.DEV)
    out = R.guarded(n, 1, dst)

    def run():
        R.sentinel_fill(out[:n])
        R.call("cmpc_cast", src, s, dst, out, n)
        return {"out": out.clone()}
    o = R.run_twice(run)["out"]
    R.assert_guard(o, n, "cast")
    got = o[:n, 0].cpu()
    nan = torch.isnan(ref)
    assert torch.equal(torch.isnan(got), nan)
    assert torch.equal(R._bits(got[~nan]), R._bits(ref[~nan])), "cast: not bit-identical to round-to-nearest-even"
    if dst == R.F16 and src == R.F32:
        assert got[4] == float("inf") and got[5] == -float("inf") and got[11] == 65504.0


@DTS
@pytest.mark.parametrize("n", [8, 4096, 1000008])
def test_axpy(dt, n):
    """y += a x elementwise (cmpc.h:116-117)"""
    g = R.gen(2)
    x = torch.randn(n, generator=g, dtype=torch.float64).to(R.TDT[dt])
    y0 = torch.randn(n, generator=g, dtype=torch.float64).to(R.TDT[dt])
    a = -0.7
    xd = x.to(R.DEV)

    def run():
        y = R.guarded(n, 1, dt, y0)
        R.call("cmpc_axpy", dt, xd, y, a, n)
        return {"y": y}
    y = R.run_twice(run)["y"]
    R.assert_guard(y, n, "axpy")
    R.assert_close(y[:n, 0], y0.double() + a * x.double(), dt, what="axpy")


@DTS
@pytest.mark.parametrize("C", [8, 24, 1000, 2048])
@pytest.mark.parametrize("res", [False, True])
@pytest.mark.parametrize("relu", [0, 1])
def test_bias_act_res(dt, C, res, relu):
    """y = relu?(y + bias[c] (+ res)) in place on an NHWC [R, C] map (cmpc.h:113-115)"""
    g = R.gen(3)
    Rr = 777
    y0 = torch.randn(Rr, C, generator=g, dtype=torch.float64).to(R.TDT[dt])
    rs = torch.randn(Rr, C, generator=g, dtype=torch.float64).to(R.TDT[dt])
    bias = torch.randn(C, generator=g).float()
    ref = y0.double() + bias.double() + (rs.double() if res else 0)
    if relu:
        ref = ref.clamp(min=0)
    rd, bd = rs.to(R.DEV), bias.to(R.DEV)

    def run():
        y = R.guarded(Rr, C, dt, y0)
        R.call("cmpc_bias_act_res", dt, y, bd, rd if res else None, relu, Rr, C)
        return {"y": y}
    y = R.run_twice(run)["y"]
    R.assert_guard(y, Rr, "bias_act_res")
    R.assert_close(y[:Rr], ref, dt, what="bias_act_res")


# ---------------------------------------------------------------------------------------------------------------------------
ACTS = {0: lambda y: torch.ones_like(y), 1: lambda y: (y > 0).double(), 2: lambda y: 1 - y * y, 3: lambda y: y * (1 - y)}


@DTS
@SHAPES
@pytest.mark.parametrize("act", [0, 1, 2, 3], ids=["none", "relu", "tanh", "sigmoid"])
def test_act_bwd(dt, shape, act):
    """dpre = dy * act'(y); db[c] += sum_r dpre; dsb[b][c] += per-sample sums (cmpc.h:100-104).  dy / y / dpre are windows of a matrix
    with row stride `stride` > ld; the columns between ld and stride belong to someone else and stay untouched."""
    B, N, C, ld = shape
    g = R.gen(4)
    Rr, stride = B * N, ld + 8
    dy = R.map_input(B, N, C, stride, dt, g)
    yv = R.map_input(B, N, C, stride, dt, g)
    if act == 3:
        yv = torch.sigmoid(yv.double()).to(R.TDT[dt])
    elif act == 2:
        yv = torch.tanh(yv.double()).to(R.TDT[dt])
    yv[:, C:] = 0
    dy[:, C:ld] = 0
    dy[:, ld:] = 5.0          # beyond the window: never read into a result
    db0 = _vec(1, ld + 8, C, g, pad=0.0)
    dsb0 = _vec(B, ld + 8, C, g, pad=0.0)
    dyd, yd = dy.to(R.DEV), yv.to(R.DEV)
    dpre_ref = dy.double()[:, :ld] * ACTS[act](yv.double()[:, :ld])
    dpre_ref[:, C:] = 0
    for with_y, with_dpre, with_dsb in ((True, True, True), (act == 0, False, False), (True, True, False)):
        if act != 0 and not with_y:
            continue

        def run():
            dpre = R.guarded(Rr, stride, dt)
            db = R.guarded(1, ld + 8, torch.float32, db0)
            dsb = R.guarded(B, ld + 8, torch.float32, dsb0)
            R.sentinel_fill(db[0, C:]); R.sentinel_fill(dsb[:B, C:])
            R.call("cmpc_act_bwd", dt, dyd, yd if with_y else None, dpre if with_dpre else None, act, Rr, stride, ld, C, db,
                   dsb if with_dsb else None, ld + 8, N if with_dsb else 0)
            return {"dpre": dpre, "db": db, "dsb": dsb}
        o = R.run_twice(run)
        what = f"act_bwd(y={with_y}, dpre={with_dpre}, dsb={with_dsb})"
        R.assert_guard(o["dpre"], Rr, what); R.assert_guard(o["db"], 1, what); R.assert_guard(o["dsb"], B, what)
        if with_dpre:
            R.assert_close(o["dpre"][:Rr, :ld], dpre_ref, dt, what=what + " dpre")
            R.assert_sentinel(o["dpre"][:Rr, ld:], what + " dpre beyond the window")
        else:
            R.assert_sentinel(o["dpre"], what + " dpre (NULL)")
        dq = dpre_ref.reshape(B, N, ld)[..., :C]
        # column sums of signed terms: rounding is bounded by the sum of |terms| (R.sum_atol), not by |sum|
        R.assert_close(o["db"][0, :C], db0[0, :C].double() + dq.sum((0, 1)), R.F32, K=Rr, what=what + " db", atol=R.sum_atol(dq, (0, 1)))
        R.assert_sentinel(o["db"][0, C:], what + " db pad")
        if with_dsb:
            R.assert_close(o["dsb"][:B, :C], dsb0[:, :C].double() + dq.sum(1), R.F32, K=N, what=what + " dsb", atol=R.sum_atol(dq, 1))
            R.assert_sentinel(o["dsb"][:B, C:], what + " dsb pad")
        else:
            R.assert_sentinel(o["dsb"][:B, C:], what + " dsb (NULL)")


# ---------------------------------------------------------------------------------------------------------------------------
@DTS
@SHAPES
def test_wcolsum_rowdot1_rank1(dt, shape):
    """out[b,:] += sum_n w[b,n] x[b,n,:];  s[b,n] = scale x[b,n,:] . v[b,:];  x[b,n,:] += s1 w1 v1 + s2 w2 v2 (cmpc.h:105-112)"""
    B, N, C, ld = shape
    g = R.gen(5)
    Rr = B * N
    x = R.map_input(B, N, C, ld, dt, g)
    w = torch.randn(B, N, generator=g).float()
    w2 = torch.randn(B, N, generator=g).float()
    ldv = ld + 8
    v = _vec(B, ldv, C, g, pad=7.0)          # columns >= C of v are not part of the product
    v2 = _vec(B, ldv, C, g, pad=7.0)
    out0 = _vec(B, ldv, C, g, pad=0.0)
    scale = 0.37
    xd, wd, w2d, vd, v2d = (t.to(R.DEV) for t in (x, w, w2, v, v2))
    X = x.double().reshape(B, N, ld)[..., :C]

    def run():
        out = R.guarded(B, ldv, torch.float32, out0)
        R.sentinel_fill(out[:B, C:])
        R.call("cmpc_wcolsum", dt, xd, wd, out, ldv, B, N, ld, C, scale)
        s = R.guarded(Rr, 1, torch.float32)
        R.call("cmpc_rowdot1", dt, xd, vd, ldv, s, B, N, ld, C, scale)
        return {"out": out, "s": s}
    o = R.run_twice(run)
    R.assert_guard(o["out"], B, "wcolsum"); R.assert_guard(o["s"], Rr, "rowdot1")
    tw = scale * w.double()[..., None] * X
    tv = scale * X * v.double()[:, None, :C]
    # sums of signed terms: rounding is bounded by the sum of |terms| (R.sum_atol), not by |sum|
    R.assert_close(o["out"][:B, :C], out0[:, :C].double() + tw.sum(1), K=N, what="wcolsum", atol=R.sum_atol(tw, 1))
    R.assert_sentinel(o["out"][:B, C:], "wcolsum out pad")
    R.assert_close(o["s"][:Rr, 0], tv.sum(2).reshape(-1), K=C, what="rowdot1", atol=R.sum_atol(tv, 2).reshape(-1))

    for two in (False, True):
        def run1():
            xx = R.guarded(Rr, ld, dt, x)
            R.call("cmpc_rank1_update", dt, xx, wd, vd, w2d if two else None, v2d if two else None, ldv, 0.5, -1.25, B, N, ld, C)
            return {"x": xx}
        xx = R.run_twice(run1)["x"]
        R.assert_guard(xx, Rr, "rank1_update")
        ref = X + 0.5 * w.double()[..., None] * v.double()[:, None, :C]
        if two:
            ref = ref + -1.25 * w2.double()[..., None] * v2.double()[:, None, :C]
        got = xx[:Rr].reshape(B, N, ld)
        R.assert_close(got[..., :C], ref, dt, what=f"rank1_update(two={two})")
        R.assert_zero(got[..., C:], "rank1_update pad")


# ---------------------------------------------------------------------------------------------------------------------------
@DTS
@SHAPES
def test_l2norm_rows(dt, shape):
    """tf.nn.l2_normalize over channels (cmpc.h:119-122, eps 1e-12): y, rstd (negative on the clamped branch), nz_mask; the backward
    from the stored y / rstd (the kernel's inputs), plain and accumulating"""
    B, N, C, ld = shape
    g = R.gen(6)
    Rr = B * N
    x = R.map_input(B, N, C, ld, dt, g)
    x[::5] = 0                                # all-zero rows: clamped branch, nz_mask 0
    if Rr > 2:
        # sum x^2 < eps but non-zero: clamped, nz_mask 1 (2e-7 survives f16 storage as a subnormal; 16 entries keep sum x^2 < 1e-12)
        x[1, :C] = 0
        x[1, :min(C, 16)] = 2e-7
    xd = x.to(R.DEV)
    X = x.double()[:, :C]
    ss = (X * X).sum(1, keepdim=True)
    yref = O.l2_normalize(X, 1)
    for with_nz in (True, False):
        def run():
            y, rs = R.guarded(Rr, ld, dt), R.guarded(Rr, 1, torch.float32)
            nz = R.guarded(Rr, 1, torch.float32)
            R.call("cmpc_l2norm_rows_fwd", dt, xd, y, rs, nz if with_nz else None, Rr, ld, C)
            return {"y": y, "rs": rs, "nz": nz}
        o = R.run_twice(run)
        for k in o:
            R.assert_guard(o[k], Rr, "l2norm_rows_fwd " + k)
        R.assert_close(o["y"][:Rr, :C], yref, dt, K=C, what="l2norm_rows_fwd y")
        R.assert_zero(o["y"][:Rr, C:], "l2norm_rows_fwd y pad")
        rs_ref = torch.rsqrt(ss.clamp(min=1e-12))[:, 0]
        rs_ref = torch.where(ss[:, 0] < 1e-12, -rs_ref, rs_ref)
        R.assert_close(o["rs"][:Rr, 0], rs_ref, K=C, what="l2norm_rows_fwd rstd")
        if with_nz:
            assert torch.equal(o["nz"][:Rr, 0].cpu(), (X.abs().sum(1) != 0).float()), "nz_mask"
        else:
            R.assert_sentinel(o["nz"], "nz_mask (NULL)")
    # backward from the stored forward outputs
    y_s, rs_s = o["y"][:Rr].contiguous(), o["rs"][:Rr, 0].contiguous()
    dy = R.map_input(B, N, C, ld, dt, g)
    dy[rs_s.cpu() < 0] *= 2.0 ** -12          # the clamped rows scale dy by 1e6: keep dx inside the f16 range
    dx0 = R.map_input(B, N, C, ld, dt, g)
    Y, DY, RS = y_s.double().cpu()[:, :C], dy.double()[:, :C], rs_s.double().cpu()
    # restated from the kernel's contract (y and rstd are inputs): dx = |rstd| (dy - y (dy . y)), the dot dropped on the clamped branch
    dot = torch.where(RS[:, None] < 0, torch.zeros_like(RS[:, None]), (DY * Y).sum(1, keepdim=True))
    dref = RS.abs()[:, None] * (DY - Y * dot)
    # the same through autograd of the float64 forward where y is unrounded (f32 storage, unclamped rows)
    if dt == R.F32:
        xa = X.clone().requires_grad_(True)
        O.l2_normalize(xa, 1).backward(DY)
        live = (RS > 0)
        R.assert_close(dref[live], xa.grad[live], K=C, what="restated l2norm backward vs autograd", rtol=1e-5)
    dyd = dy.to(R.DEV)
    for acc in (0, 1):
        def run():
            dx = R.guarded(Rr, ld, dt, dx0)
            R.call("cmpc_l2norm_rows_bwd", dt, dyd, y_s, rs_s, dx, Rr, ld, C, acc)
            return {"dx": dx}
        dx = R.run_twice(run)["dx"]
        R.assert_guard(dx, Rr, "l2norm_rows_bwd")
        R.assert_close(dx[:Rr, :C], dref + (dx0.double()[:, :C] if acc else 0), dt, K=C, what=f"l2norm_rows_bwd acc={acc}")
        R.assert_zero(dx[:Rr, C:], "l2norm_rows_bwd pad")


# ---------------------------------------------------------------------------------------------------------------------------
def _ln_ref(Yd, B, N, C):
    """whole-sample LayerNorm statistics of a [B*N, C] float64 map: mean, rstd per sample (tf_layer_norm, eps 1e-12)"""
    Ys = Yd.reshape(B, N * C)
    mean = Ys.mean(1)
    var = ((Ys - mean[:, None]) ** 2).mean(1)
    return mean, torch.rsqrt(var + 1e-12)


@DTS
@SHAPES
def test_sample_stats_gconv_pre(dt, shape):
    """sample_stats (cmpc.h:124-130) into a NaN-filled stat block; gconv_pre_fwd G = relu(X + LN(Y)) and gconv_pre_bwd
    (cmpc.h:159-165): dX (+)= dG [G > 0], dY = LN backward, dgamma / dbeta +=, bsums (its own NaN-filled stat block)"""
    B, N, C, ld = shape
    g = R.gen(7)
    Rr = B * N
    Y = R.map_input(B, N, C, ld, dt, g, scale=2.0, offset=0.5)
    X = R.map_input(B, N, C, ld, dt, g)
    gamma = _vec(1, ld, C, g, scale=0.3, offset=1.0)[0]
    beta = _vec(1, ld, C, g, scale=0.3)[0]
    Yd_, Xd_, gmd, btd = Y.to(R.DEV), X.to(R.DEV), gamma.to(R.DEV), beta.to(R.DEV)

    def run():
        sums = R.stat_block(B)
        R.call("cmpc_sample_stats", dt, Yd_, sums, B, N, ld, C)
        G = R.guarded(Rr, ld, dt)
        R.call("cmpc_gconv_pre_fwd", dt, Yd_, Xd_, sums, gmd, btd, G, B, N, ld, C)
        return {"sums": sums, "G": G}
    o = R.run_twice(run)
    sums, G = o["sums"], o["G"]
    Yv = Y.double()[:, :C]
    assert not bool(torch.isnan(sums).any()), "sample_stats left NaN in unused stat-block slots"
    tot = sums.sum(1).cpu()
    # sum x cancels: its rounding is bounded by the sum of |x|, not by |sum x|
    R.assert_close(tot[:, 0], Yv.reshape(B, -1).sum(1), K=N * C, what="sample_stats sum x", atol=1e-7 * float(Yv.abs().sum()) / B)
    R.assert_close(tot[:, 1], (Yv * Yv).reshape(B, -1).sum(1), K=N * C, what="sample_stats sum x^2")
    mean, rstd = _ln_ref(Yv, B, N, C)
    Yt = Yv.reshape(B, 1, N, C)
    gref = torch.relu(X.double()[:, :C] + O.tf_layer_norm(Yt, gamma.double()[:C], beta.double()[:C]).reshape(Rr, C))
    R.assert_guard(G, Rr, "gconv_pre_fwd")
    R.assert_close(G[:Rr, :C], gref, dt, K=N * C, what="gconv_pre_fwd G")
    R.assert_zero(G[:Rr, C:], "gconv_pre_fwd pad")

    # backward
    Gs = G[:Rr].contiguous()
    dG = R.map_input(B, N, C, ld, dt, g)
    dX0 = R.map_input(B, N, C, ld, dt, g)
    dgam0 = _vec(1, ld, C, g, pad=0.0)[0]
    dbet0 = _vec(1, ld, C, g, pad=0.0)[0]
    dGd = dG.to(R.DEV)
    mask = (Gs[:, :C].double().cpu() > 0).double()
    dz = dG.double()[:, :C] * mask
    ya = Yt.clone().requires_grad_(True)
    gm = gamma.double()[:C].clone().requires_grad_(True)
    bt = beta.double()[:C].clone().requires_grad_(True)
    O.tf_layer_norm(ya, gm, bt).backward(dz.reshape(B, 1, N, C))
    xh = ((Yv.reshape(B, N * C) - mean[:, None]) * rstd[:, None]).reshape(Rr, C)
    dxh = dz * gamma.double()[:C]
    for acc in (0, 1):
        def run():
            dX = R.guarded(Rr, ld, dt, dX0)
            dY = R.guarded(Rr, ld, dt)
            dgam = R.guarded(1, ld, torch.float32, dgam0)
            dbet = R.guarded(1, ld, torch.float32, dbet0)
            R.sentinel_fill(dgam[0, C:]); R.sentinel_fill(dbet[0, C:])
            bsums = R.stat_block(B)
            R.call("cmpc_gconv_pre_bwd", dt, dGd, Gs, Yd_, sums, gmd, dX, acc, dY, dgam, dbet, bsums, B, N, ld, C)
            return {"dX": dX, "dY": dY, "dgam": dgam, "dbet": dbet, "bsums": bsums}
        o = R.run_twice(run)
        what = f"gconv_pre_bwd acc={acc}"
        for k in ("dX", "dY"):
            R.assert_guard(o[k], Rr, what + " " + k)
            R.assert_zero(o[k][:Rr, C:], what + " " + k + " pad")
        R.assert_guard(o["dgam"], 1, what); R.assert_guard(o["dbet"], 1, what)
        assert not bool(torch.isnan(o["bsums"]).any()), "gconv_pre_bwd left NaN in unused bsums slots"
        R.assert_close(o["dX"][:Rr, :C], dz + (dX0.double()[:, :C] if acc else 0), dt, what=what + " dX")
        # dY: pass 1 stores dxh = dz gamma in dY (a 16-bit intermediate), pass 2 reads it back: half an ulp of |rstd dxh| more
        R.assert_close(o["dY"][:Rr, :C], ya.grad.reshape(Rr, C), dt, K=N * C, what=what + " dY",
                       atol=0.5 * R.ULP[dt] * (rstd.repeat_interleave(N)[:, None] * dxh).abs())
        # column sums of signed terms: the rounding is bounded by the sum of |terms| (atol), not by |sum|
        R.assert_close(o["dgam"][0, :C], dgam0.double()[:C] + gm.grad, K=Rr, what=what + " dgamma", atol=1e-7 * float((dz * xh).abs().sum(0).max()))
        R.assert_close(o["dbet"][0, :C], dbet0.double()[:C] + bt.grad, K=Rr, what=what + " dbeta", atol=1e-7 * float(dz.abs().sum(0).max()))
        R.assert_sentinel(o["dgam"][0, C:], what + " dgamma pad"); R.assert_sentinel(o["dbet"][0, C:], what + " dbeta pad")


@DTS
@SHAPES
def test_gconv_post(dt, shape):
    """gconv_post_fwd out = l2norm(relu(LN(U))), rstd_row; gconv_post_bwd dU, dgamma / dbeta += (cmpc.h:166-171), with the sums from
    sample_stats in a NaN-filled stat block"""
    B, N, C, ld = shape
    g = R.gen(8)
    Rr = B * N
    U = R.map_input(B, N, C, ld, dt, g, scale=1.5, offset=-0.2)
    gamma = _vec(1, ld, C, g, scale=0.3, offset=1.0)[0]
    beta = _vec(1, ld, C, g, scale=0.3)[0]
    Ud, gmd, btd = U.to(R.DEV), gamma.to(R.DEV), beta.to(R.DEV)
    sums = R.stat_block(B)
    R.call("cmpc_sample_stats", dt, Ud, sums, B, N, ld, C)

    def run():
        out, rs = R.guarded(Rr, ld, dt), R.guarded(Rr, 1, torch.float32)
        R.call("cmpc_gconv_post_fwd", dt, Ud, sums, gmd, btd, out, rs, B, N, ld, C)
        return {"out": out, "rs": rs}
    o = R.run_twice(run)
    Uv = U.double()[:, :C]
    ua = Uv.reshape(B, 1, N, C).clone().requires_grad_(True)
    gm = gamma.double()[:C].clone().requires_grad_(True)
    bt = beta.double()[:C].clone().requires_grad_(True)
    h = torch.relu(O.tf_layer_norm(ua, gm, bt)).reshape(Rr, C)
    ss = (h * h).sum(1)
    outref = O.l2_normalize(h, 1)
    R.assert_guard(o["out"], Rr, "gconv_post_fwd"); R.assert_guard(o["rs"], Rr, "gconv_post_fwd rstd_row")
    R.assert_close(o["out"][:Rr, :C], outref.detach(), dt, K=N * C, what="gconv_post_fwd out")
    R.assert_zero(o["out"][:Rr, C:], "gconv_post_fwd pad")
    rsr = torch.rsqrt(ss.detach().clamp(min=1e-12))
    R.assert_close(o["rs"][:Rr, 0], torch.where(ss.detach() < 1e-12, -rsr, rsr), K=N * C, what="gconv_post_fwd rstd_row")

    out_s, rs_s = o["out"][:Rr].contiguous(), o["rs"][:Rr, 0].contiguous()
    dout = R.map_input(B, N, C, ld, dt, g)
    dgam0 = _vec(1, ld, C, g, pad=0.0)[0]
    dbet0 = _vec(1, ld, C, g, pad=0.0)[0]
    # the l2norm part from the kernel's inputs (stored out, rstd_row), then autograd of the float64 LayerNorm + relu
    OS, RS, DO = out_s.double().cpu()[:, :C], rs_s.double().cpu(), dout.double()[:, :C]
    dot = torch.where(RS[:, None] < 0, torch.zeros_like(RS[:, None]), (DO * OS).sum(1, keepdim=True))
    dh = RS.abs()[:, None] * (DO - OS * dot) * (OS > 0).double()
    ln = O.tf_layer_norm(ua, gm, bt)
    ln.backward(dh.reshape(B, 1, N, C))
    mean, rstd = _ln_ref(Uv, B, N, C)
    dxh = dh * gamma.double()[:C]
    doutd = dout.to(R.DEV)

    def run():
        dU = R.guarded(Rr, ld, dt)
        dgam = R.guarded(1, ld, torch.float32, dgam0)
        dbet = R.guarded(1, ld, torch.float32, dbet0)
        bsums = R.stat_block(B)
        R.call("cmpc_gconv_post_bwd", dt, doutd, out_s, rs_s, Ud, sums, gmd, dU, dgam, dbet, bsums, B, N, ld, C)
        return {"dU": dU, "dgam": dgam, "dbet": dbet, "bsums": bsums}
    o = R.run_twice(run)
    R.assert_guard(o["dU"], Rr, "gconv_post_bwd")
    assert not bool(torch.isnan(o["bsums"]).any()), "gconv_post_bwd left NaN in unused bsums slots"
    # dU: pass 1 stores dxh in dU (a 16-bit intermediate) and pass 2 reads it back: half an ulp of |rstd dxh| more
    R.assert_close(o["dU"][:Rr, :C], ua.grad.reshape(Rr, C), dt, K=N * C, what="gconv_post_bwd dU",
                   atol=0.5 * R.ULP[dt] * (rstd.repeat_interleave(N)[:, None] * dxh).abs())
    R.assert_zero(o["dU"][:Rr, C:], "gconv_post_bwd pad")
    xh = ((Uv.reshape(B, N * C) - mean[:, None]) * rstd[:, None]).reshape(Rr, C)
    # column sums of signed terms: the rounding is bounded by the sum of |terms| (atol), not by |sum|
    R.assert_close(o["dgam"][0, :C], dgam0.double()[:C] + gm.grad, K=Rr, what="gconv_post_bwd dgamma", atol=1e-7 * float((dh * xh).abs().sum(0).max()))
    R.assert_close(o["dbet"][0, :C], dbet0.double()[:C] + bt.grad, K=Rr, what="gconv_post_bwd dbeta", atol=1e-7 * float(dh.abs().sum(0).max()))
