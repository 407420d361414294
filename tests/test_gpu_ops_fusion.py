"""Op-level tests of csrc/ops_fusion.hip against float64 references: softmax_n_fwd/bwd, l2norm_all_fwd/bwd, exchange_combine_fwd/bwd
(two branches, one branch, db1 / db2 present and NULL, accumulate_dfeat) and mutan_fwd/bwd (pre_tanh 0 and 1), in f32, bf16 and f16
storage where the entry point takes a dtype.  Maps have zero pad columns (the producers' contract); the per-sample gate vectors g carry
garbage past C (their pad channels are never part of a result)."""
import pytest
import torch

from tests import opref as R
from tests.util import O

pytestmark = pytest.mark.gpu

DTS = pytest.mark.parametrize("dt", R.DTS, ids=R.DT_IDS)
SHAPES = pytest.mark.parametrize("shape", R.clip_shapes(1024), ids=R.shape_id)       # these kernels keep <= 2 column blocks: ld <= 1024


@pytest.mark.parametrize("B,N", [(1, 1), (3, 49), (8, 1600), (2, 4097)])
def test_softmax_n_and_l2norm_all(B, N):
    """softmax over the N nodes of each sample and its backward; tf.nn.l2_normalize over a whole [B, N] tensor and its backward
    (cmpc.h:174-179)"""
    g = R.gen(31)
    x = (torch.randn(B, N, generator=g, dtype=torch.float64) * 4).float()
    xa = x.double().clone().requires_grad_(True)
    y = torch.softmax(xa, 1)
    xd = x.to(R.DEV)

    def run():
        a = R.guarded(B, N, torch.float32)
        R.call("cmpc_softmax_n_fwd", xd, a, B, N)
        return {"a": a}
    a = R.run_twice(run)["a"]
    R.assert_guard(a, B, "softmax_n_fwd")
    R.assert_close(a[:B], y.detach(), K=N, what="softmax_n_fwd")
    dy = torch.randn(B, N, generator=g).float()
    y.backward(dy.double())
    a_s, dyd = a[:B].contiguous(), dy.to(R.DEV)

    def run():
        dx = R.guarded(B, N, torch.float32)
        R.call("cmpc_softmax_n_bwd", dyd, a_s, dx, B, N)
        return {"dx": dx}
    dx = R.run_twice(run)["dx"]
    R.assert_guard(dx, B, "softmax_n_bwd")
    R.assert_close(dx[:B], xa.grad, K=N, what="softmax_n_bwd", atol=R.sum_atol(y.detach() * dy.double(), 1)[:, None] * y.detach())

    n = B * N
    for scale in (1.0, 1e-9):                  # 1e-9: sum x^2 < eps, the clamped branch
        xa = (x.double() * scale).float().double().clone().requires_grad_(True)
        yr = O.l2_normalize(xa)
        xs = xa.detach().float().to(R.DEV)

        def run():
            yy, rs = R.guarded(n, 1, torch.float32), R.guarded(1, 1, torch.float32)
            R.call("cmpc_l2norm_all_fwd", xs, yy, rs, n)
            return {"y": yy, "rs": rs}
        o = R.run_twice(run)
        R.assert_guard(o["y"], n, "l2norm_all_fwd"); R.assert_guard(o["rs"], 1, "l2norm_all_fwd rstd")
        R.assert_close(o["y"][:n, 0], yr.detach().reshape(-1), K=n, what=f"l2norm_all_fwd scale {scale}")
        ss = float((xa.detach() ** 2).sum())
        rs_ref = (1.0 / max(ss, 1e-12) ** 0.5) * (-1 if ss < 1e-12 else 1)
        R.assert_close(o["rs"][0, 0:1], torch.tensor([rs_ref], dtype=torch.float64), K=n, what="l2norm_all_fwd rstd")
        yr.backward(dy.double())
        y_s, rs_s = o["y"][:n].contiguous(), o["rs"][:1].contiguous()

        def run():
            dxx = R.guarded(n, 1, torch.float32)
            R.call("cmpc_l2norm_all_bwd", dyd, y_s, rs_s, dxx, n)
            return {"dx": dxx}
        dxx = R.run_twice(run)["dx"]
        R.assert_guard(dxx, n, "l2norm_all_bwd")
        yv, dv = yr.detach().reshape(-1), dy.double().reshape(-1)
        # dy - y (dy . y) cancels: rounding bounded by |rstd| (|dy| + |y| sum |dy y|), not by the result
        R.assert_close(dxx[:n, 0], xa.grad.reshape(-1), K=n, what=f"l2norm_all_bwd scale {scale}",
                       atol=3e-7 * abs(rs_ref) * (dv.abs() + yv.abs() * float((dv * yv).abs().sum())))


@DTS
@SHAPES
def test_exchange_combine(dt, shape):
    """out = l2norm_rows(feat + r1 g1[b] + r2 g2[b]) (cmpc.h:180-187) and its backward: dfeat (+)= dE, dp1 = dE g1 [r1 > 0], dp2 likewise,
    dg1 / dg2 [B][ld_g] += sum_n dE r, db1 / db2 [C] += column sums of dp1 / dp2 as stored -- with two branches and with one
    (r2 = g2 = NULL), with db present and NULL"""
    B, N, C, ld = shape
    g = R.gen(32)
    Rr, ld_g = B * N, ld + 8
    feat = R.map_input(B, N, C, ld, dt, g)
    r1 = R.map_input(B, N, C, ld, dt, g).double().clamp(min=0).to(R.TDT[dt])     # relu outputs of the trans_feat convolutions
    r2 = R.map_input(B, N, C, ld, dt, g).double().clamp(min=0).to(R.TDT[dt])
    g1 = torch.randn(B, ld_g, generator=g).float(); g1[:, C:] = float("nan")
    g2 = torch.randn(B, ld_g, generator=g).float(); g2[:, C:] = float("nan")
    fd, r1d, r2d, g1d, g2d = (t.to(R.DEV) for t in (feat, r1, r2, g1, g2))
    for two in (True, False):
        F_, A1, A2 = feat.double()[:, :C], r1.double()[:, :C], r2.double()[:, :C]
        G1 = g1.double()[:, :C].repeat_interleave(N, 0).clone().requires_grad_(True)
        G2 = g2.double()[:, :C].repeat_interleave(N, 0).clone().requires_grad_(True)
        Fa = F_.clone().requires_grad_(True)
        E = Fa + A1 * G1 + (A2 * G2 if two else 0)
        out_ref = O.l2_normalize(E, 1)

        def run():
            out, rs = R.guarded(Rr, ld, dt), R.guarded(Rr, 1, torch.float32)
            R.call("cmpc_exchange_combine_fwd", dt, fd, r1d, r2d if two else None, g1d, g2d if two else None, ld_g, out, rs, B, N, ld, C)
            return {"out": out, "rs": rs}
        o = R.run_twice(run)
        what = f"exchange_combine_fwd(two={two})"
        R.assert_guard(o["out"], Rr, what); R.assert_guard(o["rs"], Rr, what)
        R.assert_close(o["out"][:Rr, :C], out_ref.detach(), dt, K=C, what=what + " out")
        R.assert_zero(o["out"][:Rr, C:], what + " pad")

        # backward from the stored out / rstd (the kernel's inputs): dE restated (cmpc.h:183), the rest by autograd of E
        out_s, rs_s = o["out"][:Rr].contiguous(), o["rs"][:Rr, 0].contiguous()
        dout = R.map_input(B, N, C, ld, dt, g)
        df0 = R.map_input(B, N, C, ld, dt, g)
        dg10 = torch.randn(B, ld_g, generator=g).float()
        dg20 = torch.randn(B, ld_g, generator=g).float()
        db10 = torch.randn(1, ld, generator=g).float()
        db20 = torch.randn(1, ld, generator=g).float()
        OS, RS, DO = out_s.double().cpu()[:, :C], rs_s.double().cpu()[:, None], dout.double()[:, :C]
        dot = torch.where(RS < 0, torch.zeros_like(RS), (DO * OS).sum(1, keepdim=True))
        dE = RS.abs() * (DO - OS * dot)
        E.backward(dE)
        dp1 = R.rnd(dE * g1.double()[:, :C].repeat_interleave(N, 0) * (A1 > 0), dt)
        dp2 = R.rnd(dE * g2.double()[:, :C].repeat_interleave(N, 0) * (A2 > 0), dt)
        doutd = dout.to(R.DEV)
        for with_db, acc in ((True, 1), (False, 0)):
            def run():
                dfeat = R.guarded(Rr, ld, dt, df0)
                p1, p2 = R.guarded(Rr, ld, dt), R.guarded(Rr, ld, dt)
                dg1 = R.guarded(B, ld_g, torch.float32, dg10); dg2 = R.guarded(B, ld_g, torch.float32, dg20)
                R.sentinel_fill(dg1[:B, C:]); R.sentinel_fill(dg2[:B, C:])
                db1 = R.guarded(1, ld, torch.float32, db10); db2 = R.guarded(1, ld, torch.float32, db20)
                R.call("cmpc_exchange_combine_bwd", dt, doutd, out_s, rs_s, r1d, r2d if two else None, g1d, g2d if two else None, ld_g,
                       dfeat, acc, p1, p2, dg1, dg2, db1 if with_db else None, db2 if (with_db and two) else None, B, N, ld, C)
                return {"dfeat": dfeat, "p1": p1, "p2": p2, "dg1": dg1, "dg2": dg2, "db1": db1, "db2": db2}
            o2 = R.run_twice(run)
            w2 = f"exchange_combine_bwd(two={two}, db={with_db}, acc={acc})"
            for k in ("dfeat", "p1", "p2"):
                R.assert_guard(o2[k], Rr, w2 + " " + k)
            for k in ("dg1", "dg2"):
                R.assert_guard(o2[k], B, w2 + " " + k)
            R.assert_close(o2["dfeat"][:Rr, :C], dE + (df0.double()[:, :C] if acc else 0), dt, K=C, what=w2 + " dfeat")
            R.assert_zero(o2["dfeat"][:Rr, C:], w2 + " dfeat pad")
            R.assert_close(o2["p1"][:Rr, :C], dp1, dt, K=C, what=w2 + " dp1")
            R.assert_zero(o2["p1"][:Rr, C:], w2 + " dp1 pad")
            if two:
                R.assert_close(o2["p2"][:Rr, :C], dp2, dt, K=C, what=w2 + " dp2")
            else:
                R.assert_sentinel(o2["p2"][:Rr], w2 + " dp2 (one branch)")
            t1 = (dE * A1).reshape(B, N, C)
            # sums over the nodes of signed terms: rounding bounded by the sum of |terms|
            R.assert_close(o2["dg1"][:B, :C], dg10.double()[:, :C] + t1.sum(1), K=N, what=w2 + " dg1", atol=R.sum_atol(t1, 1))
            R.assert_sentinel(o2["dg1"][:B, C:], w2 + " dg1 pad")
            if two:
                t2 = (dE * A2).reshape(B, N, C)
                R.assert_close(o2["dg2"][:B, :C], dg20.double()[:, :C] + t2.sum(1), K=N, what=w2 + " dg2", atol=R.sum_atol(t2, 1))
            else:
                assert torch.equal(o2["dg2"][:B, :C].cpu(), dg20[:, :C]), w2 + " dg2 written with one branch"
            if with_db:
                # the kernel sums dp1 as stored; the reference rounds float64 values, which may land one 16-bit ulp away per term
                R.assert_close(o2["db1"][0, :C], db10.double()[0, :C] + dp1.sum(0), K=Rr, what=w2 + " db1",
                               atol=R.sum_atol(dp1, 0) + R.ULP[dt] * dp1.abs().sum(0))
            else:
                assert torch.equal(o2["db1"][:1].cpu(), db10), w2 + " db1 written while NULL"
            if with_db and two:
                R.assert_close(o2["db2"][0, :C], db20.double()[0, :C] + dp2.sum(0), K=Rr, what=w2 + " db2",
                               atol=R.sum_atol(dp2, 0) + R.ULP[dt] * dp2.abs().sum(0))
            else:
                assert torch.equal(o2["db2"][:1].cpu(), db20), w2 + " db2 written while NULL"


@DTS
@SHAPES
@pytest.mark.parametrize("pre_tanh", [0, 1])
def test_mutan(dt, shape, pre_tanh):
    """mutan_fwd (cmpc.h:132-136): P [R, 5 ld] -> tanh(P_h) in place (read only when pre_tanh), X1 = l2norm(tanh(sum_h tanh(P_h) g_h));
    mutan_bwd (cmpc.h:143-145): Th -> dP_h, dg [B][5 ld] += column sums.  P's tanh values are a documented 16-bit intermediate: the
    backward reference starts from them as stored."""
    B, N, C, ld = shape
    g = R.gen(33)
    Rr = B * N
    P = torch.randn(Rr, 5, ld, generator=g, dtype=torch.float64) * 1.5
    P[..., C:] = 0
    if pre_tanh:
        P = torch.tanh(P)
    P = P.to(R.TDT[dt])
    gg = torch.tanh(torch.randn(B, 5, ld, generator=g, dtype=torch.float64))
    gg[..., C:] = float("nan")                      # lang_trans pad channels are never part of a result
    gg = gg.float()
    gd = gg.to(R.DEV)
    Th = P.double()[..., :C] if pre_tanh else torch.tanh(P.double()[..., :C])
    Gb = gg.double()[..., :C].repeat_interleave(N, 0)

    def run():
        Pb = R.guarded(Rr, 5 * ld, dt, P)
        X1, rs = R.guarded(Rr, ld, dt), R.guarded(Rr, 1, torch.float32)
        R.call("cmpc_mutan_fwd", dt, Pb, gd, X1, rs, B, N, ld, C, pre_tanh)
        return {"P": Pb, "X1": X1, "rs": rs}
    o = R.run_twice(run)
    R.assert_guard(o["P"], Rr, "mutan_fwd P"); R.assert_guard(o["X1"], Rr, "mutan_fwd X1"); R.assert_guard(o["rs"], Rr, "mutan_fwd rstd")
    Ps = o["P"][:Rr].cpu().reshape(Rr, 5, ld)
    if pre_tanh:
        assert torch.equal(R._bits(Ps), R._bits(P)), "mutan_fwd wrote P with pre_tanh"
    else:
        R.assert_close(Ps[..., :C], Th, dt, what="mutan_fwd tanh(P)")
        R.assert_zero(Ps[..., C:], "mutan_fwd P pad")
    Z = torch.tanh((Th * Gb).sum(1))
    zn = ((Th * Gb).abs().sum(1) * torch.rsqrt((Z * Z).sum(1, keepdim=True).clamp(min=1e-12)))
    # sum_h tanh(P_h) g_h cancels: rounding bounded by rstd sum_h |tanh(P_h) g_h|, not by |X1|
    R.assert_close(o["X1"][:Rr, :C], O.l2_normalize(Z, 1), dt, K=5 * C, what="mutan_fwd X1", atol=1e-7 * zn)
    R.assert_zero(o["X1"][:Rr, C:], "mutan_fwd X1 pad")

    # backward from the stored Th, X1 and rstd
    Th_s = Ps.double()[..., :C].clone().requires_grad_(True)
    Ga = gg.double()[..., :C].clone().requires_grad_(True)
    X1s, RS = o["X1"][:Rr].double().cpu()[:, :C], o["rs"][:Rr].double().cpu()
    dX1 = R.map_input(B, N, C, ld, dt, g)
    D = dX1.double()[:, :C]
    dot = torch.where(RS < 0, torch.zeros_like(RS), (D * X1s).sum(1, keepdim=True))
    # the kernel recovers tanh(S) as X1 / |rstd| from the stored X1 (ops_fusion.hip mutan_bwd_kernel): so does the reference
    Zq = X1s / RS.abs()
    dS = RS.abs() * (D - X1s * dot) * (1 - Zq * Zq)
    S = (Th_s * Ga.repeat_interleave(N, 0)).sum(1)
    S.backward(dS)
    dP = Th_s.grad * (1 - Th_s.detach() ** 2)
    dg0 = torch.randn(B, 5, ld, generator=g).float()
    Pin, X1in, rsin, dX1d = o["P"][:Rr].contiguous(), o["X1"][:Rr].contiguous(), o["rs"][:Rr].contiguous(), dX1.to(R.DEV)

    def run():
        Thb = R.guarded(Rr, 5 * ld, dt, Pin.cpu())
        dgb = R.guarded(B, 5 * ld, torch.float32, dg0)
        R.call("cmpc_mutan_bwd", dt, Thb, gd, X1in, rsin, dX1d, dgb, B, N, ld, C)
        return {"dP": Thb, "dg": dgb}
    o2 = R.run_twice(run)
    R.assert_guard(o2["dP"], Rr, "mutan_bwd dP"); R.assert_guard(o2["dg"], B, "mutan_bwd dg")
    dPg = o2["dP"][:Rr].cpu().reshape(Rr, 5, ld)
    R.assert_close(dPg[..., :C], dP, dt, K=C, what="mutan_bwd dP")
    R.assert_zero(dPg[..., C:], "mutan_bwd dP pad")
    dgg = o2["dg"][:B].cpu().reshape(B, 5, ld)
    terms = (Th_s.detach() * dS[:, None, :]).reshape(B, N, 5, C)
    # column sums over the nodes of signed terms: rounding bounded by the sum of |terms|
    R.assert_close(dgg[..., :C], dg0.double()[..., :C] + Ga.grad, K=N, what="mutan_bwd dg", atol=R.sum_atol(terms, 1))
    assert torch.equal(dgg[..., C:], dg0[..., C:]), "mutan_bwd dg pad columns changed"


F32_LOWEST = -3.4028234663852886e38          # tf.float32.min: the logit of a padded word in CMPC_model.py:389-394


def _graph_softmax_ref(A0, pr, mask, T, mask_after):
    """gw_w = softmax_T(mask pr A0 + (1 - mask) float32.min) (mask_after 0) or mask softmax_T(pr A0) (mask_after 1); gw_v =
    softmax_N(pr A0) mask (cmpc.h:147-156), on the first T word columns"""
    a = pr[:, None, :] * A0[..., :T]
    m = mask[:, None, :]
    if mask_after:
        gw = m * torch.softmax(a, 2)
    else:
        gw = torch.softmax(torch.where(m > 0, a, torch.full_like(a, F32_LOWEST)), 2)
    gv = torch.softmax(a, 1) * m
    return gw, gv


# (B, N, T, Tp, seq_len): T < Tp, T = Tp = 64, a sample with seq_len 1, N not a multiple of 64 (chunks of 64 rows)
GS_SHAPES = [(1, 1, 1, 8, (1,)), (3, 49, 20, 24, (20, 1, 7)), (8, 1600, 33, 40, (33, 1, 5, 33, 12, 20, 2, 30)), (2, 4097, 64, 64, (64, 1)),
             (2, 130, 5, 8, (3, 5))]


@pytest.mark.parametrize("dt", R.DTS, ids=R.DT_IDS)
@pytest.mark.parametrize("mask_after", [0, 1])
@pytest.mark.parametrize("shape", GS_SHAPES, ids=lambda s: "B%d-N%d-T%d-Tp%d" % s[:4])
def test_graph_softmax(dt, mask_after, shape):
    """graph_softmax_fwd/bwd: f32 results and their dt copies, pad word columns [T, Tp) written 0, dpr overwritten.  pr is masked
    (pr = parse_R = parse * seq_mask, cmpc_parse_softmax_fwd), as the engine feeds it."""
    B, N, T, Tp, sl = shape
    g = R.gen(34)
    mask = (torch.arange(T)[None, :] < torch.tensor(sl)[:, None]).float()
    A0 = (torch.randn(B, N, Tp, generator=g, dtype=torch.float64) * 2).float()
    A0[..., T:] = float("nan")                      # columns >= T of A0 are never read
    pr = (torch.rand(B, T, generator=g) * mask).float()
    ch = (N + 63) // 64
    A0d, prd, md = A0.to(R.DEV), pr.to(R.DEV), mask.to(R.DEV)
    Aa = A0.double()[..., :T].clone().requires_grad_(True)
    pa = pr.double().clone().requires_grad_(True)
    gw, gv = _graph_softmax_ref(Aa, pa, mask.double(), T, mask_after)

    def run():
        o = {k: R.guarded(B * N, Tp, torch.float32) for k in ("gw", "gv")}
        o.update({k: R.guarded(B * N, Tp, dt) for k in ("gwt", "gvt")})
        scr = torch.full((B * ch * 128,), float("nan"), device=R.DEV)
        R.call("cmpc_graph_softmax_fwd", dt, mask_after, A0d, prd, md, o["gw"], o["gv"], o["gwt"], o["gvt"], scr, B, N, T, Tp)
        return o
    o = R.run_twice(run)
    for k in o:
        R.assert_guard(o[k], B * N, "graph_softmax_fwd " + k)
    for k, kt, ref in (("gw", "gwt", gw), ("gv", "gvt", gv)):
        got = o[k][:B * N].reshape(B, N, Tp)
        R.assert_close(got[..., :T], ref.detach(), K=T if k == "gw" else N, what=f"graph_softmax_fwd {k}")
        R.assert_zero(got[..., T:], f"graph_softmax_fwd {k} pad")
        assert torch.equal(o[kt][:B * N].cpu(), got.reshape(B * N, Tp).cpu().to(R.TDT[dt])), f"graph_softmax_fwd {kt}: not the rounded f32 result"

    dgw = torch.randn(B, N, Tp, generator=g).float()
    dgv = torch.randn(B, N, Tp, generator=g).float()
    (gw * dgw.double()[..., :T] + gv * dgv.double()[..., :T]).sum().backward()
    gw_s, gv_s = o["gw"][:B * N].contiguous(), o["gv"][:B * N].contiguous()
    dgwd, dgvd = dgw.to(R.DEV), dgv.to(R.DEV)

    def run():
        dA, dAt = R.guarded(B * N, Tp, torch.float32), R.guarded(B * N, Tp, dt)
        dpr = R.guarded(B, T, torch.float32)
        scr = torch.full((B * ch * 128,), float("nan"), device=R.DEV)
        R.call("cmpc_graph_softmax_bwd", dt, dgwd, dgvd, gw_s, gv_s, A0d, prd, md, dA, dAt, dpr, scr, B, N, T, Tp)
        return {"dA": dA, "dAt": dAt, "dpr": dpr}
    o2 = R.run_twice(run)
    for k, n in (("dA", B * N), ("dAt", B * N), ("dpr", B)):
        R.assert_guard(o2[k], n, "graph_softmax_bwd " + k)
    dA = o2["dA"][:B * N].reshape(B, N, Tp)
    terms = (gw.detach() * dgw.double()[..., :T]).abs().sum(2, keepdim=True) + gv.detach().abs() * (gv.detach() * dgv.double()[..., :T]).abs().sum(1, keepdim=True)
    # softmax backward subtracts a dot product: rounding bounded by pr (|p dy| + p sum |p dy|), not by |dA0|
    R.assert_close(dA[..., :T], Aa.grad, K=max(T, N), what="graph_softmax_bwd dA0", atol=1e-7 * (terms + gw.detach().abs() + gv.detach().abs()))
    R.assert_zero(dA[..., T:], "graph_softmax_bwd dA0 pad")
    assert torch.equal(o2["dAt"][:B * N].cpu(), o2["dA"][:B * N].cpu().to(R.TDT[dt])), "graph_softmax_bwd dA0_t: not the rounded f32 result"
    dpr = o2["dpr"][:B].cpu()
    live = mask > 0
    dterm = (Aa.grad.abs() * A0.double()[..., :T].abs() / pr.double().clamp(min=1e-3)[:, None, :]).sum(1)
    R.assert_close(dpr[live], pa.grad[live], K=N, what="graph_softmax_bwd dpr", atol=1e-7 * dterm[live])
    # padded words: their parse_R is mask * softmax and takes no gradient upstream; the kernel leaves their dpr 0 (cmpc.h)
    assert bool((dpr[~live] == 0).all()), "graph_softmax_bwd dpr of padded words"
