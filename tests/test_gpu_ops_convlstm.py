"""Op-level tests of csrc/ops_convlstm.hip against float64 references: cmpc_convlstm_a/b/c (one ConvLSTMCell.call step from the gate
pre-activations Yg) and cmpc_convlstm_bwd, in every storage type, plus a 3-step chain as engine.hip's clstm_fwd / clstm_bwd run it.

The reference restates ConvLSTMCell.call (reference util/cell.py:36-79) in float64 torch: peepholes on i and f from c_prev, whole-sample
layer_norm (eps 1e-12) of j, i, f, forget bias 1, c = c f + i tanh(j), peephole on o from the new c, LayerNorm of o and c,
h = sigmoid(o) tanh(LN c); the state is LN c.  Gradients come from float64 autograd.  Each stage is checked from the values the previous
stage actually STORED (16-bit included), so 1-ulp tolerances stay meaningful; one chained comparison covers the whole step.

Tolerance terms beyond opref.assert_close's (each stated where it is used) come from `mag`, the float64 magnitude an output's error scales
with: the sum of |terms| a float32 evaluation passes through.  The gate functions are sigmoid_fast (|error| < 2e-7) and cmpc_tanh
(|error| < 1.2e-7 absolute), cmpc_common.h; both are absolute errors on values in (-1, 1), so they enter as a multiple of the magnitude."""
import math

import pytest
import torch

from tests import opref as R

pytestmark = pytest.mark.gpu

_lib = R._lib
EPS = 1e-12
# (B, N, M, ld): the product shape (M = 500: the last lane's 8 columns straddle M); two column blocks with every grid striding (4096 rows >
# 4 x the 512-row cap of the peephole gradients); a small map; N = 1 with B = 8; M == ld
SHAPES = [(2, 1600, 500, 512), (1, 4096, 1000, 1024), (3, 7, 24, 64), (8, 1, 8, 64), (1, 257, 512, 512)]
# float32 evaluation of a gate expression: one rounding (6e-8) per operation over a few operations, plus the sigmoid_fast / cmpc_tanh
# errors (2e-7, 1.2e-7) -- 4e-7 of the magnitude the expression passes through
U_F32 = 4e-7


def sid(s):
    return "B%d-N%d-M%d-ld%d" % s


def _ln(x):
    """whole-sample normalisation of x [B, N, M]: (xhat, mean, rstd), biased variance, eps 1e-12 (tf.contrib.layers.layer_norm)"""
    m = x.mean((1, 2), keepdim=True)
    r = 1.0 / torch.sqrt(((x - m) ** 2).mean((1, 2), keepdim=True) + EPS)
    return (x - m) * r, m, r


def _lnin_mag(x, g, b):
    """magnitude of the float32 error of LN(x) g + b as the kernels form it ((x - mean) * rstd * gamma + beta)"""
    _, m, r = _ln(x)
    return (x.abs() + m.abs()) * r * g.abs() + b.abs()


def cell(Yg, c, W, g, b):
    """ConvLSTMCell.call from the gate pre-activations.  Yg [B, N, 4, M] (j, i, f, o), c [B, N, M] or None, W = (W_ci, W_cf, W_co) [N, M],
    g / b = five LayerNorm vectors [M] in the order j, i, f, o, c.  Returns every intermediate the kernels store."""
    j, i, f, o = Yg.unbind(2)
    if c is not None:
        i = i + W[0] * c
        f = f + W[1] * c
    jn = _ln(j)[0] * g[0] + b[0]
    inn = _ln(i)[0] * g[1] + b[1]
    fn = _ln(f)[0] * g[2] + b[2]
    cp = torch.sigmoid(inn) * torch.tanh(jn)
    if c is not None:
        cp = c * torch.sigmoid(fn + 1.0) + cp
    op = o + W[2] * cp
    cn = _ln(cp)[0] * g[4] + b[4]
    h = torch.sigmoid(_ln(op)[0] * g[3] + b[3]) * torch.tanh(cn)
    return {"i1": i, "f1": f, "cp": cp, "op": op, "cn": cn, "h": h}


# ----------------------------------------------------------------------------------------------------------------------------
# device buffers and launches
# ----------------------------------------------------------------------------------------------------------------------------
def _vecs(rows, g):
    return [(1.0 + 0.2 * torch.randn(rows, generator=g, dtype=torch.float64)).float() for _ in range(5)]


def make_case(shape, dt, seed, with_c=True):
    B, N, M, ld = shape
    g = R.gen(seed)
    Rr = B * N
    Y = torch.zeros(Rr, 4, ld, dtype=torch.float64)
    Y[..., :M] = torch.randn(Rr, 4, M, generator=g, dtype=torch.float64) + torch.tensor([0.3, -0.2, 0.5, 0.1], dtype=torch.float64)[:, None]
    c = torch.zeros(Rr, ld, dtype=torch.float64)
    c[:, :M] = torch.randn(Rr, M, generator=g, dtype=torch.float64)
    W = [(0.5 * torch.randn(N, M, generator=g, dtype=torch.float64)).float() for _ in range(3)]
    gam = _vecs(M, g)
    bet = [(0.2 * torch.randn(M, generator=g, dtype=torch.float64)).float() for _ in range(5)]
    dh = torch.zeros(Rr, ld, dtype=torch.float64)
    dh[:, :M] = torch.randn(Rr, M, generator=g, dtype=torch.float64)
    dcn = torch.zeros(Rr, ld, dtype=torch.float64)
    dcn[:, :M] = 0.5 * torch.randn(Rr, M, generator=g, dtype=torch.float64)
    T = R.TDT[dt]
    return {"shape": shape, "dt": dt, "Y": Y.reshape(Rr, 4 * ld).to(T), "c": c.to(T) if with_c else None, "W": W, "gamma": gam, "beta": bet,
            "dh": dh.to(T), "dcn": dcn.to(T), "g": g}


def _ln_struct(gd, bd):
    ln = _lib.ConvLstmLn()
    for k in range(5):
        ln.gamma[k], ln.beta[k] = gd[k].data_ptr(), bd[k].data_ptr()
    return ln


def _dln_struct(dg, db):
    d = _lib.ConvLstmDln()
    for k in range(5):
        d.dgamma[k], d.dbeta[k] = dg[k].data_ptr(), db[k].data_ptr()
    return d


def _dev(case):
    dev = {"W": [w.to(R.DEV) for w in case["W"]], "gamma": [R.guarded(1, v.numel(), torch.float32, v) for v in case["gamma"]],
           "beta": [R.guarded(1, v.numel(), torch.float32, v) for v in case["beta"]]}
    dev["ln"] = _ln_struct(dev["gamma"], dev["beta"])
    return dev


def run_fwd(case, dev, Yin=None, c_dev="case", W_ab=None):
    """A, B, C on fresh buffers.  Returns Yg after A, Yg after B, the stat block after A and after B, c_pre, c_new, h (guarded)."""
    B, N, M, ld = case["shape"]
    dt, Rr = case["dt"], B * N
    Y = R.guarded(Rr, 4 * ld, dt, case["Y"] if Yin is None else Yin)
    c = c_dev if not isinstance(c_dev, str) else (case["c"].to(R.DEV) if case["c"] is not None else None)
    Wi, Wf = W_ab if W_ab is not None else dev["W"][:2]
    sums = R.stat_block(5 * B)
    R.call("cmpc_convlstm_a", dt, Y, c, Wi, Wf, sums, B, N, ld, M)
    YA, sA = Y.clone(), sums.clone()
    cp = R.guarded(Rr, ld, dt)
    R.call("cmpc_convlstm_b", dt, Y, c, dev["W"][2], dev["ln"], sums, cp, B, N, ld, M)
    cn, h = R.guarded(Rr, ld, dt), R.guarded(Rr, ld, dt)
    R.call("cmpc_convlstm_c", dt, Y, cp, dev["ln"], sums, cn, h, B, N, ld, M)
    return {"YA": YA, "sA": sA, "Y": Y, "sums": sums, "cp": cp, "cn": cn, "h": h}


def _bnm(t, B, N, M, ld, blocks=1):
    """[B*N(+guard), blocks*ld] device / CPU map -> float64 [B, N, (blocks,) M] of its valid columns"""
    t = t[:B * N].double().cpu().reshape(B, N, blocks, ld)[..., :M]
    return t[:, :, 0] if blocks == 1 else t


def _check_pads(t, B, N, M, ld, blocks, what):
    R.assert_zero(t[:B * N].reshape(B * N, blocks, ld)[..., M:], what + " pad columns")


def _check_stats(sums, idx, vals, B, N, what):
    """the pairs of statistic idx*B + b summed over the 128 slots equal float64 sums of the stored values; the slots past the producing
    workgroups are 0 (the rows_grid caps: at most 100 workgroups per sample)"""
    s = sums.cpu().reshape(5, B, R.STAT_PARTS, 2)[idx]
    gx = max(1, min(100, (N + 3) // 4))
    assert bool((s[:, gx:] == 0).all()), f"{what}: unused stat slots not cleared"
    x = vals.reshape(B, -1)
    # each lane adds <= 16 float32 terms of a row before its float64 accumulator: 16 roundings of 6e-8 of sum |terms|
    R.assert_close(s[:, :gx, 0].sum(1), x.sum(1), K=N, what=what + " sum", atol=1e-6 * x.abs().sum(1))
    R.assert_close(s[:, :gx, 1].sum(1), (x * x).sum(1), K=N, what=what + " sum of squares", atol=1e-6 * (x * x).sum(1))


def _gb(case):
    return [v.double() for v in case["gamma"]], [v.double() for v in case["beta"]]


# ----------------------------------------------------------------------------------------------------------------------------
# forward
# ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", R.DTS, ids=R.DT_IDS)
@pytest.mark.parametrize("shape", SHAPES, ids=sid)
def test_convlstm_forward(dt, shape):
    B, N, M, ld = shape
    case = make_case(shape, dt, 21)
    dev = _dev(case)
    o = R.run_twice(lambda: run_fwd(case, dev))
    Rr = B * N
    for k, rows in (("YA", Rr), ("Y", Rr), ("cp", Rr), ("cn", Rr), ("h", Rr)):
        R.assert_guard(o[k], rows, "convlstm " + k)
    for k in ("gamma", "beta"):
        for v in dev[k]:
            R.assert_guard(v, 1, "LayerNorm vector")
    gam, bet = _gb(case)
    W = [w.double() for w in case["W"]]
    Y0 = _bnm(case["Y"], B, N, M, ld, 4)
    c = _bnm(case["c"], B, N, M, ld)
    # ---- A: i and f after the peepholes (in place), j and o untouched
    YA = _bnm(o["YA"], B, N, M, ld, 4)
    i1, f1 = Y0[:, :, 1] + W[0] * c, Y0[:, :, 2] + W[1] * c
    # i + w c in float32: one rounding of the larger term (cancellation: relative to |i| + |w c|)
    R.assert_close(YA[:, :, 1], i1, dt, what="A: i + W_ci c", atol=2e-7 * (Y0[:, :, 1].abs() + (W[0] * c).abs()))
    R.assert_close(YA[:, :, 2], f1, dt, what="A: f + W_cf c", atol=2e-7 * (Y0[:, :, 2].abs() + (W[1] * c).abs()))
    assert torch.equal(YA[:, :, 0], Y0[:, :, 0]) and torch.equal(YA[:, :, 3], Y0[:, :, 3]), "A: j or o changed"
    _check_pads(o["YA"], B, N, M, ld, 4, "A: Yg")
    for q in range(3):
        _check_stats(o["sA"], q, YA[:, :, q], B, N, f"A: stats of gate {'jif'[q]}")
    # ---- B: from the stored j, i, f (A's output) and o
    j, i, f, o0 = YA.unbind(2)
    jh, ih, fh = _ln(j)[0], _ln(i)[0], _ln(f)[0]
    jn, inn, fn = jh * gam[0] + bet[0], ih * gam[1] + bet[1], fh * gam[2] + bet[2]
    fg, ig, jt = torch.sigmoid(fn + 1), torch.sigmoid(inn), torch.tanh(jn)
    cp = c * fg + ig * jt
    # c_pre: sigmoid / tanh errors and the float32 LayerNorm inputs (each gate derivative <= 1), scaled by |c| for the forget gate
    mag_cp = c.abs() * (1 + _lnin_mag(f, gam[2], bet[2])) + 1 + _lnin_mag(i, gam[1], bet[1]) + 1 + _lnin_mag(j, gam[0], bet[0])
    cps = _bnm(o["cp"], B, N, M, ld)
    R.assert_close(cps, cp, dt, what="B: c_pre", atol=U_F32 * mag_cp)
    op = o0 + W[2] * cp
    Yb = _bnm(o["Y"], B, N, M, ld, 4)
    # o + W_co c_pre: c_pre enters unrounded (float32), so its error times |W_co|, plus the rounding of the sum
    R.assert_close(Yb[:, :, 3], op, dt, what="B: o + W_co c_pre", atol=2e-7 * (o0.abs() + (W[2] * cp).abs()) + W[2].abs() * U_F32 * mag_cp)
    assert torch.equal(Yb[:, :, :3], YA[:, :, :3]), "B: j, i or f changed"
    _check_pads(o["Y"], B, N, M, ld, 4, "B: Yg")
    _check_pads(o["cp"], B, N, M, ld, 1, "B: c_pre")
    _check_stats(o["sums"], 3, Yb[:, :, 3], B, N, "B: stats of o_pre")
    _check_stats(o["sums"], 4, cps, B, N, "B: stats of c_pre")
    # ---- C: from the stored o_pre and c_pre
    opn = _ln(Yb[:, :, 3])[0] * gam[3] + bet[3]
    cn = _ln(cps)[0] * gam[4] + bet[4]
    h = torch.sigmoid(opn) * torch.tanh(cn)
    mag_c, mag_o = _lnin_mag(cps, gam[4], bet[4]), _lnin_mag(Yb[:, :, 3], gam[3], bet[3])
    # LN(c): the float32 (x - mean) * rstd * gamma + beta
    R.assert_close(_bnm(o["cn"], B, N, M, ld), cn, dt, what="C: c_new", atol=U_F32 * mag_c)
    # h: sigmoid / tanh errors plus their inputs' (derivatives <= 1/4 and 1)
    R.assert_close(_bnm(o["h"], B, N, M, ld), h, dt, what="C: h", atol=U_F32 * (1 + mag_c + mag_o))
    _check_pads(o["cn"], B, N, M, ld, 1, "C: c_new")
    _check_pads(o["h"], B, N, M, ld, 1, "C: h")
    # ---- chained: the whole step against float64 from the raw inputs.  16-bit: A's i / f and B's c_pre / o_pre are stored, <= 1/2 ulp each
    # of values that LayerNorm maps with gain rstd * gamma (O(1) here): a few ulp of the normalised magnitude
    full = cell(Y0, c, W, gam, bet)
    u = 4 * R.ULP[dt] + U_F32
    R.assert_close(_bnm(o["cn"], B, N, M, ld), full["cn"], dt, what="chained c_new", atol=u * (1 + mag_c))
    R.assert_close(_bnm(o["h"], B, N, M, ld), full["h"], dt, what="chained h", atol=u * (1 + mag_c + mag_o))


def test_convlstm_first_step_ignores_peepholes_on_i_f():
    """c_prev == NULL (the first step): A only gathers statistics, W_ci / W_cf (NaN here) are never read, c_pre = sig(i) tanh(j)"""
    shape = (2, 49, 500, 512)
    B, N, M, ld = shape
    for dt in R.DTS:
        case = make_case(shape, dt, 22, with_c=False)
        dev = _dev(case)
        nan = torch.full((N, M), float("nan"), device=R.DEV)
        o = R.run_twice(lambda: run_fwd(case, dev, W_ab=(nan, nan)))
        Y0 = _bnm(case["Y"], B, N, M, ld, 4)
        assert torch.equal(_bnm(o["YA"], B, N, M, ld, 4), Y0), "A with c_prev NULL wrote Yg"
        gam, bet = _gb(case)
        ref = cell(Y0, None, [w.double() for w in case["W"]], gam, bet)
        j, i = Y0[:, :, 0], Y0[:, :, 1]
        mag = 2 + _lnin_mag(i, gam[1], bet[1]) + _lnin_mag(j, gam[0], bet[0])
        R.assert_close(_bnm(o["cp"], B, N, M, ld), ref["cp"], dt, what="c_pre (first step)", atol=U_F32 * mag)
        cps = _bnm(o["cp"], B, N, M, ld)
        op = Y0[:, :, 3] + case["W"][2].double() * cps
        W2 = case["W"][2].double()
        R.assert_close(_bnm(o["Y"], B, N, M, ld, 4)[:, :, 3], Y0[:, :, 3] + W2 * ref["cp"], dt, what="o_pre (first step)",
                       atol=2e-7 * (Y0[:, :, 3].abs() + (W2 * ref["cp"]).abs()) + W2.abs() * U_F32 * mag)
        assert not bool(torch.isnan(op).any())
        for k in ("cp", "cn", "h"):
            assert not bool(torch.isnan(o[k][:B * N]).any()), k


# ----------------------------------------------------------------------------------------------------------------------------
# backward
# ----------------------------------------------------------------------------------------------------------------------------
def st(x):
    """a leaf holding a stored value"""
    return x.clone().requires_grad_(True)


def bwd_reference(YF, c, cps, W, gam, bet, dh, dcn):
    """float64 autograd of the step, with every node the backward kernels READ at the value the forward STORED: Yg after B (j, i1, f1, o_pre),
    c_pre and c_prev.  A node x whose stored value is s and whose float64 expression is e is s + (e - e.detach()): value s, gradient of e.
    Returns the leaves (their .grad are the kernel's outputs) and the float64 intermediates the tolerance scales with."""
    j, i1, f1, op = [st(t) for t in YF.unbind(2)]
    c = st(c) if c is not None else None
    Wl = [st(w) for w in W]
    gl, bl = [st(v) for v in gam], [st(v) for v in bet]
    iv, fv = i1, f1
    if c is not None:                       # i1 = i + W_ci c: value stored, gradient to W_ci and c_prev
        iv = i1 + (Wl[0] * c - (Wl[0] * c).detach())
        fv = f1 + (Wl[1] * c - (Wl[1] * c).detach())
    jh, ih, fh = _ln(j)[0], _ln(iv)[0], _ln(fv)[0]
    jn, inn, fn = jh * gl[0] + bl[0], ih * gl[1] + bl[1], fh * gl[2] + bl[2]
    e = torch.sigmoid(inn) * torch.tanh(jn)
    if c is not None:
        e = c * torch.sigmoid(fn + 1.0) + e
    cp = cps + (e - e.detach())
    opv = op + (Wl[2] * cp - (Wl[2] * cp).detach())
    oh, ch = _ln(opv)[0], _ln(cp)[0]
    on, cn = oh * gl[3] + bl[3], ch * gl[4] + bl[4]
    h = torch.sigmoid(on) * torch.tanh(cn)
    on.retain_grad(); cn.retain_grad(); jn.retain_grad(); inn.retain_grad(); fn.retain_grad()
    loss = (h * dh).sum() + ((cn * dcn).sum() if dcn is not None else 0)
    loss.backward()
    return {"Y": (j, i1, f1, op), "c": c, "W": Wl, "g": gl, "b": bl, "on": on, "cn": cn, "jn": jn, "in": inn, "fn": fn,
            "xh": (jh.detach(), ih.detach(), fh.detach(), oh.detach(), ch.detach()),
            "r": [_ln(t.detach())[2] for t in (j, iv, fv, opv, cp)]}


def bwd_mags(ref, c, gam, W, dh, dcn, YF, cps, u):
    """error bounds of the backward outputs: u times the magnitudes each passes through.  u covers the float32 evaluation (U_F32) and, in
    16-bit, the kernels' stored intermediates (pass 1's dYg o-block and scratch, pass 2's j / i / f blocks and dc_prev: one ulp each) --
    the reference reads none of those, so a rounding that lands on the other side shows up as one ulp of the intermediate times its gain"""
    def ln_bwd(x_mag, xg, xh, r):     # rstd (x - mean(x) - xhat mean(x xhat)) on a magnitude
        B = xg.shape[0]
        m1 = xg.reshape(B, -1).mean(1).abs()[:, None, None]
        m2 = (xg * xh).reshape(B, -1).mean(1).abs()[:, None, None]
        return r * (x_mag + m1 + xh.abs() * m2)
    xh, r = ref["xh"], ref["r"]
    dcn_a = dcn.abs() if dcn is not None else 0
    Lq = [_lnin_mag(YF[:, :, k], gam[k], torch.zeros_like(gam[k])) + 1 for k in range(4)] + [_lnin_mag(cps, gam[4], torch.zeros_like(gam[4])) + 1]
    xo_mag = dh.abs() * gam[3].abs()                                         # don * gamma_o, |tanh|, sig' <= 1
    xc_mag = (dh.abs() + dcn_a) * gam[4].abs()
    dop = ln_bwd(xo_mag, ref["on"].grad * gam[3], xh[3], r[3])
    dc = ln_bwd(xc_mag, ref["cn"].grad * gam[4], xh[4], r[4]) + W[2].abs() * dop
    cab = c.abs() if c is not None else torch.zeros_like(dc)
    dq = [dc * Lq[0], dc * Lq[1], dc * cab * Lq[2]]                           # dc times a gate derivative (<= 1) and its input's error
    grads = [torch.zeros_like(dc) if ref[k].grad is None else ref[k].grad for k in ("jn", "in", "fn")]     # no forget gate without c_prev
    dY = [ln_bwd(gam[q].abs() * dq[q], grads[q] * gam[q], xh[q], r[q]) for q in range(3)]
    out = {"dY": [u * m for m in dY] + [u * dop],
           "dc_prev": u * (dc * (1 + cab * Lq[2]) + W[0].abs() * dY[1] + W[1].abs() * dY[2]),
           "dW": [u * (dY[1] * cab).sum(0), u * (dY[2] * cab).sum(0), u * (dop * cps.abs()).sum(0)],
           "dg": [u * (dq[q] * Lq[q] * xh[q].abs()).sum((0, 1)) for q in range(3)] +
                 [u * (dh.abs() * Lq[3] * xh[3].abs()).sum((0, 1)), u * ((dh.abs() + dcn_a) * Lq[4] * xh[4].abs()).sum((0, 1))],
           "db": [u * dq[q].sum((0, 1)) for q in range(3)] + [u * dh.abs().sum((0, 1)), u * (dh.abs() + dcn_a).sum((0, 1))]}
    return out


def run_bwd(case, dev, fw, with_dcn=True, c_dev="case", W_ab=None, pre=None):
    B, N, M, ld = case["shape"]
    dt, Rr = case["dt"], B * N
    c = c_dev if not isinstance(c_dev, str) else (case["c"].to(R.DEV) if case["c"] is not None else None)
    Wi, Wf = W_ab if W_ab is not None else dev["W"][:2]
    dY = R.guarded(Rr, 4 * ld, dt)
    dcp = R.guarded(Rr, ld, dt)
    dW = [R.guarded(N, M, torch.float32, p) for p in pre["dW"]]
    dg = [R.guarded(1, M, torch.float32, p) for p in pre["dg"]]
    db = [R.guarded(1, M, torch.float32, p) for p in pre["db"]]
    scr = torch.zeros(Rr, ld, dtype=R.TDT[dt], device=R.DEV)
    bs = R.stat_block(5 * B)
    R.call("cmpc_convlstm_bwd", dt, case["dh"].to(R.DEV), case["dcn"].to(R.DEV) if with_dcn else None, fw["Y"], c, fw["cp"], Wi, Wf,
           dev["W"][2], dev["ln"], fw["sums"], dY, dcp if c is not None else None, dW[0], dW[1], dW[2], _dln_struct(dg, db), scr, bs,
           B, N, ld, M)
    return {"dY": dY, "dcp": dcp, "dW0": dW[0], "dW1": dW[1], "dW2": dW[2], **{f"dg{k}": dg[k] for k in range(5)},
            **{f"db{k}": db[k] for k in range(5)}}


def _prefill(N, M, g):
    return {"dW": [torch.randn(N, M, generator=g).float() for _ in range(3)], "dg": [torch.randn(M, generator=g).float() for _ in range(5)],
            "db": [torch.randn(M, generator=g).float() for _ in range(5)]}


def _check_bwd(case, o, fw, with_dcn, pre, first=False):
    B, N, M, ld = case["shape"]
    dt = case["dt"]
    gam, bet = _gb(case)
    W = [w.double() for w in case["W"]]
    YF = _bnm(fw["Y"], B, N, M, ld, 4)
    cps = _bnm(fw["cp"], B, N, M, ld)
    c = None if first else _bnm(case["c"], B, N, M, ld)
    dh = _bnm(case["dh"], B, N, M, ld)
    dcn = _bnm(case["dcn"], B, N, M, ld) if with_dcn else None
    ref = bwd_reference(YF, c, cps, W, gam, bet, dh, dcn)
    u = R.ULP[dt] + U_F32
    mg = bwd_mags(ref, c, gam, W, dh, dcn, YF, cps, u)
    tag = f"bwd(dc_new={'yes' if with_dcn else 'NULL'}, c_prev={'NULL' if first else 'yes'})"
    Rr = B * N
    R.assert_guard(o["dY"], Rr, tag + " dYg")
    dY = _bnm(o["dY"], B, N, M, ld, 4)
    for q in range(4):
        rg = ref["Y"][q].grad
        rg = torch.zeros_like(dY[:, :, q]) if rg is None else rg          # no forget gate without c_prev: its block is 0
        R.assert_close(dY[:, :, q], rg, dt, what=f"{tag} dYg[{'jifo'[q]}]", atol=mg["dY"][q])
    _check_pads(o["dY"], B, N, M, ld, 4, tag + " dYg")
    if first:
        R.assert_sentinel(o["dcp"], tag + " dc_prev")
        for k in (0, 1):
            R.assert_sentinel(o[f"dW{k}"][:N], tag + f" dW_c{'if'[k]}")
    else:
        R.assert_guard(o["dcp"], Rr, tag + " dc_prev")
        R.assert_close(_bnm(o["dcp"], B, N, M, ld), ref["c"].grad, dt, what=tag + " dc_prev", atol=mg["dc_prev"])
        _check_pads(o["dcp"], B, N, M, ld, 1, tag + " dc_prev")
    # peephole and LayerNorm gradients accumulate onto the pre-filled values; sums over B (peepholes) or B N rows (LayerNorm)
    for k in range(0 if not first else 2, 3):
        R.assert_guard(o[f"dW{k}"], N, tag + f" dW_c{'ifo'[k]}")
        R.assert_close(o[f"dW{k}"][:N], pre["dW"][k].double() + ref["W"][k].grad, K=B, what=tag + f" dW_c{'ifo'[k]}",
                       atol=mg["dW"][k] + R.sum_atol(ref["W"][k].grad[None], 0))
    for k in range(5):
        for nm, ld_, p, rg, mk in (("dgamma", "dg", pre["dg"][k], ref["g"][k].grad, mg["dg"][k]), ("dbeta", "db", pre["db"][k], ref["b"][k].grad, mg["db"][k])):
            rg = torch.zeros(M, dtype=torch.float64) if rg is None else rg      # LN(f) without c_prev: no gradient, the sums stay as they were
            R.assert_guard(o[f"{ld_}{k}"], 1, f"{tag} {nm}[{k}]")
            R.assert_close(o[f"{ld_}{k}"][0], p.double() + rg, K=Rr, what=f"{tag} {nm}[{'jifoc'[k]}]", atol=mk + 1e-7 * p.double().abs())


@pytest.mark.parametrize("dt", R.DTS, ids=R.DT_IDS)
@pytest.mark.parametrize("shape", SHAPES, ids=sid)
def test_convlstm_backward(dt, shape):
    B, N, M, ld = shape
    case = make_case(shape, dt, 23)
    dev = _dev(case)
    fw = run_fwd(case, dev)
    pre = _prefill(N, M, case["g"])
    o = R.run_twice(lambda: run_bwd(case, dev, fw, pre=pre))
    _check_bwd(case, o, fw, True, pre)


@pytest.mark.parametrize("dt", R.DTS, ids=R.DT_IDS)
def test_convlstm_backward_variants(dt):
    """dc_new == NULL (the last step of the chain); c_prev == NULL (the first): W_ci / W_cf NaN and never read, dW_ci / dW_cf / dc_prev
    stay sentinel"""
    shape = (2, 49, 500, 512)
    B, N, M, ld = shape
    case = make_case(shape, dt, 24)
    dev = _dev(case)
    fw = run_fwd(case, dev)
    pre = _prefill(N, M, case["g"])
    o = R.run_twice(lambda: run_bwd(case, dev, fw, with_dcn=False, pre=pre))
    _check_bwd(case, o, fw, False, pre)
    case1 = make_case(shape, dt, 25, with_c=False)
    dev1 = _dev(case1)
    nan = torch.full((N, M), float("nan"), device=R.DEV)
    fw1 = run_fwd(case1, dev1, W_ab=(nan, nan))
    pre1 = _prefill(N, M, case1["g"])
    pre1["dW"][0] = R.sentinel_fill(torch.empty(N, M))
    pre1["dW"][1] = R.sentinel_fill(torch.empty(N, M))
    o1 = R.run_twice(lambda: run_bwd(case1, dev1, fw1, c_dev=None, W_ab=(nan, nan), pre=pre1))
    _check_bwd(case1, o1, fw1, True, pre1, first=True)


# ----------------------------------------------------------------------------------------------------------------------------
# three steps, as engine.hip clstm_fwd / clstm_bwd chain them
# ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", R.DTS, ids=R.DT_IDS)
@pytest.mark.parametrize("shape", [(2, 49, 24, 64), (2, 400, 500, 512)], ids=sid)
def test_convlstm_three_steps(dt, shape):
    """Yg_s = X_s + h_{s-1} Wh (the recurrent product in torch), c_prev = c_new of the step before (NULL at s = 0); backward from dh of the
    last h with dc_new NULL, dh_{s-1} = dYg_s Wh^T, dc_new_{s-1} = dc_prev of step s; peephole and LayerNorm gradients accumulate over the
    three launches.  Against a float64 unroll of cell() with autograd."""
    B, N, M, ld = shape
    g = R.gen(26)
    Rr, T = B * N, R.TDT[dt]
    case = make_case(shape, dt, 27)
    dev = _dev(case)
    X = [torch.randn(B, N, 4, M, generator=g, dtype=torch.float64) for _ in range(3)]
    Wh = (torch.randn(M, 4, M, generator=g, dtype=torch.float64) / math.sqrt(M))
    dhT = torch.randn(B, N, M, generator=g, dtype=torch.float64)

    def padded(x, blocks):          # [B, N, (blocks,) M] -> [R, blocks * ld] storage dtype on the device
        out = torch.zeros(Rr, blocks, ld, dtype=torch.float64)
        out[..., :M] = x.reshape(Rr, blocks, M)
        return out.reshape(Rr, blocks * ld).to(T).to(R.DEV)
    Whd = Wh.reshape(M, 4 * M).float().to(R.DEV)
    gam, bet = _gb(case)
    W = [w.double() for w in case["W"]]
    pre = _prefill(N, M, g)
    dW = [R.guarded(N, M, torch.float32, p) for p in pre["dW"]]
    dg = [R.guarded(1, M, torch.float32, p) for p in pre["dg"]]
    db = [R.guarded(1, M, torch.float32, p) for p in pre["db"]]
    dln = _dln_struct(dg, db)
    steps, h, c = [], None, None
    for s in range(3):
        Y = X[s].reshape(Rr, 4, M).clone()
        if h is not None:
            Y = Y + (h[:Rr].float().reshape(Rr, ld)[:, :M] @ Whd).double().cpu().reshape(Rr, 4, M)
        Yd = padded(Y, 4)
        fw = run_fwd({**case, "Y": None}, dev, Yin=Yd, c_dev=c)
        steps.append((fw, c))
        h, c = fw["h"][:Rr], fw["cn"][:Rr]
    dh, dc = padded(dhT, 1), None
    for s in (2, 1, 0):
        fw, cprev = steps[s]
        dY = torch.zeros(Rr, 4 * ld, dtype=T, device=R.DEV)
        dcp = torch.zeros(Rr, ld, dtype=T, device=R.DEV) if cprev is not None else None
        scr = torch.zeros(Rr, ld, dtype=T, device=R.DEV)
        R.call("cmpc_convlstm_bwd", dt, dh, dc, fw["Y"], cprev, fw["cp"], dev["W"][0], dev["W"][1], dev["W"][2], dev["ln"], fw["sums"], dY, dcp,
               dW[0], dW[1], dW[2], dln, scr, R.stat_block(5 * B), B, N, ld, M)
        dYv = dY.float().reshape(Rr, 4, ld)[..., :M].reshape(Rr, 4 * M)
        dh = padded((dYv @ Whd.t()).double().cpu(), 1)
        dc = dcp
    torch.cuda.synchronize()
    # float64 unroll
    Wl = [w.clone().requires_grad_(True) for w in W]
    gl, bl = [v.clone().requires_grad_(True) for v in gam], [v.clone().requires_grad_(True) for v in bet]
    hr, cr, outs = None, None, []
    for s in range(3):
        Y = X[s] + (0 if hr is None else torch.einsum("bnk,kgm->bngm", hr, Wh))
        o = cell(Y, cr, Wl, gl, bl)
        hr, cr = o["h"], o["cn"]
        outs.append(o)
    (hr * dhT).sum().backward()
    # chained: three steps, each stores h, c_new, Yg, c_pre and (backward) dYg, dh, dc_prev, plus the float32 products between the steps.
    # Each intermediate is O(1) and passes to the next step with gain O(1): a few ulp (and 2e-5 for float32) of the largest magnitude
    u = 4 * R.ULP[dt] + 2e-5
    R.assert_close(h.double().cpu().reshape(B, N, ld)[..., :M], hr, dt, what="3 steps: h", atol=u * float(hr.detach().abs().max()))
    R.assert_close(c.double().cpu().reshape(B, N, ld)[..., :M], cr, dt, what="3 steps: c_new", atol=u * float(cr.detach().abs().max()))
    for k in range(3):
        ref = pre["dW"][k].double() + Wl[k].grad
        R.assert_close(dW[k][:N], ref, what=f"3 steps: dW_c{'ifo'[k]}", atol=u * float(Wl[k].grad.abs().max()))
    for k in range(5):
        R.assert_close(dg[k][0], pre["dg"][k].double() + gl[k].grad, what=f"3 steps: dgamma[{'jifoc'[k]}]", atol=u * float(gl[k].grad.abs().max()))
        R.assert_close(db[k][0], pre["db"][k].double() + bl[k].grad, what=f"3 steps: dbeta[{'jifoc'[k]}]", atol=u * float(bl[k].grad.abs().max()))
