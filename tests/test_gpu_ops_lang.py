"""Op-level tests of the language-side kernels of csrc/ops_lang.hip against float64 references: embed_gather / embed_scatter,
lstm_cell_fwd / lstm_cell_bwd (tf LSTMCell, forget bias 1, dynamic_rnn length masking), the backward recurrence through lstm_bwd_step,
parse_softmax_fwd/bwd (4 and 5 classes) and lang_pool_fwd/bwd (valid, nec and the video model's action configuration).  The language
tensors are float32 end to end."""
import pytest
import torch

from tests import opref as R
from tests.util import O

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("n_words,G,ld_out,vocab", [(1, 12, 16, 50), (264, 300, 304, 1000), (8 * 33, 1000, 1024, 7)])
def test_embed_gather_scatter(n_words, G, ld_out, vocab):
    """out[r, :G] = table[words[r]] (ids clamped to [0, vocab)), out[r, G:ld_out] = 0; dtable[w] += sum of dout over w's
    occurrences (cmpc.h:228-229) -- with repeated ids, id 0 and out-of-range ids"""
    g = R.gen(21)
    table = torch.randn(vocab, G, generator=g).float()
    words = torch.randint(0, vocab, (n_words,), generator=g, dtype=torch.int32)
    words[::3] = 0
    if n_words > 4:
        words[1], words[2], words[4] = vocab + 5, -3, words[3]
    cw = words.long().clamp(0, vocab - 1)
    td, wd = table.to(R.DEV), words.to(R.DEV)

    def run():
        out = R.guarded(n_words, ld_out, torch.float32)
        R.call("cmpc_embed_gather", td, wd, out, n_words, G, ld_out, vocab)
        return {"out": out}
    out = R.run_twice(run)["out"]
    R.assert_guard(out, n_words, "embed_gather")
    assert torch.equal(out[:n_words, :G].cpu(), table[cw]), "embed_gather"
    R.assert_zero(out[:n_words, G:], "embed_gather pad")

    dout = torch.randn(n_words, ld_out, generator=g).float()
    dt0 = torch.randn(vocab, G, generator=g).float()
    dd = dout.to(R.DEV)
    ref = dt0.double().index_add(0, cw, dout.double()[:, :G])
    cnt = torch.bincount(cw, minlength=vocab).clamp(min=1)

    def run():
        dtab = R.guarded(vocab, G, torch.float32, dt0)
        R.call("cmpc_embed_scatter", dd, ld_out, wd, dtab, n_words, G, vocab)
        return {"dtab": dtab}
    dtab = R.run_twice(run)["dtab"]
    R.assert_guard(dtab, vocab, "embed_scatter")
    terms = dt0.double().abs().index_add(0, cw, dout.double().abs()[:, :G])
    # per-row sums of signed terms: rounding bounded by the sum of |terms|
    R.assert_close(dtab[:vocab], ref, K=int(cnt.max()) + 1, what="embed_scatter", atol=1e-7 * terms)


def _cell_ref(gates, c_prev, h_prev, R_):
    i, j, f, o = gates.split(gates.shape[1] // 4, 1)
    i, j, f, o = i[:, :R_], j[:, :R_], f[:, :R_], o[:, :R_]
    a = (torch.sigmoid(i), torch.tanh(j), torch.sigmoid(f + 1.0), torch.sigmoid(o))       # tf LSTMCell, forget_bias 1 (cmpc.h:230)
    c = a[2] * c_prev[:, :R_] + a[0] * a[1]
    h = a[3] * torch.tanh(c)
    return a, c, h


@pytest.mark.parametrize("B", [1, 3, 8])
@pytest.mark.parametrize("ld,R_", [(64, 40), (1024, 1000), (1024, 1024), (72, 72)])
def test_lstm_cell(B, ld, R_):
    """lstm_cell_fwd / lstm_cell_bwd (cmpc.h:230-236) at a step t where some samples are finished (t >= seq_len: state passes
    through, output 0, gate gradients 0) and units R..ld are padding"""
    g = R.gen(22)
    t = 4
    seq_len = torch.tensor([5, 4, 9, 1, 20, 4, 6, 2][:B], dtype=torch.int32)
    live = (t < seq_len).double()[:, None]
    gates = (torch.randn(B, 4 * ld, generator=g, dtype=torch.float64) * 2).float()
    c_prev = torch.randn(B, ld, generator=g).float()
    h_prev = torch.randn(B, ld, generator=g).float()
    ld_out = ld + 8
    sl, cpd, hpd = seq_len.to(R.DEV), c_prev.to(R.DEV), h_prev.to(R.DEV)

    def run():
        gt = R.guarded(B, 4 * ld, torch.float32, gates)
        c_out, h_out = R.guarded(B, ld, torch.float32), R.guarded(B, ld, torch.float32)
        out_t = R.guarded(B, ld_out, torch.float32)
        R.call("cmpc_lstm_cell_fwd", gt, cpd, hpd, sl, t, c_out, h_out, out_t, ld_out, B, ld, R_)
        return {"gt": gt, "c": c_out, "h": h_out, "out": out_t}
    o = R.run_twice(run)
    for k, n in (("gt", B), ("c", B), ("h", B), ("out", B)):
        R.assert_guard(o[k], n, "lstm_cell_fwd " + k)
    G64 = gates.double()
    a, c, h = _cell_ref(G64, c_prev.double(), h_prev.double(), R_)
    ga = o["gt"][:B].cpu().reshape(B, 4, ld)
    for q in range(4):
        R.assert_close(ga[:, q, :R_], a[q], what=f"lstm_cell_fwd gate {q}")
        R.assert_zero(ga[:, q, R_:], "lstm_cell_fwd gate pad")
    cref = live * c + (1 - live) * c_prev.double()[:, :R_]
    href = live * h + (1 - live) * h_prev.double()[:, :R_]
    R.assert_close(o["c"][:B, :R_], cref, what="lstm_cell_fwd c")
    R.assert_close(o["h"][:B, :R_], href, what="lstm_cell_fwd h")
    R.assert_close(o["out"][:B, :R_], live * h, what="lstm_cell_fwd out_t")
    R.assert_zero(o["out"][:B, R_:ld], "lstm_cell_fwd out_t pad")
    R.assert_sentinel(o["out"][:B, ld:], "lstm_cell_fwd out_t beyond ld")
    dead = (live[:, 0] == 0)
    R.assert_zero(o["out"][:B, :ld][dead.to(R.DEV)], "lstm_cell_fwd out_t of finished samples")

    # backward: gradients w.r.t. the activated gates from autograd of the cell on the stored activations and c_out, then through each
    # activation's derivative expressed by its output (the kernel's inputs are the activated gates)
    ga_s, c_s = o["gt"][:B].contiguous(), o["c"][:B].contiguous()
    dout = torch.randn(B, ld_out, generator=g).float()
    dh0 = torch.randn(B, ld, generator=g).float()
    dc0 = torch.randn(B, ld, generator=g).float()
    A = [ga.double()[:, q, :R_].clone().requires_grad_(True) for q in range(4)]
    cp = c_prev.double()[:, :R_].clone().requires_grad_(True)
    cn = A[2] * cp + A[0] * A[1]
    hn = A[3] * torch.tanh(c_s.double().cpu()[:, :R_] + (cn - cn.detach()))
    dhn = dout.double()[:, :R_] + dh0.double()[:, :R_]
    (hn * dhn + cn * dc0.double()[:, :R_]).sum().backward()
    dga = [A[0].grad * A[0] * (1 - A[0]), A[1].grad * (1 - A[1] ** 2), A[2].grad * A[2] * (1 - A[2]), A[3].grad * A[3] * (1 - A[3])]
    doutd = dout.to(R.DEV)

    def run():
        dh, dc = R.guarded(B, ld, torch.float32, dh0), R.guarded(B, ld, torch.float32, dc0)
        dg = R.guarded(B, 4 * ld, torch.float32)
        R.call("cmpc_lstm_cell_bwd", ga_s, cpd, c_s, sl, t, doutd, ld_out, dh, dc, dg, B, ld, R_)
        return {"dh": dh, "dc": dc, "dg": dg}
    o = R.run_twice(run)
    for k in o:
        R.assert_guard(o[k], B, "lstm_cell_bwd " + k)
    dg = o["dg"][:B].cpu().reshape(B, 4, ld)
    for q in range(4):
        R.assert_close(dg[:, q, :R_], live * dga[q].detach(), what=f"lstm_cell_bwd dgate {q}")
        R.assert_zero(dg[:, q, R_:], "lstm_cell_bwd dgate pad")
    R.assert_close(o["dc"][:B, :R_], live * cp.grad + (1 - live) * dc0.double()[:, :R_], what="lstm_cell_bwd dc")
    R.assert_close(o["dh"][:B, :R_], (1 - live) * dh0.double()[:, :R_], what="lstm_cell_bwd dh")
    R.assert_zero(o["dh"][:B, R_:], "lstm_cell_bwd dh pad"); R.assert_zero(o["dc"][:B, R_:], "lstm_cell_bwd dc pad")


@pytest.mark.parametrize("ncls", [4, 5])
@pytest.mark.parametrize("n,ld", [(1, 8), (264, 20), (8 * 64, 24)])
def test_parse_softmax(ncls, n, ld):
    """parse = softmax over ncls classes times seq_mask; backward dlogits (pad columns ncls..ld written 0) (cmpc.h:251-254)"""
    g = R.gen(23)
    logits = (torch.randn(n, ld, generator=g, dtype=torch.float64) * 3).float()
    mask = (torch.rand(n, generator=g) > 0.3).float()
    ld_, md = logits.to(R.DEV), mask.to(R.DEV)
    la = logits.double()[:, :ncls].clone().requires_grad_(True)
    p = torch.softmax(la, 1) * mask.double()[:, None]

    def run():
        parse = R.guarded(n, ncls, torch.float32)
        R.call("cmpc_parse_softmax_fwd", ld_, ld, md, parse, n, ncls)
        return {"p": parse}
    ps = R.run_twice(run)["p"]
    R.assert_guard(ps, n, "parse_softmax_fwd")
    R.assert_close(ps[:n], p.detach(), K=ncls, what="parse_softmax_fwd")
    dparse = torch.randn(n, ncls, generator=g).float()
    p.backward(dparse.double())
    ps_s, dpd = ps[:n].contiguous(), dparse.to(R.DEV)

    def run():
        dl = R.guarded(n, ld, torch.float32)
        R.call("cmpc_parse_softmax_bwd", dpd, ps_s, md, dl, ld, n, ncls)
        return {"dl": dl}
    dl = R.run_twice(run)["dl"]
    R.assert_guard(dl, n, "parse_softmax_bwd")
    R.assert_close(dl[:n, :ncls], la.grad, K=ncls, what="parse_softmax_bwd", atol=R.sum_atol(p.detach() * dparse.double(), 1)[:, None])
    R.assert_zero(dl[:n, ncls:], "parse_softmax_bwd pad")


@pytest.mark.parametrize("cfg", [(2, 0, 4), (3, 0, 4), (1, 3, 5), (5, 0, 5)], ids=["valid", "nec", "action", "all5"])
@pytest.mark.parametrize("B,T,ld,R_", [(1, 1, 64, 40), (3, 33, 1024, 1000), (8, 64, 2048, 2047), (2, 20, 1032, 1025)])
def test_lang_pool(cfg, B, T, ld, R_):
    """v[b] = l2norm(sum_t (sum_{cls_lo <= k < cls_lo + ncls} parse[b,t,k]) wf[b,t,:]) and its backward (cmpc.h:255-259): dparse and
    dwf accumulate; v's pad columns are written 0, dwf's pad columns stay untouched"""
    ncls, lo, ps = cfg
    g = R.gen(24)
    parse = torch.softmax(torch.randn(B, T, ps, generator=g, dtype=torch.float64), 2).float()
    wf = torch.randn(B, T, ld, generator=g).float()
    wf[..., R_:] = 0
    pd, wd = parse.to(R.DEV), wf.to(R.DEV)
    pa = parse.double().clone().requires_grad_(True)
    wa = wf.double().clone().requires_grad_(True)
    wsum = pa[..., lo:lo + ncls].sum(2)
    pooled = (wsum[..., None] * wa[..., :R_]).sum(1)
    v = O.l2_normalize(pooled, 1)

    def run():
        vv, rs = R.guarded(B, ld, torch.float32), R.guarded(B, 1, torch.float32)
        R.call("cmpc_lang_pool_fwd", pd, wd, vv, rs, B, T, ld, R_, ncls, lo, ps)
        return {"v": vv, "rs": rs}
    o = R.run_twice(run)
    R.assert_guard(o["v"], B, "lang_pool_fwd"); R.assert_guard(o["rs"], B, "lang_pool_fwd rstd")
    R.assert_close(o["v"][:B, :R_], v.detach(), K=T * R_, what="lang_pool_fwd v")
    R.assert_zero(o["v"][:B, R_:], "lang_pool_fwd pad")
    ss = (pooled.detach() ** 2).sum(1)
    R.assert_close(o["rs"][:B, 0], torch.rsqrt(ss.clamp(min=1e-12)), K=T * R_, what="lang_pool_fwd rstd")

    dv = torch.randn(B, ld, generator=g).float()
    v.backward(dv.double()[:, :R_])
    dp0 = torch.randn(B, T, ps, generator=g).float()
    dw0 = torch.randn(B, T, ld, generator=g).float()
    v_s, rs_s, dvd = o["v"][:B].contiguous(), o["rs"][:B].contiguous(), dv.to(R.DEV)

    def run():
        dp = R.guarded(B * T, ps, torch.float32, dp0)
        dw = R.guarded(B * T, ld, torch.float32, dw0)
        R.call("cmpc_lang_pool_bwd", dvd, v_s, rs_s, pd, wd, dp, dw, B, T, ld, R_, ncls, lo, ps)
        return {"dp": dp, "dw": dw}
    o = R.run_twice(run)
    R.assert_guard(o["dp"], B * T, "lang_pool_bwd dparse"); R.assert_guard(o["dw"], B * T, "lang_pool_bwd dwf")
    dpr = dp0.double() + pa.grad
    dpr[..., :lo] = dp0.double()[..., :lo]            # classes outside [cls_lo, cls_lo + ncls) receive nothing
    dpr[..., lo + ncls:] = dp0.double()[..., lo + ncls:]
    # dparse is a dot product over R columns of signed terms: rounding bounded by the sum of |terms|
    tabs = (wf.double().abs()[..., :R_] * (dv.double().abs()[:, None, :R_] + 1)).sum(2) * float(rs_s.abs().max())
    R.assert_close(o["dp"][:B * T].reshape(B, T, ps), dpr, K=R_, what="lang_pool_bwd dparse", atol=1e-7 * tabs[..., None])
    dwr = dw0.double().clone()
    dwr[..., :R_] += wa.grad[..., :R_]
    R.assert_close(o["dw"][:B * T].reshape(B, T, ld), dwr, K=R_, what="lang_pool_bwd dwf")


def _lstm_ref(xg, Wh, h0, seq_len, T, ld, R_):
    """dynamic_rnn of tf LSTMCell (forget bias 1) from h0 and a zero cell state: gates [T, B, 4 ld] (activated), h / c [T + 1, B, ld],
    outs [B, T, ld]; units >= R are padding (gates, state and outputs 0)"""
    B = h0.shape[0]
    h, c = h0.clone(), torch.zeros_like(h0)
    gates, hs, cs, outs = [], [h], [c], []
    for t in range(T):
        pre = xg[t] + h @ Wh.t()                               # Wh [4 ld][ld]: gate rows, k contiguous
        pre = pre.reshape(B, 4, ld)
        a = torch.stack([torch.sigmoid(pre[:, 0]), torch.tanh(pre[:, 1]), torch.sigmoid(pre[:, 2] + 1.0), torch.sigmoid(pre[:, 3])], 1)
        a = a * (torch.arange(ld) < R_).double()
        cn = a[:, 2] * c + a[:, 0] * a[:, 1]
        hn = a[:, 3] * torch.tanh(cn)
        live = (t < seq_len).double()[:, None]
        c = live * cn + (1 - live) * c
        h = live * hn + (1 - live) * h
        gates.append(a.reshape(B, 4 * ld)); hs.append(h); cs.append(c); outs.append(live * hn)
    return torch.stack(gates), torch.stack(hs), torch.stack(cs), torch.stack(outs, 1)


@pytest.mark.parametrize("B", [1, 3, 8])
@pytest.mark.parametrize("ld,R_", [(64, 40), (1024, 1000)])
def test_lstm_bwd_chain(B, ld, R_):
    """The per-step backward of one direction -- cmpc_lstm_cell_bwd at T-1, then cmpc_lstm_bwd_step for t-1 = T-2 .. 0 -- against
    autograd of the float64 recurrence.  Its forward inputs (activated gates, cell states) are the reference's, rounded to float32."""
    g = R.gen(25)
    T = 20
    seq_len = torch.tensor([20, 1, 7, 20, 13, 2, 19, 5][:B], dtype=torch.int32)
    units = (torch.arange(ld) < R_).double()
    xg = torch.randn(T, B, 4 * ld, generator=g, dtype=torch.float64).float()
    Wh = (torch.randn(4 * ld, ld, generator=g, dtype=torch.float64) / R_ ** 0.5 * units).float()      # columns >= R meet h = 0
    h0 = (torch.randn(B, ld, generator=g, dtype=torch.float64) * 0.5 * units).float()
    xa = xg.double().clone().requires_grad_(True)
    gates, _, cs, outs = _lstm_ref(xa, Wh.double(), h0.double(), seq_len, T, ld, R_)
    K = T * ld          # each step's state carries every earlier step's rounding

    # dgates (pre-activation gradients) from douts, against autograd of the float64 recurrence
    douts = (torch.randn(B, T, ld, generator=g, dtype=torch.float64) * units).float()
    outs.backward(douts.double())
    Wnd = Wh.t().contiguous().to(R.DEV)                        # [ld rows][4 ld]: rows of W_h^T
    sl = seq_len.to(R.DEV)
    ga_s = gates.detach().float().reshape(T * B, 4 * ld).to(R.DEV)
    c_s = cs.detach().float().reshape((T + 1) * B, ld).to(R.DEV)
    dh = torch.zeros(B, ld, device=R.DEV); dc = torch.zeros(B, ld, device=R.DEV)
    dgs = R.guarded(T * B, 4 * ld, torch.float32)
    st = lambda t: dgs[t * B:(t + 1) * B]
    dout_tb = douts.transpose(0, 1).contiguous().to(R.DEV)    # [T, B, ld]
    R.call("cmpc_lstm_cell_bwd", ga_s[(T - 1) * B:], c_s[(T - 1) * B:], c_s[T * B:], sl, T - 1, dout_tb[T - 1], ld, dh, dc, st(T - 1), B, ld, R_)
    for t in range(T - 1, 0, -1):
        R.call("cmpc_lstm_bwd_step", st(t), Wnd, 4 * ld, ga_s[(t - 1) * B:], c_s[(t - 1) * B:], c_s[t * B:], sl, t - 1, dout_tb[t - 1], ld,
               dh, dc, st(t - 1), B, ld, R_)
    torch.cuda.synchronize()
    R.assert_guard(dgs, T * B, "lstm_bwd_step")
    R.assert_close(dgs[:T * B].reshape(T, B, 4 * ld), xa.grad, K=4 * K, what="lstm_bwd_step chain dgates")
