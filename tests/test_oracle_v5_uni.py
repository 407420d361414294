"""CPU tests of the CMPCv5_model / CMPCv5_HSV_model oracle (tests/v5uni_oracle.py) against the pieces it is built from and against
known answers of the reference source: its encoder is CMPC_model's lstm(), the HSV graph with its three extra grid rows zeroed is the
plain graph, the manifest follows the reference's _conv calls, and autograd through the whole graph passes an fp64 gradcheck."""
import numpy as np
import pytest
import torch

from oracle import cmpc_torch as O
from oracle import cmpc_v5_torch as V
from tests import v5uni_oracle as U5


def _case(hsv, train=True, dtype=torch.float64, seed=0):
    cfg = U5.tiny_cfg(B=2, T=5, hsv=hsv, train_mode=train)
    hp = {k: v.to(dtype) for k, v in U5.init_head_params(cfg).items()}
    bn = {k: v.to(dtype) for k, v in U5.init_bn_state(cfg).items()}
    g = torch.Generator().manual_seed(5)
    for k in hp:
        if k.endswith(("biases", "beta")):
            hp[k] = (torch.randn(hp[k].shape, generator=g, dtype=torch.float64) * 0.05).to(dtype)
    bp = U5.init_backbone_params(cfg)
    words, im, sl, tgt = O.synth_batch(cfg, seed=seed)
    feats = [f.to(dtype) for f in U5.backbone_taps(bp, im, cfg)]
    return cfg, hp, bn, feats, words, im.to(dtype), sl, tgt.to(dtype)


def test_encoder_is_cmpc_model_lstm():
    """CMPCv5_model.py:158-178 is CMPC_model.py:144-164 (state_is_tuple aside): same words_feat and seq_mask on the same weights."""
    cfg, hp, _, _, words, _, sl, _ = _case(False)
    wf, mask = U5.lstm(hp, words, sl, cfg)
    wf_o, mask_o = O.text_lstm(hp, words, sl, cfg)
    assert torch.equal(wf, wf_o) and torch.equal(mask, mask_o)
    assert wf.shape == (cfg.batch_size, 1, cfg.num_steps, cfg.rnn_size)
    for b in range(cfg.batch_size):                       # padded words: zero rows, masked out
        n = int(sl[b])
        assert float(mask[b, 0, n:].abs().sum()) == 0.0 and float(mask[b, 0, :n].min()) == 1.0


def test_hsv_graph_with_zeroed_hsv_rows_is_the_plain_graph():
    """CMPCv5_HSV_model differs from CMPCv5_model only by the grid's three HSV channels (v5h:136-144): with the three weight rows that read
    them zeroed in every vis_trans head and fusion conv, every tap equals the plain graph's; the grid itself carries the image's HSV."""
    cfg_h, hp_h, bn, feats, words, im, sl, _ = _case(True)
    cfg_p = U5.tiny_cfg(B=2, T=5, hsv=False)
    C, R = cfg_h.v_emb_dim, cfg_h.rnn_size
    hp_p = {}
    for n, v in hp_h.items():
        if "/vis_trans_" in n and n.endswith("/DW"):
            hp_h[n] = v.clone()
            hp_h[n][:, :, C + 8:C + 11] = 0
            hp_p[n] = v[:, :, :C + 8].clone()
        elif "/fusion_" in n and n.endswith("/DW"):
            hp_h[n] = v.clone()
            hp_h[n][:, :, 2 * C + R + 8:] = 0
            hp_p[n] = v[:, :, :2 * C + R + 8].clone()
        else:
            hp_p[n] = v
    assert {n: tuple(v.shape) for n, v in hp_p.items()} == {n: s for n, s, _, _ in U5.head_param_specs(cfg_p)}
    with torch.no_grad():
        th = U5.head_forward(hp_h, bn, feats, words, sl, cfg_h, im=im)
        tp = U5.head_forward(hp_p, bn, feats, words, sl, cfg_p)
    assert set(th) == set(tp)
    for k in tp:
        if k == "spatial":
            continue
        assert torch.allclose(th[k], tp[k], rtol=0, atol=1e-12), k
    assert torch.equal(th["spatial"][..., :8], tp["spatial"])
    assert torch.equal(th["spatial"][..., 8:], V.hsv_map(im, cfg_h))
    # and with the rows live, the HSV reaches the output
    hp_h2 = U5.init_head_params(cfg_h)
    with torch.no_grad():
        t2 = U5.head_forward({k: v.double() for k, v in hp_h2.items()}, bn, feats, words, sl, cfg_h, im=im)
        t3 = U5.head_forward({k: v.double() for k, v in hp_h2.items()}, bn, feats, words, sl, cfg_h, im=im * 0.5)
    assert float((t2["vis_la_sp_c5"] - t3["vis_la_sp_c5"]).abs().max()) > 1e-3


def test_manifest_against_reference_conv_calls():
    """Names, creation order and shapes as the reference's _conv calls create them (v5u:120-122 laterals of 2048 / 1024 inputs; v5h:392,435
    vis_trans C + 8 + 3 and fusion 2C + R + 8 + 3 for the HSV graph; lstm() under dynamic_rnn's scope "rnn"), and the trainable totals
    at the full sizes of BASELINE config 4 (512 x 512, vf 64, L = 25)."""
    totals = {}
    for hsv in (False, True):
        cfg = U5.Cfg(batch_size=1, num_steps=25, vf_h=64, vf_w=64, H=512, W=512, hsv=hsv)
        specs = U5.head_param_specs(cfg)
        shapes = {n: s for n, s, _, _ in specs}
        names = [n for n, _, _, _ in specs]
        assert len(set(names)) == len(names)
        assert names[:3] == ["text_objseg/Variable", "text_objseg/rnn/lstm_cell/kernel", "text_objseg/rnn/lstm_cell/bias"]
        assert names[3:5] == ["text_objseg/c5_lateral/DW", "text_objseg/c5_lateral/biases"]
        assert not any("bidirectional_rnn" in n or "words_feat" in n or "c3_lateral" in n or "_f2/" in n for n in names)
        assert shapes["text_objseg/rnn/lstm_cell/kernel"] == (1300, 4000)
        assert shapes["text_objseg/c5_lateral/DW"] == (1, 1, 2048, 1000) and shapes["text_objseg/c4_lateral/DW"] == (1, 1, 1024, 1000)
        g = 11 if hsv else 8
        for lv in ("c5", "c4"):
            for h in range(1, 6):
                assert shapes[f"text_objseg/vis_trans_{lv}_head{h}/DW"] == (1, 1, 1000 + g, 1000)
            assert shapes[f"text_objseg/fusion_{lv}/DW"] == (1, 1, 2000 + 1000 + g, 500)
        # everything from the parser on is the BiLSTM graph's (same trunk), up to the grid widths
        v = [(n, s) for n, s, _, _ in V.head_param_specs(V.Cfg(batch_size=1, num_steps=25, vf_h=64, vf_w=64, H=512, W=512))]
        tail_v = [(n, s) for n, s in v[v.index(("text_objseg/words_parse_1/DW", (1, 1, 1000, 500))):] if "vis_trans" not in n and "fusion_" not in n]
        tail_u = [(n, shapes[n]) for n in names[names.index("text_objseg/words_parse_1/DW"):] if "vis_trans" not in n and "fusion_" not in n]
        assert tail_u == tail_v
        assert [n for n, _ in v if n.startswith("text_objseg/fusion_") or "vis_trans" in n] == [n for n in names if n.startswith("text_objseg/fusion_") or "vis_trans" in n]
        assert [s[0] for s in U5.bn_state_specs(cfg)] == [s[0] for s in V.bn_state_specs(cfg)]
        totals[hsv] = sum(int(np.prod(s)) for s in shapes.values())
    # CMPCv5_BiLSTM_model at the same sizes has 70,256,763: minus one LSTM direction (5,204,000) and words_feat (2,001,000)
    assert totals[False] == 63051763
    # + 3 grid rows in 10 vis_trans heads (3 x 1000 each) and 2 fusion convs (3 x 500 each)
    assert totals[True] == totals[False] + 10 * 3000 + 2 * 1500 == 63084763


def test_no_tanh_in_laterals_and_global_vec():
    """v5u:120-123 and v5u:317-319 have no tanh (the BiLSTM graph's v5:121,124,328 do): the lateral is l2norm(conv) exactly, and the
    exchange module's language vector is CMPC_model's."""
    cfg, hp, bn, feats, words, im, sl, _ = _case(False)
    with torch.no_grad():
        t = U5.head_forward(hp, bn, feats, words, sl, cfg)
        assert torch.allclose(t["lat_c5"], O.l2_normalize(O.conv1x1(hp, "c5_lateral", feats[2]), 3), rtol=0, atol=1e-14)
        nec = t["nec_lang"]
        gv = U5.global_vec(hp, t["fusion_c4"], nec, "c4gv_f1", cfg)
        gv_t = V.global_vec(hp, t["fusion_c4"], nec, "c4gv_f1", cfg)
    assert float((gv - gv_t).abs().max()) > 1e-6
    assert torch.allclose(gv.flatten().norm(), torch.tensor(1.0, dtype=gv.dtype))


def test_fp64_gradcheck_tiny():
    """torch.autograd.gradcheck of the whole cost (fp64, batch-norm in training mode) w.r.t. the HSV rows of a Mutan head, the fusion conv's
    HSV rows, a lateral bias and an exchange module's gv_lang bias: the oracle's analytic gradients -- what the GPU tests compare
    against -- are the derivative of its forward pass."""
    cfg, hp, bn, feats, words, im, sl, tgt = _case(True)
    cfg.num_steps = 3
    words, sl = words[:, :3], torch.clamp(sl, max=3)
    C, R = cfg.v_emb_dim, cfg.rnn_size
    kv, kf = "text_objseg/vis_trans_c5_head2/DW", "text_objseg/fusion_c4/DW"
    kl, kg = "text_objseg/c4_lateral/biases", "text_objseg/gv_lang_c5_2gv_f1/biases"
    Wv, Wf = hp[kv], hp[kf]

    def cost(rows_v, rows_f, b_l, b_g):
        p = dict(hp)
        p[kv] = torch.cat([Wv[:, :, :C + 8], rows_v.view(1, 1, 3, C)], 2)
        p[kf] = torch.cat([Wf[:, :, :2 * C + R + 8], rows_f.view(1, 1, 3, -1)], 2)
        p[kl], p[kg] = b_l, b_g
        taps = U5.head_forward(p, bn, feats, words, sl, cfg, im=im)
        return U5.losses(p, taps, tgt, cfg)["cost"]

    args = (Wv[0, 0, C + 8:].clone().requires_grad_(True), Wf[0, 0, 2 * C + R + 8:, :4].clone(), hp[kl].clone().requires_grad_(True),
            hp[kg].clone().requires_grad_(True))
    rest = Wf[0, 0, 2 * C + R + 8:, 4:]
    rows_f = args[1].requires_grad_(True)
    assert torch.autograd.gradcheck(lambda a, b, c, d: cost(a, torch.cat([b, rest], 1), c, d), (args[0], rows_f, args[2], args[3]),
                                    eps=1e-5, atol=5e-7, rtol=1e-3)   # the cost is ~1e4: central differences carry ~1e-7 of rounding
