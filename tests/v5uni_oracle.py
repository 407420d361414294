"""ORACLE (test infrastructure only) -- torch-CPU restatement of CMPCv5_model.LSTM_model and of its HSV variant CMPCv5_HSV_model.py:
build_graph() + train_op() with TF1 / tf.contrib.slim semantics, composed from oracle.cmpc_torch ("O", CMPC_model.py) and
oracle.cmpc_v5_torch ("V", CMPCv5_BiLSTM_model.py) pieces.  Only the stages in which the two graphs differ from those are restated here.

PARITY UNPINNED: TensorFlow 1.x cannot be installed here and the reference holds no golden vectors for these graphs.  Checked against its
building blocks in tests/test_oracle_v5_uni.py.

Citations are file:line in the reference; "v5u:" = CMPCv5_model.py, "v5h:" = CMPCv5_HSV_model.py, "v5:" = CMPCv5_BiLSTM_model.py.
`diff CMPCv5_BiLSTM_model.py CMPCv5_model.py` shows exactly these differences, everything else is V's:
  * vf_h = H // 8, vf_w = W // 8 (v5u:52-53; the keywords are ignored);
  * lstm() (v5u:158-178) is CMPC_model.lstm (CMPC_model.py:144-164): words_feat = l2-normalised LSTM outputs, seq_mask from all-zero
    rows; no BiLSTM, no words_feat conv, no tanh.  lang_feat is returned but build_lang2vis (v5u:415-430) never reads it;
  * laterals without tanh before the l2_normalize (v5u:120-123);
  * global_vec without tanh before the all-dims l2_normalize of gv_lang (v5u:317-319; v5:328 has it);
  * seg_feats = tf.concat(fused_feats, -1) of ONE tensor (v5u:151-152): the identity.
`diff CMPCv5_model.py CMPCv5_HSV_model.py`: the image's HSV (computed as in CMPCv5_BiLSTM_HSV_model.py:120-127) is NOT appended to the
backbone taps but to the 8-channel spatial grid, spatial_hsv with 11 channels (v5h:120-127,136-144).  It therefore enters every
vis_trans_*_head{1..5} (v_emb_dim + 8 + 3 inputs, v5h:388-392) and the fusion_* conv (v_emb_dim * 2 + rnn_size + 8 + 3, v5h:432-435);
build_spa_graph receives it and does not use it.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Dict

import torch

from oracle import cmpc_torch as O
from oracle import cmpc_v5_torch as V

LEVELS, EXG, BN_EPS = V.LEVELS, V.EXG, V.BN_EPS


@dataclass
class Cfg(V.Cfg):
    """CMPCv5_model.LSTM_model's graph-shaping arguments (v5u:21-53); hsv = CMPCv5_HSV_model.  vf_h / vf_w must equal H // 8, W // 8."""

    @property
    def lat_extra(self):
        return 0                                   # the laterals read the backbone taps only (v5h:128-134 are CMPCv5_model's)

    @property
    def grid_dim(self):
        return 11 if self.hsv else 8               # spatial (util/processing_tools.py:5-17) or spatial_hsv (v5h:136-137)


def head_param_specs(cfg: Cfg):
    """(name, shape, initialiser, flags) of the trainable variables under text_objseg in creation order (flags as V.head_param_specs)."""
    C, M, R, S = cfg.v_emb_dim, cfg.mlp_dim, cfg.rnn_size, cfg.grid_dim
    specs = []

    def conv(name, k, cin, cout):
        specs.append((f"text_objseg/{name}/DW", (k, k, cin, cout), "xavier", ("reg",)))
        specs.append((f"text_objseg/{name}/biases", (cout,), "zeros", ("x2",)))

    def ln(scope, dim):
        specs.append((f"text_objseg/{scope}/beta", (dim,), "zeros", ()))
        specs.append((f"text_objseg/{scope}/gamma", (dim,), "ones", ()))

    specs.append(("text_objseg/Variable", (cfg.vocab_size, cfg.glove_dim), "glove", ()))                     # v5u:159
    specs.append(("text_objseg/rnn/lstm_cell/kernel", (cfg.glove_dim + R, 4 * R), "glorot", ()))            # v5u:163-170 (dynamic_rnn scope "rnn")
    specs.append(("text_objseg/rnn/lstm_cell/bias", (4 * R,), "zeros", ()))
    conv("c5_lateral", 1, cfg.vf_dim, C)                                                                       # v5u:120
    conv("c4_lateral", 1, cfg.c4_dim, C)                                                                       # v5u:122
    conv("words_parse_1", 1, R, cfg.parse_dim)                                                                 # v5u:432-437
    conv("words_parse_2", 1, cfg.parse_dim, 4)
    for lv in LEVELS:                                                                                          # build_lang2vis v5u:415-430
        for h in range(1, 6):
            conv(f"vis_trans_{lv}_head{h}", 1, C + S, C)                                                       # v5h:390-392
            conv(f"lang_trans_{lv}_head{h}", 1, R, C)
        conv(f"words_trans_{lv}", 1, R, R)
        conv(f"spa_graph_trans2_{lv}", 1, C, C)
        ln(f"gconv_feat_ln_spa_graph_{lv}", C)
        conv(f"gconv_update_spa_graph_{lv}", 1, C, C)
        ln(f"gconv_update_ln_spa_graph_{lv}", C)
        conv(f"fusion_{lv}", 1, 2 * C + R + S, M)                                                              # v5h:432-435
    conv("score_c5", 3, cfg.mlp_dim, 1)                                                                        # v5u:140-143
    conv("score_c4", 3, cfg.mlp_dim, 1)
    for lv in EXG:                                                                                             # v5u:323-337
        conv(f"spa_graph_key_{lv}gv_f1", 1, M, M)
        conv(f"lang_query_{lv}gv_f1", 1, R, M)
        conv(f"gv_lang_{lv}gv_f1", 1, M + R, M)
        conv(f"lang_feat_{lv}_f1", 1, M, M)
        conv(f"trans_feat_{lv}_f1", 1, M, M)
    pre = "rnn/conv_lstm_cell"                                                                                 # util/cell.py:36-66
    specs.append((f"text_objseg/{pre}/kernel", (1, 1, 2 * M, 4 * M), "glorot", ()))
    specs.append((f"text_objseg/{pre}/W_ci", (cfg.vf_h, cfg.vf_w, M), "glorot", ()))
    specs.append((f"text_objseg/{pre}/W_cf", (cfg.vf_h, cfg.vf_w, M), "glorot", ()))
    ln(f"{pre}/LayerNorm", M)
    ln(f"{pre}/LayerNorm_1", M)
    ln(f"{pre}/LayerNorm_2", M)
    specs.append((f"text_objseg/{pre}/W_co", (cfg.vf_h, cfg.vf_w, M), "glorot", ()))
    ln(f"{pre}/LayerNorm_3", M)
    ln(f"{pre}/LayerNorm_4", M)
    for scope, k, cin, cout in V.bn_scopes(cfg):                                                               # the v5 trunk's slim convs
        specs.append((f"text_objseg/{scope}/weights", (k, k, cin, cout), "vscale", ("reg",)))
        specs.append((f"text_objseg/{scope}/BatchNorm/beta", (cout,), "zeros", ()))
        specs.append((f"text_objseg/{scope}/BatchNorm/gamma", (cout,), "ones", ()))
    specs.append(("text_objseg/decoder/upsampling_logits/conv_1x1/weights", (1, 1, cfg.aspp_depth, 1), "vscale", ("reg",)))
    specs.append(("text_objseg/decoder/upsampling_logits/conv_1x1/biases", (1,), "zeros", ("x2",)))
    return specs


bn_state_specs, init_bn_state = V.bn_state_specs, V.init_bn_state
init_backbone_params, backbone_taps = V.init_backbone_params, V.backbone_taps


def init_head_params(cfg: Cfg, seed: int = 1234, glove_seed: int = 7, dtype=torch.float32) -> Dict[str, torch.Tensor]:
    """The initialisers of V.init_head_params over this graph's variables."""
    g = torch.Generator().manual_seed(seed)
    out = {}
    for name, shape, kind, _ in head_param_specs(cfg):
        if kind in ("xavier", "glorot"):
            fi, fo = O._fans(shape)
            t = (torch.rand(shape, generator=g, dtype=torch.float64) * 2 - 1) * math.sqrt(6.0 / (fi + fo))
        elif kind == "vscale":
            fi, _ = O._fans(shape)
            t = torch.randn(shape, generator=g, dtype=torch.float64) * math.sqrt(2.0 / fi)
        elif kind == "zeros":
            t = torch.zeros(shape, dtype=torch.float64)
        elif kind == "ones":
            t = torch.ones(shape, dtype=torch.float64)
        elif kind == "glove":
            t = torch.randn(shape, generator=torch.Generator().manual_seed(glove_seed), dtype=torch.float64) * 0.4
        else:
            raise ValueError(kind)
        out[name] = t.to(dtype)
    return out


# ----------------------------------------------------------------------------------------
# the stages that differ
# ----------------------------------------------------------------------------------------
def lstm(p, words, seq_len, cfg: Cfg):
    """lstm(), v5u:158-178: one tf LSTMCell under dynamic_rnn(sequence_length) (V._lstm_dir), words_feat = l2_normalize(outputs, -1)
    [B,1,T,R], seq_mask from the all-zero rows of words_feat (v5u:177).  lang_feat (v5u:174) has no consumer."""
    emb = p["text_objseg/Variable"][words.long()]                                   # v5u:159-162
    outs = V._lstm_dir(emb, p["text_objseg/rnn/lstm_cell/kernel"], p["text_objseg/rnn/lstm_cell/bias"], seq_len, cfg.rnn_size)
    words_feat = O.l2_normalize(outs, -1).unsqueeze(1)                              # v5u:172-173
    seq_mask = (words_feat.abs().sum(-1, keepdim=True) != 0).to(emb.dtype)          # v5u:177
    return words_feat, seq_mask


def lateral(p, name, x):
    """v5u:120-123: 1x1 conv + l2_normalize over the channels, no tanh."""
    return O.l2_normalize(O.conv1x1(p, name, x), 3)


def spatial_grid(cfg: Cfg, im=None, dtype=torch.float32):
    """spatial (v5u:128) or, for the HSV graph, spatial_hsv = [spatial | HSV of the image resized to the map] (v5h:120-127,136-137)."""
    spatial = O.generate_spatial_batch(cfg.batch_size, cfg.vf_h, cfg.vf_w, dtype=dtype)
    if not cfg.hsv:
        return spatial
    return torch.cat([spatial, V.hsv_map(im, cfg).to(dtype)], -1)


def global_vec(p, feat, lang, lv, cfg):
    """global_vec, v5u:290-321: V.global_vec without the tanh on gv_lang (= CMPC_model's, O.global_vec)."""
    return O.global_vec(p, feat, lang, lv, cfg)


def gated_exchange_module(p, feat, feat1, lang, lv, cfg):
    """v5u:323-337: one gated branch."""
    gv = global_vec(p, feat, lang, lv + "gv_f1", cfg)
    return feat + O.lang_se(p, feat1, gv, lv + "_f1")


def head_forward(p, bn, feats, words, seq_len, cfg: Cfg, im=None, new_state=None):
    """build_graph(), v5u:101-156 / v5h:100-165.  feats = (c2, c4, c5) NHWC = res2b_relu, res4b22_relu, res5c_relu; im (BGR minus mean) is
    read by the HSV graph only.  Returns all taps ("spatial" = the grid the Mutan heads and the fusion read)."""
    assert cfg.vf_h == cfg.H // 8 and cfg.vf_w == cfg.W // 8, "CMPCv5_model.py:52-53 derives vf_h = H // 8, vf_w = W // 8"
    c2, c4, c5 = feats
    taps = {}
    words_feat, seq_mask = lstm(p, words, seq_len, cfg)
    taps["words_feat"], taps["seq_mask"] = words_feat, seq_mask
    v5 = lateral(p, "c5_lateral", c5)
    v4 = lateral(p, "c4_lateral", c4)
    taps["lat_c5"], taps["lat_c4"] = v5, v4
    spatial = spatial_grid(cfg, im, dtype=c5.dtype)
    taps["spatial"] = spatial
    words_parse = O.lang_parser(p, words_feat, seq_mask)                             # v5u:130
    taps["words_parse"] = words_parse
    fus = {}
    for lv, v in (("c5", v5), ("c4", v4)):                                           # v5u:132-135, v5h:141-144
        fus[lv] = V.build_lang2vis(p, v, words_feat, words_parse, seq_mask, spatial, lv, cfg, taps)
        taps[f"fusion_{lv}"] = fus[lv]
    for lv in LEVELS:                                                                # v5u:140-143
        sc = O.conv3x3(p, f"score_{lv}", fus[lv])
        taps[f"score_{lv}"] = sc
        taps[f"up_{lv}"] = O.resize_bilinear(sc, cfg.H, cfg.W)
    nec = O.weighted_lang(words_parse, words_feat, "nec")                            # v5u:147
    taps["nec_lang"] = nec
    f4, f5 = fus["c4"], fus["c5"]                                                    # gated_exchange_fusion_lstm_2times v5u:339-378
    e4 = O.l2_normalize(gated_exchange_module(p, f4, f5, nec, "c4", cfg), 3)
    e5 = O.l2_normalize(gated_exchange_module(p, f5, f4, nec, "c5", cfg), 3)
    e42 = O.l2_normalize(gated_exchange_module(p, e4, e5, nec, "c4_2", cfg), 3)
    e52 = O.l2_normalize(gated_exchange_module(p, e5, e4, nec, "c5_2", cfg), 3)
    taps["exg_c4"], taps["exg_c5"], taps["exg_c4_2"], taps["exg_c5_2"] = e4, e5, e42, e52
    fused = V.conv_lstm(p, (e42, e52), cfg)
    taps["fused"] = fused
    enc = V.aspp(p, bn, torch.cat([fused], -1), cfg, new_state, taps)                # v5u:151-153: concat of one tensor
    taps["aspp"] = enc
    pred = V.decoder(p, bn, enc, c2, cfg, new_state, taps)                           # v5u:154
    taps["pred"] = pred
    taps["up"] = O.resize_bilinear(pred, cfg.H, cfg.W)                               # v5u:155
    taps["sigm"] = torch.sigmoid(taps["up"])
    return taps


def losses(p, taps, target_fine, cfg: Cfg):
    """train_op() loss part (v5u:510-533): 0.8 final + 0.1 c5 + 0.1 c4, L2 on 'DW' / 'weights'."""
    def wll(scores):
        return O.sigmoid_xent(scores, target_fine).sum(dim=(1, 2, 3)).mean()
    out = {"loss_c5": wll(taps["up_c5"]), "loss_c4": wll(taps["up_c4"]), "loss_last": wll(taps["up"])}
    out["loss_all"] = 0.8 * out["loss_last"] + 0.1 * out["loss_c5"] + 0.1 * out["loss_c4"]
    reg = 0.0
    for name, _, _, flags in head_param_specs(cfg):
        if "reg" in flags:
            reg = reg + (p[name] ** 2).sum() / 2
    out["reg_loss"] = cfg.weight_decay * reg
    out["cost"] = out["loss_all"] + out["reg_loss"]
    pred, labl = taps["up"] > 0, target_fine != 0
    inter = (pred & labl).sum(dim=(1, 2, 3)).to(torch.float64)
    union = (pred | labl).sum(dim=(1, 2, 3)).to(torch.float64)
    out["mIoU"] = (inter / union).mean()
    return out


def grads_of(p, bn, feats, words, seq_len, target_fine, cfg: Cfg, im=None, tap_grads=False):
    """d cost / d every trainable variable with the x2 on 'biases'.  Returns (scalars, grads, taps, new bn state); tap_grads: grads also
    holds d cost / d c5, c4 under "dc5", "dc4" (conv5=True: the backbone taps' gradients, v5u:521-525 as v5's)."""
    leaves = {k: v.detach().clone().requires_grad_(True) for k, v in p.items()}
    c2, c4, c5 = feats
    if tap_grads:
        c4, c5 = c4.detach().clone().requires_grad_(True), c5.detach().clone().requires_grad_(True)
    new_state = {}
    taps = head_forward(leaves, bn, (c2, c4, c5), words, seq_len, cfg, im=im, new_state=new_state)
    ls = losses(leaves, taps, target_fine, cfg)
    names = list(leaves)
    wrt = [leaves[n] for n in names] + ([c5, c4] if tap_grads else [])
    gs = torch.autograd.grad(ls["cost"], wrt, allow_unused=True)
    flags = {n: f for n, _, _, f in head_param_specs(cfg)}
    grads = {}
    for n, g in zip(names, gs):
        g = torch.zeros_like(leaves[n]) if g is None else g
        grads[n] = (g * 2.0 if "x2" in flags[n] else g).detach()
    if tap_grads:
        grads["dc5"], grads["dc4"] = gs[-2].detach(), gs[-1].detach()
    return {k: float(v.detach()) for k, v in ls.items()}, grads, {k: v.detach() for k, v in taps.items()}, new_state


def train_step(p, bn, opt: O.TFAdam, step, feats, words, seq_len, target_fine, cfg: Cfg, im=None):
    """One sess.run([train, ...]): UPDATE_OPS (moving statistics) then TF-Adam.  p and bn updated in place."""
    scal, grads, _, new_state = grads_of(p, bn, feats, words, seq_len, target_fine, cfg, im=im)
    lr = O.poly_lr(step, cfg)
    with torch.no_grad():
        opt.step(p, grads, lr)
        bn.update(new_state)
    scal["lr"] = lr
    return scal


def tiny_cfg(B=2, T=6, hw=8, C=40, M=24, hsv=False, train_mode=True):
    """V.tiny_cfg's shrunken graph (H = W = 8 hw, so vf_h = H // 8 holds)."""
    v = V.tiny_cfg(B=B, T=T, hw=hw, C=C, M=M, hsv=hsv, train_mode=train_mode)
    return Cfg(**{k: getattr(v, k) for k in v.__dataclass_fields__})
