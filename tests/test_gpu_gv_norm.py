"""GPU tests of the per-sample gv_lang norm (cmpc_set_gv_norm / LSTM_model.set_gv_norm("sample")): l2_normalize(gv_lang) has no axis
(CMPC_model.py:241), so the graph built at batch_size = B couples the samples of a batch while every inference loop of the reference
runs it at batch_size = 1.  Mode "sample" must BE the reference at batch 1: the oracles here are evaluated one sample at a time with
batch_size = 1 and the product, run on the whole batch, is held to the bars of the existing parity tests (test_gpu_parity.py: taps
2e-5 in f32 and 6e-3 in f16, gradients 2e-4, mean-IoU delta 1e-4; test_gpu_v5.py / test_gpu_v5_uni.py for the v5 graphs)."""
import dataclasses

import pytest
import torch

from tests import util as U
from tests.util import O

pytestmark = pytest.mark.gpu


def _one(x, b):
    return x[b: b + 1]


def per_sample_taps(head_forward, feats, words, sl, cfg, B):
    """The oracle at batch_size = 1 on each sample, taps concatenated along the batch axis."""
    c1 = dataclasses.replace(cfg, batch_size=1)
    with torch.no_grad():
        ts = [head_forward([_one(f, b) for f in feats], _one(words, b), _one(sl, b), c1, b) for b in range(B)]
    return {k: torch.cat([t[k] for t in ts], 0) for k in ts[0]}


def _case(B, seed=0):
    torch.set_num_threads(8)
    cfg = U.tiny_cfg(B=B)
    hp, bp = O.init_head_params(cfg), O.init_backbone_params(cfg)
    words, im, sl, tgt = O.synth_batch(cfg, seed=seed)
    feats = O.backbone_forward(bp, im, cfg)
    return dict(cfg=cfg, hp=hp, bp=bp, words=words, im=im, sl=sl, tgt=tgt, feats=feats)


def _model(case, dtype, mode="train"):
    return U.pkg().LSTM_model(head_params=case["hp"], backbone_params=case["bp"], **U.model_kwargs(case["cfg"], dtype, mode))


def _check(pt, ref, bar, what):
    errs = {k: U.rel_err(pt[k], r) for k, r in ref.items()}
    worst = max(errs.items(), key=lambda kv: kv[1])
    print("%s: worst tap %s %.2e (bar %.0e), up %.2e" % (what, worst[0], worst[1], bar, errs["up"]))
    for k, e in errs.items():
        assert e < bar, (what, k, e)


@pytest.mark.parametrize("B", [2, 4])
@pytest.mark.parametrize("dtype,bar", [("f32", 2e-5), ("f16", 6e-3)])
def test_sample_mode_is_the_oracle_at_batch_1(B, dtype, bar):
    case = _case(B)
    cfg, hp = case["cfg"], case["hp"]
    with torch.no_grad():
        batch = O.head_forward(hp, case["feats"], case["words"], case["sl"], cfg)
    alone = per_sample_taps(lambda f, w, s, c1, b: O.head_forward(hp, f, w, s, c1), case["feats"], case["words"], case["sl"], cfg, B)
    print("oracle, B = %d: up of the batch graph vs each sample alone %.2e" % (B, U.rel_err(batch["up"], alone["up"])))
    m = _model(case, dtype)
    assert m.gv_norm == "batch"
    feats = [f.to(m.device) for f in case["feats"]]
    ups = {}
    for mode, ref in (("sample", alone), ("batch", batch), ("sample", alone)):        # back and forth: the switch is not sticky
        m.set_gv_norm(mode)
        assert m.gv_norm == mode
        o = m.head(feats, case["words"], case["sl"])
        torch.cuda.synchronize()
        pt = U.product_taps_as_oracle(o, cfg)
        _check(pt, ref, bar, "%s B=%d mode %s" % (dtype, B, mode))
        ups[mode] = pt["up"].clone()
    d = U.rel_err(ups["sample"], ups["batch"])
    print("%s B=%d: up, mode sample vs mode batch %.2e" % (dtype, B, d))
    if dtype == "f32":
        assert d > bar              # the switch does something (the oracle's own difference is 1.2e-2 at B = 2)
    with pytest.raises(ValueError):
        m.set_gv_norm("rows")
    assert m.gv_norm == "sample"


def _v5_bars(pt, alone32, alone64, what, loose):
    """test_gpu_v5.py:104 / test_gpu_v5_uni.py:113: against the float64 oracle, 2e-5 (the taps listed in `loose` at their bars there) or
    3x the float32 oracle's own distance from it."""
    for k, ref in alone32.items():
        e, own = U.rel_err(pt[k], alone64[k]), U.rel_err(ref, alone64[k])
        bar = max(loose.get(k, 2e-5), 3 * own)
        if e > 0.25 * bar or k == "up":
            print("%s: %s %.2e (bar %.2e, f32 oracle vs f64 %.2e)" % (what, k, e, bar, own))
        assert e < bar, (what, k, e, bar)


@pytest.mark.parametrize("graph", ["CMPCv5_BiLSTM_model", "CMPCv5_model"])
def test_v5_graphs_in_eval_mode(graph):
    """The v5 graphs' batch norms use moving statistics in eval mode, so there too only gv_lang couples the samples."""
    if graph == "CMPCv5_BiLSTM_model":
        import tests.test_gpu_v5 as T5
        from oracle import cmpc_v5_torch as V
        loose = {"aspp_image": 2e-3, "aspp": 3e-4, "dec_cat": 3e-4, "dec_net2": 3e-4, "pred": 3e-4, "up": 3e-4, "sigm": 3e-4}      # test_gpu_v5.py:102
    else:
        import tests.test_gpu_v5_uni as T5
        from tests import v5uni_oracle as V
        loose = T5.LOOSE
    case = T5.make_case(hsv=False, train=False, B=2)
    cfg, B = case["cfg"], 2
    hp64, bn64 = {k: v.double() for k, v in case["hp"].items()}, {k: v.double() for k, v in case["bn"].items()}
    f64 = [f.double() for f in case["feats"]]
    fwd32 = lambda f, w, s, c1, b: V.head_forward(case["hp"], case["bn"], f, w, s, c1, im=_one(case["im"], b))
    fwd64 = lambda f, w, s, c1, b: V.head_forward(hp64, bn64, f, w, s, c1, im=_one(case["im"], b).double())
    alone32 = per_sample_taps(fwd32, case["feats"], case["words"], case["sl"], cfg, B)
    alone64 = per_sample_taps(fwd64, f64, case["words"], case["sl"], cfg, B)
    with torch.no_grad():
        batch32 = V.head_forward(case["hp"], case["bn"], case["feats"], case["words"], case["sl"], cfg, im=case["im"])
        batch64 = V.head_forward(hp64, bn64, f64, case["words"], case["sl"], cfg, im=case["im"].double())
    print("%s oracle: up of the batch graph vs each sample alone %.2e" % (graph, U.rel_err(batch64["up"], alone64["up"])))
    m = T5.build(case, "f32", mode="eval")
    feats = [f.to(m.device) for f in case["feats"]]
    ups = {}
    for mode, r32, r64 in (("sample", alone32, alone64), ("batch", batch32, batch64)):
        m.set_gv_norm(mode)
        o = m.head(feats, case["words"], case["sl"], im=case["im"])
        torch.cuda.synchronize()
        pt = T5.taps_as_oracle(o, cfg)
        _v5_bars(pt, r32, r64, "%s mode %s" % (graph, mode), loose)
        ups[mode] = pt["up"].clone()
    d = U.rel_err(ups["sample"], ups["batch"])
    print("%s: up, mode sample vs mode batch %.2e" % (graph, d))
    assert d > loose["up"]


def _ref_grad(cfg, hp, grads, n):
    """test_gpu_parity._ref_grad: oracle gradient of `cost` -> gradient of cls_loss_all."""
    flags = {k: f for k, _, _, f in O.head_param_specs(cfg)}
    g = grads[n] / (2.0 if "x2" in flags[n] else 1.0)
    return g - cfg.weight_decay * hp[n] if "reg" in flags[n] else g


def test_gradients_in_sample_mode():
    """The loss is the mean over the batch, so in mode "sample" every gradient is the mean of the oracle's per-sample batch-1 gradients.
    Names, bars and the two documented exceptions as in test_head_forward_backward_fp32_matches_oracle.  The backward pass follows the
    mode its forward ran in, also when the mode is switched between the two."""
    B = 2
    case = _case(B)
    cfg, hp = case["cfg"], case["hp"]
    c1 = dataclasses.replace(cfg, batch_size=1)
    per = [O.grads_of(hp, [_one(f, b) for f in case["feats"]], _one(case["words"], b), _one(case["sl"], b), _one(case["tgt"], b), c1) for b in range(B)]
    grads = {n: sum(p[1][n] for p in per) / B for n in per[0][1]}
    scal = {k: sum(p[0][k] for p in per) / B for k in ("loss_c5", "loss_c4", "loss_c3", "loss_last", "loss_all")}
    m = _model(case, "f32")
    m.set_gv_norm("sample")
    feats = [f.to(m.device) for f in case["feats"]]
    o = m.loss_and_grads(feats, case["words"], case["tgt"], case["sl"])
    torch.cuda.synchronize()
    for k, v in scal.items():
        print("%s product %.6f oracle mean %.6f" % (k, float(o[k]), v))
        assert abs(float(o[k]) - v) <= 1e-5 * abs(v), k
    g = {n: t.clone() for n, t in m.store.grad_dict().items()}
    errs = {}
    for n in grads:
        ref = _ref_grad(cfg, hp, grads, n)
        if "spa_graph_key" in n and n.endswith("biases"):
            # softmax over nodes is invariant to b_k.q: the exact gradient is 0 (the oracle returns rounding noise)
            assert float(g[n].abs().max()) == 0.0 and float(ref.abs().max()) < 1e-6
            continue
        errs[n] = (U.rel_err(g[n], ref), 2e-3 if ("spa_graph_trans2" in n and n.endswith("biases")) else 2e-4)    # cancellation-dominated
    print("largest gradient errors:", sorted(((e, n) for n, (e, _) in errs.items()), reverse=True)[:5])
    for n, (e, tol) in errs.items():
        assert e < tol, (n, e)
    # the same step with the mode switched after the forward pass: cmpc_backward differentiates what that forward computed
    m2 = _model(case, "f32")
    m2.set_gv_norm("sample")
    m2.head(feats, case["words"], case["sl"], case["tgt"])
    m2.set_gv_norm("batch")
    m2.eng.backward()
    torch.cuda.synchronize()
    g2 = m2.store.grad_dict()
    for n in g:
        assert torch.equal(g[n], g2[n]), n
    # and the batch mode's gradients are the batch graph's, different from these
    m2.loss_and_grads(feats, case["words"], case["tgt"], case["sl"])
    torch.cuda.synchronize()
    _, gb, _ = O.grads_of(hp, case["feats"], case["words"], case["sl"], case["tgt"], cfg)
    n = "text_objseg/fusion_c5/DW"
    gbatch = m2.store.grad_dict()[n]
    assert U.rel_err(gbatch, _ref_grad(cfg, hp, gb, n)) < 2e-4 and U.rel_err(gbatch, g[n]) > 2e-4


@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_sample_mode_makes_samples_independent(dtype):
    """In mode "sample" a sample kept at its batch position gives bit-identical `up` and `sigm` whatever the other samples are: nothing
    but gv_lang couples the samples of a batch (layer norms, softmaxes and the ConvLSTM are per sample).  Across batch positions and batch
    sizes only the parity bars of test_sample_mode_is_the_oracle_at_batch_1 apply: tile dispatch and per-tile statistics may differ, so
    equality there is not asserted."""
    B = 4
    a, b = _case(B, seed=0), _case(B, seed=9)
    m = _model(a, dtype, mode="eval")
    for keep in (0, 2):
        mix = {}
        for k in ("words", "im", "sl"):
            mix[k] = b[k].clone()
            mix[k][keep] = a[k][keep]
        outs = {}
        for mode in ("sample", "batch"):
            m.set_gv_norm(mode)
            x = m.forward(a["words"], a["im"], a["sl"])
            y = m.forward(mix["words"], mix["im"], mix["sl"])
            torch.cuda.synchronize()
            outs[mode] = (x, y)
        x, y = outs["sample"]
        for k in ("up", "sigm", "pred"):
            assert torch.equal(x[k][keep], y[k][keep]), (dtype, keep, k, float((x[k][keep].float() - y[k][keep].float()).abs().max()))
        assert not torch.equal(x["up"], y["up"])                                   # the mates did change
        x, y = outs["batch"]
        if dtype == "f32":
            assert not torch.equal(x["up"][keep], y["up"][keep])                   # the batch-wide norm carries them over


@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_full_size_mean_iou_in_sample_mode(dtype):
    """BASELINE.json config 2 (320 x 320, L = 20, B = 8) on bench.py's synthetic batch, mode "sample": mean-IoU delta against the oracle
    run one sample at a time with batch_size = 1, bar 1e-4 (the project's parity bar)."""
    from bench import synth_batch
    torch.set_num_threads(16)
    B = 8
    cfg = O.Cfg(batch_size=B)
    c1 = dataclasses.replace(cfg, batch_size=1)
    hp, bp = O.init_head_params(cfg), O.init_backbone_params(cfg)
    w, im, sl, tg = map(torch.from_numpy, synth_batch(B, 20, 320, 320, cfg.vocab_size, 0))
    with torch.no_grad():
        feats = O.backbone_forward(bp, im, cfg)
        ious, ups = [], []
        for b in range(B):
            taps = O.head_forward(hp, [_one(f, b) for f in feats], _one(w, b), _one(sl, b), c1)
            ious.append(float(O.losses(hp, taps, _one(tg, b), c1)["mIoU"]))
            ups.append(taps["up"])
        ref_miou, ref_up = sum(ious) / B, torch.cat(ups, 0)
    m = U.pkg().LSTM_model(batch_size=B, mode="train", dtype=dtype, head_params=hp, backbone_params=bp)
    m.set_gv_norm("sample")
    with torch.no_grad():
        o = m.head(m.features(im), w, sl, tg)
    torch.cuda.synchronize()
    up = o["up"].float().cpu()
    d = abs(float(o["mIoU"]) - ref_miou)
    print("%s B=8 mode sample: dIoU=%.2e flipped_px=%d up_rel_err=%.2e oracle mIoU %.6f" % (
        dtype, d, int(((up > 0) != (ref_up > 0)).sum()), U.rel_err(up, ref_up), ref_miou))
    assert d <= 1e-4
