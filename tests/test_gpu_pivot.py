"""GPU tests of the pivot-frame step: cmpc_mask_pool against tests/pivot_ref.py's float64 sums within the derived bound (every output,
f32 / f16 / bf16 taps, both modes, edge shapes, guarded buffers, bit-identical reruns, strided taps), cmpc_level_agree's counts with ==,
and describe= inside FrameSegmenter / ClipSegmenter: the masks stay bit-identical, and every logged descriptor, area and count equals
the op-level wrappers called on the taps and fetches of the same batches."""
import functools
import importlib

import numpy as np
import pytest
import torch

from tests import pivot_ref as R
from tests import test_gpu_clip_segment as TGC
from tests import test_gpu_segment as TG
from tests.test_gpu_segment_jf import Recorder

pytestmark = pytest.mark.gpu

HU = importlib.import_module("cmpc-refseg_amd.hostutil")
EV = importlib.import_module("cmpc-refseg_amd.evaluate")
SG = importlib.import_module("cmpc-refseg_amd.segment")
L = importlib.import_module("cmpc-refseg_amd._lib")

GUARD = -1515870811                    # 0xA5A5A5A5 as int32
THR = 0.5
TDT = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
CH = L.POOL_CHUNK
# (n, h, w, C, score strides): the smallest call; odd sizes under a strided score; channels that are no multiple of a workgroup's 512
# and more than one chunk of positions; the largest n; h * w one below, at and one above the chunk of positions; the real c4 tap
SHAPES = [(1, 1, 1, 8, (1, 1)), (3, 3, 5, 24, (2, 3)), (5, 7, 9, 1000, (1, 1)), (32, 8, 8, 40, (1, 1)),
          (2, 7, 9, 16, (1, 2)), (2, 8, 8, 16, (2, 1)), (2, 5, 13, 16, (1, 1)), (2, 40, 40, 1024, (8, 8))]
assert [h * w for _, h, w, _, _ in SHAPES[4:7]] == [CH - 1, CH, CH + 1]


@functools.lru_cache(maxsize=None)
def _case(shape, dtype):
    """Inputs and float64 references of one (shape, storage type), made once: the first half of the channels post-ReLU, the rest signed;
    a tenth of the score exactly at the threshold and a tenth exactly 0."""
    n, h, w, C, (fy, fx) = shape
    rng = np.random.default_rng([n, h, w, C, ("f32", "f16", "bf16").index(dtype)])
    x = rng.normal(0, 1, (n, h, w, C)).astype(np.float32)
    x[..., : C // 2] = np.maximum(x[..., : C // 2], 0)
    score = rng.uniform(0, 1, (n, h * fy, w * fx)).astype(np.float32)
    pick = rng.uniform(0, 1, score.shape)
    score[pick < 0.1] = np.float32(THR)
    score[pick > 0.9] = 0.0
    feat = torch.from_numpy(x).to(TDT[dtype]).cuda()
    stored = feat.float().cpu().numpy()                    # the stored values, upcast
    refs = {mode: R.pool(stored, score, mode, THR) for mode in ("soft", "hard")}
    return feat, torch.from_numpy(score).cuda(), refs


def _guarded_pool(feat, score, mode, thr, n=None):
    """cmpc_mask_pool called directly with desc, area and the workspace inside one guard-filled buffer; checks the guard band and that
    nothing past the workspace's stated size is written.  Returns (desc, area) as host arrays."""
    n = feat.shape[0] if n is None else n
    h, w, C = feat.shape[1:]
    need = EV.pool_workspace(n, h, w, C)
    up4 = lambda v: -(-v // 4) * 4
    o_desc = 16
    o_area = o_desc + n * C + 16
    o_ws = up4(o_area + n + 16)
    total = o_ws + need // 4 + 16
    buf = torch.full((total,), GUARD, dtype=torch.int32, device="cuda")
    base = buf.data_ptr()
    assert base % 16 == 0
    stride = feat.stride(0) if feat.shape[0] > 1 else h * w * C
    L.call("cmpc_mask_pool", EV._POOL_DT[feat.dtype], feat.data_ptr(), stride, score.data_ptr(), score.shape[1], score.shape[2], n, h, w, C,
           L.POOL_MODES[mode], float(thr), base + 4 * o_desc, base + 4 * o_area, base + 4 * o_ws, need, torch.cuda.current_stream().cuda_stream)
    host = buf.cpu().numpy()
    inside = np.zeros(total, bool)
    inside[o_desc: o_desc + n * C] = inside[o_area: o_area + n] = inside[o_ws: o_ws + need // 4] = True
    assert np.all(host[~inside] == GUARD), "words outside desc, area and the workspace were written"
    return host[o_desc: o_desc + n * C].view(np.float32).reshape(n, C).copy(), host[o_area: o_area + n].view(np.float32).copy()


@pytest.mark.parametrize("mode", ["soft", "hard"])
@pytest.mark.parametrize("dtype", ["f32", "f16", "bf16"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(str(v) for v in s[:4]))
def test_mask_pool_within_the_bound(shape, dtype, mode):
    """Every output: |got - ref| <= (N + 1) 2^-24 sum |wgt * x| (tests/pivot_ref.bound), area by the same rule; a second call and the
    Python wrapper give the same bits; the guard band is intact."""
    n, h, w, C, _ = shape
    feat, score, refs = _case(shape, dtype)
    ref, ref_area, mag, amag = refs[mode]
    desc, area = _guarded_pool(feat, score, mode, THR)
    err, lim = np.abs(desc.astype(np.float64) - ref), R.bound(h, w, mag)
    aerr, alim = np.abs(area.astype(np.float64) - ref_area), R.bound(h, w, amag)
    worst = float(np.max(err / np.maximum(lim, 1e-300))) if lim.max() > 0 else 0.0
    print("%s %s %s: worst error / bound %.3f (desc), %.3f (area)" % (shape[:4], dtype, mode, worst,
                                                                     float(np.max(aerr / np.maximum(alim, 1e-300))) if alim.max() > 0 else 0.0))
    assert np.all(np.isfinite(desc)) and np.all(err <= lim), (int((err > lim).sum()), worst)
    assert np.all(aerr <= alim)
    if mode == "hard":
        assert np.array_equal(area, ref_area.astype(np.float32))              # a count of at most 1600 ones is exact in float32
    d2, a2 = _guarded_pool(feat, score, mode, THR)
    assert np.array_equal(desc.view(np.uint32), d2.view(np.uint32)) and np.array_equal(area.view(np.uint32), a2.view(np.uint32))
    d3, a3 = EV.mask_pool(feat, score, mode, THR)
    assert d3.dtype == torch.float32 and tuple(d3.shape) == (n, C) and tuple(a3.shape) == (n,)
    assert np.array_equal(d3.cpu().numpy().view(np.uint32), desc.view(np.uint32)) and np.array_equal(a3.cpu().numpy().view(np.uint32), area.view(np.uint32))


def test_mask_pool_threshold_is_tested_on_the_float_itself():
    """Hard weights: values one ulp either side of the threshold fall on their own sides, the threshold itself counts."""
    t = np.float32(THR)
    score = np.full((1, 8, 8), np.nextafter(t, np.float32(0)), np.float32)
    score[0, 2:4, 2:6] = t
    score[0, 6, 1:4] = np.nextafter(t, np.float32(1))
    feat = torch.ones(1, 8, 8, 8, device="cuda")
    desc, area = EV.mask_pool(feat, torch.from_numpy(score).cuda(), "hard", float(t))
    assert area.item() == 11.0 and torch.all(desc == 11.0)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_mask_pool_strided_taps_and_part_of_a_batch(dtype):
    """Results read from every other tap of a batch, and n smaller than the batch: the same bits as a contiguous copy; more than
    MAX_BATCH results go in chunks; one result does not depend on the results beside it."""
    rng = np.random.default_rng(2)
    big = torch.from_numpy(rng.normal(0, 1, (8, 7, 9, 24)).astype(np.float32)).to(TDT[dtype]).cuda()
    score = torch.from_numpy(rng.uniform(0, 1, (3, 14, 9)).astype(np.float32)).cuda()
    sel = big[::2][:3]
    assert sel.stride(0) == 2 * 7 * 9 * 24 and not sel.is_contiguous()
    d0, a0 = EV.mask_pool(sel.contiguous(), score)
    d1, a1 = EV.mask_pool(sel, score)
    d2, a2 = _guarded_pool(big[::2], score, "soft", THR, n=3)                  # n smaller than the batch, through the entry point
    for d, a in ((d1.cpu().numpy(), a1.cpu().numpy()), (d2, a2)):
        assert np.array_equal(d.view(np.uint32), d0.cpu().numpy().view(np.uint32)) and np.array_equal(a.view(np.uint32), a0.cpu().numpy().view(np.uint32))
    d3, a3 = EV.mask_pool(big[4:5], score[2:3])                                # result 2 on its own
    assert torch.equal(d3[0], d0[2]) and torch.equal(a3[0], a0[2])
    many = big[:5].repeat(8, 1, 1, 1)                                          # 40 results: two calls
    ms = score[[0, 1, 2, 0, 1]].repeat(8, 1, 1)
    dm, am = EV.mask_pool(many, ms)
    assert torch.equal(dm[35:40], dm[:5]) and torch.equal(am[35:40], am[:5]) and torch.equal(dm[0], d0[0])


AGREE_SHAPES = [(1, 5, 7), (32, 3, 3), (3, 33, 65), (2, 200, 161)]


@pytest.mark.parametrize("shape", AGREE_SHAPES, ids=lambda s: "x".join(str(v) for v in s))
def test_level_agree_counts_are_exact(shape):
    """counts == the reference: odd sizes, one and many workgroups per map, n = 1 and 32, values exactly at the threshold (not above
    it), a result whose maps are both empty (U = 0), inside a guarded buffer."""
    n, h, w = shape
    rng = np.random.default_rng(n * h)
    logit = EV.agree_logit(0.2)
    a = rng.normal(-1.4, 1.0, shape).astype(np.float32)
    b = (a + rng.normal(0, 0.7, shape)).astype(np.float32)
    a[rng.uniform(0, 1, shape) < 0.1] = np.float32(logit)
    b[rng.uniform(0, 1, shape) < 0.1] = np.float32(logit)
    a[-1], b[-1] = np.float32(logit), np.float32(logit) - 1                    # the last result: both maps empty
    want = R.agree(a, b, logit)
    assert want[-1].tolist() == [0, 0] and (h * w < 100 or (0 < want[0, 0] < want[0, 1] < h * w))
    ad, bd = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    got = EV.level_agree(ad, bd, 0.2)
    assert got.dtype == torch.int64 and np.array_equal(got.cpu().numpy(), want), (got.cpu().numpy().tolist(), want.tolist())
    assert np.array_equal(EV.level_agree(ad[..., None], bd[..., None]).cpu().numpy(), want)
    buf = torch.full((2 * n + 8,), GUARD, dtype=torch.int64, device="cuda")
    L.call("cmpc_level_agree", ad.data_ptr(), bd.data_ptr(), n, h, w, logit, buf[4:].data_ptr(), torch.cuda.current_stream().cuda_stream)
    host = buf.cpu().numpy()
    assert np.array_equal(host[4: 4 + 2 * n].reshape(n, 2), want) and np.all(host[:4] == GUARD) and np.all(host[4 + 2 * n:] == GUARD)


# ---- describe= inside the segmenters ---------------------------------------------------------------------------------------------------
SIZES = [(48, 80), (100, 64)]


def _frames(rng, n):
    return [TG._image(rng, *SIZES[(f // 3) % 2]) for f in range(n)]


def _compare_log(log, seq, want, h, w):
    """want: {(e, f): (desc, area, counts, ref, mag)} from the op-level wrappers and pivot_ref."""
    assert len(log) == len(want) and sorted(log.seqs) == sorted({(seq, e) for e, _ in want})
    for (e, f), (desc, area, cnt, ref, mag) in want.items():
        got_d, got_a, got_c = log.seqs[(seq, e)][f]
        assert np.array_equal(got_d.view(np.uint32), desc.view(np.uint32)), (e, f)
        assert np.float32(got_a).view(np.uint32) == np.float32(area).view(np.uint32), (e, f)
        c = HU.consistency(*cnt)
        assert (np.isnan(got_c) and np.isnan(c)) or got_c == c, (e, f, got_c, cnt)
        assert np.all(np.abs(got_d.astype(np.float64) - ref) <= R.bound(h, w, mag)), (e, f)


def _frame_oplevel(model, frames, exprs, level, mode, thr):
    """The op-level wrappers on the taps and fetches of the same padded batches, in mode "sample": {(e, f): ...} as _compare_log takes."""
    B, H, W = model.batch_size, model.H, model.W
    out = {}
    prev = model.gv_norm
    model.set_gv_norm("sample")
    with torch.no_grad():
        for idx in SG.plan_batches(len(frames), B):
            feed, _ = EV.prepare_images([frames[i] for i in idx], H, W)
            feats, ev = model.features_async(feed)
            n = len(set(idx))
            for e, (ids, sl) in enumerate(exprs):
                o = model.head(feats, torch.from_numpy(np.repeat(ids[None], B, 0)), torch.full((B,), sl, dtype=torch.int32), after=ev, im=feed)
                sigm = o["sigm"].float().reshape(B, H, W)
                tap = feats[level]
                desc, area = EV.mask_pool(tap[:n], sigm[:n], mode, thr)
                cnt = EV.level_agree(o["score_c4"][:n], o["score_c5"][:n], SG.AGREE_THRESHOLD)
                ref, _, mag, _ = R.pool(tap[:n].float().cpu().numpy(), sigm[:n].cpu().numpy(), mode, thr)
                desc, area, cnt = desc.cpu().numpy(), area.cpu().numpy(), cnt.cpu().numpy()
                for b in range(n):
                    out[(e, idx[b])] = (desc[b], area[b], cnt[b], ref[b], mag[b])
    model.set_gv_norm(prev)
    return out


@pytest.mark.parametrize("dcrf,level,mode", [(False, "c4", "soft"), (False, "c3", "hard"), (True, "c5", "soft")])
def test_frame_segmenter_describes_what_it_segments(dcrf, level, mode):
    """7 frames of two non-square sizes in batches of 4 (a short last batch), three expressions: the masks are bit-identical with and
    without describe=, and with ground_truth on at the same time, whose J / F counts are unchanged; the log holds frames x expressions
    entries, each equal to the op-level wrappers' results and within the bound of pivot_ref.  With DenseCRF the descriptor still
    weighs the tap by the head's sigm."""
    model, cfg = TG._tiny_model(4, "f32")
    rng = np.random.default_rng(3)
    frames, exprs = _frames(rng, 7), TG._expressions(rng, cfg.num_steps, cfg.vocab_size)
    if dcrf:
        thr, kw = 0.5, dict(dcrf=True, dcrf_method="lattice", out_size=SG.full_size)
    else:
        sig, _ = TG._host_loop(model, frames, exprs)
        thr = float(np.median(np.stack([s.reshape(-1) for s in sig.values()])))
        kw = dict(threshold=thr)
    plain = list(SG.FrameSegmenter(model, **kw).run(frames, exprs))
    assert len(plain) == 21
    seg = SG.FrameSegmenter(model, describe=level, describe_weights=mode, **kw)
    got = list(seg.run(iter(frames), exprs, seq="vid"))
    assert model.gv_norm == "batch"
    assert [x[:2] for x in got] == [x[:2] for x in plain] and all(np.array_equal(a[2], b[2]) for a, b in zip(got, plain))
    want = _frame_oplevel(model, frames, exprs, SG.DESCRIBE_LEVELS.index(level), mode, thr)
    assert len(want) == 21
    _compare_log(seg.pivots, "vid", want, cfg.vf_h, cfg.vf_w)
    areas = np.concatenate([seg.pivots.areas(("vid", e)) for e in range(3)])
    assert np.all(areas > 0 if mode == "soft" else areas >= 0) and np.all(areas <= cfg.vf_h * cfg.vf_w)
    assert len(seg.pivots.meta()) == 3 and all(0 <= f < 7 for p in seg.pivots.meta().values() for f in p)
    if dcrf:
        return
    # scoring and describing at once: the same masks, the J / F counts of a scored run without describe=, the same log
    gts = {(e, f): np.roll(mk, (1, 2), (0, 1)) for e, f, mk in plain}
    gt = lambda e, f: gts[(e, f)] if f % 2 == 0 else None
    base, both = Recorder(), Recorder()
    list(SG.FrameSegmenter(model, **kw).run(frames, exprs, ground_truth=gt, jf=base, seq="vid"))
    seg2, log2 = SG.FrameSegmenter(model, describe=level, describe_weights=mode, **kw), HU.PivotLog()
    got2 = list(seg2.run(frames, exprs, ground_truth=gt, jf=both, seq="vid", pivots=log2))
    assert seg2.pivots is log2 and all(np.array_equal(a[2], b[2]) for a, b in zip(got2, plain))
    assert sorted(both.counts) == sorted(base.counts) and len(base.counts) == 3 * 4
    assert all(np.array_equal(both.counts[k], base.counts[k]) for k in base.counts)
    _compare_log(log2, "vid", want, cfg.vf_h, cfg.vf_w)


def _clip_oplevel(model, frames, exprs, level, mode, thr):
    """The op-level wrappers on frame f's own tap among its gathered clip and on the head's fetches, every frame's taps taken through
    the backbone in the segmenter's own batches of 5: {(e, f): ...} as _compare_log takes."""
    N, H, W = len(frames), model.H, model.W
    B, own = len(TGC.MD.FRAME_IDX), TGC.MD.FRAME_IDX.index(model.frames // 2)
    taps, want = {}, {}
    with torch.no_grad():
        for s in range(0, N, B):
            ims = frames[s: s + B]
            feed, _ = EV.prepare_images(ims + [ims[0]] * (B - len(ims)), H, W)
            feats = [t.clone() for t in model.features(feed)]
            for j in range(len(ims)):
                taps[s + j] = [t[j] for t in feats]
        for f in range(N):
            gathered = [torch.stack([taps[g][lv] for g in SG.sampled_frames(f, N, model.frames)]) for lv in range(3)]
            for e, (ids, sl) in enumerate(exprs):
                o = model.head_video(gathered, torch.from_numpy(np.ascontiguousarray(ids[None])), torch.full((1,), sl, dtype=torch.int32))
                sigm = o["sigm"].float().reshape(1, H, W)
                tap = gathered[level][own: own + 1]
                desc, area = EV.mask_pool(tap, sigm, mode, thr)
                cnt = EV.level_agree(o["score_c4"], o["score_c5"], SG.AGREE_THRESHOLD)
                ref, _, mag, _ = R.pool(tap.float().cpu().numpy(), sigm.cpu().numpy(), mode, thr)
                want[(e, f)] = (desc.cpu().numpy()[0], area.cpu().numpy()[0], cnt.cpu().numpy()[0], ref[0], mag[0])
    return want


@pytest.mark.parametrize("score,level,mode", [("up", "c4", "soft"), ("up", "c5", "hard"), ("sigm", "c3", "hard")])
def test_clip_segmenter_describes_what_it_segments(score, level, mode):
    """8 frames, three expressions: bit-identical masks with and without describe=, frames x expressions entries, each equal to the
    op-level wrappers on frame f's own tap among the gathered ones and the head's fetches and within the bound of pivot_ref.  "hard"
    weights are sigm >= 0.5 when the run thresholds `up` and sigm >= threshold when it thresholds sigm.  With ground_truth on at the
    same time (every other frame annotated, one expression absent from one of them): the same masks, the J / F counts of a scored run
    without describe=, the same log -- here the heads write the describe tail BEFORE cmpc_mask_jf writes its counts in front of it."""
    model, cfg = TGC._tiny_model("f32")
    rng = np.random.default_rng(4)
    frames = [TGC._frame(rng, *SIZES[(f // 3) % 2], 3 * f) for f in range(8)]
    T = cfg.num_steps
    exprs = TGC._expressions(rng, T, cfg.vocab_size, [1, T // 2, T])
    ups = TGC._driver_loop(model, frames[:2], exprs[:1])
    if score == "up":
        thr, pool_thr = TGC._median_threshold([ups]), 0.5
    else:
        thr = pool_thr = float(np.float32(np.median(np.concatenate([sg.reshape(-1) for _, sg in ups.values()]))))
    kw = dict(score=score, threshold=thr)
    plain = list(SG.ClipSegmenter(model, **kw).run(frames, exprs))
    seg = SG.ClipSegmenter(model, describe=level, describe_weights=mode, **kw)
    got = list(seg.run(iter(frames), exprs, seq="clip"))
    assert len(got) == 24 and [x[:2] for x in got] == [x[:2] for x in plain] and all(np.array_equal(a[2], b[2]) for a, b in zip(got, plain))
    fg = np.mean([mk.mean() / 255 for _, _, mk in plain])
    assert 0.02 < fg < 0.98, fg                                                # mixed masks: the threshold cuts through the maps
    want = _clip_oplevel(model, frames, exprs, SG.DESCRIBE_LEVELS.index(level), mode, pool_thr)
    assert len(want) == 24
    _compare_log(seg.pivots, "clip", want, cfg.vf_h, cfg.vf_w)
    assert seg.stats == {"frames": 8, "backbone_passes": 2, "gathers": 8, "heads": 24}
    if mode == "hard":
        areas = np.concatenate([seg.pivots.areas(("clip", e)) for e in range(3)])
        assert np.all(areas == np.round(areas)) and np.all(areas <= cfg.vf_h * cfg.vf_w)            # counts of positions
        if score == "sigm":                                                    # the median of sigm cuts through the maps: neither none nor all
            assert 0 < areas.sum() < 24 * cfg.vf_h * cfg.vf_w
    # scoring and describing at once
    gts = {(e, f): np.roll(mk, (1, 2), (0, 1)) for e, f, mk in plain}
    gt = lambda e, f: gts[(e, f)] if f % 2 == 0 and not (e == 2 and f == 4) else None
    base, both = Recorder(), Recorder()
    got1 = list(SG.ClipSegmenter(model, **kw).run(frames, exprs, ground_truth=gt, jf=base, seq="clip"))
    seg2, log2 = SG.ClipSegmenter(model, describe=level, describe_weights=mode, **kw), HU.PivotLog()
    got2 = list(seg2.run(frames, exprs, ground_truth=gt, jf=both, seq="clip", pivots=log2))
    assert seg2.pivots is log2 and seg2.jf is both
    for g in (got1, got2):
        assert [x[:2] for x in g] == [x[:2] for x in plain] and all(np.array_equal(a[2], b[2]) for a, b in zip(g, plain))
    assert sorted(both.counts) == sorted(base.counts) and len(base.counts) == 3 * 4 - 1
    assert all(np.array_equal(both.counts[k], base.counts[k]) for k in base.counts)
    assert both.result() == base.result()
    _compare_log(log2, "clip", want, cfg.vf_h, cfg.vf_w)
