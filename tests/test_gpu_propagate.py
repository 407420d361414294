"""GPU tests of mask propagation: cmpc_label_propagate against tests/propagate_ref.py's float64 softmax within the derived bound (every
output, f32 / f16 / bf16 taps, two temperatures, edge shapes around the 16-position tile, guarded buffers, bit-identical reruns, items on
their own, strided banks), cmpc_prop_fuse within its bound and exact where it must be, and FrameSegmenter(propagate=) end to end."""
import functools
import importlib

import numpy as np
import pytest
import torch

from tests import propagate_ref as R
from tests import test_gpu_segment as TG
from tests.test_gpu_segment_jf import Recorder

pytestmark = pytest.mark.gpu

HU = importlib.import_module("cmpc-refseg_amd.hostutil")
EV = importlib.import_module("cmpc-refseg_amd.evaluate")
SG = importlib.import_module("cmpc-refseg_amd.segment")
L = importlib.import_module("cmpc-refseg_amd._lib")

GUARD = -1515870811                    # 0xA5A5A5A5 as int32
TDT = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
# (n, h, w, C, radius, nsrc): the smallest call; odd sizes with C no multiple of the MFMA's 32; the whole grid; w one below, at and one
# above the 16-position tile; the largest n with the most sources; one real c4 tap (the target tile stays in LDS for the 16-bit types and
# streams for float32); the channels of a real c5 tap on a small grid of two tiles (the tile streams for every type)
SHAPES = [(1, 1, 1, 8, 0, 1), (3, 3, 5, 24, 1, 2), (2, 7, 9, 40, -1, 1), (2, 4, 15, 64, 2, 2), (2, 4, 16, 64, 2, 2), (2, 4, 17, 64, 2, 2),
          (32, 4, 4, 16, 1, 4), (2, 40, 40, 1024, 12, 2), (2, 3, 18, 2048, 1, 2)]
TEMPS = [0.07, 1.0]
_id = lambda s: "x".join(str(v) for v in s)


@functools.lru_cache(maxsize=None)
def _case(shape, dtype):
    """Inputs on the device and the float64 references at both temperatures, made once and never changed."""
    feat, labels, items = R.case(shape, dtype)
    radius = shape[4]
    refs = {t: R.propagate(feat, labels, items, radius, t) for t in TEMPS}
    return torch.from_numpy(feat).to(TDT[dtype]).cuda(), torch.from_numpy(labels).cuda(), items, refs


def _guarded(feat, labels, items, radius, temperature, want_peak=True, frames=None):
    """cmpc_label_propagate called directly with out, peak and the workspace inside one guard-filled buffer; checks the guard band and
    that nothing past the workspace's stated size is written.  Returns (out, peak) as host arrays."""
    frames = feat.shape[0] if frames is None else frames
    h, w, C = (int(v) for v in feat.shape[1:])
    n = len(items)
    need = EV.prop_workspace(n, h, w)
    up4 = lambda v: -(-v // 4) * 4
    o_out = 16
    o_peak = up4(o_out + n * h * w + 16)
    o_ws = up4(o_peak + n * h * w + 16)
    total = o_ws + need // 4 + 16
    buf = torch.full((total,), GUARD, dtype=torch.int32, device="cuda")
    base = buf.data_ptr()
    assert base % 16 == 0
    stride = feat.stride(0) if feat.shape[0] > 1 else h * w * C
    its = EV.prop_items(items)
    L.call("cmpc_label_propagate", EV._POOL_DT[feat.dtype], feat.data_ptr(), stride, frames, labels.data_ptr(), labels.shape[0],
           (L.PropItem * n)(*its), n, h, w, C, radius, float(temperature), base + 4 * o_out, base + 4 * o_peak if want_peak else None,
           base + 4 * o_ws, need, torch.cuda.current_stream().cuda_stream)
    host = buf.cpu().numpy()
    inside = np.zeros(total, bool)
    inside[o_out: o_out + n * h * w] = inside[o_ws: o_ws + need // 4] = True
    if want_peak:
        inside[o_peak: o_peak + n * h * w] = True
    assert np.all(host[~inside] == GUARD), "words outside out, peak and the workspace were written"
    return (host[o_out: o_out + n * h * w].view(np.float32).reshape(n, h, w).copy(),
            host[o_peak: o_peak + n * h * w].view(np.float32).reshape(n, h, w).copy())


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("temperature", TEMPS)
@pytest.mark.parametrize("dtype", ["f32", "f16", "bf16"])
@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_label_propagate_within_the_bound(shape, dtype, temperature):
    """Every output: |out - ref| <= bound(C, candidates, temperature, 1) and |peak - ref| <= delta(C) (tests/propagate_ref.py); the
    guard band is intact; a second call, the call without peak and the Python wrapper give the same bits; item k alone gives the bits
    it has within the batch."""
    n, h, w, C, radius, nsrc = shape
    feat, labels, items, refs = _case(shape, dtype)
    ref, ref_peak, cnt = refs[temperature]
    out, peak = _guarded(feat, labels, items, radius, temperature)
    lim = R.bound(C, cnt, temperature, 1.0)
    err, perr = np.abs(out.astype(np.float64) - ref), np.abs(peak.astype(np.float64) - ref_peak)
    print("%s %s T=%g: worst error / bound %.3f (out), %.3f (peak)" % (shape, dtype, temperature, float((err / lim).max()),
                                                                     float(perr.max() / R.delta(C))))
    assert np.all(np.isfinite(out)) and np.all(err <= lim), (int((err > lim).sum()), float((err / lim).max()))
    assert np.all(perr <= R.delta(C)), float(perr.max() / R.delta(C))
    o2, p2 = _guarded(feat, labels, items, radius, temperature)
    assert np.array_equal(_bits(out), _bits(o2)) and np.array_equal(_bits(peak), _bits(p2))
    o3, _ = _guarded(feat, labels, items, radius, temperature, want_peak=False)
    assert np.array_equal(_bits(out), _bits(o3))
    o4, p4 = EV.label_propagate(feat, labels, items, radius, temperature, want_peak=True)
    assert o4.dtype == torch.float32 and tuple(o4.shape) == (n, h, w)
    assert np.array_equal(_bits(o4.cpu().numpy()), _bits(out)) and np.array_equal(_bits(p4.cpu().numpy()), _bits(peak))
    for k in sorted({0, n // 2, n - 1}):
        o5, p5 = _guarded(feat, labels, items[k: k + 1], radius, temperature)
        assert np.array_equal(_bits(o5[0]), _bits(out[k])) and np.array_equal(_bits(p5[0]), _bits(peak[k])), k


@pytest.mark.parametrize("temperature", TEMPS)
@pytest.mark.parametrize("dtype", ["f32", "f16", "bf16"])
@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_label_propagate_strided_bank(shape, dtype, temperature):
    """Every case: a bank that is every other frame of a larger one gives the bits of a contiguous copy, through the wrapper and
    through the entry point in guarded buffers (the real tap has the large frame offsets); more items than MAX_BATCH go in chunks."""
    n, h, w, C, radius, nsrc = shape
    feat, labels, items, _ = _case(shape, dtype)
    want = EV.label_propagate(feat, labels, items, radius, temperature)
    big = torch.zeros((2 * feat.shape[0],) + tuple(feat.shape[1:]), dtype=feat.dtype, device="cuda")
    big[::2] = feat
    big[1::2] = 7.0
    sel = big[::2]
    assert not sel.is_contiguous()
    assert torch.equal(EV.label_propagate(sel, labels, items, radius, temperature), want)
    o, _ = _guarded(sel, labels, items, radius, temperature)
    assert np.array_equal(_bits(o), _bits(want.cpu().numpy()))
    many = items * (-(-(EV.MAX_BATCH + 1) // n))                                 # just above MAX_BATCH items: two calls
    assert EV.MAX_BATCH < len(many) <= 2 * EV.MAX_BATCH
    om = EV.label_propagate(sel, labels, many, radius, temperature)
    assert torch.equal(om[-n:], want) and torch.equal(om[:n], want)


@pytest.mark.parametrize("dtype", ["f32", "f16", "bf16"])
def test_radius_zero_returns_the_label(dtype):
    """radius = 0 with one source: the only candidate is p = q, its weight is exp(0) / exp(0): out equals that source's label exactly,
    at any temperature -- with labels that are no 0 / 1 too."""
    rng = np.random.default_rng(5)
    feat = torch.from_numpy(rng.normal(0, 1, (3, 5, 19, 24)).astype(np.float32)).to(TDT[dtype]).cuda()
    feat[1, 2, 3] = 0
    labels = torch.from_numpy(rng.normal(0, 3, (2, 5, 19)).astype(np.float32)).cuda()
    items = [(0, [(1, 1)]), (2, [(2, 0)])]
    for t in (0.01, 0.07, 1.0, 50.0):
        out, peak = EV.label_propagate(feat, labels, items, 0, t, want_peak=True)
        assert torch.equal(out[0], labels[1]) and torch.equal(out[1], labels[0]), t
    assert float((peak[1] - 1).abs().max()) <= R.delta(24)                      # a frame against itself: cosine 1


FUSE_SHAPES = [(2, 1, 1, 1, 1), (3, 5, 7, 40, 56), (2, 40, 40, 320, 320)]


@pytest.mark.parametrize("shape", FUSE_SHAPES, ids=_id)
def test_prop_fuse(shape):
    """Within fuse_bound at alpha 0.5 and 0.3; alpha = 0 returns own bit for bit; alpha = 1 at positions (k H / h, k W / w) equals
    prop exactly; only `fused` is written."""
    n, h, w, H, W = shape
    rng = np.random.default_rng([n, h, w])
    own = rng.uniform(0, 1, (n, H, W)).astype(np.float32)
    prop = rng.uniform(0, 1, (n, h, w)).astype(np.float32)
    own[0, 0, 0] = -0.0
    od, pd = torch.from_numpy(own).cuda(), torch.from_numpy(prop).cuda()
    for alpha in (0.5, 0.3):
        buf = torch.full((n * H * W + 32,), GUARD, dtype=torch.int32, device="cuda")
        L.call("cmpc_prop_fuse", od.data_ptr(), pd.data_ptr(), n, h, w, H, W, alpha, buf.data_ptr() + 64, torch.cuda.current_stream().cuda_stream)
        host = buf.cpu().numpy()
        assert np.all(host[:16] == GUARD) and np.all(host[16 + n * H * W:] == GUARD)
        got = host[16: 16 + n * H * W].view(np.float32).reshape(n, H, W)
        ref, lim = R.fuse(own, prop, alpha)
        err = np.abs(got.astype(np.float64) - ref)
        print("%s alpha=%g: worst error / bound %.3f" % (shape, alpha, float((err / lim).max())))
        assert np.all(err <= lim)
        assert np.array_equal(_bits(EV.prop_fuse(od, pd, alpha).cpu().numpy()), _bits(got))
    assert np.array_equal(_bits(EV.prop_fuse(od, pd, 0.0).cpu().numpy()), _bits(own))
    one = EV.prop_fuse(od, pd, 1.0).cpu().numpy()
    assert np.array_equal(_bits(one[:, :: H // h, :: W // w]), _bits(prop))


@pytest.mark.parametrize("seed", R.MASK_SEEDS)
def test_mask_case_against_the_float64_chain(seed):
    """evaluate.label_propagate -> prop_fuse -> masks_out on tests/propagate_ref.mask_case(seed) -- the seeded inputs on which
    tests/test_propagate_host.py asserts the excluded share with the float64 reference alone -- against R.mask_reference: the masks
    agree everywhere except where the reference's fused value lies within the bound of the threshold, at most 1 % of a mask."""
    s = R.MASK_SHAPE
    feat, sigm = R.mask_case(seed)
    F, H, W = s["frames"], s["H"], s["W"]
    plan = HU.propagation_plan(range(F), [0, 4], 2)
    res = R.mask_reference(feat, sigm, plan, s["radius"], s["temperature"], s["alpha"], s["threshold"])
    bank = torch.from_numpy(feat).half().cuda()
    assert np.array_equal(bank.float().cpu().numpy(), feat)                      # the taps are f16 values
    sg = torch.from_numpy(sigm).cuda()
    labels = sg[:, :: H // s["h"], :: W // s["w"]].contiguous()
    frames = sorted(plan)
    prop = EV.label_propagate(bank, labels, [(f, [(p, p) for p in plan[f]]) for f in frames], s["radius"], s["temperature"])
    fused = EV.prop_fuse(sg[frames].contiguous(), prop, s["alpha"])
    buf, d = EV.masks_out(fused, [(H, W)] * len(frames), s["threshold"], value=1)
    worst = 0.0
    for f, mk in zip(frames, EV.unpack_masks(buf, d)):
        ref, lim, mask, unsure = res[f]
        got = mk.cpu().numpy() > 0
        worst = max(worst, float(unsure.mean()))
        assert unsure.mean() <= 0.01, (f, float(unsure.mean()))
        assert np.array_equal(got[~unsure], mask[~unsure]), (f, int((got != mask)[~unsure].sum()))
        assert 0.05 < got.mean() < 0.95
    print("seed %d: largest share of a mask within the bound of the threshold %.4f %%" % (seed, 100 * worst))


# ---- FrameSegmenter(propagate=) ----------------------------------------------------------------------------------------------------------
PIVOTS = {0: [2, 8], 1: [0, 5, 10], 2: [4]}            # per expression; with num_propagate = 2 expression 2 leaves frames 0, 1, 7 .. 10 out
RADIUS, TEMP = 3, 0.07
N_FRAMES = 11


@functools.lru_cache(maxsize=None)
def _video_case():
    """The tiny model of tests/test_gpu_segment.py, 11 frames of three sizes in batches of 4, three expressions; the taps and sigm of the
    same padded batches through the model's own calls (mode "sample"), the threshold (the median of sigm) and run()'s plain masks."""
    model, cfg = TG._tiny_model(4, "f32")
    rng = np.random.default_rng(21)
    frames, exprs = TG._video(rng, N_FRAMES), TG._expressions(rng, cfg.num_steps, cfg.vocab_size)
    B, H, W = model.batch_size, model.H, model.W
    taps, sigm = {}, {}
    prev = model.gv_norm
    model.set_gv_norm("sample")
    with torch.no_grad():
        for idx in SG.plan_batches(len(frames), B):
            feed, _ = EV.prepare_images([frames[i] for i in idx], H, W)
            feats, ev = model.features_async(feed)
            n = len(set(idx))
            for e, (ids, sl) in enumerate(exprs):
                o = model.head(feats, torch.from_numpy(np.repeat(ids[None], B, 0)), torch.full((B,), sl, dtype=torch.int32), after=ev, im=feed)
                s = o["sigm"].float().reshape(B, H, W)
                for b in range(n):
                    sigm[(e, idx[b])] = s[b].clone()
                    if e == 0:
                        taps[idx[b]] = [t[b].clone() for t in feats]
    model.set_gv_norm(prev)
    thr = float(np.median(torch.stack([sigm[k] for k in sorted(sigm)]).cpu().numpy()))
    plain = {(e, f): mk for e, f, mk in SG.FrameSegmenter(model, threshold=thr).run(frames, exprs)}
    assert len(plain) == 3 * N_FRAMES
    return model, cfg, frames, exprs, taps, sigm, thr, plain


def _plans():
    return {e: HU.propagation_plan(range(N_FRAMES), PIVOTS[e], 2, L.PROP_MAX_SOURCES) for e in PIVOTS}


def _segmenter(alpha, level="c4", **kw):
    model, cfg, frames, exprs, taps, sigm, thr, plain = _video_case()
    seg = SG.FrameSegmenter(model, threshold=thr, propagate={"level": level, "radius": RADIUS, "temperature": TEMP, "alpha": alpha}, **kw)
    return seg


def test_run_is_unchanged_and_banks_hold_the_models_own_values():
    """run()'s masks and their order are bit-identical with and without propagate=; afterwards the banks hold, bit for bit, the taps of
    the model's own backbone pass, the head's float32 sigm and its point samples."""
    model, cfg, frames, exprs, taps, sigm, thr, plain = _video_case()
    base = list(SG.FrameSegmenter(model, threshold=thr).run(frames, exprs))
    for level in ("c4", "c5"):
        seg = _segmenter(0.5, level)
        got = list(seg.run(iter(frames), exprs))               # an iterator: read into a list first
        assert [x[:2] for x in got] == [x[:2] for x in base] and all(np.array_equal(a[2], b[2]) for a, b in zip(got, base))
        st, lv = seg.stage, SG.DESCRIBE_LEVELS.index(level)
        fy, fx = model.H // cfg.vf_h, model.W // cfg.vf_w
        for f in range(N_FRAMES):
            assert torch.equal(st.tap_bank[f], taps[f][lv]), f
            for e in range(3):
                r = e * N_FRAMES + f
                assert torch.equal(st.sigm_bank[r], sigm[(e, f)]) and torch.equal(st.label_bank[r], sigm[(e, f)][::fy, ::fx]), (e, f)
    assert model.gv_norm == "batch"


def test_alpha_zero_gives_runs_masks_for_the_plans_frames():
    """alpha = 0: the fused map is the frame's own sigm bit for bit, so propagate()'s masks are run()'s; the yielded (e, f), in order,
    are propagation_plan's."""
    model, cfg, frames, exprs, taps, sigm, thr, plain = _video_case()
    seg = _segmenter(0.0)
    assert len(list(seg.run(frames, exprs))) == 3 * N_FRAMES
    got = list(seg.propagate(PIVOTS))
    plans = _plans()
    assert [x[:2] for x in got] == [(e, f) for e in range(3) for f in sorted(plans[e])]
    assert len(got) == 8 + 8 + 4
    for e, f, mk in got:
        assert mk.dtype == np.uint8 and np.array_equal(mk, plain[(e, f)]), (e, f)


def _oplevel(seg, e, fr, srcs, alpha, sizes, thr):
    """evaluate.label_propagate, prop_fuse and masks_out on the taps and sigm of the model's own calls."""
    model, cfg, frames, exprs, taps, sigm, _, _ = _video_case()
    lv = SG.DESCRIBE_LEVELS.index(seg.prop.level)
    fy, fx = model.H // cfg.vf_h, model.W // cfg.vf_w
    bank = torch.stack([taps[f][lv] for f in range(N_FRAMES)])
    labels = torch.stack([sigm[(e, f)][::fy, ::fx] for f in range(N_FRAMES)]).contiguous()
    prop = EV.label_propagate(bank, labels, [(f, [(p, p) for p in s]) for f, s in zip(fr, srcs)], RADIUS, TEMP)
    fused = EV.prop_fuse(torch.stack([sigm[(e, f)] for f in fr]), prop, alpha)
    buf, d = EV.masks_out(fused, sizes, thr, value=255)
    return [m.cpu().numpy() for m in EV.unpack_masks(buf, d)], fused


def test_propagated_masks_equal_the_oplevel_chain():
    """alpha = 0.5: every yielded mask equals label_propagate -> prop_fuse -> masks_out on the taps and sigm of the same batches; a
    PivotLog gives the same as the dict of its pivots; a second propagate() gives the same masks."""
    model, cfg, frames, exprs, taps, sigm, thr, plain = _video_case()
    seg = _segmenter(0.5, describe="c4")
    list(seg.run(frames, exprs, seq="vid"))
    piv = {e: seg.pivots.pivots(("vid", e), 2) for e in range(3)}
    got = list(seg.propagate(seg.pivots))
    again = list(seg.propagate(piv, seq="other"))
    assert [x[:2] for x in got] == [x[:2] for x in again] and all(np.array_equal(a[2], b[2]) for a, b in zip(got, again))
    got = {(e, f): mk for e, f, mk in got}
    changed = 0
    for e in range(3):
        plan = HU.propagation_plan(range(N_FRAMES), piv[e], 2, 4)
        assert sorted(f for ee, f in got if ee == e) == sorted(plan) and sorted(list(plan) + piv[e]) == list(range(N_FRAMES))
        todo = sorted(plan)
        for s in range(0, len(todo), model.batch_size):
            fr = todo[s: s + model.batch_size]
            want, _ = _oplevel(seg, e, fr, [plan[f] for f in fr], 0.5, [SG.half_size(*frames[f].shape[:2]) for f in fr], thr)
            for f, w in zip(fr, want):
                assert np.array_equal(got[(e, f)], w), (e, f)
                changed += int((got[(e, f)] != plain[(e, f)]).sum())
    print("pixels that propagation changed: %d" % changed)
    assert changed > 0                                         # the threshold cuts through the maps: fusing moves some pixels


def test_propagated_masks_against_the_float64_chain():
    """At the map's own size (out_size -> (H, W): the resampling is the identity) the masks agree with tests/propagate_ref.py's float64
    chain on the banked taps and sigm everywhere except where its fused value lies within the bound of the threshold: at most 1 % of
    a mask's pixels.  These inputs (the tiny model's own taps and sigm, the threshold at sigm's median) exist only on the device, so
    the cap is asserted here; the host test asserts it ahead of any GPU run for test_mask_case_against_the_float64_chain's inputs."""
    model, cfg, frames, exprs, taps, sigm, thr, plain = _video_case()
    seg = _segmenter(0.5, out_size=lambda h, w: (model.H, model.W))
    list(seg.run(frames, exprs))
    got = {(e, f): mk for e, f, mk in seg.propagate(PIVOTS)}
    feat = seg.stage.tap_bank[:N_FRAMES].float().cpu().numpy()
    worst = 0.0
    for e, plan in _plans().items():
        sg = seg.stage.sigm_bank[e * N_FRAMES: (e + 1) * N_FRAMES].cpu().numpy()
        res = R.mask_reference(feat, sg, plan, RADIUS, TEMP, 0.5, np.float32(thr))
        assert sorted(res) == sorted(f for ee, f in got if ee == e)
        for f, (ref, lim, mask, unsure) in res.items():
            worst = max(worst, float(unsure.mean()))
            assert unsure.mean() <= 0.01, (e, f, float(unsure.mean()))
            assert np.array_equal((got[(e, f)] > 0)[~unsure], mask[~unsure]), (e, f, int(((got[(e, f)] > 0) != mask)[~unsure].sum()))
    print("largest share of a mask within the bound of the threshold: %.4f %%" % (100 * worst))


def test_clean_and_ground_truth_on_propagated_masks():
    """clean= and ground_truth=: the yielded masks are evaluate.mask_clean of the masks an uncleaned propagate() yields, the statistics
    are that call's, and the J / F counts are evaluate.mask_jf's on the yielded masks."""
    model, cfg, frames, exprs, taps, sigm, thr, plain = _video_case()
    raw_seg = _segmenter(0.5)
    list(raw_seg.run(frames, exprs))
    raw = {(e, f): mk for e, f, mk in raw_seg.propagate(PIVOTS)}
    gts = {k: np.roll(mk, (1, 2), (0, 1)) for k, mk in raw.items()}
    gt = lambda e, f: gts[(e, f)] if f % 2 == 1 else None
    seg = _segmenter(0.5, clean={"keep": 1, "min_area": 3})
    rec = Recorder()
    list(seg.run(frames, exprs, ground_truth=lambda e, f: None, seq="v"))
    got = list(seg.propagate(PIVOTS, ground_truth=gt, jf=rec))
    assert seg.prop_jf is rec and [x[:2] for x in got] == sorted(raw)
    keys = [x[:2] for x in got]
    cleaned, stats = EV.mask_clean([raw[k] for k in keys], keep=1, min_area=3)
    for (e, f, mk), want, st in zip(got, cleaned, stats):
        assert np.array_equal(mk, want), (e, f)
        assert seg.prop_cleaned.seqs[("v", e)][f] == tuple(int(v) for v in st), (e, f)
    scored = [(e, f, mk) for e, f, mk in got if f % 2 == 1]
    assert sorted(rec.counts) == sorted((("v", e), f) for e, f, _ in scored) and len(scored) > 0
    counts = EV.mask_jf([mk for _, _, mk in scored], [gts[(e, f)] for e, f, _ in scored])
    for (e, f, _), c in zip(scored, counts):
        assert np.array_equal(rec.counts[(("v", e), f)], c), (e, f)


def test_oversize_video_dcrf_and_order_of_calls():
    model, cfg, frames, exprs, taps, sigm, thr, plain = _video_case()
    for opt in ({"bank": N_FRAMES - 1}, {"results": 3 * N_FRAMES - 1}):
        seg = SG.FrameSegmenter(model, threshold=thr, propagate=opt)
        with pytest.raises(ValueError, match="exceed the banks"):
            next(seg.run(iter(frames), exprs))
    assert len(list(SG.FrameSegmenter(model, threshold=thr, propagate={"bank": N_FRAMES, "results": 3 * N_FRAMES}).run(frames, exprs))) == 3 * N_FRAMES
    with pytest.raises(ValueError, match="dcrf"):
        SG.FrameSegmenter(model, dcrf=True, propagate={})
    seg = _segmenter(0.5)
    with pytest.raises(RuntimeError, match="propagate="):
        next(seg.propagate(PIVOTS))
    with pytest.raises(RuntimeError, match="propagate="):
        next(SG.FrameSegmenter(model).propagate(PIVOTS))
    list(seg.run(frames, exprs))
    with pytest.raises(ValueError, match="pivot 11"):
        next(seg.propagate({0: [11], 1: [0], 2: [0]}))
    with pytest.raises(ValueError, match="no pivots for expression 2"):
        next(seg.propagate({0: [1], 1: [0]}))
