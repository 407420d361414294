"""GPU tests of the picture renderers (csrc/ops_vis.hip, visualize.py) against the NumPy restatement tests/vis_ref.py: overlays and
word sheets bit for bit, heat maps bit for bit wherever no device exp() enters and within one index step at <= 1e-3 of the pixels
where one does (the condition tests/test_gpu_eval.py puts on proc_im), and Evaluator(visualize=fn) end to end on the tiny model."""
import importlib

import numpy as np
import pytest
import torch

from tests import util as U
from tests import vis_ref as R

pytestmark = pytest.mark.gpu

HU = importlib.import_module("cmpc-refseg_amd.hostutil")
EV = importlib.import_module("cmpc-refseg_amd.evaluate")
V = importlib.import_module("cmpc-refseg_amd.visualize")
CRF = importlib.import_module("cmpc-refseg_amd.crf")
pkg = importlib.import_module("cmpc-refseg_amd")

DEV = "cuda:0"
SENTINEL = 0xA5
OVERLAY_SIZES = [(1, 1), (7, 1), (5, 3), (33, 47), (48, 64)]


def _frame(rng, h, w, grey=False):
    return rng.integers(0, 256, (h, w) if grey else (h, w, 3), dtype=np.uint8)


def _mask(rng, h, w):
    return rng.choice(np.array([0, 0, 1, 255], np.uint8), (h, w))         # values {0, 1, 255}


def _check_overlay(kind, frames, masks_arg, masks_np):
    sizes = [m.shape for m in masks_np]
    _, nbytes = V.plan_pictures(sizes)
    out = torch.full((nbytes + 64,), SENTINEL, dtype=torch.uint8, device=DEV)
    buf, descs = V.overlays(frames if kind == "pred" else None, masks_arg, kind, DEV, out=out)
    host = buf.cpu().numpy()
    written = np.zeros(host.shape, bool)
    for b, (pic, d) in enumerate(zip(V.unpack_pictures(host, descs), descs)):
        want = R.overlay_pred(frames[b], masks_np[b]) if kind == "pred" else R.overlay_gt(masks_np[b])
        assert pic.shape == want.shape and np.array_equal(pic, want), (kind, b, sizes[b])
        assert d.offset % 16 == 0
        written[d.offset: d.offset + d.h * d.w * 3] = True
    assert (host[~written] == SENTINEL).all()                              # bytes between and behind the samples are not touched


@pytest.mark.parametrize("kind", ["pred", "gt"])
def test_overlay_exact(kind):
    rng = np.random.default_rng(11)
    # mixed sizes and a grey frame in one batch, masks as device tensors holding 0 / 1 / 255
    sizes = OVERLAY_SIZES + [(33, 47)]
    frames = [_frame(rng, h, w) for h, w in OVERLAY_SIZES] + [_frame(rng, 33, 47, grey=True)]
    masks = [_mask(rng, h, w) for h, w in sizes]
    _check_overlay(kind, frames, [torch.from_numpy(m).to(DEV) for m in masks], masks)
    # a batch of 1 (host mask: non-zero = foreground) and a batch of 32 through a packed (buf, descs) pair
    _check_overlay(kind, frames[3:4], masks[3:4], masks[3:4])
    sizes32 = [OVERLAY_SIZES[i % 5] for i in range(32)]
    frames32 = [_frame(rng, h, w, grey=(i % 7 == 3)) for i, (h, w) in enumerate(sizes32)]
    masks32 = [_mask(rng, h, w) for h, w in sizes32]
    descs, nbytes = EV.plan_masks(sizes32, 64, 64)
    packed = np.full(nbytes, 7, np.uint8)
    for m, d in zip(masks32, descs):
        packed[d.offset: d.offset + m.size] = m.reshape(-1)
    _check_overlay(kind, frames32, (torch.from_numpy(packed).to(DEV), descs), masks32)


# ---- heat maps ------------------------------------------------------------------------------------------------------------------------
HEAT_CASES = {(32, 32): [(48, 64), (20, 50), (33, 47), (32, 32), (16, 12), (7, 1)], (24, 40): [(30, 50), (45, 31), (9, 15)]}
SHRINKING = {(16, 12), (7, 1), (9, 15)}                                   # a Gaussian, hence the device's exp(), enters here
FIXED = (0.0, 1.0)


def _smooth(rng, B, H, W):
    y, x = np.mgrid[0:H, 0:W]
    maps = []
    for _ in range(B):
        a, b, p, q = rng.uniform(3, 9), rng.uniform(3, 9), rng.uniform(0, 6), rng.uniform(0, 6)
        maps.append(0.5 + 0.7 * np.sin(y / a + p) * np.cos(x / b + q) + rng.normal(0, 0.02, (H, W)))      # about [-0.25, 1.25]: a fixed (0, 1) clips
    return np.stack(maps).astype(np.float32)


_HEAT = {}


def _heat_case(shape):
    """Maps, and the oracle's (idx, (lo, hi)) per (sigmoid, auto) and sample -- computed once."""
    if shape not in _HEAT:
        sizes = HEAT_CASES[shape]
        raw = _smooth(np.random.default_rng(shape[1]), len(sizes), *shape)
        ref = {}
        for sig in (False, True):
            m = (6 * (raw - 0.5)).astype(np.float32) if sig else raw
            for auto in (False, True):
                ref[sig, auto] = [R.heat(m[b], h, w, sigmoid=sig, vrange=None if auto else FIXED) for b, (h, w) in enumerate(sizes)]
            ref[sig] = m
        _HEAT[shape] = (sizes, ref)
    return _HEAT[shape]


def _run_heat(m, sizes, sig, auto, lut=None, want="both"):
    rng_out = torch.zeros(len(sizes), 2, dtype=torch.float64, device=DEV)
    res = V.heat_maps(torch.from_numpy(m).to(DEV), sizes, sigmoid=sig, vrange=None if auto else FIXED, lut=lut, want=want, range_out=rng_out)
    return res, rng_out.cpu().numpy()


@pytest.mark.parametrize("shape", list(HEAT_CASES))
@pytest.mark.parametrize("sig", [False, True])
@pytest.mark.parametrize("auto", [False, True])
def test_heat_against_reference(shape, sig, auto):
    sizes, ref = _heat_case(shape)
    m = ref[sig]
    ((rgb, rdescs), (idx, idescs)), rng_ = _run_heat(m, sizes, sig, auto)
    idx_h, rgb_h = idx.cpu().numpy(), rgb.cpu().numpy()
    jet = V.jet_lut()
    for b, (got, pic) in enumerate(zip(V.unpack_pictures(idx_h, idescs), V.unpack_pictures(rgb_h, rdescs))):
        want, (lo, hi) = ref[sig, auto][b]
        exact = not sig and sizes[b] not in SHRINKING
        diff = np.abs(got.astype(int) - want.astype(int))
        print(shape, sizes[b], "sigmoid" if sig else "raw", "auto" if auto else "fixed", "max diff", diff.max(), "share", (diff > 0).mean(),
              "range", tuple(rng_[b]), (lo, hi))
        assert got.shape == want.shape == sizes[b]
        if exact:
            assert np.array_equal(got, want), (sizes[b], diff.max(), (diff > 0).mean())
            assert tuple(rng_[b]) == (lo, hi)
        else:
            assert diff.max() <= 1 and (diff > 0).mean() <= 1e-3, (sizes[b], diff.max(), (diff > 0).mean())
            # the range used: the float32 sigmoid is within 2 ulp of NumPy's (values <= 1: 2^-23), and a Gaussian weight within a few
            # float64 ulp, so v moves by at most ~1e-15 |v| through the weights and 2^-23 through the sigmoid
            assert np.allclose(rng_[b], (lo, hi), rtol=0, atol=2.0 ** -23 if sig else 1e-13)
        assert np.array_equal(pic, jet[got])                               # RGB = lut[idx] of the kernel's own index plane


def test_heat_lut_rerun_and_batch_independence():
    sizes, ref = _heat_case((32, 32))
    lut = np.random.default_rng(5).integers(0, 256, (256, 3), dtype=np.uint8)
    for sig, auto in ((False, True), (True, False), (True, True)):
        m = ref[sig]
        ((rgb, rdescs), (idx, idescs)), rng_ = _run_heat(m, sizes, sig, auto, lut=lut)
        idx_h, rgb_h = idx.cpu().numpy(), rgb.cpu().numpy()
        for got, pic in zip(V.unpack_pictures(idx_h, idescs), V.unpack_pictures(rgb_h, rdescs)):
            assert np.array_equal(pic, lut[got])
        ((rgb2, _), (idx2, _)), rng2 = _run_heat(m, sizes, sig, auto, lut=lut)
        planes = [V.unpack_pictures(idx2.cpu().numpy(), idescs), V.unpack_pictures(rgb2.cpu().numpy(), rdescs)]
        for b in range(len(sizes)):                                        # two runs agree bit for bit (written bytes; the gaps are not written)
            assert np.array_equal(planes[0][b], V.unpack_pictures(idx_h, idescs)[b]) and np.array_equal(planes[1][b], V.unpack_pictures(rgb_h, rdescs)[b])
        assert np.array_equal(rng_.view(np.uint64), rng2.view(np.uint64))
        for b in (0, 4, 5):                                                # a sample alone gives what it gave among its batch mates
            (i1, d1), r1 = _run_heat(m[b: b + 1], sizes[b: b + 1], sig, auto, want="index")
            assert np.array_equal(V.unpack_pictures(i1.cpu().numpy(), d1)[0], V.unpack_pictures(idx_h, idescs)[b])
            assert np.array_equal(r1.view(np.uint64), rng_[b: b + 1].view(np.uint64))
    rgb_only, d = V.heat_maps(torch.from_numpy(ref[False][:1]).to(DEV), sizes[:1], want="rgb")
    assert np.array_equal(V.unpack_pictures(rgb_only.cpu().numpy(), d)[0], V.jet_lut()[ref[False, False][0][0]])


# ---- word sheets ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("zoom", [1, 3])
@pytest.mark.parametrize("cols", [1, 5])
@pytest.mark.parametrize("gap", [0, 2])
def test_word_sheets_exact(zoom, cols, gap):
    rng = np.random.default_rng(3)
    gh, gw, ld, nw = 4, 5, 8, (0, 3, 8)
    g = rng.normal(0, 1, (3, gh * gw, ld)).astype(np.float32)
    g[1, :, 1] = 0.375                                                     # a constant panel: hi == lo -> index 0
    g[2, :, 5] = -2.0
    for lut in (V.jet_lut(), rng.integers(0, 256, (256, 3), dtype=np.uint8)):
        sheets = V.word_sheets(torch.from_numpy(g).to(DEV), nw, (gh, gw), zoom=zoom, cols=cols, gap=gap, lut=lut, max_words=8).cpu().numpy()
        assert sheets.shape == (3,) + R.sheet_size(gh, gw, 8, zoom, cols, gap) + (3,)
        for b in range(3):
            assert np.array_equal(sheets[b], R.word_sheet(g[b], nw[b], (gh, gw), 8, zoom, cols, gap, lut)), (b, zoom, cols, gap)
    # max_words defaults to the longest sentence
    assert V.word_sheets(torch.from_numpy(g[:2]).to(DEV), (2, 3), (gh, gw), zoom=zoom, cols=cols, gap=gap).shape[1:3] == R.sheet_size(gh, gw, 3, zoom, cols, gap)


# ---- Evaluator(visualize=fn) ----------------------------------------------------------------------------------------------------------
def _samples(rng, n, T, vocab, sizes):
    out = []
    for i in range(n):
        h, w = sizes[i % len(sizes)]
        L = int(rng.integers(1, T + 1))
        ids = np.zeros(T, np.int32)
        ids[:L] = rng.integers(1, vocab, L)
        y, x = np.mgrid[0:h, 0:w]
        gt = (y - h * rng.uniform(0.2, 0.8)) ** 2 + (x - w * rng.uniform(0.2, 0.8)) ** 2 < (0.3 * min(h, w)) ** 2
        out.append((ids, L, _frame(rng, h, w, grey=(i == 2)), gt))
    return out


@pytest.mark.parametrize("dcrf", [False, True])
def test_evaluator_visualize_hook(dcrf):
    cfg = U.tiny_cfg(B=2)
    model = pkg.LSTM_model(**U.model_kwargs(cfg, "f32", mode="eval"))
    samples = _samples(np.random.default_rng(9), 5, cfg.num_steps, cfg.vocab_size, [(48, 80), (100, 64), (64, 64), (37, 50)])
    kw = dict(dcrf=True, dcrf_method="lattice") if dcrf else {}
    plain = EV.Evaluator(model, **kw)
    seen = []
    hooked = EV.Evaluator(model, visualize=lambda i, pics: seen.append((i, {k: v.copy() for k, v in pics.items()})), **kw)
    for s in samples:
        plain.add(*s)
        hooked.add(*s)
    assert [i for i, _ in seen] == [0, 1]                                  # batch 0 delivered once batch 1 was enqueued; nothing for the queue
    res = hooked.result()
    assert res == plain.result() and np.array_equal(hooked.per_sample(), plain.per_sample())
    assert [i for i, _ in seen] == [0, 1, 2, 3, 4]                         # once each, in order; the pad of the last batch never
    names = {"im", "gt", "pred"} | ({"pred_dcrf"} if dcrf else set())
    B, H, W = model.batch_size, model.H, model.W
    for s0 in range(0, 5, B):
        chunk = samples[s0: s0 + B]
        n = len(chunk)
        pad = chunk + [chunk[0]] * (B - n)
        feed, proc = EV.prepare_images([s[2] for s in pad], H, W)
        out = model.forward(np.stack([s[0] for s in pad]), feed, np.array([s[1] for s in pad], np.int32))
        gts = [s[3] for s in chunk]
        _, masks = EV.mask_iu(out["up"][:n].float(), gts, 1e-9, want_masks=True)
        if dcrf:
            crf_masks = CRF.dense_crf_batch(out["sigm"].float()[:n].reshape(n, H, W), proc[:n], device=model.device, method="lattice")
            _, masks_crf = EV.mask_iu(crf_masks, gts, 0.5, want_masks=True)
        for b, s in enumerate(chunk):
            i, pics = seen[s0 + b]
            assert set(pics) == names and all(p.dtype == np.uint8 and p.shape == s[2].shape[:2] + (3,) for p in pics.values())
            assert np.array_equal(pics["im"], R._rgb(s[2]))
            assert np.array_equal(pics["gt"], R.overlay_gt(s[3]))
            assert np.array_equal(pics["pred"], R.overlay_pred(s[2], masks[b].cpu().numpy()))
            if dcrf:
                assert np.array_equal(pics["pred_dcrf"], R.overlay_pred(s[2], masks_crf[b].cpu().numpy()))
