"""GPU tests of the video model's prediction path over whole videos: cmpc_taps_copy (exact, guarded), the backbone's independence of the
batch position (the precondition of caching taps per frame), and segment.ClipSegmenter end to end against the literal driver loop --
for every (frame, expression) prepare_images on the 16 frames of clip_window(f), model.forward_video on front-padded words, then
resize_and_crop(up >= thr) > 0 at the frame's size -- with no allowance."""
import ctypes
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import util as U
from oracle import cmpc_torch as O
from oracle import cmpc_video_torch as VD

pytestmark = pytest.mark.gpu

HU = importlib.import_module("cmpc-refseg_amd.hostutil")
EV = importlib.import_module("cmpc-refseg_amd.evaluate")
CRF = importlib.import_module("cmpc-refseg_amd.crf")
MD = importlib.import_module("cmpc-refseg_amd.model")
SG = importlib.import_module("cmpc-refseg_amd.segment")
L = importlib.import_module("cmpc-refseg_amd._lib")
NAME = "CMPC_video_mm_tgraph_allvec"


# ---- 1. the kernel ---------------------------------------------------------------------------------------------------------------------
GUARD = 0xA5


def _taps_copy(dst, src, nbytes, di, si, dcap, scap):
    n, lv = len(di), len(dst)
    L.call("cmpc_taps_copy", lv, (ctypes.c_void_p * lv)(*[t.data_ptr() for t in dst]), (ctypes.c_void_p * lv)(*[t.data_ptr() for t in src]),
           (ctypes.c_int64 * lv)(*nbytes), n, (ctypes.c_int * n)(*di), (ctypes.c_int * n)(*si), dcap, scap,
           torch.cuda.current_stream().cuda_stream)


def _check_copy(nbytes, di, si, dcap, scap, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    src = [torch.randint(0, 256, (scap, b), dtype=torch.uint8, device="cuda", generator=g) for b in nbytes]
    dst = [torch.full((dcap, b), GUARD, dtype=torch.uint8, device="cuda") for b in nbytes]
    _taps_copy(dst, src, nbytes, di, si, dcap, scap)
    torch.cuda.synchronize()
    for l, b in enumerate(nbytes):
        want = torch.full((dcap, b), GUARD, dtype=torch.uint8, device="cuda")
        for d, s in zip(di, si):
            want[d] = src[l][s]
        assert torch.equal(dst[l], want), (nbytes, di, si, l, int((dst[l] != want).sum()))      # the blocks, and the guard everywhere else


@pytest.mark.parametrize("n", [1, 5, 8])
def test_taps_copy_exact_and_guarded(n):
    """Three levels of 16, 8*8*72*2 and 8*8*256*4 bytes per frame: a gather with repeated source indices into 0..n-1, a scatter from
    0..n-1 to scattered destinations, and both at once; every destination block equals its source, every other byte keeps the guard."""
    nbytes = [16, 8 * 8 * 72 * 2, 8 * 8 * 256 * 4]
    rng = np.random.default_rng(n)
    si = [int(x) for x in rng.integers(0, 11, n)]
    if n > 1:
        si[-1] = si[0]                                                     # a clamped window repeats frames
    _check_copy(nbytes, list(range(n)), si, 8, 11, 1)                     # gather: ring -> contiguous
    di = [int(x) for x in rng.permutation(13)[:n]]
    _check_copy(nbytes, di, list(range(n)), 13, 8, 2)                     # scatter: contiguous -> ring slots
    _check_copy(nbytes, di[::-1], si, 13, 11, 3)
    for lv in (1, 2):                                                      # fewer levels
        _check_copy(nbytes[3 - lv:], di, si, 13, 11, 4)


def test_taps_copy_strided_path_and_ragged_tail():
    """Blocks large enough that the grid is capped and a workgroup strides over its block (more than 4096 x 16 KiB in all), with a size
    that is no multiple of a workgroup's 16 KiB: the tail chunks are copied, nothing past them is."""
    _check_copy([12 * (1 << 20) + 4096 + 16, 16 * 1025], [6, 0, 3, 1, 7, 4, 2, 5], [1, 1, 0, 2, 3, 3, 1, 0], 9, 4, 5)


# ---- the tiny video model and the driver loop ---------------------------------------------------------------------------------------------
def _frame(rng, h, w, phase):
    y, x = np.mgrid[0:h, 0:w]
    base = 127 + 100 * np.sin((x + phase) / 13.0)[..., None] * np.cos(y / 17.0)[..., None] * np.array([1.0, 0.7, -0.5])
    return np.clip(base + rng.normal(0, 25, (h, w, 3)), 0, 255).astype(np.uint8)


def _video(rng, n, h, w):
    return [_frame(rng, h, w, 3 * k) for k in range(n)]


def _tiny_model(dtype="f32"):
    cfg = VD.tiny_cfg()
    hp, bp = VD.init_head_params(cfg), O.init_backbone_params(cfg)
    g = torch.Generator().manual_seed(3)
    for k in hp:
        if k.endswith(("biases", "beta")):
            hp[k] = (torch.randn(hp[k].shape, generator=g) * 0.05).float()
    m = U.pkg().get_segmentation_model(NAME, head_params=hp, backbone_params=bp, frames=cfg.frames, **U.model_kwargs(cfg, dtype, "eval"))
    return m, cfg


def _expressions(rng, T, vocab, lengths):
    """(ids, length) per expression: END-padded for ClipSegmenter; _front() gives the driver's feeds."""
    out = []
    for n in lengths:
        ids = np.zeros(T, np.int32)
        ids[:n] = rng.integers(1, vocab, n)
        out.append((ids, n))
    return out


def _front(ids, n):
    T = ids.shape[0]
    w = np.zeros((1, T), np.int64)
    w[0, T - n:] = ids[:n]
    return w, np.array([[T - n]], np.int32)


def _driver_loop(model, frames, exprs, want_proc=False):
    """trainval_video.py:186-226 for every frame of the video: {(e, f): (up, sigm)} as float32 [H, W] host arrays (and frame f's proc_im)."""
    H, W, N = model.H, model.W, len(frames)
    out, procs = {}, {}
    for f in range(N):
        clip, proc = EV.prepare_images([frames[i] for i in SG.clip_window(f, N, model.frames)], H, W)
        if want_proc:
            procs[f] = proc[model.frames // 2].clone()
        for e, (ids, n) in enumerate(exprs):
            words, vi = _front(ids, n)
            o = model.forward_video(words, None, vi, clip[None])
            out[(e, f)] = (o["up"].float().reshape(H, W).cpu().numpy(), o["sigm"].float().reshape(H, W).cpu().numpy())
    return (out, procs) if want_proc else out


def _ref_masks(ups, frames, thr):
    ref = {}
    for (e, f), (up, _) in ups.items():
        h, w = frames[f].shape[:2]
        ref[(e, f)] = (HU.resize_and_crop((up >= np.float32(thr)).astype(np.float32), h, w) > 0).astype(np.uint8) * 255
    return ref


def _median_threshold(ups_list):
    return float(np.float32(np.median(np.concatenate([u.reshape(-1) for ups in ups_list for u, _ in ups.values()]))))


def _run(seg, frames, exprs):
    return [(e, f, mk) for e, f, mk in seg.run(iter(frames), exprs)]


def _assert_exact(got, ref, N, E, tag):
    assert [(e, f) for e, f, _ in got] == [(e, f) for f in range(N) for e in range(E)], tag
    for e, f, mk in got:
        assert mk.dtype == np.uint8 and mk.shape == ref[(e, f)].shape, (tag, e, f)
        assert np.array_equal(mk, ref[(e, f)]), (tag, e, f, int((mk != ref[(e, f)]).sum()))


@pytest.fixture(scope="module")
def tiny():
    """The tiny f32 model, three videos of 23, 7 and 1 frames (one size each), 3 expressions of lengths 1, T // 2 and T, and the driver
    loop's results on them -- computed once, shared, left unchanged."""
    model, cfg = _tiny_model("f32")
    rng = np.random.default_rng(21)
    T = cfg.num_steps
    videos = [_video(rng, n, h, w) for n, (h, w) in zip((23, 7, 1), [(48, 80), (100, 64), (37, 50)])]
    exprs = _expressions(rng, T, cfg.vocab_size, [1, T // 2, T])
    ups = [_driver_loop(model, v, exprs) for v in videos]
    thr = _median_threshold(ups)
    refs = [_ref_masks(u, v, thr) for u, v in zip(ups, videos)]
    for r in refs:
        for a in r.values():
            a.setflags(write=False)
    return dict(model=model, cfg=cfg, videos=videos, exprs=exprs, ups=ups, thr=thr, refs=refs)


# ---- 2. the precondition ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_taps_do_not_depend_on_batch_position(dtype):
    """model.features on [a, b, c, d, e] and on [c, a, a, e, b]: every frame's taps are bit-identical wherever it sits and whatever
    shares its batch -- what allows a frame's taps to be computed once and reused by every clip that samples it."""
    model, cfg = _tiny_model(dtype)
    g = torch.Generator().manual_seed(5)
    x = (torch.rand(5, cfg.H, cfg.W, 3, generator=g) * 255 - 120).cuda()
    perm = [2, 0, 0, 4, 1]
    with torch.no_grad():
        a = [t.clone() for t in model.features(x)]
        b = [t.clone() for t in model.features(x[perm].contiguous())]
    torch.cuda.synchronize()
    for lv, (ta, tb) in enumerate(zip(a, b)):
        assert ta.shape[0] == 5 and ta.dtype == MD.tdt(model.dt)
        for j, p in enumerate(perm):
            assert torch.equal(tb[j], ta[p]), (dtype, lv, j, p)


# ---- 3. end to end, tiny f32 --------------------------------------------------------------------------------------------------------------
def test_clip_segmenter_end_to_end_tiny(tiny):
    model, exprs, thr = tiny["model"], tiny["exprs"], tiny["thr"]
    fg = np.mean([r.mean() / 255 for ref in tiny["refs"] for r in ref.values()])
    print("threshold %.6g, foreground share of the reference masks %.3f" % (thr, fg))
    assert 0.05 < fg < 0.95
    E = len(exprs)
    base = SG.ClipSegmenter(model, threshold=thr)
    for frames, ref in zip(tiny["videos"], tiny["refs"]):
        N = len(frames)
        got = _run(base, frames, exprs)
        _assert_exact(got, ref, N, E, ("default", N))
        assert base.stats == {"frames": N, "backbone_passes": -(-N // 5), "gathers": N, "heads": N * E}
        for e, f, mk in got:
            assert set(np.unique(mk)) <= {0, 255}
    frames, ref = tiny["videos"][0], tiny["refs"][0]
    N = len(frames)
    for kw in (dict(ring=SG.min_ring(16, SG.CLIP_LOOKAHEAD)), dict(ring=32), dict(depth=1), dict(depth=3),
               dict(lookahead=0, ring=SG.min_ring(16, 0)), dict(lookahead=2, ring=SG.min_ring(16, 2))):
        _assert_exact(_run(SG.ClipSegmenter(model, threshold=thr, **kw), frames, exprs), ref, N, E, kw)
    # one object, run again (its ring, events and pinned slots are reused), and views instead of copies
    _assert_exact(_run(base, frames, exprs), ref, N, E, "second run")
    seg = SG.ClipSegmenter(model, threshold=thr, copy=False, value=1)
    for _ in range(2):
        n = 0
        for e, f, mk in seg.run(frames, exprs):
            assert np.array_equal(mk * 255, ref[(e, f)]), (e, f)
            n += 1
        assert n == N * E
    with pytest.raises(ValueError, match="video"):
        SG.FrameSegmenter(model)


# ---- 4. config 5 at full size --------------------------------------------------------------------------------------------------------------
def test_clip_segmenter_config5_full_size():
    """320 x 320, L = 20, f16, 12 frames of 360 x 640 (fewer than a window: every clamp path), 2 expressions: exact against the driver loop."""
    model = U.pkg().get_segmentation_model(NAME, mode="eval", batch_size=1, num_steps=20, H=320, W=320, dtype="f16")
    assert model.dt == L.DT_F16
    rng = np.random.default_rng(31)
    frames = _video(rng, 12, 360, 640)
    exprs = _expressions(rng, 20, model.cfg.vocab_size, [7, 20])
    ups = _driver_loop(model, frames, exprs)
    thr = _median_threshold([ups])
    ref = _ref_masks(ups, frames, thr)
    fg = np.mean([r.mean() / 255 for r in ref.values()])
    print("threshold %.6g, foreground share of the reference masks %.3f" % (thr, fg))
    assert 0.05 < fg < 0.95
    seg = SG.ClipSegmenter(model, threshold=thr)
    _assert_exact(_run(seg, frames, exprs), ref, 12, 2, "config 5")
    assert seg.stats == {"frames": 12, "backbone_passes": 3, "gathers": 12, "heads": 24}


# ---- 5. DenseCRF and the sigm rule ---------------------------------------------------------------------------------------------------------
def test_clip_segmenter_dcrf_and_sigm(tiny):
    model, exprs = tiny["model"], tiny["exprs"][1:]
    H, W = model.H, model.W
    frames = tiny["videos"][1][:6]
    res, procs = _driver_loop(model, frames, exprs, want_proc=True)
    got = _run(SG.ClipSegmenter(model, dcrf=True, dcrf_method="lattice", value=1), frames, exprs)
    assert [(e, f) for e, f, _ in got] == [(e, f) for f in range(6) for e in range(2)]
    for e, f, mk in got:
        h, w = frames[f].shape[:2]
        sigm = torch.from_numpy(res[(e, f)][1]).cuda().reshape(1, H, W)
        lab = CRF.dense_crf_batch(sigm, procs[f][None], device=model.device, method="lattice").cpu().numpy()[0]
        want = HU.resize_and_crop(lab.astype(np.float32), h, w) > 0
        assert mk.shape == (h, w) and np.array_equal(mk, want.astype(np.uint8)), (e, f)
    got = _run(SG.ClipSegmenter(model, score="sigm", threshold=0.5, out_size=SG.half_size), frames, exprs)
    for e, f, mk in got:
        h, w = frames[f].shape[:2]
        want = HU.resize_and_crop((res[(e, f)][1] >= np.float32(0.5)).astype(np.float32), h // 2, w // 2) > 0
        assert np.array_equal(mk, want.astype(np.uint8) * 255), (e, f)


# ---- 6. the example script -----------------------------------------------------------------------------------------------------------------
def test_segment_clip_video_script(tmp_path, tiny):
    """examples/segment_clip_video.py as a fresh child process on a tiny snapshot, a folder of 6 frames and two sentences: the masks it
    writes equal ClipSegmenter's in this process."""
    CK = importlib.import_module("cmpc-refseg_amd.checkpoint")
    model, cfg = tiny["model"], tiny["cfg"]
    snap = CK.Saver(fmt="npz").save(model, str(tmp_path / "snap"))
    frames = tiny["videos"][0][:6]
    fdir, out = tmp_path / "frames", tmp_path / "out"
    fdir.mkdir()
    for f, a in enumerate(frames):
        np.save(str(fdir / ("%05d.npy" % f)), a)
    words = ["<pad>", "<unk>", "the", "dog", "on", "left", "a", "red", "car"]
    (tmp_path / "vocabulary.txt").write_text("\n".join(words) + "\n")
    vocab = HU.load_vocab_dict_from_file(str(tmp_path / "vocabulary.txt"))
    sentences = ["the dog on the left", "a red car"]
    want = {(e, f): mk for e, f, mk in SG.ClipSegmenter(model, vocab=vocab).run(frames, sentences)}
    kw = "vf_h=8,vf_w=8,vf_dim=256,c4_dim=128,c3_dim=64,vocab_size=50,v_emb_dim=40,mlp_dim=24,rnn_size=40,glove_dim=12,parse_dim=20," \
         "backbone_width=8,backbone_blocks=1:1:2:1,dtype=f32"
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cmd = [sys.executable, os.path.join(root, "examples", "segment_clip_video.py"), "--frames", str(fdir), "--vocab",
           str(tmp_path / "vocabulary.txt"), "--snapshot", snap, "--out", str(out), "--H", "64", "--W", "64", "--T", str(cfg.num_steps),
           "--model-kwargs", kw]
    for s in sentences:
        cmd += ["--sentence", s]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    assert "12 masks (2 expressions x 6 frames, 2 backbone passes)" in p.stdout
    assert sorted(os.listdir(str(out))) == sorted("exp%d_frame%05d.npy" % k for k in want)
    for (e, f), mk in want.items():
        assert np.array_equal(np.load(str(out / ("exp%d_frame%05d.npy" % (e, f)))), mk), (e, f)
