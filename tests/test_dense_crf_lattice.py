"""DenseCRF through the permutohedral lattice (crf.py method="lattice", csrc/ops_crf_lattice.hip).  The CPU tests pin the float64
restatement (tests/crf_lattice_ref.py) by properties every correct lattice has and by its distance from the exact oracle; the GPU tests
compare the HIP path with the restatement and check batching, determinism, the full-size run and the evaluators.  Parity against
pydensecrf itself is UNPINNED (not installed)."""
import importlib

import numpy as np
import pytest

from oracle import dense_crf_numpy as OC
from tests import crf_lattice_ref as R

CRF = importlib.import_module("cmpc-refseg_amd.crf")


def _case(rng, H, W):
    """A noisy disc: sigmoid map and a two-tone image that follows it (the shape of test_dense_crf.py's cases)."""
    yy, xx = np.mgrid[0:H, 0:W]
    p = 1 / (1 + np.exp(-(((xx - W / 2) ** 2 + (yy - H / 2) ** 2 < (min(H, W) / 3) ** 2) * 3.0 - 1.5 + rng.normal(0, 0.8, (H, W)))))
    rgb = np.clip(rng.normal(0, 6, (H, W, 3)) + np.where(p[..., None] > 0.5, 150, 60), 0, 255).astype(np.uint8)
    return p, rgb


# ---- CPU: the restatement ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("HW", [(12, 13), (20, 24), (1, 17)])
def test_lattice_operator_linear_transpose_positive(HW):
    H, W = HW
    rng = np.random.default_rng(H * W)
    rgb = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    for lat in R.lattices((H, W), rgb):
        N, d = H * W, lat.d
        assert lat.M <= N * (d + 1) and np.allclose(lat.w.sum(1), 1, atol=1e-6) and (lat.w > -1e-6).all()
        u, v = rng.normal(size=(N, 1)), rng.normal(size=(N, 1))
        # linear
        assert np.allclose(lat.apply(2.0 * u - 3.0 * v), 2.0 * lat.apply(u) - 3.0 * lat.apply(v), atol=1e-10)
        # splat is the transpose of slice: <S u, x> = <u, S^T x> for vertex values x
        x = rng.normal(size=(lat.M + 1, 1)); x[lat.M] = 0
        assert abs((lat.splat(u) * x).sum() - lat.alpha ** -1 * (u * lat.slice(x)).sum()) < 1e-10 * np.abs(u).sum() * np.abs(x).sum()
        # every blur pass is symmetric: <B_j y, x> = <y, B_j x>
        y = rng.normal(size=(lat.M + 1, 1)); y[lat.M] = 0
        for j in range(d + 1):
            assert abs((lat.blur(y, [j]) * x).sum() - (y * lat.blur(x, [j])).sum()) < 1e-10 * (np.abs(x).sum() + np.abs(y).sum()) ** 2
        # hence u.L v = v.L' u with L' the passes in reverse order.  The product of the passes is not symmetric itself where a vertex a
        # two-step path would cross is absent (pydensecrf's compute(..., reverse=True) exists for that), so u.L v = v.L u is not asserted.
        a = (u * lat.apply(v)).sum()
        assert abs(a - (v * lat.apply(u, order=range(d, -1, -1))).sum()) <= 1e-10 * max(1.0, abs(a))
        # positive
        assert lat.apply(np.ones((N, 1))).min() > 0


def test_lattice_closed_forms_and_strong_edge():
    rng = np.random.default_rng(0)
    p = rng.uniform(0.05, 0.95, (6, 7))
    rgb = rng.integers(0, 256, (6, 7, 3), dtype=np.uint8)
    for q in (R.dense_crf(p, rgb, iters=0), R.dense_crf(p, rgb, compat_g=0.0, compat_b=0.0, iters=3)):
        assert np.allclose(q[1], p, atol=1e-12) and np.allclose(q[0], 1 - p, atol=1e-12)
    p3 = np.concatenate([np.full((8, 4), 0.9), np.full((8, 4), 0.1)], 1)
    im3 = np.concatenate([np.full((8, 4, 3), 200, np.uint8), np.full((8, 4, 3), 20, np.uint8)], 1)
    m = R.dense_crf(p3, im3).argmax(0)
    assert m[:, :4].all() and not m[:, 4:].any()


def test_lattice_masks_close_to_exact_oracle():
    # The lattice approximates the Gaussian kernels (Adams et al. 2010), so its masks may differ from the exact ones where the exact
    # pairwise energy is close to balancing the unary.  Measured on these 16 cases (seeds 0-3): 15 of 8468 "sure" pixels
    # (|Q1 - Q0| > 1e-3 under the exact oracle) disagree, 0.18 %; the worst case is 8 of 481 (1.7 %), always the 13 x 37 one with the
    # non-default sxy_b 9 / srgb 6 (a narrow image: most pixels lie near a border of the disc).  Seeds 0-7: 32 of 16936, worst 1.7 %.
    # The bar, 3 % per case and 0.5 % overall, leaves room for that and fails on a wrong lattice (a lost blur direction or normaliser
    # flips whole regions).
    bad = tot = 0
    for seed in range(4):
        rng = np.random.default_rng(seed)
        for H, W, kw in ((20, 24, {}), (13, 37, dict(sxy_g=2.0, compat_g=1.5, sxy_b=9.0, srgb=6.0, compat_b=4.0, iters=3)),
                         (16, 16, dict(iters=1)), (30, 30, {})):
            p, rgb = _case(rng, H, W)
            ql, qe = R.dense_crf(p, rgb, **kw), OC.dense_crf(p, rgb, **kw)
            sure = np.abs(qe[1] - qe[0]) > 1e-3
            d = int((ql.argmax(0)[sure] != qe.argmax(0)[sure]).sum())
            assert d <= 0.03 * sure.sum(), (seed, H, W, d, sure.sum())
            bad, tot = bad + d, tot + int(sure.sum())
    assert bad <= 0.005 * tot, (bad, tot)


def test_lattice_bad_inputs_rejected_without_a_gpu(pkg):
    p = np.full((4, 5), 0.5, np.float32)
    rgb = np.zeros((4, 5, 3), np.uint8)
    with pytest.raises(ValueError):
        CRF.dense_crf(p, rgb, device="cpu", method="permutohedral")
    with pytest.raises(ValueError):
        CRF.dense_crf_batch(p, rgb, device="cpu", method="lattice")                  # not [B, H, W]
    with pytest.raises(ValueError):
        CRF.dense_crf_batch(p[None], rgb[None, :3], device="cpu", method="lattice")  # rgb does not match
    with pytest.raises(ValueError):
        CRF.dense_crf_batch(p[None], rgb[None].astype(np.float32), device="cpu", method="lattice")
    # the entry point validates its parameters before touching a device
    lib = pkg._lib.load()
    fake = 256
    good = dict(sxy_g=3.0, compat_g=3.0, sxy_b=20.0, srgb=3.0, compat_b=10.0)

    def rc(B=2, H=320, W=320, iters=5, **kw):
        a = dict(good); a.update(kw)
        return lib.cmpc_dense_crf_lattice(fake, fake, B, H, W, a["sxy_g"], a["compat_g"], a["sxy_b"], a["srgb"], a["compat_b"], iters,
                                          fake, fake, None)
    assert rc(B=0) == -1 and rc(H=0) == -1 and rc(iters=-1) == -1 and rc(srgb=0.0) == -1 and rc(sxy_g=-1.0) == -1
    assert rc(srgb=0.1) == -1 and b"12-bit" in lib.cmpc_last_error()                     # colour keys beyond +-2047
    assert rc(sxy_b=0.5) == -1 and b"bilateral" in lib.cmpc_last_error()
    assert rc(sxy_g=1e-7) == -1 and b"Gaussian" in lib.cmpc_last_error()


# ---- GPU -----------------------------------------------------------------------------------------------------------------------------

GPU_CASES = [
    (20, 24, {}),
    (13, 37, dict(sxy_g=2.0, compat_g=1.5, sxy_b=9.0, srgb=6.0, compat_b=4.0, iters=3)),
    (9, 9, dict(iters=0)),
    (16, 16, dict(iters=1)),
    (1, 29, {}),
    (31, 1, dict(iters=1)),
    (23, 31, dict(sxy_g=1.5, compat_g=5.0, sxy_b=6.0, srgb=10.0, compat_b=2.0, iters=5)),
]


@pytest.mark.gpu
@pytest.mark.parametrize("case", range(len(GPU_CASES)))
def test_hip_lattice_matches_restatement(case):
    H, W, kw = GPU_CASES[case]
    p, rgb = _case(np.random.default_rng(10 + case), H, W)
    ref = R.dense_crf(p, rgb, **kw)
    q = CRF.dense_crf(p.astype(np.float32), rgb, method="lattice", **kw).cpu().numpy()
    m = CRF.dense_crf_mask(p.astype(np.float32), rgb, method="lattice", **kw).cpu().numpy()
    assert np.abs(q - ref).max() < 2e-4, (H, W, np.abs(q - ref).max())
    sure = np.abs(ref[1] - ref[0]) > 1e-3
    assert np.array_equal(m[sure], ref.argmax(0)[sure].astype(np.uint8))


@pytest.mark.gpu
def test_hip_lattice_batch_independent_and_bit_identical():
    import torch
    rng = np.random.default_rng(5)
    H, W = 40, 52
    cases = [_case(rng, H, W) for _ in range(3)]
    sig = torch.tensor(np.stack([c[0] for c in cases]).astype(np.float32), device="cuda:0")
    rgb = torch.tensor(np.stack([c[1] for c in cases]), device="cuda:0")
    q, m = CRF.dense_crf_batch(sig, rgb, method="lattice", want_q=True)
    q2, m2 = CRF.dense_crf_batch(sig, rgb, method="lattice", want_q=True)
    torch.cuda.synchronize()
    assert torch.equal(q, q2) and torch.equal(m, m2)
    for b in range(3):
        qb = CRF.dense_crf(sig[b], rgb[b], method="lattice")
        mb = CRF.dense_crf_mask(sig[b], rgb[b], method="lattice")
        assert torch.equal(q[b], qb) and torch.equal(m[b], mb), b
    # the batch in another order: each sample's bits do not depend on its position
    perm = [2, 0, 1]
    qp, mp = CRF.dense_crf_batch(sig[perm], rgb[perm], method="lattice", want_q=True)
    assert torch.equal(qp, q[perm]) and torch.equal(mp, m[perm])
    # the exact method through dense_crf_batch: per-sample calls of cmpc_dense_crf
    me = CRF.dense_crf_batch(sig, rgb)
    for b in range(3):
        assert torch.equal(me[b], CRF.dense_crf_mask(sig[b], rgb[b]))


@pytest.mark.gpu
def test_hip_lattice_full_size_disc():
    import torch
    rng = np.random.default_rng(1)
    H = W = 320
    yy, xx = np.mgrid[0:H, 0:W]
    disc = (xx - 170) ** 2 + (yy - 150) ** 2 < 70 ** 2
    p = np.clip(np.where(disc, 0.8, 0.2) + rng.normal(0, 0.25, (H, W)), 0.01, 0.99).astype(np.float32)
    rgb = np.clip(rng.normal(0, 4, (H, W, 3)) + np.where(disc[..., None], 180, 40), 0, 255).astype(np.uint8)
    q = CRF.dense_crf(p, rgb, method="lattice")
    qe = CRF.dense_crf(p, rgb)
    torch.cuda.synchronize()
    q, qe = q.cpu().numpy(), qe.cpu().numpy()
    assert np.isfinite(q).all() and np.allclose(q.sum(0), 1, atol=1e-5)
    raw_err = ((p > 0.5) != disc).mean(); crf_err = ((q[1] > q[0]) != disc).mean()
    assert raw_err > 0.05 and crf_err < 0.002, (raw_err, crf_err)
    agree = ((q[1] > q[0]) == (qe[1] > qe[0])).mean()
    print("lattice vs exact mask agreement on the 320 x 320 disc: %.6f (%d pixels differ)" % (agree, int(round((1 - agree) * H * W))))
    assert agree > 0.995


@pytest.mark.gpu
def test_hip_lattice_invalid_inputs():
    import torch
    p = np.full((8, 9), 0.5, np.float32)
    rgb = np.zeros((8, 9, 3), np.uint8)
    with pytest.raises(ValueError):
        CRF.dense_crf(p, rgb[:4], method="lattice")
    with pytest.raises(ValueError):
        CRF.dense_crf(p, rgb.astype(np.int16), method="lattice")
    with pytest.raises(ValueError):
        CRF.dense_crf_batch(p, rgb, method="lattice")
    with pytest.raises(ValueError):
        CRF.dense_crf_mask(p, rgb, method="Lattice")
    for kw in (dict(srgb=0.05), dict(sxy_b=0.01), dict(iters=-1), dict(sxy_g=0.0)):      # keys beyond +-2047, bad args
        with pytest.raises(CRF._lib.CmpcError):
            CRF.dense_crf_mask(p, rgb, method="lattice", **kw)
    # a valid call still works after the refused ones
    m = CRF.dense_crf_mask(p, rgb, method="lattice")
    torch.cuda.synchronize()
    assert m.shape == (8, 9)


@pytest.mark.gpu
def test_evaluator_dcrf_lattice():
    import tests.test_gpu_eval as TE
    EV, HU = TE.EV, TE.HU
    model, cfg = TE._tiny_model(3)
    rng = np.random.default_rng(3)
    samples = TE._samples(rng, 4, cfg.num_steps, cfg.vocab_size, [(48, 80), (100, 64)])
    with pytest.raises(ValueError):
        EV.Evaluator(model, dcrf=True, dcrf_method="dense")
    ev = EV.Evaluator(model, dcrf=True, dcrf_method="lattice")
    for s in samples:
        ev.add(*s)
    res = ev.result()
    seg = HU.SegEval()
    B = model.batch_size
    for s0 in range(0, 4, B):
        chunk = samples[s0: s0 + B]
        pad = chunk + [chunk[0]] * (B - len(chunk))
        feed, proc = EV.prepare_images([s[2] for s in pad], model.H, model.W)
        out = model.forward(np.stack([s[0] for s in pad]), feed, np.array([s[1] for s in pad], np.int32))
        for b, s in enumerate(chunk):
            m = CRF.dense_crf_mask(out["sigm"][b].float().reshape(model.H, model.W), proc[b], method="lattice").cpu().numpy()
            seg.add(HU.resize_and_crop(m.astype(np.float32), s[3].shape[0], s[3].shape[1]), s[3])
    for k, v in seg.result().items():
        assert res["dcrf_" + k] == v, k


@pytest.mark.gpu
def test_video_evaluator_dcrf_lattice():
    import tests.test_gpu_eval_video as TV
    EV, HU = TV.EV, TV.HU
    model, cfg = TV._tiny_model()
    rng = np.random.default_rng(3)
    T = cfg.num_steps
    samples = TV._clips(rng, 3, T, cfg.vocab_size, [(48, 80), (100, 64)], [3, T])
    seg = HU.SegEval(TV.THR)
    for text, im, frames, mask in samples:
        vi = np.array([[HU.first_valid_idx(text)]], np.int32)
        clip, _ = EV.prepare_images(list(frames), model.H, model.W)
        out = model.forward_video(text[None], None, vi, clip[None])
        _, proc = EV.prepare_images([im], model.H, model.W)
        m = CRF.dense_crf_mask(out["sigm"][0].float().reshape(model.H, model.W), proc[0], method="lattice").cpu().numpy()
        seg.add(HU.resize_and_crop(m.astype(np.float32), mask.shape[0], mask.shape[1]), mask)
    ev = EV.VideoEvaluator(model, dcrf=True, dcrf_method="lattice")
    for s in samples:
        ev.add(*s)
    res = ev.result()
    for k, v in seg.result().items():
        assert res["dcrf_" + k] == v, k
