"""DenseCRF cost, exact (cmpc_dense_crf, 4-sigma window) against the permutohedral lattice (cmpc_dense_crf_lattice), on one GPU:
  per_sample_ms   event-timed device time per 320 x 320 sample with the reference's parameters (5 iterations), B = 1 and B = 8
                  (exact at B = 8: crf.dense_crf_batch, one cmpc_dense_crf call per sample; lattice: one call for the batch)
  evaluator       Evaluator samples/s at config 2 (CMPC_model, f16, B = 8, seeded synthetic 480 x 640 images and masks): no dcrf,
                  dcrf_method "exact" and dcrf_method "lattice"
  agreement       lattice vs exact mask agreement on the 320 x 320 noisy-disc fixture of the tests
usage: python scripts/crf_bench.py [--short] [--lattice-only]   (--lattice-only: the lattice runs alone, for a kernel trace)"""
import argparse, importlib, json, os, sys, time
import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pkg = importlib.import_module("cmpc-refseg_amd")
EV = importlib.import_module("cmpc-refseg_amd.evaluate")
CRF = importlib.import_module("cmpc-refseg_amd.crf")

ap = argparse.ArgumentParser()
ap.add_argument("--short", action="store_true", help="fewer repetitions and a 0.3 s evaluator window")
ap.add_argument("--lattice-only", action="store_true", help="time the lattice path only (no evaluator)")
args = ap.parse_args()
REPS = 3 if args.short else 10
WINDOW = 0.3 if args.short else 2.0
S = 320


def disc_case(rng):
    """The full-size fixture of tests/test_dense_crf.py: a noisy disc on a two-tone image (centre jittered per sample)."""
    yy, xx = np.mgrid[0:S, 0:S]
    cx, cy = 170 + rng.integers(-20, 21), 150 + rng.integers(-20, 21)
    disc = (xx - cx) ** 2 + (yy - cy) ** 2 < 70 ** 2
    p = np.clip(np.where(disc, 0.8, 0.2) + rng.normal(0, 0.25, (S, S)), 0.01, 0.99).astype(np.float32)
    rgb = np.clip(rng.normal(0, 4, (S, S, 3)) + np.where(disc[..., None], 180, 40), 0, 255).astype(np.uint8)
    return p, rgb, disc


def event_ms(fn, reps):
    fn(); torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    best = []
    for _ in range(reps):
        e0.record(); fn(); e1.record(); torch.cuda.synchronize()
        best.append(e0.elapsed_time(e1))
    return float(np.median(best))


rng = np.random.default_rng(0)
cases = [disc_case(rng) for _ in range(8)]
sig = torch.tensor(np.stack([c[0] for c in cases]), device="cuda:0")
rgb = torch.tensor(np.stack([c[1] for c in cases]), device="cuda:0")
res = {}
for B in (1, 8):
    res["lattice_ms_per_sample_B%d" % B] = event_ms(lambda: CRF.dense_crf_batch(sig[:B], rgb[:B], method="lattice"), REPS) / B
    if not args.lattice_only:
        res["exact_ms_per_sample_B%d" % B] = event_ms(lambda: CRF.dense_crf_batch(sig[:B], rgb[:B], method="exact"), REPS) / B
        res["speedup_B%d" % B] = res["exact_ms_per_sample_B%d" % B] / res["lattice_ms_per_sample_B%d" % B]

if not args.lattice_only:
    ql, mask_l = CRF.dense_crf_batch(sig, rgb, method="lattice", want_q=True)
    mask_e = CRF.dense_crf_batch(sig, rgb, method="exact")
    discs = torch.tensor(np.stack([c[2] for c in cases]), device="cuda:0")
    res["agreement_lattice_vs_exact"] = float((mask_l == mask_e).float().mean())
    res["crf_err_lattice"] = float((mask_l.bool() != discs).float().mean())
    res["crf_err_exact"] = float((mask_e.bool() != discs).float().mean())
    res["q_sum_max_dev_lattice"] = float((ql.sum(1) - 1).abs().max())

    Bm, T, h, w = 8, 20, 480, 640
    model = pkg.get_segmentation_model("CMPC_model", mode="eval", batch_size=Bm, num_steps=T, H=S, W=S, dtype="f16")
    ims = [np.random.default_rng(i).integers(0, 256, (h, w, 3), dtype=np.uint8) for i in range(2 * Bm)]
    gts = [np.random.default_rng(100 + i).random((h, w)) < 0.3 for i in range(2 * Bm)]
    ids = np.random.default_rng(7).integers(1, model.cfg.vocab_size, (2 * Bm, T)).astype(np.int32)
    sl = np.full(2 * Bm, T, np.int32)

    def rate(**kw):
        def run():
            ev = EV.Evaluator(model, **kw)
            for i in range(4 * Bm):
                k = i % (2 * Bm)
                ev.add(ids[k], sl[k], ims[k], gts[k])
            ev.result()
        run(); torch.cuda.synchronize()
        n, t0 = 0, time.perf_counter()
        while True:
            run(); n += 1
            if time.perf_counter() - t0 >= WINDOW:
                break
        torch.cuda.synchronize()
        return n * 4 * Bm / (time.perf_counter() - t0)
    res["evaluator_samples_per_s_no_dcrf"] = rate()
    res["evaluator_samples_per_s_dcrf_exact"] = rate(dcrf=True)
    res["evaluator_samples_per_s_dcrf_lattice"] = rate(dcrf=True, dcrf_method="lattice")
print(json.dumps({k: round(v, 5) if isinstance(v, float) else v for k, v in res.items()}))
