"""Evaluation throughput on one box, in one run (config-2 CMPC_model, f16, B=8, seeded synthetic 480x640 images and masks):
  evaluator   Evaluator.add / result: prepare_images -> forward -> mask_iu, per-sample (I, U) read back once
  host_loop   trainval_model.test()'s loop with hostutil: resize_and_pad + img_as_ubyte + image_feed on the host, forward,
              resize_and_crop + SegEval on the host
  forward     forward only, device-resident feed
and the two kernels' time per batch from hipEvents around them.  Byte model per sample (both kernels read and write every byte once):
  eval_prep     h*w*3 (source) + H*W*3 (proc_im) + H*W*3*4 (feed)
  eval_mask_iu  H*W*4 (score map, the taps reread it from cache) + mh*mw (ground truth)
usage: python scripts/eval_bench.py [--short]"""
import argparse, importlib, json, os, sys, time
import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pkg = importlib.import_module("cmpc-refseg_amd")
EV = importlib.import_module("cmpc-refseg_amd.evaluate")
HU = importlib.import_module("cmpc-refseg_amd.hostutil")

ap = argparse.ArgumentParser()
ap.add_argument("--short", action="store_true", help="one warm-up and a 0.3 s window (profiling runs)")
args = ap.parse_args()
WINDOW = 0.3 if args.short else 2.0
B, T, H, W, h, w = 8, 20, 320, 320, 480, 640
rng = np.random.default_rng(0)
model = pkg.get_segmentation_model("CMPC_model", mode="eval", batch_size=B, num_steps=T, H=H, W=W, dtype="f16")
ims = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for _ in range(2 * B)]
gts = [rng.random((h, w)) < 0.3 for _ in range(2 * B)]
ids = rng.integers(1, model.cfg.vocab_size, (2 * B, T)).astype(np.int32)
sl = np.full(2 * B, T, np.int32)


def timed(fn, per_call):
    fn(); torch.cuda.synchronize()
    n, t0 = 0, time.perf_counter()
    while True:
        fn(); n += 1
        if time.perf_counter() - t0 >= WINDOW:
            break
    torch.cuda.synchronize()
    return n * per_call / (time.perf_counter() - t0)


def evaluator():
    ev = EV.Evaluator(model)
    for i in range(4 * B):
        k = i % (2 * B)
        ev.add(ids[k], sl[k], ims[k], gts[k])
    ev.result()


def host_loop():
    seg = HU.SegEval()
    for s in range(0, 2 * B, B):
        feed = np.stack([HU.image_feed(HU.img_as_ubyte(HU.resize_and_pad(ims[s + b], H, W))) for b in range(B)])
        up = model.forward(ids[s: s + B], feed, sl[s: s + B])["up"].float().cpu().numpy()
        for b in range(B):
            seg.add(HU.resize_and_crop((up[b, :, :, 0] >= 1e-9).astype(np.float32), h, w), gts[s + b])
    seg.result()


feed_dev, _ = EV.prepare_images(ims[:B], H, W)
res = {"evaluator_samples_per_s": timed(evaluator, 4 * B),
       "forward_images_per_s": timed(lambda: model.forward(ids[:B], feed_dev, sl[:B]), B)}
if not args.short:
    res["host_loop_samples_per_s"] = timed(host_loop, 2 * B)
# the kernels alone, bracketed by events (device time per batch of B)
up = model.forward(ids[:B], feed_dev, sl[:B])["up"].float()
e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
reps = 20
for f in (lambda: EV.prepare_images(ims[:B], H, W), lambda: EV.mask_iu(up, gts[:B], 1e-9)):
    f()
torch.cuda.synchronize()
ms = []
for f in (lambda: EV.prepare_images(ims[:B], H, W), lambda: EV.mask_iu(up, gts[:B], 1e-9)):
    tot = 0.0
    for _ in range(reps):
        f(); torch.cuda.synchronize()                  # the H2D staging copy happens before the first event
        e[0].record(); f(); e[1].record(); torch.cuda.synchronize()
        tot += e[0].elapsed_time(e[1])
    ms.append(tot / reps)
res["prep_plus_h2d_ms_per_batch"], res["mask_iu_plus_h2d_ms_per_batch"] = ms
res["bytes_prep_per_batch"] = B * (h * w * 3 + H * W * 3 + H * W * 12)
res["bytes_mask_per_batch"] = B * (H * W * 4 + h * w)
res["ratio_evaluator_to_forward"] = res["evaluator_samples_per_s"] / res["forward_images_per_s"]
print(json.dumps({k: round(v, 4) if isinstance(v, float) else v for k, v in res.items()}))
