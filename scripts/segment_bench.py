"""Per-expression video segmentation on one box, in one run (config-2 CMPC_model, f16, B = 8, a seeded synthetic 32-frame 720 x 1280
video, E = 1 and E = 4 expressions, masks at (h // 2, w // 2)):
  segmenter    segment.FrameSegmenter.run: backbone once per frame batch, head once per expression, cmpc_eval_mask_out, pinned ring
  parent       what predict_masks did before cmpc_eval_mask_out, per expression and 8 frames: prepare_images, model.forward,
               mask_iu(want_masks) against all-zero ground truths, .cpu() per mask (the backbone runs once per expression)
  forward      forward only, device-resident feed, in mode "batch" and in mode "sample" (the yardstick Evaluator / VideoEvaluator are
               quoted against)
  host_loop    test.py:250-329 as written: batch 1, hostutil resize on the host (context figure, a few frames)
Three alternating rounds of device-synchronised windows (>= 3 s each) after a warm-up of every shape; (frame, expression) pairs per
second.  Then cmpc_eval_mask_out and the head's forward pass of the same batch, bracketed by events.
usage: python scripts/segment_bench.py [--short]"""
import argparse, importlib, json, os, sys, time
import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pkg = importlib.import_module("cmpc-refseg_amd")
EV = importlib.import_module("cmpc-refseg_amd.evaluate")
SG = importlib.import_module("cmpc-refseg_amd.segment")
HU = importlib.import_module("cmpc-refseg_amd.hostutil")

ap = argparse.ArgumentParser()
ap.add_argument("--short", action="store_true", help="0.3 s windows, one round (profiling runs)")
args = ap.parse_args()
WINDOW, ROUNDS = (0.3, 1) if args.short else (3.0, 3)
B, T, H, W, h, w, F = 8, 20, 320, 320, 720, 1280, 32
rng = np.random.default_rng(0)
model = pkg.get_segmentation_model("CMPC_model", mode="eval", batch_size=B, num_steps=T, H=H, W=W, dtype="f16")
frames = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for _ in range(F)]
exprs = []
for n in (5, 9, 14, 20):
    ids = np.zeros(T, np.int32)
    ids[:n] = rng.integers(1, model.cfg.vocab_size, n)
    exprs.append((ids, n))
half = [(h // 2, w // 2)] * B
zeros_half = [np.zeros(s, np.uint8) for s in half]
seg = SG.FrameSegmenter(model, threshold=0.5, copy=False)


def segmenter(E):
    n = 0
    for _ in seg.run(frames, exprs[:E]):
        n += 1
    assert n == F * E


def parent(E):
    """The earlier predict_masks, at half size: per expression and 8 frames a full forward pass, a ground truth of zeros uploaded for I / U
    nobody reads, one synchronising .cpu() per mask."""
    for s in range(0, F, B):
        for ids, n in exprs[:E]:
            feed, _ = EV.prepare_images(frames[s: s + B], H, W, model.device)
            up = model.forward(np.repeat(ids[None], B, 0), feed, np.full(B, n, np.int32))["sigm"]
            _, masks = EV.mask_iu(up.float(), zeros_half, 0.5, want_masks=True)
            [mk.cpu().numpy() for mk in masks]


feed_dev, _ = EV.prepare_images(frames[:B], H, W)
ids8, sl8 = np.repeat(exprs[3][0][None], B, 0), np.full(B, exprs[3][1], np.int32)


def forward(mode):
    model.set_gv_norm(mode)
    model.forward(ids8, feed_dev, sl8)
    model.set_gv_norm("batch")


def window(fn, units):
    torch.cuda.synchronize()
    n, t0 = 0, time.perf_counter()
    while True:
        fn(); n += 1
        if time.perf_counter() - t0 >= WINDOW:
            break
    torch.cuda.synchronize()
    return n * units / (time.perf_counter() - t0)


VARIANTS = [("segmenter_E1", lambda: segmenter(1), F), ("parent_E1", lambda: parent(1), F), ("segmenter_E4", lambda: segmenter(4), 4 * F),
            ("parent_E4", lambda: parent(4), 4 * F), ("forward_batch", lambda: forward("batch"), B), ("forward_sample", lambda: forward("sample"), B)]
for _, fn, _ in VARIANTS:               # every shape once (backbone graphs, workspaces, staging buffers, the pinned ring)
    fn()
    fn()
torch.cuda.synchronize()
rounds = {k: [] for k, _, _ in VARIANTS}
for r in range(ROUNDS):
    for k, fn, units in VARIANTS:
        rounds[k].append(window(fn, units))
res = {"unit": "(frame, expression) pairs per second; forward_*: images per second", "rounds": {k: [round(x, 1) for x in v] for k, v in rounds.items()}}
res["median"] = {k: round(float(np.median(v)), 1) for k, v in rounds.items()}
res["spread"] = {k: round((max(v) - min(v)) / float(np.median(v)), 4) for k, v in rounds.items()}
md = res["median"]
res["segmenter_E1_over_parent_E1"] = round(md["segmenter_E1"] / md["parent_E1"], 3)
res["segmenter_E4_over_parent_E4"] = round(md["segmenter_E4"] / md["parent_E4"], 3)
res["segmenter_E4_over_segmenter_E1"] = round(md["segmenter_E4"] / md["segmenter_E1"], 3)
res["segmenter_E1_over_forward"] = round(md["segmenter_E1"] / md["forward_batch"], 3)
res["forward_sample_over_batch"] = round(md["forward_sample"] / md["forward_batch"], 4)

# cmpc_eval_mask_out and the head's forward pass of the same batch, bracketed by events (device time per call)
model.set_gv_norm("sample")
feats, done = model.features_async(feed_dev)
words = torch.from_numpy(ids8).to(model.device)
sl_d = torch.from_numpy(sl8).to(model.device)
sigm = model.head(feats, words, sl_d, after=done)["sigm"].float().reshape(B, H, W).clone()
buf = torch.empty(B * (-(-(h // 2) * (w // 2) // 16) * 16), dtype=torch.uint8, device=model.device)
e = [torch.cuda.Event(enable_timing=True) for _ in range(2)]


def event_ms(fn, reps=30):
    fn(); torch.cuda.synchronize()
    tot = []
    for _ in range(reps):
        e[0].record(); fn(); e[1].record(); torch.cuda.synchronize()
        tot.append(e[0].elapsed_time(e[1]))
    return float(np.median(tot))


res["mask_out_ms_per_call"] = round(event_ms(lambda: EV.masks_out(sigm, half, 0.5, value=255, out=buf)), 4)
res["head_forward_ms_per_call"] = round(event_ms(lambda: model.head(feats, words, sl_d)), 4)
res["mask_out_over_head_forward"] = round(res["mask_out_ms_per_call"] / res["head_forward_ms_per_call"], 4)
res["mask_out_bytes_per_call"] = B * (H * W * 4 + (h // 2) * (w // 2))
model.set_gv_norm("batch")

if not args.short:
    # context: test.py's loop as written -- one sample per forward pass, every resize on the host
    m1 = pkg.get_segmentation_model("CMPC_model", mode="eval", batch_size=1, num_steps=T, H=H, W=W, dtype="f16")

    def host_loop():
        for f in frames[:4]:
            feed = HU.image_feed(HU.img_as_ubyte(HU.resize_and_pad(f, H, W)))[None]
            s = m1.forward(exprs[3][0][None], feed, np.array([exprs[3][1]], np.int32))["sigm"].float().cpu().numpy()[0, :, :, 0]
            (HU.resize_and_crop((s >= 0.5).astype(np.float32), h // 2, w // 2) > 0).astype(np.uint8) * 255
    host_loop()
    res["host_loop_pairs_per_s_context"] = round(window(host_loop, 4), 2)
print(json.dumps(res))
