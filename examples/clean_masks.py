"""Clean a segmenter's masks on the device: keep the largest connected component of every mask before it is scored.  A synthetic
video (three moving discs, every frame annotated) goes through segment.FrameSegmenter twice, without and with clean={"keep": 1}, with
ground truth both times, so J, F and J&F are those of the raw and of the cleaned masks; then hostutil.CleanLog.fragmented() lists the
frames whose largest component holds less than 90 % of the foreground -- a per-frame quality signal beside PivotLog.inconsistent().
The weights are random, so the numbers only show the plumbing: cmpc_mask_components labels the masks where cmpc_eval_mask_out left
them, drops all but the largest component in place, cmpc_mask_jf scores what is left, and four integers per result (components, area,
largest area, kept area) come back with the masks.
usage: python examples/clean_masks.py [--frames 24] [--height 240 --width 427] [--keep 1] [--min-area 0]"""
import argparse, importlib, json, os, sys
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=24)
ap.add_argument("--height", type=int, default=240)
ap.add_argument("--width", type=int, default=427)
ap.add_argument("--keep", type=int, default=1)
ap.add_argument("--min-area", type=int, default=0)
args = ap.parse_args()

pkg = importlib.import_module("cmpc-refseg_amd")
HU = importlib.import_module("cmpc-refseg_amd.hostutil")
SG = importlib.import_module("cmpc-refseg_amd.segment")

h, w, N, T = args.height, args.width, args.frames, 20
yy, xx = np.mgrid[0:h, 0:w]
frames, gts = [], {}
for f in range(N):
    im = np.stack([xx * 255 // w, yy * 255 // h, np.full((h, w), 90)], -1).astype(np.uint8)
    for e in range(3):
        cx = w // 6 + (w * 2 // 3) * f // N
        disc = (yy - h * (1 + e) // 4) ** 2 + (xx - cx) ** 2 <= (h // (5 + e)) ** 2
        im[disc] = (60 + 80 * e, 200 - 70 * e, 40 + 100 * e)
        gts[(e, f)] = disc[::2, ::2][: h // 2, : w // 2].view(np.uint8)       # FrameSegmenter writes masks at half size
    frames.append(im)

rng = np.random.default_rng(0)
model = pkg.get_segmentation_model("CMPC_model", mode="eval", batch_size=8, num_steps=T, H=320, W=320, dtype="f16")
exprs = []
for n in (4, 9, 15):
    ids = np.zeros(T, np.int32)
    ids[:n] = rng.integers(1, model.cfg.vocab_size, n)
    exprs.append((ids, n))

for name, clean in (("raw masks", None), ("cleaned masks", {"keep": args.keep, "min_area": args.min_area})):
    seg = SG.FrameSegmenter(model, clean=clean)
    n = sum(1 for _ in seg.run(frames, exprs, ground_truth=lambda e, f: gts[(e, f)], seq="synthetic"))
    res = seg.jf.result()
    print("%-14s %d masks: J %.4f  F %.4f  J&F %.4f" % (name, n, res["J_mean"], res["F_mean"], res["J&F"]))
log = seg.cleaned
for e in range(len(exprs)):
    st, _ = log.stats(("synthetic", e))
    print("  expression %d: %.1f components per frame, %.1f %% of the foreground in the largest, %.1f %% kept" % (
        e, st[:, 0].mean(), 100.0 * st[:, 2].sum() / max(st[:, 1].sum(), 1), 100.0 * st[:, 3].sum() / max(st[:, 1].sum(), 1)))
frag = log.fragmented(0.9)
print("fragmented frames (largest component < 90 %% of the foreground): %d of %d" % (len(frag), len(log)))
print("  " + ", ".join("e%d f%d" % (s[1], f) for s, f in frag[:12]) + (" ..." if len(frag) > 12 else ""))
print("first entry of CleanLog.dump():", json.dumps(log.dump()[0]))
