"""Mask propagation from pivot frames: the step the reference's find_pivot_frames was written for ("Find pivot frames for propagate",
test.py:150-181) and never got.  FrameSegmenter segments a video with describe="c4" (the descriptors find_pivot_frames needs) and
propagate={...} (the taps, sigm maps and labels a propagator needs stay in device banks); PivotLog.meta() picks the pivot frames per
expression; seg.propagate() then carries each pivot frame's answer to the frames within num_propagate of it along cosine affinities
between the c4 taps (cmpc_label_propagate), blends it with the frame's own sigm (cmpc_prop_fuse) and yields the new masks of those
frames.  The video is synthetic and the weights random, so the numbers only show the plumbing.
usage: python examples/propagate_video.py [--frames 24] [--height 240 --width 427] [--propagate 2] [--alpha 0.5] [--radius 12]"""
import argparse, importlib, os, sys
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=24)
ap.add_argument("--height", type=int, default=240)
ap.add_argument("--width", type=int, default=427)
ap.add_argument("--propagate", type=int, default=2)
ap.add_argument("--alpha", type=float, default=0.5)
ap.add_argument("--radius", type=int, default=12)
args = ap.parse_args()

pkg = importlib.import_module("cmpc-refseg_amd")
SG = importlib.import_module("cmpc-refseg_amd.segment")

h, w, N, T = args.height, args.width, args.frames, 20
yy, xx = np.mgrid[0:h, 0:w]
frames = []
for f in range(N):
    im = np.stack([xx * 255 // w, yy * 255 // h, np.full((h, w), 90)], -1).astype(np.uint8)
    for k in range(3):
        cx = w // 6 + (w * (2 + 2 * k) // 3) * f // N
        im[(yy - h * (1 + k) // 4) ** 2 + (xx - cx) ** 2 <= (h // (5 + k)) ** 2] = (60 + 80 * k, 200 - 70 * k, 40 + 100 * k)
    frames.append(im)

rng = np.random.default_rng(0)
model = pkg.get_segmentation_model("CMPC_model", mode="eval", batch_size=8, num_steps=T, H=320, W=320, dtype="f16")
exprs = []
for n in (4, 9, 15):
    ids = np.zeros(T, np.int32)
    ids[:n] = rng.integers(1, model.cfg.vocab_size, n)
    exprs.append((ids, n))

seg = SG.FrameSegmenter(model, describe="c4", propagate={"radius": args.radius, "alpha": args.alpha, "num_propagate": args.propagate,
                                                          "bank": N, "results": N * len(exprs)})
masks = {(e, f): mk for e, f, mk in seg.run(frames, exprs, seq="synthetic")}
meta = seg.pivots.meta(args.propagate)
print("%d masks; meta_pivot_frames: %s" % (len(masks), {str(k): v for k, v in meta.items()}))
n = moved = 0
for e, f, mk in seg.propagate(seg.pivots):
    n += 1
    moved += int((mk != masks[(e, f)]).sum())
    masks[(e, f)] = mk                                  # pivot frames keep the masks run() gave
print("%d of %d masks received their pivots' answers (alpha %.2f, radius %d): %d pixels changed" % (n, len(masks), args.alpha, args.radius, moved))
