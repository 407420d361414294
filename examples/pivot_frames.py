"""Pivot frames per expression: the last step of the reference's inference driver (test.py:150-181, 289-330).  While FrameSegmenter
segments a video, describe="c4" pools the c4 backbone tap under each result's own sigm (cmpc_mask_pool) and counts where the c4 and c5
score levels agree (cmpc_level_agree); a few KB per result ride back with the masks into a hostutil.PivotLog, from which
find_pivot_frames picks the frames a mask propagator would start from and the frames whose levels disagree are listed.  The video is
synthetic and the weights random, so the numbers only show the plumbing.  (As the reference writes the selection, the frame least like
the most typical one is tried first; nearest_first=True tries the most typical one first.  The reference's function cannot run, so parity
against it is unpinned.)
usage: python examples/pivot_frames.py [--frames 24] [--height 240 --width 427] [--propagate 2]"""
import argparse, importlib, os, sys
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=24)
ap.add_argument("--height", type=int, default=240)
ap.add_argument("--width", type=int, default=427)
ap.add_argument("--propagate", type=int, default=2)
args = ap.parse_args()

pkg = importlib.import_module("cmpc-refseg_amd")
SG = importlib.import_module("cmpc-refseg_amd.segment")

h, w, N, T = args.height, args.width, args.frames, 20
yy, xx = np.mgrid[0:h, 0:w]
frames = []
for f in range(N):
    im = np.stack([xx * 255 // w, yy * 255 // h, np.full((h, w), 90)], -1).astype(np.uint8)
    for k in range(3):
        cx = w // 6 + (w * (2 + 2 * k) // 3) * f // N              # the third object leaves the picture on the right
        im[(yy - h * (1 + k) // 4) ** 2 + (xx - cx) ** 2 <= (h // (5 + k)) ** 2] = (60 + 80 * k, 200 - 70 * k, 40 + 100 * k)
    frames.append(im)

rng = np.random.default_rng(0)
model = pkg.get_segmentation_model("CMPC_model", mode="eval", batch_size=8, num_steps=T, H=320, W=320, dtype="f16")
exprs = []
for n in (4, 9, 15):
    ids = np.zeros(T, np.int32)
    ids[:n] = rng.integers(1, model.cfg.vocab_size, n)
    exprs.append((ids, n))

seg = SG.FrameSegmenter(model, describe="c4")
n = sum(1 for _ in seg.run(frames, exprs, seq="synthetic"))
log = seg.pivots
print("%d masks, %d described results in %d sequences" % (n, len(log), len(log.seqs)))
for s in log.seqs:
    d, ids = log.descriptors(s)
    c = log.consistencies(s)
    print("  %-18s descriptors %s, mean area %.1f of 1600, level consistency %.3f .. %.3f" % (
        s, d.shape, log.areas(s).mean(), np.nanmin(c) if not np.all(np.isnan(c)) else float("nan"), np.nanmax(c) if not np.all(np.isnan(c)) else float("nan")))
    print("    pivots as written    %s" % log.pivots(s, args.propagate))
    print("    pivots nearest first %s" % log.pivots(s, args.propagate, nearest_first=True))
bad = log.inconsistent(below=0.3)
print("inconsistent frames (I / U of the c4 and c5 levels below 0.3): %d of %d" % (len(bad), len(log)))
for s, f in bad[:10]:
    print("  %s frame %d" % (s, f))
print("meta_pivot_frames:", {str(k): v for k, v in log.meta(args.propagate).items()})
