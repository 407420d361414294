"""Score a segmented video with J, F and J&F, the measures Refer-YouTube-VOS and Refer-DAVIS are ranked by, for both segmenters: the
image model through segment.FrameSegmenter and the video model through segment.ClipSegmenter.  The video and its colour-coded
annotations are synthetic (three moving objects in the Refer-YouTube-VOS colours, every fifth frame annotated, one object leaving the
picture), the weights random, so the numbers only show the plumbing: ground_truth(e, f) hands over the annotation of frame f and the key
colour of expression e's object, cmpc_mask_jf scores the masks where they lie on the device, and six integers per result come back
with the masks.  (The definitions restate the DAVIS-2017 evaluation code; parity against it is unpinned.)
usage: python examples/score_video.py [--frames 30] [--height 240 --width 427]"""
import argparse, importlib, os, sys
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=30)
ap.add_argument("--height", type=int, default=240)
ap.add_argument("--width", type=int, default=427)
args = ap.parse_args()

pkg = importlib.import_module("cmpc-refseg_amd")
FD = importlib.import_module("cmpc-refseg_amd.feed")
HU = importlib.import_module("cmpc-refseg_amd.hostutil")
SG = importlib.import_module("cmpc-refseg_amd.segment")

h, w, N, T = args.height, args.width, args.frames, 20
OBJECTS = ["1", "2", "3"]                                     # obj_id of each expression's object
yy, xx = np.mgrid[0:h, 0:w]
frames, annotations = [], {}
for f in range(N):
    im = np.stack([xx * 255 // w, yy * 255 // h, np.full((h, w), 90)], -1).astype(np.uint8)
    ann = np.zeros((h, w, 3), np.uint8)
    for k, obj in enumerate(OBJECTS):
        cx = w // 6 + (w * (2 + 2 * k) // 3) * f // N              # the third object leaves the picture on the right
        disc = (yy - h * (1 + k) // 4) ** 2 + (xx - cx) ** 2 <= (h // (5 + k)) ** 2
        im[disc] = (60 + 80 * k, 200 - 70 * k, 40 + 100 * k)
        ann[disc] = FD.REFVOS_OBJECT_COLOR[obj]
    frames.append(im)
    if f % 5 == 0:
        annotations[f] = ann


def ground_truth_at(out_size):
    def ground_truth(e, f):
        """None for a frame without annotation; else (annotation, key colour): hostutil.object_mask cuts expression e's object."""
        if f not in annotations:
            return None
        oh, ow = out_size(h, w)
        ann = annotations[f] if (oh, ow) == (h, w) else annotations[f][:: h // oh, :: w // ow][:oh, :ow]
        return ann, FD.REFVOS_OBJECT_COLOR[OBJECTS[e]]
    return ground_truth


rng = np.random.default_rng(0)
image_model = pkg.get_segmentation_model("CMPC_model", mode="eval", batch_size=8, num_steps=T, H=320, W=320, dtype="f16")
video_model = pkg.get_segmentation_model("CMPC_video_mm_tgraph_allvec", mode="eval", batch_size=1, num_steps=T, H=320, W=320, dtype="f16")
exprs = []
for n in (4, 9, 15):
    ids = np.zeros(T, np.int32)
    ids[:n] = rng.integers(1, min(image_model.cfg.vocab_size, video_model.cfg.vocab_size), n)
    exprs.append((ids, n))

for name, seg in (("FrameSegmenter (CMPC_model, masks at half size)", SG.FrameSegmenter(image_model)),
                  ("ClipSegmenter (CMPC_video_mm_tgraph_allvec, masks at full size)", SG.ClipSegmenter(video_model, score="sigm", threshold=0.5))):
    n = sum(1 for _ in seg.run(frames, exprs, ground_truth=ground_truth_at(seg.out_size), seq="synthetic"))
    res = seg.jf.result()
    print("%s: %d masks, %d scored frames in %d sequences" % (name, n, res["frames"], res["sequences"]))
    for s, r in res["per_sequence"].items():
        print("  %-18s J %.3f  F %.3f  (%d frames; J recall %.2f decay %+.3f, F recall %.2f decay %+.3f)" % (
            s, r["J_mean"], r["F_mean"], r["frames"], r["J_recall"], r["J_decay"], r["F_recall"], r["F_decay"]))
    print("  J %.4f  F %.4f  J&F %.4f" % (res["J_mean"], res["F_mean"], res["J&F"]))
