"""The reference's Refer-YouTube-VOS prediction loop (test.py:250-329) on a synthetic video: every referring expression over every
frame through segment.FrameSegmenter, one uint8 {0, 255} mask per (expression, frame) at half the frame's size, written as .npy files
where test.py writes PNGs (decoding and encoding image files is the caller's business).  Random weights unless --snapshot is given.
usage: python examples/segment_video.py [--frames 20] [--batch 8] [--out /tmp/cmpc_segment] [--snapshot PATH] [--dcrf]"""
import argparse, importlib, os, sys, tempfile, time
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=20)
ap.add_argument("--batch", type=int, default=8)
ap.add_argument("--out", default="/tmp/cmpc_segment")
ap.add_argument("--snapshot", default=None)
ap.add_argument("--dcrf", action="store_true")
args = ap.parse_args()

pkg = importlib.import_module("cmpc-refseg_amd")
CK = importlib.import_module("cmpc-refseg_amd.checkpoint")
HU = importlib.import_module("cmpc-refseg_amd.hostutil")
SG = importlib.import_module("cmpc-refseg_amd.segment")
H = W = 320
T = 20

WORDS = ["<pad>", "<unk>", "the", "a", "person", "dog", "car", "on", "left", "right", "red", "blue", "small", "large", "in", "front"]
vocab_path = os.path.join(tempfile.mkdtemp(), "vocabulary_synthetic.txt")
with open(vocab_path, "w") as f:
    f.write("\n".join(WORDS) + "\n")
vocab = HU.load_vocab_dict_from_file(vocab_path)
expressions = ["the red car on the left", "a small dog", "the person in front"]


def video(n, h=360, w=640):
    """A bright disc drifting over noise: frames are produced lazily, as a decoder would."""
    y, x = np.mgrid[0:h, 0:w]
    for f in range(n):
        rng = np.random.default_rng(f)
        im = rng.integers(0, 64, (h, w, 3), dtype=np.uint8)
        cx = w * (0.2 + 0.6 * f / max(1, n - 1))
        im[(y - h / 2) ** 2 + (x - cx) ** 2 < (h / 5) ** 2] += np.uint8(128)
        yield im


model = pkg.get_segmentation_model("CMPC_model", mode="eval", batch_size=args.batch, num_steps=T, H=H, W=W, vocab_size=len(WORDS))
if args.snapshot:
    CK.Saver().restore(model, args.snapshot)
seg = SG.FrameSegmenter(model, vocab=vocab, dcrf=args.dcrf)            # gv_norm="sample": every pair as the batch-1 loop computes it
os.makedirs(args.out, exist_ok=True)
t0, n = time.perf_counter(), 0
for e, f, mask in seg.run(video(args.frames), expressions):
    np.save(os.path.join(args.out, "exp%d_frame%05d.npy" % (e, f)), mask)
    n += 1
dt = time.perf_counter() - t0
print("%d masks of %s (%d expressions x %d frames) in %.2f s: %.1f pairs/s; written to %s" % (
    n, mask.shape, len(expressions), args.frames, dt, n / dt, args.out))
