"""The drivers' pictures from the device: the `-v` switch of trainval_model.py (im / gt / pred per sample of a split), the panels of
test_visualize_fusion*.py (sigmoid(up_c3 | up_c4 | up_c5 | sigm) at the frame's size through `jet`) and of test_visualize_graph.py (one
panel per word of gw_v).  Samples are synthetic and the weights random, so the pictures only show the plumbing: Evaluator(visualize=fn)
hands fn every sample's pictures as host arrays, visualize.heat_maps / word_sheets render the fetched maps where they lie.  (The colour
index is taken on the arrays' own pixels; matplotlib's imshow resamples to the screen: parity with it is unpinned.)
Pictures are saved as PNG when Pillow imports, as .npy otherwise.
usage: python examples/visualize_split.py [--samples 5] [--out vis_out]"""
import argparse, importlib, os, sys
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--samples", type=int, default=5)
ap.add_argument("--out", default="vis_out")
args = ap.parse_args()

pkg = importlib.import_module("cmpc-refseg_amd")
EV = importlib.import_module("cmpc-refseg_amd.evaluate")
VIS = importlib.import_module("cmpc-refseg_amd.visualize")

try:
    from PIL import Image
except ImportError:
    Image = None
os.makedirs(args.out, exist_ok=True)


def save(name, pic):
    if Image is not None:
        Image.fromarray(pic).save(os.path.join(args.out, name + ".png"))
    else:
        np.save(os.path.join(args.out, name + ".npy"), pic)


T, B = 20, 4
model = pkg.get_segmentation_model("CMPC_model", mode="eval", batch_size=B, num_steps=T, H=320, W=320, dtype="f16")
rng = np.random.default_rng(0)
samples = []
for i in range(args.samples):
    h, w = [(480, 640), (375, 500), (640, 427)][i % 3]
    yy, xx = np.mgrid[0:h, 0:w]
    disc = (yy - h * rng.uniform(0.3, 0.7)) ** 2 + (xx - w * rng.uniform(0.3, 0.7)) ** 2 <= (min(h, w) * 0.25) ** 2
    im = np.stack([xx * 255 // w, yy * 255 // h, np.full((h, w), 90)], -1).astype(np.uint8)
    im[disc] = (220, 60, 40)
    n = int(rng.integers(3, T + 1))
    ids = np.zeros(T, np.int32)
    ids[:n] = rng.integers(1, model.cfg.vocab_size, n)
    samples.append((ids, n, im, disc))

# the -v switch: im.png / gt.png / pred.png per sample (visualize_seg)
ev = EV.Evaluator(model, visualize=lambda i, pics: [save("%04d_%s" % (i, k), v) for k, v in pics.items()])
for s in samples:
    ev.add(*s)
res = ev.result()
print("samples = %d; overall IoU = %f; mean IoU = %f" % (res["samples"], res["overall_IoU"], res["mean_IoU"]))

# the fusion figure and the word graph of the first batch
chunk = samples[:B] + [samples[0]] * max(0, B - len(samples))
feed, _ = EV.prepare_images([s[2] for s in chunk], model.H, model.W, model.device)
out = model.forward(np.stack([s[0] for s in chunk]), feed, np.array([s[1] for s in chunk], np.int32))
sizes = [s[2].shape[:2] for s in chunk]
for name in ("up_c3", "up_c4", "up_c5", "sigm"):                     # the script's sigmoid on `sigm` too is the caller's choice
    buf, descs = VIS.heat_maps(out[name].float(), sizes, sigmoid=True)
    for b, pic in enumerate(VIS.unpack_pictures(buf.cpu().numpy(), descs)[:len(samples)]):
        save("%04d_heat_%s" % (b, name), pic)
sheets = VIS.word_sheets(out["gw_v"].float(), [s[1] for s in chunk], (model.cfg.vf_h, model.cfg.vf_w)).cpu().numpy()
for b in range(min(B, len(samples))):
    save("%04d_words" % b, sheets[b])
print("wrote %s pictures to %s" % ("PNG" if Image is not None else ".npy", args.out))
