"""What propagating costs beside segmenting, on one box, in one run (config 2: CMPC_model, f16, B = 8, FrameSegmenter; seeded synthetic
videos of 60 frames of 480 x 640 and of 720 x 1280, masks at the frame's size, E = 1 and E = 3 expressions):
  plain      segmenter.run(frames, exprs) of a segmenter without propagate=: the path as it was
  banked     the same run with propagate= on: the taps, sigm maps and labels are also kept in the device banks
  propagate  seg.propagate(pivots) behind that run, pivots every fifth frame (num_propagate = 2: four of five frames receive):
             cmpc_label_propagate, cmpc_prop_fuse and cmpc_eval_mask_out per batch of 8 frames; no backbone and no head
Alternating rounds of device-synchronised windows after a warm-up of every variant; (frame, expression) results per second.  Then the
two kernels alone on one batch's inputs, bracketed by events.
usage: python scripts/propagate_bench.py [--short]"""
import argparse, importlib, json, os, sys, time
import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pkg = importlib.import_module("cmpc-refseg_amd")
EV = importlib.import_module("cmpc-refseg_amd.evaluate")
SG = importlib.import_module("cmpc-refseg_amd.segment")

ap = argparse.ArgumentParser()
ap.add_argument("--short", action="store_true", help="0.3 s windows, one round (profiling runs)")
args = ap.parse_args()
WINDOW, ROUNDS = (0.3, 1) if args.short else (1.5, 3)
T, H, W, F = 20, 320, 320, 60
SIZES = {"480": (480, 640), "720": (720, 1280)}
rng = np.random.default_rng(0)


def video(h, w):
    """Smooth frames: a few moving discs on a gradient."""
    yy, xx = np.mgrid[0:h, 0:w]
    frames = []
    for f in range(F):
        im = np.stack([(xx * 255 // w), (yy * 255 // h), np.full((h, w), 90)], -1).astype(np.uint8)
        for e in range(3):
            cy, cx, rad = h * (1 + e) // 4, w // 6 + (w * 2 // 3) * f // F, h // (5 + e)
            im[(yy - cy) ** 2 + (xx - cx) ** 2 <= rad * rad] = (60 + 80 * e, 200 - 70 * e, 40 + 100 * e)
        frames.append(im)
    return frames


videos = {k: video(*s) for k, s in SIZES.items()}
m2 = pkg.get_segmentation_model("CMPC_model", mode="eval", batch_size=8, num_steps=T, H=H, W=W, dtype="f16")
plain = SG.FrameSegmenter(m2, out_size=SG.full_size, copy=False)
banked = SG.FrameSegmenter(m2, out_size=SG.full_size, copy=False, propagate={"bank": F, "results": 3 * F})
exprs = []
for n in (5, 12, 20):
    ids = np.zeros(T, np.int32)
    ids[:n] = rng.integers(1, m2.cfg.vocab_size, n)
    exprs.append((ids, n))
PIVOTS = list(range(2, F, 5))
N_PROP = F - len(PIVOTS)


def run(seg, size, E):
    assert sum(1 for _ in seg.run(videos[size], exprs[:E])) == F * E


def propagate(E):
    assert sum(1 for _ in banked.propagate({e: PIVOTS for e in range(E)})) == N_PROP * E


def window(fn, units, before=None):
    if before is not None:
        before()
    torch.cuda.synchronize()
    n, t0 = 0, time.perf_counter()
    while True:
        fn(); n += 1
        if time.perf_counter() - t0 >= WINDOW:
            break
    torch.cuda.synchronize()
    return n * units / (time.perf_counter() - t0)


VARIANTS = []
for size in SIZES:
    for E in (1, 3):
        VARIANTS.append(("%s_E%d_plain" % (size, E), (lambda size=size, E=E: run(plain, size, E)), F * E, None))
        VARIANTS.append(("%s_E%d_banked" % (size, E), (lambda size=size, E=E: run(banked, size, E)), F * E, None))
        # the propagate pass reads the banks of the banked run of the same size and E: that run goes first, outside the window
        VARIANTS.append(("%s_E%d_propagate" % (size, E), (lambda E=E: propagate(E)), N_PROP * E, (lambda size=size, E=E: run(banked, size, E))))
for _, fn, _, before in VARIANTS:       # every variant once (backbone graphs, workspaces, staging buffers, rings)
    if before is not None:
        before()
    fn()
torch.cuda.synchronize()
rounds = {k: [] for k, _, _, _ in VARIANTS}
for r in range(ROUNDS):
    for k, fn, units, before in VARIANTS:
        rounds[k].append(window(fn, units, before))
res = {"unit": "(frame, expression) results per second", "rounds": {k: [round(x, 1) for x in v] for k, v in rounds.items()}}
res["median"] = md = {k: round(float(np.median(v)), 1) for k, v in rounds.items()}
res["spread"] = {k: round((max(v) - min(v)) / float(np.median(v)), 4) for k, v in rounds.items()}
res["banked_over_plain"] = {k[:-6]: round(md[k[:-6] + "_banked"] / md[k], 3) for k in md if k.endswith("_plain")}
res["propagate_over_run"] = {k[:-6]: round(md[k[:-6] + "_propagate"] / md[k[:-6] + "_banked"], 3) for k in md if k.endswith("_plain")}

# the two kernels alone, on the inputs of one batch of config 2 (8 items of two sources each on a 40 x 40 x 1024 f16 tap bank)
e2 = [torch.cuda.Event(enable_timing=True) for _ in range(2)]


def event_ms(fn, reps=50):
    fn(); torch.cuda.synchronize()
    tot = []
    for _ in range(reps):
        e2[0].record(); fn(); e2[1].record(); torch.cuda.synchronize()
        tot.append(e2[0].elapsed_time(e2[1]))
    return float(np.median(tot))


g = torch.Generator(device="cuda").manual_seed(0)
bank = torch.randn(12, 40, 40, 1024, device="cuda", generator=g).relu().half()
labels = torch.rand(12, 40, 40, device="cuda", generator=g)
own = torch.rand(8, H, W, device="cuda", generator=g)
res["label_propagate_ms"], res["prop_fuse_ms"] = {}, {}
for nsrc in (1, 2):
    items = [(i, [((i + 1 + k) % 12, (i + 1 + k) % 12) for k in range(nsrc)]) for i in range(8)]
    for radius in (12, -1):
        ms = event_ms(lambda: EV.label_propagate(bank, labels, items, radius, 0.07))       # includes the wrapper's one small allocation
        res["label_propagate_ms"]["n8_src%d_r%d" % (nsrc, radius)] = round(ms, 4)
prop = EV.label_propagate(bank, labels, items, 12, 0.07)
res["prop_fuse_ms"]["n8"] = round(event_ms(lambda: EV.prop_fuse(own, prop, 0.5)), 4)
print(json.dumps(res))
