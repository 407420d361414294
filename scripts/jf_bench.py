"""What scoring J and F costs the segmenters, on one box, in one run (config 2: CMPC_model, f16, B = 8, FrameSegmenter; config 5:
CMPC_video_mm_tgraph_allvec, f16, ClipSegmenter; seeded synthetic videos of 60 frames of 480 x 640 and of 720 x 1280, masks at the
frame's size, E = 1 and E = 3 expressions, EVERY frame annotated -- Refer-YouTube-VOS annotates every fifth):
  plain    segmenter.run(frames, exprs): the path as it was
  scored   segmenter.run(frames, exprs, ground_truth=...): ground truths uploaded, cmpc_mask_jf on the device, six integers per result
  host     the plain run's masks scored on the host with tests/jf_ref.py (seconds per pair, a few pairs: context figure)
Alternating rounds of device-synchronised windows after a warm-up of every variant; (frame, expression) results per second.  Then
cmpc_mask_jf alone on one result's masks, bracketed by events.
usage: python scripts/jf_bench.py [--short] [--only frame|clip]"""
import argparse, importlib, json, os, sys, time
import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pkg = importlib.import_module("cmpc-refseg_amd")
EV = importlib.import_module("cmpc-refseg_amd.evaluate")
SG = importlib.import_module("cmpc-refseg_amd.segment")
HU = importlib.import_module("cmpc-refseg_amd.hostutil")
from tests import jf_ref as R

ap = argparse.ArgumentParser()
ap.add_argument("--short", action="store_true", help="0.3 s windows, one round, no host loop (profiling runs)")
ap.add_argument("--only", choices=["frame", "clip"], default=None)
args = ap.parse_args()
WINDOW, ROUNDS = (0.3, 1) if args.short else (1.5, 3)
T, H, W, F = 20, 320, 320, 60
SIZES = {"480": (480, 640), "720": (720, 1280)}
rng = np.random.default_rng(0)


def video(h, w):
    """Smooth frames (a few moving discs on a gradient) and, per expression, the moving disc's mask as the ground truth."""
    yy, xx = np.mgrid[0:h, 0:w]
    frames, gts = [], {}
    for f in range(F):
        im = np.stack([(xx * 255 // w), (yy * 255 // h), np.full((h, w), 90)], -1).astype(np.uint8)
        for e in range(3):
            cy, cx, rad = h * (1 + e) // 4, w // 6 + (w * 2 // 3) * f // F, h // (5 + e)
            disc = (yy - cy) ** 2 + (xx - cx) ** 2 <= rad * rad
            im[disc] = (60 + 80 * e, 200 - 70 * e, 40 + 100 * e)
            gts[(e, f)] = disc.view(np.uint8)
        frames.append(im)
    return frames, gts


videos = {k: video(*s) for k, s in SIZES.items()}
segs = {}
if args.only != "clip":
    m2 = pkg.get_segmentation_model("CMPC_model", mode="eval", batch_size=8, num_steps=T, H=H, W=W, dtype="f16")
    segs["frame"] = SG.FrameSegmenter(m2, out_size=SG.full_size, copy=False)
if args.only != "frame":
    m5 = pkg.get_segmentation_model("CMPC_video_mm_tgraph_allvec", mode="eval", batch_size=1, num_steps=T, H=H, W=W, dtype="f16")
    segs["clip"] = SG.ClipSegmenter(m5, score="sigm", threshold=0.5, copy=False)
exprs = []
for n in (5, 12, 20):
    ids = np.zeros(T, np.int32)
    ids[:n] = rng.integers(1, min(sg.model.cfg.vocab_size for sg in segs.values()), n)
    exprs.append((ids, n))


def run(kind, size, E, scored, keep=None):
    frames, gts = videos[size]
    kw = dict(ground_truth=lambda e, f: gts[(e, f)]) if scored else {}
    n = 0
    for e, f, mk in segs[kind].run(frames, exprs[:E], **kw):
        n += 1
        if keep is not None and len(keep) < 3:
            keep.append((e, f, mk.copy()))
    assert n == F * E
    if scored:
        assert segs[kind].jf.result()["frames"] == F * E


def window(fn, units):
    torch.cuda.synchronize()
    n, t0 = 0, time.perf_counter()
    while True:
        fn(); n += 1
        if time.perf_counter() - t0 >= WINDOW:
            break
    torch.cuda.synchronize()
    return n * units / (time.perf_counter() - t0)


VARIANTS = [("%s_%s_E%d_%s" % (kind, size, E, "scored" if sc else "plain"), (lambda kind=kind, size=size, E=E, sc=sc: run(kind, size, E, sc)), F * E)
            for kind in segs for size in SIZES for E in (1, 3) for sc in (False, True)]
for _, fn, _ in VARIANTS:               # every variant once (backbone graphs, workspaces, staging buffers, rings)
    fn()
torch.cuda.synchronize()
rounds = {k: [] for k, _, _ in VARIANTS}
for r in range(ROUNDS):
    for k, fn, units in VARIANTS:
        rounds[k].append(window(fn, units))
res = {"unit": "(frame, expression) results per second", "rounds": {k: [round(x, 1) for x in v] for k, v in rounds.items()}}
res["median"] = md = {k: round(float(np.median(v)), 1) for k, v in rounds.items()}
res["spread"] = {k: round((max(v) - min(v)) / float(np.median(v)), 4) for k, v in rounds.items()}
res["scored_over_plain"] = {k[:-6]: round(md[k[:-6] + "_scored"] / md[k], 3) for k in md if k.endswith("_plain")}

# cmpc_mask_jf alone: one result's masks (the plain run's first three) against their ground truths, bracketed by events
e2 = [torch.cuda.Event(enable_timing=True) for _ in range(2)]


def event_ms(fn, reps=30):
    fn(); torch.cuda.synchronize()
    tot = []
    for _ in range(reps):
        e2[0].record(); fn(); e2[1].record(); torch.cuda.synchronize()
        tot.append(e2[0].elapsed_time(e2[1]))
    return float(np.median(tot))


kind0 = "frame" if "frame" in segs else "clip"
res["mask_jf_ms_per_pair"], res["boundary_pixels"], res["host_s_per_pair"], res["J&F_of_the_random_model"] = {}, {}, {}, {}
for size in SIZES:
    kept = []
    run(kind0, size, 1, False, keep=kept)
    gts = videos[size][1]
    pd = [torch.from_numpy(mk).cuda() for _, _, mk in kept]
    gd = [torch.from_numpy(gts[(e, f)]).cuda() for e, f, _ in kept]
    counts = EV.mask_jf(pd, gd)
    res["mask_jf_ms_per_pair"][size] = round(event_ms(lambda: EV.mask_jf(pd, gd)) / len(kept), 4)      # includes the result's own copy
    res["boundary_pixels"][size] = [int(c[2]) for c in counts]
    if not args.short:
        t0 = time.perf_counter()
        ref = np.stack([R.counts(mk, gts[(e, f)], HU.jf_radius(*mk.shape)) for e, f, mk in kept])
        res["host_s_per_pair"][size] = round((time.perf_counter() - t0) / len(kept), 3)
        assert np.array_equal(ref, counts), size
for kind in segs:
    res["J&F_of_the_random_model"][kind] = round(segs[kind].jf.result()["J&F"], 4)
print(json.dumps(res))
