"""What describe= costs the segmenters, on one box, in one run (config 2: CMPC_model, f16, B = 8, FrameSegmenter; config 5:
CMPC_video_mm_tgraph_allvec, f16, ClipSegmenter; seeded synthetic videos of 60 frames of 480 x 640 and of 720 x 1280, masks at the
frame's size, E = 1 and E = 3 expressions):
  plain      segmenter.run(frames, exprs): the path as it was
  described  the same run of a segmenter built with describe="c4": cmpc_mask_pool on the c4 tap and cmpc_level_agree behind each head,
             descriptor, area and counts in the tail of the slot's one copy, a hostutil.PivotLog filled as the masks are handed out
Alternating rounds of device-synchronised windows after a warm-up of every variant; (frame, expression) results per second.  Then the
two kernels alone on one head call's inputs, bracketed by events.
usage: python scripts/pivot_bench.py [--short] [--only frame|clip]"""
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
ap.add_argument("--only", choices=["frame", "clip"], default=None)
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
segs = {}
if args.only != "clip":
    m2 = pkg.get_segmentation_model("CMPC_model", mode="eval", batch_size=8, num_steps=T, H=H, W=W, dtype="f16")
    segs["frame"] = {False: SG.FrameSegmenter(m2, out_size=SG.full_size, copy=False),
                     True: SG.FrameSegmenter(m2, out_size=SG.full_size, copy=False, describe="c4")}
if args.only != "frame":
    m5 = pkg.get_segmentation_model("CMPC_video_mm_tgraph_allvec", mode="eval", batch_size=1, num_steps=T, H=H, W=W, dtype="f16")
    segs["clip"] = {False: SG.ClipSegmenter(m5, score="sigm", threshold=0.5, copy=False),
                    True: SG.ClipSegmenter(m5, score="sigm", threshold=0.5, copy=False, describe="c4")}
exprs = []
for n in (5, 12, 20):
    ids = np.zeros(T, np.int32)
    ids[:n] = rng.integers(1, min(sg[False].model.cfg.vocab_size for sg in segs.values()), n)
    exprs.append((ids, n))


def run(kind, size, E, described):
    seg = segs[kind][described]
    n = sum(1 for _ in seg.run(videos[size], exprs[:E]))
    assert n == F * E
    if described:
        assert len(seg.pivots) == F * E


def window(fn, units):
    torch.cuda.synchronize()
    n, t0 = 0, time.perf_counter()
    while True:
        fn(); n += 1
        if time.perf_counter() - t0 >= WINDOW:
            break
    torch.cuda.synchronize()
    return n * units / (time.perf_counter() - t0)


VARIANTS = [("%s_%s_E%d_%s" % (kind, size, E, "described" if d else "plain"), (lambda kind=kind, size=size, E=E, d=d: run(kind, size, E, d)), F * E)
            for kind in segs for size in SIZES for E in (1, 3) for d in (False, True)]
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
res["described_over_plain"] = {k[:-6]: round(md[k[:-6] + "_described"] / md[k], 3) for k in md if k.endswith("_plain")}

# the two kernels alone, on the inputs of one head call of config 2 (8 results, a 40 x 40 x 1024 f16 tap) and of config 5 (1 result)
e2 = [torch.cuda.Event(enable_timing=True) for _ in range(2)]


def event_ms(fn, reps=50):
    fn(); torch.cuda.synchronize()
    tot = []
    for _ in range(reps):
        e2[0].record(); fn(); e2[1].record(); torch.cuda.synchronize()
        tot.append(e2[0].elapsed_time(e2[1]))
    return float(np.median(tot))


g = torch.Generator(device="cuda").manual_seed(0)
res["mask_pool_ms"], res["level_agree_ms"], res["mask_pool_GBps"] = {}, {}, {}
for n in (8, 1):
    tap = torch.randn(n, 40, 40, 1024, device="cuda", generator=g).relu().half()
    sigm = torch.rand(n, H, W, device="cuda", generator=g)
    a, b = torch.randn(n, 40, 40, device="cuda", generator=g), torch.randn(n, 40, 40, device="cuda", generator=g)
    for mode in ("soft", "hard"):
        ms = event_ms(lambda: EV.mask_pool(tap, sigm, mode))            # includes the wrapper's two small allocations
        res["mask_pool_ms"]["n%d_%s" % (n, mode)] = round(ms, 4)
        res["mask_pool_GBps"]["n%d_%s" % (n, mode)] = round(tap.numel() * 2 / ms / 1e6, 1)
    res["level_agree_ms"]["n%d" % n] = round(event_ms(lambda: EV.level_agree(a, b)), 4)
print(json.dumps(res))
