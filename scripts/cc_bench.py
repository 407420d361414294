"""What cleaning masks by their connected components costs, on one box, in one run.
  kernels   cmpc_mask_components (keep = 1, 8-connectivity; the checkerboard 4-connectivity) on 8 masks already on the device, at
            360 x 640 and 720 x 1280, bracketed by events: a blob with speckle (the realistic case), the one-pixel serpentine and the
            checkerboard (the adversarial ones: the longest equivalence chain, the most components).  Median and the 10th..90th
            percentile of REPS calls after a warm-up; every result is checked against hostutil.clean_mask first.
  host      hostutil.clean_mask (scipy.ndimage.label) on the same 8 masks: the loop the kernels replace, seconds per 8 masks.
  segment   FrameSegmenter (config 2: CMPC_model, f16, B = 8) and ClipSegmenter (config 5: CMPC_video_mm_tgraph_allvec, f16) on seeded
            synthetic videos of 60 frames, masks at the frame's size, one expression: run() with clean={"keep": 1} against without,
            alternating rounds of device-synchronised windows after a warm-up of every variant; results per second.
usage: python scripts/cc_bench.py [--short] [--only kernels|frame|clip]"""
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
ap.add_argument("--short", action="store_true", help="fewer repetitions, 0.3 s windows, one round (profiling runs)")
ap.add_argument("--only", choices=["kernels", "frame", "clip"], default=None)
args = ap.parse_args()
REPS, HOST_REPS = (20, 1) if args.short else (200, 3)
WINDOW, ROUNDS = (0.3, 1) if args.short else (1.0, 3)
NMASK = 8
rng = np.random.default_rng(0)
res = {}


def blob_with_speckle(h, w, k):
    yy, xx = np.mgrid[0:h, 0:w]
    cy, cx = h // 2 + 5 * k, w // 3 + 11 * k
    m = ((yy - cy) / (h / 4.0)) ** 2 + ((xx - cx) / (w / 5.0)) ** 2 <= 1.0
    return m | (rng.random((h, w)) < 0.002)


def serpentine(h, w, k):
    m = np.zeros((h, w), bool)
    m[0::2] = True
    for y in range(1, h, 2):
        m[y, w - 1 if (y // 2) % 2 == 0 else 0] = True
    return m


def checkerboard(h, w, k):
    yy, xx = np.mgrid[0:h, 0:w]
    return (yy + xx + k) % 2 == 0


def kernels():
    dev = torch.device("cuda:0")
    cd = EV._CcDevice(dev)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    out = {}
    for h, w in ((360, 640), (720, 1280)):
        for name, make, conn in (("blob_speckle", blob_with_speckle, 8), ("serpentine", serpentine, 8), ("checkerboard", checkerboard, 4)):
            masks = [make(h, w, k).astype(np.uint8) * 255 for k in range(NMASK)]
            step = -(-h * w // 16) * 16
            src = torch.zeros(NMASK * step, dtype=torch.uint8, device=dev)
            for k, m in enumerate(masks):
                src[k * step: k * step + h * w] = torch.from_numpy(m.reshape(-1)).to(dev)
            work = torch.empty_like(src)
            stats = torch.empty(NMASK, 4, dtype=torch.int64, device=dev)
            descs = EV.cc_descs([(h, w)] * NMASK, [k * step for k in range(NMASK)])

            def call():
                cd.run(work.data_ptr(), work.numel(), descs, NMASK, conn, 1, 0, stats.data_ptr())
            # the answer first (one untimed call ahead: the first pays SciPy's import)
            HU.clean_mask(masks[0], 1, 0, conn)
            t0 = time.perf_counter()
            for _ in range(HOST_REPS):
                ref = [HU.clean_mask(m, 1, 0, conn) for m in masks]
            host_s = (time.perf_counter() - t0) / HOST_REPS
            work.copy_(src); call(); torch.cuda.synchronize()
            assert int(cd.status().item()) == 0
            got = work.cpu().numpy()
            for k, (rm, rs) in enumerate(ref):
                assert np.array_equal(got[k * step: k * step + h * w].reshape(h, w), rm) and np.array_equal(stats[k].cpu().numpy(), rs), (name, k)
            for _ in range(10):
                work.copy_(src); call()
            torch.cuda.synchronize()
            ms = []
            for _ in range(REPS):
                work.copy_(src)                    # the call cleans in place: every repetition starts from the uncleaned masks
                ev[0].record(); call(); ev[1].record(); torch.cuda.synchronize()
                ms.append(ev[0].elapsed_time(ev[1]))
            ms = np.array(ms)
            out["%s_%dx%d" % (name, h, w)] = {
                "device_ms_per_%d_masks" % NMASK: round(float(np.median(ms)), 4), "p10": round(float(np.percentile(ms, 10)), 4),
                "p90": round(float(np.percentile(ms, 90)), 4), "host_ms_per_%d_masks" % NMASK: round(1e3 * host_s, 2),
                "host_over_device": round(1e3 * host_s / float(np.median(ms)), 1), "components": int(ref[0][1][0]), "connectivity": conn}
    return out


if args.only in (None, "kernels"):
    res["kernels"] = kernels()

# ---- the segmenters with and without clean= -------------------------------------------------------------------------------------------
T, H, W, F = 20, 320, 320, 60
SIZES = {"480": (480, 640), "720": (720, 1280)}


def video(h, w):
    yy, xx = np.mgrid[0:h, 0:w]
    frames = []
    for f in range(F):
        im = np.stack([(xx * 255 // w), (yy * 255 // h), np.full((h, w), 90)], -1).astype(np.uint8)
        for e in range(3):
            cy, cx, rad = h * (1 + e) // 4, w // 6 + (w * 2 // 3) * f // F, h // (5 + e)
            im[(yy - cy) ** 2 + (xx - cx) ** 2 <= rad * rad] = (60 + 80 * e, 200 - 70 * e, 40 + 100 * e)
        frames.append(im)
    return frames


def window(fn, units):
    torch.cuda.synchronize()
    n, t0 = 0, time.perf_counter()
    while True:
        fn(); n += 1
        if time.perf_counter() - t0 >= WINDOW:
            break
    torch.cuda.synchronize()
    return n * units / (time.perf_counter() - t0)


kinds = [k for k in ("frame", "clip") if args.only in (None, k)]
if kinds:
    videos = {k: video(*s) for k, s in SIZES.items()}
    segs = {}
    if "frame" in kinds:
        m2 = pkg.get_segmentation_model("CMPC_model", mode="eval", batch_size=8, num_steps=T, H=H, W=W, dtype="f16")
        segs["frame"] = {c: SG.FrameSegmenter(m2, out_size=SG.full_size, copy=False, clean={"keep": 1} if c else None) for c in (False, True)}
        vocab = m2.cfg.vocab_size
    if "clip" in kinds:
        m5 = pkg.get_segmentation_model("CMPC_video_mm_tgraph_allvec", mode="eval", batch_size=1, num_steps=T, H=H, W=W, dtype="f16")
        segs["clip"] = {c: SG.ClipSegmenter(m5, score="sigm", threshold=0.5, copy=False, clean={"keep": 1} if c else None) for c in (False, True)}
        vocab = m5.cfg.vocab_size
    ids = np.zeros(T, np.int32)
    ids[:12] = rng.integers(1, vocab, 12)
    exprs = [(ids, 12)]
    frag = {}

    def run(kind, size, clean):
        seg = segs[kind][clean]
        n = sum(1 for _ in seg.run(videos[size], exprs))
        assert n == F
        if clean:
            st, _ = seg.cleaned.stats((None, 0))
            frag["%s_%s" % (kind, size)] = {"mean_components": round(float(st[:, 0].mean()), 2), "fragmented_frames": len(seg.cleaned.fragmented())}

    VARIANTS = [("%s_%s_%s" % (kind, size, "clean" if c else "plain"), (lambda kind=kind, size=size, c=c: run(kind, size, c)), F)
                for kind in kinds for size in SIZES for c in (False, True)]
    for _, fn, _ in VARIANTS:           # every variant once (backbone graphs, workspaces, staging buffers, rings)
        fn()
    torch.cuda.synchronize()
    rounds = {k: [] for k, _, _ in VARIANTS}
    for r in range(ROUNDS):
        for k, fn, units in VARIANTS:
            rounds[k].append(window(fn, units))
    md = {k: round(float(np.median(v)), 1) for k, v in rounds.items()}
    res["segment"] = {"unit": "(frame, expression) results per second", "rounds": {k: [round(x, 1) for x in v] for k, v in rounds.items()},
                      "median": md, "spread": {k: round((max(v) - min(v)) / float(np.median(v)), 4) for k, v in rounds.items()},
                      "clean_over_plain": {k[:-6]: round(md[k[:-6] + "_clean"] / md[k], 3) for k in md if k.endswith("_plain")},
                      "masks_of_the_random_model": frag}
print(json.dumps(res))
