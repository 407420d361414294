"""What the `-v` pictures cost an evaluation, on one box, in one run (config 2: CMPC_model, f16, B = 8, 320 x 320; seeded synthetic
samples of 480 x 640 and of 720 x 1280):
  plain    Evaluator(model): the path as it was
  hooked   Evaluator(model, visualize=no-op): cmpc_vis_overlay for gt and pred on the staged frames, the pictures read back
  host     the host loop: evaluate.predict_masks plus tests/vis_ref.py's overlays (seconds per sample on a few samples: context figure)
Alternating rounds of device-synchronised windows after a warm-up of every variant; samples per second.  Then the hook's parts alone
on one batch (the two overlay launches, the read-back, and what uploading the frames a second time would cost), and
visualize.heat_maps of four maps per sample with its read-back against tests/vis_ref.py's heat on the host.
usage: python scripts/vis_bench.py [--short]"""
import argparse, importlib, json, os, sys, time
import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pkg = importlib.import_module("cmpc-refseg_amd")
EV = importlib.import_module("cmpc-refseg_amd.evaluate")
VIS = importlib.import_module("cmpc-refseg_amd.visualize")
from tests import vis_ref as R

ap = argparse.ArgumentParser()
ap.add_argument("--short", action="store_true", help="0.3 s windows, one round, no host loops (profiling runs)")
args = ap.parse_args()
WINDOW, ROUNDS = (0.3, 1) if args.short else (1.5, 3)
T, H, W, B, N = 20, 320, 320, 8, 32
SIZES = {"480": (480, 640), "720": (720, 1280)}
rng = np.random.default_rng(0)
model = pkg.get_segmentation_model("CMPC_model", mode="eval", batch_size=B, num_steps=T, H=H, W=W, dtype="f16")


def make(h, w):
    yy, xx = np.mgrid[0:h, 0:w]
    out = []
    for i in range(N):
        disc = (yy - h * rng.uniform(0.3, 0.7)) ** 2 + (xx - w * rng.uniform(0.3, 0.7)) ** 2 <= (min(h, w) * rng.uniform(0.1, 0.3)) ** 2
        im = np.stack([xx * 255 // w, yy * 255 // h, np.full((h, w), 90)], -1).astype(np.uint8)
        im[disc] = (220, 60, 40)
        n = int(rng.integers(3, T + 1))
        ids = np.zeros(T, np.int32)
        ids[:n] = rng.integers(1, model.cfg.vocab_size, n)
        out.append((ids, n, im, disc.view(np.uint8)))
    return out


samples = {k: make(*s) for k, s in SIZES.items()}
stats = {}


def run(size, hooked):
    seen = []
    ev = EV.Evaluator(model, visualize=(lambda i, pics: seen.append(i)) if hooked else None)
    for s in samples[size]:
        ev.add(*s)
    res = ev.result()
    if hooked:
        assert seen == list(range(N))
        stats[size] = ev.pictures.bytes_read_back / N
    return res


def window(fn, units):
    torch.cuda.synchronize()
    n, t0 = 0, time.perf_counter()
    while True:
        fn(); n += 1
        if time.perf_counter() - t0 >= WINDOW:
            break
    torch.cuda.synchronize()
    return n * units / (time.perf_counter() - t0)


VARIANTS = [("%s_%s" % (size, "hooked" if hk else "plain"), (lambda size=size, hk=hk: run(size, hk)), N) for size in SIZES for hk in (False, True)]
for size in SIZES:                      # every variant once (backbone graphs, staging buffers); the hook changes no metric
    assert run(size, False) == run(size, True)
torch.cuda.synchronize()
rounds = {k: [] for k, _, _ in VARIANTS}
for r in range(ROUNDS):
    for k, fn, units in VARIANTS:
        rounds[k].append(window(fn, units))
res = {"unit": "samples per second", "rounds": {k: [round(x, 1) for x in v] for k, v in rounds.items()}}
res["median"] = md = {k: round(float(np.median(v)), 1) for k, v in rounds.items()}
res["spread"] = {k: round((max(v) - min(v)) / float(np.median(v)), 4) for k, v in rounds.items()}
res["hooked_over_plain"] = {s: round(md[s + "_hooked"] / md[s + "_plain"], 3) for s in SIZES}
res["bytes_read_back_per_sample"] = {s: int(stats[s]) for s in SIZES}

e2 = [torch.cuda.Event(enable_timing=True) for _ in range(2)]


def event_ms(fn, reps=20):
    fn(); torch.cuda.synchronize()
    tot = []
    for _ in range(reps):
        e2[0].record(); fn(); e2[1].record(); torch.cuda.synchronize()
        tot.append(e2[0].elapsed_time(e2[1]))
    return float(np.median(tot))


def wall_ms(fn, reps=10):
    fn(); torch.cuda.synchronize()
    tot = []
    for _ in range(reps):
        t0 = time.perf_counter(); fn(); torch.cuda.synchronize()
        tot.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(tot))


# the hook's parts alone, one batch of B samples: wall clock with a synchronise (host packing included), and the kernels by events
res["hook_parts_ms_per_batch"], res["host_s_per_sample"], res["heat_ms_per_sample"], res["heat_host_s_per_sample"] = {}, {}, {}, {}
for size, (h, w) in SIZES.items():
    chunk = samples[size][:B]
    frames, gts = [s[2] for s in chunk], [s[3] for s in chunk]
    masks = [torch.from_numpy(g).cuda() for g in gts]
    staging = EV._Staging(model.device)
    fdescs, fbytes = VIS._plan_frames([f.shape for f in frames])
    pinned = torch.empty(2 * 3 * h * w * B + 4096, dtype=torch.uint8, pin_memory=True)
    bufs = [VIS.overlays(frames, masks, "pred")[0], VIS.overlays(None, masks, "gt")[0]]

    def readback():
        o = 0
        for b_ in bufs:
            pinned[o: o + b_.numel()].copy_(b_, non_blocking=True)
            o += b_.numel()

    kernels = event_ms(lambda: (VIS.overlays(None, masks, "gt"), VIS.overlays(None, masks, "gt")))       # two launches, no upload in the bracket
    res["hook_parts_ms_per_batch"][size] = {"a_second_upload_would_cost": round(wall_ms(lambda: staging.upload(frames, fdescs, fbytes)), 3),
                                            "overlay_pred_with_upload": round(wall_ms(lambda: VIS.overlays(frames, masks, "pred")), 3),
                                            "two_overlay_launches_device": round(kernels, 4),
                                            "read_back": round(wall_ms(readback), 3),
                                            "picture_bytes": int(sum(b_.numel() for b_ in bufs))}
    # heat maps: four maps per sample (up_c3, up_c4, up_c5, sigm) with the read-back
    feed, _ = EV.prepare_images(frames, H, W, model.device)
    out = model.forward(np.stack([s[0] for s in chunk]), feed, np.array([s[1] for s in chunk], np.int32))
    maps = {k: out[k].float().reshape(B, H, W).contiguous() for k in ("up_c3", "up_c4", "up_c5", "sigm")}
    sizes = [(h, w)] * B

    def heat4():
        return [VIS.heat_maps(m, sizes, sigmoid=True)[0].cpu() for m in maps.values()]

    res["heat_ms_per_sample"][size] = {"four_maps_with_read_back": round(wall_ms(heat4) / B, 3),
                                       "one_launch_device_per_sample": round(event_ms(lambda: VIS.heat_maps(maps["up_c3"], sizes, sigmoid=True)) / B, 4),
                                       "auto_range_device_per_sample": round(event_ms(lambda: VIS.heat_maps(maps["up_c3"], sizes, sigmoid=True, vrange=None)) / B, 4)}
    if not args.short:
        k = 2
        t0 = time.perf_counter()
        hm = EV.predict_masks(model, [s[0] for s in chunk[:k]], [s[1] for s in chunk[:k]], frames[:k])
        pics = [(R.overlay_pred(frames[b], hm[b]), R.overlay_gt(gts[b])) for b in range(k)]
        res["host_s_per_sample"][size] = round((time.perf_counter() - t0) / k, 4)
        got = VIS.unpack_pictures(VIS.overlays(frames[:k], hm, "pred")[0].cpu().numpy(), VIS.plan_pictures([(h, w)] * k)[0])
        assert all(np.array_equal(got[b], pics[b][0]) for b in range(k))
        mh = {kk: v[0].cpu().numpy() for kk, v in maps.items()}
        R.heat(mh["sigm"][:8, :8], 12, 12, sigmoid=True)                    # SciPy's first call imports and warms up
        t0 = time.perf_counter()
        ref = [R.heat(mh[kk], h, w, sigmoid=True)[0] for kk in mh]
        res["heat_host_s_per_sample"][size] = round(time.perf_counter() - t0, 4)
        idx, d = VIS.heat_maps(maps["up_c3"][:1], [(h, w)], sigmoid=True, want="index")
        diff = np.abs(VIS.unpack_pictures(idx.cpu().numpy(), d)[0].astype(int) - ref[0].astype(int))
        assert diff.max() <= 1 and (diff > 0).mean() <= 1e-3, (diff.max(), (diff > 0).mean())
if not args.short:
    res["hooked_over_host"] = {s: round(md[s + "_hooked"] * res["host_s_per_sample"][s], 1) for s in SIZES}
print(json.dumps(res))
