"""The video model over a whole video on one box, in one run (config 5: CMPC_video_mm_tgraph_allvec, 320 x 320, L = 20, f16; a seeded
synthetic video of 60 frames of 480 x 640; E = 1 and E = 3 expressions; masks at the frame's size):
  clip_la<k>   segment.ClipSegmenter.run with lookahead k = 0 (backbone and heads do not overlap), 1, 2: each frame through the backbone
               once, one cmpc_taps_copy gather per frame, one head per (frame, expression), cmpc_eval_mask_out, pinned ring
  parent       the only route before ClipSegmenter: one model.forward_video_frames call per (frame, expression) on device-resident
               prepared frames (5 backbone frames per result; no mask is produced or copied out, which favours this side)
Three alternating rounds of device-synchronised windows (>= 2 s each) after a warm-up of every variant; results ((frame, expression)
pairs) per second.  Then cmpc_taps_copy as the gather and as the scatter and the head's forward pass on the gathered taps, bracketed
by events.
usage: python scripts/clip_segment_bench.py [--short]"""
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
WINDOW, ROUNDS = (0.3, 1) if args.short else (2.0, 3)
T, H, W, h, w, F = 20, 320, 320, 480, 640, 60
rng = np.random.default_rng(0)
model = pkg.get_segmentation_model("CMPC_video_mm_tgraph_allvec", mode="eval", batch_size=1, num_steps=T, H=H, W=W, dtype="f16")
frames = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for _ in range(F)]
exprs = []
for n in (5, 12, 20):
    ids = np.zeros(T, np.int32)
    ids[:n] = rng.integers(1, model.cfg.vocab_size, n)
    exprs.append((ids, n))
segs = {k: SG.ClipSegmenter(model, copy=False, lookahead=k, ring=32) for k in (0, 1, 2)}


def clip(k, E):
    n = 0
    for _ in segs[k].run(frames, exprs[:E]):
        n += 1
    assert n == F * E and segs[k].stats["backbone_passes"] == F // 5


feed_all = torch.cat([EV.prepare_images(frames[s: s + 20], H, W)[0] for s in range(0, F, 20)])
front = []
for ids, n in exprs:
    wd = np.zeros((1, T), np.int64)
    wd[0, T - n:] = ids[:n]
    front.append((wd, np.array([[T - n]], np.int32)))
sampled = [torch.tensor(SG.sampled_frames(f, F), device=model.device) for f in range(F)]


def parent(E):
    for f in range(F):
        fr = feed_all.index_select(0, sampled[f])
        for wd, vi in front[:E]:
            model.forward_video_frames(wd, vi, fr)


def window(fn, units):
    torch.cuda.synchronize()
    n, t0 = 0, time.perf_counter()
    while True:
        fn(); n += 1
        if time.perf_counter() - t0 >= WINDOW:
            break
    torch.cuda.synchronize()
    return n * units / (time.perf_counter() - t0)


VARIANTS = []
for E in (1, 3):
    VARIANTS += [("clip_la%d_E%d" % (k, E), (lambda k=k, E=E: clip(k, E)), F * E) for k in (0, 1, 2)]
    VARIANTS.append(("parent_E%d" % E, (lambda E=E: parent(E)), F * E))
for _, fn, _ in VARIANTS:               # every variant once (backbone graphs, workspaces, staging buffers, rings)
    fn()
torch.cuda.synchronize()
rounds = {k: [] for k, _, _ in VARIANTS}
for r in range(ROUNDS):
    for k, fn, units in VARIANTS:
        rounds[k].append(window(fn, units))
res = {"unit": "(frame, expression) results per second", "rounds": {k: [round(x, 1) for x in v] for k, v in rounds.items()}}
res["median"] = {k: round(float(np.median(v)), 1) for k, v in rounds.items()}
res["spread"] = {k: round((max(v) - min(v)) / float(np.median(v)), 4) for k, v in rounds.items()}
md = res["median"]
for E in (1, 3):
    for k in (0, 1, 2):
        res["clip_la%d_E%d_over_parent" % (k, E)] = round(md["clip_la%d_E%d" % (k, E)] / md["parent_E%d" % E], 3)

# cmpc_taps_copy both ways and the head on the gathered taps, bracketed by events (device time per call)
st = segs[SG.CLIP_LOOKAHEAD].stage
e = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
main = torch.cuda.current_stream(model.device)


def event_ms(fn, reps=30):
    fn(); torch.cuda.synchronize()
    tot = []
    for _ in range(reps):
        e[0].record(); fn(); e[1].record(); torch.cuda.synchronize()
        tot.append(e[0].elapsed_time(e[1]))
    return float(np.median(tot))


def gather():
    for j, g in enumerate((3, 7, 11, 15, 18)):
        st._idx_b[j] = g
    st._copy(3, st._gath_p, st._cache_p, st._bytes, 5, st._seq, st._idx_b, 5, st.ring, main)


def scatter():
    for j, g in enumerate((20, 21, 22, 23, 24)):
        st._idx_a[j] = g
    st._copy(3, st._cache_p, st._gath_p, st._bytes, 5, st._idx_a, st._seq, st.ring, 5, main)


st.set_expressions(exprs)
words, sl = st.words[2]
with torch.no_grad():
    res["gather_ms_per_call"] = round(event_ms(gather), 4)
    res["scatter_ms_per_call"] = round(event_ms(scatter), 4)
    res["head_ms_per_call"] = round(event_ms(lambda: model.head_video(st.gathered, words, sl)), 4)
    fr = feed_all.index_select(0, sampled[30])
    res["forward_video_frames_ms_per_call"] = round(event_ms(lambda: model.forward_video_frames(front[2][0], front[2][1], fr)), 4)
res["copy_bytes_per_call"] = 2 * 5 * sum(st.bytes)
res["gather_GBps"] = round(res["copy_bytes_per_call"] / res["gather_ms_per_call"] / 1e6, 1)
res["gather_over_head"] = round(res["gather_ms_per_call"] / res["head_ms_per_call"], 4)
res["scatter_over_head"] = round(res["scatter_ms_per_call"] / res["head_ms_per_call"], 4)
print(json.dumps(res))
