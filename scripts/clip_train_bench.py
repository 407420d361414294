"""Training the video model from raw clips on one box, in one run (config 5: CMPC_video_mm_tgraph_allvec, 320 x 320, L = 20, f16; seeded
synthetic clips of 16 frames of 480 x 640 with a disc annotation), clips per second of
  resident      model.train_step_video on one resident host clip [1, 16, 320, 320, 3]: the parent commit's path, what bench.py config 5 times
  feeder        feed.ClipTrainFeeder.step(): the 5 sampled frames uploaded raw, one cmpc_clip_prep per clip on the side stream
  feeder_acc    the same with accuracy=True (one cmpc_train_accuracy launch per step)
  host_loop     the loop a user had before: hostutil resampling of all 16 frames and the mask on the CPU, then train_step_video
Every variant is warmed up past both backbone-graph captures; then --rounds alternating rounds, each a region bounded by device events
around --steps steps (host_loop: --host-steps).  Median and spread ((max - min) / median) per variant, and the ratios.
usage: python scripts/clip_train_bench.py [--steps 60] [--rounds 3] [--host-steps 2] [--clips 8]"""
import argparse, importlib, json, os, sys
import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pkg = importlib.import_module("cmpc-refseg_amd")
HU = importlib.import_module("cmpc-refseg_amd.hostutil")
FD = importlib.import_module("cmpc-refseg_amd.feed")

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=60)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--host-steps", type=int, default=2)
ap.add_argument("--clips", type=int, default=8)
args = ap.parse_args()
if args.rounds < 3:
    raise SystemExit("--rounds must be >= 3 (median and spread)")
T, H, W, h, w, F = 20, 320, 320, 480, 640, 16
model = pkg.get_segmentation_model("CMPC_video_mm_tgraph_allvec", mode="train", batch_size=1, num_steps=T, H=H, W=W, dtype="f16")
V = model.cfg.vocab_size


def make_clip(i):
    rng = np.random.default_rng(i)
    frames = rng.integers(0, 256, (F, h, w, 3), dtype=np.uint8)
    y, x = np.mgrid[0:h, 0:w]
    mask = (y - rng.uniform(0.3, 0.7) * h) ** 2 + (x - rng.uniform(0.3, 0.7) * w) ** 2 < (rng.uniform(0.1, 0.3) * h) ** 2
    n = int(rng.integers(5, T + 1))
    row = np.zeros(T, np.int64)
    row[T - n:] = rng.integers(1, V, n)              # front-padded ids, as the stored batches hold them
    return frames, mask, None, row


clips = [make_clip(i) for i in range(args.clips)]    # decoded clips held in memory: decoding files is not what is measured
MU = HU.MU


def host_feeds(sample):
    """The driver's feeds from one raw clip on the CPU: every frame and the mask through hostutil's resampler."""
    frames, mask, _, row = sample
    clip = np.stack([HU.img_as_ubyte(HU.resize_and_pad(f, H, W))[..., ::-1].astype(np.float32) - np.float32(MU) for f in frames])
    tgt = (HU.resize_and_pad(mask, H, W) > 0).astype(np.float32)[None, :, :, None]
    return row[None], tgt, np.array([[HU.first_valid_idx(row)]], np.int32), clip[None]


words0, tgt0, vi0, clip0 = host_feeds(clips[0])
clip0, tgt0 = torch.from_numpy(clip0), torch.from_numpy(tgt0)
feeder = FD.ClipTrainFeeder(model, clips, sampler=FD.EpochSampler(len(clips), seed=0), max_hw=(h, w))
state = {"k": 0}


def resident():
    model.train_step_video(words0, None, tgt0, vi0, clip0)


def host_loop():
    wd, tg, vi, cl = host_feeds(clips[state["k"] % len(clips)])
    state["k"] += 1
    model.train_step_video(wd, None, tg, vi, cl)


VARIANTS = [("resident", resident, args.steps), ("feeder", lambda: feeder.step(), args.steps),
            ("feeder_acc", lambda: feeder.step(accuracy=True), args.steps), ("host_loop", host_loop, args.host_steps)]
for name, fn, _ in VARIANTS:                         # warm-up: past both backbone-graph captures (the 3rd and 4th backbone pass)
    for _ in range(1 if name == "host_loop" else 6):
        fn()
torch.cuda.synchronize()
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
rounds = {k: [] for k, _, _ in VARIANTS}
for r in range(args.rounds):
    for name, fn, steps in VARIANTS:
        torch.cuda.synchronize()
        e0.record()
        for _ in range(steps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        rounds[name].append(steps / (e0.elapsed_time(e1) * 1e-3))
feeder.close()
res = {"unit": "clips per second", "config": "CMPC_video_mm_tgraph_allvec 320x320 L=20 f16, raw clips 16 x 480x640",
       "steps_per_round": {k: s for k, _, s in VARIANTS}, "rounds": {k: [round(x, 2) for x in v] for k, v in rounds.items()}}
res["median"] = {k: round(float(np.median(v)), 2) for k, v in rounds.items()}
res["spread"] = {k: round((max(v) - min(v)) / float(np.median(v)), 4) for k, v in rounds.items()}
md = res["median"]
res["ms_per_clip"] = {k: round(1e3 / v, 3) for k, v in md.items()}
res["feeder_over_resident"] = round(md["feeder"] / md["resident"], 3)
res["feeder_acc_over_resident"] = round(md["feeder_acc"] / md["resident"], 3)
res["feeder_over_host_loop"] = round(md["feeder"] / md["host_loop"], 1)
res["accuracy_cost_ms_per_clip"] = round(1e3 / md["feeder_acc"] - 1e3 / md["feeder"], 3)
print(json.dumps(res))
