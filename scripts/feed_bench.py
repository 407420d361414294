"""Training throughput from raw samples on one box, in one run (config-2 CMPC_model, f16, B=8, seeded synthetic in-memory raw samples:
uint8 images, colour-coded annotations, sentences), per source size (480x640: the evaluator bench's; 720x1280: a Refer-YouTube-VOS frame):
  resident    train_step on one prepared device-resident batch (what bench.py measures)
  feeder      the same model driven by TrainFeeder.step(), and with lookahead=True (the staged batch behind it as next_im)
  host_loop   feeds made by hostutil.train_sample in the reference's arrangement: one prefetch thread, a queue of samples
and the prep's device time per batch from hipEvents around copy + cmpc_train_prep on an idle device.  Byte model per sample (every
byte read or written once): eval_prep h*w*3 + H*W*3*4, train_target h*w*c + H*W*4; host-to-device copy h*w*(3 + c) + ids.
usage: python scripts/feed_bench.py [--short] [--only resident|feeder] [--sizes 480x640,720x1280]"""
import argparse, importlib, json, os, queue, sys, threading, time
import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bench import synth_batch
pkg = importlib.import_module("cmpc-refseg_amd")
FD = importlib.import_module("cmpc-refseg_amd.feed")
HU = importlib.import_module("cmpc-refseg_amd.hostutil")

ap = argparse.ArgumentParser()
ap.add_argument("--short", action="store_true", help="a 0.5 s window and no host loop (profiling runs)")
ap.add_argument("--only", choices=("resident", "feeder"), default=None)
ap.add_argument("--sizes", default="480x640,720x1280")
args = ap.parse_args()
WINDOW = 0.5 if args.short else 3.0
B, T, H, W = 8, 20, 320, 320
KEY = FD.REFVOS_OBJECT_COLOR["2"]
VOCAB = {w: i for i, w in enumerate(["<pad>", "<unk>"] + ["w%d" % i for i in range(998)])}
model = pkg.get_segmentation_model("CMPC_model", batch_size=B, num_steps=T, vf_h=H // 8, vf_w=W // 8, H=H, W=W, mode="train", dtype="f16")
dev = model.device


def raw_samples(h, w, n):
    rng = np.random.default_rng(h)
    y, x = np.mgrid[0:h, 0:w]
    out = []
    for _ in range(n):
        im = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        cy, cx, r = rng.uniform(0, h), rng.uniform(0, w), rng.uniform(0.1, 0.3) * h
        ann = rng.integers(0, 6, (h, w, 3), dtype=np.uint8)
        ann[(y - cy) ** 2 + (x - cx) ** 2 < r * r] = KEY
        sent = " ".join("w%d" % k for k in rng.integers(0, 998, int(rng.integers(3, T + 1))))
        out.append((im, ann, KEY, sent))
    return out


def window(step, per_call, warm):
    for _ in range(warm):
        step()
    torch.cuda.synchronize()
    n, t0 = 0, time.perf_counter()
    while time.perf_counter() - t0 < WINDOW:
        step(); n += 1
    torch.cuda.synchronize()
    return n * per_call / (time.perf_counter() - t0)


res = {}
# the set-up steps bench.py takes (workspaces, MIOpen's search, the two backbone graphs) and its resident loop
w_, im_, sl_, tg_ = (torch.from_numpy(a).to(dev) for a in synth_batch(B, T, H, W, model.cfg.vocab_size, seed=0))
torch.cuda.synchronize()
ready = torch.cuda.Event(); ready.record()
for _ in range(6):
    model.train_step(w_, im_, tg_, sl_, ready=ready)
torch.cuda.synchronize()
if args.only in (None, "resident"):
    res["resident_images_per_s"] = window(lambda: model.train_step(w_, im_, tg_, sl_, ready=ready), B, 5)
    res["resident_lookahead_images_per_s"] = window(lambda: model.train_step(w_, im_, tg_, sl_, ready=ready, next_im=im_, next_ready=ready), B, 5)

for size in ([] if args.only == "resident" else args.sizes.split(",")):
    h, w = (int(v) for v in size.split("x"))
    data = raw_samples(h, w, 4 * B)
    for look in (False, True):
        with FD.TrainFeeder(model, data, sampler=FD.EpochSampler(len(data), seed=1), vocab=VOCAB, max_hw=(h, w), lookahead=look) as fd:
            res["feeder%s_images_per_s_%s" % ("_lookahead" if look else "", size)] = window(fd.step, B, 8)
    # copy + prep alone on an idle device: events around stage() on the feeder's stream
    with FD.TrainFeeder(model, data, sampler=FD.EpochSampler(len(data), seed=1), vocab=VOCAB, max_hw=(h, w)) as fd:
        e0, e1, tot, reps = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True), 0.0, 10
        for i in range(reps + 2):
            torch.cuda.synchronize()
            fd._release_current()
            hb = fd.pipe.get()
            e0.record(fd.stage.stream)
            fd._current = fd.stage.stage(hb)
            e1.record(fd.stage.stream)
            torch.cuda.synchronize()
            tot += e0.elapsed_time(e1) if i >= 2 else 0.0
            fd._recycle()
        res["copy_plus_prep_ms_per_batch_%s" % size] = tot / reps
    res["bytes_eval_prep_per_batch_%s" % size] = B * (h * w * 3 + H * W * 12)
    res["bytes_train_target_per_batch_%s" % size] = B * (h * w * 3 + H * W * 4)
    res["bytes_h2d_per_batch_%s" % size] = B * (h * w * 6 + T * 4 + 4)
    if not args.short and args.only is None:
        # the reference's arrangement: one prefetch thread fills a queue with finished samples (DataReader, prefetch_num=8)
        q, stop = queue.Queue(maxsize=8), threading.Event()

        def prefetch():
            k = 0
            while not stop.is_set():
                im, ann, key, sent = data[k % len(data)]
                feed, tgt = HU.train_sample(im, ann, key, H, W)
                ids, n = HU.preprocess_sentence_lstm(sent, VOCAB, T)
                while not stop.is_set():
                    try:
                        q.put((np.asarray(ids, np.int32), feed, tgt, n), timeout=0.1); break
                    except queue.Full:
                        pass
                k += 1

        th = threading.Thread(target=prefetch, daemon=True); th.start()

        def host_step():
            s = [q.get() for _ in range(B)]
            model.train_step(np.stack([x[0] for x in s]), np.stack([x[1] for x in s]), np.stack([x[2] for x in s]), np.array([x[3] for x in s], np.int32))

        host_step(); torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(3):
            host_step()
        torch.cuda.synchronize()
        res["host_loop_images_per_s_%s" % size] = 3 * B / (time.perf_counter() - t0)
        stop.set(); th.join()
    if "resident_images_per_s" in res:
        res["ratio_feeder_to_resident_%s" % size] = res["feeder_images_per_s_%s" % size] / res["resident_images_per_s"]
        res["ratio_feeder_lookahead_to_resident_%s" % size] = res["feeder_lookahead_images_per_s_%s" % size] / res["resident_images_per_s"]
print(json.dumps({k: round(v, 4) if isinstance(v, float) else v for k, v in res.items()}))
