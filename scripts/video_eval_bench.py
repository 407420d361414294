"""Video evaluation throughput on one box, in one run: config 5 (CMPC_video_mm_tgraph_allvec, 320x320, L=20, f16, batch 1), seeded synthetic
in-memory A2D-like clips (16 uint8 frames, key image = frame 8, mask at the key image's size) at two frame sizes, 480x640 and 360x640:
  evaluator   VideoEvaluator.add / per_sample: one pinned upload + cmpc_eval_prep over the 5 sampled frames -> forward on the device feed
              -> cmpc_eval_mask_iu; overlap off and on, alternated (A/B on the same box, several rounds)
  forward     forward_video_frames on a device-resident feed (the 5 prepared frames), the forward pass alone
  host_loop   trainval_video.py's loop with hostutil: resize_and_pad + img_as_ubyte + image_feed of all 16 frames on the host,
              forward_video, resize_and_crop + SegEval on the host
and the two evaluation kernels' device time per clip, from hipEvents around each launch alone (sources already on the device).
usage: python scripts/video_eval_bench.py [--short] [--out FILE]"""
import argparse, importlib, json, os, statistics, sys, time
import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pkg = importlib.import_module("cmpc-refseg_amd")
EV = importlib.import_module("cmpc-refseg_amd.evaluate")
HU = importlib.import_module("cmpc-refseg_amd.hostutil")
MD = importlib.import_module("cmpc-refseg_amd.model")
L = importlib.import_module("cmpc-refseg_amd._lib")

ap = argparse.ArgumentParser()
ap.add_argument("--short", action="store_true", help="short windows, one A/B round, no host loop")
ap.add_argument("--out", default="")
args = ap.parse_args()
WINDOW = 0.3 if args.short else 2.0
ROUNDS = 1 if args.short else 3
T, H, W, NCLIP = 20, 320, 320, 4
SIZES = [(480, 640), (360, 640)]
model = pkg.get_segmentation_model("CMPC_video_mm_tgraph_allvec", mode="eval", batch_size=1, num_steps=T, H=H, W=W, dtype="f16")
rng = np.random.default_rng(0)


def make_clips(h, w):
    out = []
    for i in range(NCLIP):
        frames = rng.integers(0, 256, (16, h, w, 3), dtype=np.uint8)
        text = np.zeros(T, np.int64)
        n = 5 + 3 * i
        text[T - n:] = rng.integers(1, model.cfg.vocab_size, n)
        mask = rng.random((h, w)) < 0.3
        out.append((text, frames[8].copy(), frames, mask))
    return out


def rate(fn, per_call):
    fn(); torch.cuda.synchronize()
    n, t0 = 0, time.perf_counter()
    while True:
        fn(); n += 1
        if time.perf_counter() - t0 >= WINDOW:
            break
    torch.cuda.synchronize()
    return n * per_call / (time.perf_counter() - t0)


def evaluator_rate(clips, overlap):
    ev = EV.VideoEvaluator(model, overlap=overlap)

    def run():
        for c in clips:
            ev.add(*c)
        ev.per_sample()                    # flushes the pending clip and reads (I, U) back
    return rate(run, len(clips))


def host_loop(clips):
    seg = HU.SegEval(EV.VIDEO_THRESHOLDS)
    for text, im, frames, mask in clips[:2]:
        clip = np.stack([HU.image_feed(HU.img_as_ubyte(HU.resize_and_pad(f, H, W))) for f in frames]).astype(np.float32)
        up = model.forward_video(text[None], None, np.array([[HU.first_valid_idx(text)]], np.int32), clip[None])["up"].float().cpu().numpy()
        seg.add(HU.resize_and_crop((up[0, :, :, 0] >= 1e-9).astype(np.float32), mask.shape[0], mask.shape[1]), mask)
    seg.result()


def kernel_us(clips, reps=50):
    """Device time of one cmpc_eval_prep launch over the 5 sampled frames and one cmpc_eval_mask_iu launch of `up` at the mask's size."""
    text, im, frames, mask = clips[0]
    ims = [np.ascontiguousarray(frames[k]) for k in MD.FRAME_IDX]
    descs, nb = EV.plan_prep([a.shape for a in ims], H, W)
    host = np.zeros(nb, np.uint8)
    for a, d in zip(ims, descs):
        host[d.offset: d.offset + a.size] = a.reshape(-1)
    src = torch.from_numpy(host).cuda()
    proc = torch.empty(5, H, W, 3, dtype=torch.uint8, device="cuda")
    feed = torch.empty(5, H, W, 3, dtype=torch.float32, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    L.call("cmpc_eval_prep", src.data_ptr(), nb, descs, 5, H, W, proc.data_ptr(), feed.data_ptr(), st)
    up = model.forward_video_frames(text, HU.first_valid_idx(text), feed)["up"].float()
    md, mb = EV.plan_masks([mask.shape], H, W)
    gt = torch.from_numpy(np.ascontiguousarray(np.pad((mask != 0).astype(np.uint8).reshape(-1), (0, mb - mask.size)))).cuda()
    iu = torch.empty(1, 2, dtype=torch.int64, device="cuda")
    launches = {"prep": lambda: L.call("cmpc_eval_prep", src.data_ptr(), nb, descs, 5, H, W, proc.data_ptr(), feed.data_ptr(), st),
                "mask_iu": lambda: L.call("cmpc_eval_mask_iu", up.data_ptr(), L.EVAL_F32, 1, H, W, 1e-9, gt.data_ptr(), mb, md, iu.data_ptr(),
                                          None, st)}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    out = {}
    for k, f in launches.items():
        f(); torch.cuda.synchronize()
        ts = []
        for _ in range(reps):
            e0.record(); f(); e1.record(); e1.synchronize()
            ts.append(1e3 * e0.elapsed_time(e1))
        out[k] = statistics.median(ts)
    return out


lines = []
for h, w in SIZES:
    clips = make_clips(h, w)
    feed_dev, _ = EV.prepare_images(list(clips[0][2][list(MD.FRAME_IDX)]), H, W)
    t0 = clips[0][0]
    vi0 = HU.first_valid_idx(t0)
    res = {"frame_size": "%dx%d" % (h, w), "forward_clips_per_s": rate(lambda: model.forward_video_frames(t0, vi0, feed_dev), 1)}
    ab = {False: [], True: []}
    for _ in range(ROUNDS):
        for ov in (False, True):
            ab[ov].append(evaluator_rate(clips, ov))
    res["evaluator_clips_per_s_overlap_off"] = [round(x, 2) for x in ab[False]]
    res["evaluator_clips_per_s_overlap_on"] = [round(x, 2) for x in ab[True]]
    off, on = statistics.median(ab[False]), statistics.median(ab[True])
    res["overlap_gain"] = on / off - 1.0
    res["evaluator_clips_per_s"] = on if EV.VIDEO_OVERLAP else off
    res["ratio_evaluator_to_forward"] = res["evaluator_clips_per_s"] / res["forward_clips_per_s"]
    if not args.short:
        res["host_loop_clips_per_s"] = rate(lambda: host_loop(clips), 2)
    k = kernel_us(clips)
    res["prep_us_per_clip"], res["mask_iu_us_per_clip"] = k["prep"], k["mask_iu"]
    res["kernels_fraction_of_forward"] = (k["prep"] + k["mask_iu"]) * 1e-6 * res["forward_clips_per_s"]
    line = json.dumps({a: round(b, 4) if isinstance(b, float) else b for a, b in res.items()})
    print(line, flush=True)
    lines.append(line)
if args.out:
    with open(args.out, "w") as f:
        f.write("# scripts/video_eval_bench.py: config 5 (CMPC_video_mm_tgraph_allvec, f16, 320x320, L=20, batch 1), synthetic A2D-like clips, "
                "one MI355X\n# default overlap = %s\n" % EV.VIDEO_OVERLAP)
        f.write("\n".join(lines) + "\n")
