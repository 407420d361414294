"""The video driver's train loop (CMPC_video/trainval_video.py:56-133) over a folder of train samples in build_A2D_batches.py's layout
(:137-143): one .npz per clip with `frames` uint8 [16, H, W, 3], `mask_batch` bool [H, W], `text_batch` front-padded ids [T].  The clips
go through feed.ClipTrainFeeder -- only the 5 sampled frames are uploaded, prepared on the GPU and staged a clip ahead on a side stream --
and the loss / accuracy lines the driver prints every 100 iterations come from hostutil.TrainLog on the step's device scalars and
accuracy counts, read only when a line is due.  A snapshot is written every --snapshot iterations and at the end.
usage: python examples/train_video_clips.py --data DIR [--iters 1000] [--snapshot 500] [--out DIR] [--restore PATH] [--lr 0.00025]
                                            [--iters-per-log 100] [--no-shuffle] [--H 320 --W 320 --T 20] [--model-kwargs JSON]"""
import argparse, glob, importlib, json, os, sys
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--data", required=True, help="a folder of .npz train samples (frames, mask_batch, text_batch)")
ap.add_argument("--iters", type=int, default=1000)
ap.add_argument("--snapshot", type=int, default=500)
ap.add_argument("--out", default="/tmp/cmpc_video_ckpt")
ap.add_argument("--restore", default="", help="a snapshot to start from (the driver restores the DeepLab weights here)")
ap.add_argument("--lr", type=float, default=0.00025)
ap.add_argument("--lr-decay-step", type=int, default=800000)
ap.add_argument("--iters-per-log", type=int, default=100)
ap.add_argument("--no-shuffle", action="store_true")
ap.add_argument("--seed", type=int, default=0)
ap.add_argument("--finetune", action="store_true")
ap.add_argument("--H", type=int, default=320)
ap.add_argument("--W", type=int, default=320)
ap.add_argument("--T", type=int, default=20)
ap.add_argument("--model-kwargs", type=json.loads, default={}, metavar="JSON",
                help='further LSTM_model keywords as a JSON object, e.g. \'{"dtype": "f32"}\' (the tests pass a shrunken graph this way)')
args = ap.parse_args()

pkg = importlib.import_module("cmpc-refseg_amd")
CK = importlib.import_module("cmpc-refseg_amd.checkpoint")
HU = importlib.import_module("cmpc-refseg_amd.hostutil")
FD = importlib.import_module("cmpc-refseg_amd.feed")
NAME = "CMPC_video_mm_tgraph_allvec"


class Clips:
    """Train samples by file, in sorted order; a file is read when the feeder's loader threads ask for it."""

    def __init__(self, folder):
        self.files = sorted(glob.glob(os.path.join(folder, "*.npz")))
        if not self.files:
            raise SystemExit("no .npz samples in %s" % folder)

    def __len__(self):
        return len(self.files)

    def __getitem__(self, i):
        z = np.load(self.files[i])
        return z["frames"], z["mask_batch"], None, np.asarray(z["text_batch"]).reshape(-1).astype(np.int64)


extra = {k: tuple(v) if isinstance(v, list) else v for k, v in args.model_kwargs.items()}
model = pkg.get_segmentation_model(NAME, mode="train", batch_size=1, num_steps=args.T, H=args.H, W=args.W, start_lr=args.lr,
                                   lr_decay_step=args.lr_decay_step, finetune=args.finetune, **extra)
if args.restore:
    CK.Saver().restore(model, args.restore)
data = Clips(args.data)
saver = CK.Saver(max_to_keep=4)
os.makedirs(args.out, exist_ok=True)
log = HU.TrainLog(iters_per_log=args.iters_per_log)
sampler = FD.EpochSampler(len(data), shuffle=not args.no_shuffle, seed=args.seed)
with FD.ClipTrainFeeder(model, data, sampler=sampler, max_hw=(args.H, args.W)) as feeder:
    for n_iter in range(args.iters):
        step, scal = feeder.step(accuracy=True)
        log.add(n_iter, scal["loss_last"], scal["learning_rate"], scal["accuracy_counts"])      # cls_loss = the last level's loss (vid:571)
        for line in log.lines(n_iter):
            print(line, flush=True)
        if (n_iter + 1) % args.snapshot == 0 or (n_iter + 1) >= args.iters:
            print("snapshot saved to " + saver.save(model, os.path.join(args.out, "a2d_iter"), global_step=n_iter + 1), flush=True)
print("Optimization done.")
