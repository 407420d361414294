#!/usr/bin/env python3
"""bench.py -- images/sec of the CMPC train step (backbone forward + HIP head forward/backward +
gradient all-reduce + fused Adam) at 320x320, L=20, B=8 per GPU, synthetic data.

  python bench.py --gpus 1 --steps 20 --warmup 5
  python bench.py --gpus 1 --steps 20 --warmup 5 --dump-outputs bench_out/run1   # + the last timed step's outputs as .npy
  python bench.py --gpus 1 --steps 20 --warmup 5 --full                          # + everything beyond the headline figure
  python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
         bench.py --gpus N --steps K --warmup W

Prints ONE JSON line on rank 0 (contract in the project brief): metric/value/unit, ms_per_step.  A plain run does only what that
headline figure needs: set-up, W warm-up steps, K timed steps, --dump-outputs, the line.  --full adds, after the timed steps:
`roofline` for the dominant kernel family (the 16-bit MFMA gemm_nt, timed live with hipEvents on the launch stream inside the
library: cmpc_kernel_timing) with the per-kernel HBM / overall roofline beside it, the forward-only rate, the bf16-storage rate,
BASELINE configs 4 and 5, and `cpu_baseline` (the oracle -- a torch-CPU fp32 restatement of the reference graph, since TensorFlow
cannot run here -- timed on the host's cores on a bounded sample).  The --no-* switches leave single parts out of a --full run.
"""
from __future__ import annotations

import argparse
import importlib
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

MU = np.array((104.00698793, 116.66876762, 122.67891434), dtype=np.float32)


def synth_batch(B, T, H, W, vocab, seed):
    """SURVEY.md 8d synthetic inputs: uint8 image -> BGR minus mean; seq_len ~ U{3..T} (sample 0 = T);
    words ~ U{4..V-1}, 0-padded at the end; one random rectangle per image as the mask."""
    rng = np.random.default_rng(seed)
    im = rng.integers(0, 256, size=(B, H, W, 3), dtype=np.uint8).astype(np.float32)[:, :, :, ::-1] - MU
    seq_len = rng.integers(3, T + 1, size=(B,)).astype(np.int32)
    seq_len[0] = T
    words = np.zeros((B, T), dtype=np.int32)
    for b in range(B):
        words[b, :seq_len[b]] = rng.integers(4, vocab, size=(seq_len[b],))
    target = np.zeros((B, H, W, 1), dtype=np.float32)
    for b in range(B):
        hh, ww = rng.integers(40, 201, size=2) if min(H, W) >= 320 else rng.integers(H // 8, H // 2 + 1, size=2)
        y0, x0 = rng.integers(0, H - hh + 1), rng.integers(0, W - ww + 1)
        target[b, y0:y0 + hh, x0:x0 + ww, 0] = 1.0
    return words, np.ascontiguousarray(im), seq_len, target


def cpu_baseline(args):
    """The oracle (test infrastructure) timed as the CPU baseline on this box's host cores: BASELINE.json config 2's train step
    (backbone forward + head forward/backward + TF-Adam, batch of `cpu_images`) -- the `value` -- and config 1 (4 images, forward
    only: the reference's own CPU-runnable case) next to it."""
    from oracle import cmpc_torch as O
    # the GPU box gives one GPU a 16-core CPU share; os.cpu_count() reports the whole host
    try:
        nthreads = len(os.sched_getaffinity(0))
    except AttributeError:
        nthreads = os.cpu_count() or 1
    nthreads = max(1, min(nthreads, 16))
    torch.set_num_threads(nthreads)
    B = args.cpu_images
    cfg = O.Cfg(batch_size=B)
    hp, bp = O.init_head_params(cfg), O.init_backbone_params(cfg)
    w, im, sl, tg = synth_batch(B, cfg.num_steps, cfg.H, cfg.W, cfg.vocab_size, 0)
    w, im, sl, tg = map(torch.from_numpy, (w, im, sl, tg))
    opt = O.TFAdam(hp)
    log(f"cpu baseline: {nthreads} threads, {B} image(s)")
    best = None
    for step in range(args.cpu_steps):
        t0 = time.time()
        with torch.no_grad():
            feats = O.backbone_forward(bp, im, cfg)
        O.train_step(hp, opt, step, feats, w, sl, tg, cfg)
        dt = time.time() - t0
        log(f"cpu baseline step {step}: {dt:.1f} s")
        best = dt if best is None else min(best, dt)
    # config 1: 4 images, forward only
    cfg4 = O.Cfg(batch_size=4)
    hp4 = O.init_head_params(cfg4)
    w4, im4, sl4, _ = map(torch.from_numpy, synth_batch(4, cfg4.num_steps, cfg4.H, cfg4.W, cfg4.vocab_size, 7))
    best4 = None
    for _ in range(2):
        t0 = time.time()
        with torch.no_grad():
            O.head_forward(hp4, O.backbone_forward(bp, im4, cfg4), w4, sl4, cfg4)
        d4 = time.time() - t0
        best4 = d4 if best4 is None else min(best4, d4)
    log(f"cpu baseline forward (4 images): {best4:.1f} s")
    return {"value": B / best, "unit": "images/sec", "cores": nthreads, "kind": "port",
            "forward_only_config1": {"images_per_sec": 4 / best4, "s_per_batch": best4, "what": "BASELINE config 1: 4 images 320x320 L=20, forward only"},
            "sample": f"best of {args.cpu_steps} train steps (backbone fwd + head fwd/bwd + Adam) on a batch of {B} synthetic "
                      f"320x320 L=20 images, torch-CPU fp32 restatement of the TF graph (TensorFlow unavailable), {best:.1f} s/step"}


def config4_rate(pkg, dev, args, B=8):
    """BASELINE config 4: CMPCv5_BiLSTM_HSV_model 512x512 L=25, B images, f16 storage, batch-norm in training mode."""
    T, H, W = 25, 512, 512
    m = pkg.get_segmentation_model("CMPCv5_BiLSTM_HSV_model", batch_size=B, num_steps=T, vf_h=64, vf_w=64, H=H, W=W, mode="train", dtype=args.dtype, device=str(dev))
    w, im, sl, tg = (torch.from_numpy(x).to(dev) for x in synth_batch(B, T, H, W, m.cfg.vocab_size, seed=4))
    torch.cuda.synchronize()
    for _ in range(6 + args.warmup):
        m.train_step(w, im, tg, sl)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        _, scal = m.train_step(w, im, tg, sl)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    for _ in range(2):
        m.forward(w, im, sl)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        m.forward(w, im, sl)
    torch.cuda.synchronize()
    df = time.perf_counter() - t0
    out = {"workload": f"CMPCv5_BiLSTM_HSV_model 512x512 B={B} L=25 {args.dtype} storage, ResNet-101 backbone (frozen, taps res2b / res4b22 / res5c), "
                       "batch-norm in training mode, random-init weights", "images_per_sec": B * args.steps / dt, "ms_per_step": 1e3 * dt / args.steps,
           "forward_only_images_per_sec": B * args.steps / df, "forward_only_ms": 1e3 * df / args.steps, "final_loss": float(scal["loss_all"]),
           "head_launches_per_step": m.eng.launch_count(), "grad_nonfinite": m.grad_nonfinite()}
    del m
    torch.cuda.empty_cache()
    return out


def config5_rate(pkg, dev, args):
    """BASELINE config 5: CMPC_video_mm_tgraph_allvec, one 16-frame 320x320 clip per step (the reference graph is batch 1), L=20, ResNet-101
    on the 5 sampled frames, f16 storage."""
    m = pkg.get_segmentation_model("CMPC_video_mm_tgraph_allvec", batch_size=1, mode="train", dtype=args.dtype, device=str(dev))
    g = torch.Generator().manual_seed(5)
    words = torch.zeros(1, 20, dtype=torch.int64)
    words[0, 20 - 9:] = torch.randint(1, m.cfg.vocab_size, (9,), generator=g)             # front-padded, as the reference driver feeds them
    vi = torch.tensor([[11]], dtype=torch.int32)
    clip = (torch.rand(1, 16, 320, 320, 3, generator=g) * 255 - 120).to(dev)
    tg = (torch.rand(1, 320, 320, 1, generator=g) < 0.2).float().to(dev)
    torch.cuda.synchronize()                                                              # words / valid_idx stay host arrays: they are feed_dict values in the reference driver
    for _ in range(6 + args.warmup):
        m.train_step_video(words, None, tg, vi, clip)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        _, scal = m.train_step_video(words, None, tg, vi, clip)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    for _ in range(2):
        m.forward_video(words, None, vi, clip)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        m.forward_video(words, None, vi, clip)
    torch.cuda.synchronize()
    df = time.perf_counter() - t0
    out = {"workload": f"CMPC_video_mm_tgraph_allvec: one 16-frame 320x320 clip (5 sampled frames through ResNet-101, frozen), L=20, batch 1, "
                       f"{args.dtype} storage, random-init weights", "clips_per_sec": args.steps / dt, "ms_per_step": 1e3 * dt / args.steps,
           "forward_only_clips_per_sec": args.steps / df, "forward_only_ms": 1e3 * df / args.steps, "final_loss": float(scal["loss_all"]),
           "head_launches_per_step": m.eng.launch_count(), "grad_nonfinite": m.grad_nonfinite()}
    del m
    torch.cuda.empty_cache()
    return out


def stage_model(B, es=2, N=1600, T=20, C=1000, M=500, H=320, W=320, n_params=76055608):
    """Algorithmic work per train step of every launch name of CMPC_model (3 levels, 6 exchange modules, 3 ConvLSTM steps; SURVEY 8d's
    compulsory-traffic model: a stage reads its unique inputs once and writes its outputs once; a kernel that passes over its input
    twice shows up as a lower fraction).  name -> ("hbm", bytes) | ("mfma", flops) | ("latency", 0): the small language-side launches
    ([B, .] / [B*T, .] rows) and the partial-row folds are launch-latency bound and carry no byte model."""
    R, Cp, Mp, Tp = B * N, 1024, 512, 64
    MC, MM, AT, AT2, UP = R * Cp * es, R * Mp * es, R * Tp * 4, R * Tp * es, B * H * W * 4
    hbm = {
        "l2norm_rows_fwd": 3 * 2 * MC, "l2norm_rows_bwd": 3 * 3 * MC,
        "mutan_fwd": 3 * 6 * MC, "mutan_bwd": 3 * 12 * MC,
        "graph_softmax_fwd": 3 * (3 * AT + 2 * AT2), "graph_softmax_bwd": 3 * (6 * AT + AT2),
        "lowrank_nn": 3 * (AT2 + MC) + 6 * (AT2 + 2 * MC),
        "sample_stats": 6 * MC, "gconv_pre_fwd": 3 * 3 * MC, "gconv_post_fwd": 3 * 2 * MC, "gconv_post_bwd": 3 * 4 * MC, "gconv_pre_bwd": 3 * 6 * MC,
        "score_conv_fwd": 4 * MM, "score_conv_bwd": 3 * 3 * MM + 2 * MM, "upsample_fwd": 4 * 2 * UP + UP, "upsample_loss_bwd": 4 * 2 * UP,
        "act_bwd": 3 * 3 * MM + (3 + 15 + 3) * MC + 12 * MM + 3 * AT,
        "rowdot1": 12 * MM, "wcolsum": 12 * MM, "rank1_update": 6 * 2 * MM,
        "exchange_combine_fwd": 6 * 4 * MM, "exchange_combine_bwd": 6 * 7 * MM, "add_n": 6 * 4 * MM,
        "convlstm_a": 3 * 6 * MM, "convlstm_b": 3 * 7 * MM, "convlstm_c": 3 * 4 * MM, "convlstm_bwd": 3 * 13 * MM,
        "adam_step": 7 * 4 * n_params, "pack_weights": 8 * n_params,
    }
    macs_img = (2048 + 1024 + 512) * C * N + 15 * 1008 * C * N + 3 * C * C * N + 3 * 2008 * M * N + 12 * M * M * N + 3 * (2 * M) * (4 * M) * N
    mfma = {"gemm_tn_grouped": 2.0 * macs_img * B, "conv_nhwc": 138.2e9 * B}       # dW of every visual weight; frozen backbone forward
    out = {k: ("hbm", float(v)) for k, v in hbm.items()}
    out.update({k: ("mfma", float(v)) for k, v in mfma.items()})
    return out


def launch_trace(pkg, model, steps, feeds):
    """Per-name kernel time of `steps` train steps with every launch on ONE stream (cmpc_launch_trace: an event behind every launch of the
    library; the backbone eager instead of replayed from its graph so that its convolutions are launches of the library too)."""
    import ctypes as C
    lib = pkg._lib.load()
    w, im, tg, sl = feeds
    model.set_lanes(1)
    graph_on, model._bb_graph_on = model._bb_graph_on, False
    for _ in range(2):
        model.train_step(w, im, tg, sl)
    torch.cuda.synchronize()
    pkg._lib.call("cmpc_launch_trace", 1, C.c_void_p(torch.cuda.current_stream().cuda_stream))
    for _ in range(steps):
        model.train_step(w, im, tg, sl)
    torch.cuda.synchronize()
    name, ms, n = C.c_char_p(), C.c_double(), C.c_int64()
    out, i = {}, 0
    while lib.cmpc_launch_trace_read(i, C.byref(name), C.byref(ms), C.byref(n)) == 0:
        out[name.value.decode()] = (ms.value / steps, n.value / steps)
        i += 1
    pkg._lib.call("cmpc_launch_trace", 0, None)
    model._bb_graph_on = graph_on
    return out


def log(msg):
    print(f"[bench {time.strftime('%H:%M:%S')}] {msg}", file=sys.stderr, flush=True)


DUMP_SAMPLE = 1 << 21        # elements of the flat parameter / gradient buffers kept by --dump-outputs (8 MB each as float32)
DUMP_LIMIT = 64 << 20        # bytes written by --dump-outputs, all files together


def dump_outputs(model, step, scal, out_dir):
    """--dump-outputs: what the LAST timed train step computed, as float32 / float64 .npy files, so that two builds can be compared
    output for output: the scalars train_step returned (losses, mean IoU, learning rate, global step), its forward fetches (pred, up,
    sigm) and a fixed, seeded sample of the updated parameters and of the step's gradients (loss scale divided out; the full flat
    buffers hold ~76M elements each)."""
    torch.cuda.synchronize()
    eng = model.eng
    out = {"global_step": np.float64(step)}
    out.update({k: np.float64(float(v)) for k, v in scal.items()})
    for k in ("pred", "up", "sigm"):
        out[k] = eng.tap(k).detach().float().cpu().numpy()
    idx = np.sort(np.random.default_rng(0).choice(eng.total, size=min(DUMP_SAMPLE, eng.total), replace=False))
    ix = torch.from_numpy(idx).to(eng.params.device)
    out["params_sample"] = eng.params[ix].float().cpu().numpy()
    out["grads_sample"] = (eng.grads[ix].double() / eng.loss_scale).float().cpu().numpy()
    nbytes = sum(a.nbytes for a in out.values())
    if nbytes > DUMP_LIMIT:
        raise SystemExit(f"--dump-outputs: {nbytes} bytes exceed the {DUMP_LIMIT} byte limit")
    os.makedirs(out_dir, exist_ok=True)
    for k, a in out.items():
        np.save(os.path.join(out_dir, k + ".npy"), a)
    log(f"dumped {len(out)} arrays ({nbytes / 2**20:.1f} MB) of the last timed step to {out_dir}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=50)        # warm-up 10, time 50
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--batch", type=int, default=8, help="images per GPU")
    ap.add_argument("--dtype", default="f16", choices=("f16", "bf16", "f32"),
                    help="storage of maps / visual GEMM operands. f16 and bf16 run the same MFMA pipelines at the same rate; f16 (default) is "
                         "the one that meets BASELINE's 1e-4 mean-IoU bar (bf16 storage: up to 1.6e-4), see tests/test_gpu_parity.py")
    ap.add_argument("--full", action="store_true",
                    help="after the headline figure, also measure what else the line can report: per-kernel timing and roofline, forward-only "
                         "rate, bf16-storage rate, BASELINE configs 4 and 5, CPU baseline (off by default; the --no-* switches trim it)")
    ap.add_argument("--no-alt-dtype", action="store_true", help="skip the bf16-storage rate reported next to the f16 one")
    ap.add_argument("--cpu-images", type=int, default=8)
    ap.add_argument("--cpu-steps", type=int, default=2)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-kernel-timing", action="store_true")
    ap.add_argument("--no-forward-only", action="store_true", help="skip the forward-only rate (profiling runs)")
    ap.add_argument("--model", default="CMPC_model", choices=("CMPC_model", "CMPCv5_BiLSTM_model", "CMPCv5_BiLSTM_HSV_model"),
                    help="CMPC_model = BASELINE config 2 (the metric); the CMPCv5 models run BASELINE config 4 (512x512, L=25) as the line's workload")
    ap.add_argument("--prefetch-gate", default="fwd", choices=("fwd", "bwd"), help="with --prefetch: the next batch's backbone starts behind this step's levels' forward / backward")
    ap.add_argument("--prefetch", action="store_true", help="hand train_step the next batch, whose backbone pass then runs behind this step's levels instead "
                    "of at the start of its own step (measured SLOWER: 11.2 vs 10.5 ms, DESIGN 7; off by default)")
    ap.add_argument("--no-config4", action="store_true", help="skip the BASELINE config 4 rate reported inside the --full line")
    ap.add_argument("--no-config5", action="store_true", help="skip the BASELINE config 5 (video) rate reported inside the --full line")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last one computed as DIR/<name>.npy (float32 / float64, <= 64 MB; rank 0). "
                         "bench_out/<tag> is ignored by git")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    full = args.full

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        # CMPC_BENCH_REHEARSAL=1 (development only): rehearse the multi-process control flow on a ONE-GPU box -- every rank
        # on cuda:0, gradients exchanged with gloo.  The measured configuration is always one rank per GPU over RCCL.
        if os.environ.get("CMPC_BENCH_REHEARSAL"):
            torch.distributed.init_process_group("gloo")
            local = 0
        else:
            torch.distributed.init_process_group("nccl", device_id=torch.device(f"cuda:{local}"))
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X; there is no CPU path for the product")
    torch.cuda.set_device(local)
    dev = torch.device(f"cuda:{local}")

    pkg = importlib.import_module("cmpc-refseg_amd")
    v5 = args.model != "CMPC_model"
    B, T, H, W = (args.batch, 20, 320, 320) if not v5 else (args.batch, 25, 512, 512)
    log("building model")
    model = pkg.get_segmentation_model(args.model, batch_size=B, num_steps=T, vf_h=H // 8, vf_w=W // 8, H=H, W=W, mode="train", dtype=args.dtype, device=str(dev))
    model.enable_data_parallel()
    w, im, sl, tg = synth_batch(B, T, H, W, model.cfg.vocab_size, seed=rank)
    words = torch.from_numpy(w).to(dev)
    im = torch.from_numpy(im).to(dev)
    seq_len = torch.from_numpy(sl).to(dev)
    target = torch.from_numpy(tg).to(dev)
    torch.cuda.synchronize()
    ready = torch.cuda.Event()
    ready.record()                                   # the synthetic batch is resident in HBM from here on

    def barrier():
        if world > 1:
            torch.distributed.barrier()
        torch.cuda.synchronize()

    # Set-up, not warm-up: the first passes size the library's per-stream partial-sum workspaces, run MIOpen's search for
    # the stem convolution and capture the two backbone graphs; they are taken here so that the W warm-up steps and the K
    # timed steps below run in steady state whatever W is.
    SETUP_STEPS = 6
    # --prefetch: a prefetching loader (the reference's DataReader thread) has the next batch resident while the current one trains; train_step
    # is told about it and enqueues its frozen-backbone pass inside the current step (same work per step, every step runs its own pass)
    nxt = {"next_im": im, "next_ready": ready, "next_gate": args.prefetch_gate} if args.prefetch else {}
    for _ in range(SETUP_STEPS):
        model.train_step(words, im, target, seq_len, ready=ready, **nxt)
    torch.cuda.synchronize()
    log("model built; warmup")
    for i in range(args.warmup):
        model.train_step(words, im, target, seq_len, ready=ready, **nxt)
        torch.cuda.synchronize()
        log(f"warmup step {i} done")
    barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        gstep, scal = model.train_step(words, im, target, seq_len, ready=ready, **nxt)
    barrier()
    dt = time.perf_counter() - t0
    if args.dump_outputs and rank == 0:
        dump_outputs(model, gstep, scal, args.dump_outputs)
    loss = float(scal["loss_all"])
    launches = model.eng.launch_count()            # library launches of the last forward + backward + optimizer step
    # Per-launch timing of the dominant kernel family: in the timed region above the three pyramid levels run on three
    # lane streams, so a kernel's start->end event interval also contains other streams' kernels.  The event pairs
    # (cmpc_kernel_timing: hipEvents on the stream each launch is issued on, inside the library) are therefore taken over the
    # same K steps re-run on ONE stream (same kernels, same shapes, same data), which is also how the committed rocprof
    # summary is collected.
    ktime = None
    if full and not args.no_kernel_timing:
        model.set_lanes(1)
        model.train_step(words, im, target, seq_len)
        torch.cuda.synchronize()
        model.eng.kernel_timing(True)
        for _ in range(args.steps):
            model.train_step(words, im, target, seq_len)
        ktime = model.eng.kernel_timing_read()
        model.eng.kernel_timing(False)
        model.set_lanes(3 if int(os.environ.get("CMPC_STREAMS", "3")) > 1 else 1)
    # the second half of the roofline: every launch name timed on one stream, HBM-bound stages priced against their byte model
    trace = None
    if full and not args.no_kernel_timing and world == 1 and not v5 and args.dtype != "f32":
        trace = launch_trace(pkg, model, args.steps, (words, im, target, seq_len))
        model.set_lanes(3 if int(os.environ.get("CMPC_STREAMS", "3")) > 1 else 1)
    # forward-only rate (SURVEY 8d reports both): sess.run([pred, up, sigm]) on the same batch, same K
    dt_fwd = None
    if full and not args.no_forward_only:
        for _ in range(2):
            model.forward(words, im, seq_len)
        barrier()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            model.forward(words, im, seq_len)
        barrier()
        dt_fwd = time.perf_counter() - t0
    # the same train step with bf16 storage (BASELINE config 2 names bf16): same kernels, same rate, misses the IoU bar
    alt = None
    if full and world == 1 and args.dtype == "f16" and not args.no_alt_dtype and not v5:
        del model
        torch.cuda.empty_cache()
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            m2 = pkg.LSTM_model(batch_size=B, num_steps=T, H=H, W=W, mode="train", dtype="bf16", device=str(dev))
        for _ in range(SETUP_STEPS + args.warmup):
            m2.train_step(words, im, target, seq_len, ready=ready)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            m2.train_step(words, im, target, seq_len, ready=ready)
        torch.cuda.synchronize()
        d2 = time.perf_counter() - t0
        alt = {"dtype": "bf16", "images_per_sec": B * args.steps / d2, "ms_per_step": 1e3 * d2 / args.steps,
               "note": "bf16 storage: same MFMA pipelines; mean-IoU delta vs the oracle up to 1.6e-4 (bar 1e-4), f16 storage <= 3.5e-5"}
        del m2
    # BASELINE config 4 (CMPCv5_BiLSTM + HSV branch, 512x512, L=25) on the same GPU: train-step and forward-only rate, reported inside the line
    cfg4 = None
    if full and world == 1 and not v5 and not args.no_config4:
        model = None
        torch.cuda.empty_cache()
        cfg4 = config4_rate(pkg, dev, args)
    cfg5 = None
    if full and world == 1 and not v5 and not args.no_config5:
        model = None
        torch.cuda.empty_cache()
        cfg5 = config5_rate(pkg, dev, args)
    tmax = torch.tensor([dt], device=dev, dtype=torch.float64)
    if world > 1:
        torch.distributed.all_reduce(tmax, op=torch.distributed.ReduceOp.MAX)
    dt = float(tmax.item())
    log(f"timed {args.steps} steps in {dt:.3f} s")

    if rank == 0:
        out = {
            "metric": "images/sec at 320x320 L=20 (train step: backbone fwd + CMPC head fwd/bwd + grad all-reduce + Adam)" if not v5 else
                      "images/sec at 512x512 L=25 (BASELINE config 4 train step: backbone fwd + CMPCv5_BiLSTM head fwd/bwd + Adam)",
            "value": B * world * args.steps / dt, "unit": "images/sec", "n_gpus": world, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": 1e3 * dt / args.steps, "higher_is_better": True, "scaling": "weak",
            "vs_baseline": None, "dtype": args.dtype, "data": "synthetic",
            "config": {"workload": f"{args.model} {H}x{W} B={B}/gpu L={T} {args.dtype} storage (f16 in place of the bf16 BASELINE config 2 names: bf16 storage "
                                   f"misses the 1e-4 mean-IoU bar, f16 meets it at the same MFMA rate), ResNet-101 backbone (frozen), random-init weights",
                       "global_batch": B * world, "parallelism": f"dp{world}", "setup_steps_before_warmup": SETUP_STEPS},
            "final_loss": loss,
        }
        if dt_fwd is not None:
            out["forward_only"] = {"images_per_sec": B * world * args.steps / dt_fwd, "ms_per_step": 1e3 * dt_fwd / args.steps,
                                   "what": "model.forward: backbone + head forward -> pred, up, sigm (rank-0 clock)"}
        out["head_launches_per_step"] = launches
        if ktime is not None and ktime[3] > 0:
            t, f, by, n = ktime
            peak = 2500.0 if args.dtype != "f32" else 157.3          # dense 16-bit MFMA peak (f16 = bf16 rate), fp32 MFMA peak
            # HBM-side bytes per launch from the committed PMC passes (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE on this
            # same command, scripts/pmc_traffic.py); bench.py cannot run the profiler on itself
            traffic, traffic_src = None, None
            tp = os.path.join(os.path.dirname(os.path.abspath(__file__)), "profiles", "r03_gemm_nt_traffic.json")
            if args.dtype != "f32" and B == 8 and os.path.exists(tp):
                import hashlib
                raw = open(tp, "rb").read()
                traffic = json.loads(raw)["hbm_bytes_per_launch"]
                # not measured in this run: which committed profile the number comes from (content hash, so a stale file is visible)
                traffic_src = "profiles/r03_gemm_nt_traffic.json sha1 " + hashlib.sha1(raw).hexdigest()[:12] + " (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes of scripts/collect_profiles.sh)"
            out["roofline"] = {"bound": "mfma", "achieved": f / t / 1e12, "peak": peak, "unit": "TFLOP/s",
                               "frac": f / t / 1e12 / peak, "traffic": traffic, "traffic_source": traffic_src,
                               "algorithmic_bytes_per_launch": by / n,
                               "kernel": "gemm_nt_v5/v4/v3_kernel<%s> (every 1x1-conv / dX product of the head)" % args.dtype,
                               "measured": "hipEvent pairs around every launch (cmpc_kernel_timing, on the launch stream) over the same K steps re-run on ONE stream (in the timed region the lane streams overlap, so a start->end interval there also contains other streams' kernels)",
                               "launches_per_step": n / args.steps, "ms_per_step_in_kernel": 1e3 * t / args.steps}
        if trace is not None and ktime is not None and ktime[3] > 0:
            sm = stage_model(B)
            step_ms = 1e3 * dt / args.steps
            fam = {"hbm": [0.0, 0.0], "mfma": [0.0, 0.0], "latency": [0.0, 0.0]}
            per = {}
            nt_names = [k for k in trace if k.startswith("gemm_nt(v5)") or k.startswith("gemm_nt(v4") or k.startswith("gemm_nt(pair)")]
            nt_ms = sum(trace[k][0] for k in nt_names)
            bound_ms = 0.0
            for k, (ms_k, n_k) in sorted(trace.items(), key=lambda kv: -kv[1][0]):
                if k in nt_names:
                    continue
                kind, work = sm.get(k, ("latency", 0.0))
                fam[kind][0] += ms_k; fam[kind][1] += work
                if kind == "hbm":
                    per[k] = {"ms": round(ms_k, 4), "launches": n_k, "GB_per_s": round(work / ms_k / 1e6, 1), "frac": round(work / ms_k / 1e6 / 8000.0, 3)}
                    bound_ms += work / 8e12 * 1e3
                elif kind == "mfma":
                    per[k] = {"ms": round(ms_k, 4), "launches": n_k, "TFLOP_per_s": round(work / ms_k / 1e9, 1), "frac": round(work / ms_k / 1e9 / 2500.0, 3)}
                    bound_ms += work / 2.5e15 * 1e3
                else:
                    per[k] = {"ms": round(ms_k, 4), "launches": n_k}
            nt_flops = ktime[1] / args.steps
            bound_ms += nt_flops / 2.5e15 * 1e3
            per["gemm_nt(16-bit tiles)"] = {"ms": round(nt_ms, 4), "launches": sum(trace[k][1] for k in nt_names), "TFLOP_per_s": round(nt_flops / nt_ms / 1e9, 1),
                                            "frac": round(nt_flops / nt_ms / 1e9 / 2500.0, 3)}
            hb, hw = fam["hbm"]
            out["roofline_hbm"] = {"bound": "hbm", "achieved": hw / hb / 1e6, "peak": 8000.0, "unit": "GB/s", "frac": hw / hb / 1e6 / 8000.0,
                                   "ms_per_step_in_kernels": hb, "algorithmic_bytes_per_step": hw, "traffic": None,
                                   "what": "every HBM-bound stage kernel of the head (normalisations, softmaxes, gating, ConvLSTM gates, score / upsample / loss, Adam + pack): "
                                           "compulsory bytes (unique inputs once, outputs once; SURVEY 8d) / time from cmpc_launch_trace on one stream",
                                   "latency_bound_launches": {"ms_per_step": fam["latency"][0], "what": "language-side [B, .] launches and partial-row folds: no byte model"}}
            out["roofline_overall"] = {"frac": bound_ms / step_ms, "lower_bound_ms": bound_ms, "ms_per_step": step_ms,
                                       "one_stream_kernel_ms": sum(v[0] for v in trace.values()),
                                       "what": "sum over launch names of max(FLOPs / 2.5 PFLOP/s, bytes / 8 TB/s) divided by the measured step time (lanes overlapped)"}
            out["kernel_breakdown"] = per
        if alt is not None:
            out["alt_dtype"] = alt
        if cfg4 is not None:
            out["config4"] = cfg4
        if cfg5 is not None:
            out["config5"] = cfg5
        if full and world == 1 and not args.no_cpu_baseline:
            log("cpu baseline (oracle on host cores)")
            out["cpu_baseline"] = cpu_baseline(args)
        print(json.dumps(out), flush=True)
    if world > 1:
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
