"""Step time of CMPCv5_model and CMPCv5_HSV_model beside config 4 (CMPCv5_BiLSTM_HSV_model): B = 8, 512x512, L = 25, f16 storage, ResNet-101
backbone, batch-norm in training mode -- the train step (backbone + head forward / backward + Adam) and the forward pass, timed as bench.py's
config4_rate does.  Each graph runs in a child process of its own under a time limit; the first failing or timed-out child ends the run.
usage: python scripts/v5uni_bench.py [--steps 20] [--warmup 3] [--limit 300] [--models CMPCv5_model,CMPCv5_HSV_model,CMPCv5_BiLSTM_HSV_model]"""
import argparse
import importlib
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def measure(name, steps, warmup, B=8):
    import torch
    sys.path.insert(0, ROOT)
    from bench import synth_batch
    pkg = importlib.import_module("cmpc-refseg_amd")
    T, H, W = 25, 512, 512
    m = pkg.get_segmentation_model(name, batch_size=B, num_steps=T, vf_h=64, vf_w=64, H=H, W=W, mode="train", dtype="f16")
    dev = m.device
    w, im, sl, tg = (torch.from_numpy(x).to(dev) for x in synth_batch(B, T, H, W, m.cfg.vocab_size, seed=4))
    torch.cuda.synchronize()
    for _ in range(6 + warmup):
        m.train_step(w, im, tg, sl)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        _, scal = m.train_step(w, im, tg, sl)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    for _ in range(2):
        m.forward(w, im, sl)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        m.forward(w, im, sl)
    torch.cuda.synchronize()
    df = time.perf_counter() - t0
    return {"model": name, "B": B, "ms_per_step": 1e3 * dt / steps, "images_per_sec": B * steps / dt, "forward_only_ms": 1e3 * df / steps,
            "final_loss": float(scal["loss_all"]), "grad_nonfinite": m.grad_nonfinite(), "head_launches_per_step": m.eng.launch_count()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--limit", type=int, default=300, help="seconds allowed per graph")
    ap.add_argument("--models", default="CMPCv5_model,CMPCv5_HSV_model,CMPCv5_BiLSTM_HSV_model")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        print(json.dumps(measure(a.child, a.steps, a.warmup)), flush=True)
        return 0
    for name in a.models.split(","):
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", name, "--steps", str(a.steps), "--warmup", str(a.warmup)],
                               capture_output=True, text=True, timeout=a.limit)
        except subprocess.TimeoutExpired:
            print(json.dumps({"model": name, "error": f"timed out after {a.limit} s"}), flush=True)
            return 1
        if r.returncode != 0:
            print(json.dumps({"model": name, "error": f"exit status {r.returncode}", "stderr": r.stderr[-2000:]}), flush=True)
            return 1
        print(r.stdout.strip().splitlines()[-1], flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
