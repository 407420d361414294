"""Phase boundaries of the multi-stream train step on the GPU clock (cmpc_phase_marks: hipEvents at the stage boundaries, no
profiler, so the overlap between the lanes is the real one).  usage: python scripts/phase_timeline.py [dtype] [steps]"""
import collections, importlib, os, sys
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench import synth_batch
pkg = importlib.import_module("cmpc-refseg_amd")
dev = torch.device("cuda:0")
dtype = sys.argv[1] if len(sys.argv) > 1 else "f16"
N = int(sys.argv[2]) if len(sys.argv) > 2 else 10
m = pkg.LSTM_model(batch_size=8, mode="train", dtype=dtype)
w, im, sl, tg = [torch.from_numpy(x).to(dev) for x in synth_batch(8, 20, 320, 320, m.cfg.vocab_size, 0)]
torch.cuda.synchronize(); ready = torch.cuda.Event(); ready.record()
for _ in range(8): m.train_step(w, im, tg, sl, ready=ready)
torch.cuda.synchronize()
m.eng.phase_marks(True)
for _ in range(N): m.train_step(w, im, tg, sl, ready=ready)
torch.cuda.synchronize()
marks = m.eng.phase_marks_read()
steps, cur = [], None
for name, t in marks:
    if name == "fwd:start":
        cur = []; steps.append(cur)
    cur.append((name, t))
acc = collections.OrderedDict()
for i in range(1, len(steps) - 1):
    t0 = steps[i][0][1]
    for name, t in steps[i]:
        acc.setdefault(name, []).append(t - t0)
    acc.setdefault("next fwd:start", []).append(steps[i + 1][0][1] - t0)
print("phase boundary, ms after fwd:start on the GPU clock (min / mean / max over %d steps)" % (len(steps) - 2))
for name, v in sorted(acc.items(), key=lambda kv: sum(kv[1]) / len(kv[1])):
    print(f"  {name:22s} {min(v):8.3f} {sum(v)/len(v):8.3f} {max(v):8.3f}")
# the intervals between boundaries, per step (a boundary's spread above includes the drift of everything before it)
IV = [("fwd:level_c3_done", "fwd:exch1_done"), ("fwd:exch1_done", "fwd:clstm_done"), ("bwd:start", "bwd:clstm_done"),
      ("bwd:clstm_done", "bwd:exch2_done"), ("bwd:exch2_done", "bwd:exch1_done"), ("bwd:clstm_done", "bwd:exch1_done"),
      ("bwd:text_done", "bwd:end"), ("bwd:text_done", "opt:end"), ("fwd:start", "next fwd:start")]
print("interval, ms (min / mean / max)")
for a, b in IV:
    if a in acc and b in acc and len(acc[a]) == len(acc[b]):
        d = [y - x for x, y in zip(acc[a], acc[b])]
        print(f"  {a + ' -> ' + b:44s} {min(d):8.3f} {sum(d)/len(d):8.3f} {max(d):8.3f}")
