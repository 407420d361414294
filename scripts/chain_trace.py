"""Lane overlap inside the train step's serial windows, from a multi-stream rocprofv3 kernel trace (3 lanes):
    cd /tmp && rocprofv3 --kernel-trace --output-format csv -d <out> -- python3 scripts/prof_step.py 14 3
    python scripts/chain_trace.py <out>/.../*_kernel_trace.csv [skip_first_steps=4]
Per window and averaged over the steady-state steps: wall time, busy time per stream (kernel durations clipped to the window) and the time
during which 0 / 1 / 2 / >=3 streams have a kernel running.  The windows are cut at kernels every schedule has:
  fwd round 1    first rowdot1<f16> of the step           -> end of the 3rd exch_combine_fwd
  fwd round 2    end of the 3rd exch_combine_fwd          -> end of the 6th
  clstm bwd      start of the 1st clstm_bwd1              -> end of the 3rd clstm_bwd3
  bwd round 2    start of the 1st exch_combine_bwd        -> the last of the round-1 fan-in add_n<f16> has started
  bwd round 1    that point                               -> the last of the levels' fan-in add_n<f16> has started
The profiler adds a few microseconds to every launch, so the walls are longer than scripts/phase_timeline.py's; the shares are the point."""
import collections, csv, re, sys

rows = list(csv.DictReader(open(sys.argv[1])))
skip = int(sys.argv[2]) if len(sys.argv) > 2 else 4
ev = sorted((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"], r["Stream_Id"]) for r in rows)


def is_(n, key, f16=False):
    return key in n and (not f16 or "DF16_" in n)


starts = [i for i, e in enumerate(ev) if "embed_gather_kernel" in e[2]]           # first launch of a step's forward pass
steps = [ev[a:b] for a, b in zip(starts[skip:-1], starts[skip + 1:])]
acc = collections.OrderedDict()
for st in steps:
    def sel(key, f16=False):
        return [e for e in st if is_(e[2], key, f16)]
    cf, cb, an = sel("exch_combine_fwd"), sel("exch_combine_bwd"), sel("add_n_kernel", True)
    b1, b3, rd = sel("clstm_bwd1"), sel("clstm_bwd3"), sel("rowdot1_kernel", True)
    if len(cf) != 6 or len(cb) != 6 or len(an) != 6 or len(b1) != 3:
        continue
    cf.sort(key=lambda e: e[1])
    t3 = cf[2][1]
    fan1, fanL = max(e[0] for e in an[:3]), max(e[0] for e in an[3:])
    wins = [("fwd round 1", rd[0][0], t3), ("fwd round 2", t3, cf[5][1]), ("clstm bwd", b1[0][0], max(e[1] for e in b3)),
            ("bwd round 2", cb[0][0], fan1), ("bwd round 1", fan1, fanL)]
    for name, lo, hi in wins:
        a = acc.setdefault(name, {"wall": [], "busy": collections.defaultdict(list), "conc": collections.defaultdict(list), "n": collections.defaultdict(list)})
        a["wall"].append(hi - lo)
        edges, busy, cnt = [], collections.Counter(), collections.Counter()
        for s, e, n, q in st:
            s2, e2 = max(s, lo), min(e, hi)
            if e2 > s2:
                busy[q] += e2 - s2; cnt[q] += 1
                edges += [(s2, 1, q), (e2, -1, q)]
        edges.sort()
        live, conc, t = collections.Counter(), collections.Counter(), lo
        for x, d, q in edges:
            conc[min(3, sum(1 for v in live.values() if v > 0))] += x - t
            t = x; live[q] += d
        conc[0] += hi - t
        for q in busy: a["busy"][q].append(busy[q]); a["n"][q].append(cnt[q])
        for k in range(4): a["conc"][k].append(conc[k])
m = lambda v, n: sum(v) / max(1, n) / 1e3
print(f"{sys.argv[1].split('/')[-1]}: {len(steps)} steps; times in us, means over the steps")
for name, a in acc.items():
    n = len(a["wall"])
    print(f"{name:12s} wall {m(a['wall'], n):7.1f} (min {min(a['wall'])/1e3:.1f} max {max(a['wall'])/1e3:.1f})   streams running 0/1/2/>=3: "
          + " / ".join(f"{m(a['conc'][k], n):6.1f}" for k in range(4)))
    for q in sorted(a["busy"]):
        print(f"{'':12s}   stream {q}: busy {m(a['busy'][q], n):7.1f}  kernels {sum(a['n'][q]) / n:5.1f}")
