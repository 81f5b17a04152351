"""Early-stopping decode against the full decode at the cfg3 shape (Neural BG2 z=384, T=20, B=65536, weights 0.5).

One process, one device.  For each Eb/N0 point (the bench's Philox channel) three steps are timed with HIP events,
alternating within the point so that they share the box's state (bench.py's timed() pattern: warm-up steps, a
synchronise, one event pair per step, a synchronise):
  early   nldpc.decode.decode_early_stop (out, iters, unsat)
  full    nldpc.decode.decode with all T posteriors written
  last    nldpc.decode.decode with out_mask keeping only the last posterior
  syn     nldpc.channel.syndrome_weight on one posterior (the pass that fills `unsat`, part of `early`)
Prints one JSON line per point (median and min / max of the step times in ms, the mean of iters, the fraction of
codewords that ended as codewords) and, with --out, writes the same lines to a file.

    python tools/bench_early_stop.py [--ebn0 -4,2,3,4,6] [--batch 65536] [--iters 20] [--steps 5] [--warmup 2]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "neural-ldpc-decoder-torch_amd", "src"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)


def timed(dev, steps, warmup, fns):
    """Per-step ms of each function in fns, the functions alternating step by step."""
    for _ in range(warmup):
        for f in fns:
            f()
    torch.cuda.synchronize(dev)
    ev = [[(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in fns]
          for _ in range(steps)]
    for row in ev:
        for (e0, e1), f in zip(row, fns):
            e0.record()
            f()
            e1.record()
    torch.cuda.synchronize(dev)
    return [[row[k][0].elapsed_time(row[k][1]) for row in ev] for k in range(len(fns))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ebn0", default="-4,2,3,4,6")
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--z", type=int, default=384)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    from nldpc.channel import awgn_llr, sigma_for, syndrome_weight
    from nldpc.decode import KIND_NEURAL, DecodeCfg, decode, decode_early_stop
    from nldpc.graph import LiftedGraph

    dev = torch.device("cuda:0")
    bg = np.loadtxt(os.path.join(ROOT, "resources", "basegraph2_set0.txt"), int, delimiter="\t")
    M, N = bg.shape
    Z, T, B = args.z, args.iters, args.batch
    g = LiftedGraph(bg, Z)
    w = torch.full((T, g.E), 0.5, device=dev)
    b = torch.zeros((T, g.E), device=dev)
    cfg = DecodeCfg(kind=KIND_NEURAL, keep_state=False, path="fused")
    last_only = [False] * (T - 1) + [True]
    lines = []
    for e in [float(v) for v in args.ebn0.split(",")]:
        xa = awgn_llr(B, N, Z, sigma_for(e, (N - M) / (N - 2)), seed=2042, device=dev)
        res = {}

        # (each step frees the others' results first: two sets of T posteriors do not fit beside each other)
        def early():
            res.clear()
            res["es"] = decode_early_stop(g, cfg, xa, T, w_cn=w, bias=b)

        def full():
            res.clear()
            res["full"] = decode(g, cfg, xa, T, w_cn=w, bias=b)

        def last():
            res.clear()
            res["last"] = decode(g, cfg, xa, T, w_cn=w, bias=b, out_mask=last_only)

        keep = decode_early_stop(g, cfg, xa, T, w_cn=w, bias=b)
        _, iters, unsat = keep

        def syn():
            res.clear()
            res["syn"] = syndrome_weight(keep[0], g)

        ms = timed(dev, args.steps, args.warmup, [early, full, last, syn])
        stat = lambda v: {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)}  # noqa: E731
        line = {"ebn0_db": e, "Z": Z, "T": T, "B": B, "early_stop_ms": stat(ms[0]), "full_all_outputs_ms": stat(ms[1]),
                "full_last_output_ms": stat(ms[2]), "syndrome_ms": stat(ms[3]), "mean_iters": round(float(iters.float().mean()), 3),
                "codeword_fraction": round(float((unsat == 0).float().mean()), 5), "device": torch.cuda.get_device_name(0)}
        print(json.dumps(line), flush=True)
        lines.append(json.dumps(line))
        res.clear()
        del keep
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
