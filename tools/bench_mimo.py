"""The fused MIMO channel (nldpc.mimo.qam_llr) against the fused flat-fading channel (nldpc.fading.qam_llr, given gains)
over the same number of LLRs.

At the cfg3 front-end shape of tools/bench_modulation.py (B = 65536 codewords, E = 7680 sent bits): one process, one
device, HIP events, the steps alternating (tools/bench_encode.py's timed()).  For each qm and one demapper method, for
the six (nt, nr) pairs: the fused kernel at L = 1 and L = 64, each with drawn and with given channels, and
fading.qam_llr with given gains at the same L in the same alternation as the yardstick.  Beside them, for the question
of DESIGN §4.4 (how the filter's L-fold redundancy is handled): mimo.filter alone on the L = 1 and the L = 64 table (what
a filter-table pre-pass would cost before the detecting kernel reads the table back) and mimo.detect on the samples of
the fused run.  One JSON line per (qm, nt, nr) and a text table.

    python tools/bench_mimo.py [--batch 65536] [--E 7680] [--qm 2,4,6,8] [--method maxlog] [--steps 7] [--warmup 2] [--out FILE]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "neural-ldpc-decoder-torch_amd", "src"), ROOT, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

from bench_encode import copy_rate, stat, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--E", type=int, default=7680)
    ap.add_argument("--qm", default="2,4,6,8")
    ap.add_argument("--method", default="maxlog")
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from nldpc import fading, mimo
    dev = torch.device("cuda:0")
    lines = []

    def emit(text):
        print(text, flush=True)
        lines.append(text)

    B, E = args.batch, args.E
    rate = copy_rate(dev)
    floor_ms = 5 * E * B / rate * 1e3
    f = torch.from_numpy(np.random.default_rng(1).integers(0, 2, (B, E)).astype(np.uint8)).to(dev)
    llr = torch.empty((B, E), dtype=torch.float32, device=dev)
    emit(f"# {torch.cuda.get_device_name(0)}, B={B}, E={E}, steps={args.steps}, method {args.method}; copy rate "
         f"{rate / 1e12:.2f} TB/s, 5*E*B = {5 * E * B / 1e9:.2f} GB: floor {floor_ms:.3f} ms\n"
         "# median ms (min-max); x = the median / the median of fading.qam_llr (given gains, same L) of the same alternation")
    for qm in (int(q) for q in args.qm.split(",")):
        S = E // qm
        for nt, nr in mimo.DIMS:
            if S % nt:
                emit(f"qm={qm} {nt}x{nr}: E / qm = {S} is no multiple of nt, skipped")
                continue
            R = S // nt
            sigma = mimo.sigma_for(6.0, 0.5, qm, nt)
            names, fns, base_of = [], [], {}
            for L in (1, 64):
                gains = fading.gains(B, S, L=L, device=dev)
                names.append(f"fading L={L} given")
                fns.append(lambda L=L, gains=gains: fading.qam_llr(f, qm, sigma, L=L, gain=gains, method=args.method, out=llr))
                base_of[L] = len(names) - 1
                table = mimo.channels(B, R, nt=nt, nr=nr, L=L, device=dev)
                for hname, h in (("drawn", None), ("given", table)):
                    names.append(f"L={L} {hname}")
                    fns.append(lambda L=L, h=h: mimo.qam_llr(f, qm, sigma, nt=nt, nr=nr, L=L, h=h, method=args.method, out=llr))
                names.append(f"L={L} filter alone")
                fns.append(lambda table=table: mimo.filter(table, sigma))
                y = mimo.qam_llr(f, qm, sigma, nt=nt, nr=nr, L=L, h=table, return_symbols=True)[1]
                names.append(f"L={L} detect")
                fns.append(lambda L=L, y=y, table=table: mimo.detect(y, qm, sigma, table, L=L, method=args.method, out=llr))
            s = [stat(v) for v in timed(dev, args.steps, args.warmup, fns)]
            emit(f"qm={qm} {nt}x{nr}  R={R}")
            for i, (n, x) in enumerate(zip(names, s)):
                L = 1 if "L=1 " in n else 64
                base = s[base_of[L]]["median"]
                ratio = "" if i == base_of[L] else f"  x {x['median'] / base:5.2f}"
                emit(f"  {n:<20} {x['median']:7.3f} ({x['min']:.3f}-{x['max']:.3f}){ratio}")
            emit(json.dumps({"mode": "timing", "qm": qm, "nt": nt, "nr": nr, "method": args.method, "B": B, "E": E,
                             "copy_TBps": round(rate / 1e12, 3), "floor_ms": round(floor_ms, 4), "ms": dict(zip(names, s))}))
            del fns
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
