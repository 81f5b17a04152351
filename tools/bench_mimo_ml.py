"""The max-log ML MIMO detector (nldpc.mimo.qam_llr_ml, nldpc.mimo.detect_ml) against the fused LMMSE channel
(nldpc.mimo.qam_llr, max-log) over the same bits, samples and channels.

At the cfg3 front-end shape of tools/bench_mimo.py (B = 65536 codewords, E = 7680 sent bits): one process, one device,
HIP events, the steps alternating (tools/bench_encode.py's timed()).  For every supported (qm, nt, nr), with a given
channel table at L = 1 (one matrix per resource element: the most table traffic; the detector itself does not depend
on L): mimo.qam_llr (max-log), mimo.qam_llr_ml and mimo.detect_ml on the samples of the fused run, in one alternation.
Reported per kernel: the median ms, the ratio to mimo.qam_llr and the candidate metrics per second (resource elements
times 2^qm for one layer, 2 * 2^(qm (nt - 1)) for several).  One JSON line per (qm, nt, nr) and a text table.

    python tools/bench_mimo_ml.py [--batch 65536] [--E 7680] [--qm 2,4,6,8] [--steps 7] [--warmup 2] [--out FILE]
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


def candidates(qm, nt):
    return 2 ** qm if nt == 1 else 2 * 2 ** (qm * (nt - 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--E", type=int, default=7680)
    ap.add_argument("--qm", default="2,4,6,8")
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from nldpc import mimo
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
    emit(f"# {torch.cuda.get_device_name(0)}, B={B}, E={E}, steps={args.steps}, given channels, L=1; copy rate "
         f"{rate / 1e12:.2f} TB/s, 5*E*B = {5 * E * B / 1e9:.2f} GB: floor {floor_ms:.3f} ms\n"
         "# median ms (min-max); x = the median / the median of mimo.qam_llr (max-log) of the same alternation; "
         "Gcand/s = candidate metrics per second")
    for qm in (int(q) for q in args.qm.split(",")):
        S = E // qm
        for nt, nr in mimo.DIMS:
            if S % nt:
                emit(f"qm={qm} {nt}x{nr}: E / qm = {S} is no multiple of nt, skipped")
                continue
            if nt == 4 and qm > 4:
                emit(f"qm={qm} {nt}x{nr}: unsupported (tree search), skipped")
                continue
            R = S // nt
            sigma = mimo.sigma_for(6.0, 0.5, qm, nt)
            table = mimo.channels(B, R, nt=nt, nr=nr, L=1, device=dev)
            y = mimo.qam_llr(f, qm, sigma, nt=nt, nr=nr, L=1, h=table, return_symbols=True)[1]
            names = ["lmmse qam_llr", "ml qam_llr_ml", "ml detect_ml"]
            fns = [lambda: mimo.qam_llr(f, qm, sigma, nt=nt, nr=nr, L=1, h=table, method="maxlog", out=llr),
                   lambda: mimo.qam_llr_ml(f, qm, sigma, nt=nt, nr=nr, L=1, h=table, out=llr),
                   lambda: mimo.detect_ml(y, qm, sigma, table, L=1, out=llr)]
            s = [stat(v) for v in timed(dev, args.steps, args.warmup, fns)]
            n_cand = B * R * candidates(qm, nt)
            emit(f"qm={qm} {nt}x{nr}  R={R}  candidates per RE {candidates(qm, nt)}")
            for i, (n, x) in enumerate(zip(names, s)):
                tail = "" if i == 0 else f"  x {x['median'] / s[0]['median']:7.2f}  {n_cand / x['median'] / 1e6:8.1f} Gcand/s"
                emit(f"  {n:<16} {x['median']:9.3f} ({x['min']:.3f}-{x['max']:.3f}){tail}")
            emit(json.dumps({"mode": "timing", "qm": qm, "nt": nt, "nr": nr, "B": B, "E": E, "candidates_per_re": candidates(qm, nt),
                             "copy_TBps": round(rate / 1e12, 3), "floor_ms": round(floor_ms, 4), "ms": dict(zip(names, s)),
                             "Gcand_per_s": {n: round(n_cand / x["median"] / 1e6, 2) for n, x in list(zip(names, s))[1:]}}))
            del fns, table, y
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
