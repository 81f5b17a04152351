"""The QAM channel at the cfg3 front-end shape (B = 65536 codewords, E = 7680 sent bits: BG2 z=384 at rate 1/2) against
the BPSK channel launch over the same number of LLRs.

One process, one device, HIP events, the steps alternating (tools/bench_encode.py's timed()).  Timed, for qm = 2, 4, 6, 8
and both demapper methods:
  qam_llr         nldpc.modulation.qam_llr          bits [B, E] uint8 -> LLRs [B, E], symbols never in memory
  modulate        nldpc.modulation.modulate         bits -> symbols [B, E/qm, 2]      } the unfused pair (its symbols
  demap           nldpc.modulation.demap            symbols -> LLRs                   } carry no noise: a floor for it)
  awgn_llr        nldpc.channel.awgn_llr(B, E, 1)   the BPSK channel, one normal per LLR (qam_llr draws 2/qm)
and beside them the 5*E*B-byte floor (E bytes read, 4*E written per codeword) at the copy rate nldpc_hbm_probe (kind 0)
measures in this process; the unfused pair moves (5 + 16/qm)*E*B bytes (the symbols written and read back).

One JSON line per (qm, method) and a text table; --out writes the table and the lines to a file.

    python tools/bench_modulation.py [--batch 65536] [--E 7680] [--qm 2,4,6,8] [--steps 7] [--warmup 2] [--tag T] [--out FILE]
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
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--tag", default=None, help="label of the build under test (a variant of DESIGN §4.4)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    from nldpc.channel import awgn_llr
    from nldpc.modulation import demap, modulate, qam_llr, sigma_for

    dev = torch.device("cuda:0")
    B, E = args.batch, args.E
    rate = copy_rate(dev)
    floor_ms = 5 * E * B / rate * 1e3
    f = torch.from_numpy(np.random.default_rng(1).integers(0, 2, (B, E)).astype(np.uint8)).to(dev)
    llr = torch.empty((B, E), dtype=torch.float32, device=dev)
    head = (f"# {torch.cuda.get_device_name(0)}, B={B}, E={E}, steps={args.steps}"
            + (f", build {args.tag}" if args.tag else "") + f"; copy rate {rate / 1e12:.2f} TB/s, "
            f"5*E*B = {5 * E * B / 1e9:.2f} GB: floor {floor_ms:.3f} ms\n"
            "# median ms (min-max); x = time / floor\n"
            f"{'qm':>2} {'method':>6} {'qam_llr':>22} {'x':>5} {'modulate':>20} {'demap':>20} {'pair':>7} {'pair x':>6} "
            f"{'awgn_llr':>22} {'x':>5}")
    rows, lines = [head], []
    for qm in (int(q) for q in args.qm.split(",")):
        sigma = sigma_for(6.0, 0.5, qm)
        sym = torch.empty((B, E // qm, 2), dtype=torch.float32, device=dev)
        pair_floor = (5 + 16 / qm) * E * B / rate * 1e3
        for method in ("maxlog", "logmap"):
            t = timed(dev, args.steps, args.warmup, [
                lambda: qam_llr(f, qm, sigma, method=method, out=llr),
                lambda: modulate(f, qm, out=sym),
                lambda: demap(sym, qm, sigma, method=method, out=llr),
                lambda: awgn_llr(B, E, 1, sigma, y=f, out=llr.view(B, E, 1)),
            ])
            s = [stat(v) for v in t]
            pair = s[1]["median"] + s[2]["median"]
            fmt = lambda x: f"{x['median']:.3f} ({x['min']:.3f}-{x['max']:.3f})"  # noqa: E731
            rows.append(f"{qm:>2} {method:>6} {fmt(s[0]):>22} {s[0]['median'] / floor_ms:5.2f} {fmt(s[1]):>20} "
                        f"{fmt(s[2]):>20} {pair:7.3f} {pair / pair_floor:6.2f} {fmt(s[3]):>22} "
                        f"{s[3]['median'] / floor_ms:5.2f}")
            lines.append(json.dumps({"qm": qm, "method": method, "B": B, "E": E, "tag": args.tag,
                                     "copy_TBps": round(rate / 1e12, 3), "floor_ms": round(floor_ms, 4),
                                     "pair_floor_ms": round(pair_floor, 4), "qam_llr_ms": s[0], "modulate_ms": s[1],
                                     "demap_ms": s[2], "awgn_llr_ms": s[3]}))
        del sym
    text = "\n".join(rows + lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
