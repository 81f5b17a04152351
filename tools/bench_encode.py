"""The on-device encoder at the cfg3 shape (BG2 z=384, B=65536), and what the all-zero codeword hides.

One process, one device, HIP events, the steps alternating (tools/bench_early_stop.py's timed()).

Default: three launches are timed,
  encode_philox   nldpc.channel.encode(graph, B=B)            info bits drawn on the device
  encode_given    nldpc.channel.encode(graph, info)           info bits read from a [B, K*Z] uint8 tensor
  awgn_llr_y      nldpc.channel.awgn_llr(..., y=codewords)    the channel launch the encoder feeds
and the byte floor (K + N) * Z * B bytes at the copy rate nldpc_hbm_probe measures in the same process is printed
beside them (the encoder reads K*Z and writes N*Z bytes per codeword; the channel kernel writes 4 * N*Z).

--ber: per-iteration bit and frame error counts of the count-only decode (Neural, weights 0.5, bias 0, T iterations)
for the all-zero codeword and for encoded random codewords on the same noise (same seed: the noise stream does not
depend on y), with and without puncturing the first 2Z bits, at each Eb/N0 (sigma from the design rate K / N').

One JSON line per measurement; --out writes the same lines to a file.

    python tools/bench_encode.py [--batch 65536] [--z 384] [--steps 7] [--warmup 2] [--out FILE]
    python tools/bench_encode.py --ber [--ebn0 1,2,3,4,6] [--iters 20] [--out FILE]
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


def copy_rate(dev, gib=1.0):
    """Bytes per second of nldpc_hbm_probe's stream copy (kind 0), the best of 6 launches."""
    from nldpc import _lib
    n = int(gib * (1 << 30) // 4) // 4 * 4
    a = torch.ones(n, dtype=torch.float32, device=dev)
    b = torch.empty(n, dtype=torch.float32, device=dev)
    best = None
    for _ in range(6):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        _lib.check(_lib.lib().nldpc_hbm_probe(0, b.data_ptr(), a.data_ptr(), n, _lib.stream_of(dev)), "nldpc_hbm_probe")
        e1.record()
        e1.synchronize()
        ms = e0.elapsed_time(e1)
        best = ms if best is None else min(best, ms)
    return 8 * n / (best / 1000.0)


def stat(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--z", type=int, default=384)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--ber", action="store_true")
    ap.add_argument("--ebn0", default="1,2,3,4,6")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    from nldpc.channel import awgn_llr, encode, sigma_for, syndrome_weight
    from nldpc.decode import KIND_NEURAL, DecodeCfg, decode_count
    from nldpc.graph import LiftedGraph

    dev = torch.device("cuda:0")
    bg = np.loadtxt(os.path.join(ROOT, "resources", "basegraph2_set0.txt"), int, delimiter="\t")
    M, N = bg.shape
    Z, B = args.z, args.batch
    g = LiftedGraph(bg, Z)
    K = g.K
    name = torch.cuda.get_device_name(0)
    lines = []

    def emit(line):
        line["device"] = name
        print(json.dumps(line), flush=True)
        lines.append(json.dumps(line))

    if not args.ber:
        y = encode(g, B=B, seed=2042, device=dev)
        info = y[:, :K * Z].contiguous()
        y2 = torch.empty_like(y)
        xa = torch.empty((B, N, Z), dtype=torch.float32, device=dev)
        sigma = sigma_for(3.0, K / N)
        fns = [lambda: encode(g, B=B, seed=2042, out=y), lambda: encode(g, info, out=y2),
               lambda: awgn_llr(B, N, Z, sigma, seed=7, out=xa, y=y)]
        ms = timed(dev, args.steps, args.warmup, fns)
        assert torch.equal(y, y2)
        unsat_max = int(syndrome_weight(2.0 * y[:4096].float() - 1.0, g).max())
        rate = copy_rate(dev)
        floor_ms = (K + N) * Z * B / rate * 1e3
        med = [statistics.median(v) for v in ms]
        emit({"Z": Z, "B": B, "K": K, "N": N, "encode_philox_ms": stat(ms[0]), "encode_given_ms": stat(ms[1]),
              "awgn_llr_y_ms": stat(ms[2]), "hbm_copy_TBps": round(rate / 1e12, 3),
              "encode_bytes": (K + N) * Z * B, "channel_write_bytes": 4 * N * Z * B, "byte_floor_ms": round(floor_ms, 4),
              "encode_philox_over_floor": round(med[0] / floor_ms, 2), "encode_given_over_floor": round(med[1] / floor_ms, 2),
              "encode_philox_over_awgn": round(med[0] / med[2], 3), "encode_given_over_awgn": round(med[1] / med[2], 3),
              "max_syndrome_weight_first_4096": unsat_max})
    else:
        T = args.iters
        w = torch.full((T, g.E), 0.5, device=dev)
        b = torch.zeros((T, g.E), device=dev)
        cfg = DecodeCfg(kind=KIND_NEURAL, keep_state=False)
        y = encode(g, B=B, seed=2042, device=dev)
        for punct in (None, (1, 2 * Z)):
            n_sent = N - (2 if punct else 0)
            for e in [float(v) for v in args.ebn0.split(",")]:
                sigma = sigma_for(e, K / n_sent)
                res = {}
                for label, cw in (("all_zero", None), ("encoded", y)):
                    xa = awgn_llr(B, N, Z, sigma, seed=7, device=dev, y=cw, puncturing=punct)
                    c = decode_count(g, cfg, xa, T, w_cn=w, bias=b, y=cw).cpu().numpy()
                    res[label + "_bit_errors"] = c[:, 0].tolist()
                    res[label + "_frame_errors"] = c[:, 1].tolist()
                    del xa
                emit({"ebn0_db": e, "code_rate": round(K / n_sent, 4), "punctured_bits": 2 * Z if punct else 0, "Z": Z,
                      "B": B, "T": T, "kind": "Neural w=0.5 b=0", **res})
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
