"""Rate matching and rate recovery at the cfg3 shape (BG2 z=384, B=65536, rv0, no fillers, E = 7680: rate 1/2), and
what the rate-matched front end costs against the full-length channel launch it replaces.

One process, one device, HIP events, the steps alternating (tools/bench_encode.py's timed()).  Timed, for qm = 1 and
for qm = 6:
  rate_match      nldpc.ratematch.rate_match        codewords [B, N*Z] uint8 -> sent bits [B, E] uint8
  awgn_llr_E      nldpc.channel.awgn_llr over the E sent bits
  rate_recover    nldpc.ratematch.rate_recover      LLRs [B, E] -> decoder input [B, N, Z]
  awgn_llr_full   the parent path, awgn_llr over all N*Z bits of the codeword (measured here, in the same process)
and beside them the byte floors at the copy rate nldpc_hbm_probe (kind 0) measures in this process: 2*E*B bytes for
rate_match (one byte read and one written per sent bit), 4*(E + N*Z)*B bytes for rate_recover.  The write-only fill
rate (kind 1) is printed too: most of rate_recover's bytes are writes.

One JSON line per qm; --out writes the same lines to a file.

    python tools/bench_ratematch.py [--batch 65536] [--z 384] [--E 7680] [--qm 1,6] [--steps 7] [--warmup 2] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "neural-ldpc-decoder-torch_amd", "src"), ROOT, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

from bench_encode import copy_rate, stat, timed  # noqa: E402


def fill_rate(dev, gib=1.0):
    """Bytes per second of nldpc_hbm_probe's write-only fill (kind 1), the best of 6 launches."""
    from nldpc import _lib
    n = int(gib * (1 << 30) // 4) // 4 * 4
    b = torch.empty(n, dtype=torch.float32, device=dev)
    best = None
    for _ in range(6):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        _lib.check(_lib.lib().nldpc_hbm_probe(1, b.data_ptr(), b.data_ptr(), n, _lib.stream_of(dev)), "nldpc_hbm_probe")
        e1.record()
        e1.synchronize()
        ms = e0.elapsed_time(e1)
        best = ms if best is None else min(best, ms)
    return 4 * n / (best / 1000.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--z", type=int, default=384)
    ap.add_argument("--E", type=int, default=7680)
    ap.add_argument("--qm", default="1,6")
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--tag", default=None, help="label of the build under test (a variant of DESIGN §4.4)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    from nldpc.channel import awgn_llr, encode, sigma_for
    from nldpc.graph import LiftedGraph
    from nldpc.ratematch import RateMatch, code_rate, index, rate_match, rate_recover

    dev = torch.device("cuda:0")
    bg = np.loadtxt(os.path.join(ROOT, "resources", "basegraph2_set0.txt"), int, delimiter="\t")
    N = bg.shape[1]
    Z, B, E = args.z, args.batch, args.E
    g = LiftedGraph(bg, Z)
    name = torch.cuda.get_device_name(0)
    lines = []

    y = encode(g, B=B, seed=2042, device=dev)
    f = torch.empty((B, E), dtype=torch.uint8, device=dev)
    llr = torch.empty((B, E, 1), dtype=torch.float32, device=dev)
    xa = torch.empty((B, N, Z), dtype=torch.float32, device=dev)
    xa_full = torch.empty((B, N, Z), dtype=torch.float32, device=dev)
    rate, fill = copy_rate(dev), fill_rate(dev)
    for qm in [int(v) for v in args.qm.split(",")]:
        rm = RateMatch.nr5g(g, E, rv=0, qm=qm)
        sigma = sigma_for(3.0, code_rate(g, rm))
        llr2 = llr.view(B, E)
        fns = [lambda: rate_match(g, rm, y, out=f),
               lambda: awgn_llr(B, E, 1, sigma, seed=7, out=llr, y=f),
               lambda: rate_recover(g, rm, llr2, out=xa, erasure_value=1e-3),
               lambda: awgn_llr(B, N, Z, sigma, seed=7, out=xa_full, y=y)]
        ms = timed(dev, args.steps, args.warmup, fns)
        # the timed outputs are the real thing: the first 256 codewords against the host index
        idx = torch.from_numpy(index(g, rm).astype(np.int64)).to(dev)
        assert torch.equal(f[:256], y[:256][:, idx])
        if E <= N * Z - 2 * Z:  # (no bit is sent twice: recovery is a plain scatter)
            want = torch.full((256, N * Z), 1e-3, dtype=torch.float32, device=dev)
            want[:, idx] = llr2[:256]
            assert torch.equal(xa[:256].reshape(256, -1), want)
        med = [statistics.median(v) for v in ms]
        floor_match = 2 * E * B / rate * 1e3
        floor_recover = 4 * (E + N * Z) * B / rate * 1e3
        line = {"Z": Z, "B": B, "N": N, "E": E, "qm": qm, "code_rate": round(code_rate(g, rm), 4),
                "rate_match_ms": stat(ms[0]), "awgn_llr_E_ms": stat(ms[1]), "rate_recover_ms": stat(ms[2]),
                "awgn_llr_full_ms": stat(ms[3]), "hbm_copy_TBps": round(rate / 1e12, 3), "hbm_fill_TBps": round(fill / 1e12, 3),
                "rate_match_bytes": 2 * E * B, "rate_match_floor_ms": round(floor_match, 4),
                "rate_match_over_floor": round(med[0] / floor_match, 2),
                "rate_recover_bytes": 4 * (E + N * Z) * B, "rate_recover_floor_ms": round(floor_recover, 4),
                "rate_recover_over_floor": round(med[2] / floor_recover, 2),
                "front_end_ms": round(med[0] + med[1] + med[2], 4),
                "front_end_over_full_channel": round((med[0] + med[1] + med[2]) / med[3], 3),
                "device": name}
        if args.tag:
            line["build"] = args.tag
        print(json.dumps(line), flush=True)
        lines.append(json.dumps(line))
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
