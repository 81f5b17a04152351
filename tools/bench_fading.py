"""The fused flat-fading QAM channel (nldpc.fading.qam_llr) against the AWGN channel (nldpc.modulation.qam_llr).

Timing mode (default), at the cfg3 front-end shape of tools/bench_modulation.py (B = 65536 codewords, E = 7680 sent bits):
one process, one device, HIP events, the steps alternating (tools/bench_encode.py's timed()).  For qm = 2, 4, 6, 8 and one
demapper method: the fading kernel at L = 1, L = 64 and L >= S, each with drawn and with given gains, without and with
a scramble table, and modulation.qam_llr (no scramble table) in the same alternation as the yardstick.  The 5*E*B-byte
floor (E bytes read, 4*E written per codeword) is taken at the copy rate nldpc_hbm_probe (kind 0) measures in this
process; a given table adds 4*B*ceil(S/L) bytes read.  One JSON line per qm and a text table.

--ber: BG2 z=96 at rate 1/2 (E = 1920), 64-QAM max-log, encoded words, Neural decoder (weights 0.75, bias 0, erasures
1e-3), frame errors per iteration.  Channels: AWGN, Rayleigh L = 1, Rayleigh L = S/10; each with RateMatch(qm=6) and with
RateMatch(qm=1) in front of the same mapper; on the fading channels also a mismatched receiver, modulation.demap of the
received symbols, which ignores the gains.  A coarse sweep in 1 dB steps on a quarter of the batch (CSI receiver,
interleaver qm = 6) finds per channel the first Eb/N0 whose frame error rate after the last iteration is at most 10 %;
the three points reported are that one and 1 dB to either side of it.

    python tools/bench_fading.py [--batch 65536] [--E 7680] [--qm 2,4,6,8] [--method maxlog] [--steps 7] [--warmup 2] [--out FILE]
    python tools/bench_fading.py --ber [--batch 8192] [--iters 20] [--out FILE]      (--out appends)
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


def timing(args, dev, emit):
    from nldpc import fading, modulation
    from nldpc.scrambling import sequence
    B, E = args.batch, args.E
    rate = copy_rate(dev)
    floor_ms = 5 * E * B / rate * 1e3
    f = torch.from_numpy(np.random.default_rng(1).integers(0, 2, (B, E)).astype(np.uint8)).to(dev)
    llr = torch.empty((B, E), dtype=torch.float32, device=dev)
    seq = sequence(list(range(1, 9)), E, device=dev)
    emit(f"# {torch.cuda.get_device_name(0)}, B={B}, E={E}, steps={args.steps}, method {args.method}; copy rate "
         f"{rate / 1e12:.2f} TB/s, 5*E*B = {5 * E * B / 1e9:.2f} GB: floor {floor_ms:.3f} ms\n"
         "# median ms (min-max) of fading.qam_llr, and x = its median / the median of modulation.qam_llr (AWGN, no scramble "
         "table) of the same alternation")
    for qm in (int(q) for q in args.qm.split(",")):
        S = E // qm
        sigma = modulation.sigma_for(6.0, 0.5, qm)
        names, fns = ["awgn"], [lambda: modulation.qam_llr(f, qm, sigma, method=args.method, out=llr)]
        for L in (1, 64, S):
            table = fading.gains(B, S, L=L, device=dev)
            for gname, gain in (("drawn", None), ("given", table)):
                for sname, scr in (("plain", None), ("scr", seq)):
                    names.append(f"L={'S' if L == S else L} {gname} {sname}")
                    fns.append(lambda L=L, gain=gain, scr=scr: fading.qam_llr(f, qm, sigma, L=L, gain=gain, scramble=scr,
                                                                              method=args.method, out=llr))
        s = [stat(v) for v in timed(dev, args.steps, args.warmup, fns)]
        base = s[0]["median"]
        emit(f"qm={qm}  awgn {base:.3f} ({s[0]['min']:.3f}-{s[0]['max']:.3f}) ms, {base / floor_ms:.2f} x floor")
        for n, x in zip(names[1:], s[1:]):
            emit(f"  {n:<18} {x['median']:7.3f} ({x['min']:.3f}-{x['max']:.3f})  x {x['median'] / base:5.2f}")
        emit(json.dumps({"mode": "timing", "qm": qm, "method": args.method, "B": B, "E": E,
                         "copy_TBps": round(rate / 1e12, 3), "floor_ms": round(floor_ms, 4),
                         "ms": dict(zip(names, s))}))


def ber(args, dev, emit):
    from nldpc import fading, modulation
    from nldpc.channel import encode
    from nldpc.decode import KIND_NEURAL, DecodeCfg, decode_count
    from nldpc.graph import LiftedGraph
    from nldpc.ratematch import RateMatch, code_rate, rate_match, rate_recover
    bg = np.loadtxt(os.path.join(ROOT, "resources", "basegraph2_set0.txt"), int, delimiter="\t")
    g = LiftedGraph(bg, 96)
    B, T, QM, E = args.batch, args.iters, 6, 2 * g.K * g.Z
    S = E // QM
    w, b = torch.full((T, g.E), 0.75, device=dev), torch.zeros((T, g.E), device=dev)
    cfg = DecodeCfg(kind=KIND_NEURAL, keep_state=False)
    y = encode(g, B=B, seed=2042, device=dev)
    rms = {q: RateMatch.nr5g(g, E, rv=0, qm=q) for q in (QM, 1)}
    R = code_rate(g, rms[QM])
    channels = [("awgn", None), ("rayleigh L=1", 1), (f"rayleigh L={S // 10}", S // 10)]
    emit(f"# {torch.cuda.get_device_name(0)}, BG2 z=96, E={E} (rate {R:.3f}), 64-QAM max-log, Neural T={T} w=0.75, B={B} "
         "encoded words; frame errors per iteration")

    def frames(L, iq, ebn0, nb, mismatched=False):
        yy, rm = y[:nb], rms[iq]
        sigma = modulation.sigma_for(ebn0, R, QM)
        f = rate_match(g, rm, yy)
        if L is None:
            llr = modulation.qam_llr(f, QM, sigma, seed=7)
        elif not mismatched:
            llr = fading.qam_llr(f, QM, sigma, L=L, seed=7)
        else:
            llr = modulation.demap(fading.qam_llr(f, QM, sigma, L=L, seed=7, return_symbols=True)[1], QM, sigma)
        xa = rate_recover(g, rm, llr, erasure_value=1e-3)
        return decode_count(g, cfg, xa, T, w_cn=w, bias=b, y=yy).cpu().numpy()[:, 1].tolist()

    for name, L in channels:
        nb, found = max(B // 4, 1), None
        for e in range(0, 41):
            fe = frames(L, QM, float(e), nb)[-1]
            if fe <= 0.1 * nb:
                found = e
                break
        emit(f"# {name}: coarse sweep (B={nb}, 1 dB steps from 0 dB): first point with FER <= 10 % is {found} dB")
        if found is None:
            continue
        for e in (found - 1.0, float(found), found + 1.0):
            for iq in (QM, 1):
                line = {"mode": "ber", "channel": name, "ebn0_db": e, "interleaver_qm": iq, "B": B, "T": T,
                        "frame_errors": frames(L, iq, e, B)}
                if L is not None:
                    line["frame_errors_mismatched"] = frames(L, iq, e, B, mismatched=True)
                line["fer_last"] = round(line["frame_errors"][-1] / B, 5)
                emit(json.dumps(line))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=None)
    ap.add_argument("--E", type=int, default=7680)
    ap.add_argument("--qm", default="2,4,6,8")
    ap.add_argument("--method", default="maxlog")
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--ber", action="store_true")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.batch is None:
        args.batch = 8192 if args.ber else 65536
    dev = torch.device("cuda:0")
    lines = []

    def emit(text):
        print(text, flush=True)
        lines.append(text)

    (ber if args.ber else timing)(args, dev, emit)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a" if args.ber else "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
