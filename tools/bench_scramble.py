"""Gold-sequence scrambling at the cfg3 front-end shape (B = 65536 codewords, E = 7680 sent bits, 64-QAM), and what the
all-zero word hides over 16-QAM and above.

One process, one device, HIP events, the steps alternating (tools/bench_encode.py's timed()).  Timed:
  sequence_1       scrambling.sequence(one c_init, E = 25344)          a single table row
  sequence_4096    scrambling.sequence(4096 c_inits, E = 7680)         one row per transport block
  scramble         scrambling.scramble                                 bits [B, E] -> bits ^ c
  descramble       scrambling.descramble                               LLRs [B, E] -> sign-flipped LLRs
  qam_llr          modulation.qam_llr(f)                               the plain fused channel
  qam_llr_scr      modulation.qam_llr(f, scramble=table)               the fused channel that scrambles in flight
  composition      scramble + qam_llr + descramble                     three launches, 15 bytes per bit against 5
for both demapper methods, with the ratios (a) qam_llr_scr / qam_llr, (b) qam_llr_scr / composition and, with
--naive-lib, (c) sequence / the naive generator: a second build of the library whose nldpc_gold_sequence gives one
thread a whole sequence, which it steps through from its first bit (no jump inside the row):
    cd neural-ldpc-decoder-torch_amd && mkdir -p lib_exp/gold_naive && \\
    hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -fno-fast-math -I../include -Icsrc \\
          -DNLDPC_GOLD_RUN=0 -x hip -c csrc/nldpc_scramble.hip -o lib_exp/gold_naive/nldpc_scramble.o && \\
    hipcc --offload-arch=gfx950 -shared -fPIC -o lib_exp/gold_naive/libgold_naive.so lib_exp/gold_naive/nldpc_scramble.o
(one translation unit; it is loaded after libnldpc.so, whose error helpers it binds to).  Its tables are compared with
the library's before they are timed.

--ber: BG2 z=96 at rate 1/2 (E = 1920, punct_cols = 0), 64-QAM max-log, the count-only Neural decode of
tools/bench_encode.py --ber (weights 0.5, bias 0, T iterations, noise seed 7): per-iteration frame errors of
  (a) the all-zero word unscrambled   (b) the all-zero word scrambled   (c) encoded random words unscrambled
on the same noise.  (b) should track (c); (a) sends one constellation point only.  (b) uses --n-seq sequences (one per
codeword modulo that number); (b1) is the same with one sequence for every codeword, i.e. one pattern of constellation
points for the whole batch.

One JSON line per measurement and a text table; --out writes both to a file.

    python tools/bench_scramble.py [--batch 65536] [--E 7680] [--qm 6] [--steps 7] [--warmup 2] [--naive-lib SO] [--out FILE]
    python tools/bench_scramble.py --ber [--ebn0 9,10,11] [--iters 20] [--batch 65536] [--n-seq 4096] [--out FILE]
"""
import argparse
import ctypes
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


def _fmt(x):
    return f"{x['median']:.4f} ({x['min']:.4f}-{x['max']:.4f})"


def timings(args, dev, emit):
    from nldpc import _lib
    from nldpc.modulation import qam_llr, sigma_for
    from nldpc.scrambling import descramble, scramble, sequence

    B, E, qm = args.batch, args.E, args.qm
    rate = copy_rate(dev)
    floor_ms = 5 * E * B / rate * 1e3
    rng = np.random.default_rng(1)
    f = torch.from_numpy(rng.integers(0, 2, (B, E)).astype(np.uint8)).to(dev)
    fs = torch.empty_like(f)
    llr = torch.empty((B, E), dtype=torch.float32, device=dev)
    llr2 = torch.empty_like(llr)
    ci1 = torch.tensor([0x12345], dtype=torch.int32, device=dev)
    ciN = torch.from_numpy(rng.integers(0, 2 ** 31, 4096).astype(np.int32)).to(dev)
    seq1 = torch.empty((1, (25344 + 31) // 32), dtype=torch.int32, device=dev)
    seqN = torch.empty((4096, (E + 31) // 32), dtype=torch.int32, device=dev)
    sigma = sigma_for(6.0, 0.5, qm)
    emit(f"# {torch.cuda.get_device_name(0)}, B={B}, E={E}, qm={qm}, steps={args.steps}; copy rate {rate / 1e12:.2f} TB/s, "
         f"5*E*B = {5 * E * B / 1e9:.2f} GB: floor {floor_ms:.3f} ms\n# median ms (min-max)")

    fns = [lambda: sequence(ci1, 25344, out=seq1), lambda: sequence(ciN, E, out=seqN)]
    names = ["sequence_1", "sequence_4096"]
    if args.naive_lib:
        naive = ctypes.CDLL(os.path.abspath(args.naive_lib))
        naive.nldpc_gold_sequence.restype = ctypes.c_int32
        naive.nldpc_gold_sequence.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p]
        n1, nN = torch.empty_like(seq1), torch.empty_like(seqN)

        def run_naive(ci, n, length, out):
            if naive.nldpc_gold_sequence(ci.data_ptr(), n, length, out.data_ptr(), _lib.stream_of(dev)) != 0:
                raise RuntimeError("the naive build's nldpc_gold_sequence failed")

        fns += [lambda: run_naive(ci1, 1, 25344, n1), lambda: run_naive(ciN, 4096, E, nN)]
        names += ["naive_1", "naive_4096"]
    t = dict(zip(names, (stat(v) for v in timed(dev, args.steps, args.warmup, fns))))
    if args.naive_lib:
        assert torch.equal(n1, seq1) and torch.equal(nN, seqN), "the naive build's tables differ"
    for k, v in t.items():
        emit(f"{k:>14} {_fmt(v)}")
    line = {"what": "sequence", "E_1": 25344, "E_4096": E, **{k + "_ms": v for k, v in t.items()}}
    if args.naive_lib:
        line["c_sequence_over_naive_1"] = round(t["sequence_1"]["median"] / t["naive_1"]["median"], 4)
        line["c_sequence_over_naive_4096"] = round(t["sequence_4096"]["median"] / t["naive_4096"]["median"], 4)
        emit(f"(c) sequence / naive: n_seq=1 {line['c_sequence_over_naive_1']:.4f}, n_seq=4096 "
             f"{line['c_sequence_over_naive_4096']:.4f}")
    emit(json.dumps(line))

    for n_seq, seq in ((1, seqN[:1].contiguous()), (4096, seqN)):
        for method in ("maxlog", "logmap"):
            t = timed(dev, args.steps, args.warmup, [
                lambda: scramble(f, seq, out=fs),
                lambda: descramble(llr2, seq, out=llr2),
                lambda: qam_llr(f, qm, sigma, method=method, out=llr),
                lambda: qam_llr(f, qm, sigma, method=method, out=llr, scramble=seq),
                lambda: descramble(qam_llr(scramble(f, seq, out=fs), qm, sigma, method=method, out=llr2), seq, out=llr2),
            ])
            s = dict(zip(("scramble", "descramble", "qam_llr", "qam_llr_scr", "composition"), (stat(v) for v in t)))
            assert torch.equal(llr.view(torch.int32), llr2.view(torch.int32)), "fused and composed LLRs differ"
            a = s["qam_llr_scr"]["median"] / s["qam_llr"]["median"]
            b = s["qam_llr_scr"]["median"] / s["composition"]["median"]
            emit(f"n_seq={n_seq} {method}: " + ", ".join(f"{k} {_fmt(v)}" for k, v in s.items())
                 + f"; (a) scr / plain {a:.3f}, (b) scr / composition {b:.3f}, scr / floor "
                 f"{s['qam_llr_scr']['median'] / floor_ms:.2f}, scramble at {2 * E * B / s['scramble']['median'] / 1e9:.2f} TB/s, "
                 f"descramble at {8 * E * B / s['descramble']['median'] / 1e9:.2f} TB/s")
            emit(json.dumps({"what": "channel", "qm": qm, "method": method, "n_seq": n_seq, "B": B, "E": E,
                             "copy_TBps": round(rate / 1e12, 3), "floor_ms": round(floor_ms, 4),
                             **{k + "_ms": v for k, v in s.items()}, "a_scr_over_plain": round(a, 4),
                             "b_scr_over_composition": round(b, 4)}))


def ber(args, dev, emit):
    from nldpc.channel import encode
    from nldpc.decode import KIND_NEURAL, DecodeCfg, decode_count
    from nldpc.graph import LiftedGraph
    from nldpc.modulation import qam_llr, sigma_for
    from nldpc.ratematch import RateMatch, code_rate, rate_match, rate_recover
    from nldpc.scrambling import sequence

    bg = np.loadtxt(os.path.join(ROOT, "resources", "basegraph2_set0.txt"), int, delimiter="\t")
    Z, B, T, qm = 96, args.batch, args.iters, 6
    g = LiftedGraph(bg, Z)
    E = 2 * g.K * Z
    rm = RateMatch(E=E, k0=0, punct_cols=0, n_filler=0, ncb=0, qm=qm)
    R = code_rate(g, rm)
    w = torch.full((T, g.E), 0.5, device=dev)
    b = torch.zeros((T, g.E), device=dev)
    cfg = DecodeCfg(kind=KIND_NEURAL, keep_state=False)
    y = encode(g, B=B, seed=2042, device=dev)
    fy = rate_match(g, rm, y)
    seq1 = sequence(0x12345, E, device=dev)
    seq = sequence(np.random.default_rng(3).integers(0, 2 ** 31, args.n_seq).tolist(), E, device=dev)
    emit(f"# {torch.cuda.get_device_name(0)}: BG2 z={Z}, E={E} (rate {R:.3f}, punct_cols 0), 64-QAM max-log, Neural w=0.5 b=0 "
         f"T={T}, B={B}, noise seed 7, (b) {args.n_seq} sequences, (b1) one; frame errors per iteration")
    for e in [float(v) for v in args.ebn0.split(",")]:
        sigma = sigma_for(e, R, qm)
        res = {}
        for label, f, cw, table in (("a_zero_plain", None, None, None), ("b_zero_scrambled", None, None, seq),
                                    ("b1_zero_one_sequence", None, None, seq1), ("c_encoded_plain", fy, y, None)):
            llr = qam_llr(f, qm, sigma, B=B, E=E, seed=7, scramble=table, device=dev)
            xa = rate_recover(g, rm, llr, erasure_value=1e-3)
            c = decode_count(g, cfg, xa, T, w_cn=w, bias=b, y=cw).cpu().numpy()
            res[label] = c[:, 1].tolist()
            res[label + "_bit_errors_last"] = int(c[-1, 0])
            emit(f"{e:5.2f} dB {label:>20}: {c[:, 1].tolist()}")
            del llr, xa
        emit(json.dumps({"what": "ber", "ebn0_db": e, "sigma": round(sigma, 6), "Z": Z, "E": E, "B": B, "T": T, **res}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--E", type=int, default=7680)
    ap.add_argument("--qm", type=int, default=6)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--naive-lib", default=None, help="a build with -DNLDPC_GOLD_RUN=0 (see the module docstring)")
    ap.add_argument("--ber", action="store_true")
    ap.add_argument("--ebn0", default="9,10,11")
    ap.add_argument("--n-seq", type=int, default=4096, help="--ber: sequences of the scrambled all-zero word")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    rows = []

    def emit(text):
        print(text, flush=True)
        rows.append(text)

    (ber if args.ber else timings)(args, dev, emit)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as fh:
            fh.write("\n".join(rows) + "\n")


if __name__ == "__main__":
    main()
