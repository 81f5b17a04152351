"""Transport-block segmentation, concatenation and checking at the cfg3 shape: BG2 z=384, W = kcb = 3840, A = 61032,
CRC24A (C = 16 code blocks of K' = 3840 bits, no fillers), Btb = 4096 transport blocks = 65536 code blocks,
G = 16 * 7680 sent bits per TB, 64-QAM (qm = 6: E_r = 7680 for every block).

One process, one device, HIP events, the steps alternating (tools/bench_encode.py's timed()).  Timed:
  tb_check        nldpc.transport.check(posterior [C*Btb, N*Z] fp32) -> cb_ok, tb_ok   reads K' floats of every row
  tb_check_cb_only  cb_ok alone: the first kernel without the combining launch (their difference is the second pass)
  tb_check_ref    the same with ref_tb and the four counts
  tb_check_out    the same with tb_out (desegmentation: writes B' bytes per TB)
  crc_check_24B   nldpc.crc.check(posterior, "24B", A = K' - 24) -> ok: the plain code-block check on the same tensor,
                  the yardstick of tb_check (same bytes, one remainder instead of two)
  segment         nldpc_tb_segment alone (tb [Btb, B'] given)                          reads B' per TB, writes W per block
  concat_u8       nldpc.transport.concat of the rate-matched bits [C*Btb, E] uint8     reads and writes G bytes per TB
  deconcat_f32    nldpc.transport.deconcat of the LLRs [Btb, G] fp32                   reads and writes 4 G bytes per TB
and as yardsticks nldpc_hbm_probe in the same alternation:
  probe_read_4Kp  kind 2 (read only) over the 4 K' C Btb bytes both checks need, as one contiguous range
  probe_copy_seg / probe_copy_cat / probe_copy_decat   kind 0 (copy) moving the bytes segment / concat / deconcat move
The posterior is the BPSK channel output of the encoded blocks at noise sigma (no decode: the check's time does not depend
on the values); the counts are printed.

A text table and one JSON line; --out writes both to a file.

    python tools/bench_transport.py [--btb 4096] [--steps 9] [--warmup 2] [--sigma 0.25] [--tag NAME] [--out FILE]
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

from bench_encode import stat, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--btb", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sigma", type=float, default=0.25, help="noise of the channel output that stands in for a posterior")
    ap.add_argument("--tag", default=None, help="label of the build under test")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import ctypes

    from nldpc import _lib
    from nldpc.channel import awgn_llr, encode
    from nldpc.crc import check as crc_check
    from nldpc.graph import LiftedGraph
    from nldpc.transport import TBPlan, check, concat, deconcat, segment, split_E

    dev = torch.device("cuda:0")
    bg = np.loadtxt(os.path.join(ROOT, "resources", "basegraph2_set0.txt"), int, delimiter="\t")
    Z, Btb, qm = 384, args.btb, 6
    g = LiftedGraph(bg, Z)
    W, NZ = g.K * Z, g.N * Z
    plan = TBPlan.make(61032, W=W, tb_crc="24A", kcb=W)
    C, Kp, Bp = plan.C, plan.Kp, plan.Bp
    rows, G = C * Btb, C * 7680
    E_lo, E_hi, C_lo = split_E(plan, G, qm)
    assert (C, Kp, plan.F, E_lo, E_hi, C_lo) == (16, 3840, 0, 7680, 7680, 16)

    info, tb = segment(plan, Btb=Btb, seed=2042, device=dev)
    info2 = torch.empty_like(info)
    y = encode(g, info)
    post = awgn_llr(rows, g.N, Z, args.sigma, seed=7, device=dev, y=y).view(rows, NZ)
    del y
    f = torch.randint(0, 2, (rows, E_lo), dtype=torch.uint8, device=dev)
    gbits = torch.empty((Btb, G), dtype=torch.uint8, device=dev)
    gllr = torch.randn((Btb, G), dtype=torch.float32, device=dev)
    fllr = torch.empty((rows, E_lo), dtype=torch.float32, device=dev)
    cb_ok = torch.empty((rows,), dtype=torch.uint8, device=dev)
    tb_ok = torch.empty((Btb,), dtype=torch.uint8, device=dev)
    tb_out = torch.empty((Btb, Bp), dtype=torch.uint8, device=dev)
    cnt = torch.zeros((4,), dtype=torch.int64, device=dev)
    sink = torch.empty((8192 * 4,), dtype=torch.float32, device=dev)
    wbuf = torch.empty((Btb * G,), dtype=torch.float32, device=dev)
    lib, flat, c_plan = _lib.lib(), post.view(-1), plan._c()

    def probe(kind, nbytes):
        """kind 2 reads nbytes; kind 0 copies nbytes / 2 (reads and writes nbytes in all)"""
        nf = (nbytes if kind == 2 else nbytes // 2) // 16 * 4
        dst = sink if kind == 2 else wbuf
        return lambda: _lib.check(lib.nldpc_hbm_probe(kind, dst.data_ptr(), flat.data_ptr(), nf, _lib.stream_of(dev)),
                                  "nldpc_hbm_probe")

    def seg():
        _lib.check(lib.nldpc_tb_segment(ctypes.byref(c_plan), tb.data_ptr(), Btb, info2.data_ptr(), _lib.stream_of(dev)),
                   "nldpc_tb_segment")

    b_check, b_seg, b_cat, b_decat = 4 * Kp * rows, Btb * Bp + rows * W, 2 * Btb * G, 8 * Btb * G
    # (name, launch, the bytes it needs)
    runs = [
        ("tb_check", lambda: check(plan, post, cb_ok=cb_ok, tb_ok=tb_ok), b_check),
        ("tb_check_cb_only", lambda: check(plan, post, cb_ok=cb_ok, tb_ok=False), b_check),
        ("tb_check_ref", lambda: check(plan, post, ref_tb=tb, cb_ok=cb_ok, tb_ok=tb_ok, counts=cnt), b_check + Btb * Bp),
        ("tb_check_out", lambda: check(plan, post, cb_ok=cb_ok, tb_ok=tb_ok, tb_out=tb_out), b_check + Btb * Bp),
        ("crc_check_24B", lambda: crc_check(post, "24B", Kp - 24, ok=cb_ok), b_check),
        ("segment", seg, b_seg),
        ("concat_u8", lambda: concat(f, None, Btb, out=gbits), b_cat),
        ("deconcat_f32", lambda: deconcat(gllr, C, C_lo, E_lo, E_hi, out=(fllr, None)), b_decat),
        ("probe_read_4Kp", probe(2, b_check), b_check),
        ("probe_copy_seg", probe(0, b_seg), b_seg),
        ("probe_copy_cat", probe(0, b_cat), b_cat),
        ("probe_copy_decat", probe(0, b_decat), b_decat),
    ]
    names, fns, nbytes = (list(col) for col in zip(*runs))
    ms = timed(dev, args.steps, args.warmup, fns)
    assert torch.equal(info, info2)
    assert torch.equal(deconcat(concat(f, None, Btb), C, C_lo, E_lo, E_hi)[0], f)
    cnt.zero_()
    res = check(plan, post, ref_tb=tb, counts=cnt, tb_out=tb_out)
    c = res.counts.cpu().tolist()
    plain = crc_check(post, "24B", Kp - 24)
    assert torch.equal(res.cb_ok, plain) and c[3] == int((plain == 0).sum())
    clean = check(plan, info, ref_tb=tb, counts=True, tb_out=True)
    assert clean.counts.tolist() == [0, 0, 0, 0] and torch.equal(clean.tb_out, tb)

    s = {k: stat(v) for k, v in zip(names, ms)}
    head = (f"# {torch.cuda.get_device_name(0)}, BG2 z={Z}, A={plan.A}, CRC{plan.tb_crc}, C={C}, K'={Kp}, Btb={Btb} "
            f"({rows} code blocks), G={G}, N*Z={NZ}, steps={args.steps}" + (f", build {args.tag}" if args.tag else "")
            + f"\n# posterior: channel output at sigma {args.sigma}: TB CRC failures {c[0]}, undetected {c[1]}, TB errors {c[2]} "
            f"of {Btb}; code-block CRC failures {c[3]} of {rows}"
            "\n# median ms (min-max); bytes the launch needs; TB/s = bytes / median")
    out = [head]
    for k, nb in zip(names, nbytes):
        out.append(f"{k:>16} {s[k]['median']:8.4f} ({s[k]['min']:.4f}-{s[k]['max']:.4f}) {nb / 1e9:8.3f} GB "
                   f"{nb / s[k]['median'] / 1e9:7.3f} TB/s")
    m = {k: s[k]["median"] for k in names}
    out.append(f"# tb_check / crc_check_24B = {m['tb_check'] / m['crc_check_24B']:.2f}, / probe_read_4Kp = "
               f"{m['tb_check'] / m['probe_read_4Kp']:.2f}; tb_check_cb_only / tb_check = {m['tb_check_cb_only'] / m['tb_check']:.2f}, "
               f"tb_check_ref / tb_check = {m['tb_check_ref'] / m['tb_check']:.2f}, "
               f"tb_check_out / tb_check = {m['tb_check_out'] / m['tb_check']:.2f}; segment / probe_copy_seg = "
               f"{m['segment'] / m['probe_copy_seg']:.2f}; concat_u8 / probe_copy_cat = "
               f"{m['concat_u8'] / m['probe_copy_cat']:.2f}; deconcat_f32 / probe_copy_decat = "
               f"{m['deconcat_f32'] / m['probe_copy_decat']:.2f}")
    line = json.dumps({"Z": Z, "Btb": Btb, "C": C, "A": plan.A, "Kp": Kp, "G": G, "tag": args.tag, "sigma": args.sigma,
                       "counts": c, "ms": s, "bytes": dict(zip(names, nbytes))})
    text = "\n".join(out + [line])
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
