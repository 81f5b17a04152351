"""CRC attachment and checking at the cfg3 shape (BG2 z=384, B = 65536, A = 3816 payload bits, CRC24A, W = K*Z = 3840)
beside the read-only HBM probe over the same bytes and beside the syndrome launch on the same batch.

One process, one device, HIP events, the steps alternating (tools/bench_encode.py's timed()).  Timed:
  attach_given      nldpc.crc.attach(payload [B, A] uint8)      reads A, writes W bytes per block
  attach_drawn      nldpc.crc.attach(None, B=B, A=A)            payload drawn on the device; writes W bytes per block
  check_llr         nldpc.crc.check(posterior [B, N*Z] fp32)    reads the first n = A + L floats of every N*Z-float row
  check_llr_ref     the same with ref = the codewords [B, N*Z] uint8 and the three counts
  check_llr_packed  the same values as a contiguous [B, n] tensor: the strided reads as one range
  check_bits        nldpc.crc.check(codewords [B, N*Z] uint8)   reads the first n bytes of every N*Z-byte row
  syndrome          nldpc.channel.syndrome_weight(posterior)    the other genie-free verdict; reads every row in full
and as yardsticks nldpc_hbm_probe over the posterior's memory, in the same alternation:
  probe_read_4n     kind 2 (read only) over the 4 n B bytes check_llr needs, as one contiguous range
  probe_rows_4NZ    kind 2 over the 4 N*Z B bytes of the whole rows those reads are spread over: the lower bracket
  probe_read_n      kind 2 over the n B bytes check_bits needs;  probe_rows_NZ  over its whole rows
  probe_read_A+W    kind 2 over the (A + W) B bytes attach_given moves
  probe_write_W     kind 1 (write only) over the W B bytes both attach launches write
  probe_read4B_4n   kind 3 (read only, 4 bytes per lane) over check_llr's bytes
The posterior is the BPSK channel output of the encoded blocks at noise sigma 0.25 (no decode: the check's time does not
depend on the values; about a tenth of the blocks hold a wrong bit); the counts are printed.

A text table and one JSON line; --out writes both to a file.

    python tools/bench_crc.py [--batch 65536] [--z 384] [--crc 24A] [--steps 9] [--warmup 2] [--sigma 0.25] [--out FILE]
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
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--z", type=int, default=384)
    ap.add_argument("--crc", default="24A")
    ap.add_argument("--steps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sigma", type=float, default=0.25, help="noise of the channel output that stands in for a posterior")
    ap.add_argument("--tag", default=None, help="label of the build under test (a variant of DESIGN §4.4, F9)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    from nldpc import _lib
    from nldpc.channel import awgn_llr, encode, syndrome_weight
    from nldpc.crc import CRCS, attach, check, payload_len
    from nldpc.graph import LiftedGraph

    dev = torch.device("cuda:0")
    bg = np.loadtxt(os.path.join(ROOT, "resources", "basegraph2_set0.txt"), int, delimiter="\t")
    Z, B, crc = args.z, args.batch, args.crc
    g = LiftedGraph(bg, Z)
    L = CRCS[crc][1]
    W, NZ = g.K * Z, g.N * Z
    A = payload_len(g, crc)
    n = A + L

    info = attach(None, crc, graph=g, B=B, A=A, seed=2042, device=dev)
    payload = info[:, :A].contiguous()
    info2 = torch.empty_like(info)
    y = encode(g, info)
    post = awgn_llr(B, g.N, Z, args.sigma, seed=7, device=dev, y=y).view(B, NZ)
    ok = torch.empty((B,), dtype=torch.uint8, device=dev)
    cnt = torch.zeros((3,), dtype=torch.int64, device=dev)
    sink = torch.empty((8192 * 4,), dtype=torch.float32, device=dev)
    wbuf = torch.empty((B * W // 4,), dtype=torch.float32, device=dev)
    lib, flat = _lib.lib(), post.view(-1)

    def probe(kind, nbytes, buf=None):
        nf = nbytes // 16 * 4
        dst, src = (buf, flat) if kind == 1 else (sink, flat)
        return lambda: _lib.check(lib.nldpc_hbm_probe(kind, dst.data_ptr(), src.data_ptr(), nf, _lib.stream_of(dev)),
                                  "nldpc_hbm_probe")

    packed = post[:, :n].contiguous()  # the same values with stride A + L: the check's reads as one contiguous range
    # (name, launch, the bytes it needs)
    runs = [
        ("attach_given", lambda: attach(payload, crc, W=W, out=info2), (A + W) * B),
        ("attach_drawn", lambda: attach(None, crc, W=W, B=B, A=A, seed=2042, out=info2), W * B),
        ("check_llr", lambda: check(post, crc, A, ok=ok), 4 * n * B),
        ("check_llr_ref", lambda: check(post, crc, A, ref=y, ok=ok, counts=cnt), 5 * n * B),
        ("check_llr_packed", lambda: check(packed, crc, A, ok=ok), 4 * n * B),
        ("check_bits", lambda: check(y, crc, A, ok=ok), n * B),
        ("syndrome", lambda: syndrome_weight(post, g), 4 * NZ * B),
        ("probe_read_4n", probe(2, 4 * n * B), 4 * n * B),
        ("probe_rows_4NZ", probe(2, 4 * NZ * B), 4 * NZ * B),
        ("probe_read_n", probe(2, n * B), n * B),
        ("probe_rows_NZ", probe(2, NZ * B), NZ * B),
        ("probe_read_A+W", probe(2, (A + W) * B), (A + W) * B),
        ("probe_write_W", probe(1, W * B, wbuf), W * B),
        ("probe_read4B_4n", probe(3, 4 * n * B), 4 * n * B),
    ]
    names, fns, nbytes = (list(col) for col in zip(*runs))
    ms = timed(dev, args.steps, args.warmup, fns)
    assert torch.equal(info, info2)
    cnt.zero_()
    _, c = check(post, crc, A, ref=y, ok=ok, counts=cnt)
    c = c.cpu().tolist()
    assert not check(y, crc, A).eq(0).any()

    s = {k: stat(v) for k, v in zip(names, ms)}
    head = (f"# {torch.cuda.get_device_name(0)}, BG2 z={Z}, B={B}, CRC{crc}, A={A}, W={W}, N*Z={NZ}, steps={args.steps}"
            + (f", build {args.tag}" if args.tag else "")
            + f"\n# posterior: channel output at sigma {args.sigma}: CRC failures {c[0]}, undetected {c[1]}, block errors {c[2]} of {B}"
            "\n# median ms (min-max); bytes the launch needs; TB/s = bytes / median")
    rows = [head]
    for k, nb in zip(names, nbytes):
        rows.append(f"{k:>16} {s[k]['median']:8.4f} ({s[k]['min']:.4f}-{s[k]['max']:.4f}) {nb / 1e9:8.3f} GB "
                    f"{nb / s[k]['median'] / 1e9:7.3f} TB/s")
    m = {k: s[k]["median"] for k in names}
    rows.append(f"# check_llr / probe_read_4n = {m['check_llr'] / m['probe_read_4n']:.2f}, / probe_rows_4NZ = "
                f"{m['check_llr'] / m['probe_rows_4NZ']:.2f}, / syndrome = {m['check_llr'] / m['syndrome']:.3f}; "
                f"check_bits / probe_read_n = {m['check_bits'] / m['probe_read_n']:.2f}; attach_given / probe_read_A+W = "
                f"{m['attach_given'] / m['probe_read_A+W']:.2f}, / probe_write_W = {m['attach_given'] / m['probe_write_W']:.2f}")
    line = json.dumps({"Z": Z, "B": B, "crc": crc, "A": A, "W": W, "NZ": NZ, "tag": args.tag, "sigma": args.sigma, "counts": c,
                       "ms": s, "bytes": dict(zip(names, nbytes))})
    text = "\n".join(rows + [line])
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
