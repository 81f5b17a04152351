"""Build the tanh correction table of the SP check node (lib/nldpc_tanh_ref.bin).

The reference's sum-product check node calls torch.tanh on a CPU fp32 tensor
(src/boosted_neural_ldpc_decoder/BoostedNeuralLDPCDecoder.py:402).  ATen evaluates it with the BLAS
vendor's vector math (this image's torch: MKL VML vsTanh, high-accuracy mode), whose results are
within one ulp of the correctly rounded tanh but not equal to it: 803 349 of the 1.09e9 fp32 inputs
with |x| <= 10 differ, by exactly one ulp (measured here; odd symmetric).  Through atanh's
1 / (1 - P^2) near saturation one ulp of a factor moves an SP message by up to ~1e-3 relative, so
the device reproduces torch.tanh exactly: it rounds a double-precision tanh (correct rounding except
near a halfway point) and applies this table of the inputs where torch.tanh differs.

The check-node inputs are -0.5 * clamp(m, -20, 20), so |x| <= 10 covers every value the decoder
evaluates.  Inputs whose double tanh lies within 8 double ulps of a fp32 halfway point are listed
separately with their exact torch.tanh value, so the table does not depend on which double tanh
the device uses.

File layout (little-endian uint32): magic 0x4841544E ("NTAH"), version 2, SH, KMAX, n_entries,
n_override; provenance[16] (64 bytes of NUL-padded ASCII: the torch version, ATen's CPU capability and
the CPU model of the build host -- the table is what THAT torch.tanh computes; tests compare it with
the torch of the machine they run on); idx[(KMAX >> SH) + 2] (bucket b = key >> SH holds entries idx[b]..idx[b+1]);
entries[n_entries] = key | dir << 31, ascending in key (key = |x| bits; dir 1: torch.tanh is one ulp
above the correctly rounded value, 0: one ulp below); overrides[n_override] = (key, result bits).

The table the fixtures under tests/golden/ were made with is committed in packed form
(tests/golden/nldpc_tanh_ref.xz, a quarter of a megabyte) and the build unpacks it, byte for byte, into
lib/nldpc_tanh_ref.bin: torch.tanh differs between hosts (see above), so a table measured on the build
host would not reproduce the fixtures everywhere.  Packed layout: xz of the 88 header bytes, the
overrides, the four byte planes (low byte first) of the entries' key differences, and the dir bits
(numpy.packbits); idx is recomputed from the keys.

Usage: python3 gen_tanh_table.py OUT.bin               measure this host's torch.tanh
       python3 gen_tanh_table.py --pack IN.bin OUT.xz
       python3 gen_tanh_table.py --unpack IN.xz OUT.bin
"""
import lzma
import os
import struct
import sys

import numpy as np
import torch

SH = 15
KMAX = int(np.float32(10.0).view(np.uint32))  # 0x41200000


def provenance():
    """torch version | ATen CPU capability | CPU model of this host (what the table was measured on)."""
    cpu = "?"
    try:
        with open("/proc/cpuinfo") as f:
            cpu = next((ln.split(":", 1)[1].strip() for ln in f if ln.startswith("model name")), "?")
    except OSError:
        pass
    return f"{torch.__version__}|{torch.backends.cpu.get_cpu_capability()}|{cpu}"


def main(out):
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    entries, overrides = [], []
    chunk = 1 << 24
    for base in range(0, KMAX + 1, chunk):
        u = np.arange(base, min(base + chunk, KMAX + 1), dtype=np.uint32)
        x = torch.from_numpy(u.view(np.float32))
        ref = torch.tanh(x).numpy().view(np.uint32)  # what the reference's torch computes
        d = torch.tanh(x.double())
        cr = d.float()
        # halfway point between cr and its neighbour on d's side
        crd = cr.double()
        nb = torch.nextafter(cr, torch.where(d > crd, torch.full_like(cr, 2.0), torch.full_like(cr, -2.0))).double()
        mid = 0.5 * (crd + nb)
        amb = ((d - mid).abs() <= 8 * d.abs() * 2.0 ** -52).numpy()
        crb = cr.numpy().view(np.uint32)
        diff = ref.astype(np.int64) - crb.astype(np.int64)
        if np.abs(diff[~amb]).max(initial=0) > 1:
            raise SystemExit("gen_tanh_table: torch.tanh is more than one ulp from the rounded double tanh")
        sel = (diff != 0) & ~amb
        entries.append(u[sel] | ((diff[sel] > 0).astype(np.uint32) << np.uint32(31)))
        for k in np.nonzero(amb)[0]:
            overrides.append((int(u[k]), int(ref[k])))
    ent = np.concatenate(entries).astype(np.uint32)
    keys = ent & np.uint32(0x7FFFFFFF)
    assert np.all(np.diff(keys.astype(np.int64)) > 0)
    nb = (KMAX >> SH) + 2
    idx = np.searchsorted(keys, (np.arange(nb, dtype=np.uint64) << np.uint64(SH)).astype(np.uint32)).astype(np.uint32)
    idx[-1] = len(ent)
    hdr = struct.pack("<6I", 0x4841544E, 2, SH, KMAX, len(ent), len(overrides)) + provenance().encode()[:63].ljust(64, b"\0")
    tmp = out + ".tmp"
    with open(tmp, "wb") as f:
        f.write(hdr)
        f.write(idx.tobytes())
        f.write(ent.tobytes())
        for k, v in overrides:
            f.write(struct.pack("<2I", k, v))
    os.replace(tmp, out)
    print(f"gen_tanh_table: {len(ent)} corrections, {len(overrides)} overrides -> {out}")


def _index(keys, sh, kmax):
    nb = (kmax >> sh) + 2
    idx = np.searchsorted(keys, (np.arange(nb, dtype=np.uint64) << np.uint64(sh)).astype(np.uint32)).astype(np.uint32)
    idx[-1] = len(keys)
    return idx


def pack(src, out):
    raw = np.fromfile(src, dtype=np.uint32)
    magic, ver, sh, kmax, n, nov = (int(v) for v in raw[:6])
    if magic != 0x4841544E or ver != 2:
        raise SystemExit(f"gen_tanh_table: {src} is not a version 2 table")
    nb = (kmax >> sh) + 2
    ent, ov = raw[22 + nb:22 + nb + n], raw[22 + nb + n:]
    keys = ent & np.uint32(0x7FFFFFFF)
    if len(ov) != 2 * nov or not np.array_equal(raw[22:22 + nb], _index(keys, sh, kmax)):
        raise SystemExit(f"gen_tanh_table: {src} is inconsistent")
    delta = np.diff(keys, prepend=np.uint32(0))
    planes = b"".join(((delta >> np.uint32(8 * i)) & np.uint32(0xFF)).astype(np.uint8).tobytes() for i in range(4))
    blob = raw[:22].tobytes() + ov.tobytes() + planes + np.packbits((ent >> np.uint32(31)).astype(np.uint8)).tobytes()
    with open(out, "wb") as f:
        f.write(lzma.compress(blob, preset=9 | lzma.PRESET_EXTREME))
    unpack(out, out + ".check")
    same = open(out + ".check", "rb").read() == raw.tobytes()
    os.remove(out + ".check")
    if not same:
        raise SystemExit("gen_tanh_table: the packed table does not unpack to its source")
    print(f"gen_tanh_table: {src} ({raw.nbytes} bytes) -> {out} ({os.path.getsize(out)} bytes)")


def unpack(src, out):
    with open(src, "rb") as f:
        blob = lzma.decompress(f.read())
    hdr = np.frombuffer(blob[:88], dtype=np.uint32)
    magic, ver, sh, kmax, n, nov = (int(v) for v in hdr[:6])
    if magic != 0x4841544E or ver != 2 or len(blob) != 88 + 8 * nov + 4 * n + (n + 7) // 8:
        raise SystemExit(f"gen_tanh_table: {src} is not a packed version 2 table")
    o = 88 + 8 * nov
    delta = np.zeros(n, dtype=np.uint32)
    for i in range(4):
        delta |= np.frombuffer(blob[o + i * n:o + (i + 1) * n], dtype=np.uint8).astype(np.uint32) << np.uint32(8 * i)
    keys = np.cumsum(delta, dtype=np.uint64).astype(np.uint32)
    dirs = np.unpackbits(np.frombuffer(blob[o + 4 * n:], dtype=np.uint8))[:n].astype(np.uint32)
    tmp = out + ".tmp"
    with open(tmp, "wb") as f:
        f.write(blob[:88])
        f.write(_index(keys, sh, kmax).tobytes())
        f.write((keys | dirs << np.uint32(31)).tobytes())
        f.write(blob[88:o])
    os.replace(tmp, out)


if __name__ == "__main__":
    if sys.argv[1] == "--pack":
        pack(sys.argv[2], sys.argv[3])
    elif sys.argv[1] == "--unpack":
        unpack(sys.argv[2], sys.argv[3])
    else:
        main(sys.argv[1])
