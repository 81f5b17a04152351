"""Golden fixtures for the special-value batch (tests/edge_inputs.py), made by running the REFERENCE in the
development container (like gen_golden.py; the GPU box never sees it).  BG2 z=16, B=6, T=4: an erased
codeword, punctured columns, an integer grid, values at +-20, values far beyond +-20, -0.0; CN weights
with exact zeros and negatives, Neural biases that kill messages.

  neural_bg2_z16_edges            NeuralLDPCDecoder outputs, BCE loss, weight / bias gradients
  boosted_bg2_z16_<kind>_nw102_edges   MS, SP, QMS q=5, 6, -5, 4, 3: per-edge CN, per-column VN weights
  boosted_bg2_z16_<kind>_nw112_edges   MS and QMS q=5 with UCN weights
  train_bg2_z16_<kind>_<nw>_edges      MS (1,0,2), SP (3,0,3), QMS q=6 and q=3 (1,0,2): outputs, LDPCDecoderLoss
                                       BCE value and parameter gradients
The QMS channel is quantised as the reference's datagen does (Functions.Cal_MSA_Q on the f64 values).
What is written is data only: inputs, parameters, outputs, losses, gradients.

Run (from the repo root):  PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_edges.py
"""
import argparse
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import edge_inputs as ei  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    args = ap.parse_args()
    sys.path.insert(0, os.path.join(args.ref, "src"))
    res = os.path.join(args.ref, "resources")
    import boosted_neural_ldpc_decoder as bref
    import neural_ldpc_decoder as nref
    from boosted_neural_ldpc_decoder.BoostedNeuralLDPCDecoder import BoostedNeuralLDPCDecoder
    from boosted_neural_ldpc_decoder.Functions import Functions
    from boosted_neural_ldpc_decoder.LDPCDecoderLoss import LDPCDecoderLoss
    from boosted_neural_ldpc_decoder.struct.DecoderType import DecoderType
    from boosted_neural_ldpc_decoder.struct.LossType import LossType
    from boosted_neural_ldpc_decoder.struct.NodeWeightSharingConfig import NodeWeightSharingConfig as NW

    torch.manual_seed(0)
    bg2 = np.loadtxt(os.path.join(res, "basegraph2_set0.txt"), int, delimiter="\t")
    M, N = bg2.shape
    E = int((bg2 != -1).sum())
    Z, B, T = 16, 6, 4
    x0 = ei.edge_batch(B, N, Z).numpy()
    y = np.zeros((B, N * Z), np.int8)  # the batch starts from the all-zero codeword's LLRs

    def save(name, **arrs):
        path = os.path.join(HERE, name + ".npz")
        np.savez_compressed(path, **arrs)
        print(f"wrote {name}.npz ({os.path.getsize(path) / 1024:.1f} KiB)")

    # ------------------------------------------------------------------ Neural
    w, b = (v.numpy() for v in ei.edge_neural_params(T, E))
    conn = nref.ConnectingMatrixTorch(nref.ConnectingMatrix(Z, bg2.copy()), device=torch.device("cpu"))
    model = nref.NeuralLDPCDecoder(T, B, conn)
    with torch.no_grad():
        for t in range(T):
            model.weights_var[t].copy_(torch.from_numpy(w[t]))
            model.biases_var[t].copy_(torch.from_numpy(b[t]))
    outs = model(torch.from_numpy(x0))
    yt = torch.from_numpy(y.astype(np.float32))
    loss = sum(torch.nn.functional.binary_cross_entropy_with_logits(o, yt) for o in outs) / T
    loss.backward()
    save("neural_bg2_z16_edges", x=x0, y=y, weights=w, biases=b, T=np.int32(T), Z=np.int32(Z), E=np.int32(E),
         outputs=np.stack([o.detach().numpy() for o in outs]).astype(np.float32), loss=np.float32(loss.item()),
         grad_w=np.stack([p.grad.numpy() for p in model.weights_var]).astype(np.float32),
         grad_b=np.stack([p.grad.numpy() for p in model.biases_var]).astype(np.float32))

    # ------------------------------------------------------------------ Boosted
    def boosted(name, dtype, q, nw, train):
        x = x0
        if dtype == DecoderType.QMS:
            x = np.asarray(Functions.Cal_MSA_Q(x0.astype(np.float64), q), dtype=np.float32)
        conn = bref.ConnectingMatrixTorch(bref.ConnectingMatrix(Z, bg2.copy()), device=torch.device("cpu"))
        model = BoostedNeuralLDPCDecoder(iter_node_counts=T, batch_size=B, connecting_matrix=conn,
                                         node_weight_sharing_config=NW(*nw), decoding_type=dtype, decoder_qms_qbit=q)
        tied = np.random.default_rng(7).uniform(0.5, 1.5, (3, T)).astype(np.float32)  # sharing code 3: no dead iteration
        src = {"CN": ei.edge_cn_weights(T, E).numpy(), "UCN": ei.edge_cn_weights(T, E, ei.SEED + 1).numpy(),
               "VN": ei.edge_vn_weights(T, N).numpy()}
        params = {}
        with torch.no_grad():
            for pname, p in model.named_parameters():
                _, node, t = pname.split("_")
                code = nw[("CN", "UCN", "VN").index(node)]
                v = src[node][int(t)] if code != 3 else tied[("CN", "UCN", "VN").index(node), int(t)]
                v = np.asarray(v, np.float32).reshape(tuple(p.shape))
                p.copy_(torch.from_numpy(v))
                params["param__" + pname] = v
        common = dict(x=x, y=y, T=np.int32(T), Z=np.int32(Z), q=np.int32(q), dtype=np.int32(dtype.value),
                      nw=np.array(nw, np.int32))
        if not train:
            with torch.no_grad():
                outs = model(torch.from_numpy(x))
            save(name, **common, fixed_nodes=np.array([], np.int32),
                 outputs=np.stack([o.numpy() for o in outs]).astype(np.float32), **params)
            return
        outs = model(torch.from_numpy(x), target_iter=list(range(T)))
        loss = LDPCDecoderLoss(loss_type=LossType.BCE, etha=1.0)(outs, torch.from_numpy(y.astype(np.float32)),
                                                                 coeff_param=list(range(len(outs))))
        loss.backward()
        grads = {"grad__" + n: p.grad.numpy().astype(np.float32) for n, p in model.named_parameters()
                 if p.grad is not None}
        save(name, **common, loss=np.float32(loss.item()), out_iters=np.arange(T, dtype=np.int32),
             outputs=np.stack([o.detach().numpy() for o in outs]).astype(np.float32), **params, **grads)

    QMS, MS, SP = DecoderType.QMS, DecoderType.MS, DecoderType.SP
    for tag, dt, q in (("ms", MS, 5), ("sp", SP, 5), ("qms5", QMS, 5), ("qms6", QMS, 6), ("qmsm5", QMS, -5),
                       ("qms4", QMS, 4), ("qms3", QMS, 3)):
        boosted(f"boosted_bg2_z16_{tag}_nw102_edges", dt, q, (1, 0, 2), False)
    boosted("boosted_bg2_z16_ms_nw112_edges", MS, 5, (1, 1, 2), False)
    boosted("boosted_bg2_z16_qms5_nw112_edges", QMS, 5, (1, 1, 2), False)
    boosted("train_bg2_z16_ms_nw102_edges", MS, 5, (1, 0, 2), True)
    boosted("train_bg2_z16_sp_nw303_edges", SP, 5, (3, 0, 3), True)
    boosted("train_bg2_z16_qms6_nw102_edges", QMS, 6, (1, 0, 2), True)
    boosted("train_bg2_z16_qms3_nw102_edges", QMS, 3, (1, 0, 2), True)


if __name__ == "__main__":
    main()
