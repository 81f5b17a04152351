"""MI355X-native neural belief-propagation LDPC decoding (host runtime).

Layers:
  nldpc._lib        ctypes binding of libnldpc.so (include/nldpc.h): HIP kernels for gfx950
  nldpc.graph       lifted QC graph as an edge list, device handles
  nldpc.decode      decode / autograd over nldpc_forward / nldpc_backward
  nldpc.channel     on-device AWGN channel and fused BER/FER counters
  nldpc.ratematch   circular-buffer rate matching and LLR rate recovery (TS 38.212 §5.4.2) around the channel
  nldpc.modulation  QAM modulation, soft demapping and the fused QAM/AWGN channel (TS 38.211 §5.1.3-5.1.6)
  nldpc.scrambling  Gold-sequence bit scrambling in front of the mapper and LLR descrambling behind the demapper
                    (TS 38.211 §5.2.1, §6.3.1.1, §7.3.1.1); modulation.qam_llr(scramble=) does both in the fused channel
  nldpc.fading      flat block fading (Rician / Rayleigh, drawn or given gains) with perfect-CSI demapping for the QAM
                    channel, fused like modulation.qam_llr and bit-identical to it at unit gain
  nldpc.mimo        spatial multiplexing of one codeword over 1, 2 or 4 layers, an nr x nt flat block-fading channel and
                    LMMSE soft detection in front of the demapper, fused like fading.qam_llr (TS 38.211 §6.3.1.3); or
                    exact max-log ML (joint) detection of the layers (detect_ml, qam_llr_ml)
  nldpc.crc         CRC attachment in front of the encoder, CRC checking and error accounting behind the decoder
                    (TS 38.212 §5.1)
  nldpc.transport   transport blocks: the TB CRC, code-block segmentation, per-block rate matching and concatenation,
                    and the TB verdict from the per-block remainders (TS 38.212 §5.2.2, §5.4.2.1, §5.5)
  nldpc.distributed one-process-per-GPU sharded decoding with an RCCL reduction of the counters
The drop-in packages neural_ldpc_decoder, boosted_neural_ldpc_decoder and checkpoint_utils (next to
this package) mirror the reference's Python API on top of it.
"""
from .graph import LiftedGraph  # noqa: F401
from .decode import DecodeCfg, decode, decode_autograd, KIND_SP, KIND_MS, KIND_QMS, KIND_NEURAL  # noqa: F401
