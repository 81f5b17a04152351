/*
 * nldpc.h — C ABI of the MI355X-native neural belief-propagation LDPC decoder.
 *
 * The reference (ShapeLayer/neural-ldpc-decoder-torch) has no FFI: its hot path is the Python
 * nn.Module API.  This header is the native boundary that the drop-in modules
 * (neural-ldpc-decoder-torch_amd/src/{neural_ldpc_decoder,boosted_neural_ldpc_decoder}) bind
 * through ctypes; each entry point names the reference interface it replaces.
 *
 * Conventions
 *   - int status: 0 = NLDPC_OK; anything else is an error, nldpc_last_error() gives the text
 *     (thread-local).  No C++ exception crosses this boundary.
 *   - Every tensor argument is a DEVICE pointer to contiguous fp32 (or the stated type) memory,
 *     allocated by the caller (e.g. the torch caching allocator).  Host arrays are marked "host".
 *   - All launches are stream-ordered on the `stream` argument (a hipStream_t); no entry point
 *     synchronises the device or allocates device memory, so every call is graph-capturable.
 *   - A graph handle owns only its device edge tables; it is immutable after creation and may be
 *     used from several streams at once.
 *   - Layouts: channel LLR xa [B][N][Z]; outputs [B][N*Z] (bit index j*Z+v, reference layout);
 *     message state [B][E][Z] with E in C-order (row-major over the base graph).
 */
#ifndef NLDPC_H
#define NLDPC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NLDPC_ABI_VERSION 4

enum nldpc_status {
    NLDPC_OK = 0,
    NLDPC_EINVAL = 1,      /* bad argument (ValueError on the Python side) */
    NLDPC_EHIP = 2,        /* HIP runtime error */
    NLDPC_EUNSUPPORTED = 3 /* valid but not implemented configuration */
};

/* Decoder kinds.  SP/MS/QMS keep the reference DecoderType values
 * (src/boosted_neural_ldpc_decoder/struct/DecoderType.py:4-7); NEURAL is
 * src/neural_ldpc_decoder/NeuralLDPCDecoder.py. */
enum nldpc_kind { NLDPC_SP = 0, NLDPC_MS = 1, NLDPC_QMS = 2, NLDPC_NEURAL = 3 };

typedef struct nldpc_graph nldpc_graph;

/* Per-call decoder configuration (the constructor arguments of BoostedNeuralLDPCDecoder,
 * BoostedNeuralLDPCDecoder.py:15-49, reduced to what the arithmetic needs). */
typedef struct nldpc_cfg {
    int32_t kind;    /* enum nldpc_kind */
    int32_t qbit;    /* QMS quantiser: 6, 5, -5, 4, 3; anything else = identity (:187-214) */
    int32_t ucn;     /* 1: compute unsatisfied-check flags and mix w_ucn (:339-374, :436-488) */
    int32_t vn_cumulative; /* 1: xin_t = Q(xin_{t-1} * w_vn[t]) (:325-337); 0: no VN weight */
    float llr_lo;    /* allowed_llr_range.start (Clipping, :36) */
    float llr_hi;    /* allowed_llr_range.end */
    int32_t first_iter; /* absolute index of the first iteration of this call (UCN uses xin at 0) */
    int32_t c2v_in;  /* 1: read the c2v state at the start; 0: start from all-zero messages */
    int32_t vn_prefix; /* rows of w_vn applied before this call's first iteration (cumulative VN
                          weighting carried over earlier iterations of the same forward) */
    int32_t flags;   /* NLDPC_FLAG_* */
} nldpc_cfg;

/* cfg->flags */
#define NLDPC_FLAG_STREAM 1      /* force the streaming (two kernels per iteration) path */
#define NLDPC_FLAG_FUSED 2       /* require the register-resident fused path (error if ineligible) */
#define NLDPC_FLAG_NO_STATE 4    /* the caller does not need the final c2v state: c2v may be NULL
                                    when the fused path runs */
#define NLDPC_FLAG_CN_TIED 8     /* (ABI 4, nldpc_backward; r6: also a saving nldpc_forward without UCN, which then runs
                                    a kernel that reads one CN weight per iteration, w_cn[t][0]) every row of w_cn
                                    repeats one weight (sharing code 3,
                                    BoostedNeuralLDPCDecoder.py:114-124): g_w_cn may receive each iteration's total
                                    in a few entries of its row and zeros elsewhere -- only row sums are meaningful,
                                    which is all a tied weight's gradient is.  The results (every gradient) are
                                    UNDEFINED unless every row of w_cn is one value: the tied kernel derives a row's
                                    check-node masks from its first weight (the Python side sets the flag only for a
                                    stride-0 expand, nldpc.decode._honour_tied) */

/* ---- library ---------------------------------------------------------------------------- */
int nldpc_abi_version(void);
const char* nldpc_last_error(void);

/* ---- graph: replaces ConnectingMatrix(Z, basegraph) + ConnectingMatrixTorch(cm, device)
 *      (src/boosted_neural_ldpc_decoder/ConnectingMatrix.py:5-80, ConnectingMatrixTorch.py:7-54;
 *       src/neural_ldpc_decoder/ConnectingMatrix.py:4-66, ConnectingMatrixTorch.py:7-46).
 *      basegraph: host [M*N] row-major shift table, -1 = no edge; shifts are taken mod Z. ------ */
int nldpc_graph_create(int32_t M, int32_t N, int32_t Z, const int32_t* basegraph, int32_t device,
                       nldpc_graph** out);
int nldpc_graph_destroy(nldpc_graph* g);
/* dims[0..7] = M, N, Z, E, max check degree, max variable degree, device, reserved */
int nldpc_graph_dims(const nldpc_graph* g, int32_t* dims);
/* host copies of the C-order edge tables: check, variable, shift (mod Z) of every edge */
int nldpc_graph_edges(const nldpc_graph* g, int32_t* chk, int32_t* var, int32_t* shift);
/* (ABI 3) A register-resident kernel compiled at run time for this lifted graph (gen_fused.py --jit
 *      output, `hipcc --genco` for gfx950; entry point nldpc_fx, or nldpc_fxb for the backward): the
 *      library's own fused kernels cover a fixed set of (base graph, Z); any other graph gets its kernels
 *      this way, per mode (0 decode, 1 decode + save for backward, 2 / 3 count-only, 4 backward) and
 *      kind, with the geometry they were generated for (codewords per workgroup, threads, waves per
 *      part).  The graph keeps the loaded module until nldpc_graph_destroy.  No-op for a graph the
 *      library already covers.  Replaces nothing in the reference (its dense path has no per-Z code);
 *      it is what makes ConnectingMatrix(Z, basegraph) at any Z (ConnectingMatrix.py:5-53) fast.
 *      The code object's global nldpc_sig (the kernel argument layout it was generated for) must be this
 *      library's, else NLDPC_EUNSUPPORTED (r5: a skewed build is refused instead of running a kernel that
 *      leaves its outputs unwritten).  r6: the signature is read from the host copy of the code object (no
 *      device copy, no wait on work in flight).  Loading the module (hipModuleLoadData) is not a stream
 *      operation: attach a geometry's kernels -- i.e. run the first decode of a run-time geometry -- outside
 *      any stream / graph capture (nldpc.jit compiles and attaches on that first call). */
int nldpc_graph_attach_kernel(nldpc_graph* g, int32_t mode, int32_t kind, const void* code, size_t bytes,
                              int32_t G, int32_t threads, int32_t waves_per_part);
/* (r6, additive to ABI 4) The argument-layout signature a code object was generated for (its nldpc_sig, read on the host from
 *      the hipcc --genco offload bundle or a bare gfx950 ELF) and the one this library's mode needs (mode 0-3:
 *      forward kernels, 4: backward).  NLDPC_EINVAL when the object carries no readable nldpc_sig.  Lets a
 *      caller validate a cached code object before nldpc_graph_attach_kernel; no device is touched. */
int nldpc_code_object_sig(const void* code, size_t bytes, int32_t mode, uint32_t* sig, uint32_t* expected);
/* (ABI 3) *mask: bit (mode * 4 + kind) set when that fused kernel exists for the graph (modes as above) */
int nldpc_graph_kernels(const nldpc_graph* g, uint32_t* mask);

/* ---- execution path.  *eligible = 1 when nldpc_forward with these arguments runs the fused
 *      register-resident kernel: a (base graph, lifting size) compiled in, no incoming message state
 *      (c2v_in == 0; a resumed UCN segment passes app_prev instead), T <= 64, no NLDPC_FLAG_STREAM;
 *      every kind, UCN and cumulative VN weights included, saving for backward included; QMS only
 *      with an active quantiser (qbit 3, 4, 5, -5, 6: an identity quantiser decodes on the streaming
 *      kernels, r3).  Then v2c is unused, and c2v is unused too with
 *      NLDPC_FLAG_NO_STATE.  Otherwise the streaming kernels run and need both buffers. */
int nldpc_fast_path(const nldpc_graph* g, const nldpc_cfg* cfg, int64_t B, int32_t T, int32_t saving,
                    int32_t* eligible);
/*      (ABI 3) saving = 2 / 3 asks the same for nldpc_forward_count (all-zero codeword, decoder convention /
 *      any convention or codeword), whose fused kernels are separate variants; saving = 4 asks it for
 *      nldpc_forward_early_stop (additionally: no UCN, first_iter == 0). */

/* ---- decode forward: replaces NeuralLDPCDecoder.forward (NeuralLDPCDecoder.py:44-100) and
 *      BoostedNeuralLDPCDecoder.forward (BoostedNeuralLDPCDecoder.py:260-538).
 *   T        iterations run by this call (iteration k of the call = absolute cfg->first_iter + k)
 *   xa       [B][N][Z] channel LLRs
 *   w_cn     [T][E] per-edge check-node weight, NULL = |x| (sharing code 0).  Shared codes (per
 *            check, per iteration) are expanded to per-edge by the caller.
 *   w_ucn    [T][E] per-edge UCN weight (cfg->ucn), else NULL
 *   bias     [T][E] per-edge bias (NEURAL), else NULL
 *   w_vn     [vn_prefix + T][N] per-column VN weights (cfg->vn_cumulative), else NULL; iteration k
 *            of the call uses xin = Q(..Q(xa*w_vn[0])..*w_vn[vn_prefix+k])
 *   outs     host array of T device pointers, each [B][N*Z]; NULL entries are not written
 *            (with cfg->ucn every entry but the last must be non-NULL: iteration k reads k-1)
 *   app_prev [B][N*Z] posterior of iteration first_iter-1 (UCN with first_iter > 0), else NULL
 *   c2v      [B][E][Z] message state in/out: read at the start when cfg->c2v_in (otherwise a
 *            fresh all-zero state), holds the state after the last iteration on return
 *   v2c      [B][E][Z] scratch of the streaming path (unused, may be NULL, when nldpc_fast_path
 *            reports 1; also NULL-able for a non-QMS training call, which streams through `saved`)
 *   saved    device buffer of nldpc_saved_bytes() bytes that receives what nldpc_backward needs
 *            (every iteration's variable-to-check messages -- fp32, or for QMS one int8 code per
 *            message holding Q(m) and its clip mask --, the Boosted output clamp masks, and the
 *            cumulative-VN-weight channel values), or NULL (inference); needs every `outs` entry
 *   stream   hipStream_t */
int nldpc_saved_bytes(const nldpc_graph* g, const nldpc_cfg* cfg, int64_t B, int32_t T, size_t* bytes);
int nldpc_forward(const nldpc_graph* g, const nldpc_cfg* cfg, int64_t B, int32_t T, const float* xa,
                  const float* w_cn, const float* w_ucn, const float* bias, const float* w_vn,
                  float* const* outs, const float* app_prev, float* c2v, float* v2c, void* saved,
                  void* stream);

/* ---- decode backward (config 5: training through the unrolled decoder; the reference gets this
 *      from autograd over BoostedNeuralLDPCDecoder.py:320-526 / NeuralLDPCDecoder.py:54-98).
 *   outs       forward outputs (needed for UCN flags and the output clamp mask)
 *   grad_outs  host array of T device pointers [B][N*Z] (NULL entry = zero gradient)
 *   saved      as written by nldpc_forward
 *   grad_c2v_out [B][E][Z] gradient arriving at the final message state (the state a later segment
 *              of the same forward resumed from: list-valued xa, split iteration runs), or NULL
 *   grad_c2v_in  [B][E][Z] out: gradient of the incoming message state (cfg->c2v_in), or NULL
 *              (either of the two selects the streaming backward)
 *   g_w_cn, g_w_ucn, g_bias: [T][E] accumulated (+=) per-edge gradients, NULL if not wanted
 *   g_w_vn     [vn_prefix + T][N] accumulated (+=) per-column gradients, NULL if not wanted
 *   work       device scratch of nldpc_backward_workspace() bytes */
int nldpc_backward_workspace(const nldpc_graph* g, const nldpc_cfg* cfg, int64_t B, int32_t T,
                             size_t* bytes);
int nldpc_backward(const nldpc_graph* g, const nldpc_cfg* cfg, int64_t B, int32_t T, const float* xa,
                   const float* w_cn, const float* w_ucn, const float* bias, const float* w_vn,
                   const float* const* outs, const float* const* grad_outs, const float* app_prev,
                   const void* saved, const float* grad_c2v_out, float* grad_c2v_in, float* g_w_cn,
                   float* g_w_ucn, float* g_bias, float* g_w_vn, void* work, size_t work_bytes, void* stream);

/* ---- BER/FER accounting: replaces Functions.evaluate_ber_fer (Functions.py:85-102) and the
 *      per-iteration .item() loop of train/train_BoostedNeuralLDPCDecoder.py:363-383.
 *   llr [B][L]; y [B][L] uint8 bits or NULL (all-zero codeword); counts int64[2] += (bit errors,
 *   frame errors).  convention 0: bit = (LLR > 0) (decoder convention);
 *   convention 1: bit = (LLR < 0) (the reference helper's literal, inverted rule). */
int nldpc_ber_count(const float* llr, const uint8_t* y, int64_t B, int64_t L, int32_t convention,
                    int64_t* counts, void* stream);

/* ---- count-only decode (§8 F2): nldpc_forward followed by nldpc_ber_count on every iteration's
 *      output (the test loop of test/test_*.py around Functions.evaluate_ber_fer, Functions.py:85-102),
 *      fused into the decoder: each iteration's posterior is compared with the codeword bit inside
 *      the register-resident kernel and only the counts leave the chip (no T x [B][N*Z] outputs).
 *   arguments as nldpc_forward (no outs / app_prev / c2v / v2c / saved); y [B][N*Z] uint8 bits or
 *   NULL (all-zero codeword); counts int64 [T][2] device, += (bit errors, frame errors) of iteration
 *   first_iter + k in row k; convention as nldpc_ber_count.  Needs the fused path (nldpc_fast_path
 *   with saving = 0 reports 1), NLDPC_EUNSUPPORTED otherwise. */
int nldpc_forward_count(const nldpc_graph* g, const nldpc_cfg* cfg, int64_t B, int32_t T, const float* xa,
                        const float* w_cn, const float* w_ucn, const float* bias, const float* w_vn,
                        const uint8_t* y, int32_t convention, int64_t* counts, void* stream);

/* ---- parity-check syndrome weight (additive to ABI 4): is a decoder output a codeword?
 *   llr [B][N*Z]; unsat int32 [B] device, overwritten: the number of the M*Z lifted check rows whose XOR of the
 *   hard decisions over the row's edges is 1 (edge (i, j, s) joins check copy h to variable copy (h + s) mod Z,
 *   as nldpc_graph_edges lists them); 0 = the hard decision is a codeword.  convention as nldpc_ber_count
 *   (0: bit = LLR > 0, an exact 0 is bit 0).  Reads the graph's device edge tables; any graph and Z, no fused
 *   kernel needed; stream-ordered, no synchronisation, no allocation. */
int nldpc_syndrome(const nldpc_graph* g, const float* llr, int64_t B, int32_t convention, int32_t* unsat,
                   void* stream);

/* ---- early-stopping decode (additive to ABI 4): nldpc_forward, stopped per codeword at the first iteration whose
 *      hard decision (LLR > 0) satisfies every parity check.  With t*(b) the smallest t in 0..T-1 whose posterior
 *      has syndrome weight 0, or T-1 if there is none:
 *   out    [B][N*Z]  out[b] = the posterior of iteration t*(b), bit for bit what nldpc_forward writes there
 *   iters  int32 [B] t*(b) + 1, or NULL
 *   unsat  int32 [B] syndrome weight of out[b] (0 = a codeword), or NULL; filled by an nldpc_syndrome launch on out
 *   other arguments as nldpc_forward_count.  Inference only: no saved buffer, c2v_in == 0, first_iter == 0, no UCN.
 *   Runs the register-resident early-stop kernels (a MODE of their own; the parity of every check copy is taken
 *   inside the kernel each iteration, and a workgroup leaves as soon as all its codewords have stopped), which the
 *   library builds for its compiled base graphs only: a run-time compiled geometry (nldpc_graph_attach_kernel) has
 *   no such kernel and gets NLDPC_EUNSUPPORTED like every other ineligible call (c2v_in, first_iter > 0, T > 64,
 *   UCN, NLDPC_FLAG_STREAM, no compiled graph); nldpc_fast_path with saving = 4 answers for this entry point.
 *   The fallback is nldpc_forward with all T outputs, nldpc_syndrome on each and a selection (nldpc.decode does it). */
int nldpc_forward_early_stop(const nldpc_graph* g, const nldpc_cfg* cfg, int64_t B, int32_t T, const float* xa,
                             const float* w_cn, const float* w_ucn, const float* bias, const float* w_vn,
                             float* out, int32_t* iters, int32_t* unsat, void* stream);

/* ---- multi-iteration BCE loss (config 5's training loss): replaces LDPCDecoderLoss.forward with
 *      LossType.BCE over a list of outputs and one label tensor
 *      (src/boosted_neural_ldpc_decoder/LDPCDecoderLoss.py:70-108, binary_cross_entropy_with_logits
 *      per term) and its autograd backward, in one pass over the T outputs instead of a chain of
 *      elementwise ops per term.
 *   logits   host array of K device pointers, each [n] fp32 (K <= 64)
 *   coef     host [K]: weight of term k (etha^c_k / sum_k etha^c_k)
 *   target   [n] fp32 labels shared by every term, or NULL (all zero)
 *   loss     device fp32 scalar out: sum_k coef[k] * mean_i bce(logits[k][i], target[i]), with
 *            bce(x, t) = (1 - t) * x - log_sigmoid(x) (fp32 terms, fp64 fixed-order sums)
 *   work     device scratch of nldpc_bce_workspace() bytes
 *   grads    (nldpc_bce_grad) K device pointers [n]: grads[k][i] = (*gseed) * coef[k] / n *
 *            (sigmoid(logits[k][i]) - target[i]); gseed is a device fp32 scalar (dL/dloss) */
int nldpc_bce_workspace(int64_t n, int32_t K, size_t* bytes);
int nldpc_bce_loss(const float* const* logits, int32_t K, const float* coef, const float* target, int64_t n,
                   float* loss, void* work, size_t work_bytes, void* stream);
int nldpc_bce_grad(const float* const* logits, int32_t K, const float* coef, const float* target, int64_t n,
                   const float* gseed, float* const* grads, void* stream);
/* The training step's pair in one pass over the logits (read once for the loss and the gradients): the
 * loss as nldpc_bce_loss and grads[k] as nldpc_bce_grad would write them for *gseed == 1 (what
 * loss.backward() sends), bit for bit.  nldpc_bce_grad_unless_unit then runs at backward time with the
 * seed that arrived: it returns at once on the device when *gseed == 1 and otherwise overwrites grads
 * as nldpc_bce_grad does, so the pair equals nldpc_bce_loss + nldpc_bce_grad for any seed. */
int nldpc_bce_loss_grad(const float* const* logits, int32_t K, const float* coef, const float* target, int64_t n,
                        float* loss, float* const* grads, void* work, size_t work_bytes, void* stream);
int nldpc_bce_grad_unless_unit(const float* const* logits, int32_t K, const float* coef, const float* target,
                               int64_t n, const float* gseed, float* const* grads, void* stream);

/* ---- synthetic AWGN channel (the step before the path; replaces the all-zero branch of
 *      AWGNPassedDatagen, boosted.../AWGNPassedDatagen.py:75-134, generated on the device):
 *   xa[b][n] = 2*(-1 + sigma*g)/sigma^2 with g ~ N(0,1) from Philox-4x32-10(seed) at counter
 *   (b_offset + b)*L + n, so a sharded run draws the same noise as a single-device run.
 *   qbit != 0 applies the QMS quantiser (Functions.Cal_MSA_Q, Functions.py:69-83). */
int nldpc_awgn_llr(float* xa, int64_t B, int64_t L, float sigma, uint64_t seed, int64_t b_offset,
                   int32_t qbit, void* stream);
/* ---- the same channel with the rest of AWGNPassedDatagen._gendata_* (AWGNPassedDatagen.py:75-134,
 *      §8 F1): y [B][L] uint8 codeword bits (NULL = all-zero), BPSK (-1)^(1-y); after the quantiser,
 *      bits [puncture_start-1, puncture_end) of every codeword are set to puncture_value (the
 *      reference: 0, or 0.001 for SP) and bits [shorten_start-1, shorten_end) to shorten_value
 *      (-|allowed_llr_range.end|); a start of 0 disables the range (Puncture(0, 0) / Shortening(0, 0)).
 *      nldpc_awgn_llr(...) == nldpc_channel_llr(..., NULL, 0, 0, 0, 0, 0, 0, stream). */
int nldpc_channel_llr(float* xa, int64_t B, int64_t L, float sigma, uint64_t seed, int64_t b_offset,
                      int32_t qbit, const uint8_t* y, int64_t puncture_start, int64_t puncture_end,
                      float puncture_value, int64_t shorten_start, int64_t shorten_end, float shorten_value,
                      void* stream);

/* ---- systematic QC-LDPC encoder (additive to ABI 4): the codewords the channel, the count-only decode and the
 *      error counters take as y.  The reference has one generator matrix (resources/gen_matrix_bg2_z16.txt, BG2
 *      z=16 only; train/train_BoostedNeuralLDPCDecoder.py multiplies info bits by it); this encodes for any base
 *      graph whose parity part can be solved by substitution, at any Z.  Info columns are the first K = N - M base
 *      columns, parity columns the last M.
 *   nldpc_encode_plan (host only, no device): the substitution order.  A parity column with one entry is solved
 *      last from its own row; in the remaining core a row with one unsolved parity column solves it, and when none is
 *      left the XOR of the unused core rows must leave exactly one monomial on the unsolved columns (5G BG1/BG2 and
 *      802.16e: the weight-3 column).  Step s (M steps, sorted by dependency level step_level[s] in 0..*n_levels-1)
 *      sets y[step_col[s]][(h + step_shift[s]) mod Z] to the XOR over its terms k in step_ptr[s]..step_ptr[s+1] of
 *      y[term_col[k]][(h + term_shift[k]) mod Z], for every check copy h; every term column is an info column or the
 *      target of a step of a lower level; all degree-1 columns share one level.
 *      step_col / step_shift / step_level host [M], step_ptr host [M+1], term_col / term_shift host [term_cap].
 *      NLDPC_EUNSUPPORTED: the graph has no such order; NLDPC_EINVAL: term_cap too small (2 * E always suffices).
 *   nldpc_encode: info [B][K*Z] uint8 (any non-zero byte is 1) -> y [B][N*Z] uint8 0/1, y[b][0..K*Z) = the info bits
 *      and every parity check of y[b] satisfied.  info == NULL: the info bits come from Philox-4x32-10: with
 *      c = b_offset + b and W = ceil(K*Z / 128), bit i of codeword c is bit (i & 31) of output word (i >> 5) & 3 at
 *      counter (lo32(c*W + (i >> 7)), hi32(c*W + (i >> 7)), 0x454E4331, 0), key (lo32(seed), hi32(seed)) -- the
 *      noise stream of nldpc_channel_llr has 0 in counter word 2 --, so a sharded batch draws the words of the
 *      unsharded one.  One kernel over the plan's device tables, which nldpc_graph_create builds; stream-ordered,
 *      no synchronisation, no allocation.  NLDPC_EUNSUPPORTED: the graph has no plan, or N*Z bytes do not fit the
 *      kernel's LDS image. */
int nldpc_encode_plan(int32_t M, int32_t N, int32_t Z, const int32_t* basegraph, int32_t* step_col,
                      int32_t* step_shift, int32_t* step_level, int32_t* step_ptr, int32_t* term_col,
                      int32_t* term_shift, int32_t term_cap, int32_t* n_levels);
int nldpc_encode(const nldpc_graph* g, const uint8_t* info, int64_t B, uint64_t seed, int64_t b_offset, uint8_t* y,
                 void* stream);

/* ---- circular-buffer rate matching and LLR rate recovery (additive to ABI 4): implements the bit selection and bit
 *      interleaving of 3GPP TS 38.212 §5.4.2 (filler skipping, redundancy-version start, limited buffer), generalised
 *      to graphs without 5G's two punctured columns.  The reference has no counterpart: it runs a graph at its mother
 *      rate, apart from one Puncture(start, end) range (nldpc_channel_llr).
 *   With K = N - M, P = punct_cols * Z, codeword y[0 .. N*Z): the buffer is d[p] = y[P + p], p in [0, Ncb), Ncb = ncb or
 *      N*Z - P when ncb == 0; the last F = n_filler info bits (buffer positions [f0, f1) = [K*Z - F - P, K*Z - P)) are
 *      known zeros and never sent.  Selection (§5.4.2.1): k = j = 0; while k < E: p = (k0 + j) mod Ncb; if p is not a
 *      filler, e[k++] = d[p]; j++.  Interleaver (§5.4.2.2): f[i + j*qm] = e[i*(E/qm) + j], i < qm, j < E/qm.
 *   Rules (NLDPC_EINVAL otherwise): 0 <= punct_cols <= K; 0 <= F <= (K - punct_cols)*Z; ncb == 0 or
 *      K*Z - P <= ncb <= N*Z - P; Ncb - F >= 1; 0 <= k0 < Ncb; E >= 1, qm >= 1, E % qm == 0; E < 2^31, N*Z < 2^31.
 *   nldpc_rm_k0 (host only): Table 5.4.2.1-2, k0 = floor(num * ncb / (den * Z)) * Z with num / den for rv 0..3 =
 *      {0, 17, 33, 56} / 66 (bg 1), {0, 13, 25, 43} / 50 (bg 2); ncb > 0 (the resolved buffer length).
 *   nldpc_rm_index (host only, no device, no graph handle): idx[m], m in [0, E), = the codeword bit index f[m]
 *      carries, computed with the inline functions the kernels use (csrc/nldpc_rm_index.h).
 *   nldpc_rate_match: y [B][N*Z] uint8 (any non-zero byte is 1) -> f [B][E] uint8 0/1, f[b][m] = y[b][idx[m]].
 *   nldpc_rate_recover: llr [B][E] fp32 in the order of f -> xa [B][N][Z] fp32 (the decoder's input).  Per codeword
 *      position n: a filler position is set to filler_value (the shortening convention: -|llr_hi|); a position that
 *      idx names at least once gets acc = (accumulate ? xa[n] : +0) plus its received values added one by one in
 *      ascending selection index k (one fp32 rounding each), clamped to [-clip, clip] when clip > 0 (a NaN stays a
 *      NaN); every other position (n < P, beyond the buffer, never selected) is set to erasure_value when
 *      accumulate == 0 and left unwritten when accumulate == 1.  A further redundancy version is soft-combined by
 *      calling again with accumulate = 1 on the same xa.  The Neural check node masks exact zeros out of its minimum
 *      (NeuralLDPCDecoder.py:74-75), so an erasure_value of 0 is not an erasure for it: use a small non-zero value.
 *   Both launches are stream-ordered, synchronise and allocate nothing, write nothing outside f / xa, and work for
 *      any graph and Z (only the graph's dimensions are read; no fused kernel, no device table). */
typedef struct nldpc_rm {
    int32_t punct_cols;  /* leading base columns never sent (5G: 2; otherwise 0) */
    int32_t qm;          /* interleaver rows; 1 = none; divides E */
    int64_t n_filler;    /* F */
    int64_t ncb;         /* 0 = the full buffer N*Z - P */
    int64_t k0;          /* start position in the buffer */
    int64_t E;           /* bits sent per codeword */
} nldpc_rm;
int nldpc_rm_k0(int32_t bg, int32_t rv, int64_t ncb, int32_t Z, int64_t* k0);
int nldpc_rm_index(int32_t M, int32_t N, int32_t Z, const nldpc_rm* rm, int32_t* idx);
int nldpc_rate_match(const nldpc_graph* g, const nldpc_rm* rm, const uint8_t* y, int64_t B, uint8_t* f,
                     void* stream);
int nldpc_rate_recover(const nldpc_graph* g, const nldpc_rm* rm, const float* llr, int64_t B, float erasure_value,
                       float filler_value, float clip, int32_t accumulate, float* xa, void* stream);

/* ---- QAM modulation and soft demapping (additive to ABI 4): the channel between nldpc_rate_match and
 *      nldpc_rate_recover for the modulations NR uses with LDPC (3GPP TS 38.211 §5.1.3-5.1.6: QPSK, 16-, 64-, 256-QAM);
 *      nldpc_channel_llr stays the BPSK channel (qm = 1).  The reference has no counterpart (BPSK only,
 *      AWGNPassedDatagen.py:97-103).  The arithmetic is the inline functions of csrc/nldpc_qam.h on host and device.
 *   qm in {2, 4, 6, 8}, h = qm / 2.  A symbol carries qm consecutive bits b_0 .. b_{qm-1} of f, f[b][s*qm + i] -- the
 *      grouping nldpc_rate_match's interleaver produces with the same qm --; its I dimension takes c_k = b_{2k}, its Q
 *      dimension c_k = b_{2k+1}, k < h.  Integer amplitude a = (1-2c_0)[2^{h-1} - (1-2c_1)[2^{h-2} - .. - (1-2c_{h-1})]]
 *      (odd, |a| <= 2^h - 1); level = (float)a * A, one fp32 rounding, A = the fp32 nearest to 1/sqrt(2), 1/sqrt(10),
 *      1/sqrt(42), 1/sqrt(170) (unit average symbol energy).  Symbols are interleaved fp32 pairs (I, Q), S = E / qm
 *      per codeword.
 *   LLR = log P(b=1)/P(b=0): LLR > 0 means bit 1 (nldpc_ber_count convention 0, the decoders).  38.211 keeps bit 0 on
 *      the positive side, so a noiseless symbol gives negative LLRs for its 0 bits.
 *   Demapper, per real dimension with received x: for each of the 2^h levels l, t = x - l and d = t * t (two fp32
 *      roundings, no FMA); w = (float)(1.0 / (2.0 * (double)sigma * (double)sigma)); sigma is the noise standard
 *      deviation per real dimension.
 *        method 0 (max-log): LLR_k = (min_{c_k=0} d - min_{c_k=1} d) * w
 *        method 1 (log-MAP): with m = -(d * w), lse_v = M_v + logf(sum_{c_k=v} expf(m - M_v)), M_v = max_{c_k=v} m, the
 *                            sum in ascending order of the label c_0 .. c_{h-1} read as a binary number, from +0;
 *                            LLR_k = lse_1 - lse_0 (fp32 throughout)
 *   nldpc_qam_points (host only): iq[2v], iq[2v+1] = (I, Q) of the symbol of bits b_i = (v >> (qm-1-i)) & 1, v < 2^qm.
 *   nldpc_qam_demap_ref (host only, no device): sym host [S][2] -> llr host [S*qm], the functions the kernels run.
 *   nldpc_qam_modulate: f [B][E] uint8 (any non-zero byte is 1) -> sym [B][S][2].
 *   nldpc_qam_demap: sym [B][S][2] -> llr [B][S*qm] in the order of f.
 *   nldpc_qam_channel_llr: bits -> symbols -> AWGN -> LLRs in one kernel (no symbol goes through memory).  f NULL = the
 *      all-zero word.  Noisy symbol r = (float)((double)level + (double)sigma * n), one rounding per dimension; llr is
 *      bit for bit what nldpc_qam_demap computes from those r; sym_out (nullable) receives the r, [B][S][2].  n: with
 *      G = (b_offset + b) * S + s the global index of a symbol, the four fp64 Box-Muller normals of nldpc_channel_llr
 *      (sqrt(-2 ln u0) cos(2 pi u1), .. sin .., the same of (u2, u3); u = (word + 1) / 2^32) of Philox-4x32-10 at
 *      counter (lo32(G >> 1), hi32(G >> 1), 0x51414D31, 0), key (lo32(seed), hi32(seed)), are (I, Q) of the even symbol
 *      2 (G >> 1), then (I, Q) of the odd one.  Counter word 2 ("QAM1") keeps the stream apart from the BPSK noise (0)
 *      and the encoder's info bits (0x454E4331); a shard that starts at b_offset draws the unsharded batch's noise,
 *      also when S and b_offset are odd and a pair straddles two codewords.
 *   NLDPC_EINVAL: qm not in {2, 4, 6, 8}, method not 0 / 1, E % qm != 0, !(sigma > 0), B <= 0, E <= 0 (S <= 0),
 *      E >= 2^31 (S * qm >= 2^31), b_offset < 0, a NULL required pointer, a float pointer off a 4-byte boundary (f may
 *      start anywhere).  NLDPC_EUNSUPPORTED: B or b_offset >= 2^31.
 *   The three launches are stream-ordered on the current device, synchronise and allocate nothing and write nothing
 *      outside sym / llr / sym_out. */
int nldpc_qam_points(int32_t qm, float* iq);
int nldpc_qam_demap_ref(int32_t qm, int32_t method, float sigma, const float* sym, int64_t S, float* llr);
int nldpc_qam_modulate(int32_t qm, const uint8_t* f, int64_t B, int64_t E, float* sym, void* stream);
int nldpc_qam_demap(int32_t qm, int32_t method, float sigma, const float* sym, int64_t B, int64_t S, float* llr,
                    void* stream);
int nldpc_qam_channel_llr(int32_t qm, int32_t method, const uint8_t* f, int64_t B, int64_t E, float sigma,
                          uint64_t seed, int64_t b_offset, float* llr, float* sym_out, void* stream);

/* ---- CRC attachment and checking (additive to ABI 4): the cyclic redundancy checks of 3GPP TS 38.212 §5.1, the step in
 *      front of nldpc_encode and behind the decoder.  The reference has no counterpart (its error figures all need the
 *      transmitted word).  The arithmetic is the inline functions of csrc/nldpc_crc.h on host and device.
 *   Polynomials: enum nldpc_crc, lengths L = 24, 24, 24, 16, 11, 6; without the leading term x^L they are 0x864CFB,
 *      0x800063, 0xB2B117, 0x1021, 0x621, 0x21.
 *   Rule: bits a_0 .. a_{A-1} get parity p_0 .. p_{L-1} so that a_0 x^{A+L-1} + .. + a_{A-1} x^L + p_0 x^{L-1} + .. +
 *      p_{L-1} is divisible by g(x) over GF(2).  The register starts at zero, nothing is reflected and there is no
 *      final XOR.  A block passes when the remainder of its first A + L bits is zero.  Two consequences: leading zero
 *      bits do not change the remainder (a payload may be padded in front for free), and the all-zero block passes (an
 *      all-zero posterior, e.g. of a dead input, is not flagged; nldpc_syndrome does not flag it either).  A CRC pass and
 *      syndrome weight 0 are different verdicts: a wrong codeword has syndrome 0 and, but for a chance of 2^-L, fails
 *      its CRC.
 *   nldpc_crc_ref (host only, no device): *parity = the L parity bits of bits[0..A) (any non-zero byte is 1), p_0 the
 *      most significant of the low L bits.  Computed with the functions the kernels use: the remainder of each
 *      chunk-bit piece (the last may be shorter), multiplied by x^n mod g for the n bits that follow it, XORed
 *      together; chunk >= 1 is the caller's, every value gives the same result.
 *   nldpc_crc_attach: a [B][A] uint8 (any non-zero byte is 1), or NULL -> info [B][W] uint8, written in full: [0, A) the
 *      payload as 0 / 1, [A, A+L) the parity, p_0 first, [A+L, W) zeros (filler bits).  With W = K*Z this is
 *      nldpc_encode's info, and nldpc_rm.n_filler = W - A - L.  a == NULL: the payload is drawn on the device from the
 *      encoder's info-bit stream: bit i < A of block c = b_offset + b is the bit nldpc_encode(info = NULL) documents
 *      for a row of K*Z = W bits (counter word 2 = 0x454E4331, W' = ceil(W / 128) counters per block), so the first A
 *      bits equal those of nldpc_encode with the same seed and a sharded batch draws the unsharded one's payloads.
 *      NLDPC_EINVAL unless B >= 1, A >= 1, A + L <= W < 2^31, b_offset >= 0, info non-NULL; NLDPC_EUNSUPPORTED for B or
 *      b_offset >= 2^31.
 *   nldpc_crc_check: exactly one of llr (fp32 [B][stride]; hard decision by `convention` as nldpc_ber_count, so an
 *      exact 0, -0 or NaN is bit 0 under convention 0) and bits (uint8 [B][stride], non-zero is 1) is given; the first
 *      A + L positions of each row are checked.  stride >= A + L is in elements and need not be a multiple of anything:
 *      a decoder posterior [B][N*Z] is passed as it is (its first K*Z positions are the info bits).  ok: uint8 [B],
 *      nullable, 1 when the block passes, else 0.  ref: nullable, the true bits [B][ref_stride] (e.g. nldpc_encode's y
 *      with ref_stride = N*Z, >= A + L).  counts: nullable device int64[3], += as nldpc_ber_count does: [0] blocks whose
 *      CRC fails; [1] blocks whose CRC passes although their A + L bits differ from ref (undetected errors); [2] blocks
 *      whose A + L bits differ from ref; [1] and [2] get nothing without ref.  At least one of ok and counts is non-NULL.
 *      NLDPC_EINVAL: B < 1, A < 1, A + L >= 2^31, a stride below A + L, convention not 0 / 1, both or neither of llr and
 *      bits, ok and counts both NULL, llr off a 4-byte or counts off an 8-byte boundary; NLDPC_EUNSUPPORTED: B >= 2^31.
 *   Both launches are stream-ordered on the current device, synchronise and allocate nothing, write nothing outside
 *      info / ok / counts and need no graph handle. */
enum nldpc_crc { NLDPC_CRC24A = 0, NLDPC_CRC24B, NLDPC_CRC24C, NLDPC_CRC16, NLDPC_CRC11, NLDPC_CRC6 };
int nldpc_crc_ref(int32_t crc, const uint8_t* bits, int64_t A, int64_t chunk, uint32_t* parity);
int nldpc_crc_attach(int32_t crc, const uint8_t* a, int64_t B, int64_t A, int64_t W, uint64_t seed, int64_t b_offset,
                     uint8_t* info, void* stream);
int nldpc_crc_check(int32_t crc, const float* llr, const uint8_t* bits, int64_t B, int64_t A, int64_t stride,
                    int32_t convention, const uint8_t* ref, int64_t ref_stride, uint8_t* ok, int64_t* counts,
                    void* stream);

/* ---- transport blocks (additive to ABI 4): code-block segmentation with the code-block CRC (3GPP TS 38.212 §5.2.2),
 *      the per-block rate-matching lengths E_r (§5.4.2.1), code-block concatenation (§5.5) and, at the receiver, the
 *      inverses and the transport-block verdict.  The reference has no counterpart.  The arithmetic is the inline
 *      functions of csrc/nldpc_tb.h and csrc/nldpc_crc.h on host and device.
 *   Sizes: a payload of A bits carries a TB CRC (tb_crc, one of enum nldpc_crc; §5.1 uses CRC24A, or CRC16 up to A = 3824)
 *      of L_tb bits: B' = A + L_tb.  The TB is cut into C parts of K' - L bits, B' = C (K' - L); a part followed by its
 *      CRC24B of L bits (L = 24, or 0 when C == 1: no code-block CRC) and F = W - K' filler zeros is one code block, a row
 *      of W bits (nldpc_encode's info with W = K*Z; nldpc_rm.n_filler = F).
 *   Layout: a batch of Btb transport blocks is BLOCK-MAJOR: code block r of TB t is row r * Btb + t of every
 *      per-code-block array, so the blocks that share a rate-matching length are one contiguous range of rows and
 *      nldpc_encode, nldpc_rate_match, nldpc_rate_recover, the decoders and nldpc_crc_check run on it unchanged.
 *   nldpc_tb_plan (host only): B' = A + L_tb; kcb == 0 means W; B' <= kcb: C = 1, L = 0; otherwise L = 24 and
 *      C = ceil(B' / (kcb - 24)); B'' = B' + C L, K' = B'' / C, F = W - K'.  NLDPC_EINVAL: tb_crc not of enum nldpc_crc,
 *      A < 1, W < 1, kcb < 0, kcb > W, kcb <= 24 when B' > kcb, C does not divide B'', K' > W, or A, W, kcb, B' or
 *      B'' >= 2^31.  The launches below take any plan that satisfies these relations (C need not be the smallest).
 *   nldpc_tb_lifting_size (host only, a helper: the plan takes whatever graph the caller has): Bp = B'.  Kb of §5.2.2
 *      (bg 1: 22; bg 2: 10 / 9 / 8 / 6 for B' > 640 / > 560 / > 192 / else) and Zc, the smallest Z = a * 2^j <= 384,
 *      a in {2, 3, 5, 7, 9, 11, 13, 15} (Table 5.3.2-1), with Kb * Z >= K', K' = ceil(B'' / C) for the base graph's own
 *      Kcb (8448 / 3840).  NLDPC_EINVAL: bg not 1 / 2, Bp < 1 or >= 2^31, a NULL pointer, no size large enough.
 *   nldpc_tb_er (host only): with G' = G / (NL Qm), blocks r < C_lo = C - (G' mod C) get E_lo = NL Qm floor(G' / C), the
 *      others E_hi = NL Qm ceil(G' / C) (E_hi == E_lo when C divides G').  NLDPC_EINVAL unless NL, Qm, C >= 1,
 *      1 <= G < 2^31, NL Qm divides G and E_lo >= 1.
 *   nldpc_tb_crc_ref (host only, no device): one TB as its C host rows blocks[r * stride ..], uint8 (any non-zero byte is
 *      1), stride >= K'.  cb_ok[r] (nullable, [C]) = 1 when the first K' bits of row r pass CRC24B (C == 1: when the TB
 *      CRC passes).  *tb_rem (nullable) = what nldpc_crc_ref(tb_crc) gives as the parity of the reassembled B' bits
 *      (TB(x) x^L_tb mod g), 0 = the TB passes: the remainder of each part under the TB polynomial, combined by
 *      acc = acc * x^{K' - L} xor R(part r) over r = 0 .. C-1 with the functions nldpc_tb_check runs.
 *   nldpc_tb_segment: tb uint8 [Btb][B'] (the TB bits with the TB CRC, what nldpc_crc_attach writes with W = B'; any
 *      non-zero byte is 1) -> info uint8 [C * Btb][W], written in full: row r * Btb + t = tb[t][r (K'-L) .. (r+1)(K'-L))
 *      as 0 / 1, the CRC24B parity of those bits, p_0 first (nothing when C == 1), F zeros.
 *   nldpc_tb_concat: elem_bytes 1 (bits) or 4 (fp32 / any 4-byte element, copied as it is).  f_lo [C_lo * Btb][E_lo]
 *      and f_hi [(C - C_lo) * Btb][E_hi], block-major (f_lo NULL allowed when C_lo == 0 -- never produced by
 *      nldpc_tb_er --, f_hi when C_lo == C) -> g [Btb][G], G = C_lo E_lo + (C - C_lo) E_hi: block r of TB t sits at
 *      g[t][sum_{j<r} E_j ..].  nldpc_tb_deconcat is the inverse, g -> f_lo, f_hi.  Elements are copied unchanged.
 *      NLDPC_EINVAL: elem_bytes not 1 / 4, Btb < 1, C < 1, C_lo outside [0, C], E_lo or E_hi < 1, G or C * Btb >= 2^31,
 *      a NULL pointer that is needed, a pointer off a 4-byte boundary when elem_bytes == 4.
 *   nldpc_tb_check: exactly one of llr (fp32 [C * Btb][stride], hard decision by `convention` as nldpc_crc_check) and
 *      bits (uint8 [C * Btb][stride], non-zero is 1); stride >= K' in elements: decoder posteriors [C * Btb][N*Z] go in as
 *      they are.  The first K' positions of every row are read once.  cb_ok uint8 [C * Btb] (nullable): 1 when the
 *      block's CRC24B passes (C == 1: the TB verdict).  tb_ok uint8 [Btb] (nullable): 1 when the TB CRC over the
 *      reassembled B' bits passes; it is combined from the per-part remainders, no TB is materialised for it.  tb_out
 *      uint8 [Btb][B'] (nullable): the reassembled bits as 0 / 1 (desegmentation).  ref_tb uint8 [Btb][B'] (nullable,
 *      non-zero is 1): the true TB bits.  counts (nullable) device int64[4], +=: [0] TBs whose TB CRC fails; [1] TBs that
 *      pass although their B' bits differ from ref_tb (undetected errors); [2] TBs whose B' bits differ from ref_tb;
 *      [3] code blocks whose CRC fails (C == 1: equal to [0]); [1] and [2] get nothing without ref_tb.  The all-zero TB
 *      passes, and a TB in which a code block was replaced by another valid code block passes every code-block CRC and
 *      fails only the TB CRC.  work: device scratch of at least the bytes nldpc_tb_workspace answers (4 per code
 *      block), 4-byte aligned; the first kernel leaves each part's TB remainder there (left-aligned, its error and
 *      verdict flags in the two lowest bits), a second launch of one thread per TB combines them in ascending r.
 *      NLDPC_EINVAL: a plan that breaks the relations above, Btb < 1, C * Btb >= 2^31, both or neither of llr and bits,
 *      stride < K', convention not 0 / 1, every output NULL, work NULL or too small or off a 4-byte boundary, llr off a
 *      4-byte or counts off an 8-byte boundary.
 *   All launches are stream-ordered on the current device, synchronise and allocate nothing, write nothing outside
 *      their outputs (and work) and need no graph handle. */
typedef struct nldpc_tb {
    int64_t A;       /* payload bits */
    int32_t tb_crc;  /* enum nldpc_crc of the TB CRC */
    int64_t W;       /* bits of a code-block row (K*Z) */
    int32_t C;       /* code blocks */
    int32_t L;       /* code-block CRC bits: 24, or 0 when C == 1 */
    int64_t Kp;      /* K': part + L */
    int64_t F;       /* filler bits W - K' */
} nldpc_tb;
int nldpc_tb_plan(int64_t A, int32_t tb_crc, int64_t W, int64_t kcb, nldpc_tb* plan);
int nldpc_tb_lifting_size(int32_t bg, int64_t Bp, int32_t* Kb, int32_t* Zc);
int nldpc_tb_er(int64_t G, int32_t NL, int32_t Qm, int32_t C, int64_t* E_lo, int64_t* E_hi, int32_t* C_lo);
int nldpc_tb_crc_ref(const nldpc_tb* plan, const uint8_t* blocks, int64_t stride, uint8_t* cb_ok,
                     uint32_t* tb_rem);
int nldpc_tb_workspace(const nldpc_tb* plan, int64_t Btb, size_t* bytes);
int nldpc_tb_segment(const nldpc_tb* plan, const uint8_t* tb, int64_t Btb, uint8_t* info, void* stream);
int nldpc_tb_concat(int32_t elem_bytes, const void* f_lo, const void* f_hi, int64_t Btb, int32_t C, int32_t C_lo,
                    int64_t E_lo, int64_t E_hi, void* g, void* stream);
int nldpc_tb_deconcat(int32_t elem_bytes, const void* g, int64_t Btb, int32_t C, int32_t C_lo, int64_t E_lo,
                      int64_t E_hi, void* f_lo, void* f_hi, void* stream);
int nldpc_tb_check(const nldpc_tb* plan, const float* llr, const uint8_t* bits, int64_t Btb, int64_t stride,
                   int32_t convention, const uint8_t* ref_tb, uint8_t* cb_ok, uint8_t* tb_ok, uint8_t* tb_out,
                   int64_t* counts, void* work, size_t work_bytes, void* stream);

/* ---- Gold-sequence scrambling (additive to ABI 4): bit scrambling with the length-31 Gold sequence of 3GPP TS 38.211
 *      §5.2.1 (PUSCH §6.3.1.1, PDSCH §7.3.1.1), the step between code-block concatenation (nldpc_tb_concat) and the
 *      mapper (nldpc_qam_*), and its inverse on the LLRs in front of nldpc_tb_deconcat / nldpc_rate_recover.  The
 *      reference has no counterpart.  The arithmetic is the inline functions of csrc/nldpc_gold.h on host and device.
 *   Sequence: x1(n+31) = x1(n+3) ^ x1(n), x1(0) = 1, x1(1..30) = 0; x2(n+31) = x2(n+3) ^ x2(n+2) ^ x2(n+1) ^ x2(n),
 *      x2(i) = (c_init >> i) & 1 for i < 31; c(n) = x1(n + 1600) ^ x2(n + 1600); 0 <= c_init < 2^31.
 *   Packing: a sequence of E bits is Wc = ceil(E / 32) words of 32 bits, bit n in bit n & 31 of word n >> 5 (least
 *      significant first); the bits at and beyond E in the last word are 0.  A table is seq[n_seq][Wc]; row b of a batch
 *      uses sequence (b_offset + b) mod n_seq: n_seq = 1 is one sequence for every row, and a table with one sequence
 *      per transport block shards as the Philox streams do.
 *   nldpc_gold_cinit (host only): *c_init = rnti * 2^15 + q * 2^14 + n_id.  NLDPC_EINVAL unless 0 <= rnti < 2^16, q in
 *      {0, 1}, 0 <= n_id < 1024, c_init non-NULL.
 *   nldpc_gold_ref (host only, no device): c[i] = c(n0 + i), i < n, as bytes 0 / 1.  It jumps to n0 (x^(n0 + 1600) mod
 *      the register's polynomial by squaring: with r = x^n mod p, x(n + j) = XOR over the k with r_k = 1 of x(k + j), so
 *      the state at n follows from r and the register's first 61 bits), then steps 32 bits at a time; it does not run
 *      from 0.  NLDPC_EINVAL: c_init >= 2^31, n0 < 0, n < 1, n0 + n > 2^31, c NULL.
 *   nldpc_gold_sequence: c_init device int32 [n_seq] -> seq device [n_seq][Wc], written in full.  Of each c_init entry
 *      the low 31 bits are used (a negative entry cannot be reported by a launch that does not synchronise).  One
 *      kernel; a thread jumps to its run of words as nldpc_gold_ref does, so the words do not depend on the run length
 *      or the grid.  NLDPC_EINVAL: n_seq < 1, E < 1, E >= 2^31, a NULL pointer, a pointer off a 4-byte boundary;
 *      NLDPC_EUNSUPPORTED: n_seq * Wc >= 2^31.
 *   nldpc_scramble: out[b][i] = (f[b][i] != 0) ^ c_s(i) as 0 / 1, s = (b_offset + b) mod n_seq; f, out uint8 [B][E], any
 *      start address; f NULL = the all-zero word (out is the sequence unpacked); out == f (in place) is allowed, any
 *      other overlap is the caller's error.
 *   nldpc_descramble_llr: out[b][i] = llr[b][i] with its sign bit XORed with c_s(i), an integer operation on the bit
 *      pattern: -0, infinities and NaN payloads pass with only the sign changed, and applying it twice is the identity
 *      bit for bit.  llr, out fp32 [B][E]; in place is allowed.
 *   nldpc_qam_channel_llr_scrambled: nldpc_qam_channel_llr with f ^ c going into the mapper and the sign flip coming
 *      out, in one kernel: llr is bit for bit nldpc_descramble_llr(nldpc_qam_channel_llr(nldpc_scramble(f))) -- counters,
 *      tag and Box-Muller unchanged, a symbol's noise is the one nldpc_qam_channel_llr draws for it --, and sym_out
 *      (nullable) receives the noisy symbols of the scrambled bits (what is on the air).  f NULL = the all-zero word,
 *      which then visits every constellation point while the decoder still sees "bit 0 sent" everywhere.  The argument
 *      rules are those of nldpc_qam_channel_llr, and seq non-NULL and 4-byte aligned, n_seq >= 1.
 *   For the three table users: NLDPC_EINVAL: seq NULL or off a 4-byte boundary, n_seq < 1, B < 1, E < 1, E >= 2^31,
 *      b_offset < 0, a NULL required pointer, a float pointer off a 4-byte boundary; NLDPC_EUNSUPPORTED: B or b_offset
 *      >= 2^31, n_seq * Wc >= 2^31.  seq must have Wc = ceil(E / 32) words per row (not checkable from a pointer).
 *   All launches are stream-ordered on the current device, synchronise and allocate nothing and write nothing outside
 *      seq / out / llr / sym_out. */
int nldpc_gold_cinit(int32_t rnti, int32_t q, int32_t n_id, uint32_t* c_init);
int nldpc_gold_ref(uint32_t c_init, int64_t n0, int64_t n, uint8_t* c);
int nldpc_gold_sequence(const int32_t* c_init, int64_t n_seq, int64_t E, uint32_t* seq, void* stream);
int nldpc_scramble(const uint8_t* f, const uint32_t* seq, int64_t n_seq, int64_t B, int64_t E, int64_t b_offset,
                   uint8_t* out, void* stream);
int nldpc_descramble_llr(const float* llr, const uint32_t* seq, int64_t n_seq, int64_t B, int64_t E, int64_t b_offset,
                         float* out, void* stream);
int nldpc_qam_channel_llr_scrambled(int32_t qm, int32_t method, const uint8_t* f, int64_t B, int64_t E, float sigma,
                                    uint64_t seed, int64_t b_offset, const uint32_t* seq, int64_t n_seq, float* llr,
                                    float* sym_out, void* stream);

/* ---- Flat block fading with perfect CSI for the QAM channel (additive to ABI 4): nldpc_qam_channel_llr with a real gain
 *      g >= 0 between the mapper and the noise -- the channel's magnitude after the receiver's exact phase de-rotation,
 *      under which circular noise stays circular -- and a demapper that knows g.  The reference has no counterpart.  The
 *      arithmetic is the inline functions of csrc/nldpc_fading.h (and nldpc_qam.h) on host and device.
 *   Model, per real dimension: r = (float)((double)fl32(g * level) + (double)sigma * n), n exactly the normal
 *      nldpc_qam_channel_llr draws for that symbol (same counter, tag "QAM1", same Box-Muller).  The demapper of the QAM
 *      section runs unchanged on the levels fl32(g * l), one fp32 multiply per level, shared by I and Q of a symbol, with
 *      the same w = (float)(1 / (2 sigma^2)).  g = 1 reproduces nldpc_qam_channel_llr / nldpc_qam_demap bit for bit;
 *      g = 0 gives +-0 for every LLR of the symbol, both methods.  E[g^2] = 1 for drawn gains, so sigma means what it
 *      means for AWGN.
 *   Fading blocks: gains are constant over L >= 1 consecutive symbols of a row (the coherence length); n_blk =
 *      ceil(S / L), the last block of a row may be short, blocks never span rows; L = 1 is fast fading, L >= S one gain
 *      per row.  Symbol j of row b has the gain of global block Gf = (b_offset + b) * n_blk + j div L.  A gain table is
 *      fp32 [B][n_blk], contiguous.
 *   Drawn gains (Rician factor K >= 0 as a double; K = 0 is Rayleigh and no special case): Philox-4x32-10 with key
 *      (lo32(seed), hi32(seed)) at counter (lo32(Gf >> 1), hi32(Gf >> 1), 0x46414431 "FAD1", 0); words (x, y) serve an
 *      even Gf, (z, w) an odd one.  With the block's words (r0, r1), u = (word + 1) / 2^32, all in double without FMA:
 *      rad = sqrt(-2 log u(r0)), th = 6.283185307179586 u(r1), a = rad cos(th), b = rad sin(th),
 *      mu = sqrt(K / (K + 1)), s = sqrt(1 / (2 (K + 1))), g = (float)sqrt((mu + s a)^2 + (s b)^2), rounded to fp32
 *      once.  b_offset moves the gain stream as it moves the noise stream: a shard draws the unsharded batch's gains.
 *   Given gains must be finite and >= 0; nothing checks that (it would take a pass over the table), and a negative,
 *      infinite or NaN gain gives LLRs of no meaning, never a write outside the outputs.
 *   nldpc_fading_gain_ref (host only, no device): g[i] from the word pair (words[2i], words[2i+1]), i < n.
 *   nldpc_qam_demap_csi_ref (host only, no device): sym host [B][S][2], gain host [B][n_blk] -> llr host [B][S*qm].
 *   nldpc_fading_gains: the drawn table g [B][n_blk] of the rows b_offset .. b_offset + B - 1, written in full.
 *   nldpc_qam_demap_csi: sym [B][S][2] and gain [B][n_blk] -> llr [B][S*qm].
 *   nldpc_qam_fading_channel_llr: bits -> (scramble) -> levels -> gain -> noise -> CSI demap -> (descramble) in one
 *      kernel.  f NULL = the all-zero word.  gain_in NULL draws the gains (K, seed), else it is the table and K is only
 *      checked.  seq NULL = no scrambling, else the table of nldpc_gold_sequence for rows of E bits, n_seq sequences,
 *      used as nldpc_qam_channel_llr_scrambled uses it (n_seq is ignored without seq).  llr is bit for bit
 *      nldpc_qam_demap_csi of the symbols and gains it returns (and of those descrambled with seq): sym_out (nullable)
 *      receives the r, [B][S][2]; gain_out (nullable) the gains, [B][n_blk], written in full, bit for bit
 *      nldpc_fading_gains when drawn, a copy of gain_in when given.  gain_out must not overlap gain_in.
 *   NLDPC_EINVAL: the rules of nldpc_qam_demap (the two demappers) and nldpc_qam_channel_llr (the fused channel), and
 *      L < 1, K negative, infinite or NaN, B * n_blk >= 2^31, n_blk < 1 or >= 2^31 (nldpc_fading_gains), a NULL required
 *      pointer, a float pointer or seq off a 4-byte boundary, n_seq < 1 with seq.  NLDPC_EUNSUPPORTED: B or b_offset
 *      >= 2^31 (device calls), n_seq * Wc >= 2^31.
 *   The three launches are stream-ordered on the current device, synchronise and allocate nothing and write nothing
 *      outside g / llr / sym_out / gain_out. */
int nldpc_fading_gain_ref(double K, const uint32_t* words, int64_t n, float* g);
int nldpc_qam_demap_csi_ref(int32_t qm, int32_t method, float sigma, const float* sym, const float* gain, int64_t B,
                            int64_t S, int64_t L, float* llr);
int nldpc_fading_gains(double K, uint64_t seed, int64_t B, int64_t n_blk, int64_t b_offset, float* g, void* stream);
int nldpc_qam_demap_csi(int32_t qm, int32_t method, float sigma, const float* sym, const float* gain, int64_t B,
                        int64_t S, int64_t L, float* llr, void* stream);
int nldpc_qam_fading_channel_llr(int32_t qm, int32_t method, const uint8_t* f, int64_t B, int64_t E, float sigma,
                                 uint64_t seed, int64_t b_offset, int64_t L, double K, const float* gain_in,
                                 const uint32_t* seq, int64_t n_seq, float* llr, float* sym_out, float* gain_out,
                                 void* stream);

/* ---- MIMO spatial multiplexing with LMMSE soft detection (additive to ABI 4): one codeword over nt layers (3GPP TS 38.211
 *      §6.3.1.3 / §7.3.1.3, identity precoding), an nr x nt flat block-fading channel and a linear MMSE detector in front
 *      of the demapper of the QAM section.  The reference has no counterpart.  The arithmetic is the inline functions of
 *      csrc/nldpc_mimo.h (and nldpc_qam.h, nldpc_fading.h) on host and device.
 *   Geometry: nt in {1, 2, 4} layers, nr in {1, 2, 4} receive antennas, nr >= nt (six pairs).  A row of E bits is
 *      S = E / qm symbols d(0 .. S-1), S a multiple of nt, and R = S / nt resource elements (REs): RE i carries
 *      x_k(i) = d(nt i + k) on layer k.  In memory the layer mapping is the identity: an RE is nt consecutive symbols and
 *      nt qm consecutive bits / LLRs.  Received samples are fp32 [B][R][nr][2] (re, im).
 *   Fading blocks: the rules of the fading section counted in REs: H is constant over L >= 1 consecutive REs of a row,
 *      n_blk = ceil(R / L) (1 when L >= R), blocks never span rows, RE i of row b has the matrix of global block
 *      Gf = (b_offset + b) * n_blk + i div L.  A channel table is fp32 [B][n_blk][nr][nt][2], contiguous: h(r, t) is the
 *      path from layer t to antenna r.
 *   Complex arithmetic, everywhere below: (a + ib)(c + id) = (fl(fl(a c) - fl(b d)), fl(fl(a d) + fl(b c))), four rounded
 *      products, one rounded difference and one rounded sum, no FMA; with a conjugated factor the signs move, the count
 *      does not: conj(a + ib)(c + id) = (fl(fl(a c) + fl(b d)), fl(fl(a d) - fl(b c))) and (a + ib) conj(c + id) =
 *      (fl(fl(a c) + fl(b d)), fl(fl(b c) - fl(a d))).  A sum over an index starts from its first term and adds the others in ascending order, real and
 *      imaginary parts separately.  |z|^2 = fl(fl(re re) + fl(im im)).
 *   Channel, fp32: s(r) = sum_t h(r, t) x_t, t ascending; each real component of y(r) is
 *      (float)((double)s + (double)sigma * n), sigma the standard deviation per real dimension and receive antenna.
 *   Noise: Philox-4x32-10 with key (lo32(seed), hi32(seed)) at counter (lo32(Gre), hi32(Gre), 0x4D494E31 "MIN1", q),
 *      Gre = (b_offset + b) * R + i the global RE index, q < ceil(nr / 2) the antenna pair.  Words (x, y) give antenna 2q:
 *      u = (word + 1) / 2^32, rad = sqrt(-2 log u(x)), th = 6.283185307179586 u(y), (n_re, n_im) = (rad cos th,
 *      rad sin th), in double; words (z, w) give antenna 2q + 1 the same way (unused for nr = 1).  A shard draws the
 *      noise of the unsharded batch.
 *   Drawn channels: Rayleigh, i.i.d. CN(0, 1 / nt) entries, so the mean received energy per antenna and RE is 1 and
 *      sigma keeps its per-receive-antenna meaning.  Entry e = r * nt + t of global block Gf: counter (lo32(Gf), hi32(Gf),
 *      0x4D494831 "MIH1", e >> 1), words (x, y) for an even e, (z, w) for an odd one; with the entry's words (r0, r1),
 *      rad and th as above, s = sqrt(1 / (2 nt)): re = (float)(s * (rad * cos th)), im = (float)(s * (rad * sin th)),
 *      everything in double, each component rounded to fp32 once.  Rician entries, spatial correlation and precoding
 *      are not drawn; a given table covers them.
 *   Detector, per fading block, in double from the fp32 table (sigma the fp32 the ABI takes): n0 = 2 (sigma sigma),
 *      q = 1 / n0.  With G = H^H H + n0 I the quantities wanted are W = G^-1 H^H (nt x nr), e_k = n0 [G^-1]_kk (the MMSE
 *      of layer k), mu_k = 1 - e_k.  They are computed from the Cholesky factor of Gn = G / n0 = I + (H^H H) q, which
 *      makes e_k = [Gn^-1]_kk a sum of squares (positive, no cancellation, no final product) and gives e_k = 1, mu_k = 0
 *      exactly for a zero channel:
 *        A(j,k) = sum_r conj(h(r,j)) h(r,k) for j >= k, r ascending; the diagonal is real, sum_r |h(r,k)|^2;
 *        Gn(j,k) = A(j,k) q (each component) for j > k, Gn(k,k) = A(k,k) q + 1;
 *        Gn = C C^H, C lower triangular, by columns j = 0 .. nt-1: d = Gn(j,j) - |C(j,0)|^2 - .. - |C(j,j-1)|^2 (subtracted
 *          one by one, k ascending), C(j,j) = sqrt(d), c_j = 1 / C(j,j); for i > j: z = Gn(i,j) - C(i,0) conj(C(j,0)) - ..
 *          - C(i,j-1) conj(C(j,j-1)) (one by one, k ascending, each component), C(i,j) = z c_j (each component);
 *        M = C^-1: M(j,j) = c_j; for i > j: M(i,j) = -(sum_{k=j}^{i-1} C(i,k) M(k,j)) c_i (each component);
 *        e_k = M(k,k)^2 + |M(k+1,k)|^2 + .. + |M(nt-1,k)|^2 (added one by one), mu_k = 1 - e_k, p = mu_k e_k,
 *          w_k = 1 / p when p is positive and finite, else 0;
 *        T(i,r) = sum_{k=0}^{i} M(i,k) conj(h(r,k));  W(k,r) = (sum_{i=k}^{nt-1} conj(M(i,k)) T(i,r)) q (each component).
 *      W [nt][nr][2], mu [nt] and w [nt] are each rounded to fp32 once.  Only + - * / sqrt occur, in this order, so host,
 *      device and a scalar float64 restatement agree bit for bit.
 *   Equalise and demap, per RE, fp32: x^_k = sum_r W(k,r) y(r), r ascending; layer k is demapped by the demapper of the
 *      QAM section, unchanged, on the levels fl32(mu_k * l) with the weight w_k in place of 1 / (2 sigma^2).  This is the
 *      biased-LMMSE Gaussian approximation: x^_k = mu_k x_k + (interference + noise) of variance mu_k e_k, i.e.
 *      mu_k e_k / 2 per real dimension.  For nt = nr = 1 and a real h = g it is analytically the CSI demapper of the
 *      fading section: (x^ - mu l)^2 w = (y - g l)^2 / (2 sigma^2).  A zero channel gives +-0 for every LLR, both
 *      methods, never NaN.  The LLRs of layers that interfere are not independent given the bits, and the residual
 *      interference is not Gaussian; the decoder is handed them as if they were.
 *   nldpc_mimo_entry_ref (host only, no device): the entry (h[2i], h[2i+1]) from the word pair (words[2i], words[2i+1]),
 *      i < n, with s of nt.  NLDPC_EINVAL: nt not 1, 2 or 4, a NULL pointer, n < 1.
 *   nldpc_mimo_filter_ref (host only, no device): h host [n][nr][nt][2] -> W [n][nt][nr][2], mu [n][nt], w [n][nt].
 *   nldpc_mimo_detect_ref (host only, no device): y host [B][R][nr][2], h host [B][n_blk][nr][nt][2] -> llr host
 *      [B][R * nt * qm].
 *   nldpc_mimo_channels: the drawn table h [B][n_blk][nr][nt][2] of the rows b_offset .. b_offset + B - 1, in full.
 *   nldpc_mimo_filter: h [B][n_blk][nr][nt][2] -> W [B][n_blk][nt][nr][2], mu [B][n_blk][nt], w [B][n_blk][nt].
 *   nldpc_mimo_detect: y [B][R][nr][2] and h [B][n_blk][nr][nt][2] -> llr [B][R * nt * qm].
 *   nldpc_mimo_channel_llr: bits -> (scramble) -> map -> H x -> noise -> filter -> equalise -> demap -> (descramble) in
 *      one kernel.  f NULL = the all-zero word.  h_in NULL draws the channels (seed), else it is the table.  seq NULL = no
 *      scrambling, else the table of nldpc_gold_sequence for rows of E bits, n_seq sequences, used as
 *      nldpc_qam_channel_llr_scrambled uses it (n_seq is ignored without seq).  llr is bit for bit nldpc_mimo_detect of
 *      the samples and channels it returns (and of those descrambled with seq): sym_out (nullable) receives y,
 *      [B][R][nr][2]; h_out (nullable) the channels, written in full, bit for bit nldpc_mimo_channels when drawn, a copy
 *      of h_in when given.  h_out must not overlap h_in.
 *   NLDPC_EINVAL: qm not 2, 4, 6, 8; method not 0 / 1; sigma not positive; (nt, nr) not one of the six pairs; B, R, E or
 *      n_blk < 1; b_offset < 0; L < 1; E >= 2^31 or not a multiple of qm; E / qm not a multiple of nt; R * nt * qm >= 2^31;
 *      B * n_blk >= 2^31; a NULL required pointer; a float pointer or seq off a 4-byte boundary; n_seq < 1 with seq; h_out
 *      overlapping h_in.  NLDPC_EUNSUPPORTED: B or b_offset >= 2^31 (device calls), n_seq * Wc >= 2^31.
 *   The four launches are stream-ordered on the current device, synchronise and allocate nothing and write nothing
 *      outside h / W / mu / w / llr / sym_out / h_out. */
int nldpc_mimo_entry_ref(int32_t nt, const uint32_t* words, int64_t n, float* h);
int nldpc_mimo_filter_ref(int32_t nt, int32_t nr, float sigma, const float* h, int64_t n, float* W, float* mu, float* w);
int nldpc_mimo_detect_ref(int32_t qm, int32_t method, int32_t nt, int32_t nr, float sigma, const float* y, const float* h,
                          int64_t B, int64_t R, int64_t L, float* llr);
int nldpc_mimo_channels(int32_t nt, int32_t nr, uint64_t seed, int64_t B, int64_t n_blk, int64_t b_offset, float* h,
                        void* stream);
int nldpc_mimo_filter(int32_t nt, int32_t nr, float sigma, const float* h, int64_t B, int64_t n_blk, float* W, float* mu,
                      float* w, void* stream);
int nldpc_mimo_detect(int32_t qm, int32_t method, int32_t nt, int32_t nr, float sigma, const float* y, const float* h,
                      int64_t B, int64_t R, int64_t L, float* llr, void* stream);
int nldpc_mimo_channel_llr(int32_t qm, int32_t method, int32_t nt, int32_t nr, const uint8_t* f, int64_t B, int64_t E,
                           float sigma, uint64_t seed, int64_t b_offset, int64_t L, const float* h_in,
                           const uint32_t* seq, int64_t n_seq, float* llr, float* sym_out, float* h_out, void* stream);

/* ---- Exact max-log ML (joint) soft detection for the MIMO section (additive to ABI 4).  Geometry, fading blocks, complex
 *      arithmetic, noise and channel streams are those of the MIMO section; only the detector differs.  The reference
 *      has no counterpart.  The arithmetic is the inline functions of csrc/nldpc_mimo_ml.h (on nldpc_mimo.h and
 *      nldpc_qam.h) on host and device.
 *   Definition, per RE, with n0 = 2 sigma^2:  LLR(b) = (min_{x: b = 0} d(x) - min_{x: b = 1} d(x)) / n0,
 *      d(x) = sum_r |y(r) - sum_t h(r,t) x_t|^2, x over all 2^(qm nt) symbol vectors; sign and bit order as
 *      nldpc_mimo_detect (> 0 means bit 1, layer k's qm bits at k qm).  Max-log only: an exact log-MAP needs every
 *      candidate.  No Gaussian approximation is involved: these are the max-log LLRs of y.
 *   Reduction (exact): a pass enumerates the symbols of the layers in a set En and slices the remaining layer s, whose
 *      best symbol given the others is the constellation point nearest to z = h_s^H r / |h_s|^2, r = y - sum_{t in En}
 *      h_t x_t, Re and Im independently.  Since the sliced layer is unconstrained, the pass yields the exact minima for
 *      every bit of every layer of En.  nt = 1: one pass, En = {0}, nothing sliced (2^qm candidates).  nt >= 2: pass A,
 *      En = {0 .. nt-2}, s = nt-1, gives the layers 0 .. nt-2; pass B, En = {1 .. nt-1}, s = 0, gives layer nt-1
 *      (2 * 2^(qm (nt-1)) candidates, no QR).
 *   Supported: nt = 1 and 2 with qm = 2, 4, 6, 8; nt = 4 with qm = 2, 4.  nt = 4 with qm = 6 or 8 (2 * 64^3 and
 *      2 * 256^3 candidates per RE) needs a tree search: NLDPC_EUNSUPPORTED.  nr follows the six (nt, nr) pairs.
 *   Arithmetic, fp32, one rounding per operation, no FMA, complex products and ascending sums as the MIMO section
 *      states them; A = the level scale of the QAM section, l(c) the level of label c:
 *        sliced layer, per pass:  g = sum_r |h(r,s)|^2, r ascending;  q = fl(1 / g);  inv = q when g > 0 and q is finite,
 *          else 0 (so |h_s|^2 = 0 gives z = 0).
 *        candidate (labels (ci_t, cq_t) of the layers t of En):  res(r) = y(r), then for t in En ascending
 *          res(r) = res(r) - h(r,t) (l(ci_t) + i l(cq_t)), each component: Re res - fl(fl(a li) - fl(b lq)),
 *          Im res - fl(fl(a lq) + fl(b li)) with h(r,t) = a + i b.
 *        slice:  num = sum_r conj(h(r,s)) res(r), r ascending;  z = (fl(Re num * inv), fl(Im num * inv));  per component
 *          u = fl(fl(z K) + 2^(h-1)) with K = 1 / (2 A) = 0.70710678118654752, 1.5811388300841897, 3.2403703492039302,
 *          6.5192024052026492 for qm = 2, 4, 6, 8 (evaluated in double, rounded to fp32 once);  j = floor(u) clamped
 *          to 0 .. 2^h - 1 by (j > 0 ? j : 0) then (j < 2^h - 1 ? j : 2^h - 1), so a NaN gives 0;  x^ component =
 *          fl((2 j - (2^h - 1)) A), which is the level of amplitude 2 j - (2^h - 1) as the QAM section computes it.
 *          A near-tie can pick the neighbouring point; its metric exceeds the minimum over x_s by at most
 *          4 A |h_s|^2 times the error of z per dimension.
 *        metric:  e(r) = res(r) - h(r,s) x^ (each component as above; nt = 1: e = res);  d = sum_r |e(r)|^2, r ascending:
 *          always the metric of a true candidate, whichever point the slice picked.
 *        minima:  per layer t of En and label c, minI_t[c] = min of d over the candidates with ci_t = c, minQ_t[c]
 *          likewise with cq_t = c; a minimum starts from +inf and takes d when d < minimum (a NaN never enters).  A
 *          minimum is exact, so the order in which candidates are visited does not show.
 *        LLR of bit k of the I dimension of layer t (bit 2k of the symbol; Q: bit 2k+1 from minQ_t):
 *          fl(fl(min_{c: c_k = 0} minI_t[c] - min_{c: c_k = 1} minI_t[c]) w),  w = (float)(1 / (2 sigma sigma)) evaluated
 *          in double from the fp32 sigma: the finish of the QAM section's max-log demapper on minI_t in place of d.
 *      A zero channel gives every candidate the metric sum_r |y(r)|^2 and hence +0 for every LLR.  Host, device and
 *      a float32 restatement agree bit for bit.
 *   nldpc_mimo_detect_ml_ref (host only, no device): arguments as nldpc_mimo_detect_ref without method.
 *   nldpc_mimo_detect_ml: y [B][R][nr][2] and h [B][n_blk][nr][nt][2] -> llr [B][R * nt * qm]; arguments as
 *      nldpc_mimo_detect without method.
 *   nldpc_mimo_channel_llr_ml: bits -> (scramble) -> map -> H x -> noise -> ML detect -> (descramble) in one kernel;
 *      arguments as nldpc_mimo_channel_llr without method.  The noise and channel streams are those of
 *      nldpc_mimo_channel_llr, so sym_out and h_out are bit for bit what that function returns for the same arguments,
 *      and llr is bit for bit nldpc_mimo_detect_ml of them (descrambled with seq).
 *   NLDPC_EINVAL: the rules of the MIMO section (without method).  NLDPC_EUNSUPPORTED: nt = 4 with qm >= 6; and as in
 *      the MIMO section.  The launches are stream-ordered on the current device, synchronise and allocate nothing and
 *      write nothing outside llr / sym_out / h_out. */
int nldpc_mimo_detect_ml_ref(int32_t qm, int32_t nt, int32_t nr, float sigma, const float* y, const float* h, int64_t B,
                             int64_t R, int64_t L, float* llr);
int nldpc_mimo_detect_ml(int32_t qm, int32_t nt, int32_t nr, float sigma, const float* y, const float* h, int64_t B,
                         int64_t R, int64_t L, float* llr, void* stream);
int nldpc_mimo_channel_llr_ml(int32_t qm, int32_t nt, int32_t nr, const uint8_t* f, int64_t B, int64_t E, float sigma,
                              uint64_t seed, int64_t b_offset, int64_t L, const float* h_in, const uint32_t* seq,
                              int64_t n_seq, float* llr, float* sym_out, float* h_out, void* stream);

/* ---- benchmark instrumentation: per-kernel HIP-event timing of nldpc_forward / nldpc_backward
 *   launches.  nldpc_profile_begin arms a recorder for up to `capacity` launches (not thread-safe);
 *   nldpc_profile_end synchronises on the recorded events and returns summed milliseconds and
 *   launch counts per kernel kind (0 = variable-node, 1 = check-node, 2 = final posterior,
 *   3 = fused decoder, 4 = variable-node backward, 5 = check-node backward). */
int nldpc_profile_begin(int32_t capacity);
int nldpc_profile_end(int32_t nkinds, float* ms, int32_t* count);

/* ---- benchmark instrumentation: measured HBM ceilings (SURVEY §8(d) D4 "report the measured
 *   stream-copy ceiling too").  One launch over n floats (n % 4 == 0; 16 B per lane unless stated):
 *   kind 0 = copy src -> dst, 1 = write-only fill of dst, 2 = read-only pass over src (dst receives
 *   one float4 per workgroup, 2048 workgroups), 3 = read-only with 4 B per lane (dst receives one float4 per
 *   workgroup, 8192 workgroups).  r6: kinds 0-2 keep 8 float4 loads in flight per lane, non-temporal. */
int nldpc_hbm_probe(int32_t kind, float* dst, const float* src, int64_t n, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* NLDPC_H */
