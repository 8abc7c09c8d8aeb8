/* omk.h -- C ABI of libomnimamba_hip.so: the MI355X (gfx950) kernels behind OmniMamba's Mamba-2 hot path.
 *
 * The reference has NO native boundary of its own: every hot op is a Python import from the third-party
 * packages mamba_ssm==2.2.2 / causal-conv1d==1.4.0 (/root/reference/requirements.txt:12-13), whose pybind11
 * Torch extensions take at::Tensor.  This header is the drop-in boundary this repo defines instead: plain
 * pointers, sizes and element strides, no torch types, no exceptions.  Each entry point names the reference
 * call site it serves (paths relative to /root/reference) and the upstream Python symbol it stands behind.
 *
 * Conventions
 *   - every function returns 0 (OMK_OK) or a negative omk_status; omk_last_error() gives thread-local text.
 *   - all launches are asynchronous on the hipStream_t passed as `stream` (0 = default stream); the library
 *     never allocates or frees device memory, never synchronises, keeps no mutable global state -> safe
 *     under hipGraph capture and one-process-per-GPU data parallelism.
 *   - tensors are described by OmkTensor (device pointer + dtype + shape + ELEMENT strides); data == NULL
 *     marks an absent optional tensor.  Scratch is caller-owned: ask omk_*_workspace_bytes first.
 *   - all arithmetic is fp32 internally; dtype says how a tensor is stored.
 */
#ifndef OMK_H
#define OMK_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OMK_ABI_VERSION 17
#define OMK_MAX_DIMS 5

typedef enum { OMK_OK = 0, OMK_EINVAL = -1, OMK_EARCH = -2, OMK_ELAUNCH = -3, OMK_EUNSUPPORTED = -4 } omk_status;
typedef enum { OMK_F32 = 0, OMK_BF16 = 1, OMK_F16 = 2, OMK_U8 = 3 /* masks only */, OMK_I32 = 4 /* ABI 8: slot indices; ABI 10 / 13: per-row lengths */,
               OMK_F8E4M3 = 5 /* ABI 11: OCP e4m3fn (bias 7, max 448, 0x7F / 0xFF NaN, no infinities; NOT the fnuz form) -- the weight of
                                 omk_norm_linear only, together with OmkNormLinear.weight_scale */ } omk_dtype;
typedef void* omk_stream; /* hipStream_t */

typedef struct {
  void* data;
  int32_t dtype; /* omk_dtype */
  int32_t ndim;
  int64_t shape[OMK_MAX_DIMS];
  int64_t stride[OMK_MAX_DIMS]; /* elements */
} OmkTensor;

int omk_abi_version(void);
const char* omk_last_error(void);
/* 1 when the library was built for the emulator (tests only), 0 for the real gfx950 build */
int omk_is_emulated(void);
/* sizeof() of the named parameter struct ("OmkTensor", "OmkSsdFwd", ...), 0 when unknown: lets a foreign-language
 * binding check its own struct layout against the library at load time */
size_t omk_sizeof(const char* struct_name);

/* ---- fused residual-add + RMSNorm/LayerNorm -------------------------------------------------------------
 * upstream mamba_ssm.ops.triton.layer_norm.layer_norm_fn / rms_norm_fn / RMSNorm
 * reference call sites: models/stage2/block.py:10,86-95 ; models/stage2/mixer_seq_simple.py:30,428-437      */
typedef struct {
  OmkTensor x;            /* (rows, cols) activation */
  OmkTensor residual;     /* optional (rows, cols) */
  OmkTensor weight;       /* (cols) */
  OmkTensor bias;         /* optional (cols) */
  OmkTensor y;            /* out (rows, cols), dtype of x */
  OmkTensor residual_out; /* optional out (rows, cols): x + residual, its own dtype (fp32 when residual_in_fp32) */
  OmkTensor rstd;         /* optional out (rows) f32 */
  OmkTensor mean;         /* optional out (rows) f32, LayerNorm only */
  float eps;
  int32_t is_rms_norm;
} OmkAddNormFwd;
int omk_add_norm_fwd(const OmkAddNormFwd* p, omk_stream stream);

typedef struct {
  OmkTensor dy;            /* (rows, cols) */
  OmkTensor dresidual_out; /* optional incoming grad of the prenorm residual output */
  OmkTensor xsum;          /* (rows, cols) the pre-norm sum saved by forward (residual_out, or x when no residual) */
  OmkTensor weight;
  OmkTensor rstd;          /* (rows) f32 */
  OmkTensor mean;          /* optional (rows) f32 */
  OmkTensor dx;            /* out (rows, cols) */
  OmkTensor dresidual_in;  /* optional out (rows, cols): same value as dx in the residual's dtype */
  OmkTensor dweight;       /* optional out (cols) f32; absent (frozen weight): no partial sums, no reduction launch */
  OmkTensor dbias;         /* optional out (cols) f32 */
  void* workspace;
  size_t workspace_bytes;
  int32_t is_rms_norm;
  int32_t has_bias;
} OmkAddNormBwd;
size_t omk_add_norm_bwd_workspace_bytes(const OmkAddNormBwd* p);
int omk_add_norm_bwd(const OmkAddNormBwd* p, omk_stream stream);

/* ---- gated RMSNorm -----------------------------------------------------------------------------------------
 * upstream mamba_ssm.ops.triton.layernorm_gated.{RMSNorm, rmsnorm_fn}; used as Mamba2.norm(y, z)
 * reference reach: models/stage2/block.py:117 -> Mamba2.forward / Mamba2.step                                 */
typedef struct {
  OmkTensor x;      /* (rows, cols) */
  OmkTensor z;      /* optional gate (rows, cols) */
  OmkTensor weight; /* (cols) */
  OmkTensor bias;   /* optional */
  OmkTensor y;      /* out (rows, cols) */
  OmkTensor rstd;   /* optional out (rows, ngroups) f32 */
  int64_t group_size;
  float eps;
  int32_t norm_before_gate;
} OmkNormGatedFwd;
int omk_norm_gated_fwd(const OmkNormGatedFwd* p, omk_stream stream);

typedef struct {
  OmkTensor dy, x, z, weight; /* z optional */
  OmkTensor dx, dz;           /* out; dz optional */
  OmkTensor dweight;          /* optional out (cols) f32; absent (frozen weight): no partial sums, no reduction launch */
  void* workspace;
  size_t workspace_bytes;
  int64_t group_size;
  float eps;
  int32_t norm_before_gate;
} OmkNormGatedBwd;
size_t omk_norm_gated_bwd_workspace_bytes(const OmkNormGatedBwd* p);
int omk_norm_gated_bwd(const OmkNormGatedBwd* p, omk_stream stream);

/* ---- causal depthwise conv1d ---------------------------------------------------------------------------
 * upstream causal_conv1d.{causal_conv1d_fn, causal_conv1d_update}
 * reference reach: models/stage2/mixer_seq_simple.py:17,200-205 (Mamba2) ; decode via
 * models/stage2/generation.py:195-211,412-431.  Logical shape (batch, channels, seqlen); strides make both the
 * channel-last (B, L, C) storage the Mamba-2 block uses and channel-first storage legal.                    */
typedef struct {
  OmkTensor x;              /* (B, C, L) logical */
  OmkTensor weight;         /* (C, W), W in 2..4 */
  OmkTensor bias;           /* optional (C) */
  OmkTensor initial_states; /* optional (B, C, W-1) */
  OmkTensor out;            /* (B, C, L) logical */
  OmkTensor final_states;   /* optional out (B, C, W-1) */
  int32_t silu;
  /* ABI 10, optional int32 (B), 0 <= seq_lens[b] <= L: the rows of a right-padded batch end at different positions.  final_states[b]
   * holds the last state_len inputs BEFORE position seq_lens[b] (left zero-padded, initial_states standing in front as without it)
   * instead of before L; out is the same at every position.  Read on the device only (graph-capturable); a value outside 0 .. L is
   * clamped.  Present, the final states are written by a second small launch (B * C * state_len
   * threads) instead of the channel-last kernels' epilogues.  Absent: every row has length L. */
  OmkTensor seq_lens;
} OmkConv1dFwd;
int omk_causal_conv1d_fwd(const OmkConv1dFwd* p, omk_stream stream);

typedef struct {
  OmkTensor x, weight, bias, initial_states; /* bias / initial_states optional */
  OmkTensor dout;                            /* (B, C, L) */
  OmkTensor dx;                              /* out (B, C, L) */
  OmkTensor dweight;                         /* out (C, W) f32, ACCUMULATED into (caller zeroes) */
  OmkTensor dbias;                           /* optional out (C) f32, accumulated */
  OmkTensor dinitial_states;                 /* optional out (B, C, W-1) */
  int32_t silu;
  /* ABI 7, optional: with a workspace of omk_causal_conv1d_bwd_workspace_bytes() the long channel-last 16-bit kernel leaves one partial
   * dweight / dbias row per (batch, 256-token tile) and a second launch adds them up in a fixed order -- the same gradients on every run
   * and ~ 12 us less at the 1.3B slice than the fp32 atomics taken without one (NULL / too small: atomics; other layouts: unused) */
  void* workspace;
  size_t workspace_bytes;
} OmkConv1dBwd;
size_t omk_causal_conv1d_bwd_workspace_bytes(const OmkConv1dBwd* p);
int omk_causal_conv1d_bwd(const OmkConv1dBwd* p, omk_stream stream);

typedef struct {
  OmkTensor x;          /* (B, C, T), T small (1 for decode) */
  OmkTensor conv_state; /* (B, C, S), S >= W-1, updated in place */
  OmkTensor weight, bias;
  OmkTensor out;        /* (B, C, T) */
  int32_t silu;
  /* ABI 8, optional int32 (B): row b of x / out reads and writes conv_state row conv_state_indices[b] of a pool whose batch
   * dimension may exceed B.  A negative index (or one >= the pool's rows) marks a padding row: no state is read or written
   * and the row's out is zeros.  Two rows with the same non-negative index: undefined result.  Indices are read on the
   * device only (graph-capturable).  Absent: conv_state is (B, C, S) and row b is state row b. */
  OmkTensor conv_state_indices;
  /* ABI 13, optional int32 (B): row b applies only its first n_b = clamp(seq_lens[b], 0, T) tokens (the rows of a right-padded batch of
   * follow-up turns).  Afterwards its state holds the last S values of (old state ++ x[b, :, :n_b]), out[b, :, t] for t < n_b is what a
   * call on that row alone with T = n_b gives, bit for bit, and out[b, :, t] = 0 for t >= n_b.  n_b == 0: the row's state is neither
   * read nor written.  Read on the device only (graph-capturable).  Absent: every row applies T tokens, as in ABI 12. */
  OmkTensor seq_lens;
} OmkConv1dUpdate;
int omk_causal_conv1d_update(const OmkConv1dUpdate* p, omk_stream stream);

/* ---- single-token SSM state update ---------------------------------------------------------------------
 * upstream mamba_ssm.ops.triton.selective_state_update.selective_state_update (Mamba2.step)
 * reference reach: models/stage2/generation.py:195-211,412-424 -> MixerModel.forward -> Block -> Mamba2.step */
typedef struct {
  OmkTensor state;   /* (B, H, P, N) in place */
  OmkTensor x;       /* (B, H, P) */
  OmkTensor dt;      /* (B, H, P) stride 0 on P allowed */
  OmkTensor A;       /* (H, P, N) stride 0 on P,N allowed */
  OmkTensor Bm, Cm;  /* (B, G, N) */
  OmkTensor D;       /* optional (H, P) */
  OmkTensor z;       /* optional (B, H, P) */
  OmkTensor dt_bias; /* optional (H, P) */
  OmkTensor out;     /* (B, H, P) */
  int32_t dt_softplus;
  /* ABI 8, optional int32 (B): row b of x / dt / B / C / z / out reads and writes state row state_batch_indices[b] of a pool
   * whose batch dimension may exceed B.  A negative index (or one >= the pool's rows) marks a padding row: no state is read
   * or written and the row's out is zeros.  Two rows with the same non-negative index: undefined result.  Indices are read
   * on the device only (graph-capturable).  Absent: state is (B, H, P, N) and row b is state row b. */
  OmkTensor state_batch_indices;
} OmkStateUpdate;
int omk_selective_state_update(const OmkStateUpdate* p, omk_stream stream);

/* ---- multi-token SSM state extend (ABI 9) ----------------------------------------------------------------
 * T tokens of ONE turn applied to a cached state in one pass: a follow-up turn of a conversation continues the state the previous
 * turn left instead of re-running the whole conversation (Mamba2.forward with a cache at seqlen_offset > 0 and L > 1).  Per token
 * t in order:  s <- s * exp(dt_t A) + dt_t x_t (x) B_t ;  y_t = s . C_t + D x_t ;  y_t *= silu(z_t)  (dt_t: + dt_bias, softplus as
 * in OmkStateUpdate).  The fields mean what they mean in OmkStateUpdate with a token dimension after the batch; the state is
 * read once, kept in fp32 for all T tokens and stored once (one rounding for a 16-bit state).  An fp32 state ends bit-identical
 * to T omk_selective_state_update calls.  Layouts: N in {16, 32, 64, 128} with unit stride on n and 4-element aligned rows of
 * state / B / C, any T >= 0; anything else returns OMK_EUNSUPPORTED (step such a state token by token).  Graph-capturable. */
typedef struct {
  OmkTensor state;   /* (B, H, P, N) in place */
  OmkTensor x;       /* (B, T, H, P) */
  OmkTensor dt;      /* (B, T, H, P) stride 0 on P allowed */
  OmkTensor A;       /* (H, P, N) stride 0 on P,N allowed */
  OmkTensor Bm, Cm;  /* (B, T, G, N) */
  OmkTensor D;       /* optional (H, P) */
  OmkTensor z;       /* optional (B, T, H, P) */
  OmkTensor dt_bias; /* optional (H, P) */
  OmkTensor out;     /* (B, T, H, P): y_t of every token */
  int32_t dt_softplus;
  /* optional int32 (B), ABI 8's meaning: row b extends state row state_batch_indices[b] of a pool whose batch dimension may
   * exceed B; a negative index (or one >= the pool's rows) marks a padding row: no state is read or written and its T outputs
   * are zeros.  Absent: state is (B, H, P, N) and row b is state row b. */
  OmkTensor state_batch_indices;
  /* ABI 13, optional int32 (B): row b applies only its first n_b = clamp(seq_lens[b], 0, T) tokens (the rows of a right-padded batch of
   * follow-up turns).  Its state is stored once, after token n_b - 1; out[b, t] for t < n_b and the state are what a call on that row
   * alone with T = n_b gives, bit for bit; out[b, t] = 0 for n_b <= t < T.  n_b == 0: the row's state is neither read nor written
   * (what a padding slot does).  Read on the device only (graph-capturable).  Absent: every row applies T tokens, as in ABI 12. */
  OmkTensor seq_lens;
} OmkStateExtend;
int omk_selective_state_extend(const OmkStateExtend* p, omk_stream stream);

/* ---- Mamba-1 selective scan ----------------------------------------------------------------------------
 * upstream mamba_ssm.ops.selective_scan_interface.selective_scan_fn (BASELINE.json configs[0] signature)
 * reference reach: models/stage2/mixer_seq_simple.py:16,197-201 (ssm_cfg.layer == "Mamba1")                  */
typedef struct {
  OmkTensor u, delta;   /* (B, D, L) logical, any strides */
  OmkTensor A;          /* (D, N) f32 */
  OmkTensor Bm, Cm;     /* (B, G, N, L) logical (G=1 for the 3-d form) or (D, N) constant (ndim == 2) */
  OmkTensor D;          /* optional (D) */
  OmkTensor z;          /* optional (B, D, L) */
  OmkTensor delta_bias; /* optional (D) */
  OmkTensor out;        /* (B, D, L) */
  OmkTensor last_state; /* optional out (B, D, N) f32 */
  OmkTensor pass_states;/* optional out (B, D, ceil(L / 512), N) f32, contiguous: the state in front of every 512-token pass of the
                           chunked scan -- hand it to omk_selective_scan_bwd and the backward skips its state-only forward pass.
                           Needs L-contiguous u / delta / z / out / B / C and L >= 64, or form 2 below (OMK_EUNSUPPORTED otherwise). */
  int32_t delta_softplus;
} OmkSelScanFwd;
int omk_selective_scan_fwd(const OmkSelScanFwd* p, omk_stream stream);
/* Which form omk_selective_scan_fwd takes for these tensors (nothing is launched): 2 = lanes-are-channels sweep (channel-last (B, L, D)
 * or L-contiguous storage, d_state <= 16, variable B / C of u's dtype, and enough (batch, 64-channel tile) waves to fill the chip --
 * or L < 64), 1 = chunked associative scan (L-contiguous rows, lanes = time), 0 = per-channel sequential kernel; < 0: omk_status.
 * A host that holds channel-last views asks before it decides to make L-contiguous copies (omnimamba_amd/selective_scan.py). */
int omk_selective_scan_fwd_form(const OmkSelScanFwd* p);

typedef struct {
  OmkTensor u, delta, A, Bm, Cm, D, z, delta_bias; /* as forward */
  OmkTensor dout;                                  /* (B, D, L) */
  OmkTensor du, ddelta;                            /* out (B, D, L) */
  OmkTensor dA;                                    /* out (D, N) f32 accumulated */
  OmkTensor dB, dC;                                /* out f32 accumulated: (B, G, N, L) for variable B / C, (D, N) for constant */
  OmkTensor dD;                                    /* optional out (D) f32 accumulated */
  OmkTensor dz;                                    /* optional out (B, D, L) */
  OmkTensor ddelta_bias;                           /* optional out (D) f32 accumulated */
  OmkTensor pass_states;                           /* optional in: what omk_selective_scan_fwd left (chunked form only) */
  void* workspace;                                 /* state checkpoints of the recomputed forward */
  size_t workspace_bytes;
  int32_t delta_softplus;
} OmkSelScanBwd;
/* ABI 6: which form omk_selective_scan_bwd takes on these views (nothing is launched; it is the launch's own decision): 2 = the
 * lanes-are-channels reverse sweep on channel-last (B, L, D) views as they lie (input-dependent B / C of u's dtype, d_state <= 16, enough
 * sequences to fill the chip), 1 = the chunked scan (L-contiguous u / delta / z / dout / du / ddelta / dz / B / C, input-dependent B / C of
 * u's dtype, fp32 A, 8 | channels per group, L >= 64), 0 = the per-channel kernel (which refuses d_state > 16).  The host mirror asks
 * before it decides about L-contiguous copies (omk_selective_scan_fwd_form's twin). */
int omk_selective_scan_bwd_form(const OmkSelScanBwd* p);
size_t omk_selective_scan_bwd_workspace_bytes(const OmkSelScanBwd* p);
int omk_selective_scan_bwd(const OmkSelScanBwd* p, omk_stream stream);   /* L-contiguous rows, variable B / C, L >= 64, 8 | channels
                                                                             per group: d_state <= 64; other layouts: d_state <= 16 */

/* ---- decode-step projection fused with the normalisation in front of it ----------------------------------
 * one launch for: reference block.py:86-95 (fused add + RMSNorm) -> lora.py:185-279 (base + task LoRA) at one token
 * per sequence, and for Mamba2.step's gated RMSNorm -> out_proj (upstream mamba2.py step()).  One sequence: any dtype mix.  Two to eight
 * sequences: one dtype for activations / weights / norm weight / LoRA (fp32 or bf16), in_features 1024 / 2048 / 4096.
 * Anything else returns OMK_EUNSUPPORTED: use the separate ops.
 *
 * ABI 11, weight-only fp8: `weight` may hold OMK_F8E4M3 codes with one fp32 scale per output row in `weight_scale`:
 *   out = rstd * (weight_scale[row] * sum_i decode(weight[row, i]) * u_i  +  lora_scale * B (A u))  [+ bias, conv tail as above]
 * The codes are converted at the multiply and the scale is applied once per row, in fp32, behind the wave reduction; no dequantised copy
 * of the matrix exists.  Activations, norm weight, LoRA factors, bias, conv tensors and the output keep ONE dtype (fp32 or bf16, the dtype
 * of x; the residual fp32 or that dtype).  Served by the uniform-dtype kernels only -- one norm group, LoRA rank <= 8, in_features 1024 /
 * 2048 / 4096, B <= 8, weight rows 16-byte aligned (stride(0) % 16 == 0); anything else returns OMK_EUNSUPPORTED, never the
 * run-time-dtype kernel.  Two to eight sequences: under bf16 activations the matrix form (ABI 12: the codes become bf16 operands of
 * v_mfma_f32_16x16x32_bf16 as they land -- exact -- under the conditions of a bf16 weight), under fp32 activations the vector form.  weight_scale without an fp8 weight, an fp8 weight without weight_scale, or a
 * scale that is not contiguous fp32 (out): OMK_EINVAL.                                                                */
typedef struct {
  OmkTensor x;             /* (B, in) */
  OmkTensor residual;      /* optional (B, in): added before the norm */
  OmkTensor z;             /* optional (B, in): gate of the gated norm (dtype of x) */
  OmkTensor norm_weight;   /* optional (in): RMSNorm weight; absent = no normalisation */
  OmkTensor weight;        /* (out, in) f32 / bf16 / f16, or OMK_F8E4M3 with weight_scale (ABI 11); 16-byte aligned rows */
  OmkTensor bias;          /* optional (out) */
  OmkTensor lora_a;        /* optional (r, in), r <= 16 */
  OmkTensor lora_b;        /* optional (out, r) */
  OmkTensor residual_out;  /* optional out (B, in): x + residual */
  OmkTensor out;           /* out (B, out) */
  /* optional tail for the in_proj call of Mamba2.step: output rows [conv_offset, conv_offset + C) are the new xBC inputs;
   * they are pushed through causal_conv1d_update (+ SiLU) right where they are produced -- out holds the convolved
   * values, conv_state (B, C, S) is rolled in place -- so the step needs no separate convolution launch.  Only taken by
   * the uniform-dtype kernel (all of x / weight / conv tensors one dtype); otherwise OMK_EUNSUPPORTED. */
  OmkTensor conv_state;    /* optional (B, C, S), S = W-1 .. 4, in place */
  OmkTensor conv_weight;   /* (C, W), W = 2 .. 4 */
  OmkTensor conv_bias;     /* optional (C) */
  int64_t group_size;      /* norm group size (0 = in) */
  int64_t conv_offset;
  float eps;
  float lora_scale;
  int32_t norm_before_gate;
  int32_t conv_silu;
  /* ABI 8, optional int32 (B), only with conv_state: sequence b rolls conv_state row conv_state_indices[b] of a pool whose
   * batch dimension may exceed B.  A negative index (or one >= the pool's rows) marks a padding row: its conv state is not
   * read or written and its conv columns [conv_offset, conv_offset + C) of out are zeros (the other columns are computed as
   * usual).  Two rows with the same non-negative index: undefined result.  Indices are read on the device only. */
  OmkTensor conv_state_indices;
  /* ABI 11, fp32 contiguous (out): the per-row scale of an OMK_F8E4M3 weight.  Present exactly when weight.dtype == OMK_F8E4M3. */
  OmkTensor weight_scale;
} OmkNormLinear;
int omk_norm_linear(const OmkNormLinear* p, omk_stream stream);
/* ABI 12: which kernel omk_norm_linear runs for this call (nothing is launched; it is the launch's own decision, made by the same code):
 * GENERIC = one sequence, run-time dtypes; FAST = one sequence, uniform dtype; BATCHED = two to eight sequences on the vector pipe;
 * MATRIX = two to eight sequences on the matrix pipe (bf16 weights; fp8 weights under bf16 activations; fp32 weights at eight sequences
 * with LoRA and <= 2048 features).  < 0: the omk_status with which omk_norm_linear would refuse the call.  A call with no sequence or no
 * output row launches nothing and reports GENERIC. */
enum { OMK_NL_FORM_GENERIC = 0, OMK_NL_FORM_FAST = 1, OMK_NL_FORM_BATCHED = 2, OMK_NL_FORM_MATRIX = 3 };
int omk_norm_linear_form(const OmkNormLinear* p);

/* ---- task LoRA of a projection: out += scale * h lora_b^T, in place ------------------------------------------
 * reference models/stage2/lora.py:263-279 (result += lora_B(lora_A(dropout(x))) * scaling) at training / prefill token counts.
 * Rank 8 or 16, 16-byte aligned rows; otherwise OMK_EUNSUPPORTED (callers use a GEMM).                              */
typedef struct {
  OmkTensor out;     /* (T, N) in place */
  OmkTensor h;       /* (T, r) = lora_A(dropout(x)), dtype of out */
  OmkTensor lora_b;  /* (N, r) */
  OmkTensor mask;    /* optional (T, N) u8, rows contiguous: only elements with a non-zero mask byte receive the update (the
                        dropout in front of lora_A, seen from its backward: dx += mask / (1 - p) * (dh A)) */
  float scale;
} OmkLoraAdd;
int omk_lora_add(const OmkLoraAdd* p, omk_stream stream);

/* ---- backward of the rank-r up-projection, both products in ONE pass over dy --------------------------------------------
 * dh (T, r) = dy (T, N) lora_b (N, r)   and   dlora_b (N, r) = dy^T h (T, r)   (reference lora.py:263-279, backward of
 * lora_B(.)).  As two library GEMMs each reads the (tokens, 8512) gradient once (279 MB at 16 k tokens: 69 + 59 us).
 * bf16 dy / h, rank 8, 16-byte aligned rows.  The kernel leaves PARTIAL sums -- dh per 256-column block of dy, dlora_b per token
 * chunk -- that the caller adds up (two small reductions: deterministic, no atomics); omk_lora_up_bwd_parts gives the counts.   */
typedef struct {
  OmkTensor dy;       /* (T, N) bf16 */
  OmkTensor lora_b;   /* (N, r) f32 / bf16 / f16 */
  OmkTensor h;        /* (T, r) bf16 */
  OmkTensor dh;       /* out (column_blocks, T, r) f32, dense: every element is written */
  OmkTensor dlora_b;  /* out (token_chunks, N, r) f32, dense: every element is written */
} OmkLoraUpBwd;
/* column_blocks -> parts[0], token_chunks -> parts[1] for a (T, N) gradient */
int omk_lora_up_bwd_parts(int64_t T, int64_t N, int32_t* parts);
int omk_lora_up_bwd(const OmkLoraUpBwd* p, omk_stream stream);

/* ---- Mamba-2 SSD chunked scan ----------------------------------------------------------------------------
 * upstream mamba_ssm.ops.triton.ssd_combined.mamba_chunk_scan_combined (+ the scan stage of
 * mamba_split_conv1d_scan_combined); reference reach: models/stage2/block.py:117 -> Mamba2.forward              */
typedef struct {
  OmkTensor x;              /* (B, L, H, P) */
  OmkTensor dt;             /* (B, L, H) raw dt (before bias/softplus/clamp) */
  OmkTensor A;              /* (H) f32, negative */
  OmkTensor Bm, Cm;         /* (B, L, G, N) */
  OmkTensor D;              /* optional (H) or (H, P) */
  OmkTensor z;              /* optional (B, L, H, P): out = y * silu(z) */
  OmkTensor dt_bias;        /* optional (H) */
  OmkTensor initial_states; /* optional (B, H, P, N) */
  OmkTensor out;            /* (B, L, H, P); absent = the STATE-ONLY pass: only final_states is produced (one shard of a
                             * sequence cut over several GPUs, omnimamba_amd/context_parallel.py) -- MFMA shape only, else
                             * OMK_EUNSUPPORTED; Cm, D are ignored */
  OmkTensor out_x;          /* optional out (B, L, H, P): the pre-gate y (only meaningful with z; saved for backward) */
  OmkTensor final_states;   /* optional out (B, H, P, N) f32 */
  OmkTensor window_states;  /* optional out, bf16, contiguous, omk_ssd_scan_fwd_window_states_bytes(p) bytes: the carried state in
                             * front of every 128-token window, (B, ceil(L / 128), H) images of 16 KB in the kernel's own operand
                             * layout.  A training forward saves it and hands it to omk_ssd_scan_bwd, which then skips its own
                             * state pass over x (upstream's backward recomputes the chunk states the same way, ssd_combined.py
                             * _mamba_chunk_scan_combined_bwd).  Opaque: only omk_ssd_scan_bwd reads it */
  void* workspace;
  size_t workspace_bytes;
  float dt_min, dt_max;     /* clamp (dt_limit); (0, +inf) = none */
  int32_t dt_softplus;
  int32_t chunk_size;       /* API parity only: the result does not depend on it */
  int32_t force_generic;    /* 1 = use the shape-generic fp32 VALU kernel even when the MFMA kernel applies */
  int32_t flags;            /* ABI 6: OMK_SSD_* bits below, 0 = the default kernels.  Per call -- the library reads no environment
                             * variable but the test hooks of INTEGRATION.md section 4, which only lower size thresholds */
  OmkTensor conv_weight;    /* ABI 6, optional (H * P, width <= 4): K2 fusion of the forward-only path (prefill / inference).  When present,
                             * x is the PRE-conv input of upstream's causal_conv1d_fn(..., activation="silu") for the x channels of xBC, and
                             * the scan applies out[t] = silu(bias + sum_k w[k] x[t - width + 1 + k]) (zeros in front of the sequence) while
                             * it stages x -- same fp32 arithmetic and the same single bf16 rounding as omk_causal_conv1d_fwd, so the result
                             * equals conv kernel + scan bit for bit.  B / C stay the conv OUTPUT (a 2 G N-channel conv launch of the caller).
                             * Plain bf16 forward on the specialised-wave kernel only (no z / out_x / window_states / PRECISE, sequence not
                             * split): otherwise OMK_EUNSUPPORTED and the caller runs conv + scan separately.
                             * reference: models/stage2/generation.py:195-211 prefill, scripts/inference_mmu.py:137-147 */
  OmkTensor conv_bias;      /* optional (H * P) */
  OmkTensor seq_lens;       /* ABI 10, optional int32 (B), 0 <= seq_lens[b] <= L: the rows of a right-padded batch end at different positions.
                             * Tokens t >= seq_lens[b] do not change row b's state: final_states[b] is the state after seq_lens[b] tokens
                             * (after 0 tokens: initial_states[b], or zero); out[b, t] for t < seq_lens[b] is what it is without seq_lens,
                             * for the masked t it is finite for finite inputs and otherwise unspecified.  The masked tokens enter every
                             * scan kernel with dt' = +0 (written by the dt preparation), the way tokens behind L already do inside the
                             * last chunk; no chunk is skipped.  Works with initial_states and conv_weight; window_states / the state-only
                             * pass take none (OMK_EINVAL).  Read on the device only (graph-capturable).  Absent: every row has length L. */
} OmkSsdFwd;
/* OmkSsdFwd::flags / OmkSsdBwd::flags */
#define OMK_SSD_PRECISE      1  /* forward, bf16 MFMA scan: the carried state meets C as a bf16 hi + lo pair and the state-update operand is
                                 * hi + lo: y within 1e-3 (arithmetic, rel-L2) of the fp32 recurrence on EVERY head, slow-decay heads
                                 * included (the default rounds both to bf16 once, as the reference pipeline does: 1.3e-3 .. 2.3e-3 there).
                                 * Price: profiles/r06_precise.txt.  Window states cannot be saved by a PRECISE forward */
#define OMK_SSD_KHILO        2  /* forward: only the state-update operand as hi + lo (the carried state / final_states exact to fp32
                                 * accumulation); implied whenever final_states is asked for */
#define OMK_SSD_EVERY_CHUNK  4  /* specialised-wave kernel: rescale the carried state at every chunk end instead of only where its basis
                                 * drifts by 2^60 (the arithmetic of the column-slice kernel, bit for bit; tests) */
#define OMK_SSD_NO_SPLIT     8  /* never cut the sequence into segments (few (batch, head) sequences normally are: csrc/ssd_scan.h) */
#define OMK_SSD_COLUMN_SLICE 16 /* class A scans on the column-slice kernel (ssd_a6.hip) instead of the specialised-wave kernel */
/* Measurement aid (ABI 6): the kernels the LAST recording call of this thread launched, ';'-separated, template arguments included, e.g.
 * "ssd_dt_prep;ssd_a8<mode=0,dump=1,khilo=0,precise=0>", "selscan_fwd_shared<lc=8,nu=2,state_only=0>" or
 * "conv1d_bwd_cl4<t=bf16,w=4,wf=1>;conv1d_bwd_fold".  Recording calls: omk_ssd_scan_fwd / _bwd, omk_selective_scan_fwd / _bwd and the
 * backward ops omk_causal_conv1d_bwd, omk_add_norm_bwd and omk_norm_gated_bwd.  Each resets the list on entry -- a refused or empty call
 * leaves it empty -- so read it right behind the call you mean.  bench.py puts it next to its HIP-event time and refuses a PMC traffic file
 * (profiles/ssd_*_traffic.json) recorded for another kernel. */
const char* omk_ssd_last_kernels(void);
size_t omk_ssd_scan_fwd_workspace_bytes(const OmkSsdFwd* p);
/* bytes of window_states for these arguments (window_states itself is not looked at); 0 = this forward cannot save them (shape
 * outside the MFMA kernel, gate / out_x requested, fp32 activations): pass none */
size_t omk_ssd_scan_fwd_window_states_bytes(const OmkSsdFwd* p);
int omk_ssd_scan_fwd(const OmkSsdFwd* p, omk_stream stream);

typedef struct {
  OmkTensor x, dt, A, Bm, Cm, D, dt_bias, initial_states; /* as forward.  z gating is NOT part of this call: the
                                caller passes dout * silu(z) and forms dz = dout * out_x * silu'(z) itself (out_x = the
                                forward's pre-gate output) */
  OmkTensor y;               /* optional (B, L, H, P): the forward's pre-gate output.  Accepted for signature parity with
                                upstream's backward; no kernel reads it (the scans recompute what they need) */
  OmkTensor dout;            /* (B, L, H, P) grad of the (pre-gate) output */
  OmkTensor dfinal_states;   /* optional (B, H, P, N) f32 */
  OmkTensor dx;              /* out (B, L, H, P) */
  OmkTensor ddt;             /* out (B, L, H) f32: grad wrt RAW dt */
  OmkTensor dA;              /* out (H) f32 */
  OmkTensor dB, dC;          /* out (B, L, G, N) */
  OmkTensor dD;              /* optional out (H) or (H, P) f32 */
  OmkTensor ddt_bias;        /* optional out (H) f32 */
  OmkTensor dinitial_states; /* optional out (B, H, P, N) f32 */
  OmkTensor window_states;   /* optional in: what omk_ssd_scan_fwd left in its window_states for the SAME x, dt, A, Bm, dt_bias,
                                initial_states and clamp; ignored by the paths that do not use window states */
  void* workspace;
  size_t workspace_bytes;
  float dt_min, dt_max;
  int32_t dt_softplus;
  int32_t chunk_size;
  int32_t force_generic;
  int32_t flags;             /* ABI 6: OMK_SSD_NO_SPLIT, OMK_SSD_COLUMN_SLICE, OMK_SSD_EVERY_CHUNK, OMK_SSD_SEQUENTIAL_BWD */
} OmkSsdBwd;
#define OMK_SSD_SEQUENTIAL_BWD 32 /* backward: the three sequential MFMA scans of rounds 1 - 2 instead of the chunk-parallel dB / dC */
size_t omk_ssd_scan_bwd_workspace_bytes(const OmkSsdBwd* p);
int omk_ssd_scan_bwd(const OmkSsdBwd* p, omk_stream stream);

/* ---- cross entropy over one block of logits: loss per row + the gradient written over the logits ----------------
 * The loss the reference forms from the heads' outputs (models/mamba_vlm.py:88-102 shift + flatten; models/omnimamba.py:63,
 * 276-279,305-306: torch.nn.CrossEntropyLoss(), mean over the labels that are not -100).  Used by the chunked fused
 * linear + cross-entropy of omnimamba_amd/fused_ce.py, which never holds more than one token block of logits
 * (SURVEY.md section 8 row f1).  Per row r (label y):  loss[r] = logsumexp(logits[r]) - logits[r][y];
 * logits[r][v] <- (softmax(logits[r])[v] - [v == y]) * grad_scale[0]   (rows with label == ignore_index: loss 0, gradient 0). */
typedef struct {
  OmkTensor logits;        /* (T, V) in / out (the gradient), unit stride on V */
  const int64_t* labels;   /* (T) */
  OmkTensor losses;        /* out (T) f32 */
  const float* grad_scale; /* device scalar the gradient is multiplied with (1 / number of counted labels); NULL = 1 */
  int64_t ignore_index;
  int32_t write_grad;      /* 0: only the losses */
} OmkCrossEntropy;
int omk_cross_entropy(const OmkCrossEntropy* p, omk_stream stream);

/* ---- token sampling inside the decode step --------------------------------------------------------------
 * reference models/stage2/generation.py:87-121 `sample(logits, top_k, top_p, min_p, temperature)`: the top_k == 1 short cut
 * (argmax) and the top_k > 0 branch (top-k -> / temperature -> top-p filter of :64-76 -> multinomial), for 1 <= top_k <= 64.
 * One uniform per row from Philox4x32-10 keyed by (seed, row, *step_counter + offset): the reference draws with
 * torch.multinomial, so the ids agree in distribution (and exactly for top_k == 1), not stream for stream.  step_counter is a
 * device int64 the caller advances (inside its captured graph), NULL = 0.  top_k == 0 is the whole-vocabulary branch (:107-119):
 * the plain multinomial of softmax(logits / temperature) (the default arguments of t2i_generate), behind the reference's top-p cut
 * when 0 < top_p < 1 (ascending cumulative probability <= 1 - top_p is cut, ties at the boundary in index order) or, ABI 7, behind its
 * min_p filter when min_p > 0 (a raw logit below min_p x the largest softmax(logits) probability is cut -- the reference's own
 * comparison, :43; top_p is ignored then, as there; a row with nothing left returns its arg max where the reference raises).      */
typedef struct {
  OmkTensor logits;        /* (batch, vocab) f32 / bf16 / f16, unit last stride */
  OmkTensor out_ids;       /* out (batch) int64, dense (dtype field ignored) */
  const void* step_counter; /* optional device int64 */
  uint64_t seed, offset;
  int32_t top_k;           /* 0 (whole vocabulary) or 1 .. 64 */
  float top_p, temperature;
  float min_p;             /* ABI 7 (occupies the former tail padding): 0 = off; > 0 only with top_k == 0 */
} OmkSample;
int omk_sample(const OmkSample* p, omk_stream stream);

/* ---- ABI 14: the sampler with one set of settings PER ROW (continuous batching: every row of a decode step is another request) ----
 * One launch, one workgroup per row, the branches of omk_sample chosen row by row; every setting is a device array of `batch` entries,
 * so the launch reads nothing from the host and a captured step replays it while the arrays are rewritten in between.
 * Random stream: row b draws the uniform that omk_sample draws for row 0 of a one-row batch with seed = seeds[b], offset = steps[b] and no
 * step_counter -- Philox4x32-10, counter (0, steps[b] lo, steps[b] hi, 0), key seeds[b].  The row index is NOT in the counter: the id of a
 * row depends on its logits and its own settings only, not on where in the batch it sits or on what its neighbours are.
 * Repetition penalty (reference generation.py:73-85, optional): the logit of every id in history[b][0 .. history_lens[b]) is multiplied by
 * penalty[b] when negative and divided by it (IEEE division) otherwise, ONCE however often the id occurs, and rounded to the dtype of the
 * logits, before any branch looks at the row; penalty[b] == 1 (or no penalty / history array) leaves the row alone.  `logits` is never
 * written.  Nothing in the arrays can be checked on the host, so the kernel defines it: top_k is clamped to [0, 64], a history id outside
 * [0, vocab) is skipped, history_lens[b] is clamped to [0, history_cap].  A non-positive or NaN temperature counts as 1, a non-positive
 * penalty as 1, min_p applies with top_k == 0 only.  active[b] == 0 (optional; the padding rows of a bucket): the row writes nothing and
 * none of its settings has any effect (they may hold anything; its history and penalty are not read).  Its entries are still loaded: every
 * required array holds `batch` valid entries, inactive rows included.  OMK_EUNSUPPORTED: a history with a vocabulary too large for the kernel's id map (penalise a copy instead).
 * ---- ABI 16: per-row logit edits (logit_bias, banned ids, allowed token sets), fused into the same launch as a third instantiation -------
 * Row b carries a list of edit_lens[b] entries (edit_ids[b][j], edit_vals[b][j]) and a mode edit_mode[b].  Every branch sees, in every one
 * of its passes, the row e instead of the raw row x (T the dtype of the logits):
 *   p_i = the repetition-penalised x_i, rounded to T, as above (x_i when token i is not in the history or the penalty is off)
 *   i listed:      e_i = round_T(float(p_i) + edit_vals[b][j]), j the LOWEST entry index with edit_ids[b][j] == i (the first entry wins)
 *   i not listed:  e_i = -inf when edit_mode[b] == 1 (allow-only: the list is the set of tokens that may be drawn), p_i otherwise
 * `logits` is never written.  Nothing in the arrays is trusted, the kernel defines it: edit_lens[b] is clamped to [0, edit_cap]; an id
 * outside [0, vocab) is skipped; an edit_mode other than 1 counts as 0; an allow-only row whose list holds no valid id is unconstrained
 * (mode 0 with an empty list).  A value of -inf bans the token.  A value of +inf or NaN, and a row left without a finite logit, give an
 * unspecified id in [0, vocab) in bounded time.  Inactive rows read none of it.  Absent edit_ids, or edit_cap == 0: the launch is the ABI
 * 14 launch, instruction for instruction.  edit_ids without edit_vals or edit_lens: OMK_EINVAL.  OMK_EUNSUPPORTED: edit_cap above 512, or
 * edits with a vocabulary too large for the id map (65 536 tokens) -- edit a copy instead.  LDS of a workgroup: 44 792 B static, the id
 * map (vocab rounded up to 16 B: bit 0 of a byte = the token is in the history, bit 1 = it is listed, bits 2 - 7 = entry index / 8 of the
 * first entry that lists it), 8 B per entry of edit_cap rounded up to 8, one word: at most 114 436 B of the 163 840 B of a workgroup.      */
typedef struct {
  OmkTensor logits;          /* (batch, vocab) f32 / bf16 / f16, unit last stride; read only */
  OmkTensor out_ids;         /* out (batch) int64, dense (dtype field ignored) */
  const void* top_k;         /* device int32 (batch) */
  const void* top_p;         /* device f32 (batch) */
  const void* temperature;   /* device f32 (batch) */
  const void* min_p;         /* device f32 (batch) */
  const void* seeds;         /* device uint64 (batch) */
  const void* steps;         /* device int64 (batch) */
  const void* penalty;       /* optional device f32 (batch); NULL = 1 everywhere */
  const void* history;       /* optional device int64 (batch, history_cap), row b at history + b * history_stride */
  const void* history_lens;  /* device int32 (batch); required with history */
  const void* active;        /* optional device int32 (batch); NULL = every row */
  int64_t history_stride;    /* elements between the rows of history */
  int64_t history_cap;       /* width of history */
  const void* edit_ids;      /* ABI 16, optional: device int64 (batch, edit_cap), row b at edit_ids + b * edit_stride */
  const void* edit_vals;     /* ABI 16: device f32, the layout of edit_ids; required with edit_ids */
  const void* edit_lens;     /* ABI 16: device int32 (batch); required with edit_ids */
  const void* edit_mode;     /* ABI 16, optional: device int32 (batch), 1 = allow-only; NULL = 0 everywhere */
  int64_t edit_stride;       /* ABI 16: elements between the rows of edit_ids and of edit_vals */
  int64_t edit_cap;          /* ABI 16: width of edit_ids and edit_vals, at most 512; 0 = no edits */
} OmkSampleRows;
int omk_sample_rows(const OmkSampleRows* p, omk_stream stream);
/* Which launch omk_sample_rows takes for *p, decided by the code that launches (nothing is launched here): OMK_SAMPLE_ROWS_*, or the
 * negative omk_status the call would be refused with (omk_last_error says why). */
#define OMK_SAMPLE_ROWS_PLAIN 0   /* no id map: no penalty with a history, no edits */
#define OMK_SAMPLE_ROWS_PENALTY 1 /* the id map of the histories (ABI 14) */
#define OMK_SAMPLE_ROWS_EDIT 2    /* the id map and the rows' edit lists (ABI 16) */
int omk_sample_rows_form(const OmkSampleRows* p);

/* ---- ABI 15: log-probabilities of the tokens a decode step sampled, the top_n most likely tokens of every row and the sampled token's rank ----
 * One launch, one workgroup per row, a launch of its own behind the sampler (the sampler kernels are not touched); nothing is read from
 * the host, so a captured step replays it while logits, ids and active are rewritten in between.  All values are those of the RAW row:
 * no temperature, filter or repetition penalty (what serving APIs report by default).
 *   lse        = m + log(sum_v exp(x_v - m)), x in fp32, m the row maximum; the sum runs in a fixed order that depends on neither the row's
 *                index nor the batch size: the outputs of a row are the same bits wherever it sits
 *   logprob[b] = x[ids[b]] - lse
 *   The tokens of a row are ordered by (value descending, index ascending): top_ids / top_logprobs hold the first top_n of that order, entries
 *   past vocab (top_n > vocab) id -1 and logprob -inf; rank[b] is the 1-based position of ids[b] in it.
 * Nothing in ids is trusted: an id outside [0, vocab) gives logprob NaN and rank 0 and reads nothing.  A -inf logit scores -inf.  A row whose
 * maximum is -inf, or that holds a NaN, gives unspecified values in bounded time; the mutual order of -0 and +0 is unspecified.
 * active[b] == 0 (optional; the padding rows of a bucket): the row writes nothing and none of its inputs has an effect.
 * ids == NULL: top_n only (logprob and rank are not written); with ids, logprob is required and rank optional.                          */
typedef struct {
  OmkTensor logits;          /* (rows, vocab) f32 / bf16 / f16, unit last stride, any row stride; read only */
  OmkTensor logprob;         /* out (rows) f32, any stride; required with ids */
  OmkTensor rank;            /* out (rows) int32, any stride; optional */
  OmkTensor top_ids;         /* out (rows, top_n) int64, any strides (dtype field ignored); required with top_n > 0 */
  OmkTensor top_logprobs;    /* out (rows, top_n) f32, any strides; required with top_n > 0 */
  const void* ids;           /* optional device int64 (rows): the token to score in each row */
  const void* active;        /* optional device int32 (rows); NULL = every row */
  int32_t top_n;             /* 0 .. 64 */
} OmkTokenLogprobs;
int omk_token_logprobs(const OmkTokenLogprobs* p, omk_stream stream);

/* ---- ABI 17: presence and frequency penalties as a device-built edit list for omk_sample_rows ------------------------------------------
 * One launch in front of the sampler, one workgroup per row, nothing read from the host: row b's edit list for OMK_SAMPLE_ROWS_EDIT is built
 * from its history and merged with the request's own list.  The sampler kernels are not touched.  In fp32 unless said otherwise:
 *   len     = clamp(history_lens[b], 0, history_cap); the COUNTED RANGE is history[b][clamp(count_start[b], 0, len) .. len)
 *   c_i     = how often token i occurs in the counted range (ids outside [0, vocab) are skipped)
 *   delta_i = 0 when c_i == 0, else -((frequency[b] * float(c_i)) + presence[b]) -- the product and the sum are rounded SEPARATELY, never
 *             a fused multiply-add; a non-finite frequency[b] or presence[b] counts as 0
 * With the list this launch writes, omk_sample_rows sees (p_i and round_T as ABI 14 / 16 define them, val_i the value of the FIRST user
 * entry that names i):
 *   i listed and counted:      e_i = round_T(float(p_i) + (val_i + delta_i))      (the inner sum first)
 *   i listed, not counted:     e_i = round_T(float(p_i) + val_i)                  (ABI 16 as it is)
 *   i not listed, counted:     e_i = round_T(float(p_i) + delta_i); -inf in an allow-only row (the allowed set wins)
 *   neither:                   e_i = p_i; -inf in an allow-only row
 * Allow-only as in ABI 16: edit_mode[b] == 1 and the user list holds a valid id (without one the row is unconstrained and gets the
 * penalties).  Row b's output:
 *   1. its n_user = clamp(edit_lens[b], 0, edit_cap) user entries first, in their order, ids unchanged (invalid ones too); the value of a
 *      valid id with c_id > 0 is edit_vals + delta_id (-inf stays -inf), every other value is unchanged
 *   2. not allow-only: behind them one entry (i, delta_i) for every distinct counted token i that no valid user entry names, in the order
 *      of their first occurrence in the counted range
 *   3. out_lens[b] = the total, clamped to out_cap; entries that do not fit are dropped, entries behind out_lens[b] are not written
 *   4. out_mode[b] = 1 for an allow-only row, else 0
 *   5. active[b] == 0 (optional): the row writes nothing
 *   6. both penalties zero or non-finite, or an empty counted range: the user list, as it is
 * Correct for a counted range of any length up to history_cap; the work grows with its square, and it is sized for the at most 512 entries
 * a row's list holds in omk_sample_rows.  The outputs must not overlap the user list.  Capturable; every array may be rewritten between
 * replays.  OMK_EINVAL: a required array missing (history, history_lens, count_start, frequency, presence, the four outputs), edit_ids
 * without edit_vals or edit_lens, a negative cap or batch, a vocabulary outside [1, 2^31), with more than one row a row stride below the
 * width of its array.  batch == 0: OMK_OK, nothing is launched.                                                                      */
typedef struct {
  const void* history;       /* device int64 (batch, history_cap), row b at history + b * history_stride */
  const void* history_lens;  /* device int32 (batch) */
  const void* count_start;   /* device int32 (batch): where in the row's history the counted range begins */
  const void* frequency;     /* device f32 (batch) */
  const void* presence;      /* device f32 (batch) */
  const void* active;        /* optional device int32 (batch); NULL = every row */
  int64_t history_stride;    /* elements between the rows of history */
  int64_t history_cap;       /* width of history */
  const void* edit_ids;      /* optional user list, the layout of OmkSampleRows: device int64 (batch, edit_cap) */
  const void* edit_vals;     /* device f32, the layout of edit_ids; required with edit_ids */
  const void* edit_lens;     /* device int32 (batch); required with edit_ids */
  const void* edit_mode;     /* optional device int32 (batch), 1 = allow-only; NULL = 0 everywhere */
  int64_t edit_stride;       /* elements between the rows of edit_ids and of edit_vals */
  int64_t edit_cap;          /* width of edit_ids and edit_vals; 0 = no user list */
  void* out_ids;             /* out: device int64 (batch, out_cap), row b at out_ids + b * out_stride */
  void* out_vals;            /* out: device f32, the layout of out_ids */
  void* out_lens;            /* out: device int32 (batch) */
  void* out_mode;            /* out: device int32 (batch) */
  int64_t out_stride;        /* elements between the rows of out_ids and of out_vals */
  int64_t out_cap;           /* width of out_ids and out_vals */
  int64_t batch;             /* rows */
  int64_t vocab;             /* ids outside [0, vocab) are skipped */
} OmkPenaltyEdits;
int omk_penalty_edits(const OmkPenaltyEdits* p, omk_stream stream);

/* ---- guided decoding: a per-row token bitmask in the row-wise sampler (added under ABI 17: additive, no existing layout changed) -------
 * New symbols and one new struct only: OmkSampleRows is what it was byte for byte, omk_sample_rows and omk_sample_rows_form keep their
 * behaviour and their values 0 / 1 / 2, so every existing caller stays valid and the version number did not move.
 * Row b carries mask_words 32-bit words at mask + b * mask_stride: bit (i & 31) of word (i >> 5) set = token i may be drawn (the format
 * grammar engines emit per step).  With e_i what ABI 14 / 16 / 17 define for token i of row b (repetition penalty, then the edits, -inf
 * for the unlisted tokens of an allow-only row), every branch sees, in every one of its passes and through the one loader:
 *   m_i = e_i    when the row is unmasked (mask_on[b] == 0) or bit i of its mask is set
 *   m_i = -inf   otherwise
 * The mask is applied LAST: a masked-out token stays -inf even when an edit entry gives it a bias, and an allow-only row draws from the
 * intersection of its list and its mask.  `logits` and `mask` are never written.  Bits at positions >= vocab are ignored.  Nothing in the
 * arrays is trusted: a mask_on[b] other than 0 counts as 1.  Inactive rows (active[b] == 0) read neither their mask row nor mask_on[b].
 * A row whose mask leaves no finite logit gives an unspecified id in [0, vocab) in bounded time (ABI 16's "a row left without a finite
 * logit").  mask == NULL: the call IS omk_sample_rows(&p->rows) -- the same plan, the same kernels, and the form function returns what
 * omk_sample_rows_form returns.  With a mask two more instantiations take the call:
 *   OMK_SAMPLE_ROWS_MASK       no penalty history and no edit list: no id map; dynamic LDS holds the row's ceil(vocab / 32) words (at most
 *                              8 192 B) next to the 44 792 B static
 *   OMK_SAMPLE_ROWS_EDIT_MASK  the ABI 16 instantiation (id map, list in whole buckets, one word) with the words behind the list; edit_cap
 *                              == 0 is legal here (a penalty history with a mask and no list).  At most 44 800 + 65 536 + 4 096 + 4 +
 *                              8 192 = 122 628 B of the 163 840 B of a workgroup
 * OMK_EINVAL: a negative mask_words or mask_stride, mask_words < ceil(vocab / 32), with more than one row mask_stride < mask_words, and
 * whatever omk_sample_rows refuses.  OMK_EUNSUPPORTED: a mask with vocab > 65 536 (one bound for everything the sampler keeps in LDS:
 * mask a copy instead), and what omk_sample_rows declines.  Capturable: nothing is read from the host, every array may be rewritten
 * between replays.                                                                                                                     */
typedef struct {
  OmkSampleRows rows;        /* everything omk_sample_rows takes, with its meaning unchanged */
  const void* mask;          /* optional device int32 (batch, mask_words): bit (i & 31) of word (i >> 5) set = token i may be drawn */
  const void* mask_on;       /* optional device int32 (batch): 0 = the row ignores its mask; NULL = every row is masked */
  int64_t mask_stride;       /* elements between the rows of mask */
  int64_t mask_words;        /* width of mask, >= ceil(vocab / 32) */
} OmkSampleRowsMasked;
int omk_sample_rows_masked(const OmkSampleRowsMasked* p, omk_stream stream);
/* Which launch omk_sample_rows_masked takes for *p: OMK_SAMPLE_ROWS_* (0 / 1 / 2 without a mask), or the negative omk_status. */
#define OMK_SAMPLE_ROWS_MASK 3       /* bit array only: no id map */
#define OMK_SAMPLE_ROWS_EDIT_MASK 4  /* id map (+ edit list) and the bit array */
int omk_sample_rows_masked_form(const OmkSampleRowsMasked* p);

#ifdef __cplusplus
}
#endif
#endif /* OMK_H */
