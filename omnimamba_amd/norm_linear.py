"""Decode-step projections fused with the normalisation in front of them (omk_norm_linear, csrc/norm_linear.hip).

At one token per sequence the reference runs `layer_norm_fn` (block.py:86-95), the task LoRA `Linear` (lora.py:185-279:
base GEMV, A GEMV, B GEMV, scale, add) and later `RMSNormGated` + `out_proj` (upstream Mamba2.step) as separate launches
of a few microseconds each; here each group is ONE kernel that streams the weight matrix once.  Inference only (no
autograd); one to eight sequences per call.  Callers fall back to the unfused ops when `applies()` says no.

Weight-only fp8 (ABI 11): `weight` may be a `torch.float8_e4m3fn` matrix with `weight_scale`, one fp32 scale per output row
(`omnimamba_amd.quant.quantize_rows_e4m3`): out = rstd * (scale[row] * sum_i decode(W[row, i]) u_i + LoRA term).  Half the bytes of a
bf16 weight stream, a quarter of an fp32 one; everything else of the call keeps the dtype of `x` (fp32 or bf16).  At two to eight sequences
under bf16 activations the codes run on the matrix pipe like a bf16 weight (ABI 12); `form(...)` tells which kernel a call takes.
"""
from __future__ import annotations

import torch

from . import _capi as K
from ._lib import get_lib, require_device, slot_indices

MAX_BATCH = 8     # sequences per call; larger decode batches take the separate ops
# what `form` answers (omk_norm_linear_form): one sequence with run-time dtypes / one sequence, uniform dtype / two to eight sequences on the
# vector pipe / two to eight sequences on the matrix pipe; a negative value is the omk_status of a call the library refuses
GENERIC, FAST, BATCHED, MATRIX = K.NL_FORM_GENERIC, K.NL_FORM_FAST, K.NL_FORM_BATCHED, K.NL_FORM_MATRIX
FORM_NAMES = {GENERIC: "generic", FAST: "fast", BATCHED: "batched", MATRIX: "matrix"}


def _uniform(weight, *others) -> bool:
    """The templated kernels' dtype rule: fp32 or bf16 weights, every other tensor of the same dtype."""
    return weight.dtype in (torch.float32, torch.bfloat16) and all(t is None or t.dtype == weight.dtype for t in others)


def _fp8_applies(x, weight, norm_weight, same_dtype, weight_scale, lora_a, group_size, residual, residual_out_dtype, z) -> bool:
    """An fp8 weight with its scale: the uniform-dtype kernels or nothing ("same dtype" = the dtype of x, fp32 or bf16).  Mirrors every
    condition under which omk_norm_linear returns OMK_EUNSUPPORTED for an fp8 weight, so that a caller who holds a master weight can decide
    BEFORE the call."""
    In = weight.shape[1] if weight.dim() == 2 else 0
    nb = 1 if x.shape[0] == 1 else (2 if x.shape[0] <= 2 else (4 if x.shape[0] <= 4 else 8))
    rdt = (torch.float32, x.dtype)
    if residual is not None:        # fp32 or the dtype of x; residual_out in the residual's dtype; no gate next to it in a batch
        if residual.dtype not in rdt or (residual_out_dtype is not None and residual_out_dtype != residual.dtype) or (z is not None and nb > 1):
            return False
    elif residual_out_dtype is not None and residual_out_dtype not in rdt:
        return False
    if any(t is not None and t.dim() == 2 and t.stride(1) != 1 for t in (lora_a, z, *same_dtype)):
        return False
    return (weight_scale is not None and weight_scale.dtype == torch.float32 and weight_scale.dim() == 1 and weight.dim() == 2
            and weight_scale.shape[0] == weight.shape[0] and weight_scale.is_contiguous()
            and norm_weight is not None and x.dtype in (torch.float32, torch.bfloat16)
            and all(t is None or t.dtype == x.dtype for t in (norm_weight, lora_a, z, *same_dtype))
            and In in (1024, 2048, 4096) and x.shape[1] == In and weight.stride(1) == 1 and weight.stride(0) % 16 == 0 and weight.data_ptr() % 16 == 0
            and x.stride(0) % 4 == 0 and x.data_ptr() % 16 == 0 and (group_size is None or group_size == In)
            and (lora_a is None or lora_a.shape[0] <= 8) and weight.shape[0] <= 64 * 1024
            and (nb == 1 or nb * In * x.element_size() <= 144 * 1024))


def applies(x: torch.Tensor, weight: torch.Tensor, norm_weight=None, *same_dtype, weight_scale=None, lora_a=None, group_size=None,
            residual=None, residual_out_dtype=None, z=None) -> bool:
    """Fused path preconditions (shape / dtype / no autograd).  One sequence: any supported dtype mix.  Two to eight
    sequences: the uniform-dtype kernel only -- pass the norm weight and every tensor that must share the weight's dtype
    (gate, LoRA factors, bias).
    An fp8 (`float8_e4m3fn`) weight needs `weight_scale` and is served by the uniform-dtype kernels only, at every batch size: the
    tensors passed must share the dtype of x (fp32 or bf16), in_features 1024 / 2048 / 4096, rows 16-byte aligned, one norm group
    (`group_size` None or in_features) and a LoRA rank of at most 8; `residual` fp32 or of x's dtype with `residual_out_dtype` equal to
    it, no gate `z` next to a residual at two or more sequences, LoRA factors with unit inner stride (`lora_a`, `residual`,
    `residual_out_dtype`, `z`: looked at for fp8 weights only -- with them, True means the library takes the call)."""
    if torch.is_grad_enabled() and (x.requires_grad or weight.requires_grad):
        return False
    if x.dim() != 2 or x.shape[0] > MAX_BATCH or x.shape[0] == 0:
        return False
    if weight.dtype == torch.float8_e4m3fn or weight_scale is not None:
        return weight.dtype == torch.float8_e4m3fn and _fp8_applies(x, weight, norm_weight, same_dtype, weight_scale, lora_a, group_size,
                                                                   residual, residual_out_dtype, z)
    vec = 4 if weight.dtype == torch.float32 else 8
    ok = (weight.dim() == 2 and weight.stride(1) == 1 and weight.shape[1] % 1024 == 0 and weight.shape[1] <= 8192
          and weight.stride(0) % vec == 0 and x.stride(0) % 4 == 0 and x.data_ptr() % 16 == 0)
    if x.shape[0] == 1:
        return ok and x.shape[1] * 4 <= 96 * 1024
    nb = 2 if x.shape[0] <= 2 else (4 if x.shape[0] <= 4 else 8)
    return (ok and norm_weight is not None and _uniform(weight, x, norm_weight, *same_dtype) and weight.shape[1] in (1024, 2048, 4096)
            and nb * weight.shape[1] * weight.element_size() <= 144 * 1024 and weight.shape[0] <= 64 * 1024)


def conv_tail_applies(x, weight, norm_weight, conv_state, conv_weight, conv_bias, lora_a=None, bias=None, residual=None, weight_scale=None) -> bool:
    """Whether `norm_linear(..., conv_state=...)` is served (the uniform-dtype kernel: fp32 or bf16 everywhere).  conv_state may be
    a pool with more rows than x has sequences (addressed through `conv_state_indices`).  An fp8 weight with its `weight_scale`: the
    one dtype is that of x."""
    if (weight.dtype == torch.float8_e4m3fn) != (weight_scale is not None):
        return False
    dt = x.dtype if weight_scale is not None else weight.dtype
    same = lambda t: t is None or t.dtype == dt
    W, S = conv_weight.shape[-1], conv_state.shape[-1]
    return (dt in (torch.float32, torch.bfloat16) and x.dtype == dt and norm_weight is not None and same(norm_weight) and same(lora_a)
            and same(bias) and same(conv_bias) and conv_state.dtype == dt and conv_weight.dtype == dt
            and (residual is None or residual.dtype in (torch.float32, dt)) and weight.shape[1] in (1024, 2048, 4096)
            and 2 <= W <= 4 and W - 1 <= S <= 4 and (lora_a is None or lora_a.shape[0] <= 8))


def norm_linear(x, weight, bias=None, *, norm_weight=None, eps=1e-5, residual=None, residual_out_dtype=None, z=None,
                group_size=None, norm_before_gate=False, lora_a=None, lora_b=None, lora_scale=0.0, out_dtype=None,
                conv_state=None, conv_weight=None, conv_bias=None, conv_offset=0, conv_silu=True, conv_state_indices=None,
                weight_scale=None, out=None, residual_out=None):
    """out = norm(x [+ residual] | gated by z) @ weight^T [+ bias] [+ lora_scale * (n @ lora_a^T) @ lora_b^T].
    x: (B, in).  Returns out, or (out, residual_out) when `residual_out_dtype` is given (residual_out = x + residual).
    conv_state (B, C, S) + conv_weight (C, W): output columns [conv_offset, conv_offset + C) additionally go through
    causal_conv1d_update (+ SiLU): out holds the convolved values and conv_state is rolled in place.
    conv_state_indices (B,) int32 (int64 is cast: one extra launch): sequence b rolls conv_state row conv_state_indices[b] of a pool
    with any number of rows; a negative index marks a padding sequence -- its conv state is neither read nor written and its conv
    columns of out are zeros.  The values are never read on the host.
    weight_scale (out,) fp32: the per-row scale of a `float8_e4m3fn` weight (required with one, refused without).
    out (B, out) / residual_out (B, in): write into these tensors instead of fresh ones (rows may be strided, e.g. column slices of a wider
    buffer; their dtypes stand in for `out_dtype` / `residual_out_dtype`)."""
    lib, p, x, out, ro = _params(x, weight, bias, norm_weight, eps, residual, residual_out_dtype, z, group_size, norm_before_gate, lora_a, lora_b,
                                 lora_scale, out_dtype, conv_state, conv_weight, conv_bias, conv_offset, conv_silu, conv_state_indices, weight_scale,
                                 out, residual_out)
    K.run(lib, "omk_norm_linear", p, x)
    return out if ro is None else (out, ro)


def form(x, weight, bias=None, *, norm_weight=None, eps=1e-5, residual=None, residual_out_dtype=None, z=None,
         group_size=None, norm_before_gate=False, lora_a=None, lora_b=None, lora_scale=0.0, out_dtype=None,
         conv_state=None, conv_weight=None, conv_bias=None, conv_offset=0, conv_silu=True, conv_state_indices=None,
         weight_scale=None, out=None, residual_out=None) -> int:
    """Which kernel `norm_linear` runs for these arguments: GENERIC, FAST, BATCHED or MATRIX, or the negative omk_status with which the
    library refuses the call.  The launch's own decision (omk_norm_linear_form); nothing is launched."""
    import ctypes
    lib, p, _, _, _ = _params(x, weight, bias, norm_weight, eps, residual, residual_out_dtype, z, group_size, norm_before_gate, lora_a, lora_b,
                              lora_scale, out_dtype, conv_state, conv_weight, conv_bias, conv_offset, conv_silu, conv_state_indices, weight_scale,
                              out, residual_out)
    return int(lib.omk_norm_linear_form(ctypes.byref(p)))


def _params(x, weight, bias, norm_weight, eps, residual, residual_out_dtype, z, group_size, norm_before_gate, lora_a, lora_b, lora_scale,
            out_dtype, conv_state, conv_weight, conv_bias, conv_offset, conv_silu, conv_state_indices, weight_scale, out=None, residual_out=None):
    """The call's descriptor and its outputs (the caller's, or freshly allocated): what `norm_linear` hands to the library and `form` asks about."""
    lib = get_lib()
    require_device(lib, x, weight, bias, norm_weight, residual, z, lora_a, lora_b, conv_state, conv_weight, conv_bias, conv_state_indices,
                   weight_scale, out, residual_out)
    if conv_state_indices is not None and conv_state is None:
        raise ValueError("conv_state_indices need conv_state")
    idx = slot_indices(conv_state_indices, x.shape[0], x.device, "conv_state_indices")
    if x.stride(-1) != 1:
        x = x.contiguous()
    if z is not None and (z.dtype != x.dtype or z.stride(-1) != 1):
        z = z.to(x.dtype).contiguous()
    B = x.shape[0]
    if out is None:
        out = torch.empty(B, weight.shape[0], dtype=out_dtype or x.dtype, device=x.device)
    ro = residual_out
    if ro is None and residual_out_dtype is not None:
        ro = torch.empty(B, x.shape[1], dtype=residual_out_dtype, device=x.device)
    p = K.NormLinear(x=K.T(x), residual=K.T(residual), z=K.T(z), norm_weight=K.T(norm_weight), weight=K.T(weight), bias=K.T(bias),
                     lora_a=K.T(lora_a), lora_b=K.T(lora_b), residual_out=K.T(ro), out=K.T(out),
                     conv_state=K.T(conv_state), conv_weight=K.T(conv_weight), conv_bias=K.T(conv_bias),
                     group_size=0 if group_size is None else int(group_size), conv_offset=int(conv_offset), eps=float(eps),
                     lora_scale=float(lora_scale), norm_before_gate=int(bool(norm_before_gate)), conv_silu=int(bool(conv_silu)),
                     conv_state_indices=K.T(idx), weight_scale=K.T(weight_scale))
    p._keep = (x, z, idx)   # (the descriptor holds raw pointers: the copies made here live as long as it does)
    return lib, p, x, out, ro
