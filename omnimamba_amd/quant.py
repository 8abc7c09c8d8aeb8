"""Weight-only fp8 for the decode step: OCP e4m3 copies of `in_proj` / `out_proj` with one fp32 scale per output row.

Decode streams weights: a layer-step of the 1.3B model reads 110 MB of in_proj + out_proj in fp32 and 55 MB in bf16.  The fused
decode-step projections (`norm_linear`, csrc/norm_linear.hip) take an e4m3 weight stream instead -- 27 MB -- decode it at the
multiply and apply the row's scale once, in fp32, on the reduced sum.  Activations, states, LoRA factors, norm weights, the conv
tail and the accumulation stay as they are.

It pays at every batch size the fused step serves under bf16 activations (1.3B model, MI355X): one sequence
1.226 -> 1.113 ms/token; two to eight sequences run the codes on the matrix pipe like bf16 weights (converted to bf16 operands as
they land, exact) -- per launch in_proj 18.1 -> 12.7 us and out_proj 10.9 -> 10.6 us at eight sequences, 16.6 -> 11.6 and 7.6 -> 6.3 us
at two, eight-slot MMU batching 2974 -> 3277 tokens/s.  Under fp32 activations two to eight sequences stay on the vector form, which
is no faster than fp32 weights there (33.7 against 30.9 us for in_proj at eight sequences): an fp32 server gains at one slot only.

The quantised copy accelerates the FUSED STEP ONLY.  Prefill, extend, training, the heads and every step the fused kernel does
not take (more than eight sequences, autograd on, dropout on the LoRA input) read the master weights, which stay in the model:
`state_dict()` does not change.  Nothing here is a hot path: plain torch, once per model.

    quantize_decode_weights(model)      # after the model is on its device and in its dtype; before a graph is captured
    ...decode as usual...
    clear_decode_weights(model)
"""
from __future__ import annotations

import torch

E4M3_MAX = 448.0
_Q, _S, _V = "decode_weight_q", "decode_weight_scale", "_decode_weight_version"


def quantize_rows_e4m3(w: torch.Tensor):
    """(out, in) weight -> (q float8_e4m3fn (out, in) contiguous, scale fp32 (out)) with w ~ q * scale[:, None].
    scale = absmax(row) / 448 in fp32 (all-zero rows: 1); q = clamp(w / scale, +-448) rounded to nearest even by the cast."""
    if w.dim() != 2:
        raise ValueError("quantize_rows_e4m3 takes an (out, in) matrix")
    wf = w.detach().float()
    amax = wf.abs().amax(dim=1)
    scale = torch.where(amax > 0, amax / E4M3_MAX, torch.ones_like(amax))
    q = (wf / scale[:, None]).clamp_(-E4M3_MAX, E4M3_MAX).to(torch.float8_e4m3fn).contiguous()
    return q, scale.contiguous()


def dequantize_rows(q: torch.Tensor, scale: torch.Tensor, dtype=torch.float32) -> torch.Tensor:
    """q * scale[:, None] (the operator's definition of the quantised weight), rounded to `dtype`."""
    return (q.float() * scale.float()[:, None]).to(dtype)


def _projections(model):
    """Every block's mixer.in_proj / mixer.out_proj (modules with a .mixer that has both)."""
    for m in model.modules():
        mx = getattr(m, "mixer", None)
        if mx is not None and isinstance(getattr(mx, "in_proj", None), torch.nn.Linear) and isinstance(getattr(mx, "out_proj", None), torch.nn.Linear):
            yield mx.in_proj
            yield mx.out_proj


def quantize_decode_weights(model, fmt: str = "fp8_e4m3") -> int:
    """Attach the e4m3 codes and row scales of every block's `mixer.in_proj` / `mixer.out_proj` as two non-persistent buffers
    (`state_dict()` keys do not change).  The copy remembers the master weight's `_version`: after an in-place change of the master
    the step ignores the stale copy and reads the master again (call this function again to refresh).  Call it once the model is on
    its device and in its dtype -- a later `.to(dtype)` would convert the codes, which also invalidates them -- and before a decode
    graph is captured.  Returns the number of projections quantised."""
    if fmt != "fp8_e4m3":
        raise ValueError(f"unknown decode weight format {fmt!r} (fp8_e4m3)")
    n = 0
    with torch.no_grad():
        for lin in _projections(model):
            q, s = quantize_rows_e4m3(lin.weight)
            for name, t in ((_Q, q), (_S, s)):
                if name in lin._buffers:
                    del lin._buffers[name]
                lin.register_buffer(name, t, persistent=False)
            setattr(lin, _V, lin.weight._version)
            n += 1
    return n


def clear_decode_weights(model) -> None:
    """Remove what `quantize_decode_weights` attached."""
    for m in model.modules():
        if _Q in getattr(m, "_buffers", {}):
            del m._buffers[_Q]
            del m._buffers[_S]
            m._non_persistent_buffers_set.discard(_Q)
            m._non_persistent_buffers_set.discard(_S)
            if hasattr(m, _V):
                delattr(m, _V)


def decode_weights(lin):
    """(codes, scales) of a projection when it has a quantised copy that still matches its master weight, else None."""
    q = lin._buffers.get(_Q)
    if q is None:
        return None
    s, w = lin._buffers.get(_S), lin.weight
    if (s is None or getattr(lin, _V, None) != w._version or q.dtype != torch.float8_e4m3fn or s.dtype != torch.float32
            or q.shape != w.shape or q.device != w.device or s.device != w.device):
        return None
    return q, s
