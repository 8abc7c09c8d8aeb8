"""Single-token SSM state update and its multi-token extend on the MI355X (decode step of Mamba2.step).

Mirrors ``mamba_ssm.ops.triton.selective_state_update.selective_state_update``; reference reach:
/root/reference/models/stage2/generation.py:195-211,412-424 -> MixerModel.forward -> Block -> Mamba2.step.
Kernel: omk_selective_state_update (omnimamba_amd/csrc/state_update.hip), in place on ``state``, graph-capturable.
``selective_state_extend``: T tokens of a follow-up turn in one launch (omk_selective_state_extend, same file).
"""
from __future__ import annotations

import torch

from . import _capi as K
from ._lib import get_lib, require_device, slot_indices


def selective_state_update(state, x, dt, A, B, C, D=None, z=None, dt_bias=None, dt_softplus=False,
                           state_batch_indices=None):
    """state: (batch, dim, dstate) or (batch, nheads, dim, dstate), updated IN PLACE.
    x, dt, z: (batch, dim) or (batch, nheads, dim); A: (dim, dstate) or (nheads, dim, dstate);
    B, C: (batch, dstate) or (batch, ngroups, dstate); D, dt_bias: (dim) or (nheads, dim).  Returns out like x.
    state_batch_indices: optional (batch,) int32 (int64 is cast: one extra launch): row b uses state row
    state_batch_indices[b] of a pool with any number of rows; a negative index marks a padding row -- its state is neither
    read nor written and its output is zeros.  The values are never read on the host (graph-capturable)."""
    lib = get_lib()
    require_device(lib, state, x, dt, A, B, C, D, z, dt_bias, state_batch_indices)
    idx = slot_indices(state_batch_indices, x.shape[0], x.device, "state_batch_indices")
    has_heads = state.dim() > 3
    if not has_heads:
        state_v, x_v, dt_v, A_v = state.unsqueeze(1), x.unsqueeze(1), dt.unsqueeze(1), A.unsqueeze(0)
        B_v, C_v = (B.unsqueeze(1) if B.dim() == 2 else B), (C.unsqueeze(1) if C.dim() == 2 else C)
        D_v = None if D is None else D.unsqueeze(0)
        z_v = None if z is None else z.unsqueeze(1)
        tb_v = None if dt_bias is None else dt_bias.unsqueeze(0)
    else:
        state_v, x_v, dt_v, A_v, B_v, C_v, D_v, z_v, tb_v = state, x, dt, A, B, C, D, z, dt_bias
    if B_v.dtype != x_v.dtype:
        B_v = B_v.to(x_v.dtype)
    if C_v.dtype != x_v.dtype:
        C_v = C_v.to(x_v.dtype)
    if z_v is not None and z_v.dtype != x_v.dtype:
        z_v = z_v.to(x_v.dtype)
    out = torch.empty_like(x_v)
    if x_v.numel() > 0:
        p = K.StateUpdate(state=K.T(state_v), x=K.T(x_v), dt=K.T(dt_v), A=K.T(A_v), Bm=K.T(B_v), Cm=K.T(C_v), D=K.T(D_v),
                          z=K.T(z_v), dt_bias=K.T(tb_v), out=K.T(out), dt_softplus=int(dt_softplus), state_batch_indices=K.T(idx))
        K.run(lib, "omk_selective_state_update", p, x_v)
    return out if has_heads else out.squeeze(1)


def selective_state_extend(state, x, dt, A, B, C, D=None, z=None, dt_bias=None, dt_softplus=False, state_batch_indices=None,
                           seq_lens=None):
    """T tokens of one turn applied to a cached state in one launch (omk_selective_state_extend): what T successive
    ``selective_state_update`` calls do, with the state read once, kept in fp32 and stored once.
    state: (batch, nheads, dim, dstate), updated IN PLACE; x, z: (batch, T, nheads, dim); dt: (batch, T, nheads[, dim]);
    A: (nheads[, dim, dstate]); B, C: (batch, T, ngroups, dstate); D, dt_bias: (nheads[, dim]).  Returns out like x.
    state_batch_indices: as in ``selective_state_update`` -- row b extends pool row state_batch_indices[b], a negative index is a
    padding row (no state traffic, zero outputs).
    seq_lens: optional (batch,) int32 (int64 is cast), the rows of a right-padded batch of turns: row b applies its first
    clamp(seq_lens[b], 0, T) tokens only -- state and out[b, :n_b] bit-identical to a call on that row alone with T = n_b, out[b, n_b:]
    zeros, a row of length 0 leaves its state untouched.  The values are never read on the host (graph-capturable)."""
    lib = get_lib()
    require_device(lib, state, x, dt, A, B, C, D, z, dt_bias, state_batch_indices, seq_lens)
    if state.dim() != 4 or x.dim() != 4:
        raise ValueError("selective_state_extend: state (batch, nheads, dim, dstate) and x (batch, T, nheads, dim)")
    idx = slot_indices(state_batch_indices, x.shape[0], x.device, "state_batch_indices")
    lens = slot_indices(seq_lens, x.shape[0], x.device, "seq_lens")
    H, P, N = state.shape[1:]
    # per-head parameters as stride-0 expansions (the kernel's tied form)
    dt_v = dt[..., None].expand(*dt.shape, P) if dt.dim() == 3 else dt
    A_v = A[:, None, None].expand(H, P, N) if A.dim() == 1 else A
    D_v = D[:, None].expand(H, P) if (D is not None and D.dim() == 1) else D
    tb_v = dt_bias[:, None].expand(H, P) if (dt_bias is not None and dt_bias.dim() == 1) else dt_bias
    B_v = B if B.dtype == x.dtype else B.to(x.dtype)
    C_v = C if C.dtype == x.dtype else C.to(x.dtype)
    z_v = z if (z is None or z.dtype == x.dtype) else z.to(x.dtype)
    out = torch.empty_like(x)
    if x.numel() > 0:
        p = K.StateExtend(state=K.T(state), x=K.T(x), dt=K.T(dt_v), A=K.T(A_v), Bm=K.T(B_v), Cm=K.T(C_v), D=K.T(D_v), z=K.T(z_v),
                          dt_bias=K.T(tb_v), out=K.T(out), dt_softplus=int(dt_softplus), state_batch_indices=K.T(idx),
                          seq_lens=K.T(lens))
        K.run(lib, "omk_selective_state_extend", p, x)
    return out
