"""Loader of the HIP C-ABI library.  There is NO fallback: when libomnimamba_hip.so is missing or a tensor is
not on a HIP device every op raises.  (The CPU test-suite injects its emulator build of the same sources through
tests/emu/loader.py -- nothing in this package knows how to find it.)"""
from __future__ import annotations

import ctypes
import os

import torch

from . import _capi

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libomnimamba_hip.so")
_LIB = None


def load(path: str = LIB_PATH) -> ctypes.CDLL:
    if not os.path.exists(path):
        raise RuntimeError(
            f"omnimamba_amd: HIP extension not built ({path} missing). Run `python -m omnimamba_amd.build` "
            "(hipcc --offload-arch=gfx950). There is no CPU or PyTorch fallback for these ops.")
    return _capi.bind(ctypes.CDLL(path))


def get_lib() -> ctypes.CDLL:
    global _LIB
    if _LIB is None:
        _LIB = load()
    return _LIB


def require_device(lib, *tensors):
    """All present tensors must live where the library executes (a HIP device for the real build)."""
    emu = bool(lib.omk_is_emulated())
    dev = None
    for t in tensors:
        if t is None:
            continue
        if emu:
            if t.is_cuda:
                raise RuntimeError("emulator build only accepts CPU tensors")
        elif not t.is_cuda:
            raise RuntimeError("omnimamba_amd ops run on the MI355X only: got a CPU tensor and there is no CPU fallback")
        if dev is None:
            dev = t.device
        elif t.device != dev:
            raise RuntimeError(f"tensors on different devices: {dev} vs {t.device}")


def forward_only_seq_lens(seq_lens, *tensors):
    """seq_lens (per-row lengths of a right-padded prefill batch) exists in the forward kernels only: a call that would record a
    backward refuses it.  Checked by the public wrappers, where the grad mode is the caller's (inside an autograd node it is off)."""
    if seq_lens is not None and torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in tensors):
        raise NotImplementedError("seq_lens is forward-only (ragged prefill): no gradient through a call that passes it")


def slot_indices(idx, batch, device, name):
    """Host checks of a slot-index tensor (state_batch_indices / conv_state_indices): 1-D, `batch` long, on `device`, int32 -- or
    int64, cast here with one extra launch.  The values are never read on the host: a step that carries them stays capturable."""
    if idx is None:
        return None
    if idx.dim() != 1 or idx.shape[0] != batch:
        raise ValueError(f"{name} must be 1-D of length {batch}, got shape {tuple(idx.shape)}")
    if idx.device != device:
        raise ValueError(f"{name} is on {idx.device}, the batch on {device}")
    if idx.dtype == torch.int64:
        idx = idx.to(torch.int32)
    elif idx.dtype != torch.int32:
        raise TypeError(f"{name} must be int32 (or int64), got {idx.dtype}")
    return idx if idx.is_contiguous() else idx.contiguous()
