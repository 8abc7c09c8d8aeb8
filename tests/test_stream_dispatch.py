"""Which kernels the backward of the streaming ops launches -- causal conv1d, add + norm and gated norm: a table of calls through the C ABI
descriptors (K.Conv1dBwd, K.AddNormBwd, K.NormGatedBwd, so that no Python wrapper hides the layout) and, for each, the status of the call,
the answer of its workspace query and the exact omk_ssd_last_kernels() string -- on the emulator (the host code that chooses and launches
is the same in both builds).

Every row was recorded from the commit BEFORE conv_bwd_plan, add_bwd_plan and gated_bwd_plan (as a plan of the whole call) existed, not from
the code under test.  That commit recorded none of these kernels, so the host sections of its conv1d.hip and norms.hip got these lines, in a
scratch copy that was never committed (tn(dt) = "f32" / "bf16" / "f16"), and the case table below ran against its emulator build:

  * `kernels_reset();` as the first statement of omk_causal_conv1d_bwd, omk_add_norm_bwd and omk_norm_gated_bwd;
  * conv1d.hip: at the head of the CONV_BWD_V macro `kernels_note("conv1d_bwd_cl<t=%s,w=%d>", tn(p->x.dtype), a.W);`
    in front of the CONV_BWD_4 line `kernels_note("conv1d_bwd_cl4<t=%s,w=%d,wf=%d>", tn(p->x.dtype), a.W, (int)wf);`
    in front of the fold launch `kernels_note("conv1d_bwd_fold");`, of the generic launch `kernels_note("conv1d_bwd_generic<t=%s>", tn(p->x.dtype));`
    and of the dinit launch `kernels_note("conv1d_dinit<t=%s>", tn(p->x.dtype));`
  * norms.hip: in launch_reduce `kernels_note("reduce_parts");`
    in front of LAUNCH_B `kernels_note("add_norm_bwd<tx=%s,ts=%s,tri=%s,vec=%d,nchunk=%d,wpr=%d,grid=%d>", tn(xdt), tn(sdt), tn(ridt), plan.vec,
    plan.nchunk, plan.wpr, norm_blocks(rows, 1, plan));`
    in the gated backward `kernels_note("norm_gated_bwd_w8");`, `kernels_note("norm_gated_bwd_lean<t=%s,nchunk=%d,wpr=%d,grid=%d>", tn(p->x.dtype),
    plan.nchunk, plan.wpr, norm_blocks(rows, ng, plan));` and `kernels_note("norm_gated_bwd<t=%s,vec=%d,nchunk=%d,wpr=%d,grid=%d>", tn(p->x.dtype),
    plan.vec, plan.nchunk, plan.wpr, norm_blocks(rows, ng, plan));` in front of the three kinds of launch.

A row is (status, workspace bytes, kernel string); the query is asked on the very descriptor the call gets.

What no row reaches: the `cl` backward (conv1d_bwd_cl_kernel) is taken only when a row offset does not fit 31 bits, L * 2 * row stride >= 2^31
-- a 2 GB tensor; the workspace query answers the partial-row bytes for such a call too, although conv1d_bwd_cl_kernel uses atomics.

Some things the table shows that one might not expect: an fp32 bias 8 bytes off a 16-byte boundary keeps the short prologue (wf=1) in the
backward -- two channels per lane, one 8-byte request; the forward's kernel asks 16 (conv-bwd-cl4-bias_off8); the backward has no length
threshold (conv-bwd-cl4-L37); the workspace query of the gated backward answers max(general, w8 kernel) whichever kernel runs; the
wave-per-row plan of the norms (segments up to 1024) covers 2048 columns, so a segment it takes is never full and a group of 1024 is not
lean (gated-bwd-1024-frozen).
"""
import ctypes

import pytest
import torch

BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
_SOMEWHERE = torch.zeros(64)


def _cl(Bsz, C, L, dtype, off=8):
    """(B, C, L) channel-last view: columns off .. off + C of (B, L, off + C) rows, like xBC inside zxbcdt."""
    return torch.randn(Bsz, L, off + C).to(dtype)[:, :, off:].transpose(1, 2)


def _like(x):
    return torch.empty_like(x)      # (keeps the strides of a dense view: channel-last stays channel-last)


def _weights(C, W, weight, bias):
    """weight: 'f32' contiguous, 'bf16', or 'strided' (an fp32 view of every other column); bias: 'f32', 'off8' (fp32, 8 bytes behind a
    16-byte boundary), 'bf16' or None."""
    w = torch.randn(C, W)
    if weight == "bf16":
        w = w.bfloat16()
    elif weight == "strided":
        w = torch.randn(C, 2 * W)[:, ::2]
    b = {None: None, "f32": torch.randn(C), "bf16": torch.randn(C).bfloat16(), "off8": torch.randn(C + 2)[2:]}[bias]
    assert w.data_ptr() % 16 == 0 and (b is None or b.data_ptr() % 16 == (8 if bias == "off8" else 0))
    return w, b


def _conv_x(Bsz, C, L, dtype, layout):
    if layout == "cf":
        return torch.randn(Bsz, C, L).to(dtype)
    return _cl(Bsz, C, L, dtype, off=4 if layout == "cl4" else 8)


def _conv_bwd(lib, K, Bsz=2, C=16, L=300, W=4, dtype=BF16, layout="cl", weight="f32", bias="f32", ws=True, dinit=False):
    x = _conv_x(Bsz, C, L, dtype, layout)
    w, b = _weights(C, W, weight, bias)
    dout, dx = torch.ones_like(x), _like(x)
    dw, db = torch.zeros(C, W), (None if b is None else torch.zeros(C))
    init = torch.randn(Bsz, C, W - 1).to(dtype) if dinit else None
    di = None if init is None else torch.empty_like(init)
    p = K.Conv1dBwd(x=K.T(x), weight=K.T(w), bias=K.T(b), initial_states=K.T(init), dout=K.T(dout), dx=K.T(dx), dweight=K.T(dw), dbias=K.T(db),
                    dinitial_states=K.T(di), silu=1)
    nbytes = lib.omk_causal_conv1d_bwd_workspace_bytes(ctypes.byref(p))
    keep = K.workspace(lib, "omk_causal_conv1d_bwd_workspace_bytes", p, x) if ws else None  # noqa: F841
    return lib.omk_causal_conv1d_bwd(ctypes.byref(p), None), nbytes


def _dense(cols, dtype, misaligned, rows=3):
    """(rows, cols) with contiguous columns; misaligned: a view that starts one element behind a 16-byte boundary."""
    return torch.randn(rows, cols + 8).to(dtype)[:, 1:cols + 1] if misaligned else torch.randn(rows, cols).to(dtype)


def _add_bwd(lib, K, cols, dtype=BF16, misaligned=False, xsum=None, dweight=True, dbias=False):
    dy = _dense(cols, dtype, misaligned)
    xs = _dense(cols, xsum or dtype, misaligned)
    w, rstd, dx = torch.ones(cols), torch.ones(3), torch.empty_like(dy)
    dw, db = (torch.zeros(cols) if dweight else None), (torch.zeros(cols) if dbias else None)
    p = K.AddNormBwd(dy=K.T(dy), dresidual_out=K.T(None), xsum=K.T(xs), weight=K.T(w), rstd=K.T(rstd), mean=K.T(None), dx=K.T(dx),
                     dresidual_in=K.T(None), dweight=K.T(dw), dbias=K.T(db), is_rms_norm=1, has_bias=int(dbias))
    nbytes = lib.omk_add_norm_bwd_workspace_bytes(ctypes.byref(p))
    keep = K.workspace(lib, "omk_add_norm_bwd_workspace_bytes", p, dy)  # noqa: F841
    return lib.omk_add_norm_bwd(ctypes.byref(p), None), nbytes


def _gated_bwd(lib, K, cols, gs=0, dtype=BF16, nbg=False, dweight=True, rows=3):
    x, z, dy = (torch.randn(rows, cols).to(dtype) for _ in range(3))
    w, dx, dz, dw = torch.ones(cols), torch.empty_like(x), torch.empty_like(z), (torch.zeros(cols) if dweight else None)
    p = K.NormGatedBwd(dy=K.T(dy), x=K.T(x), z=K.T(z), weight=K.T(w), dx=K.T(dx), dz=K.T(dz), dweight=K.T(dw), group_size=gs, eps=1e-5,
                       norm_before_gate=int(nbg))
    nbytes = lib.omk_norm_gated_bwd_workspace_bytes(ctypes.byref(p))
    keep = K.workspace(lib, "omk_norm_gated_bwd_workspace_bytes", p, x)  # noqa: F841
    return lib.omk_norm_gated_bwd(ctypes.byref(p), None), nbytes


HOOK64 = {"OMK_NORM_BLOCKS": "64"}    # the test hook: at most 64 workgroups, so that a small case takes several rows per workgroup

# id -> (function, keyword arguments[, environment])
CASES = {
    # ---- conv backward
    "conv-bwd-generic-f32-cl": (_conv_bwd, dict(L=40, dtype=F32)),
    "conv-bwd-generic-bf16-cf": (_conv_bwd, dict(C=12, L=37, layout="cf")),
    "conv-bwd-cl4-W2": (_conv_bwd, dict(W=2)),
    "conv-bwd-cl4-W3": (_conv_bwd, dict(W=3)),
    "conv-bwd-cl4-W4": (_conv_bwd, dict(W=4)),
    "conv-bwd-cl4-W2-no_ws": (_conv_bwd, dict(W=2, ws=False)),
    "conv-bwd-cl4-W3-no_ws": (_conv_bwd, dict(W=3, ws=False)),
    "conv-bwd-cl4-W4-no_ws": (_conv_bwd, dict(W=4, ws=False)),
    "conv-bwd-cl4-w_bf16": (_conv_bwd, dict(weight="bf16", bias="bf16")),
    "conv-bwd-cl4-w_strided": (_conv_bwd, dict(weight="strided")),
    "conv-bwd-cl4-bias_off8": (_conv_bwd, dict(bias="off8")),                       # wf=1 here, wf=0 in conv-fwd-cl8-bias_off8
    "conv-bwd-cl4-dinit": (_conv_bwd, dict(dinit=True)),
    "conv-bwd-cl4-f16": (_conv_bwd, dict(dtype=F16)),
    "conv-bwd-cl4-L37": (_conv_bwd, dict(L=37)),                                    # (no length threshold in the backward)
    # ---- add + norm backward
    "add-bwd-512": (_add_bwd, dict(cols=512)),
    "add-bwd-2048": (_add_bwd, dict(cols=2048)),
    "add-bwd-4096": (_add_bwd, dict(cols=4096)),
    "add-bwd-8192": (_add_bwd, dict(cols=8192)),
    "add-bwd-1536": (_add_bwd, dict(cols=1536)),
    "add-bwd-100-misaligned": (_add_bwd, dict(cols=100, misaligned=True)),
    "add-bwd-8200-refused": (_add_bwd, dict(cols=8200)),
    "add-bwd-f32-xsum": (_add_bwd, dict(cols=2048, xsum=F32)),
    "add-bwd-dweight-dbias": (_add_bwd, dict(cols=2048, dbias=True)),
    "add-bwd-frozen": (_add_bwd, dict(cols=2048, dweight=False)),
    # ---- gated norm backward
    "gated-bwd-w8": (_gated_bwd, dict(cols=4096)),
    "gated-bwd-w8-frozen": (_gated_bwd, dict(cols=4096, dweight=False)),
    "gated-bwd-lean-2048": (_gated_bwd, dict(cols=2048)),
    "gated-bwd-lean-2-groups-of-4096": (_gated_bwd, dict(cols=8192, gs=4096)),
    "gated-bwd-lean-frozen": (_gated_bwd, dict(cols=2048, dweight=False)),
    "gated-bwd-1024-frozen": (_gated_bwd, dict(cols=1024, dweight=False)),
    "gated-bwd-lean-2-groups-hook64": (_gated_bwd, dict(cols=4096, gs=2048, rows=100), HOOK64),
    "gated-bwd-f32": (_gated_bwd, dict(cols=2048, dtype=F32)),
    "gated-bwd-norm_before_gate": (_gated_bwd, dict(cols=2048, nbg=True)),
    "gated-bwd-4-groups-of-64": (_gated_bwd, dict(cols=256, gs=64)),
}

def launched(case, setenv):
    """Run one case on the emulator: (the status of the call, its workspace query's answer, omk_ssd_last_kernels())."""
    from emu.loader import use_emulator
    fn, kw, env = (CASES[case] + ({},))[:3]
    for k, v in env.items():
        setenv(k, v)
    torch.manual_seed(0)
    with use_emulator() as lib:
        from omnimamba_amd import _capi as K
        rc, nbytes = fn(lib, K, **kw)
        return rc, nbytes, lib.omk_ssd_last_kernels().decode()


EXPECTED = {
    "add-bwd-100-misaligned": (0, 2400, 'add_norm_bwd<tx=bf16,ts=bf16,tri=bf16,vec=1,nchunk=32,wpr=4,grid=3>;reduce_parts'),
    "add-bwd-1536": (0, 36864, 'add_norm_bwd<tx=bf16,ts=bf16,tri=bf16,vec=8,nchunk=1,wpr=4,grid=3>;reduce_parts'),
    "add-bwd-2048": (0, 49152, 'add_norm_bwd<tx=bf16,ts=bf16,tri=bf16,vec=8,nchunk=1,wpr=4,grid=3>;reduce_parts'),
    "add-bwd-4096": (0, 98304, 'add_norm_bwd<tx=bf16,ts=bf16,tri=bf16,vec=8,nchunk=2,wpr=4,grid=3>;reduce_parts'),
    "add-bwd-512": (0, 4096, 'add_norm_bwd<tx=bf16,ts=bf16,tri=bf16,vec=8,nchunk=4,wpr=1,grid=1>;reduce_parts'),
    "add-bwd-8192": (0, 196608, 'add_norm_bwd<tx=bf16,ts=bf16,tri=bf16,vec=8,nchunk=4,wpr=4,grid=3>;reduce_parts'),
    "add-bwd-8200-refused": (-4, 0, ''),
    "add-bwd-dweight-dbias": (0, 49152, 'add_norm_bwd<tx=bf16,ts=bf16,tri=bf16,vec=8,nchunk=1,wpr=4,grid=3>;reduce_parts;reduce_parts'),
    "add-bwd-f32-xsum": (0, 49152, 'add_norm_bwd<tx=bf16,ts=f32,tri=bf16,vec=8,nchunk=1,wpr=4,grid=3>;reduce_parts'),
    "add-bwd-frozen": (0, 49152, 'add_norm_bwd<tx=bf16,ts=bf16,tri=bf16,vec=8,nchunk=1,wpr=4,grid=3>'),
    "conv-bwd-cl4-L37": (0, 640, 'conv1d_bwd_cl4<t=bf16,w=4,wf=1>;conv1d_bwd_fold'),
    "conv-bwd-cl4-W2": (0, 768, 'conv1d_bwd_cl4<t=bf16,w=2,wf=1>;conv1d_bwd_fold'),
    "conv-bwd-cl4-W2-no_ws": (0, 768, 'conv1d_bwd_cl4<t=bf16,w=2,wf=1>'),
    "conv-bwd-cl4-W3": (0, 1024, 'conv1d_bwd_cl4<t=bf16,w=3,wf=1>;conv1d_bwd_fold'),
    "conv-bwd-cl4-W3-no_ws": (0, 1024, 'conv1d_bwd_cl4<t=bf16,w=3,wf=1>'),
    "conv-bwd-cl4-W4": (0, 1280, 'conv1d_bwd_cl4<t=bf16,w=4,wf=1>;conv1d_bwd_fold'),
    "conv-bwd-cl4-W4-no_ws": (0, 1280, 'conv1d_bwd_cl4<t=bf16,w=4,wf=1>'),
    "conv-bwd-cl4-bias_off8": (0, 1280, 'conv1d_bwd_cl4<t=bf16,w=4,wf=1>;conv1d_bwd_fold'),
    "conv-bwd-cl4-dinit": (0, 1280, 'conv1d_bwd_cl4<t=bf16,w=4,wf=1>;conv1d_bwd_fold;conv1d_dinit<t=bf16>'),
    "conv-bwd-cl4-f16": (0, 1280, 'conv1d_bwd_cl4<t=f16,w=4,wf=1>;conv1d_bwd_fold'),
    "conv-bwd-cl4-w_bf16": (0, 1280, 'conv1d_bwd_cl4<t=bf16,w=4,wf=0>;conv1d_bwd_fold'),
    "conv-bwd-cl4-w_strided": (0, 1280, 'conv1d_bwd_cl4<t=bf16,w=4,wf=0>;conv1d_bwd_fold'),
    "conv-bwd-generic-bf16-cf": (0, 0, 'conv1d_bwd_generic<t=bf16>'),
    "conv-bwd-generic-f32-cl": (0, 0, 'conv1d_bwd_generic<t=f32>'),
    "gated-bwd-1024-frozen": (0, 2097152, 'norm_gated_bwd<t=bf16,vec=8,nchunk=4,wpr=1,grid=1>'),
    "gated-bwd-4-groups-of-64": (0, 524288, 'norm_gated_bwd<t=bf16,vec=8,nchunk=4,wpr=1,grid=4>;reduce_parts'),
    "gated-bwd-f32": (0, 4194304, 'norm_gated_bwd<t=f32,vec=8,nchunk=1,wpr=4,grid=3>;reduce_parts'),
    "gated-bwd-lean-2-groups-hook64": (0, 8388608, 'norm_gated_bwd_lean<t=bf16,nchunk=1,wpr=4,grid=64>;reduce_parts'),
    "gated-bwd-lean-2-groups-of-4096": (0, 16777216, 'norm_gated_bwd_lean<t=bf16,nchunk=2,wpr=4,grid=6>;reduce_parts'),
    "gated-bwd-lean-2048": (0, 4194304, 'norm_gated_bwd_lean<t=bf16,nchunk=1,wpr=4,grid=3>;reduce_parts'),
    "gated-bwd-lean-frozen": (0, 4194304, 'norm_gated_bwd_lean<t=bf16,nchunk=1,wpr=4,grid=3>'),
    "gated-bwd-norm_before_gate": (0, 4194304, 'norm_gated_bwd<t=bf16,vec=8,nchunk=1,wpr=4,grid=3>;reduce_parts'),
    "gated-bwd-w8": (0, 8388608, 'norm_gated_bwd_w8;reduce_parts'),
    "gated-bwd-w8-frozen": (0, 8388608, 'norm_gated_bwd_w8'),
}


def test_every_case_has_an_expected_row():
    assert sorted(CASES) == sorted(EXPECTED)


@pytest.mark.parametrize("case", sorted(CASES))
def test_stream_dispatch(case, monkeypatch):
    assert launched(case, monkeypatch.setenv) == EXPECTED[case]
