"""Norm kernels (omk_add_norm_*, omk_norm_gated_*) vs the oracle: under the SIMT emulator on CPU and, with -m gpu, on the MI355X."""
import pytest
import torch

import oracle as O


def rel(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30)).item()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("cols,has_res,res32,rms", [(64, True, True, True), (520, True, False, True), (48, False, True, True), (2560, True, True, True),
                                                    (100, True, True, False), (37, False, False, True)])
def test_add_norm_fwd_bwd(dev, dtype, cols, has_res, res32, rms):
    from omnimamba_amd.layer_norm import layer_norm_fn
    torch.manual_seed(0)
    x = torch.randn(3, 5, cols).to(dtype)
    res = (torch.randn(3, 5, cols).to(torch.float32 if res32 else dtype)) if has_res else None
    w = torch.randn(cols)
    b = None if rms else torch.randn(cols)
    xr, wr = x.clone().to(dev).requires_grad_(), w.clone().to(dev).requires_grad_()
    rr = None if res is None else res.clone().to(dev).requires_grad_()
    br = None if b is None else b.clone().to(dev).requires_grad_()
    y, ro = layer_norm_fn(xr, wr, br, residual=rr, eps=1e-5, prenorm=True, residual_in_fp32=res32, is_rms_norm=rms)
    gy, gr = torch.randn(y.shape).to(y.dtype), torch.randn(ro.shape).to(ro.dtype)
    torch.autograd.backward([y, ro], [gy.to(dev), gr.to(dev)])
    y, ro = y.detach().cpu(), ro.detach().cpu()
    y0, ro0 = O.add_norm_ref(x, w, b, residual=res, eps=1e-5, prenorm=True, residual_in_fp32=res32, is_rms_norm=rms)
    tol = 1e-5 if dtype == torch.float32 else 6e-3
    assert ro.dtype == ro0.dtype and rel(ro, ro0) < tol and rel(y, y0) < tol
    # gradients: autograd through an fp64 restatement
    xd, wd = x.double().requires_grad_(), w.double().requires_grad_()
    rd = None if res is None else res.double().requires_grad_()
    bd = None if b is None else b.double().requires_grad_()
    r = xd if rd is None else xd + rd
    if rms:
        yd = r * torch.rsqrt(r.pow(2).mean(-1, keepdim=True) + 1e-5) * wd
    else:
        mu = r.mean(-1, keepdim=True)
        yd = (r - mu) * torch.rsqrt((r - mu).pow(2).mean(-1, keepdim=True) + 1e-5) * wd + bd
    torch.autograd.backward([yd, r], [gy.double(), gr.double()])
    gtol = 1e-4 if dtype == torch.float32 else 1.5e-2
    assert rel(xr.grad.cpu(), xd.grad) < gtol and rel(wr.grad.cpu(), wd.grad) < gtol
    if rr is not None:
        assert rr.grad.dtype == res.dtype and rel(rr.grad.cpu(), rd.grad) < gtol
    if br is not None:
        assert rel(br.grad.cpu(), bd.grad) < gtol


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("cols,gs,nbg,has_z", [(64, None, False, True), (128, 32, False, True), (96, 48, True, True), (40, None, False, False),
                                               (4096, None, False, True), (4608, 2304, False, True)])
def test_norm_gated(dev, dtype, cols, gs, nbg, has_z):
    from omnimamba_amd.layernorm_gated import rmsnorm_fn
    torch.manual_seed(1)
    x = torch.randn(7, cols).to(dtype)
    z = torch.randn(7, cols).to(dtype) if has_z else None
    w = torch.randn(cols)
    xr, wr = x.clone().to(dev).requires_grad_(), w.clone().to(dev).requires_grad_()
    zr = None if z is None else z.clone().to(dev).requires_grad_()
    y = rmsnorm_fn(xr, wr, None, z=zr, eps=1e-5, group_size=gs, norm_before_gate=nbg)
    gy = torch.randn(y.shape).to(y.dtype)
    y.backward(gy.to(dev))
    y = y.detach().cpu()
    y0 = O.rmsnorm_gated_ref(x, w, None, z=z, eps=1e-5, group_size=gs, norm_before_gate=nbg)
    tol = 1e-5 if dtype == torch.float32 else 6e-3
    assert rel(y, y0) < tol
    xd, wd = x.double().requires_grad_(), w.double().requires_grad_()
    zd = None if z is None else z.double().requires_grad_()
    yd = O.rmsnorm_gated_ref(xd, wd, None, z=zd, eps=1e-5, group_size=gs, norm_before_gate=nbg, compute_dtype=torch.float64)
    yd.backward(gy.double())
    gtol = 1e-4 if dtype == torch.float32 else 1.5e-2
    assert rel(xr.grad.cpu(), xd.grad) < gtol and rel(wr.grad.cpu(), wd.grad) < gtol
    if zr is not None:
        assert rel(zr.grad.cpu(), zd.grad) < gtol


@pytest.mark.parametrize("cols", [2048, 4096, 8192])
def test_norm_gated_lean_kernels_walk_several_rows_per_block(dev, monkeypatch, cols):
    """The reference's mode on full segments (bf16, gate, norm_before_gate = 0, no bias) takes the software-pipelined forward and the
    one-sigmoid backward of norms.hip; a grid capped at 64 blocks makes every block walk several rows (next-row loads in flight,
    ragged last iteration), which the 7-row cases above never do.  Same results as the general kernels (x and z rows one element into a
    wider buffer: no 16-byte rows), and the oracle's."""
    from omnimamba_amd.layernorm_gated import rmsnorm_fn
    monkeypatch.setenv("OMK_NORM_BLOCKS", "64")
    torch.manual_seed(3)
    rows = 150 if cols <= 4096 else 70
    x, z, w = torch.randn(rows, cols).bfloat16(), torch.randn(rows, cols).bfloat16(), torch.randn(cols)
    gy = torch.randn(rows, cols).bfloat16()

    def run(aligned=True):
        def rows_of(t):
            if aligned:
                return t.clone().to(dev)
            wide = torch.zeros(rows, cols + 1, dtype=t.dtype, device=dev)
            wide[:, 1:] = t.to(dev)
            return wide[:, 1:]
        xr, zr, wr = rows_of(x).requires_grad_(), rows_of(z).requires_grad_(), w.clone().to(dev).requires_grad_()
        y = rmsnorm_fn(xr, wr, None, z=zr, eps=1e-5, group_size=None, norm_before_gate=False)
        y.backward(gy.to(dev))
        return [t.detach().float().cpu() for t in (y, xr.grad, zr.grad, wr.grad)]

    lean = run()
    gen = run(aligned=False)
    for a_, b_ in zip(lean, gen):
        assert rel(a_, b_) < 3e-3
    xd, zd, wd = x.double().requires_grad_(), z.double().requires_grad_(), w.double().requires_grad_()
    yd = O.rmsnorm_gated_ref(xd, wd, None, z=zd, eps=1e-5, group_size=None, norm_before_gate=False, compute_dtype=torch.float64)
    yd.backward(gy.double())
    assert rel(lean[0], yd) < 6e-3
    for got, want in zip(lean[1:], (xd.grad, zd.grad, wd.grad)):
        assert rel(got, want) < 1.5e-2


# ---------------------------------------------------------------------------------------------------------------------------------
# Dispatch paths of omk_add_norm_fwd / _bwd and omk_norm_gated_fwd / _bwd (norms.hip: plan_vec, the wvec short-lived grid, the lean
# and w8 kernels, the partial-row fold), each selected by a case below, with the bounds of tolerances.op_bound: fp64 references from
# exactly the tensors the kernel reads (the backward's from the forward's saved residual_out / rstd / mean).
# ---------------------------------------------------------------------------------------------------------------------------------
from tolerances import op_bound  # noqa: E402


def _check(got, ref, dtype=None, what=""):
    """rel(got, ref) <= op_bound(ref, dtype of the output); returns (error, bound) for the caller's messages."""
    e, bnd = rel(got.cpu(), ref.cpu()), op_bound(ref.cpu(), got.dtype if dtype is None else dtype)
    assert e <= bnd, (what, e, bnd)
    return e, bnd


def _add_norm_bwd64(xsum, w, mean, rstd, dy, dro, rms):
    """fp64 add+norm backward from the tensors omk_add_norm_bwd reads: saved xsum (= residual_out), rstd, mean; dy; dresidual_out."""
    xs, rs = xsum.double(), rstd.double()[:, None]
    xhat = (xs if rms else xs - mean.double()[:, None]) * rs
    wdy = w.double() * dy.double()
    c1 = (xhat * wdy).mean(-1, keepdim=True)
    dx = (wdy - xhat * c1 - (0.0 if rms else wdy.mean(-1, keepdim=True))) * rs
    if dro is not None:
        dx = dx + dro.double()
    return dx, (dy.double() * xhat).sum(0), dy.double().sum(0)


_RES_MODES = {   # residual dtype, residual_in_fp32 -> the (TR, TRO) instantiation of add_norm_fwd_kernel
    "res": ("x", False),       # (TX, TX): residual in x's dtype, residual_out in x's dtype
    "res32": ("f32", True),    # (float, float): fp32 residual stream
    "none32": (None, True),    # (TX, float): no residual, residual_out fp32 (the first layer with residual_in_fp32)
    "none": (None, False),     # (TX, TX), residual_out = x itself (nothing written)
}


def _add_norm_inputs(rows, cols, dtype, mode, rms, seed):
    g = torch.Generator().manual_seed(seed)
    rdt, res32 = _RES_MODES[mode]
    x = torch.randn(rows, cols, generator=g).to(dtype)
    res = None if rdt is None else torch.randn(rows, cols, generator=g).to(torch.float32 if rdt == "f32" else dtype)
    w = torch.randn(cols, generator=g)
    b = None if rms else torch.randn(cols, generator=g)
    gy = torch.randn(rows, cols, generator=g).to(dtype)
    rodt = res.dtype if res is not None else (torch.float32 if res32 else dtype)
    gr = torch.randn(rows, cols, generator=g).to(rodt)
    return x, res, w, b, res32, gy, gr


def _add_norm_run(dev, x, res, w, b, res32, rms, gy, gr, offset=0, train_w=True):
    """One forward + backward through layer_norm_fn; weight / bias as views at element `offset` of a longer buffer (offset 1: not
    16-byte aligned, the persistent grid with scalar weight loads).  Returns outputs, gradients and the forward's saved tensors."""
    from omnimamba_amd.layer_norm import layer_norm_fn
    cols = x.shape[-1]

    def buf(t):
        if t is None:
            return None, None
        base = torch.zeros(cols + 8, dtype=t.dtype)
        base[offset:offset + cols] = t
        base = base.to(dev).requires_grad_(train_w)
        return base, base[offset:offset + cols]
    wb, wv = buf(w)
    bb, bv = buf(b)
    xr = x.clone().to(dev).requires_grad_()
    rr = None if res is None else res.clone().to(dev).requires_grad_()
    y, ro = layer_norm_fn(xr, wv, bv, residual=rr, eps=1e-5, prenorm=True, residual_in_fp32=res32, is_rms_norm=rms)
    xsum, _, _, mean, rstd = [None if t is None else t.detach().cpu() for t in y.grad_fn.saved_tensors]
    torch.autograd.backward([y, ro], [gy.to(dev), gr.to(dev)])
    grad = lambda base, t: None if base is None or base.grad is None else base.grad[offset:offset + cols].cpu()
    return dict(y=y.detach().cpu(), ro=ro.detach().cpu(), dx=xr.grad.cpu(), dres=None if rr is None else rr.grad.cpu(),
                dw=grad(wb, w), db=grad(bb, b), xsum=xsum, mean=mean, rstd=rstd)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("cols,rows,mode,rms", [
    (1024, 3, "res", True),       # {8,4,1}: cols <= 1024 -- a wave per row; 3 rows < the 4 rows of a workgroup
    (1032, 37, "res32", False),   # {8,1,4}: 1025 .. 2048, no wvec (cols != 2048); 37 rows: not a multiple of the grid
    (2048, 1, "res", True),       # {8,1,4} + wvec: cols == 2048, aligned w/b; one row
    (2048, 37, "res", False),     # {8,1,4} + wvec, (TX, TX), LayerNorm (bias through the 16-byte prologue)
    (2048, 37, "res32", True),    # {8,1,4} + wvec, (float, float)
    (2048, 37, "none32", True),   # {8,1,4} + wvec, (TX, float)
    (2048, 37, "none", False),    # {8,1,4} + wvec, no residual stream
    (2056, 5, "res32", True),     # {8,2,4}: 2049 .. 4096, no wvec
    (4096, 7, "res32", False),    # {8,2,4} + wvec: cols == 4096
    (8192, 3, "res", True),       # {8,4,4} + wvec: cols == 8192
    (8184, 2, "none32", False),   # {8,4,4}, no wvec (cols != 8192)
    (2052, 6, "res", True),       # {1,32,4}: cols % 8 != 0
])
def test_add_norm_dispatch_paths(dev, cols, rows, mode, rms, dtype):
    torch.manual_seed(0)
    x, res, w, b, res32, gy, gr = _add_norm_inputs(rows, cols, dtype, mode, rms, seed=cols + rows)
    out = _add_norm_run(dev, x, res, w, b, res32, rms, gy, gr)
    # forward vs fp64 of the kernel's inputs
    r64 = x.double() if res is None else x.double() + res.double()
    y64 = O.add_norm_ref(r64, w.double(), None if b is None else b.double(), eps=1e-5, is_rms_norm=rms,
                        compute_dtype=torch.float64)
    _check(out["y"], y64, what="y")
    _check(out["ro"], r64, what="residual_out")
    # backward vs fp64 of the tensors the backward reads
    dro = gr.to(out["xsum"].dtype)
    dx64, dw64, db64 = _add_norm_bwd64(out["xsum"], w, out["mean"], out["rstd"], gy, dro, rms)
    _check(out["dx"], dx64, what="dx")
    if out["dres"] is not None:
        _check(out["dres"], dx64, what="dresidual")
    _check(out["dw"], dw64, what="dw")
    if b is not None:
        _check(out["db"], db64, what="db")
    # the saved statistics are those of the exact sum
    v = r64 if rms else r64 - r64.mean(-1, keepdim=True)
    _check(out["rstd"], torch.rsqrt(v.pow(2).mean(-1) + 1e-5), what="rstd")
    # 16-byte-misaligned weight / bias views: the persistent grid and scalar weight loads -- the same arithmetic, the same bits
    mis = _add_norm_run(dev, x, res, w, b, res32, rms, gy, gr, offset=1)
    for k in ("y", "ro", "dx", "dres", "dw", "db", "rstd"):
        if out[k] is not None:
            assert torch.equal(out[k], mis[k]), k
    # end to end (today's bounds): autograd through an fp64 restatement from x and residual
    xd, wd = x.double().requires_grad_(), w.double().requires_grad_()
    rd = None if res is None else res.double().requires_grad_()
    bd = None if b is None else b.double().requires_grad_()
    rsum = xd if rd is None else xd + rd
    yd = O.add_norm_ref(rsum, wd, bd, eps=1e-5, is_rms_norm=rms, compute_dtype=torch.float64)
    torch.autograd.backward([yd, rsum], [gy.double(), gr.double()])
    assert rel(out["dx"], xd.grad) < 1.5e-2 and rel(out["dw"], wd.grad) < 1.5e-2
    if rd is not None:
        assert out["dres"].dtype == res.dtype and rel(out["dres"], rd.grad) < 1.5e-2


def test_add_norm_fwd_f32_residual_to_16bit_residual_out(dev):
    """(TR, TRO) = (float, TX) of add_norm_fwd_kernel on the wvec path: not reachable from layer_norm_fn (its residual_out takes the
    residual's dtype), so through the C ABI."""
    from omnimamba_amd import _capi as K
    from omnimamba_amd._lib import get_lib
    torch.manual_seed(4)
    rows, cols = 37, 2048
    x, res, w = torch.randn(rows, cols).bfloat16(), torch.randn(rows, cols), torch.randn(cols)
    xd, rd, wd = x.to(dev), res.to(dev), w.to(dev)
    y, ro = torch.empty_like(xd), torch.empty_like(xd)
    rstd = torch.empty(rows, device=dev)
    K.run(get_lib(), "omk_add_norm_fwd", K.AddNormFwd(x=K.T(xd), residual=K.T(rd), weight=K.T(wd), bias=K.T(None), y=K.T(y),
                                                     residual_out=K.T(ro), rstd=K.T(rstd), mean=K.T(None), eps=1e-5, is_rms_norm=1), xd)
    r64 = x.double() + res.double()
    _check(y.cpu(), O.add_norm_ref(r64, w.double(), None, eps=1e-5, is_rms_norm=True, compute_dtype=torch.float64), what="y")
    _check(ro.cpu(), r64, what="residual_out")


def test_add_norm_wvec_grid_walks_two_block_rows(dev, monkeypatch):
    """The short-lived grid of the wvec forward gives every workgroup two block rows once rows / rows_per_block > 2048, and an odd
    count leaves a ragged last one.  On the GPU: the real threshold (cols 2048 = one row per workgroup, 2 * 2048 + 1 rows); on the
    emulator the same loop with a 64-workgroup grid (OMK_NORM_BLOCKS).  Against fp64 and, bit for bit, the persistent grid (weight and
    bias one element into their buffers)."""
    rows = 2 * 2048 + 1 if dev.type == "cuda" else 129
    if dev.type != "cuda":
        monkeypatch.setenv("OMK_NORM_BLOCKS", "64")
    x, res, w, b, res32, gy, gr = _add_norm_inputs(rows, 2048, torch.bfloat16, "res32", False, seed=11)
    out = _add_norm_run(dev, x, res, w, b, res32, False, gy, gr)
    r64 = x.double() + res.double()
    _check(out["y"], O.add_norm_ref(r64, w.double(), b.double(), eps=1e-5, is_rms_norm=False, compute_dtype=torch.float64), what="y")
    _check(out["ro"], r64, what="residual_out")
    dx64, dw64, db64 = _add_norm_bwd64(out["xsum"], w, out["mean"], out["rstd"], gy, gr, False)
    _check(out["dx"], dx64, what="dx")
    _check(out["dw"], dw64, what="dw")
    _check(out["db"], db64, what="db")
    per = _add_norm_run(dev, x, res, w, b, res32, False, gy, gr, offset=1)   # weight / bias not 16-byte aligned: the persistent grid
    for k in ("y", "ro", "rstd", "mean"):
        assert torch.equal(out[k], per[k]), k


@pytest.mark.parametrize("rms", [True, False])
def test_add_norm_frozen_weight_and_deterministic_fold(dev, rms):
    """A frozen weight (no dweight: no partial rows, no reduction launch) leaves dx / dresidual as they are; dw / db come from the
    partial rows added up in a fixed order -- the same bits on every run."""
    x, res, w, b, res32, gy, gr = _add_norm_inputs(300, 2048, torch.bfloat16, "res", rms, seed=5)
    a1 = _add_norm_run(dev, x, res, w, b, res32, rms, gy, gr)
    a2 = _add_norm_run(dev, x, res, w, b, res32, rms, gy, gr)
    for k in ("dx", "dres", "dw", "db"):
        if a1[k] is not None:
            assert torch.equal(a1[k], a2[k]), k
    fr = _add_norm_run(dev, x, res, w, b, res32, rms, gy, gr, train_w=False)
    assert fr["dw"] is None and fr["db"] is None
    assert torch.equal(fr["dx"], a1["dx"]) and torch.equal(fr["dres"], a1["dres"]) and torch.equal(fr["y"], a1["y"])


def _gated_run(dev, x, z, w, gy, gs, train_w=True, nbg=False):
    from omnimamba_amd.layernorm_gated import rmsnorm_fn
    xr, wr = x.clone().to(dev).requires_grad_(), w.clone().to(dev).requires_grad_(train_w)
    zr = None if z is None else z.clone().to(dev).requires_grad_()
    y = rmsnorm_fn(xr, wr, None, z=zr, eps=1e-5, group_size=gs, norm_before_gate=nbg)
    y.backward(gy.to(dev))
    return dict(y=y.detach().cpu(), dx=xr.grad.cpu(), dz=None if zr is None else zr.grad.cpu(), dw=None if wr.grad is None else wr.grad.cpu())


def _gated_ref64(x, z, w, gy, gs, nbg=False):
    xd, wd = x.double().requires_grad_(), w.double().requires_grad_()
    zd = None if z is None else z.double().requires_grad_()
    yd = O.rmsnorm_gated_ref(xd, wd, None, z=zd, eps=1e-5, group_size=gs, norm_before_gate=nbg, compute_dtype=torch.float64)
    yd.backward(gy.double())
    return dict(y=yd.detach(), dx=xd.grad, dz=None if zd is None else zd.grad, dw=wd.grad)


@pytest.mark.parametrize("cols,gs,rows,dtype", [
    (4096, None, 520, torch.bfloat16),   # w8: lean (bf16, z, gate after norm, no bias), one group, cols == 4096; 520 > 512 rows: workgroups 0-7 walk two
    (4096, 2048, 37, torch.bfloat16),    # lean with two groups: {8,1,4} per 2048-column group, the general bwd grid (not w8: ng != 1)
    (2048, 1024, 9, torch.bfloat16),     # two {8,4,1} groups of 1024: not full segments (< 4 x 64 x 8), so the general kernels
    (4096, None, 37, torch.float16),     # general kernels: the lean ones are bf16 only
    (4096, 2048, 37, torch.float16),     # general kernels, two groups
    (1004, None, 5, torch.float16),      # {1,32,4}: cols % 8 != 0
])
def test_norm_gated_dispatch_paths(dev, cols, gs, rows, dtype):
    g = torch.Generator().manual_seed(cols + rows)
    x, z = torch.randn(rows, cols, generator=g).to(dtype), torch.randn(rows, cols, generator=g).to(dtype)
    w, gy = torch.randn(cols, generator=g), torch.randn(rows, cols, generator=g).to(dtype)
    out = _gated_run(dev, x, z, w, gy, gs)
    ref = _gated_ref64(x, z, w, gy, gs)
    for k in ("y", "dx", "dz", "dw"):
        _check(out[k], ref[k], what=k)
        assert rel(out[k], ref[k]) < (6e-3 if k == "y" else 1.5e-2)   # today's bounds, end to end


def test_norm_gated_frozen_weight_and_deterministic_fold(dev):
    """Frozen gated-norm weight (no partial rows, no reduction): dx / dz unchanged; dw the same bits on every run (w8 and the
    two-group lean backward)."""
    g = torch.Generator().manual_seed(8)
    for cols, gs, rows in ((4096, None, 520), (4096, 2048, 37)):
        x, z = torch.randn(rows, cols, generator=g).bfloat16(), torch.randn(rows, cols, generator=g).bfloat16()
        w, gy = torch.randn(cols, generator=g), torch.randn(rows, cols, generator=g).bfloat16()
        a1, a2 = _gated_run(dev, x, z, w, gy, gs), _gated_run(dev, x, z, w, gy, gs)
        assert torch.equal(a1["dw"], a2["dw"]) and torch.equal(a1["dx"], a2["dx"])
        fr = _gated_run(dev, x, z, w, gy, gs, train_w=False)
        assert fr["dw"] is None and torch.equal(fr["dx"], a1["dx"]) and torch.equal(fr["dz"], a1["dz"]) and torch.equal(fr["y"], a1["y"])
