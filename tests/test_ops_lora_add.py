"""omk_lora_add (result += scaling * h @ lora_B^T, in place) vs the plain composition, forward and gradients."""
import pytest
import torch


def rel(a, b):
    return ((a.double().cpu() - b.double().cpu()).norm() / b.double().cpu().norm().clamp_min(1e-30)).item()


@pytest.mark.parametrize("T,N,R,dtype", [(300, 8512, 8, torch.bfloat16), (70, 264, 16, torch.bfloat16), (33, 96, 8, torch.float32)])
def test_lora_add(dev, T, N, R, dtype):
    from omnimamba_amd import lora_add as LA
    torch.manual_seed(0)
    res, h = torch.randn(T, N).to(dtype), torch.randn(T, R).to(dtype)
    Bw = torch.randn(N, R) * 0.1
    resd = res.clone().to(dev).requires_grad_()
    hd, Bd = h.clone().to(dev).requires_grad_(), Bw.clone().to(dev).requires_grad_()
    work = resd * 1.0                                    # a non-leaf buffer the op may overwrite
    assert LA.applies(work, hd, Bd)
    out = LA.lora_add(work, hd, Bd, 4.0)
    ref = res.double() + 4.0 * h.double() @ Bw.double().t()
    tol = 2e-6 if dtype == torch.float32 else 6e-3
    assert out.dtype == dtype and rel(out, ref) < tol
    g = torch.randn(T, N).to(dtype)
    out.backward(g.to(dev))
    assert rel(resd.grad, g.double()) < 1e-6
    assert rel(hd.grad, 4.0 * g.double() @ Bw.double()) < (1e-5 if dtype == torch.float32 else 1e-2)
    assert rel(Bd.grad, 4.0 * g.double().t() @ h.double()) < (1e-5 if dtype == torch.float32 else 1e-2) and Bd.grad.dtype == torch.float32


def test_lora_add_limits(dev):
    from omnimamba_amd import lora_add as LA
    assert not LA.applies(torch.randn(4, 96), torch.randn(4, 4), torch.randn(96, 4))       # rank 4: addmm
    assert not LA.applies(torch.randn(4, 98).bfloat16(), torch.randn(4, 8).bfloat16(), torch.randn(98, 8))


@pytest.mark.parametrize("T,N,R,dtype", [(300, 2048, 8, torch.bfloat16), (70, 264, 16, torch.bfloat16), (33, 96, 8, torch.float32)])
def test_lora_add_masked(dev, T, N, R, dtype):
    """The masked form (dropout backward of the LoRA A branch): only elements whose mask byte is set receive the update."""
    from omnimamba_amd import lora_add as LA
    torch.manual_seed(1)
    out, h = torch.randn(T, N).to(dtype), torch.randn(T, R).to(dtype)
    Bw = (torch.randn(N, R) * 0.1).to(dtype)
    mask = torch.rand(T, N) < 0.8
    od = out.clone().to(dev)
    LA.lora_add_(od, h.to(dev), Bw.to(dev), 1.25, mask.to(dev))
    ref = out.double() + mask.double() * 1.25 * (h.double() @ Bw.double().t())
    assert rel(od, ref) < (2e-6 if dtype == torch.float32 else 6e-3)
    assert torch.equal(od.cpu()[~mask], out[~mask])          # untouched elements are bit-identical


@pytest.mark.parametrize("T,N", [(300, 8512), (64, 256), (1000, 520)])
def test_lora_up_bwd(dev, T, N):
    """omk_lora_up_bwd: dh = dy B and dB = dy^T h from one pass over dy, vs fp64 (ragged token tail, partial last column block)."""
    from omnimamba_amd import lora_add as LA
    torch.manual_seed(3)
    dy, h = torch.randn(T, N).bfloat16(), torch.randn(T, 8).bfloat16()
    Bw = torch.randn(N, 8) * 0.1
    assert LA.up_bwd_applies(dy.to(dev), h.to(dev), Bw.to(dev))
    dh, db = LA.lora_up_bwd(dy.to(dev), h.to(dev), Bw.to(dev))
    Bq = Bw.bfloat16().double()                      # the kernel holds lora_b as bf16 MFMA fragments
    assert dh.dtype == torch.float32 and rel(dh, dy.double() @ Bq) < 1e-5
    assert db.dtype == torch.float32 and rel(db, dy.double().t() @ h.double()) < 1e-5


def _b_view(N, R, kind, dtype, g):
    """lora_b (N, R) as the kernel may receive it: contiguous (a.bvec: 16-byte requests of the lane's weights) or a view whose rows are
    not R apart (columns of a wider tensor: a.bvec = 0, per-element loads)."""
    vals = (torch.randn(N, R, generator=g) * 0.1).to(dtype)
    if kind == "contiguous":
        return vals
    wide = torch.zeros(N, 2 * R, dtype=dtype)
    wide[:, 3:3 + R] = vals
    return wide[:, 3:3 + R]


@pytest.mark.parametrize("out_dtype", [torch.bfloat16, torch.float16, torch.float32])
@pytest.mark.parametrize("b_dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("b_kind", ["contiguous", "strided"])
def test_lora_add_b_operand_paths(dev, out_dtype, b_dtype, b_kind):
    """omk_lora_add for every lora_b form and output dtype the entry accepts: a.bvec (contiguous, aligned B rows) against the per-element
    loads of a strided view -- the same bits -- and both against fp64 (tolerances.op_bound).  T 70 x N 264: a ragged token block and a
    partial column block."""
    from omnimamba_amd import lora_add as LA
    from tolerances import op_bound
    g = torch.Generator().manual_seed(7)
    T, N, R = 70, 264, 8
    res, h = torch.randn(T, N, generator=g).to(out_dtype), torch.randn(T, R, generator=g).to(out_dtype)
    Bw = _b_view(N, R, b_kind, b_dtype, g)
    ref = res.double() + 4.0 * h.double() @ Bw.double().t()

    def run(kind):
        od = res.clone().to(dev)
        Bd = Bw.to(dev).contiguous()
        if kind != "contiguous":   # the same values, as a strided view on the device
            wide = torch.zeros(N, 2 * R, dtype=b_dtype, device=dev)
            wide[:, 3:3 + R] = Bd
            Bd = wide[:, 3:3 + R]
        assert LA.applies(od, h.to(dev), Bd)
        return LA.lora_add_(od, h.to(dev), Bd, 4.0).cpu()

    out = run(b_kind)
    e, bnd = rel(out, ref), op_bound(ref, out_dtype)
    assert out.dtype == out_dtype and e <= bnd, (e, bnd)
    assert torch.equal(run("strided" if b_kind == "contiguous" else "contiguous"), out)   # the other B operand path


def test_lora_add_fp16_autograd(dev):
    """fp16 result through the autograd node: forward by the kernel, gradients by the composition."""
    from omnimamba_amd import lora_add as LA
    from tolerances import op_bound
    torch.manual_seed(2)
    T, N, R = 70, 264, 16
    res, h, Bw = torch.randn(T, N).half(), torch.randn(T, R).half(), torch.randn(N, R) * 0.1
    resd = res.clone().to(dev).requires_grad_()
    hd, Bd = h.clone().to(dev).requires_grad_(), Bw.clone().to(dev).requires_grad_()
    work = resd * 1.0
    assert LA.applies(work, hd, Bd)
    out = LA.lora_add(work, hd, Bd, 4.0)
    ref = res.double() + 4.0 * h.double() @ Bw.double().t()
    assert out.dtype == torch.float16 and rel(out, ref) <= op_bound(ref, torch.float16)
    g = torch.randn(T, N).half()
    out.backward(g.to(dev))
    assert rel(resd.grad, g.double()) < 1e-6
    assert rel(hd.grad, 4.0 * g.double() @ Bw.double()) < 1e-2 and rel(Bd.grad, 4.0 * g.double().t() @ h.double()) < 1e-2


@pytest.mark.parametrize("b_dtype,b_kind", [(torch.bfloat16, "contiguous"), (torch.float32, "strided")])
def test_lora_up_bwd_b_operand_forms(dev, b_dtype, b_kind):
    """omk_lora_up_bwd reads lora_b in its own dtype and row stride (bf16 MFMA fragments either way): a bf16 lora_b and a strided fp32
    view give dh, dB within the bounds of test_lora_up_bwd.  fp16 dy is refused (up_bwd_applies) -- lora_ext takes two GEMMs."""
    from omnimamba_amd import lora_add as LA
    g = torch.Generator().manual_seed(9)
    T, N = 1000, 520
    dy, h = torch.randn(T, N, generator=g).bfloat16(), torch.randn(T, 8, generator=g).bfloat16()
    Bw = _b_view(N, 8, b_kind, b_dtype, g)
    if b_kind == "contiguous":
        Bd = Bw.to(dev)
    else:
        wide = torch.zeros(N, 16, dtype=b_dtype, device=dev)
        wide[:, 3:11] = Bw.to(dev)
        Bd = wide[:, 3:11]
    assert LA.up_bwd_applies(dy.to(dev), h.to(dev), Bd)
    dh, db = LA.lora_up_bwd(dy.to(dev), h.to(dev), Bd)
    Bq = Bw.bfloat16().double()
    assert rel(dh, dy.double() @ Bq) < 1e-5 and rel(db, dy.double().t() @ h.double()) < 1e-5
    assert not LA.up_bwd_applies(dy.half().to(dev), h.half().to(dev), Bd)


@pytest.mark.parametrize("adt,rank", [(torch.float16, 8), (torch.bfloat16, 4)])
def test_lora_ext_backward_when_the_kernels_refuse(dev, adt, rank):
    """The A-branch backward of lora_ext falls back to the composition where the kernels refuse: fp16 (up_bwd_applies) keeps the masked
    omk_lora_add for dx; rank 4 (applies and up_bwd_applies both refuse) takes the library GEMMs for everything.  Gradients vs fp64."""
    import types
    from omnimamba_amd import lora_add as LA
    from omnimamba_amd.lora_ext import MIN_TOKENS, lora_ext_linear
    torch.manual_seed(6)
    T, in_f, out_f = MIN_TOKENS, 64, 96
    x, W = torch.randn(T, in_f).to(adt), torch.randn(out_f, in_f) * 0.1
    A, Bw = torch.randn(rank, in_f) * 0.1, torch.randn(out_f, rank) * 0.1
    gy = torch.randn(T, out_f).to(adt)
    xr, Ar, Br = (t.clone().to(dev).requires_grad_() for t in (x, A, Bw))
    y = lora_ext_linear(types.SimpleNamespace(), xr, W.to(dev), Ar, Br, 2.0, adt, 0.0)
    h_probe = torch.zeros(T, rank, dtype=adt, device=dev)
    assert LA.up_bwd_applies(gy.to(dev), h_probe, Br) is False
    assert LA.applies(torch.zeros(T, in_f, dtype=adt, device=dev), h_probe, Ar.t().contiguous()) == (rank == 8)
    y.backward(gy.to(dev))
    xd, Ad, Bd = x.double().requires_grad_(), A.double().requires_grad_(), Bw.double().requires_grad_()
    yd = xd @ W.double().t() + 2.0 * (xd @ Ad.t()) @ Bd.t()
    yd.backward(gy.double())
    assert rel(y.detach().cpu(), yd.detach()) < 1e-2
    for got, want in ((xr.grad, xd.grad), (Ar.grad, Ad.grad), (Br.grad, Bd.grad)):
        assert rel(got.cpu(), want) < 1e-2
