"""Weight-only fp8 decode (ABI 11): OCP e4m3 in_proj / out_proj with one fp32 scale per output row in the fused decode-step projections
(omk_norm_linear), the quantiser (omnimamba_amd/quant.py) and the module path that hands the quantised pair to the fused call.

The kernel tests compare against the fp64 composition over W_deq = q.double() * scale.double(): that IS the operator's definition, so the
tolerances are the ones tests/test_ops_norm_linear.py uses for the same kernels with exact weights -- 2e-5 (fp32 activations) / 5e-3 (bf16:
one output rounding); conv-tail outputs 3e-5 / 1e-2, rolled conv state 1e-6 / 6e-3."""
import pytest
import torch
import torch.nn.functional as F

import oracle as O

F8 = torch.float8_e4m3fn


def rel(a, b):
    return ((a.double().cpu() - b.double().cpu()).norm() / b.double().cpu().norm().clamp_min(1e-30)).item()


def make_weight(Out, In):
    """e4m3 codes of a Gaussian matrix with scales drawn in [0.5, 2) * 1e-3 (a dropped or mis-indexed scale cannot pass), and W_deq in fp64."""
    from omnimamba_amd.quant import quantize_rows_e4m3
    q, _ = quantize_rows_e4m3(torch.randn(Out, In) * 0.05)
    scale = ((torch.rand(Out) * 1.5 + 0.5) * 1e-3).float()
    return q, scale, q.float().double() * scale.double()[:, None]


def composition(x, nw, Wd, *, res=None, z=None, bias=None, la=None, lb=None, lscale=0.0, round_u=None):
    """fp64: q = (x + res) * silu(z); n = q * rstd * nw; y = n Wd^T + bias + lscale (n la^T) lb^T.  -> (y, q)"""
    q = x.double()
    if res is not None:
        q = q + res.double()
    qn = q * F.silu(z.double()) if z is not None else q
    n0 = qn * torch.rsqrt((qn * qn).mean(-1, keepdim=True) + 1e-5) * nw.double()
    if round_u is not None:
        n0 = n0.to(round_u).double()       # the batched kernel keeps u in bf16 (upstream's rounding point)
    y = n0 @ Wd.t()
    if bias is not None:
        y = y + bias.double()
    if la is not None:
        y = y + lscale * (n0 @ la.double().t()) @ lb.double().t()
    return y, q


# ---- 1. the quantiser (CPU only) -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_quantize_rows_e4m3(dtype):
    from omnimamba_amd.quant import dequantize_rows, quantize_rows_e4m3
    w = torch.randn(517, 2048) * 0.05
    w[11] = 0.0                                     # an all-zero row
    w[100, 7] = 3.0                                 # a row outlier
    w = w.to(dtype)
    q, scale = quantize_rows_e4m3(w)
    assert q.dtype == F8 and q.shape == w.shape and q.is_contiguous() and scale.dtype == torch.float32 and scale.shape == (517,)
    wf = w.float()
    assert torch.equal(scale, torch.where(wf.abs().amax(1) > 0, wf.abs().amax(1) / 448.0, torch.ones(517)))
    codes = q.view(torch.uint8)
    assert not ((codes & 0x7F) == 0x7F).any()       # no NaN code
    assert scale[11] == 1.0 and (codes[11] == 0).all()
    deq = dequantize_rows(q, scale)
    # half an ulp of a 3-bit mantissa | half a subnormal step (2^-9 / 2 of the scale); the factor covers ties and the fp32 division
    bound = torch.maximum(wf.abs().double() * 2.0 ** -4, scale.double()[:, None] * 2.0 ** -10) * (1 + 2.0 ** -20)
    err = (deq.double() - wf.double()).abs()
    print("largest error / bound:", (err / bound.clamp_min(1e-300)).max().item())
    assert (err <= bound).all()
    q2, scale2 = quantize_rows_e4m3(deq)            # a fixed point: the same bytes and the same scales
    assert torch.equal(q2.view(torch.uint8), codes) and torch.equal(scale2, scale)


# ---- 2. the decode table ---------------------------------------------------------------------------------------------------------
def test_decode_table(dev):
    """Every finite code once: row r holds the r-th finite code in column 5.  Pins subnormals, the sign and OCP against fnuz (a factor of 2
    on every normal code)."""
    from omnimamba_amd.norm_linear import norm_linear
    codes = torch.tensor([c for c in range(256) if (c & 0x7F) != 0x7F], dtype=torch.uint8)
    assert codes.numel() == 254
    qb = torch.zeros(254, 1024, dtype=torch.uint8)
    qb[:, 5] = codes
    # the value of a code, written out (bias 7, 3 mantissa bits, subnormals m * 2^-9) -- and torch's own decode agrees
    e, m = ((codes >> 3) & 15).double(), (codes & 7).double()
    val = torch.where(e == 0, m * 2.0 ** -9, (1 + m / 8) * 2.0 ** (e - 7)) * torch.where(codes >= 128, -1.0, 1.0)
    assert torch.equal(val, codes.view(F8).double())
    x = torch.zeros(1, 1024)
    x[0, 5] = 1.7
    nw = torch.rand(1024) + 0.5
    out = norm_linear(x.to(dev), qb.view(F8).to(dev), None, norm_weight=nw.to(dev), eps=1e-5, weight_scale=torch.ones(254).to(dev)).cpu()[0].double()
    ref = torch.rsqrt(x.double().pow(2).mean() + 1e-5) * nw[5].double() * 1.7 * val
    zero = val == 0
    # both zero codes give exactly zero.  (Its sign is not the code's: a row is a SUM over 1024 columns that starts at +0 and whose other
    # 1023 products are +0, and +0 + -0 = +0 under round-to-nearest -- for the fp64 composition as for the kernel.)
    assert zero.sum() == 2 and (out[zero] == 0).all()
    assert ((out[~zero] - ref[~zero]).abs() <= 2e-5 * ref[~zero].abs()).all()


# ---- 3. one sequence against the fp64 composition -------------------------------------------------------------------------------
@pytest.mark.parametrize("In,Out,dtype,rdtype,mode", [
    (2048, 333, torch.float32, torch.float32, "lora+residual"), (4096, 77, torch.float32, torch.float32, "gate"),
    (2048, 517, torch.bfloat16, torch.float32, "lora+residual"), (1024, 1000, torch.bfloat16, torch.bfloat16, "lora+gate"),
    (4096, 130, torch.bfloat16, torch.float32, "gate"),
    # the two production rows of the 1.3B model: in_proj with the conv tail (several row batches per wave where the grid is full), out_proj
    (2048, 8512, torch.bfloat16, torch.float32, "lora+residual+conv"), (4096, 2048, torch.bfloat16, None, "gate")])
def test_one_sequence(dev, In, Out, dtype, rdtype, mode):
    from omnimamba_amd.norm_linear import applies, conv_tail_applies, norm_linear
    q, scale, Wd = make_weight(Out, In)
    x, z = torch.randn(1, In).to(dtype), torch.randn(1, In).to(dtype)
    nw, bias = (torch.rand(In) + 0.5).to(dtype), torch.randn(Out).to(dtype)
    la, lb = (torch.randn(8, In) * 0.05).to(dtype), (torch.randn(Out, 8) * 0.05).to(dtype)
    kw, rk = dict(norm_weight=nw.to(dev), eps=1e-5, weight_scale=scale.to(dev)), dict(bias=bias)
    if "residual" in mode:
        res = torch.randn(1, In).to(rdtype)
        kw.update(residual=res.to(dev), residual_out_dtype=rdtype)
        rk.update(res=res)
    if "gate" in mode:
        kw.update(z=z.to(dev))
        rk.update(z=z)
    if "lora" in mode:
        kw.update(lora_a=la.to(dev), lora_b=lb.to(dev), lora_scale=4.0)
        rk.update(la=la, lb=lb, lscale=4.0)
    y0, q0 = composition(x, nw, Wd, **rk)
    assert applies(x.to(dev), q.to(dev), nw.to(dev), z.to(dev) if "gate" in mode else None, bias.to(dev), weight_scale=scale.to(dev),
                   lora_a=la.to(dev) if "lora" in mode else None)
    tol = 2e-5 if dtype == torch.float32 else 5e-3
    if "conv" in mode:
        C, off, W, S = 4352, 4096, 4, 4
        cw, cb = (torch.randn(C, W) * 0.5).to(dtype), (torch.randn(C) * 0.2).to(dtype)
        cst = torch.randn(1, S, C).to(dtype).transpose(1, 2)
        cst_d, cst0 = cst.transpose(1, 2).contiguous().to(dev).transpose(1, 2), cst.clone()      # (on the emulator .to(dev) is no copy)
        assert conv_tail_applies(x.to(dev), q.to(dev), nw.to(dev), cst_d, cw.to(dev), cb.to(dev), la.to(dev), bias.to(dev), res.to(dev), weight_scale=scale.to(dev))
        kw.update(conv_state=cst_d, conv_weight=cw.to(dev), conv_bias=cb.to(dev), conv_offset=off)
        y0 = y0.to(dtype)
        y0[:, off:off + C] = O.causal_conv1d_update_ref(y0[:, off:off + C].clone(), cst0, cw, cb, activation="silu")
        tol = 3e-5 if dtype == torch.float32 else 1e-2
    r = norm_linear(x.to(dev), q.to(dev), bias.to(dev), **kw)
    out = r[0] if "residual" in mode else r
    print("rel error:", rel(out, y0.double()), "bound", tol)
    assert out.dtype == dtype and out.shape == (1, Out) and rel(out, y0.double()) < tol
    if "residual" in mode:
        assert r[1].dtype == rdtype and rel(r[1], q0) < (1e-6 if rdtype == torch.float32 else 5e-3)
    if "conv" in mode:
        assert rel(cst_d, cst0.double()) < (1e-6 if dtype == torch.float32 else 6e-3)


# ---- 4. the conv tail over three steps -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("W,S", [(4, 4), (4, 3), (2, 1)])
def test_conv_tail(dev, dtype, W, S):
    """tests/test_ops_norm_linear.py::test_conv_tail's construction with an fp8 weight: three consecutive steps against projection +
    causal_conv1d_update_ref."""
    from omnimamba_amd.norm_linear import conv_tail_applies, norm_linear
    In, Out, C, off = 1024, 200, 120, 48
    q, scale, Wd = make_weight(Out, In)
    nw = (torch.rand(In) + 0.5).to(dtype)
    cw, cb = (torch.randn(C, W) * 0.5).to(dtype), (torch.randn(C) * 0.2).to(dtype)
    cst = torch.randn(1, S, C).to(dtype).transpose(1, 2)
    cst_d = cst.transpose(1, 2).contiguous().to(dev).transpose(1, 2)
    cst0 = cst.clone()
    for step in range(3):
        x, res = torch.randn(1, In).to(dtype), torch.randn(1, In)
        assert conv_tail_applies(x, q, nw, cst_d, cw, cb, residual=res, weight_scale=scale)
        out, ro = norm_linear(x.to(dev), q.to(dev), None, norm_weight=nw.to(dev), eps=1e-5, residual=res.to(dev), residual_out_dtype=torch.float32,
                              conv_state=cst_d, conv_weight=cw.to(dev), conv_bias=cb.to(dev), conv_offset=off, weight_scale=scale.to(dev))
        y0, q0 = composition(x, nw, Wd, res=res)
        y0 = y0.to(dtype)                                                        # zxbcdt as upstream stores it
        y0[:, off:off + C] = O.causal_conv1d_update_ref(y0[:, off:off + C].clone(), cst0, cw, cb, activation="silu")
        assert rel(ro, q0) < 1e-6
        assert rel(out, y0.double()) < (3e-5 if dtype == torch.float32 else 1e-2), step
        assert rel(cst_d, cst0.double()) < (1e-6 if dtype == torch.float32 else 6e-3), step


# ---- 5. two to eight sequences ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("In", [2048, 4096])
@pytest.mark.parametrize("mode", ["lora+conv", "gate"])
@pytest.mark.parametrize("B", [2, 3, 8])
def test_batched(dev, B, mode, In, dtype):
    """The vector form with an fp8 weight stream (u permuted in LDS, batches of at most 64 / NB rows); with the conv tail two consecutive steps."""
    from omnimamba_amd.norm_linear import applies, norm_linear
    Out, C, off, W, S = 203, 64, 16, 4, 4
    q, scale, Wd = make_weight(Out, In)
    nw, bias = (torch.rand(In) + 0.5).to(dtype), torch.randn(Out).to(dtype)
    la, lb = (torch.randn(8, In) * 0.05).to(dtype), (torch.randn(Out, 8) * 0.05).to(dtype)
    cw, cb = (torch.randn(C, W) * 0.5).to(dtype), (torch.randn(C) * 0.2).to(dtype)
    cst = torch.randn(B, S, C).to(dtype).transpose(1, 2)
    cst_d, cst0 = cst.transpose(1, 2).contiguous().to(dev).transpose(1, 2), cst.clone()
    ru = torch.bfloat16 if dtype == torch.bfloat16 else None
    for step in range(2 if "conv" in mode else 1):
        x, res, z = torch.randn(B, In).to(dtype), torch.randn(B, In), torch.randn(B, In).to(dtype)
        kw = dict(norm_weight=nw.to(dev), eps=1e-5, weight_scale=scale.to(dev))
        if mode == "gate":
            kw.update(z=z.to(dev))
            y0, q0 = composition(x, nw, Wd, z=z, bias=bias, round_u=ru)
            tol = 2e-5 if dtype == torch.float32 else 5e-3
        else:
            kw.update(residual=res.to(dev), residual_out_dtype=torch.float32, lora_a=la.to(dev), lora_b=lb.to(dev), lora_scale=4.0,
                      conv_state=cst_d, conv_weight=cw.to(dev), conv_bias=cb.to(dev), conv_offset=off)
            y0, q0 = composition(x, nw, Wd, res=res, bias=bias, la=la, lb=lb, lscale=4.0, round_u=ru)
            y0 = y0.to(dtype)
            y0[:, off:off + C] = O.causal_conv1d_update_ref(y0[:, off:off + C].clone(), cst0, cw, cb, activation="silu")
            tol = 3e-5 if dtype == torch.float32 else 1e-2
        assert applies(x.to(dev), q.to(dev), nw.to(dev), bias.to(dev), weight_scale=scale.to(dev), lora_a=la.to(dev) if "lora" in mode else None)
        r = norm_linear(x.to(dev), q.to(dev), bias.to(dev), **kw)
        out = r if mode == "gate" else r[0]
        assert out.shape == (B, Out) and out.dtype == dtype and rel(out, y0.double()) < tol, step
        for b in range(B):                          # no sequence left out or taken twice: each one on its own
            assert rel(out[b], y0[b].double()) < tol, (step, b)
        if mode != "gate":
            assert rel(r[1], q0) < 1e-6
            assert rel(cst_d, cst0.double()) < (1e-6 if dtype == torch.float32 else 6e-3), step


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_batched_conv_state_indices(dev, dtype):
    """Three sequences into a pool of six conv-state rows, the middle one a padding row (negative index): zeros in its conv columns, its
    other columns computed, no pool row touched that no sequence owns."""
    from omnimamba_amd.norm_linear import norm_linear
    B, In, Out, C, off, W, S = 3, 2048, 203, 64, 16, 4, 4
    q, scale, Wd = make_weight(Out, In)
    nw = (torch.rand(In) + 0.5).to(dtype)
    la, lb = (torch.randn(8, In) * 0.05).to(dtype), (torch.randn(Out, 8) * 0.05).to(dtype)
    cw, cb = (torch.randn(C, W) * 0.5).to(dtype), (torch.randn(C) * 0.2).to(dtype)
    pool = torch.randn(6, S, C).to(dtype).transpose(1, 2)
    pool_d, pool0 = pool.transpose(1, 2).contiguous().to(dev).transpose(1, 2), pool.clone()
    idx = torch.tensor([4, -1, 1], dtype=torch.int32)
    x, res = torch.randn(B, In).to(dtype), torch.randn(B, In)
    out, ro = norm_linear(x.to(dev), q.to(dev), None, norm_weight=nw.to(dev), eps=1e-5, residual=res.to(dev), residual_out_dtype=torch.float32,
                          lora_a=la.to(dev), lora_b=lb.to(dev), lora_scale=4.0, conv_state=pool_d, conv_weight=cw.to(dev), conv_bias=cb.to(dev),
                          conv_offset=off, conv_state_indices=idx.to(dev), weight_scale=scale.to(dev))
    y0, _ = composition(x, nw, Wd, res=res, la=la, lb=lb, lscale=4.0, round_u=torch.bfloat16 if dtype == torch.bfloat16 else None)
    y0 = y0.to(dtype)
    for b, s in ((0, 4), (2, 1)):
        y0[b:b + 1, off:off + C] = O.causal_conv1d_update_ref(y0[b:b + 1, off:off + C].clone(), pool0[s:s + 1], cw, cb, activation="silu")
    y0[1, off:off + C] = 0
    out = out.cpu()
    assert (out[1, off:off + C] == 0).all() and rel(out, y0.double()) < (3e-5 if dtype == torch.float32 else 1e-2)
    assert rel(out[1, off + C:], y0[1, off + C:].double()) < (3e-5 if dtype == torch.float32 else 1e-2)
    for s in (0, 2, 3, 5):
        assert torch.equal(pool_d[s].cpu(), pool[s])
    assert rel(pool_d, pool0.double()) < (1e-6 if dtype == torch.float32 else 6e-3)


# ---- 6. refusals -----------------------------------------------------------------------------------------------------------------
def test_refusals(dev):
    from omnimamba_amd import norm_linear as NL
    In, Out = 1024, 40
    q, scale, _ = make_weight(Out, In)
    x, nw = torch.randn(1, In), torch.rand(In) + 0.5
    with pytest.raises(RuntimeError, match="weight_scale"):          # fp8 weight without its scale: the C side says so
        NL.norm_linear(x.to(dev), q.to(dev), None, norm_weight=nw.to(dev))
    with pytest.raises(RuntimeError, match="weight_scale"):          # a scale with a bf16 weight
        NL.norm_linear(x.bfloat16().to(dev), (torch.randn(Out, In) * 0.05).bfloat16().to(dev), None, norm_weight=nw.bfloat16().to(dev),
                       weight_scale=scale.to(dev))
    with pytest.raises(RuntimeError, match="weight_scale"):          # a scale of the wrong length
        NL.norm_linear(x.to(dev), q.to(dev), None, norm_weight=nw.to(dev), weight_scale=torch.ones(Out + 1).to(dev))
    assert NL.applies(x, q, nw, weight_scale=scale)
    assert not NL.applies(x, q, nw) and not NL.applies(x, torch.randn(Out, In), nw, weight_scale=scale)
    q3, s3, _ = make_weight(Out, 3072)
    assert not NL.applies(torch.randn(1, 3072), q3, torch.ones(3072), weight_scale=s3)                      # in_features 3072
    assert not NL.applies(torch.randn(9, In), q, nw, weight_scale=scale)                                   # nine sequences
    assert not NL.applies(x, q, nw, weight_scale=scale, group_size=In // 2)                                # two norm groups
    assert not NL.applies(x, q, nw, weight_scale=scale, lora_a=torch.randn(16, In))                        # LoRA rank 16
    assert NL.applies(x, q, nw, weight_scale=scale, lora_a=torch.randn(8, In), group_size=In)
    assert not NL.applies(x.bfloat16(), q, nw, weight_scale=scale)                                         # the norm weight in another dtype than x
    # what the library would turn away because of the residual, the gate or a LoRA layout, applies() turns away too: the caller then
    # runs on its master weight
    xb, nb_ = x.bfloat16(), nw.bfloat16()
    assert NL.applies(xb, q, nb_, weight_scale=scale, residual=torch.randn(1, In), residual_out_dtype=torch.float32)
    assert not NL.applies(xb, q, nb_, weight_scale=scale, residual=torch.randn(1, In).half())             # a residual that is neither fp32 nor x's dtype
    assert not NL.applies(xb, q, nb_, weight_scale=scale, residual=torch.randn(1, In).bfloat16(), residual_out_dtype=torch.float32)
    assert not NL.applies(xb, q, nb_, weight_scale=scale, residual_out_dtype=torch.float16)
    assert not NL.applies(torch.randn(2, In), q, nw, weight_scale=scale, residual=torch.randn(2, In), z=torch.randn(2, In))   # gate + residual in a batch
    assert NL.applies(x, q, nw, weight_scale=scale, residual=torch.randn(1, In), z=torch.randn(1, In))
    assert not NL.applies(x, q, nw, torch.randn(8, Out).t(), weight_scale=scale, lora_a=torch.randn(8, In))                    # LoRA B with a strided inner dimension
    for kw_ in (dict(residual=torch.randn(1, In).half().to(dev), residual_out_dtype=torch.float16),
                dict(residual=torch.randn(1, In).bfloat16().to(dev), residual_out_dtype=torch.float32)):
        with pytest.raises(RuntimeError, match="omk_status -4"):
            NL.norm_linear(xb.to(dev), q.to(dev), None, norm_weight=nb_.to(dev), weight_scale=scale.to(dev), **kw_)
    # what applies() turns away the library refuses too (OMK_EUNSUPPORTED), it never runs the run-time-dtype kernel on fp8 codes
    with pytest.raises(RuntimeError, match="omk_status -4"):
        NL.norm_linear(x.to(dev), q.to(dev), None, norm_weight=nw.to(dev), weight_scale=scale.to(dev), group_size=In // 2)
    with pytest.raises(RuntimeError, match="omk_status -4"):
        NL.norm_linear(x.to(dev), q.to(dev), None, norm_weight=nw.to(dev), weight_scale=scale.to(dev),
                       lora_a=torch.randn(16, In).to(dev), lora_b=torch.randn(Out, 16).to(dev), lora_scale=1.0)
    with pytest.raises(RuntimeError, match="omk_status -4"):
        NL.norm_linear(torch.randn(1, 3072).to(dev), q3.to(dev), None, norm_weight=torch.ones(3072).to(dev), weight_scale=s3.to(dev))
    with pytest.raises(RuntimeError, match="omk_status -4"):
        NL.norm_linear(x.to(dev), q.to(dev), None, weight_scale=scale.to(dev))                            # no norm weight: the generic kernel's case


# ---- 7. the module step ----------------------------------------------------------------------------------------------------------
def wide_model(dev):
    """tests/test_stack_decode_train.py::test_fused_decode_step_equals_unfused's stack: wide enough for the fused kernels, non-trivial adapters."""
    from omnimamba_amd.stack import OmniMambaLM, StackConfig
    cfg = StackConfig(d_model=1024, n_layer=1, vocab_size=50, pad_vocab_size_multiple=16, vqvae_vocab_size=40, num_tokens=8,
                      t2i_positions=24, mmu_positions=40, ssm_cfg=dict(d_state=16, headdim=64, chunk_size=16), lora_dropout=0.05)
    torch.manual_seed(0)
    model = OmniMambaLM(cfg).to(dev).eval()
    with torch.no_grad():
        for blk in model.backbone.layers:
            for t in ("t2i", "mmu"):
                getattr(blk.mixer.in_proj, f"{t}_lora_B0").weight.normal_(std=0.05)
    return cfg, model


@pytest.mark.parametrize("task,Bsz", [("t2i", 1), ("mmu", 1), ("t2i", 3), ("mmu", 3)])
def test_module_step(dev, task, Bsz, monkeypatch):
    from omnimamba_amd import norm_linear as NL
    from omnimamba_amd import quant
    from omnimamba_amd.generation import InferenceParams
    cfg, model = wide_model(dev)
    with torch.no_grad():
        for blk in model.backbone.layers:       # masters on the fp8 grid: the two runs then differ by the fp32 rounding of q * scale only
            for lin in (blk.mixer.in_proj, blk.mixer.out_proj):
                lin.weight.copy_(quant.dequantize_rows(*quant.quantize_rows_e4m3(lin.weight)))
    emb = torch.randn(Bsz, 6, cfg.d_model).to(dev)
    calls = {"n": 0, "scaled": 0}
    real = NL.norm_linear

    def counting(*a, **k):
        calls["n"] += 1
        calls["scaled"] += k.get("weight_scale") is not None
        return real(*a, **k)

    monkeypatch.setattr(NL, "norm_linear", counting)

    def run(saved=None):
        """Prefill (or the states a prefill left, `saved`) + two steps -> prefill logits, step logits, ssm states, the states after the prefill."""
        ip = InferenceParams(max_seqlen=32, max_batch_size=Bsz)
        with torch.no_grad():
            if saved is None:
                o = model(None, emb, task=task, inference_params=ip, num_last_tokens=1)
                prefill = (o.t2i_logits if task == "t2i" else o.mmu_logits).clone()
                saved = {i: tuple(t.clone() for t in st) for i, st in ip.key_value_memory_dict.items()}
            else:
                prefill, ip.key_value_memory_dict = None, {i: tuple(t.clone() for t in st) for i, st in saved.items()}
            ip.seqlen_offset = 6
            ids, pos = torch.full((Bsz, 1), 3).to(dev), torch.full((Bsz, 1), 6, dtype=torch.long).to(dev)
            logits = []
            for step in range(2):
                o = model(ids, None, position_ids=pos + step, task=task, inference_params=ip, num_last_tokens=1)
                ip.seqlen_offset += 1
                logits.append(o.t2i_logits if task == "t2i" else o.mmu_logits)
        return prefill, torch.cat(logits, 1), [ip.key_value_memory_dict[i][1].clone() for i in range(cfg.n_layer)], saved

    keys = list(model.state_dict().keys())
    p0, l0, s0, _ = run()
    assert calls == {"n": 2 * cfg.n_layer * 2, "scaled": 0}
    assert quant.quantize_decode_weights(model) == 2 * cfg.n_layer
    assert list(model.state_dict().keys()) == keys
    calls.update(n=0, scaled=0)
    p1, l1, s1, saved = run()
    assert calls == {"n": 2 * cfg.n_layer * 2, "scaled": 2 * cfg.n_layer * 2}      # in_proj and out_proj, every layer, every step
    assert torch.equal(p0, p1)                                                   # the prefill reads the master weights
    assert rel(l1, l0) < 2e-5
    for a, b in zip(s1, s0):
        assert rel(a, b) < 2e-5
    # an in-place change of a master weight (a version bump) retires its copy: the step reads the master again
    with torch.no_grad():
        for blk in model.backbone.layers:
            blk.mixer.in_proj.weight.mul_(1.0)
    calls.update(n=0, scaled=0)
    _, l2, _, _ = run(saved)
    assert calls == {"n": 2 * cfg.n_layer * 2, "scaled": cfg.n_layer * 2} and rel(l2, l0) < 2e-5      # out_proj's copy is still valid
    quant.clear_decode_weights(model)
    for blk in model.backbone.layers:
        assert quant.decode_weights(blk.mixer.in_proj) is None and quant.decode_weights(blk.mixer.out_proj) is None
    assert list(model.state_dict().keys()) == keys and not any("decode_weight" in n for n, _ in model.named_buffers())


# ---- 8. captured decode ----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_quantised_decode_hipgraph_equals_eager():
    """decode() captures after quantisation: the graph replays the fp8 step, token for token what the eager loop samples."""
    from omnimamba_amd import norm_linear as NL
    from omnimamba_amd import quant
    from omnimamba_amd.generation import decode
    dev = torch.device("cuda:0")
    cfg, model = wide_model(dev)
    with torch.no_grad():
        model.backbone.img_embeddings.word_embeddings.weight.mul_(30.0)
    quant.quantize_decode_weights(model)
    ids, emb = torch.zeros(2, 5, dtype=torch.long, device=dev), torch.randn(2, 5, cfg.d_model, device=dev)
    seen, real = {"scaled": 0}, NL.norm_linear

    def counting(*a, **k):
        seen["scaled"] += k.get("weight_scale") is not None
        return real(*a, **k)

    NL.norm_linear = counting
    try:
        a = decode(ids, emb, model, 14, top_k=1, task="t2i", cg=False)
        assert seen["scaled"] > 0                                        # the eager loop ran the fp8 step
        b = decode(ids, emb, model, 14, top_k=1, task="t2i", cg=True)
        c = decode(ids, emb, model, 14, top_k=1, task="t2i", cg=True)    # replay of the cached graph
    finally:
        NL.norm_linear = real
    assert torch.equal(a, b) and torch.equal(a, c)
