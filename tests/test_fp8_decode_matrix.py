"""fp8 (e4m3) decode weights on the matrix pipe at two to eight sequences (ABI 12): norm_linear_mfma_kernel with an fp8 weight stream under
bf16 activations, the one selector behind omk_norm_linear and its query omk_norm_linear_form (`norm_linear.form`).

The kernel tests use tests/test_fp8_decode.py's weights (random row scales in [0.5, 2) * 1e-3: a dropped or mis-indexed scale cannot pass) and
its fp64 composition over W_deq = q * scale with u rounded to bf16, the kernel's own rounding point.  e4m3 -> bf16 is exact and the products
and sums are fp32, so the tolerances are those of the same kernel with exact bf16 weights (tests/test_ops_norm_linear.py, test_fp8_decode.py):
outputs 5e-3, conv-tail outputs 1e-2, rolled conv state 6e-3, residual_out 1e-6, each also per sequence; where a workgroup walks several tiles
the largest absolute error stays under 0.08 as in test_batched_matrix_form_walks_several_tiles_per_workgroup (a row or sequence left out or
taken twice is an error of the size of the output itself)."""
import copy

import pytest
import torch

import oracle as O
from test_fp8_decode import F8, composition, make_weight, rel, wide_model

BF = torch.bfloat16


def _call_kw(dev, B, In, Out, mode, rdtype, q, scale, *, conv=None, bias=None, lora=None, nw_scale=1.0):
    """One set of inputs for a bf16 call in `mode`: -> (x, kwargs of norm_linear on `dev`, kwargs of composition)."""
    x = torch.randn(B, In).to(BF)
    nw = ((torch.rand(In) + 0.5) * nw_scale).to(BF)
    kw, rk = dict(norm_weight=nw.to(dev), eps=1e-5, weight_scale=scale.to(dev)), dict(bias=bias, round_u=BF)
    if "residual" in mode:
        res = torch.randn(B, In).to(rdtype)
        kw.update(residual=res.to(dev), residual_out_dtype=rdtype)
        rk.update(res=res)
    if "gate" in mode:
        z = torch.randn(B, In).to(BF)
        kw.update(z=z.to(dev))
        rk.update(z=z)
        if rdtype == torch.float32:
            kw.update(residual_out_dtype=rdtype)      # (the gated kernels write no residual_out: only the dispatch looks at the type)
    if "lora" in mode:
        la, lb = lora
        kw.update(lora_a=la.to(dev), lora_b=lb.to(dev), lora_scale=4.0)
        rk.update(la=la, lb=lb, lscale=4.0)
    if conv is not None:
        kw.update(conv_state=conv["state"], conv_weight=conv["w"].to(dev), conv_bias=conv["b"].to(dev), conv_offset=conv["off"])
    return x, nw, kw, rk


def _run_mode(dev, B, In, Out, mode, rdtype, *, C=64, off=16, W=4, S=4, maxabs=None, nw_scale=1.0):
    """The fp8 matrix form against the composition: `lora+residual+conv` over two consecutive steps, `gate` once."""
    from omnimamba_amd import norm_linear as NL
    q, scale, Wd = make_weight(Out, In)
    bias = torch.randn(Out).to(BF)
    lora = ((torch.randn(8, In) * 0.05).to(BF), (torch.randn(Out, 8) * 0.05).to(BF))
    conv = None
    if "conv" in mode:
        cw, cb = (torch.randn(C, W) * 0.5).to(BF), (torch.randn(C) * 0.2).to(BF)
        cst = torch.randn(B, S, C).to(BF).transpose(1, 2)
        cst_d, cst0 = cst.transpose(1, 2).contiguous().to(dev).transpose(1, 2), cst.clone()
        conv = dict(state=cst_d, w=cw, b=cb, off=off)
    for step in range(2 if conv else 1):
        x, nw, kw, rk = _call_kw(dev, B, In, Out, mode, rdtype, q, scale, conv=conv, bias=bias, lora=lora, nw_scale=nw_scale)
        y0, q0 = composition(x, nw, Wd, **rk)
        tol = 5e-3
        if conv:
            y0 = y0.to(BF)
            y0[:, off:off + C] = O.causal_conv1d_update_ref(y0[:, off:off + C].clone(), cst0, cw, cb, activation="silu")
            tol = 1e-2
        assert NL.form(x.to(dev), q.to(dev), bias.to(dev), **kw) == NL.MATRIX
        r = NL.norm_linear(x.to(dev), q.to(dev), bias.to(dev), **kw)
        out = r[0] if isinstance(r, tuple) else r
        err = rel(out, y0.double())
        amax = float((out.double().cpu() - y0.double()).abs().max())
        print(f"B {B} In {In} Out {Out} {mode} step {step}: rel {err:.3e} (bound {tol}), max abs {amax:.4f}")
        assert out.shape == (B, Out) and out.dtype == BF and err < tol, step
        for b in range(B):                          # no sequence left out or taken twice: each one on its own
            assert rel(out[b], y0[b].double()) < tol, (step, b)
        if maxabs is not None:
            assert amax < maxabs, step
        if "residual" in mode:
            assert r[1].dtype == rdtype and rel(r[1], q0) < (1e-6 if rdtype == torch.float32 else 5e-3)
        if conv:
            assert rel(cst_d, cst0.double()) < 6e-3, step


# ---- 1. the form query -------------------------------------------------------------------------------------------------------------
def test_form(dev):
    from omnimamba_amd import norm_linear as NL
    Out = 40
    for In in (1024, 2048, 4096):
        q, scale, _ = make_weight(Out, In)
        nw = torch.rand(In) + 0.5
        la, lb = torch.randn(8, In) * 0.05, torch.randn(Out, 8) * 0.05
        for B in (2, 3, 8):
            x, z = torch.randn(B, In), torch.randn(B, In)
            for extra in (dict(), dict(lora_a=la, lora_b=lb, lora_scale=2.0), dict(z=z)):
                kb = {k: (v.to(BF).to(dev) if torch.is_tensor(v) else v) for k, v in extra.items()}
                kf = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in extra.items()}
                same16 = [v for k, v in kb.items() if k in ("z", "lora_b")]
                same32 = [v for k, v in kf.items() if k in ("z", "lora_b")]
                assert NL.form(x.to(BF).to(dev), q.to(dev), None, norm_weight=nw.to(BF).to(dev), weight_scale=scale.to(dev), **kb) == NL.MATRIX, (In, B, list(extra))
                assert NL.applies(x.to(BF).to(dev), q.to(dev), nw.to(BF).to(dev), *same16, weight_scale=scale.to(dev), lora_a=kb.get("lora_a"))
                # fp8 under fp32 activations stays on the vector form
                assert NL.form(x.to(dev), q.to(dev), None, norm_weight=nw.to(dev), weight_scale=scale.to(dev), **kf) == NL.BATCHED, (In, B, list(extra))
                assert NL.applies(x.to(dev), q.to(dev), nw.to(dev), *same32, weight_scale=scale.to(dev), lora_a=kf.get("lora_a"))
        for dt in (torch.float32, BF):              # one sequence: the uniform-dtype batch-1 kernel
            assert NL.form(torch.randn(1, In).to(dt).to(dev), q.to(dev), None, norm_weight=nw.to(dt).to(dev), weight_scale=scale.to(dev)) == NL.FAST
    In = 1024
    q, scale, _ = make_weight(Out, In)
    nw = torch.rand(In) + 0.5
    wb = (torch.randn(Out, In) * 0.05).to(BF)
    assert NL.form(torch.randn(2, In).to(BF).to(dev), wb.to(dev), None, norm_weight=nw.to(BF).to(dev)) == NL.MATRIX        # a bf16 weight
    assert NL.form(torch.randn(1, In).to(dev), torch.randn(Out, In).half().to(dev), None, norm_weight=nw.to(dev)) == NL.GENERIC  # mixed dtypes
    # what tests/test_fp8_decode.py::test_refusals lists: a negative status, and applies() says the same
    q3, s3, _ = make_weight(Out, 3072)
    x = torch.randn(1, In)
    refused = [
        (dict(x=torch.randn(1, 3072), weight=q3, norm_weight=torch.ones(3072), weight_scale=s3), dict()),                  # 3072 features
        (dict(x=torch.randn(9, In), weight=q, norm_weight=nw, weight_scale=scale), dict()),                                # nine sequences
        (dict(x=x, weight=q, norm_weight=nw, weight_scale=scale, lora_a=torch.randn(16, In), lora_b=torch.randn(Out, 16), lora_scale=1.0), dict()),
        (dict(x=x, weight=q, norm_weight=nw, weight_scale=scale, group_size=In // 2), dict())]                             # two norm groups
    for kw, _ in refused:
        kw = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in kw.items()}
        f = NL.form(kw.pop("x"), kw.pop("weight"), None, **kw)
        assert f < 0, f
    assert not NL.applies(torch.randn(1, 3072), q3, torch.ones(3072), weight_scale=s3)
    assert not NL.applies(torch.randn(9, In), q, nw, weight_scale=scale)
    assert not NL.applies(x, q, nw, weight_scale=scale, lora_a=torch.randn(16, In))
    assert not NL.applies(x, q, nw, weight_scale=scale, group_size=In // 2)
    assert NL.applies(x, q, nw, weight_scale=scale) and NL.form(x.to(dev), q.to(dev), None, norm_weight=nw.to(dev), weight_scale=scale.to(dev)) >= 0


# ---- 2. the decode table through the matrix form ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("col", [13, 645])   # position mod 16: 13 (the lane's second fragment), 5 (its first)
def test_decode_table_matrix_form(dev, col):
    """All 254 finite codes once, at two sequences in bf16: row r holds the r-th finite code in column `col`, whose position mod 16 says which
    of the lane's two A fragments carries it.  Zero codes give exactly 0; every other element is within one bf16 output rounding (2^-8
    relative, times 1 + 2^-10 for the fp32 rstd) of the fp64 value over u = bf16(x * norm_weight)."""
    from omnimamba_amd import norm_linear as NL
    assert col % 16 == (13 if col == 13 else 5)
    codes = torch.tensor([c for c in range(256) if (c & 0x7F) != 0x7F], dtype=torch.uint8)
    qb = torch.zeros(254, 1024, dtype=torch.uint8)
    qb[:, col] = codes
    e, m = ((codes >> 3) & 15).double(), (codes & 7).double()
    val = torch.where(e == 0, m * 2.0 ** -9, (1 + m / 8) * 2.0 ** (e - 7)) * torch.where(codes >= 128, -1.0, 1.0)
    assert torch.equal(val, codes.view(F8).double())
    x = torch.zeros(2, 1024)
    x[0, col], x[1, col] = 1.7, -0.3
    x, nw = x.to(BF), (torch.rand(1024) + 0.5).to(BF)
    kw = dict(norm_weight=nw.to(dev), eps=1e-5, weight_scale=torch.ones(254).to(dev))
    assert NL.form(x.to(dev), qb.view(F8).to(dev), None, **kw) == NL.MATRIX
    out = NL.norm_linear(x.to(dev), qb.view(F8).to(dev), None, **kw).cpu().double()
    u = (x.double() * nw.double()).to(BF).double()[:, col]                                     # the kernel's u: un-normalised, rounded to bf16
    rstd = torch.rsqrt(x.double().pow(2).mean(-1) + 1e-5)
    ref = (rstd * u)[:, None] * val[None, :]
    zero = (val == 0)[None, :].expand(2, -1)
    assert zero.sum() == 4 and (out[zero] == 0).all()
    bound = 2.0 ** -8 * (1 + 2.0 ** -10) * ref.abs()
    worst = ((out - ref).abs() / ref.abs().clamp_min(1e-300))[~zero].max().item()
    print("largest relative error:", worst, "bound", 2.0 ** -8 * (1 + 2.0 ** -10))
    assert ((out - ref).abs() <= bound)[~zero].all()


# ---- 3. shapes where the kernel can go wrong ---------------------------------------------------------------------------------------------
# Out = 203: a ragged last tile; fewer 16-row tiles than workgroups, so tiles of 8 rows.  1024 features: 256 threads; 2048 / 4096: 512.
_TR_BF16 = {(2, 1024), (3, 2048), (8, 4096)}        # the cases that also run with a bf16 residual / without residual_out in front of the gate


@pytest.mark.parametrize("In", [1024, 2048, 4096])
@pytest.mark.parametrize("B", [2, 3, 5, 8])
def test_lora_residual_conv_two_steps(dev, B, In):
    _run_mode(dev, B, In, 203, "lora+residual+conv", torch.float32)
    if (B, In) in _TR_BF16:
        _run_mode(dev, B, In, 203, "lora+residual+conv", BF)


@pytest.mark.parametrize("In", [1024, 2048, 4096])
@pytest.mark.parametrize("B", [2, 3, 5, 8])
def test_gate(dev, B, In):
    _run_mode(dev, B, In, 203, "gate", BF)
    if (B, In) in _TR_BF16:
        _run_mode(dev, B, In, 203, "gate", torch.float32)


@pytest.mark.parametrize("wgs,B,In", [(1, 2, 1024), (3, 3, 1024), (4, 5, 1024), (3, 5, 2048), (1, 8, 2048), (4, 8, 4096), (3, 2, 4096), (4, 3, 2048)])
def test_several_tiles_per_workgroup(dev, wgs, B, In, monkeypatch):
    """13 tiles of 16 rows (Out = 200) on 1 / 3 / 4 workgroups: odd and even tile counts per workgroup, more tiles than the four sets of
    weights in flight (13 on one workgroup, 5 on the first of three), workgroups that stop after one, three or four tiles.
    The 0.08 of test_batched_matrix_form_walks_several_tiles_per_workgroup is one bf16 step of an output below 16 (0.0625) and a margin; its
    outputs stay below 16.  make_weight's random row scales make W_deq about 3.4 times its Gaussian (1.25e-3 against absmax / 448 = 3.7e-4), so
    the norm weight is scaled by 1 / 4 here: outputs of that test's size, for which the bound was set -- a row or sequence left out or taken
    twice is still an error of several units."""
    monkeypatch.setenv("OMK_NL_MFMA_WGS", str(wgs))
    torch.manual_seed(3)
    _run_mode(dev, B, In, 200, "lora+residual+conv", torch.float32, C=100, off=60, S=3, maxabs=0.08, nw_scale=0.25)
    _run_mode(dev, B, In, 200, "gate", BF, maxabs=0.08, nw_scale=0.25)


@pytest.mark.parametrize("B,In", [(2, 1024), (5, 2048), (8, 4096)])
def test_fewer_rows_than_a_tile(dev, B, In):
    _run_mode(dev, B, In, 8, "lora+residual+conv", torch.float32, C=4, off=2)
    _run_mode(dev, B, In, 8, "gate", BF)


def test_conv_state_indices(dev):
    """Three sequences into a pool of six conv-state rows, the middle one a padding row: zeros in its conv columns, its other columns
    computed, untouched pool rows bit-equal."""
    from omnimamba_amd import norm_linear as NL
    B, In, Out, C, off, W, S = 3, 2048, 203, 64, 16, 4, 4
    q, scale, Wd = make_weight(Out, In)
    nw = (torch.rand(In) + 0.5).to(BF)
    la, lb = (torch.randn(8, In) * 0.05).to(BF), (torch.randn(Out, 8) * 0.05).to(BF)
    cw, cb = (torch.randn(C, W) * 0.5).to(BF), (torch.randn(C) * 0.2).to(BF)
    pool = torch.randn(6, S, C).to(BF).transpose(1, 2)
    pool_d, pool0 = pool.transpose(1, 2).contiguous().to(dev).transpose(1, 2), pool.clone()
    idx = torch.tensor([4, -1, 1], dtype=torch.int32)
    x, res = torch.randn(B, In).to(BF), torch.randn(B, In)
    kw = dict(norm_weight=nw.to(dev), eps=1e-5, residual=res.to(dev), residual_out_dtype=torch.float32, lora_a=la.to(dev), lora_b=lb.to(dev),
              lora_scale=4.0, conv_state=pool_d, conv_weight=cw.to(dev), conv_bias=cb.to(dev), conv_offset=off, conv_state_indices=idx.to(dev),
              weight_scale=scale.to(dev))
    assert NL.form(x.to(dev), q.to(dev), None, **kw) == NL.MATRIX
    out, ro = NL.norm_linear(x.to(dev), q.to(dev), None, **kw)
    y0, q0 = composition(x, nw, Wd, res=res, la=la, lb=lb, lscale=4.0, round_u=BF)
    y0 = y0.to(BF)
    for b, s in ((0, 4), (2, 1)):
        y0[b:b + 1, off:off + C] = O.causal_conv1d_update_ref(y0[b:b + 1, off:off + C].clone(), pool0[s:s + 1], cw, cb, activation="silu")
    y0[1, off:off + C] = 0
    out = out.cpu()
    assert (out[1, off:off + C] == 0).all() and rel(out, y0.double()) < 1e-2 and rel(ro, q0) < 1e-6
    assert rel(out[1, off + C:], y0[1, off + C:].double()) < 1e-2 and rel(out[1, :off], y0[1, :off].double()) < 1e-2
    for s in (0, 2, 3, 5):
        assert torch.equal(pool_d[s].cpu(), pool[s])
    assert rel(pool_d, pool0.double()) < 6e-3


# ---- 4. agreement with the vector form -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,In,mode", [(2, 2048, "lora+residual"), (8, 4096, "gate"), (5, 1024, "lora+residual")])
def test_matrix_and_vector_form_agree_with_the_composition(dev, B, In, mode):
    """The same fp8 call on the matrix form (bf16 activations) and on the vector form (fp32 activations holding the same bf16 values).  The two
    are not bit-comparable (u in bf16 / fp32, bf16 / fp32 output): each is held against ONE fp64 composition, u rounded in neither."""
    from omnimamba_amd import norm_linear as NL
    Out = 203
    q, scale, Wd = make_weight(Out, In)
    x, z, res = torch.randn(B, In).to(BF), torch.randn(B, In).to(BF), torch.randn(B, In)
    nw, bias = (torch.rand(In) + 0.5).to(BF), torch.randn(Out).to(BF)
    la, lb = (torch.randn(8, In) * 0.05).to(BF), (torch.randn(Out, 8) * 0.05).to(BF)
    rk = dict(bias=bias)
    if "gate" in mode:
        rk.update(z=z)
    else:
        rk.update(res=res, la=la, lb=lb, lscale=4.0)
    y0, _ = composition(x, nw, Wd, **rk)
    outs = {}
    for dt in (BF, torch.float32):
        kw = dict(norm_weight=nw.to(dt).to(dev), eps=1e-5, weight_scale=scale.to(dev))
        if "gate" in mode:
            kw.update(z=z.to(dt).to(dev))
        else:
            kw.update(residual=res.to(dev), residual_out_dtype=torch.float32, lora_a=la.to(dt).to(dev), lora_b=lb.to(dt).to(dev), lora_scale=4.0)
        assert NL.form(x.to(dt).to(dev), q.to(dev), bias.to(dt).to(dev), **kw) == (NL.MATRIX if dt == BF else NL.BATCHED)
        r = NL.norm_linear(x.to(dt).to(dev), q.to(dev), bias.to(dt).to(dev), **kw)
        outs[dt] = r[0] if isinstance(r, tuple) else r
    e16, e32 = rel(outs[BF], y0), rel(outs[torch.float32], y0)
    print(f"matrix form (bf16) {e16:.3e} (bound 5e-3), vector form (fp32) {e32:.3e} (bound 2e-5)")
    assert e16 < 5e-3 and e32 < 2e-5
    for b in range(B):
        assert rel(outs[BF][b], y0[b]) < 5e-3 and rel(outs[torch.float32][b], y0[b]) < 2e-5, b


# ---- 5. the module step ------------------------------------------------------------------------------------------------------------------
def _module_run(model, cfg, emb, Bsz, task="mmu"):
    """Prefill + two steps -> (prefill logits, step logits)."""
    from omnimamba_amd.generation import InferenceParams
    dev = emb.device
    ip = InferenceParams(max_seqlen=32, max_batch_size=Bsz)
    with torch.no_grad():
        o = model(None, emb, task=task, inference_params=ip, num_last_tokens=1)
        prefill = (o.t2i_logits if task == "t2i" else o.mmu_logits).clone()
        ip.seqlen_offset = emb.shape[1]
        ids, pos = torch.full((Bsz, 1), 3).to(dev), torch.full((Bsz, 1), emb.shape[1], dtype=torch.long).to(dev)
        logits = []
        for step in range(2):
            o = model(ids, None, position_ids=pos + step, task=task, inference_params=ip, num_last_tokens=1)
            ip.seqlen_offset += 1
            logits.append(o.t2i_logits if task == "t2i" else o.mmu_logits)
    return prefill, torch.cat(logits, 1)


def test_module_step_bf16(dev, monkeypatch):
    """The quantised bf16 model at three sequences: every fused call carries weight_scale and takes the matrix form, the prefill reads the
    master weights (bit-equal logits), and the step logits stay as close to the quantised fp32 model's as bf16 itself allows:
        d0 = rel(bf16 model, fp32 model) on the UNQUANTISED step logits (both paths exist without this feature),
        rel(fp8 under bf16, fp8 under fp32) <= 1.5 d0    (the margin: another accumulation order over the same exact products).
    The masters sit on the fp8 grid (as in test_fp8_decode.py::test_module_step), so that quantising the fp32 and the bf16 model picks the same
    codes and the comparison is one of kernels, not of two different quantisations.
    Measured on the MI355X: d0 = 5.4687e-3, rel(fp8 under bf16, fp8 under fp32) = 5.7210e-3 (bound 8.2030e-3);
    on the emulator: d0 = 5.8208e-3, 5.5052e-3 (bound 8.7313e-3)."""
    from omnimamba_amd import norm_linear as NL
    from omnimamba_amd import quant
    Bsz = 3
    cfg, m32 = wide_model(dev)
    with torch.no_grad():
        for blk in m32.backbone.layers:
            for lin in (blk.mixer.in_proj, blk.mixer.out_proj):
                lin.weight.copy_(quant.dequantize_rows(*quant.quantize_rows_e4m3(lin.weight)))
    m16 = copy.deepcopy(m32).to(BF)
    emb = torch.randn(Bsz, 6, cfg.d_model).to(dev)
    seen = {"n": 0, "scaled": 0, "forms": []}
    real = NL.norm_linear

    def counting(*a, **k):
        seen["n"] += 1
        seen["scaled"] += k.get("weight_scale") is not None
        seen["forms"].append(NL.form(*a, **k))
        return real(*a, **k)

    monkeypatch.setattr(NL, "norm_linear", counting)
    p32, l32 = _module_run(m32, cfg, emb, Bsz)
    p16, l16 = _module_run(m16, cfg, emb.to(BF), Bsz)
    assert seen["n"] == 2 * (2 * cfg.n_layer * 2) and seen["scaled"] == 0
    d0 = rel(l16, l32)
    assert quant.quantize_decode_weights(m32) == 2 * cfg.n_layer and quant.quantize_decode_weights(m16) == 2 * cfg.n_layer
    seen.update(n=0, scaled=0, forms=[])
    q32p, q32 = _module_run(m32, cfg, emb, Bsz)
    assert seen["scaled"] == 2 * cfg.n_layer * 2 and seen["forms"] == [NL.BATCHED] * (2 * cfg.n_layer * 2)      # fp32 activations: the vector form
    seen.update(n=0, scaled=0, forms=[])
    q16p, q16 = _module_run(m16, cfg, emb.to(BF), Bsz)
    assert seen["n"] == 2 * cfg.n_layer * 2 and seen["scaled"] == 2 * cfg.n_layer * 2                           # in_proj and out_proj, every layer, every step
    assert seen["forms"] == [NL.MATRIX] * (2 * cfg.n_layer * 2)
    assert torch.equal(q16p, p16) and torch.equal(q32p, p32)                                                      # the prefill reads the master weights
    d = rel(q16, q32)
    print(f"d0 = rel(bf16, fp32) unquantised {d0:.4e}; rel(fp8 under bf16, fp8 under fp32) {d:.4e}; bound {1.5 * d0:.4e}")
    assert d <= 1.5 * d0


# ---- 6. captured decode (GPU only) ------------------------------------------------------------------------------------------------------
def _quantised_bf16_model(dev):
    from omnimamba_amd import quant
    cfg, model = wide_model(dev)
    with torch.no_grad():
        model.backbone.img_embeddings.word_embeddings.weight.mul_(30.0)
    model = model.to(BF)
    quant.quantize_decode_weights(model)
    return cfg, model


@pytest.mark.gpu
def test_quantised_bf16_decode_hipgraph_equals_eager():
    """tests/test_fp8_decode.py::test_quantised_decode_hipgraph_equals_eager in bf16 at batch 2: the graph replays the matrix-form fp8 step,
    token for token what the eager loop samples (capture, then replay of the cached graph)."""
    from omnimamba_amd import norm_linear as NL
    from omnimamba_amd.generation import decode
    dev = torch.device("cuda:0")
    cfg, model = _quantised_bf16_model(dev)
    ids, emb = torch.zeros(2, 5, dtype=torch.long, device=dev), torch.randn(2, 5, cfg.d_model, device=dev).to(BF)
    seen, real = {"forms": set()}, NL.norm_linear

    def counting(*a, **k):
        if k.get("weight_scale") is not None:
            seen["forms"].add(NL.form(*a, **k))
        return real(*a, **k)

    NL.norm_linear = counting
    try:
        a = decode(ids, emb, model, 14, top_k=1, task="t2i", cg=False)
        assert seen["forms"] == {NL.MATRIX}                              # the eager loop ran the fp8 step on the matrix form
        b = decode(ids, emb, model, 14, top_k=1, task="t2i", cg=True)
        c = decode(ids, emb, model, 14, top_k=1, task="t2i", cg=True)    # replay of the cached graph
    finally:
        NL.norm_linear = real
    assert torch.equal(a, b) and torch.equal(a, c)


@pytest.mark.gpu
def test_quantised_bf16_decode_ragged_captured_equals_eager():
    """Three slots, five short requests of different lengths on the quantised bf16 model: the captured steps finish with the tokens of the
    eager ones (slots at two and three live sequences, padding rows while the queue drains)."""
    from omnimamba_amd.batch_decode import decode_ragged
    dev = torch.device("cuda:0")
    cfg, model = _quantised_bf16_model(dev)
    torch.manual_seed(11)
    reqs = [(torch.zeros(1, 3, dtype=torch.long, device=dev), torch.randn(1, L, cfg.d_model, device=dev).to(BF)) for L in (5, 7, 4, 6, 5)]
    lens = [12, 15, 10, 13, 14]
    eager = decode_ragged(reqs, model, lens, max_batch=3, task="mmu", cg=False)
    graph = decode_ragged(reqs, model, lens, max_batch=3, task="mmu", cg=True)
    assert len(eager) == len(graph) == 5
    for a, b in zip(eager, graph):
        assert torch.equal(a, b)
