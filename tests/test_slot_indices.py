"""Slot-indexed decode state (state_batch_indices / conv_state_indices, ABI 8): row b of the batch reads and writes state row idx[b] of a
pool with more rows than the batch; idx[b] < 0 (or >= the pool's rows) is a padding row.  Every case is checked against the same kernel
without indices on the gathered rows pool[idx].clone(): outputs and touched slots bit-identical, every other slot bit-unchanged, padding
outputs zero.  Emulator on CPU, MI355X under -m gpu."""
import pytest
import torch

POOL = 6
IDX = {1: [4], 2: [5, -1], 3: [3, -1, 0], 4: [3, -1, 0, 5], 8: [2, 5, -1, 0, 4, -1, 1, 3]}


def gathered(pool, idx):
    """pool rows of idx (padding rows: any row -- their results are not compared), as a batch of its own."""
    return pool[idx.clamp(min=0).long()].clone()


def check_pool(pool_after, pool_before, ref_after, idx):
    for s in range(pool_before.shape[0]):
        rows = (idx == s).nonzero().flatten().tolist()
        want = ref_after[rows[0]] if rows else pool_before[s]
        assert torch.equal(pool_after[s].cpu(), want.cpu()), f"slot {s} (rows {rows})"


def check_out(out, ref, idx):
    live = idx >= 0
    assert torch.equal(out[live.to(out.device)].cpu(), ref[live.to(ref.device)].cpu())
    assert (out[(~live).to(out.device)] == 0).all()


# ---- selective_state_update: the row kernel (existing shapes) and the tied-scalar kernel (H 64, P 64, N 128, >= 2^21 elements)
@pytest.mark.parametrize("sdt,xdt", [(torch.float32, torch.float32), (torch.bfloat16, torch.bfloat16)])
@pytest.mark.parametrize("H,P,N,G,tied,Bsz", [(4, 64, 128, 1, True, 3), (4, 8, 16, 2, True, 2), (2, 5, 64, 1, False, 3),
                                              (3, 7, 6, 1, False, 2), (64, 64, 128, 1, True, 4)])
def test_state_update_slots(dev, sdt, xdt, H, P, N, G, tied, Bsz):
    from omnimamba_amd.selective_state_update import selective_state_update
    torch.manual_seed(0)
    pool = torch.randn(POOL, H, P, N).to(sdt).to(dev)
    idx = torch.tensor(IDX[Bsz], dtype=torch.int32, device=dev)
    x, z = torch.randn(Bsz, H, P).to(xdt).to(dev), torch.randn(Bsz, H, P).to(xdt).to(dev)
    Bm, Cm = torch.randn(Bsz, G, N).to(xdt).to(dev), torch.randn(Bsz, G, N).to(xdt).to(dev)
    if tied:
        ex = lambda t: t[..., None].expand(*t.shape, P)
        dt, D, dtb = ex(torch.randn(Bsz, H).to(xdt).to(dev)), ex(torch.randn(H).to(dev)), ex(torch.randn(H).to(dev))
        A = (-(torch.rand(H) * 15 + 1)).to(dev)[:, None, None].expand(H, P, N)
    else:
        dt, A = torch.randn(Bsz, H, P).to(xdt).to(dev), (-(torch.rand(H, P, N) + 0.1)).to(dev)
        D, dtb = torch.randn(H, P).to(dev), torch.randn(H, P).to(dev)
    before = pool.clone()
    ref_state = gathered(pool, idx)
    y_ref = selective_state_update(ref_state, x, dt, A, Bm, Cm, D=D, z=z, dt_bias=dtb, dt_softplus=True)
    y = selective_state_update(pool, x, dt, A, Bm, Cm, D=D, z=z, dt_bias=dtb, dt_softplus=True, state_batch_indices=idx)
    check_out(y, y_ref, idx)
    check_pool(pool, before, ref_state, idx)


# ---- causal_conv1d_update on the cache's channel-last layout
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("Bsz", [1, 3, 8])
def test_conv1d_update_slots(dev, dtype, Bsz):
    from omnimamba_amd.causal_conv1d import causal_conv1d_update
    torch.manual_seed(1)
    C, W = 40, 4
    pool_n = max(POOL, Bsz)
    pool = torch.randn(pool_n, W, C).to(dtype).to(dev).transpose(1, 2)           # (pool, C, W) channel-last, as allocate_inference_cache
    idx = torch.tensor(IDX[Bsz], dtype=torch.int32, device=dev)
    x = torch.randn(Bsz, C).to(dtype).to(dev)
    w, b = torch.randn(C, W).to(dtype).to(dev), torch.randn(C).to(dtype).to(dev)
    before = pool.clone()
    ref_state = torch.empty(Bsz, W, C, dtype=dtype, device=dev).transpose(1, 2)
    ref_state.copy_(pool[idx.clamp(min=0).long()])
    y_ref = causal_conv1d_update(x, ref_state, w, b, "silu")
    y = causal_conv1d_update(x, pool, w, b, "silu", conv_state_indices=idx)
    check_out(y, y_ref, idx)
    check_pool(pool, before, ref_state, idx)


# ---- norm_linear with the conv tail (in_features 1024): which kernel each case reaches is fixed by the dispatch in csrc/norm_linear.hip
NL_CASES = [  # (dtype, B, LoRA rank, kernel)
    (torch.float32, 1, 0, "fast"), (torch.bfloat16, 1, 8, "fast"),
    (torch.float32, 2, 0, "batched"), (torch.float32, 4, 8, "batched"),
    (torch.float32, 8, 8, "mfma"), (torch.bfloat16, 2, 0, "mfma"), (torch.bfloat16, 4, 8, "mfma"), (torch.bfloat16, 8, 0, "mfma"),
]


@pytest.mark.parametrize("dtype,Bsz,rank,kernel", NL_CASES, ids=[f"{k}-{str(d)[6:]}-B{b}-r{r}" for d, b, r, k in NL_CASES])
def test_norm_linear_conv_tail_slots(dev, dtype, Bsz, rank, kernel):
    from omnimamba_amd.norm_linear import conv_tail_applies, norm_linear
    torch.manual_seed(2)
    In, Out, off, C, W = 1024, 224, 48, 128, 4
    pool_n = max(POOL, Bsz + 1)
    x = torch.randn(Bsz, In).to(dtype).to(dev)
    res = torch.randn(Bsz, In).to(dev)
    Wt = (torch.randn(Out, In) / 32).to(dtype).to(dev)
    nw = (1 + 0.1 * torch.randn(In)).to(dtype).to(dev)
    cw, cb = torch.randn(C, W).to(dtype).to(dev), torch.randn(C).to(dtype).to(dev)
    lora = {} if rank == 0 else dict(lora_a=(torch.randn(rank, In) / 32).to(dtype).to(dev), lora_b=(torch.randn(Out, rank) / 4).to(dtype).to(dev),
                                     lora_scale=0.5)
    pool = torch.randn(pool_n, W, C).to(dtype).to(dev).transpose(1, 2)
    idx = torch.tensor(IDX[Bsz], dtype=torch.int32, device=dev)
    assert conv_tail_applies(x, Wt, nw, pool, cw, cb, lora.get("lora_a"), None, res)
    before = pool.clone()
    ref_state = torch.empty(Bsz, W, C, dtype=dtype, device=dev).transpose(1, 2)
    ref_state.copy_(pool[idx.clamp(min=0).long()])
    kw = dict(norm_weight=nw, residual=res, residual_out_dtype=torch.float32, conv_weight=cw, conv_bias=cb, conv_offset=off, **lora)
    o_ref, r_ref = norm_linear(x, Wt, conv_state=ref_state, **kw)
    o, r = norm_linear(x, Wt, conv_state=pool, conv_state_indices=idx, **kw)
    live = (idx >= 0).to(o.device)
    assert torch.equal(r.cpu(), r_ref.cpu())
    assert torch.equal(o[live].cpu(), o_ref[live].cpu())
    # padding sequences: zeros in the conv columns only, every other column computed as usual
    assert (o[~live][:, off:off + C] == 0).all()
    assert torch.equal(o[~live][:, :off].cpu(), o_ref[~live][:, :off].cpu()) and torch.equal(o[~live][:, off + C:].cpu(), o_ref[~live][:, off + C:].cpu())
    check_pool(pool, before, ref_state, idx)


def test_index_past_the_pool_touches_nothing():
    """Emulator only (never on the GPU): an index equal to the pool's row count is a padding row -- the row right behind the pool, part of
    a larger guard buffer the pool is a slice of, stays bit-unchanged in all three ops."""
    from emu.loader import use_emulator
    from omnimamba_amd.causal_conv1d import causal_conv1d_update
    from omnimamba_amd.norm_linear import norm_linear
    from omnimamba_amd.selective_state_update import selective_state_update
    torch.manual_seed(3)
    with use_emulator():
        H, P, N = 2, 8, 16
        guard = torch.randn(POOL + 2, H, P, N)
        pool, keep = guard[1:POOL + 1], guard.clone()
        idx = torch.tensor([POOL, 2], dtype=torch.int32)
        ex = lambda t: t[..., None].expand(*t.shape, P)
        y = selective_state_update(pool, torch.randn(2, H, P), ex(torch.randn(2, H)), (-torch.rand(H) - 1)[:, None, None].expand(H, P, N),
                                   torch.randn(2, 1, N), torch.randn(2, 1, N), D=ex(torch.randn(H)), dt_bias=ex(torch.randn(H)),
                                   dt_softplus=True, state_batch_indices=idx)
        assert (y[0] == 0).all()
        assert torch.equal(guard[POOL + 1], keep[POOL + 1]) and torch.equal(guard[0], keep[0])
        assert not torch.equal(guard[3], keep[3])                 # (slot 2 of the pool was stepped)
        C, W = 24, 4
        cguard = torch.randn(POOL + 2, W, C).transpose(1, 2)
        cpool, ckeep = cguard[1:POOL + 1], cguard.clone()
        out = causal_conv1d_update(torch.randn(2, C), cpool, torch.randn(C, W), torch.randn(C), "silu", conv_state_indices=idx)
        assert (out[0] == 0).all() and torch.equal(cguard[POOL + 1], ckeep[POOL + 1]) and torch.equal(cguard[0], ckeep[0])
        C = 128
        nguard = torch.randn(POOL + 2, W, C).transpose(1, 2)
        npool, nkeep = nguard[1:POOL + 1], nguard.clone()
        for bsz in (1, 2):
            o = norm_linear(torch.randn(bsz, 1024), torch.randn(160, 1024) / 32, norm_weight=torch.ones(1024), conv_state=npool,
                            conv_weight=torch.randn(C, W), conv_bias=torch.randn(C), conv_offset=16,
                            conv_state_indices=torch.tensor([POOL, 2][:bsz], dtype=torch.int32))
            assert (o[0, 16:16 + C] == 0).all()
            assert torch.equal(nguard[POOL + 1], nkeep[POOL + 1]) and torch.equal(nguard[0], nkeep[0])


def test_index_wrapper_checks(dev):
    from omnimamba_amd.causal_conv1d import causal_conv1d_update
    from omnimamba_amd.norm_linear import norm_linear
    from omnimamba_amd.selective_state_update import selective_state_update
    torch.manual_seed(4)
    H, P, N, C, W = 2, 4, 8, 16, 4
    st = torch.randn(4, H, P, N, device=dev)
    args = lambda: (torch.randn(2, H, P, device=dev), torch.randn(2, H, P, device=dev), -torch.rand(H, P, N, device=dev) - 0.1,
                    torch.randn(2, 1, N, device=dev), torch.randn(2, 1, N, device=dev))
    with pytest.raises(TypeError):
        selective_state_update(st, *args(), state_batch_indices=torch.tensor([0.0, 1.0], device=dev))
    with pytest.raises(ValueError):
        selective_state_update(st, *args(), state_batch_indices=torch.tensor([0, 1, 2], dtype=torch.int32, device=dev))
    # int64 is cast (one extra launch) and gives the int32 result
    s1, s2 = st.clone(), st.clone()
    a = args()
    y1 = selective_state_update(s1, *a, state_batch_indices=torch.tensor([3, 1], device=dev))
    y2 = selective_state_update(s2, *a, state_batch_indices=torch.tensor([3, 1], dtype=torch.int32, device=dev))
    assert torch.equal(y1, y2) and torch.equal(s1, s2)
    cs = torch.randn(4, W, C, device=dev).transpose(1, 2)
    x, w = torch.randn(2, C, device=dev), torch.randn(C, W, device=dev)
    with pytest.raises(TypeError):
        causal_conv1d_update(x, cs, w, None, "silu", conv_state_indices=torch.tensor([0, 1], dtype=torch.int16, device=dev))
    with pytest.raises(ValueError):
        causal_conv1d_update(x, cs, w, None, "silu", conv_state_indices=torch.tensor([[0, 1]], dtype=torch.int32, device=dev))
    with pytest.raises(NotImplementedError):
        causal_conv1d_update(x, cs, w, None, "silu", cache_seqlens=torch.tensor([0, 1], dtype=torch.int32, device=dev))
    with pytest.raises(ValueError):
        norm_linear(torch.randn(1, 1024, device=dev), torch.randn(64, 1024, device=dev), norm_weight=torch.ones(1024, device=dev),
                    conv_state_indices=torch.tensor([0], dtype=torch.int32, device=dev))
