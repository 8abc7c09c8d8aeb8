"""Per-row lengths in the two kernels that apply T tokens to a cached state (ABI 13): omk_selective_state_extend and
omk_causal_conv1d_update with seq_lens.  Row b applies its first n_b = clamp(seq_lens[b], 0, T) tokens: its outputs up to n_b and its
state are BIT-identical to the same function called on that row alone with T = n_b (rows are independent and the per-token expressions
are unchanged, so no tolerance is involved), outputs behind n_b are zeros, and a row of length 0 -- like every pool slot no row points
at -- keeps its state to the bit.  Emulator on CPU, MI355X under -m gpu."""
import pytest
import torch

from test_state_extend import inputs

SHAPES = [  # (H, P, N, G, gpu only)
    (4, 64, 128, 1, False), (4, 16, 16, 2, False), (64, 64, 128, 1, True),
]
DTYPES = [(torch.float32, torch.float32), (torch.bfloat16, torch.bfloat16), (torch.float32, torch.bfloat16)]
SLOTS, POOL = [3, -1, 0, 5, 1], 7


def lengths(T):
    return [T, 0, 1, 5, T - 2]


def extend_args(kw, use, rows=slice(None), n=None):
    """(positional, keyword) arguments of selective_state_extend for batch rows `rows`, first `n` tokens."""
    cut = lambda t: t[rows, :n]
    return ((cut(kw["x"]), cut(kw["dt"]), kw["A"], cut(kw["B"]), cut(kw["C"])),
            dict(D=kw["D"] if use else None, z=cut(kw["z"]) if use else None, dt_bias=kw["dt_bias"] if use else None, dt_softplus=True))


@pytest.mark.parametrize("T", [7, 33])          # not a multiple of the prefetch distance 4; longer than the ring
@pytest.mark.parametrize("sdt,xdt", DTYPES)
@pytest.mark.parametrize("H,P,N,G,gpu_only", SHAPES)
@pytest.mark.parametrize("opt", ["zDtb", "none"])
def test_state_extend_seq_lens(dev, T, sdt, xdt, H, P, N, G, gpu_only, opt):
    from omnimamba_amd.selective_state_update import selective_state_extend
    if gpu_only and dev.type == "cpu":
        pytest.skip("emulator: the H 64 shape runs on the MI355X (-m gpu)")
    use, Bsz, lens_h = opt == "zDtb", 5, lengths(T)
    kw = inputs(Bsz, T, H, P, N, G, xdt, dev, seed=5)
    s0 = (0.5 * torch.randn(Bsz, H, P, N, generator=torch.Generator().manual_seed(6))).to(sdt).to(dev)
    args, opts = extend_args(kw, use)
    state = s0.clone()
    y = selective_state_extend(state, *args, **opts, seq_lens=torch.tensor(lens_h, dtype=torch.int32, device=dev))
    assert y.shape == kw["x"].shape and y.dtype == xdt
    for b, n in enumerate(lens_h):
        assert (y[b, n:] == 0).all(), f"row {b}: outputs behind its length"
        if n == 0:
            assert torch.equal(state[b].cpu(), s0[b].cpu()), "a row of length 0 must keep its state to the bit"
            continue
        alone = s0[b:b + 1].clone()
        a1, o1 = extend_args(kw, use, slice(b, b + 1), n)
        y1 = selective_state_extend(alone, *a1, **o1)
        assert torch.equal(y[b, :n].cpu(), y1[0].cpu()), f"row {b}: y differs from the row alone at T = {n}"
        assert torch.equal(state[b].cpu(), alone[0].cpu()), f"row {b}: state differs from the row alone at T = {n}"
    # lengths outside 0 .. T are clamped on the device
    state2 = s0.clone()
    y2 = selective_state_extend(state2, *args, **opts, seq_lens=torch.tensor([T + 5, -3] + lens_h[2:], dtype=torch.int32, device=dev))
    assert torch.equal(y2.cpu(), y.cpu()) and torch.equal(state2.cpu(), state.cpu())


@pytest.mark.parametrize("T", [7, 33])
@pytest.mark.parametrize("sdt", [torch.float32, torch.bfloat16])
def test_state_extend_seq_lens_slots(dev, sdt, T):
    from omnimamba_amd.selective_state_update import selective_state_extend
    H, P, N, G = 4, 64, 128, 1
    lens_h = lengths(T)
    kw = inputs(5, T, H, P, N, G, sdt, dev, seed=7)
    pool = torch.randn(POOL, H, P, N, generator=torch.Generator().manual_seed(8)).to(sdt).to(dev)
    before = pool.clone()
    args, opts = extend_args(kw, True)
    y = selective_state_extend(pool, *args, **opts, state_batch_indices=torch.tensor(SLOTS, dtype=torch.int32, device=dev),
                               seq_lens=torch.tensor(lens_h, dtype=torch.int32, device=dev))
    touched = set()
    for b, (s, n) in enumerate(zip(SLOTS, lens_h)):
        if s < 0 or n == 0:
            assert (y[b] == 0).all()
            continue
        touched.add(s)
        alone = before[s:s + 1].clone()
        a1, o1 = extend_args(kw, True, slice(b, b + 1), n)
        y1 = selective_state_extend(alone, *a1, **o1)
        assert torch.equal(y[b, :n].cpu(), y1[0].cpu()) and (y[b, n:] == 0).all()
        assert torch.equal(pool[s].cpu(), alone[0].cpu()), f"slot {s}"
    for s in set(range(POOL)) - touched:
        assert torch.equal(pool[s].cpu(), before[s].cpu()), f"slot {s} was not to be touched"


def conv_inputs(Bsz, rows, C, W, S, T, dt, dev):
    g = torch.Generator().manual_seed(9)
    x = torch.randn(Bsz, T, C, generator=g).to(dt).to(dev).transpose(1, 2)          # channel-last, as the module holds it
    state = torch.randn(rows, S, C, generator=g).to(dt).to(dev).transpose(1, 2)
    return x, state, torch.randn(C, W, generator=g).to(dt).to(dev), torch.randn(C, generator=g).to(dt).to(dev)


@pytest.mark.parametrize("W,S", [(2, 1), (2, 2), (4, 3), (4, 4)])     # state length W - 1 and W
@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("indexed", [False, True])
def test_conv1d_update_seq_lens(dev, W, S, dt, indexed):
    from omnimamba_amd.causal_conv1d import causal_conv1d_update
    C, T, Bsz, lens_h = 24, 6, 5, [6, 0, 1, 3, 2]                       # some lengths below the state length
    slots = SLOTS if indexed else list(range(Bsz))
    x, state, w, bias = conv_inputs(Bsz, POOL if indexed else Bsz, C, W, S, T, dt, dev)
    before = state.clone()
    out = causal_conv1d_update(x, state, w, bias, "silu", seq_lens=torch.tensor(lens_h, dtype=torch.int32, device=dev),
                               conv_state_indices=torch.tensor(slots, dtype=torch.int32, device=dev) if indexed else None)
    assert out.shape == x.shape and out.dtype == dt
    touched = set()
    for b, (s, n) in enumerate(zip(slots, lens_h)):
        if s < 0 or n == 0:
            assert (out[b] == 0).all()
            continue
        touched.add(s)
        alone = before[s:s + 1].clone()
        o1 = causal_conv1d_update(x[b:b + 1, :, :n], alone, w, bias, "silu")
        assert torch.equal(out[b, :, :n].cpu(), o1[0].cpu()), f"row {b}: out differs from the row alone at T = {n}"
        assert (out[b, :, n:] == 0).all(), f"row {b}: outputs behind its length"
        assert torch.equal(state[s].cpu(), alone[0].cpu()), f"row {b}: state differs from the row alone at T = {n}"
        # the last S values of (old state ++ the row's n inputs)
        assert torch.equal(state[s].cpu(), torch.cat([before[s], x[b, :, :n]], dim=-1)[:, -S:].cpu())
    for s in set(range(state.shape[0])) - touched:
        assert torch.equal(state[s].cpu(), before[s].cpu()), f"state row {s} was not to be touched"
    # without seq_lens the call is what it was
    st_a, st_b = before.clone(), before.clone()
    kw = dict(conv_state_indices=torch.tensor(slots, dtype=torch.int32, device=dev)) if indexed else {}
    o_a = causal_conv1d_update(x, st_a, w, bias, "silu", seq_lens=torch.tensor([T + 5] * Bsz, dtype=torch.int32, device=dev), **kw)
    o_b = causal_conv1d_update(x, st_b, w, bias, "silu", **kw)
    assert torch.equal(o_a.cpu(), o_b.cpu()) and torch.equal(st_a.cpu(), st_b.cpu())


def test_seq_lens_host_checks(dev):
    from omnimamba_amd.causal_conv1d import causal_conv1d_update
    from omnimamba_amd.selective_state_update import selective_state_extend
    T, lens_h = 7, lengths(7)
    kw = inputs(5, T, 4, 16, 16, 2, torch.float32, dev)
    args, opts = extend_args(kw, True)
    s0 = torch.randn(5, 4, 16, 16).to(dev)
    x, cs0, w, bias = conv_inputs(5, 5, 24, 4, 4, 6, torch.float32, dev)
    run_ext = lambda lens: selective_state_extend(s0.clone(), *args, **opts, seq_lens=lens)
    run_conv = lambda lens: causal_conv1d_update(x, cs0.clone(), w, bias, "silu", seq_lens=lens)
    i32, i64 = torch.tensor(lens_h, dtype=torch.int32, device=dev), torch.tensor(lens_h, dtype=torch.int64, device=dev)
    assert torch.equal(run_ext(i64).cpu(), run_ext(i32).cpu())           # int64 is cast once and accepted
    assert torch.equal(run_conv(i64).cpu(), run_conv(i32).cpu())
    for run in (run_ext, run_conv):
        with pytest.raises(ValueError):
            run(i32[:4])
        with pytest.raises(ValueError):
            run(i32[:, None])
        with pytest.raises(TypeError):
            run(i32.float())
        with pytest.raises(TypeError):
            run(i32.to(torch.int16))
