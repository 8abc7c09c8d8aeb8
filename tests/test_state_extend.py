"""omk_selective_state_extend (ABI 9): T tokens of one turn applied to a cached SSM state in one launch.

fp32 state: the final state is bit-identical to T successive selective_state_update calls (the recurrence is elementwise and both kernels
evaluate it expression for expression), every y_t is within op_bound of the fp64 recurrence started from the same state.  16-bit state:
the final state is within op_bound of the fp64 recurrence rounded once.  Slot indices: as tests/test_slot_indices.py, against the same
kernel on the gathered pool rows.  Emulator on CPU, MI355X under -m gpu."""
import pytest
import torch

import oracle.ops as O
from tolerances import op_bound, rel

SHAPES = [  # (H, P, N, G, gpu only)
    (4, 64, 128, 1, False), (64, 64, 128, 1, True), (4, 16, 16, 2, False),
]
TS = [1, 2, 7, 33, 256]


def inputs(Bsz, T, H, P, N, G, xdt, dev, seed=0):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)
    return dict(x=r(Bsz, T, H, P).to(xdt).to(dev), dt=(r(Bsz, T, H) - 1).to(xdt).to(dev), A=(-(torch.rand(H, generator=g) * 15 + 1)).to(dev),
                B=r(Bsz, T, G, N).to(xdt).to(dev), C=r(Bsz, T, G, N).to(xdt).to(dev), D=r(H).to(dev), z=r(Bsz, T, H, P).to(xdt).to(dev),
                dt_bias=(r(H) - 2).to(dev))


def stepwise(state, kw, T, use_z, use_D, use_tb):
    """T selective_state_update calls on `state` (in place) -> y (B, T, H, P)."""
    from omnimamba_amd.selective_state_update import selective_state_update
    H, P, N = state.shape[1:]
    Bsz = state.shape[0]
    ys = []
    for t in range(T):
        ys.append(selective_state_update(
            state, kw["x"][:, t], kw["dt"][:, t, :, None].expand(Bsz, H, P), kw["A"][:, None, None].expand(H, P, N), kw["B"][:, t], kw["C"][:, t],
            D=kw["D"][:, None].expand(H, P) if use_D else None, z=kw["z"][:, t] if use_z else None,
            dt_bias=kw["dt_bias"][:, None].expand(H, P) if use_tb else None, dt_softplus=True))
    return torch.stack(ys, 1)


@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("sdt,xdt", [(torch.float32, torch.float32), (torch.bfloat16, torch.bfloat16), (torch.float32, torch.bfloat16)])
@pytest.mark.parametrize("H,P,N,G,gpu_only", SHAPES)
@pytest.mark.parametrize("opt", ["zDtb", "none"])
def test_state_extend(dev, T, sdt, xdt, H, P, N, G, gpu_only, opt):
    from omnimamba_amd.selective_state_update import selective_state_extend
    if gpu_only and dev.type == "cpu":
        pytest.skip("emulator: the H 64 shape runs on the MI355X (-m gpu)")
    use = opt == "zDtb"
    Bsz = 2
    kw = inputs(Bsz, T, H, P, N, G, xdt, dev)
    s0 = (0.5 * torch.randn(Bsz, H, P, N, generator=torch.Generator().manual_seed(1))).to(sdt).to(dev)
    state = s0.clone()
    y = selective_state_extend(state, kw["x"], kw["dt"], kw["A"], kw["B"], kw["C"], D=kw["D"] if use else None, z=kw["z"] if use else None,
                               dt_bias=kw["dt_bias"] if use else None, dt_softplus=True)
    assert y.shape == kw["x"].shape and y.dtype == xdt
    y64, s64 = O.ssd_ref_sequential(kw["x"].cpu().double(), kw["dt"].cpu(), kw["A"].cpu(), kw["B"].cpu(), kw["C"].cpu(),
                                    D=kw["D"].cpu() if use else None, z=kw["z"].cpu() if use else None,
                                    dt_bias=kw["dt_bias"].cpu() if use else None, initial_states=s0.cpu(), dt_softplus=True,
                                    return_final_states=True, compute_dtype=torch.float64)
    for t in range(T):
        assert rel(y[:, t], y64[:, t]) <= op_bound(y64[:, t], xdt), f"y_{t}"
    if sdt == torch.float32:
        ref = s0.clone()
        stepwise(ref, kw, T, use, use, use)
        assert torch.equal(state.cpu(), ref.cpu()), "final state differs from T single-token updates"
    else:
        assert rel(state, s64) <= op_bound(s64, sdt)


IDX = {1: [4], 3: [3, -1, 0], 4: [3, -1, 0, 5]}


@pytest.mark.parametrize("sdt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("Bsz", [1, 3, 4])
@pytest.mark.parametrize("T", [1, 7, 33])
def test_state_extend_slots(dev, sdt, Bsz, T):
    from omnimamba_amd.selective_state_update import selective_state_extend
    H, P, N, G = 4, 64, 128, 1
    kw = inputs(Bsz, T, H, P, N, G, sdt, dev, seed=3)
    pool = torch.randn(6, H, P, N, generator=torch.Generator().manual_seed(4)).to(sdt).to(dev)
    idx = torch.tensor(IDX[Bsz], dtype=torch.int32, device=dev)
    before = pool.clone()
    ref_state = pool[idx.clamp(min=0).long()].clone()
    args = (kw["x"], kw["dt"], kw["A"], kw["B"], kw["C"])
    opts = dict(D=kw["D"], z=kw["z"], dt_bias=kw["dt_bias"], dt_softplus=True)
    y_ref = selective_state_extend(ref_state, *args, **opts)
    y = selective_state_extend(pool, *args, **opts, state_batch_indices=idx)
    live = idx >= 0
    assert torch.equal(y[live].cpu(), y_ref[live].cpu())
    assert (y[~live] == 0).all()
    for s in range(pool.shape[0]):
        rows = (idx == s).nonzero().flatten().tolist()
        want = ref_state[rows[0]] if rows else before[s]
        assert torch.equal(pool[s].cpu(), want.cpu()), f"slot {s} (rows {rows})"


def test_state_extend_refuses_unsupported_dstate(dev):
    from omnimamba_amd.selective_state_update import selective_state_extend
    kw = inputs(1, 3, 2, 4, 12, 1, torch.float32, dev)
    with pytest.raises(RuntimeError, match="omk_status -4"):
        selective_state_extend(torch.zeros(1, 2, 4, 12, device=dev), kw["x"], kw["dt"], kw["A"], kw["B"], kw["C"], dt_softplus=True)
