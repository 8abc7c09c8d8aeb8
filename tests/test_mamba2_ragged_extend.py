"""Mamba2.forward with InferenceParams.extend_lens: the rows of a right-padded batch continue their cached sequences by different numbers
of tokens in one pass (follow-up turns of several conversations), on a batch cache or, with state_indices, on rows of a slot pool.

Four rows prefilled at lengths 13 / 2 / 20 / 5 are extended raggedly, once below EXTEND_SCAN_MAX_T (conv update + extend kernel on the
states in place) and once above it (conv + chunked scan from the gathered states, with a row of length 0).  The reference is the existing
batch-1 extend of every row at its exact length: output up to the length, conv_state, ssm_state and the next decode step agree within the
module bound of test_mamba2_module.py (rel < 1e-4; the conv inputs come out of an in_proj GEMM of another M, so nothing is claimed to the
bit there).  The row of length 0 and the pool rows nobody points at keep their states to the bit.  Emulator on CPU; MI355X under -m gpu."""
import pytest
import torch

from test_mamba2_extend import cache
from test_mamba2_module import build, rel

PREFILL = [13, 2, 20, 5]
CASES = {"extend": [5, 1, 16, 3], "scan": [70, 2, 17, 0]}
SLOTS, POOL = [4, 0, 5, 2], 6
_REF = {}


def tokens(lens):
    g = torch.Generator().manual_seed(21)
    r = lambda *s: torch.randn(*s, generator=g)
    return [r(1, n, 32) for n in PREFILL], [r(1, n, 32) for n in lens], r(4, 1, 32)


def reference(m, dev, case):
    """Per row: the states after the prefill, and output / states / next step of the batch-1 extend at the row's exact length.
    Computed once per device and case, kept on the CPU, never modified."""
    key = (dev.type, case)
    if key not in _REF:
        u_pre, u_ext, nxt = tokens(CASES[case])
        rows = []
        with torch.no_grad():
            for b, n in enumerate(CASES[case]):
                ip, cs, ss = cache(m, dev, 1)
                m(u_pre[b].to(dev), inference_params=ip)
                pre = (cs.clone().cpu(), ss.clone().cpu())
                ip.seqlen_offset = PREFILL[b]
                out = m(u_ext[b].to(dev), inference_params=ip).cpu() if n > 0 else None
                post = (cs.clone().cpu(), ss.clone().cpu())
                ip.seqlen_offset = PREFILL[b] + n
                step = m(nxt[b:b + 1].to(dev), inference_params=ip).cpu()
                rows.append(dict(pre=pre, out=out, post=post, step=step))
        _REF[key] = rows
    return _REF[key]


@pytest.mark.parametrize("pooled", [False, True])
@pytest.mark.parametrize("case", ["extend", "scan"])
def test_ragged_extend_matches_each_row_alone(dev, monkeypatch, case, pooled):
    from omnimamba_amd import mamba2 as M2
    lens = CASES[case]
    assert (max(lens) <= M2.EXTEND_SCAN_MAX_T) == (case == "extend")
    m, _ = build(dev)
    ref = reference(m, dev, case)
    _, u_ext, nxt = tokens(lens)
    calls = []
    for name in ("selective_state_extend", "mamba_chunk_scan_combined", "causal_conv1d_update", "causal_conv1d_fn"):
        real = getattr(M2, name)
        monkeypatch.setattr(M2, name, lambda *a, _n=name, _f=real, **k: calls.append(_n) or _f(*a, **k))
    with torch.no_grad():
        ip, cs, ss = cache(m, dev, POOL if pooled else 4)      # every row garbage until a prefilled state is copied in
        where = SLOTS if pooled else [0, 1, 2, 3]
        for b, s in enumerate(where):
            cs[s].copy_(ref[b]["pre"][0][0])
            ss[s].copy_(ref[b]["pre"][1][0])
        before = (cs.clone(), ss.clone())
        u = torch.zeros(4, max(lens), 32)
        for b, n in enumerate(lens):
            u[b, :n] = u_ext[b][0]
        ip.seqlen_offset = 1                                    # > 0: an extend; the rows' own offsets are not read
        ip.extend_lens = torch.tensor(lens, dtype=torch.int32, device=dev)
        if pooled:
            ip.state_indices = torch.tensor(SLOTS, dtype=torch.int32, device=dev)
        calls.clear()
        out = m(u.to(dev), inference_params=ip)
        assert calls == (["causal_conv1d_update", "selective_state_extend"] if case == "extend" else ["causal_conv1d_fn", "mamba_chunk_scan_combined"])
        assert out.shape == (4, max(lens), 32) and torch.isfinite(out).all()
        for b, (s, n) in enumerate(zip(where, lens)):
            if n == 0:
                assert torch.equal(cs[s].cpu(), before[0][s].cpu()) and torch.equal(ss[s].cpu(), before[1][s].cpu()), "a row of length 0 keeps its states to the bit"
                continue
            assert rel(out[b, :n], ref[b]["out"][0]) < 1e-4, f"row {b}: output"
            assert rel(cs[s], ref[b]["post"][0][0]) < 1e-4, f"row {b}: conv_state"
            assert rel(ss[s], ref[b]["post"][1][0]) < 1e-4, f"row {b}: ssm_state"
        for s in set(range(cs.shape[0])) - set(where):
            assert torch.equal(cs[s].cpu(), before[0][s].cpu()) and torch.equal(ss[s].cpu(), before[1][s].cpu()), f"pool row {s} was not to be touched"
        # one decode step from the ragged cache against the step from every row's own cache
        ip.extend_lens = None
        step = m(nxt.to(dev), inference_params=ip)
        for b in range(4):
            assert rel(step[b], ref[b]["step"][0]) < 1e-4, f"row {b}: next step"


def test_extend_lens_belongs_to_an_extend(dev):
    m, _ = build(dev)
    lens = torch.tensor([3, 2], dtype=torch.int32, device=dev)
    with torch.no_grad():
        ip, _, _ = cache(m, dev, 2)
        ip.extend_lens = lens
        with pytest.raises(NotImplementedError):               # a prefill takes seq_lens
            m(torch.randn(2, 4, 32).to(dev), inference_params=ip)
        ip.extend_lens = None
        m(torch.randn(2, 4, 32).to(dev), inference_params=ip)
        ip.seqlen_offset, ip.extend_lens = 4, lens
        with pytest.raises(NotImplementedError):               # a decode step takes none
            m(torch.randn(2, 1, 32).to(dev), inference_params=ip)
        with pytest.raises(ValueError):                         # one length per row
            ip.extend_lens = lens[:1]
            m(torch.randn(2, 3, 32).to(dev), inference_params=ip)
    ip.extend_lens = lens
    with pytest.raises(NotImplementedError):                   # an inference path: no gradients
        m(torch.randn(2, 3, 32).to(dev), inference_params=ip)
