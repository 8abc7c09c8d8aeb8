"""Mamba2.forward with a cache at seqlen_offset > 0 and L > 1: the cached sequence continues by L tokens (a follow-up turn).  After a
prefill of L1 tokens and an extend by T, output, conv_state (all d_conv columns, bitwise) and ssm_state match a prefill of the L1 + T
concatenation within the module tolerance of test_mamba2_module.py, on both sides of EXTEND_SCAN_MAX_T (extend kernel / chunked scan
with initial states), and a following step from both caches gives the same token.  Emulator on CPU; MI355X under -m gpu."""
from types import SimpleNamespace

import pytest
import torch

from test_mamba2_module import build, rel


def cache(m, dev, batch):
    ip = SimpleNamespace(key_value_memory_dict={}, seqlen_offset=0, max_seqlen=512, max_batch_size=batch, lengths_per_sample=None)
    cs, ss = m.allocate_inference_cache(batch, 512)
    cs.fill_(7.0)                                   # garbage: the prefill must overwrite it
    ss.fill_(-3.0)
    ip.key_value_memory_dict[0] = (cs, ss)
    return ip, cs, ss


@pytest.mark.parametrize("L1,T", [(13, 1), (13, 5), (2, 5), (20, 64), (20, 300)])   # (T 1: the decode step)
def test_extend_matches_prefill_of_the_concatenation(dev, L1, T):
    from omnimamba_amd import mamba2 as M2
    m, _ = build(dev)
    torch.manual_seed(7)
    u = torch.randn(2, L1 + T, 32).to(dev)
    with torch.no_grad():
        ip_a, cs_a, ss_a = cache(m, dev, 2)
        full = m(u, inference_params=ip_a)
        ip_b, cs_b, ss_b = cache(m, dev, 2)
        head = m(u[:, :L1], inference_params=ip_b)
        ip_b.seqlen_offset = L1
        tail = m(u[:, L1:], inference_params=ip_b)
        assert tail.shape == (2, T, 32)
        assert rel(torch.cat([head, tail], 1), full) < 1e-4
        assert rel(tail, full[:, L1:]) < 1e-4
        assert torch.equal(cs_b.cpu(), cs_a.cpu())  # the last d_conv inputs of the concatenation, copies of the same values
        assert rel(ss_b, ss_a) < 1e-4
        # the next decode step from either cache
        ip_a.seqlen_offset = ip_b.seqlen_offset = L1 + T
        nxt = torch.randn(2, 1, 32).to(dev)
        assert rel(m(nxt, inference_params=ip_b), m(nxt, inference_params=ip_a)) < 1e-4
    assert M2.EXTEND_SCAN_MAX_T >= 5 and M2.EXTEND_SCAN_MAX_T < 300   # both sides of the crossover are covered above


def test_extend_uses_the_extend_kernel_below_the_crossover(dev, monkeypatch):
    """Short turns reach omk_selective_state_extend, long ones the chunked scan with initial states."""
    from omnimamba_amd import mamba2 as M2
    calls = []
    real_ext, real_scan = M2.selective_state_extend, M2.mamba_chunk_scan_combined
    monkeypatch.setattr(M2, "selective_state_extend", lambda *a, **k: calls.append("extend") or real_ext(*a, **k))
    monkeypatch.setattr(M2, "mamba_chunk_scan_combined", lambda *a, **k: calls.append("scan") or real_scan(*a, **k))
    m, _ = build(dev)
    u = torch.randn(1, 8 + M2.EXTEND_SCAN_MAX_T + 1, 32).to(dev)
    with torch.no_grad():
        ip, _, _ = cache(m, dev, 1)
        m(u[:, :4], inference_params=ip)
        calls.clear()
        ip.seqlen_offset = 4
        m(u[:, 4:8], inference_params=ip)
        ip.seqlen_offset = 8
        m(u[:, 8:], inference_params=ip)
    assert calls == ["extend", "scan"]


def test_extend_refuses_slot_indices(dev):
    m, _ = build(dev)
    with torch.no_grad():
        ip, _, _ = cache(m, dev, 1)
        m(torch.randn(1, 4, 32).to(dev), inference_params=ip)
        ip.seqlen_offset, ip.state_indices = 4, torch.zeros(1, dtype=torch.int32, device=dev)
        with pytest.raises(NotImplementedError):
            m(torch.randn(1, 3, 32).to(dev), inference_params=ip)
