"""Mamba2.forward, prefill of a right-padded batch with InferenceParams.seq_lens: every row's output (up to its length), conv_state and
ssm_state match a batch-1 prefill of that row at its exact length within the module tolerance of test_mamba2_module.py (rel < 1e-4 in
fp32), and one decode step from both caches agrees at the same bound.  The conv state is compared at that bound, not bitwise: its values
come out of an in-proj GEMM of a different M.  Emulator on CPU; MI355X under -m gpu."""
import pytest
import torch

from test_mamba2_extend import cache
from test_mamba2_module import build, rel

LENS = [37, 5, 64, 1]


@pytest.mark.parametrize("branch", ["fused_node", "unfused_env", "unfused_cache_dtype"])
def test_ragged_prefill_matches_per_row_prefills(dev, monkeypatch, branch):
    """fused_node: mamba_split_conv1d_scan_combined with conv_state_out; unfused_*: upstream's branch of separate ops, reached through the
    module's switch or -- as in production -- through a cache whose dtype differs from the activations' (fp16 states under fp32
    activations: both sides round values that agree to ~1e-6 once, to the same fp16 number but for about one element in 500 -- a relative
    L2 of ~3e-5 -- so the bound stays)."""
    if branch == "unfused_env":
        monkeypatch.setenv("OMK_FUSED_PREFILL", "0")
    m, _ = build(dev)
    torch.manual_seed(5)
    B, L = len(LENS), max(LENS)
    u = torch.randn(B, L, 32).to(dev)                      # (the padding positions hold finite garbage, not zeros)
    nxt = torch.randn(B, 1, 32).to(dev)
    calls = []
    from omnimamba_amd import mamba2 as M2
    real = M2.mamba_split_conv1d_scan_combined
    monkeypatch.setattr(M2, "mamba_split_conv1d_scan_combined", lambda *a, **k: calls.append("fused") or real(*a, **k))

    def mk(batch):
        ip, cs, ss = cache(m, dev, batch)
        if branch == "unfused_cache_dtype":
            cs, ss = m.allocate_inference_cache(batch, 512, dtype=torch.float16)
            cs.fill_(7.0)
            ss.fill_(-3.0)
            ip.key_value_memory_dict[0] = (cs, ss)
        return ip, cs, ss

    with torch.no_grad():
        ip, cs, ss = mk(B)
        ip.seq_lens = torch.tensor(LENS, dtype=torch.int32, device=dev)
        out = m(u, inference_params=ip)
        assert (calls == ["fused"]) == (branch == "fused_node")
        assert torch.isfinite(out).all()
        cs0, ss0 = cs.clone(), ss.clone()                  # (the step below moves the states on)
        ip.seq_lens, ip.seqlen_offset = None, L
        step = m(nxt, inference_params=ip)
        tol = 1e-4
        for b, n in enumerate(LENS):
            ip1, cs1, ss1 = mk(1)
            out1 = m(u[b:b + 1, :n], inference_params=ip1)
            e = (rel(out[b, :n], out1[0]), rel(cs0[b], cs1[0]), rel(ss0[b], ss1[0]))
            print(branch, b, n, e)
            assert e[0] < 1e-4 and e[1] < tol and e[2] < tol, (b, n, e)
            if n < 4:
                assert (cs0[b, :, : 4 - n] == 0).all()      # left zero padded, as a prefill of n tokens leaves it
            ip1.seqlen_offset = n
            step1 = m(nxt[b:b + 1], inference_params=ip1)
            assert rel(step[b], step1[0]) < tol, (b, n, rel(step[b], step1[0]))


def test_seq_lens_is_refused_outside_the_prefill(dev):
    m, _ = build(dev)
    with torch.no_grad():
        ip, _, _ = cache(m, dev, 2)
        m(torch.randn(2, 6, 32).to(dev), inference_params=ip)
        ip.seq_lens = torch.tensor([3, 2], dtype=torch.int32, device=dev)
        ip.seqlen_offset = 6
        with pytest.raises(NotImplementedError, match="seq_lens"):
            m(torch.randn(2, 3, 32).to(dev), inference_params=ip)        # _extend
        with pytest.raises(NotImplementedError, match="seq_lens"):
            m(torch.randn(2, 1, 32).to(dev), inference_params=ip)        # step
        with pytest.raises(NotImplementedError, match="seq_lens"):
            m._extend(torch.randn(2, 3, 32).to(dev), 2, 3, None, *ip.key_value_memory_dict[0], ip)


def test_ragged_prefill_with_gradients_raises(dev):
    m, _ = build(dev)
    ip, _, _ = cache(m, dev, 2)
    ip.seq_lens = torch.tensor([6, 2], dtype=torch.int32, device=dev)
    with pytest.raises(NotImplementedError, match="seq_lens"):
        m(torch.randn(2, 6, 32).to(dev), inference_params=ip)
