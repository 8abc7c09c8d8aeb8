"""Continuous batching (omnimamba_amd/batch_decode.py): the slot-indexed Mamba2 step, prefill into slot views, and decode_ragged /
mmu_generate_batch against mmu_generate of each request alone.  Emulator on CPU (eager), MI355X under -m gpu (eager and captured)."""
import pytest
import torch

from test_stack_decode_train import TINY_SPECIAL, tiny_path


def test_mamba2_step_with_state_indices_is_the_gathered_step(dev):
    from omnimamba_amd.mamba2 import Mamba2
    torch.manual_seed(0)
    m = Mamba2(32, d_state=16, headdim=8, layer_idx=0).to(dev).eval()
    conv, ssm = m.allocate_inference_cache(5, 0)
    conv.copy_(torch.randn(conv.shape)), ssm.copy_(torch.randn(ssm.shape))
    idx = torch.tensor([3, -1, 1], dtype=torch.int32, device=dev)
    u = torch.randn(3, 1, 32, device=dev)
    c0, s0 = conv.clone(), ssm.clone()
    gc = torch.empty(3, conv.shape[2], conv.shape[1], device=dev).transpose(1, 2)
    gc.copy_(conv[idx.clamp(min=0).long()])
    gs = ssm[idx.clamp(min=0).long()].clone()
    with torch.no_grad():
        want, _, _ = m.step(u, gc, gs)
        got, _, _ = m.step(u, conv, ssm, state_indices=idx)
    for r, s in ((0, 3), (2, 1)):
        assert torch.equal(got[r], want[r]) and torch.equal(conv[s], gc[r]) and torch.equal(ssm[s], gs[r])
    for s in (0, 2, 4):
        assert torch.equal(conv[s], c0[s]) and torch.equal(ssm[s], s0[s])


def test_prefill_into_slot_views_equals_own_cache(dev):
    """A batch-1 prefill with a cache of views (conv[s:s+1], ssm[s:s+1]) of the pool leaves the states a prefill into its own cache does
    (the fused prefill's conv_state_out and ssm_state.copy_ honour the views' strides) and touches no other slot."""
    from omnimamba_amd.generation import InferenceParams
    model = tiny_path("inference").to(dev)
    lm = model.llm_backbone.mamba
    emb = torch.randn(1, 9, 32, device=dev)
    pool = lm.allocate_inference_cache(4, 64)
    for cs, ss in pool.values():
        cs.copy_(torch.randn(cs.shape)), ss.copy_(torch.randn(ss.shape))
    before = {k: (c.clone(), s.clone()) for k, (c, s) in pool.items()}
    own = InferenceParams(max_seqlen=64, max_batch_size=1, key_value_memory_dict=lm.allocate_inference_cache(1, 64))
    view = InferenceParams(max_seqlen=64, max_batch_size=1, key_value_memory_dict={k: (c[2:3], s[2:3]) for k, (c, s) in pool.items()})
    with torch.no_grad():
        l_own = lm(None, emb, task="mmu", inference_params=own, num_last_tokens=1).mmu_logits
        l_view = lm(None, emb, task="mmu", inference_params=view, num_last_tokens=1).mmu_logits
    assert torch.equal(l_own, l_view)
    for k, (c, s) in pool.items():
        oc, os_ = own.key_value_memory_dict[k]
        assert torch.equal(c[2], oc[0]) and torch.equal(s[2], os_[0])
        for slot in (0, 1, 3):
            assert torch.equal(c[slot], before[k][0][slot]) and torch.equal(s[slot], before[k][1][slot])


def _requests(dev, n, d_feat=12, seed=5):
    g = torch.Generator().manual_seed(seed)
    lens = [3, 12, 7, 5, 9, 4, 11][:n]
    qs = [torch.randint(0, 50, (1, L), generator=g).to(dev) for L in lens]
    feats = [torch.randn(1, 5, d_feat, generator=g).to(dev) for _ in range(n)]
    return feats, qs


def _separate(model):
    with torch.no_grad():     # well separated logits: argmax is robust (test_greedy_decode_trace_and_tokens)
        model.llm_backbone.mamba.backbone.embedding.weight.mul_(30.0)


def _equivalence(model, dev, feats, qs, max_lens, max_batch, cg):
    """mmu_generate_batch == mmu_generate per request (greedy), with an EOS that some requests hit and some do not."""
    free = [model.mmu_generate(f, q, max_length=L, cg=False) for f, q, L in zip(feats, qs, max_lens)]
    # the EOS: an id that one request samples early and that does not end every request at once
    gens = [s[0, 4 + q.shape[1]:].tolist() for s, q in zip(free, qs)]
    eos = next(t for t in (g[1] for g in gens if len(g) > 2) if sum(t in g for g in gens) < len(gens))
    want = [model.mmu_generate(f, q, max_length=L, eos_token_id=eos, cg=False) for f, q, L in zip(feats, qs, max_lens)]
    got = model.mmu_generate_batch(feats, qs, max_length=max_lens, eos_token_id=eos, max_batch=max_batch, cg=cg)
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert torch.equal(g, w), (i, g.tolist(), w.tolist())
    assert any(w.shape[1] < f.shape[1] for w, f in zip(want, free))          # some requests stopped at EOS ...
    assert any(w[0, -1] != eos for w in want)                                 # ... and some at their max_length
    return got


def test_mmu_generate_batch_equals_sequential(dev):
    torch.manual_seed(6)
    model = tiny_path("inference").to(dev)
    _separate(model)
    feats, qs = _requests(dev, 5)
    max_lens = [20, 30, 24, 27, 22]             # prompts: 4 + 5 image + 3..12 question positions
    _equivalence(model, dev, feats, qs, max_lens, max_batch=2, cg=False)
    c = model.llm_backbone.mamba._ragged_cache
    assert set(c["buckets"]) <= {1, 2} and 2 in c["buckets"]


def test_decode_ragged_position_table_raises(dev):
    """A request whose step would pass the position table raises IndexError as decode() does for it alone."""
    from omnimamba_amd.batch_decode import decode_ragged
    from omnimamba_amd.generation import decode
    torch.manual_seed(7)
    model = tiny_path("inference").to(dev)
    lm = model.llm_backbone.mamba
    n_pos = lm.cfg.mmu_positions
    ok = (torch.zeros(1, 3, dtype=torch.long, device=dev), torch.randn(1, 6, 32, device=dev))
    far = (torch.zeros(1, 3, dtype=torch.long, device=dev), torch.randn(1, n_pos - 1, 32, device=dev))
    with pytest.raises(IndexError):
        decode(*far, lm, n_pos + 2, top_k=1, task="mmu")
    with pytest.raises(IndexError):
        decode_ragged([ok, far], lm, [10, n_pos + 2], max_batch=2, cg=False)
    out = decode_ragged([ok, far], lm, [10, n_pos + 1], max_batch=2, cg=False)
    assert torch.equal(out[1], decode(*far, lm, n_pos + 1, top_k=1, task="mmu"))


def test_mmu_generate_batch_fused_conv_tail_with_indices(dev, monkeypatch):
    """d_model 1024: the step's add + norm + in_proj + conv update is one norm_linear launch, here with conv_state_indices."""
    from omnimamba_amd import norm_linear as NL
    from omnimamba_amd.omni import OmniMambaPath
    from omnimamba_amd.stack import StackConfig
    cfg = StackConfig(d_model=1024, n_layer=1, vocab_size=50, pad_vocab_size_multiple=16, vqvae_vocab_size=40, num_tokens=8,
                      t2i_positions=24, mmu_positions=40, ssm_cfg=dict(d_state=16, headdim=64, chunk_size=16), lora_dropout=0.0,
                      img_sq_len=5, fused_vision_dim=12)
    torch.manual_seed(8)
    model = OmniMambaPath(cfg, stage="inference", special_ids=TINY_SPECIAL).to(dev)
    _separate(model)
    seen = []
    real = NL.norm_linear

    def spy(*a, **k):
        seen.append(k.get("conv_state_indices") is not None and k.get("conv_state") is not None)
        return real(*a, **k)
    monkeypatch.setattr(NL, "norm_linear", spy)
    feats, qs = _requests(dev, 3, seed=9)
    _equivalence(model, dev, feats, qs, [17, 21, 19], max_batch=2, cg=False)
    assert any(seen)


@pytest.mark.gpu
def test_mmu_generate_batch_captured_equals_eager():
    dev = torch.device("cuda:0")
    torch.manual_seed(10)
    model = tiny_path("inference").to(dev)
    _separate(model)
    feats, qs = _requests(dev, 5)
    max_lens = [20, 30, 24, 27, 22]
    eager = model.mmu_generate_batch(feats, qs, max_length=max_lens, max_batch=2, cg=False)
    graphed = _equivalence(model, dev, feats, qs, max_lens, max_batch=2, cg=True)
    again = model.mmu_generate_batch(feats, qs, max_length=max_lens, max_batch=2, cg=True)   # the kept graphs replayed
    assert len(graphed) == 5 and all(torch.equal(e, a) for e, a in zip(eager, again))
    c = model.llm_backbone.mamba._ragged_cache
    assert c["cg"] and set(c["buckets"]) == {1, 2} and all(b.graph is not None for b in c["buckets"].values())
