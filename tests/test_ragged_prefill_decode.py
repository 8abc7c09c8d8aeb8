"""decode_ragged / mmu_generate_batch with batched admission (prefill_batch) and bucketed prefill graphs (prefill_bucket): the result
contract is unchanged -- per request exactly what mmu_generate returns for it alone (greedy, well separated logits as in
tests/test_batch_decode.py).  Emulator on CPU (eager); MI355X under -m gpu (eager and captured)."""
import pytest
import torch

from test_batch_decode import _requests, _separate
from test_stack_decode_train import tiny_path

MAX_LENS = [20, 30, 24, 27, 22, 21, 29]     # prompts: 4 + 5 image + 3, 12, 7, 5, 9, 4, 11 question positions


def _eos_and_want(model, feats, qs, max_lens):
    """test_batch_decode._equivalence's choice of an EOS that some requests hit and some do not, and mmu_generate of each request alone."""
    free = [model.mmu_generate(f, q, max_length=L, cg=False) for f, q, L in zip(feats, qs, max_lens)]
    gens = [s[0, 4 + q.shape[1]:].tolist() for s, q in zip(free, qs)]
    eos = next(t for t in (g[1] for g in gens if len(g) > 2) if sum(t in g for g in gens) < len(gens))
    want = [model.mmu_generate(f, q, max_length=L, eos_token_id=eos, cg=False) for f, q, L in zip(feats, qs, max_lens)]
    assert any(w.shape[1] < f.shape[1] for w, f in zip(want, free)) and any(w[0, -1] != eos for w in want)
    return eos, want


def test_batched_admission_equals_sequential(dev, monkeypatch):
    from omnimamba_amd import batch_decode as BD
    torch.manual_seed(6)
    model = tiny_path("inference").to(dev)
    _separate(model)
    lm = model.llm_backbone.mamba
    feats, qs = _requests(dev, 7)
    eos, want = _eos_and_want(model, feats, qs, MAX_LENS)
    prefill_batches, groups, checked = [], [], []
    real_fwd, real_grp = lm.forward, BD._prefill_group

    def fwd(input_ids, input_embeddings, *a, **k):
        ip = k.get("inference_params")
        if input_embeddings is not None and ip is not None and ip.seqlen_offset == 0:
            prefill_batches.append(input_embeddings.shape[0])
        return real_fwd(input_ids, input_embeddings, *a, **k)

    def grp(model_, c, slots, embs, task):
        if not groups:                                      # the opening burst: every slot is free -- a sentinel in all of them
            for v in c["pool"].values():
                for t in v:
                    t.fill_(7.0)
        before = {k: tuple(t.clone() for t in v) for k, v in c["pool"].items()}
        out = real_grp(model_, c, slots, embs, task)
        others = [s for s in range(c["max_batch"]) if s not in slots]
        for k, v in c["pool"].items():
            for t, t0 in zip(v, before[k]):
                assert torch.equal(t[others], t0[others]), "a slot outside the admitted group changed"
                assert not any(torch.equal(t[s], t0[s]) for s in slots), "an admitted slot was not written"
        groups.append(list(slots))
        checked.append(len(others))
        return out

    monkeypatch.setattr(lm, "forward", fwd)
    monkeypatch.setattr(BD, "_prefill_group", grp)
    # six slots, groups of up to four: the opening burst takes slots 0 - 3 next to two free (sentinel) slots, the next group slots
    # 4 - 5 next to live ones
    got = model.mmu_generate_batch(feats, qs, max_length=MAX_LENS, eos_token_id=eos, max_batch=6, cg=False, prefill_batch=4)
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert torch.equal(g, w), (i, g.tolist(), w.tolist())
    assert max(prefill_batches) > 1 and groups[0] == [0, 1, 2, 3] and len(groups) >= 2 and {4, 5} <= set(groups[1]), (prefill_batches, groups)
    # the slots that had to stay as they were: two sentinel slots beside the first group, live ones beside the second (it also takes
    # any slot a request of the first group gave back by ending on its first id) -- never an empty comparison
    assert checked[0] == 2 and min(checked) > 0, checked
    # the same with every slot taken by the group (issue: prefill_batch=4, max_batch=4)
    groups.clear()
    got4 = model.mmu_generate_batch(feats, qs, max_length=MAX_LENS, eos_token_id=eos, max_batch=4, cg=False, prefill_batch=4)
    assert all(torch.equal(g, w) for g, w in zip(got4, want)) and groups[0] == [0, 1, 2, 3]
    # the defaults take no group
    prefill_batches.clear(), groups.clear()
    again = model.mmu_generate_batch(feats, qs, max_length=MAX_LENS, eos_token_id=eos, max_batch=4, cg=False)
    assert all(torch.equal(a, w) for a, w in zip(again, want)) and set(prefill_batches) == {1} and not groups


def test_batched_admission_states_continue_like_the_default_path(dev):
    from test_mmu_continue import conversations, model_on
    model = model_on(dev)
    n = 5
    feats, q1, q2 = conversations(dev, n)
    max1 = [26, 30, 28, 25, 32]
    eos, _ = _eos_and_want(model, feats, q1, max1)
    max2 = [m + 30 + q.shape[1] for m, q in zip(max1, q2)]
    turns = {}
    for pb in (1, 4):
        ids1, st1 = model.mmu_generate_batch(feats, q1, max_length=max1, eos_token_id=eos, max_batch=4, cg=False, return_states=True,
                                             prefill_batch=pb)
        ids2, st2 = model.mmu_continue(st1, q2, max_length=max2, eos_token_id=eos, max_batch=4, cg=False, prefill_batch=pb)
        turns[pb] = (ids1, st1, ids2, st2)
    for i in range(n):
        assert torch.equal(turns[4][0][i], turns[1][0][i]) and torch.equal(turns[4][2][i], turns[1][2][i]), i
        assert (turns[4][1][i].seqlen, turns[4][1][i].pending_id) == (turns[1][1][i].seqlen, turns[1][1][i].pending_id)
        assert (turns[4][3][i].seqlen, turns[4][3][i].pending_id) == (turns[1][3][i].seqlen, turns[1][3][i].pending_id)


def test_position_table_contract_holds_with_batched_admission(dev):
    """tests/test_batch_decode.py::test_decode_ragged_position_table_raises with prefill_batch=2."""
    from omnimamba_amd.batch_decode import decode_ragged
    from omnimamba_amd.generation import decode
    torch.manual_seed(7)
    model = tiny_path("inference").to(dev)
    lm = model.llm_backbone.mamba
    n_pos = lm.cfg.mmu_positions
    ok = (torch.zeros(1, 3, dtype=torch.long, device=dev), torch.randn(1, 6, 32, device=dev))
    far = (torch.zeros(1, 3, dtype=torch.long, device=dev), torch.randn(1, n_pos - 1, 32, device=dev))
    with pytest.raises(IndexError):
        decode_ragged([ok, far], lm, [10, n_pos + 2], max_batch=2, cg=False, prefill_batch=2)
    out = decode_ragged([ok, far], lm, [10, n_pos + 1], max_batch=2, cg=False, prefill_batch=2)
    assert torch.equal(out[1], decode(*far, lm, n_pos + 1, top_k=1, task="mmu"))
    assert torch.equal(out[0], decode(*ok, lm, 10, top_k=1, task="mmu"))


def test_bucket_length_rule():
    """ceil(P / bucket) * bucket for prompts past the exact-length capture limit, clamped to the position table; a prompt that does not
    fit the clamped bucket, a short prompt and bucket 0 take no bucket graph."""
    from omnimamba_amd import generation as G
    from omnimamba_amd.batch_decode import _bucket_len
    assert G.PREFILL_GRAPH_MAX_LEN == 512 and G._prefill_graph_ok(512) and not G._prefill_graph_ok(513)
    assert _bucket_len(853, 128, 1500) == 896 and _bucket_len(741, 128, 1500) == 768 and _bucket_len(896, 128, 1500) == 896
    assert _bucket_len(1450, 128, 1500) == 1500 and _bucket_len(1500, 128, 1500) == 1500 and _bucket_len(1501, 128, 1500) == 0
    assert _bucket_len(512, 128, 1500) == 0 and _bucket_len(853, 0, 1500) == 0 and _bucket_len(853, 128, None) == 896


def test_invalid_arguments_raise(dev):
    from omnimamba_amd.batch_decode import decode_ragged
    model = tiny_path("inference").to(dev)
    req = [(torch.zeros(1, 3, dtype=torch.long, device=dev), torch.randn(1, 6, 32, device=dev))]
    with pytest.raises(ValueError):
        decode_ragged(req, model.llm_backbone.mamba, 10, cg=False, prefill_batch=0)
    with pytest.raises(ValueError):
        decode_ragged(req, model.llm_backbone.mamba, 10, cg=False, prefill_bucket=-1)


@pytest.mark.gpu
def test_bucketed_prefill_graphs():
    """cg=True, prefill_bucket=16 with the exact-length capture limit lowered to 8 positions, so that every prompt of the tiny model
    (12 .. 21 positions) takes a bucket: ids equal to the eager run, prompts of different lengths inside one bucket replay ONE graph,
    and a second call replays the kept graphs."""
    from omnimamba_amd import generation as G
    dev = torch.device("cuda:0")
    torch.manual_seed(10)
    model = tiny_path("inference").to(dev)
    _separate(model)
    feats, qs = _requests(dev, 7)
    eager = model.mmu_generate_batch(feats, qs, max_length=MAX_LENS, max_batch=2, cg=False)
    mp = pytest.MonkeyPatch()
    try:
        mp.setattr(G, "PREFILL_GRAPH_MAX_LEN", 8)
        graphed = model.mmu_generate_batch(feats, qs, max_length=MAX_LENS, max_batch=2, cg=True, prefill_bucket=16)
        c = model.llm_backbone.mamba._ragged_cache
        keys = list(c["prefill"])
        # prompts of 12, 13, 14, 16 positions -> bucket 16; 18, 20, 21 -> bucket 32: two graphs for seven prompts of seven lengths
        assert sorted(k[0] for k in keys) == [16, 32] and all(k[2] == "bucket" for k in keys), keys
        kept = {k: c["prefill"][k] for k in keys}
        again = model.mmu_generate_batch(feats, qs, max_length=MAX_LENS, max_batch=2, cg=True, prefill_bucket=16)
        c2 = model.llm_backbone.mamba._ragged_cache
        assert c2 is c and all(c["prefill"][k] is kept[k] for k in keys) and len(c["prefill"]) == 2
    finally:
        mp.undo()
    for e, g, a in zip(eager, graphed, again):
        assert torch.equal(e, g) and torch.equal(e, a)
    # a bucket that would pass the position table (40 rows): clamped to it, and batched admission composes with the graphs
    mp = pytest.MonkeyPatch()
    try:
        mp.setattr(G, "PREFILL_GRAPH_MAX_LEN", 8)
        both = model.mmu_generate_batch(feats, qs, max_length=MAX_LENS, max_batch=4, cg=True, prefill_bucket=64, prefill_batch=4)
        assert 40 in [k[0] for k in model.llm_backbone.mamba._ragged_cache["prefill"]]
    finally:
        mp.undo()
    for e, b in zip(eager, both):
        assert torch.equal(e, b)
