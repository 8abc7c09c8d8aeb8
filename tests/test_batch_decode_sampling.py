"""Per-request sampling in continuous batching (decode_ragged / mmu_generate_batch with sampling=...): every request is sampled with
its own SamplingParams through the row-wise launch, and its ids depend on nothing but the request -- not on the requests it shares its
steps with, on max_batch, on the admission order or on grouped admission.  The tiny model in fp32; the emulator on the CPU (eager), the
MI355X under -m gpu (eager and captured)."""
import pytest
import torch

from test_batch_decode import _equivalence, _requests, _separate
from test_stack_decode_train import tiny_path

MAX_LENS = [20, 30, 24, 27, 22]             # prompts: 4 + 5 image + 3..12 question positions


def _five_params():
    from omnimamba_amd.sampling import SamplingParams as SP
    return [SP(), SP(top_k=8, seed=101), SP(top_k=0, top_p=0.9, seed=202), SP(top_k=20, repetition_penalty=1.3, seed=303),
            SP(top_k=0, min_p=0.05, temperature=1.5, seed=404)]


def _setup(dev, seed):
    torch.manual_seed(seed)
    model = tiny_path("inference").to(dev)
    feats, qs = _requests(dev, 5)
    reqs = [model._mmu_prompt(f, q) for f, q in zip(feats, qs)]
    return model, model.llm_backbone.mamba, reqs


def _alone(lm, reqs, max_lens, params, **kw):
    from omnimamba_amd.batch_decode import decode_ragged
    return [decode_ragged([r], lm, L, max_batch=1, cg=False, sampling=p, **kw) for r, L, p in zip(reqs, max_lens, params)]


def _company(dev, cg):
    from omnimamba_amd.batch_decode import decode_ragged
    model, lm, reqs = _setup(dev, 21)
    params = _five_params()
    alone = [a[0] for a in _alone(lm, reqs, MAX_LENS, params)]
    greedy = decode_ragged(reqs, lm, MAX_LENS, max_batch=4, cg=False)
    got = decode_ragged(reqs, lm, MAX_LENS, max_batch=4, cg=cg, sampling=params)
    for i, (g, w) in enumerate(zip(got, alone)):
        assert torch.equal(g, w), (i, g.tolist(), w.tolist())
    rev = decode_ragged(reqs[::-1], lm, MAX_LENS[::-1], max_batch=4, cg=cg, sampling=params[::-1])
    for i, (g, w) in enumerate(zip(rev[::-1], alone)):
        assert torch.equal(g, w), (i, g.tolist(), w.tolist())
    assert torch.equal(got[0], greedy[0])                                         # SamplingParams() is greedy
    assert sum(not torch.equal(g, w) for g, w in zip(got[1:], greedy[1:])) >= 3   # ... and the others do sample
    assert sum(g.shape[1] - r[0].shape[1] for g, r in zip(got, reqs)) < 200       # (the number of draws the exactness argument covers)


def test_a_requests_ids_do_not_depend_on_its_company(dev):
    """Five requests with five different settings through max_batch = 4 (buckets 1, 2, 4; the fifth request waits for a slot) give, per
    request, the ids of that request decoded alone with its params; so does the reversed request list.  The step kernels of one and of
    several sequences differ in the last bits of the logits; with fp32 logits, fewer than 200 draws and a 24-bit uniform no draw of these
    fixed seeds falls that close to a boundary of its CDF: exact ids, no tolerance."""
    _company(dev, cg=False)


@pytest.mark.gpu
def test_a_requests_ids_do_not_depend_on_its_company_captured():
    _company(torch.device("cuda:0"), cg=True)


def test_grouped_admission_gives_the_same_ids(dev):
    """prefill_batch = 4 and extend_batch = 4: the first ids of a group come from one row-wise launch over the group's rows, and equal
    those of request-by-request admission.  The second turn continues each stream at step0 = the ids the first turn sampled."""
    from dataclasses import replace
    from omnimamba_amd.batch_decode import decode_ragged
    model, lm, reqs = _setup(dev, 22)
    params = _five_params()
    one, states = decode_ragged(reqs, lm, MAX_LENS, max_batch=4, cg=False, sampling=params, return_states=True)
    grouped = decode_ragged(reqs, lm, MAX_LENS, max_batch=4, cg=False, sampling=params, prefill_batch=4)
    for i, (g, w) in enumerate(zip(grouped, one)):
        assert torch.equal(g, w), (i, g.tolist(), w.tolist())
    g = torch.Generator().manual_seed(23)
    turns = [torch.randint(0, 50, (1, L), generator=g).to(dev) for L in (4, 2, 6, 3, 5)]
    reqs2 = [(q, model.llm_backbone.embed_input_ids(q), st) for q, st in zip(turns, states)]
    params2 = [replace(p, step0=o.shape[1] - r[0].shape[1]) for p, o, r in zip(params, one, reqs)]
    assert all(p.step0 > 0 for p in params2)
    lens2 = [st.seqlen + 1 + q.shape[1] + 6 for st, q in zip(states, turns)]
    one2 = decode_ragged(reqs2, lm, lens2, max_batch=4, cg=False, sampling=params2)
    grouped2 = decode_ragged(reqs2, lm, lens2, max_batch=4, cg=False, sampling=params2, extend_batch=4)
    for i, (g_, w) in enumerate(zip(grouped2, one2)):
        assert torch.equal(g_, w), (i, g_.tolist(), w.tolist())
    # the stream position matters: the same turn drawn from step 0 again is another draw somewhere
    again = decode_ragged(reqs2, lm, lens2, max_batch=4, cg=False, sampling=params)
    assert any(not torch.equal(a, w) for a, w in zip(again[1:], one2[1:]))


def test_sampling_none_is_unchanged_and_default_params_are_greedy(dev):
    """Without `sampling` decode_ragged is the code it was: greedy mmu_generate_batch equals mmu_generate per request
    (test_batch_decode.test_mmu_generate_batch_equals_sequential); one SamplingParams() for all requests gives the same ids."""
    from omnimamba_amd.sampling import SamplingParams
    torch.manual_seed(6)
    model = tiny_path("inference").to(dev)
    _separate(model)
    feats, qs = _requests(dev, 5)
    got = _equivalence(model, dev, feats, qs, MAX_LENS, max_batch=2, cg=False)
    free = model.mmu_generate_batch(feats, qs, max_length=MAX_LENS, max_batch=2, cg=False)
    same = model.mmu_generate_batch(feats, qs, max_length=MAX_LENS, max_batch=2, cg=False, sampling=SamplingParams())
    assert len(got) == 5 and all(torch.equal(a, b) for a, b in zip(free, same))
    with pytest.raises(ValueError):
        model.mmu_generate_batch(feats, qs, max_length=MAX_LENS, max_batch=2, cg=False, sampling=[SamplingParams()] * 4)


def test_penalty_history_equals_decode_alone(dev):
    """repetition_penalty 1.5 with top_k 1: the ids of generation.decode(..., repetition_penalty=1.5, top_k=1) for the request alone (greedy:
    exact whatever the stream).  decode() returns every sampled id twice under a penalty, as the reference does; the slot's history holds
    it once -- duplicates are penalised once, so the ids agree."""
    from omnimamba_amd.batch_decode import decode_ragged
    from omnimamba_amd.generation import decode
    from omnimamba_amd.sampling import SamplingParams
    model, lm, reqs = _setup(dev, 24)
    ids, emb = reqs[1]
    want = decode(ids, emb, lm, 40, top_k=1, repetition_penalty=1.5, task="mmu")
    plain = decode(ids, emb, lm, 40, top_k=1, task="mmu")
    L = ids.shape[1]
    sampled = want[0, L:]
    assert torch.equal(sampled[0::2], sampled[1::2])
    assert not torch.equal(sampled[0::2], plain[0, L:]), "the penalty changes nothing here: the case does not test it"
    got = decode_ragged([reqs[1]], lm, 40, max_batch=1, cg=False, sampling=SamplingParams(top_k=1, repetition_penalty=1.5))[0]
    assert torch.equal(got[0, :L], ids[0]) and torch.equal(got[0, L:], sampled[0::2]), (got[0, L:].tolist(), sampled[0::2].tolist())
    # ... and among other requests, in a step of four
    others = [SamplingParams(top_k=8, seed=5), SamplingParams(top_k=1, repetition_penalty=1.5), SamplingParams(top_k=0, seed=6), SamplingParams()]
    got4 = decode_ragged([reqs[0], reqs[1], reqs[2], reqs[3]], lm, [20, 40, 24, 27], max_batch=4, cg=False, sampling=others)
    assert torch.equal(got4[1], got)
