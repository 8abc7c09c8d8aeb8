"""Constrained decoding in continuous batching (decode_ragged / mmu_generate_batch / mmu_continue with SamplingParams.logit_bias,
allowed_token_ids, banned_token_ids, min_new_tokens): the constraints reach every draw of a request -- its admission draw (prefill,
extend, grouped or not) and its steps -- through the row-wise launch, and change nothing for the requests that have none.  The tiny model
in fp32 (64 logits); the emulator on the CPU (eager), the MI355X under -m gpu (eager and captured).  Exact ids: the argument of
tests/test_batch_decode_sampling.py (fp32 logits, fewer than 200 draws at fixed seeds) holds here as it does there."""
import math
from dataclasses import replace

import pytest
import torch

from test_batch_decode_logprobs import _recorder
from test_batch_decode_sampling import MAX_LENS, _five_params, _setup
from test_token_logprobs import _check

SET_A, SET_B = (3, 17, 40, 41), (5, 6, 7, 8, 9, 33)


def _constrained():
    """The five settings of test_batch_decode_sampling, requests 1 and 3 with an allowed set (3 behind its repetition penalty, with a
    biased and a banned member), request 2 with a logit_bias and banned ids; 0 and 4 have no constraint."""
    p = _five_params()
    p[1] = replace(p[1], allowed_token_ids=SET_A)
    p[2] = replace(p[2], logit_bias={11: 4.0, 12: -3.0}, banned_token_ids=(1, 2))
    p[3] = replace(p[3], allowed_token_ids=SET_B, logit_bias={6: 2.5}, banned_token_ids=(9,))
    return p


def _gen(out, reqs):
    return [o[0, r[0].shape[1]:].tolist() for o, r in zip(out, reqs)]


def _company(dev, cg):
    from omnimamba_amd.batch_decode import decode_ragged
    model, lm, reqs = _setup(dev, 41)
    params = _constrained()
    alone = [decode_ragged([r], lm, L, max_batch=1, cg=False, sampling=p)[0] for r, L, p in zip(reqs, MAX_LENS, params)]
    gen = _gen(alone, reqs)
    assert set(gen[1]) <= set(SET_A) and set(gen[3]) <= set(SET_B) - {9} and not set(gen[2]) & {1, 2}
    assert len(set(gen[1])) > 1 and len(set(gen[3])) > 1, "one id only: the case does not show that the request still samples"
    for kw in (dict(max_batch=4), dict(max_batch=1), dict(max_batch=4, prefill_batch=2)):
        got = decode_ragged(reqs, lm, MAX_LENS, cg=cg, sampling=params, **kw)
        for i, (g, w) in enumerate(zip(got, alone)):
            assert torch.equal(g, w), (kw, i, g.tolist(), w.tolist())
    # the requests without constraints draw what they draw in the call without any constrained request
    free = decode_ragged(reqs, lm, MAX_LENS, max_batch=4, cg=cg, sampling=_five_params())
    assert torch.equal(free[0], alone[0]) and torch.equal(free[4], alone[4])
    assert not torch.equal(free[1], alone[1]) and not torch.equal(free[3], alone[3])


def test_an_allowed_set_holds_alone_and_in_company(dev):
    _company(dev, cg=False)


@pytest.mark.gpu
def test_an_allowed_set_holds_alone_and_in_company_captured():
    _company(torch.device("cuda:0"), cg=True)


def test_no_constraint_in_the_call_is_the_launch_without_edit_arrays(dev, monkeypatch):
    """If no request of the call has edits no edit array is passed: the launches are the parent's (omk_sample_rows_form 0 / 1); with a
    constrained request every draw of the call is the edit launch."""
    import omnimamba_amd.batch_decode as BD
    from omnimamba_amd.sampling import sample_rows_form
    model, lm, reqs = _setup(dev, 41)
    forms, rows0 = [], BD.sample_rows

    def sample_rows(lg, **kw):
        forms.append(("edit_ids" in kw, sample_rows_form(lg, **{k: v for k, v in kw.items()})))
        return rows0(lg, **kw)

    monkeypatch.setattr(BD, "sample_rows", sample_rows)
    BD.decode_ragged(reqs, lm, MAX_LENS, max_batch=4, cg=False, sampling=_five_params())
    assert forms and all(not e and f in (0, 1) for e, f in forms) and any(f == 1 for _, f in forms)
    del forms[:]
    BD.decode_ragged(reqs, lm, MAX_LENS, max_batch=4, cg=False, sampling=_constrained())
    assert forms and all(e and f == 2 for e, f in forms)


def test_min_new_tokens_bans_eos_for_the_first_ids(dev, monkeypatch):
    """eos_token_id = the id an unconstrained greedy run emits first; min_new_tokens = 3.  The first three ids are not EOS, the request
    ends the first time EOS is sampled from its fourth id on, and every id equals the reference loop over the recorded logits of the draw:
    apply_logit_edits (EOS banned while fewer than three ids are drawn), then sample_rows without edits."""
    import omnimamba_amd.batch_decode as BD
    from omnimamba_amd.sampling import SamplingParams as SP, apply_logit_edits, pack_rows, sample_rows
    model, lm, reqs = _setup(dev, 42)
    L = reqs[1][0].shape[1]
    eos = int(BD.decode_ragged([reqs[1]], lm, 40, max_batch=1, cg=False, sampling=SP())[0][0, L])
    assert BD.decode_ragged([reqs[1]], lm, 40, max_batch=1, cg=False, sampling=SP(), eos_token_id=eos)[0].shape[1] == L + 1
    with pytest.raises(ValueError):
        BD.decode_ragged([reqs[1]], lm, 40, max_batch=1, cg=False, sampling=SP(min_new_tokens=3))
    for p in (SP(min_new_tokens=3), SP(top_k=0, temperature=1.5, seed=7, min_new_tokens=3, logit_bias={eos: 8.0})):
        rec = _recorder(monkeypatch)
        got = BD.decode_ragged([reqs[1]], lm, 40, max_batch=1, cg=False, sampling=p, eos_token_id=eos)[0]
        monkeypatch.undo()
        ids = got[0, L:].tolist()
        assert len(ids) == len(rec) >= 4 and eos not in ids[:3]
        assert eos not in ids[3:-1] and (ids[-1] == eos or len(ids) == 40 - reqs[1][1].shape[1])
        bias = [i for i, _ in p.logit_bias]
        for n, r in enumerate(rec):
            ban = n < 3
            lst = ([(eos, -math.inf)] if ban else []) + [(i, v) for i, v in p.logit_bias if not (ban and i == eos)]
            e_ids = torch.tensor([[i for i, _ in lst] + [0] * (2 - len(lst))], dtype=torch.int64).to(dev)
            e_vals = torch.tensor([[v for _, v in lst] + [0.0] * (2 - len(lst))], dtype=torch.float32).to(dev)
            work = apply_logit_edits(r["logits"], e_ids, e_vals, torch.tensor([len(lst)], dtype=torch.int32).to(dev))
            pk = pack_rows([replace(p, step0=n)], dev)
            pk.pop("penalty")
            assert int(sample_rows(work, **pk)[0]) == ids[n], (n, ids)
        if bias:
            assert ids[-1] == eos, "the biased EOS was never drawn: the case does not show the end of the ban"
    # in company: requests whose ban ends at different steps (the fifth is admitted later), each as alone
    params = [replace(p, min_new_tokens=m, logit_bias={eos: 2.0}) for p, m in zip(_five_params(), (3, 0, 5, 2, 4))]
    alone = [BD.decode_ragged([r], lm, Lm, max_batch=1, cg=False, sampling=p, eos_token_id=eos)[0] for r, Lm, p in zip(reqs, MAX_LENS, params)]
    got = BD.decode_ragged(reqs, lm, MAX_LENS, max_batch=4, cg=False, sampling=params, eos_token_id=eos, prefill_batch=2)
    for i, (g, w, p) in enumerate(zip(got, alone, params)):
        assert torch.equal(g, w), (i, g.tolist(), w.tolist())
        assert eos not in _gen([g], [reqs[i]])[0][:p.min_new_tokens]


def test_logprobs_stay_those_of_the_raw_logits(dev, monkeypatch):
    """The arg max of a greedy request banned, logprobs=0: the first record has rank 2, and every logprob is the raw log_softmax value at the
    sampled id under the bound of tests/test_token_logprobs.py (the fp64 reference of the recorded logits)."""
    import omnimamba_amd.batch_decode as BD
    from omnimamba_amd.sampling import SamplingParams as SP, TokenLogprobs
    model, lm, reqs = _setup(dev, 43)
    L = reqs[2][0].shape[1]
    top = int(BD.decode_ragged([reqs[2]], lm, 24, max_batch=1, cg=False, sampling=SP())[0][0, L])
    rec = _recorder(monkeypatch)
    out, recs = BD.decode_ragged([reqs[2]], lm, 24, max_batch=1, cg=False, sampling=SP(banned_token_ids=[top]), logprobs=0)
    ids = out[0][0, L:].cpu()
    assert top not in ids.tolist() and len(rec) == ids.numel()
    x = torch.cat([r["logits"][:1] for r in rec]).cpu()
    assert int(x[0].argmax()) == top and int(recs[0].rank[0]) == 2
    _check(x, ids, 0, TokenLogprobs(logprob=recs[0].logprob, rank=recs[0].rank), "banned arg max")


def test_a_continued_request_and_a_grouped_extend_honour_the_constraints(dev):
    """The second turn of five conversations: the admission draw of an extend (one by one, and two at a time) is constrained like every
    other draw, through decode_ragged and through OmniMambaPath.mmu_continue."""
    from omnimamba_amd.batch_decode import decode_ragged
    model, lm, reqs = _setup(dev, 44)
    params = _five_params()
    one, states = decode_ragged(reqs, lm, MAX_LENS, max_batch=4, cg=False, sampling=params, return_states=True)
    g = torch.Generator().manual_seed(23)
    turns = [torch.randint(0, 50, (1, L), generator=g).to(dev) for L in (4, 2, 6, 3, 5)]
    reqs2 = [(q, model.llm_backbone.embed_input_ids(q), st) for q, st in zip(turns, states)]
    cons = _constrained()
    params2 = [replace(p, step0=o.shape[1] - r[0].shape[1]) for p, o, r in zip(cons, one, reqs)]
    lens2 = [st.seqlen + 1 + q.shape[1] + 6 for st, q in zip(states, turns)]
    free2 = decode_ragged(reqs2, lm, lens2, max_batch=4, cg=False, sampling=[replace(p, step0=q.step0) for p, q in zip(params, params2)])
    one2 = decode_ragged(reqs2, lm, lens2, max_batch=4, cg=False, sampling=params2)
    grouped2 = decode_ragged(reqs2, lm, lens2, max_batch=4, cg=False, sampling=params2, extend_batch=2)
    for i, (g_, w) in enumerate(zip(grouped2, one2)):
        assert torch.equal(g_, w), (i, g_.tolist(), w.tolist())
    gen = _gen(one2, reqs2)
    assert all(len(x) >= 2 for x in gen)
    assert set(gen[1]) <= set(SET_A) and set(gen[3]) <= set(SET_B) - {9} and not set(gen[2]) & {1, 2}
    assert torch.equal(one2[0], free2[0]) and torch.equal(one2[4], free2[4])
    assert _gen(free2, reqs2)[1][0] not in SET_A or _gen(free2, reqs2)[3][0] not in SET_B, "the admission draws are in the sets without them"
    ids, _ = model.mmu_continue(states, turns, max_length=lens2, max_batch=4, cg=False, extend_batch=2, sampling=params2)
    for i, (a, w) in enumerate(zip(ids, one2)):
        assert torch.equal(a, w), i
