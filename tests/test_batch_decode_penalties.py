"""Presence and frequency penalties in continuous batching (decode_ragged / mmu_generate_batch / mmu_continue with
SamplingParams.presence_penalty / frequency_penalty): every draw of a call that has such a request carries the rows' penalties and the
start of their counted range, the fused path (sampling.penalty_edits + the edit launch) while the lists fit, a torch-edited copy past that.
The tiny model in fp32 (64 logits); the emulator on the CPU (eager), the MI355X under -m gpu (eager and captured).  Exact ids: the argument
of tests/test_batch_decode_sampling.py (fp32 logits, fewer than 200 draws at fixed seeds) holds here as it does there.

The oracle of every test is a host loop over the RECORDED logits of the draws: per draw and row, apply_logit_edits with the request's
history so far (its input_ids + the ids it sampled, counted from the end of input_ids), then the plain one-row launch."""
from dataclasses import replace

import pytest
import torch

from test_batch_decode_sampling import MAX_LENS, _setup

EOS = 7


def _mixed():
    """none | presence only | frequency only (greedy) | both behind a repetition penalty | both with a logit_bias and min_new_tokens"""
    from omnimamba_amd.sampling import SamplingParams as SP
    return [SP(top_k=8, seed=101),
            SP(top_k=0, seed=202, presence_penalty=1.5),
            SP(top_k=1, frequency_penalty=0.8),
            SP(top_k=20, seed=303, repetition_penalty=1.3, presence_penalty=0.7, frequency_penalty=0.4),
            SP(top_k=0, temperature=1.5, seed=404, presence_penalty=-0.5, frequency_penalty=0.3, logit_bias={11: 2.0, 12: -3.0}, min_new_tokens=3)]


def _record(monkeypatch):
    """Every row-wise draw of batch_decode: the logits it was given and its keyword arguments' seeds and active flags."""
    import omnimamba_amd.batch_decode as BD
    rec, draw0 = [], BD._RowSampler._draw

    def _draw(self, logits, kw, reqs, merged=None):
        rec.append({"logits": logits.clone(), "seeds": kw["seeds"].clone(), "active": None if kw.get("active") is None else kw["active"].clone()})
        return draw0(self, logits, kw, reqs, merged)

    monkeypatch.setattr(BD._RowSampler, "_draw", _draw)
    return rec


def _host_loop(rec, reqs, params, got, dev, eos=EOS):
    """Checks every id of `got` against the statement; returns the number of ids checked."""
    from omnimamba_amd.sampling import _signed64, apply_logit_edits, pack_count_penalties, pack_edits, pack_rows, sample_rows
    by_seed = {_signed64(p.seed): i for i, p in enumerate(params)}
    assert len(by_seed) == len(params)
    drawn = [0] * len(params)
    for r in rec:
        rows = range(r["logits"].shape[0]) if r["active"] is None else [b for b, a in enumerate(r["active"].tolist()) if a]
        for b in rows:
            i = by_seed[int(r["seeds"][b])]
            p, L, n = params[i], reqs[i][0].shape[1], drawn[i]
            hist = got[i][:, :L + n].to(dev)
            if hist.shape[1] == 0:
                hist = torch.zeros(1, 1, dtype=torch.int64, device=dev)
            ed = pack_edits([p], dev, [[eos] if n < p.min_new_tokens else []])
            pk = pack_rows([replace(p, step0=p.step0 + n)], dev)
            work = apply_logit_edits(r["logits"][b:b + 1], **ed, penalty=pk.pop("penalty"), history=hist,
                                     history_lens=torch.tensor([L + n], dtype=torch.int32, device=dev), **pack_count_penalties([p], dev),
                                     count_start=torch.tensor([L], dtype=torch.int32, device=dev))
            want = int(sample_rows(work, **pk)[0])
            assert want == int(got[i][0, L + n]), (i, n, want, got[i][0, L:].tolist())
            drawn[i] += 1
    assert drawn == [g.shape[1] - r[0].shape[1] for g, r in zip(got, reqs)]
    return sum(drawn)


def _step_by_step(dev, cg, monkeypatch):
    import omnimamba_amd.batch_decode as BD
    import omnimamba_amd.sampling as S
    model, lm, reqs = _setup(dev, 51)
    params = _mixed()
    launches, pe0 = [], S.penalty_edits
    monkeypatch.setattr(S, "penalty_edits", lambda *a, **k: launches.append(1) or pe0(*a, **k))
    rec = _record(monkeypatch)
    got = BD.decode_ragged(reqs, lm, MAX_LENS, max_batch=4, cg=cg, sampling=params, eos_token_id=EOS)
    assert len(launches) == len(rec) > 5, "every draw of the call takes the fused path"
    assert _host_loop(rec, reqs, params, got, dev) >= 30
    monkeypatch.undo()
    return reqs, lm, params, got


def test_every_id_equals_the_statement_applied_to_the_draws_logits(dev, monkeypatch):
    reqs, lm, params, got = _step_by_step(dev, False, monkeypatch)
    # the penalties change what is drawn (the request without any draws what it draws in a call without penalties)
    from omnimamba_amd.batch_decode import decode_ragged
    off = decode_ragged(reqs, lm, MAX_LENS, max_batch=4, cg=False, eos_token_id=EOS,
                        sampling=[replace(p, presence_penalty=0.0, frequency_penalty=0.0) for p in params])
    assert torch.equal(off[0], got[0]) and sum(not torch.equal(a, b) for a, b in zip(off[1:], got[1:])) >= 2


@pytest.mark.gpu
def test_every_id_equals_the_statement_applied_to_the_draws_logits_captured(monkeypatch):
    _step_by_step(torch.device("cuda:0"), True, monkeypatch)


def test_a_requests_ids_are_the_same_alone_and_in_any_batch(dev):
    from omnimamba_amd.batch_decode import decode_ragged
    model, lm, reqs = _setup(dev, 52)
    params = _mixed()
    alone = [decode_ragged([r], lm, L, max_batch=1, cg=False, sampling=p, eos_token_id=EOS)[0] for r, L, p in zip(reqs, MAX_LENS, params)]
    for kw in (dict(max_batch=4), dict(max_batch=1), dict(max_batch=4, prefill_batch=2)):
        got = decode_ragged(reqs, lm, MAX_LENS, cg=False, sampling=params, eos_token_id=EOS, **kw)
        for i, (g, w) in enumerate(zip(got, alone)):
            assert torch.equal(g, w), (kw, i, g.tolist(), w.tolist())
    rev = decode_ragged(reqs[::-1], lm, MAX_LENS[::-1], max_batch=4, cg=False, sampling=params[::-1], eos_token_id=EOS)
    for i, (g, w) in enumerate(zip(rev[::-1], alone)):
        assert torch.equal(g, w), (i, g.tolist(), w.tolist())


def test_the_ids_do_not_change_where_a_call_crosses_to_the_copy_path(dev, monkeypatch):
    """PENALTY_FUSED_MAX lowered to 8: with a user width of 3 (two biases and the EOS ban) the draws are fused until a request of the draw
    has sampled 5 ids, and edit a copy from then on."""
    import omnimamba_amd.batch_decode as BD
    import omnimamba_amd.sampling as S
    model, lm, reqs = _setup(dev, 53)
    params = _mixed()
    want = BD.decode_ragged(reqs, lm, MAX_LENS, max_batch=4, cg=False, sampling=params, eos_token_id=EOS)
    fused, copies, pe0, ale0 = [], [], S.penalty_edits, BD.apply_logit_edits
    monkeypatch.setattr(S, "penalty_edits", lambda *a, **k: fused.append(1) or pe0(*a, **k))
    monkeypatch.setattr(BD, "apply_logit_edits", lambda *a, **k: copies.append(1) or ale0(*a, **k))
    BD.decode_ragged(reqs, lm, MAX_LENS, max_batch=4, cg=False, sampling=params, eos_token_id=EOS)
    assert fused and not copies
    del fused[:]
    monkeypatch.setattr(BD, "PENALTY_FUSED_MAX", 8)
    rec = _record(monkeypatch)
    got = BD.decode_ragged(reqs, lm, MAX_LENS, max_batch=4, cg=False, sampling=params, eos_token_id=EOS)
    assert len(fused) >= 3 and len(copies) >= 3 and len(fused) + len(copies) == len(rec)
    for i, (g, w) in enumerate(zip(got, want)):
        assert torch.equal(g, w), (i, g.tolist(), w.tolist())


def test_a_follow_up_turn_counts_only_the_ids_of_its_own_call(dev, monkeypatch):
    """mmu_generate_batch, then mmu_continue on its states: the second turn's counted range starts behind the turn's own input_ids, so the
    ids the first turn sampled carry no penalty (the host loop knows nothing of them and reproduces every id)."""
    model, lm, reqs = _setup(dev, 54)
    from test_batch_decode import _requests
    feats, qs = _requests(dev, 5)
    params = [replace(p, min_new_tokens=0) for p in _mixed()]
    one, states = model.mmu_generate_batch(feats, qs, max_length=MAX_LENS, max_batch=4, cg=False, sampling=params, return_states=True)
    g = torch.Generator().manual_seed(23)
    turns = [torch.randint(0, 50, (1, L), generator=g).to(dev) for L in (4, 2, 6, 3, 5)]
    params2 = [replace(p, step0=o.shape[1] - 4 - q.shape[1]) for p, o, q in zip(params, one, qs)]
    assert all(p.step0 > 0 for p in params2)
    lens2 = [st.seqlen + 1 + q.shape[1] + 8 for st, q in zip(states, turns)]
    rec = _record(monkeypatch)
    got, _ = model.mmu_continue(states, turns, max_length=lens2, max_batch=4, cg=False, sampling=params2, extend_batch=2)
    reqs2 = [(q,) for q in turns]
    assert _host_loop(rec, reqs2, params2, got, dev) >= 30


def test_penalties_off_is_the_call_without_the_fields(dev, monkeypatch):
    """Both penalties 0 in every request: no history is owned for them, no penalty_edits launch, no extra keyword reaches sample_rows -- the
    ids of the same call with SamplingParams that never heard of the fields."""
    import omnimamba_amd.batch_decode as BD
    import omnimamba_amd.sampling as S
    from test_batch_decode_sampling import _five_params
    model, lm, reqs = _setup(dev, 55)
    params = _five_params()
    want = BD.decode_ragged(reqs, lm, MAX_LENS, max_batch=4, cg=False, sampling=params)
    seen, rows0 = [], BD.sample_rows
    monkeypatch.setattr(BD, "sample_rows", lambda lg, **kw: seen.append(set(kw)) or rows0(lg, **kw))
    monkeypatch.setattr(S, "penalty_edits", lambda *a, **k: pytest.fail("penalty_edits launched without a penalty"))
    got = BD.decode_ragged(reqs, lm, MAX_LENS, max_batch=4, cg=False, sampling=[replace(p, presence_penalty=0.0, frequency_penalty=0.0) for p in params])
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    assert seen and not any(k & {"frequency", "presence", "count_start", "count_max", "merged"} for k in seen)
