"""Token log-probabilities in continuous batching (decode_ragged / mmu_generate_batch / mmu_continue with logprobs=...): every draw is
followed by one sampling.token_logprobs launch, and every request gets a record aligned with its sampled ids.

The inputs of every draw are RECORDED: a wrapper over batch_decode.sample and batch_decode.sample_rows keeps a clone of the logits and of
the ids of each call.  A request's record must equal the fp64 reference (test_token_logprobs._reference) of exactly those logits -- the
log-probabilities under that module's bound, top_ids and rank exactly.  Which rows of a draw belong to which request is read from the
seeds the row-wise sampler is called with (the five SamplingParams have five seeds); a run with sampling=None has the schedule of the
run with sampling of the same configuration (no EOS: a request retires at its max_length), so it uses that run's map.
The tiny model in fp32; the emulator on the CPU (eager), the MI355X under -m gpu (eager and captured)."""
import pytest
import torch

from test_batch_decode_sampling import MAX_LENS, _five_params, _setup
from test_token_logprobs import _check

WANT = [None, 0, 5, 64, 1]


def _recorder(monkeypatch):
    import omnimamba_amd.batch_decode as BD
    rec, sample0, rows0 = [], BD.sample, BD.sample_rows

    def sample(lg, **kw):
        t = sample0(lg, **kw)
        rec.append({"logits": lg.clone(), "ids": t.clone(), "seeds": None, "active": None})
        return t

    def sample_rows(lg, **kw):
        t = rows0(lg, **kw)
        rec.append({"logits": lg.clone(), "ids": t.clone(), "seeds": kw["seeds"].clone(),
                    "active": None if kw.get("active") is None else kw["active"].clone()})
        return t

    monkeypatch.setattr(BD, "sample", sample)
    monkeypatch.setattr(BD, "sample_rows", sample_rows)
    return rec


def _row_map(rec, params):
    """Per request the (draw, row) pairs of its ids in sampling order, from the seeds of the recorded row-wise calls."""
    by_seed = {p.seed: i for i, p in enumerate(params)}
    assert len(by_seed) == len(params)
    rows = [[] for _ in params]
    for d, r in enumerate(rec):
        act = [1] * r["logits"].shape[0] if r["active"] is None else r["active"].cpu().tolist()
        for b, sd in enumerate(r["seeds"].cpu().tolist()):
            if act[b]:
                rows[by_seed[sd]].append((d, b))
    return rows


def _check_records(recs, want, rec, rows, out, reqs, what):
    from omnimamba_amd.sampling import TokenLogprobs
    assert len(recs) == len(reqs)
    for i, (r, w) in enumerate(zip(recs, want)):
        L = reqs[i][0].shape[1]
        n_i = out[i].shape[1] - L
        assert len(rows[i]) == n_i and n_i >= 1
        if w is None:
            assert r is None
            continue
        x = torch.stack([rec[d]["logits"][b] for d, b in rows[i]]).cpu()
        ids = torch.stack([rec[d]["ids"][b] for d, b in rows[i]]).cpu()
        assert torch.equal(ids, out[i][0, L:].cpu())                         # (the recorded draws ARE the request's ids)
        assert r.logprob.shape == (n_i,) and r.rank.shape == (n_i,) and r.top_ids.shape == (n_i, w) and r.top_logprobs.shape == (n_i, w)
        assert r.top_ids.dtype == torch.int64 and r.top_logprobs.dtype == torch.float32
        got = r if w > 0 else TokenLogprobs(logprob=r.logprob, rank=r.rank)
        _check(x, ids, w, got, f"{what} request {i}")


def _same(a, b):
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


def _same_states(a, b):
    return all(sa.seqlen == sb.seqlen and sa.pending_id == sb.pending_id and all(torch.equal(x, y) for la, lb in zip(sa.layers, sb.layers) for x, y in zip(la, lb))
               for sa, sb in zip(a, b))


FIRST = {"max_batch_4": dict(max_batch=4), "max_batch_1": dict(max_batch=1), "prefill_batch_4": dict(max_batch=4, prefill_batch=4)}
SECOND = {"extend": dict(max_batch=4), "extend_batch_4": dict(max_batch=4, extend_batch=4)}
CASES = list(FIRST) + list(SECOND)


def _records_case(dev, cg, monkeypatch, case):
    """One configuration, with the five mixed SamplingParams and with sampling=None; a SECOND case is the second turn of the five
    conversations (batch-1 extends, or one grouped extend)."""
    from dataclasses import replace
    from omnimamba_amd.batch_decode import decode_ragged
    model, lm, reqs = _setup(dev, 31)
    params = _five_params()
    lens, want, want_none = MAX_LENS, WANT, [5] * 5
    if case in SECOND:
        out, states = decode_ragged(reqs, lm, MAX_LENS, max_batch=4, cg=cg, sampling=params, return_states=True)
        params = [replace(p, step0=o.shape[1] - r[0].shape[1]) for p, o, r in zip(params, out, reqs)]
        g = torch.Generator().manual_seed(23)
        turns = [torch.randint(0, 50, (1, L), generator=g).to(dev) for L in (4, 2, 6, 3, 5)]
        reqs = [(q, model.llm_backbone.embed_input_ids(q), st) for q, st in zip(turns, states)]
        lens, want, want_none = [st.seqlen + 1 + q.shape[1] + 6 for st, q in zip(states, turns)], WANT[::-1], [1, None, 0, 64, 5]
    kw = {**FIRST, **SECOND}[case]
    rec = _recorder(monkeypatch)
    # the five mixed settings: one launch over the bucket's rows (active) per step, per-request N
    plain, st_plain = decode_ragged(reqs, lm, lens, cg=cg, sampling=params, return_states=True, **kw)
    del rec[:]
    out, states, recs = decode_ragged(reqs, lm, lens, cg=cg, sampling=params, return_states=True, logprobs=want, **kw)
    assert _same(out, plain) and _same_states(states, st_plain), "logprobs changed the ids or the states"
    rows = _row_map(rec, params)
    _check_records(recs, want, rec, rows, out, reqs, f"sampling {case}")
    # sampling=None (generation.sample on the sliced logits): the same schedule
    plain = decode_ragged(reqs, lm, lens, cg=cg, **kw)
    del rec[:]
    out, recs = decode_ragged(reqs, lm, lens, cg=cg, logprobs=want_none if case in SECOND else 5, **kw)
    assert _same(out, plain)
    assert [r["logits"].shape[0] for r in rec] == [len({b for rr in rows for d_, b in rr if d_ == d}) for d in range(len(rec))]
    _check_records(recs, want_none, rec, rows, out, reqs, f"sampling=None {case}")
    for r, o, q in zip(recs, out, reqs):                                  # greedy: rank 1 everywhere, the first of the top is the id
        if r is not None:
            assert (r.rank == 1).all()
            assert r.top_ids.shape[1] == 0 or torch.equal(r.top_ids[:, 0], o[0, q[0].shape[1]:].to(r.top_ids.device))


@pytest.mark.parametrize("case", CASES)
def test_records_equal_the_reference_of_the_recorded_inputs(dev, monkeypatch, case):
    _records_case(dev, False, monkeypatch, case)


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES)
def test_records_equal_the_reference_of_the_recorded_inputs_captured(monkeypatch, case):
    _records_case(torch.device("cuda:0"), True, monkeypatch, case)


def test_off_means_off(dev, monkeypatch):
    """logprobs=None never reaches sampling.token_logprobs, and gives the ids of the call with logprobs."""
    import omnimamba_amd.sampling as S
    from omnimamba_amd.batch_decode import decode_ragged
    model, lm, reqs = _setup(dev, 32)
    params = _five_params()
    with_lp, _ = decode_ragged(reqs, lm, MAX_LENS, max_batch=4, cg=False, sampling=params, logprobs=3)
    greedy_lp, _ = decode_ragged(reqs, lm, MAX_LENS, max_batch=4, cg=False, logprobs=3)

    def boom(*a, **kw):
        raise AssertionError("token_logprobs was called with logprobs=None")

    monkeypatch.setattr(S, "token_logprobs", boom)
    assert _same(decode_ragged(reqs, lm, MAX_LENS, max_batch=4, cg=False, sampling=params), with_lp)
    assert _same(decode_ragged(reqs, lm, MAX_LENS, max_batch=4, cg=False, logprobs=None), greedy_lp)
    with pytest.raises(AssertionError, match="token_logprobs was called"):
        decode_ragged(reqs, lm, MAX_LENS, max_batch=4, cg=False, logprobs=0)
    # a list that asks for nothing launches nothing and still returns the extra element
    out, recs = decode_ragged(reqs, lm, MAX_LENS, max_batch=4, cg=False, logprobs=[None] * 5)
    assert _same(out, greedy_lp) and recs == [None] * 5


def test_per_request_n_with_eos_and_a_request_that_finishes_at_admission(dev, monkeypatch):
    """Every record has as many rows as its request has sampled ids: a request retired by EOS (the EOS row included), one whose max_length
    ends it with the id of its prefill, and the others at their max_length."""
    from omnimamba_amd.batch_decode import decode_ragged
    model, lm, reqs = _setup(dev, 33)
    params = _five_params()
    lens = list(MAX_LENS)
    lens[1] = reqs[1][1].shape[1] + 1                                          # one id, sampled from the prefill logits
    free = decode_ragged(reqs, lm, lens, max_batch=4, cg=False, sampling=params)
    eos = int(free[2][0, reqs[2][0].shape[1] + 3])                             # the fourth id request 2 samples
    rec = _recorder(monkeypatch)
    out, recs = decode_ragged(reqs, lm, lens, max_batch=4, cg=False, sampling=params, eos_token_id=eos, logprobs=WANT)
    n = [o.shape[1] - r[0].shape[1] for o, r in zip(out, reqs)]
    assert n[1] == 1 and n[2] <= 4 and int(out[2][0, -1]) == eos
    assert recs[0] is None and [tuple(r.top_ids.shape) for r in recs[1:]] == [(n[1], 0), (n[2], 5), (n[3], 64), (n[4], 1)]
    _check_records(recs, WANT, rec, _row_map(rec, params), out, reqs, "eos")


def test_public_entries_and_validation(dev):
    from omnimamba_amd.batch_decode import decode_ragged
    from omnimamba_amd.sampling import TokenLogprobs
    from test_batch_decode import _requests, _separate
    from test_stack_decode_train import tiny_path
    torch.manual_seed(34)
    model = tiny_path("inference").to(dev)
    _separate(model)
    feats, qs = _requests(dev, 3)
    lens = MAX_LENS[:3]
    plain = model.mmu_generate_batch(feats, qs, max_length=lens, max_batch=2, cg=False)
    ids, recs = model.mmu_generate_batch(feats, qs, max_length=lens, max_batch=2, cg=False, logprobs=2)
    assert _same(ids, plain) and all(isinstance(r, TokenLogprobs) and r.top_ids.shape[1] == 2 for r in recs)
    ids, states, recs = model.mmu_generate_batch(feats, qs, max_length=lens, max_batch=2, cg=False, logprobs=[0, None, 3], return_states=True)
    assert _same(ids, plain) and recs[1] is None and recs[0].top_ids.shape[1] == 0 and recs[2].top_logprobs.shape[1] == 3
    g = torch.Generator().manual_seed(35)
    turns = [torch.randint(0, 50, (1, L), generator=g).to(dev) for L in (3, 2, 4)]
    lens2 = [st.seqlen + 1 + q.shape[1] + 4 for st, q in zip(states, turns)]
    ids2, states2 = model.mmu_continue(states, turns, max_length=lens2, max_batch=2, cg=False)
    got2, gstates2, recs2 = model.mmu_continue(states, turns, max_length=lens2, max_batch=2, cg=False, logprobs=1)
    assert _same(got2, ids2) and len(gstates2) == 3
    for r, o, q in zip(recs2, got2, turns):
        assert r.logprob.shape == (o.shape[1] - q.shape[1],) and (r.rank == 1).all() and (r.logprob <= 0).all()
    lm = model.llm_backbone.mamba
    reqs = [model._mmu_prompt(f, q) for f, q in zip(feats, qs)]
    for bad in ([1, 2], [1, 2, 3, 4], -1, 65, [0, -1, 2], [0, 65, 2], [0, 1.5, 2]):
        with pytest.raises(ValueError):
            decode_ragged(reqs, lm, lens, max_batch=2, cg=False, logprobs=bad)
    assert decode_ragged([], lm, 10, logprobs=3) == ([], [])
