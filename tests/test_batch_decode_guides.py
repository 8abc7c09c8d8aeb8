"""Guided decoding in continuous batching (decode_ragged / mmu_generate_batch / mmu_continue with guides=...): a guide's packed token
mask reaches every draw of its request -- the admission draw (prefill, extend, grouped or not) and the steps -- through the masked
row-wise launch, and changes nothing for the requests that have none.  The tiny model in fp32 (64 logits: two mask words); the emulator
on the CPU (eager), the MI355X under -m gpu.

The oracle is a single-request loop that masks with torch: decode_ragged of one request at max_batch 1 whose draws are rerouted (the
module's sample_rows replaced) to the plain / edit launch on sampling.apply_token_mask(sampling.apply_logit_edits(...)) -- the masked
launch is never called there.  Exact ids: the argument of tests/test_batch_decode_sampling.py (fp32 logits, fewer than 200 draws at fixed
seeds) holds here as it does there."""
from dataclasses import replace

import pytest
import torch

from test_batch_decode_sampling import MAX_LENS, _five_params, _setup

V, EOS = 64, 63
CHOICES = [[[3, 4, 5], [3, 9], [40]], None, [[7], [7, 8, 9, 10]], [[20, 21, 22, 23, 24], [25, 26]], None]


def _choice_guides():
    from omnimamba_amd.sampling import ChoiceGuide
    return [None if c is None else ChoiceGuide(c, V, EOS) for c in CHOICES]


class HalfGuide:
    """Allows a pseudo-random half of the vocabulary per step (its own generator: the same sequence of masks wherever it runs); with
    `every` > 1 it returns None on the other steps."""

    def __init__(self, seed, every=1):
        self.seed, self.every, self.n, self.seen = seed, every, 0, []

    def mask(self):
        from omnimamba_amd.sampling import pack_token_mask
        n = self.n
        if n % self.every:
            return None
        g = torch.Generator().manual_seed(self.seed * 1000 + n)
        return pack_token_mask(torch.randperm(V, generator=g)[: V // 2].tolist(), V)

    def advance(self, tok):
        self.seen.append(int(tok))
        self.n += 1


def _gen(out, reqs):
    return [o[0, r[0].shape[1]:].tolist() for o, r in zip(out, reqs)]


def _torch_masked(monkeypatch):
    """Reroute the module's draws: the mask (and everything else) applied to a copy with torch, then the plain launch."""
    import omnimamba_amd.batch_decode as BD
    from omnimamba_amd.sampling import apply_logit_edits, apply_token_mask
    rows0 = BD.sample_rows

    def sample_rows(lg, **kw):
        tm, on = kw.pop("token_mask", None), kw.pop("mask_on", None)
        if tm is None:
            return rows0(lg, **kw)
        plain = {k: kw[k] for k in ("top_k", "top_p", "temperature", "min_p", "seeds", "steps", "active", "out") if k in kw}
        work = apply_logit_edits(lg, kw.get("edit_ids"), kw.get("edit_vals"), kw.get("edit_lens"), kw.get("edit_mode"), penalty=kw.get("penalty"),
                                 history=kw.get("history"), history_lens=kw.get("history_lens"), frequency=kw.get("frequency"),
                                 presence=kw.get("presence"), count_start=kw.get("count_start"))
        return rows0(apply_token_mask(work, tm, on), **plain)

    monkeypatch.setattr(BD, "sample_rows", sample_rows)


def _oracle(monkeypatch, lm, reqs, lens, params, make_guides, **kw):
    """Every request alone, max_batch 1, masked with torch."""
    import omnimamba_amd.batch_decode as BD
    _torch_masked(monkeypatch)
    guides = make_guides()
    out = [BD.decode_ragged([r], lm, L, max_batch=1, cg=False, sampling=p, guides=[g], **kw) for r, L, p, g in zip(reqs, lens, params, guides)]
    monkeypatch.undo()
    return out


def _count_library_calls(monkeypatch):
    """Count the library calls of the sampler by name (both ways sampling.py reaches the library)."""
    from omnimamba_amd import _capi as K
    calls, run0, try0 = [], K.run, K.try_run
    monkeypatch.setattr(K, "run", lambda lib, name, *a, **k: (calls.append(name), run0(lib, name, *a, **k))[1])
    monkeypatch.setattr(K, "try_run", lambda lib, name, *a, **k: (calls.append(name), try0(lib, name, *a, **k))[1])
    return calls


def test_choice_guides_emit_a_choice_then_eos_and_equal_the_single_request_loop(dev, monkeypatch):
    """Greedy and stochastic settings: a guided request emits one of its choices followed by EOS; its ids are those of the single-request
    loop that masks with torch, for max_batch 1 / 3 / 8, two admission orders and grouped admission; the unguided requests draw what they
    draw in the same call without guides."""
    import omnimamba_amd.batch_decode as BD
    model, lm, reqs = _setup(dev, 51)
    for params in ([type(p)() for p in _five_params()], _five_params()):
        alone = [a[0] for a in _oracle(monkeypatch, lm, reqs, MAX_LENS, params, _choice_guides, eos_token_id=EOS)]
        gen = _gen(alone, reqs)
        for i, c in enumerate(CHOICES):
            if c is not None:
                assert gen[i][-1] == EOS and gen[i][:-1] in c, (i, gen[i])
        calls = _count_library_calls(monkeypatch)
        for kw in (dict(max_batch=3), dict(max_batch=1), dict(max_batch=8), dict(max_batch=3, prefill_batch=2)):
            got = BD.decode_ragged(reqs, lm, MAX_LENS, cg=False, sampling=params, guides=_choice_guides(), eos_token_id=EOS, **kw)
            for i, (g, w) in enumerate(zip(got, alone)):
                assert torch.equal(g, w), (kw, i, g.tolist(), w.tolist())
        assert "omk_sample_rows_masked" in calls
        monkeypatch.undo()
        rev = BD.decode_ragged(reqs[::-1], lm, MAX_LENS[::-1], max_batch=3, cg=False, sampling=params[::-1], guides=_choice_guides()[::-1], eos_token_id=EOS)
        for i, (g, w) in enumerate(zip(rev[::-1], alone)):
            assert torch.equal(g, w), (i, g.tolist(), w.tolist())
        free = BD.decode_ragged(reqs, lm, MAX_LENS, max_batch=3, cg=False, sampling=params, eos_token_id=EOS)
        assert torch.equal(free[1], alone[1]) and torch.equal(free[4], alone[4])
        assert sum(not torch.equal(free[i], alone[i]) for i in (0, 2, 3)) == 3, "the guides changed nothing: the case does not test them"


@pytest.mark.gpu
def test_choice_guides_with_captured_steps():
    import omnimamba_amd.batch_decode as BD
    dev = torch.device("cuda:0")
    model, lm, reqs = _setup(dev, 51)
    params = _five_params()
    eager = BD.decode_ragged(reqs, lm, MAX_LENS, max_batch=4, cg=False, sampling=params, guides=_choice_guides(), eos_token_id=EOS)
    cap = BD.decode_ragged(reqs, lm, MAX_LENS, max_batch=4, cg=True, sampling=params, guides=_choice_guides(), eos_token_id=EOS)
    for i, (g, w) in enumerate(zip(cap, eager)):
        assert torch.equal(g, w), (i, g.tolist(), w.tolist())
    gen = _gen(cap, reqs)
    for i, c in enumerate(CHOICES):
        if c is not None:
            assert gen[i][-1] == EOS and gen[i][:-1] in c, (i, gen[i])


def test_no_guide_anywhere_launches_what_the_parent_launches(dev, monkeypatch):
    """guides=None and a list of None: omk_sample_rows_masked is never called, no mask keyword is passed, and the library calls are those
    of the call without the argument."""
    import omnimamba_amd.batch_decode as BD
    model, lm, reqs = _setup(dev, 52)
    params = _five_params()
    kws, rows0 = [], BD.sample_rows
    monkeypatch.setattr(BD, "sample_rows", lambda lg, **kw: (kws.append(set(kw)), rows0(lg, **kw))[1])
    calls = _count_library_calls(monkeypatch)
    base = BD.decode_ragged(reqs, lm, MAX_LENS, max_batch=4, cg=False, sampling=params)
    parent = list(calls)
    assert parent and "omk_sample_rows" in parent
    for guides in (None, [None] * 5):
        del calls[:], kws[:]
        got = BD.decode_ragged(reqs, lm, MAX_LENS, max_batch=4, cg=False, sampling=params, guides=guides)
        assert calls == parent and "omk_sample_rows_masked" not in calls
        assert kws and not any({"token_mask", "mask_on"} & k for k in kws)
        assert all(torch.equal(g, w) for g, w in zip(got, base))
    del calls[:]
    BD.decode_ragged(reqs, lm, MAX_LENS, max_batch=4, cg=False, sampling=params, guides=_choice_guides(), eos_token_id=EOS)
    assert "omk_sample_rows_masked" in calls


def test_guides_that_switch_between_none_and_a_mask_under_stochastic_settings(dev, monkeypatch):
    """A guide that allows a pseudo-random half of the vocabulary on every step, one that does so on every third step and returns None in
    between, an unguided request: the ids of the single-request loop at the same seed and step0; mask() ran once in front of every draw and
    advance() saw every id in order."""
    import omnimamba_amd.batch_decode as BD
    from omnimamba_amd.sampling import SamplingParams as SP, pack_token_mask
    model, lm, reqs = _setup(dev, 53)
    params = [SP(top_k=0, temperature=1.5, seed=11, step0=4), SP(top_k=20, temperature=1.2, seed=12), SP(top_k=0, top_p=0.9, seed=13),
              SP(top_k=0, min_p=0.05, temperature=1.5, seed=14), SP(top_k=8, seed=15, step0=9)]
    make = lambda: [HalfGuide(1), HalfGuide(2, every=3), None, HalfGuide(4, every=2), HalfGuide(5)]
    alone = [a[0] for a in _oracle(monkeypatch, lm, reqs, MAX_LENS, params, make)]
    for kw in (dict(max_batch=3), dict(max_batch=8, prefill_batch=4)):
        guides = make()
        got = BD.decode_ragged(reqs, lm, MAX_LENS, cg=False, sampling=params, guides=guides, **kw)
        for i, (g, w) in enumerate(zip(got, alone)):
            assert torch.equal(g, w), (kw, i, g.tolist(), w.tolist())
        gen = _gen(got, reqs)
        for i, gd in enumerate(guides):
            if gd is None:
                continue
            assert gd.seen == gen[i] and gd.n == len(gen[i])
            for n, tok in enumerate(gen[i]):
                if n % gd.every == 0:
                    g = torch.Generator().manual_seed(gd.seed * 1000 + n)
                    assert tok in torch.randperm(V, generator=g)[: V // 2].tolist(), (i, n, tok)
    free = BD.decode_ragged(reqs, lm, MAX_LENS, max_batch=3, cg=False, sampling=params)
    assert torch.equal(free[2], alone[2]) and sum(not torch.equal(free[i], alone[i]) for i in (0, 1, 3, 4)) >= 3


def test_guides_with_logprobs_a_repetition_penalty_and_a_presence_penalty(dev, monkeypatch):
    """Ids equal the single-request oracle's (the mask behind the penalties); the logprobs are those of the same ids on the raw logits."""
    import omnimamba_amd.batch_decode as BD
    from test_batch_decode_logprobs import _check_records, _recorder, _row_map
    model, lm, reqs = _setup(dev, 54)
    params = [replace(p, repetition_penalty=1.3, presence_penalty=0.8, frequency_penalty=0.3) for p in _five_params()]
    make = lambda: [HalfGuide(21), HalfGuide(22, every=2), None, HalfGuide(24), HalfGuide(25)]
    alone = [a[0] for a in _oracle(monkeypatch, lm, reqs, MAX_LENS, params, make)]
    rec = _recorder(monkeypatch)
    got, recs = BD.decode_ragged(reqs, lm, MAX_LENS, max_batch=3, cg=False, sampling=params, guides=make(), logprobs=3)
    monkeypatch.undo()
    for i, (g, w) in enumerate(zip(got, alone)):
        assert torch.equal(g, w), (i, g.tolist(), w.tolist())
    # the records: of the raw logits every draw saw (recorded), under the bound of tests/test_token_logprobs.py
    _check_records(recs, [3] * 5, rec, _row_map(rec, params), got, reqs, "guided")
    free = BD.decode_ragged(reqs, lm, MAX_LENS, max_batch=3, cg=False, sampling=params)
    assert torch.equal(free[2], alone[2]) and sum(not torch.equal(free[i], alone[i]) for i in (0, 1, 3, 4)) >= 3


def test_a_guide_on_a_follow_up_turn(dev, monkeypatch):
    """mmu_continue with guides: the admission draw of an extend (one by one, and two at a time) is masked like every other draw."""
    from omnimamba_amd.batch_decode import decode_ragged
    model, lm, reqs = _setup(dev, 55)
    params = _five_params()
    one, states = decode_ragged(reqs, lm, MAX_LENS, max_batch=4, cg=False, sampling=params, return_states=True)
    g = torch.Generator().manual_seed(23)
    turns = [torch.randint(0, 50, (1, L), generator=g).to(dev) for L in (4, 2, 6, 3, 5)]
    reqs2 = [(q, model.llm_backbone.embed_input_ids(q), st) for q, st in zip(turns, states)]
    params2 = [replace(p, step0=o.shape[1] - r[0].shape[1]) for p, o, r in zip(params, one, reqs)]
    lens2 = [st.seqlen + 1 + q.shape[1] + 7 for st, q in zip(states, turns)]
    alone = [a[0][0] for a in _oracle(monkeypatch, lm, reqs2, lens2, params2, _choice_guides, eos_token_id=EOS, return_states=True)]
    gen = _gen(alone, reqs2)
    for i, c in enumerate(CHOICES):
        if c is not None:
            assert gen[i][-1] == EOS and gen[i][:-1] in c, (i, gen[i])
    for eb in (1, 2):
        ids, st2 = model.mmu_continue(states, turns, max_length=lens2, max_batch=4, cg=False, extend_batch=eb, sampling=params2,
                                      guides=_choice_guides(), eos_token_id=EOS)
        for i, (a, w) in enumerate(zip(ids, alone)):
            assert torch.equal(a, w), (eb, i, a.tolist(), w.tolist())
        assert all(s is not None for s in st2)


def test_the_public_entry_passes_guides_through(dev):
    from omnimamba_amd.batch_decode import decode_ragged
    from test_batch_decode import _requests
    torch.manual_seed(56)
    from test_stack_decode_train import tiny_path
    model = tiny_path("inference").to(dev)
    feats, qs = _requests(dev, 5)
    reqs = [model._mmu_prompt(f, q) for f, q in zip(feats, qs)]
    want = decode_ragged(reqs, model.llm_backbone.mamba, MAX_LENS, max_batch=4, cg=False, sampling=_five_params(), guides=_choice_guides(), eos_token_id=EOS)
    got = model.mmu_generate_batch(feats, qs, max_length=MAX_LENS, max_batch=4, cg=False, sampling=_five_params(), guides=_choice_guides(), eos_token_id=EOS)
    assert all(torch.equal(g, w) for g, w in zip(got, want))


def test_validation(dev):
    from omnimamba_amd.batch_decode import decode_ragged
    from omnimamba_amd.sampling import SamplingParams as SP, pack_token_mask
    model, lm, reqs = _setup(dev, 57)

    class Bad:
        def __init__(self, m):
            self.m = m

        def mask(self):
            return self.m

        def advance(self, tok):
            pass

    ok = pack_token_mask(range(10), V)
    with pytest.raises(ValueError, match="sampling"):
        decode_ragged(reqs[:2], lm, 20, cg=False, guides=[None, Bad(ok)])
    with pytest.raises(ValueError):
        decode_ragged(reqs[:2], lm, 20, cg=False, sampling=SP(), guides=[Bad(ok)])
    with pytest.raises(ValueError):
        decode_ragged(reqs[:2], lm, 20, cg=False, sampling=SP(), guides=[None, object()])
    for bad in (ok.float(), ok[:1].clone(), torch.cat([ok, ok]), ok.long(), ok[None]):
        with pytest.raises(ValueError):
            decode_ragged(reqs[:2], lm, 20, cg=False, sampling=SP(), guides=[None, Bad(bad)])
    if dev.type == "cuda":
        with pytest.raises(ValueError):
            decode_ragged(reqs[:2], lm, 20, cg=False, sampling=SP(), guides=[None, Bad(ok.to(dev))])
    out = decode_ragged(reqs[:2], lm, 20, cg=False, sampling=SP(), guides=[None, Bad(ok)])
    assert set(_gen(out, reqs[:2])[1]) <= set(range(10))


# ---- ChoiceGuide and the packing alone: CPU, no library ---------------------------------------------------------------------------------

def _allowed(mask, vocab):
    return [i for i in range(vocab) if (int(mask[i >> 5]) >> (i & 31)) & 1]


def test_pack_token_mask_bit_order_against_apply_token_mask():
    from omnimamba_amd.sampling import apply_token_mask, pack_token_mask
    for vocab in (33, 64, 1000):
        ids = sorted({0, 31, 32, vocab - 1, vocab // 2, 7})
        m = pack_token_mask(ids, vocab)
        assert m.dtype == torch.int32 and m.shape == ((vocab + 31) // 32,) and m.device.type == "cpu"
        assert _allowed(m, vocab) == ids
        x = torch.arange(vocab, dtype=torch.float32)[None].repeat(2, 1)
        y = apply_token_mask(x, torch.stack([m, torch.zeros_like(m)]), torch.tensor([1, 0], dtype=torch.int32))
        assert torch.isfinite(y[0]).nonzero().flatten().tolist() == ids and torch.equal(y[1], x[1])
        assert torch.equal(y[0][ids], x[0][ids]) and (y[0][[i for i in range(vocab) if i not in ids]] == float("-inf")).all()
        assert not torch.isfinite(apply_token_mask(x, torch.stack([m, torch.zeros_like(m)]))[1]).any()
    assert int(pack_token_mask([31], 64)[0]) == -2 ** 31 and pack_token_mask([32], 64).tolist() == [0, 1]
    assert pack_token_mask([], 40).tolist() == [0, 0]
    for bad in ([-1], [64]):
        with pytest.raises(ValueError):
            pack_token_mask(bad, 64)


def test_choice_guide_walks_the_trie():
    from omnimamba_amd.sampling import ChoiceGuide
    g = ChoiceGuide([[3, 4, 5], [3, 9], [40], [7], [7, 8]], V, EOS)
    assert _allowed(g.mask(), V) == [3, 7, 40]
    g.advance(3)
    assert _allowed(g.mask(), V) == [4, 9]
    g.advance(9)
    assert _allowed(g.mask(), V) == [EOS]
    g.advance(EOS)
    assert _allowed(g.mask(), V) == [EOS]
    # a complete choice that is a proper prefix of another: EOS and the continuation
    g = ChoiceGuide([[7], [7, 8]], V, EOS)
    g.advance(7)
    assert _allowed(g.mask(), V) == [8, EOS]
    g.advance(8)
    assert _allowed(g.mask(), V) == [EOS]
    g = ChoiceGuide([[7], [7, 8]], V, EOS)
    g.advance(7)
    g.advance(EOS)
    assert _allowed(g.mask(), V) == [EOS]
    with pytest.raises(ValueError):
        ChoiceGuide([[7]], V, EOS).advance(8)
    for bad in ([], [[]], [[1], []], [[V]], [[-1]], [[1, 2, 64]]):
        with pytest.raises(ValueError):
            ChoiceGuide(bad, V, EOS)
