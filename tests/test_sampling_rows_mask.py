"""Guided decoding in the row-wise sampler (omk_sample_rows_masked; sampling.sample_rows(token_mask=, mask_on=)): a packed per-row token
bitmask applied LAST inside the launch, behind the repetition penalty and the edits.

The oracle needs no tolerance: the masked launch returns, bit for bit, the ids of the plain sample_rows launch on
sampling.apply_token_mask(sampling.apply_logit_edits(logits, ...)) with the same settings -- the unchanged plain instantiation on a
torch-masked copy, same random stream (its distribution is pinned by tests/test_sampling_rows.py).  Every random mask gets one bit forced
on inside [0, V), so no case depends on the "nothing left" clause."""
import ctypes
from dataclasses import replace

import pytest
import torch

# (top_k, top_p, temperature, min_p): greedy | top-k 20 | whole vocabulary plain | behind top-p 0.9 | behind min_p 0.05
BRANCHES = [(1, 0.0, 1.0, 0.0), (20, 0.0, 0.9, 0.0), (0, 0.0, 1.0, 0.0), (0, 0.9, 1.0, 0.0), (0, 0.0, 1.0, 0.05)]
NINF = float("-inf")
OMK_SAMPLE_ROWS_BYTES = 336        # sizeof(OmkSampleRows) of the parent build: the masked entry point changed no existing layout


def _params(n, penalty=1.0, settings=BRANCHES):
    from omnimamba_amd.sampling import SamplingParams
    return [SamplingParams(top_k=k, top_p=tp, temperature=t, min_p=mp, seed=900 + 41 * b, step0=2 + 7 * b, repetition_penalty=penalty)
            for b, (k, tp, t, mp) in enumerate(settings[b % len(settings)] for b in range(n))]


def _logits(V, n, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(n, V, generator=g) * 2.0).to(dtype)


def _pack(bits, words=None, tail=False):
    """(n, V) bool -> int32 (n, words) in the bit order of include/omk.h; tail: every bit at a position >= V set (garbage)."""
    n, V = bits.shape
    W = (V + 31) // 32 if words is None else words
    full = torch.zeros(n, W * 32, dtype=torch.bool)
    full[:, :V] = bits
    if tail:
        full[:, V:] = True
    w = (full.view(n, W, 32).long() << torch.arange(32)).sum(-1)
    return torch.where(w >= 2 ** 31, w - 2 ** 32, w).to(torch.int32)


def _bits(n, V, density, seed):
    """A random (n, V) bool mask of about `density`, one bit per row forced on."""
    g = torch.Generator().manual_seed(seed)
    bits = torch.ones(n, V, dtype=torch.bool) if density >= 1.0 else torch.rand(n, V, generator=g) < density
    bits[torch.arange(n), torch.randint(0, V, (n,), generator=g)] = True
    return bits


def _edits(logits, cap=8):
    """Per row a short list built from the row's ranking: the arg max banned, +30 on a middling token, small biases; row 1 is allow-only
    over 12 tokens.  Behind a row's length: the arg max with +50 (must not be read)."""
    n, V = logits.shape
    ids = torch.zeros(n, cap, dtype=torch.int64)
    vals = torch.full((n, cap), 50.0)
    lens = torch.zeros(n, dtype=torch.int32)
    mode = torch.zeros(n, dtype=torch.int32)
    for b in range(n):
        order = torch.argsort(logits[b].float(), descending=True, stable=True).tolist()
        ids[b] = order[0]
        if b == 1:
            l = [(t, 0.25 * j) for j, t in enumerate(order[:min(cap, V)])]
            mode[b] = 1
        else:
            l = [(order[0], NINF), (order[min(9, V - 1)], 30.0), (order[min(3, V - 1)], -1.5), (order[min(5, V - 1)], 2.0)]
        l = list({t: v for t, v in reversed(l)}.items())[::-1]
        for j, (t, v) in enumerate(l):
            ids[b, j], vals[b, j] = t, v
        lens[b] = len(l)
    return {"edit_ids": ids, "edit_vals": vals, "edit_lens": lens, "edit_mode": mode}


def _history(logits, cap=24):
    n, V = logits.shape
    g = torch.Generator().manual_seed(5)
    h = torch.zeros(n, cap, dtype=torch.int64)
    for b in range(n):
        top = torch.topk(logits[b].float(), min(8, V)).indices
        h[b] = torch.cat([top, torch.tensor([0, V - 1]), torch.randint(0, V, (cap,), generator=g)])[:cap]
    return h, torch.full((n,), cap - 3, dtype=torch.int32)


def _to(d, dev):
    return {k: v.to(dev) for k, v in d.items()}


def _settings(params, dev, hist):
    from omnimamba_amd.sampling import pack_rows
    pk = pack_rows(params, dev)
    pen = pk.pop("penalty")
    rep = {} if hist is None else {"penalty": pen, "history": hist[0], "history_lens": hist[1]}
    return pk, rep


def _masked(logits, params, mask, ed=None, hist=None, **kw):
    from omnimamba_amd.sampling import sample_rows
    pk, rep = _settings(params, logits.device, hist)
    return sample_rows(logits, **pk, **rep, **(ed or {}), token_mask=mask, **kw)


def _oracle(logits, params, mask, ed=None, hist=None, mask_on=None, **kw):
    """The plain launch on a copy edited and then masked with torch."""
    from omnimamba_amd.sampling import apply_logit_edits, apply_token_mask, sample_rows, sample_rows_form
    pk, rep = _settings(params, logits.device, hist)
    work = apply_token_mask(apply_logit_edits(logits, **(ed or {}), **rep), mask, mask_on)
    assert sample_rows_form(work, **pk) == 0
    return sample_rows(work, **pk, **kw)


def _check(dev, V, dtype, form, density, n=5, seed=0):
    """One masked launch of n rows (row b on branch b) against the oracle; form 3: the mask alone, form 4: with edits and a penalised
    history.  Returns how many ids the mask changed."""
    from omnimamba_amd.sampling import sample_rows, sample_rows_form
    logits_h = _logits(V, n, dtype, seed)
    params = _params(n, penalty=1.3 if form == 4 else 1.0)
    bits = _bits(n, V, density, 7 + seed)
    if form == 4:       # (the forced bit of a row may be its banned arg max, or outside the allowed set of row 1: one more, on a token the edits leave finite)
        bits[torch.arange(n), torch.argsort(logits_h.float(), descending=True, stable=True)[:, 2]] = True
    logits, mask = logits_h.to(dev), _pack(bits).to(dev)
    ed = _to(_edits(logits_h), dev) if form == 4 else None
    hist = tuple(t.to(dev) for t in _history(logits_h)) if form == 4 else None
    pk, rep = _settings(params, dev, hist)
    assert sample_rows_form(logits, **pk, **rep, **(ed or {}), token_mask=mask) == form
    before, mask_before = logits.clone(), mask.clone()
    got = _masked(logits, params, mask, ed, hist).cpu()
    assert torch.equal(logits.view(torch.uint8), before.view(torch.uint8)) and torch.equal(mask, mask_before), "the launch wrote to its inputs"
    want = _oracle(logits, params, mask, ed, hist).cpu()
    print(f"V={V} {dtype} form={form} density={density}: got {got.tolist()} want {want.tolist()}")
    assert torch.equal(got, want), (V, dtype, form, density, got.tolist(), want.tolist())
    assert all(bool(bits[b, int(got[b])]) for b in range(n)), "an id outside the mask"
    unmasked = sample_rows(logits, **pk, **rep, **(ed or {})).cpu()
    return int((got != unmasked).sum())


@pytest.mark.parametrize("form", [3, 4])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_every_branch_equals_the_plain_launch_on_a_masked_copy(dev, dtype, form):
    """V = 33: two words with a ragged tail; 1000: no multiple of 32; 4099: more than one strided round of 4 x 1024 lanes and a tail.  Five
    rows, one per branch; masks of ~50 %, ~1 % and all ones."""
    changed = 0
    for V in (33, 1000, 4099):
        for density in (0.5, 0.01):
            changed += _check(dev, V, dtype, form, density, seed=V)
        assert _check(dev, V, dtype, form, 1.0, seed=V) == 0, "an all-ones mask changed an id"
    assert changed >= 12, "the masks changed almost nothing: the case does not test them"


@pytest.mark.gpu
@pytest.mark.parametrize("form", [3, 4])
@pytest.mark.parametrize("V", [50288, 65536])
def test_the_mmu_vocabulary_and_the_largest_mask(V, form):
    """50 288: the MMU vocabulary; 65 536: the largest mask and id map (the whole LDS budget of form 4)."""
    dev = torch.device("cuda:0")
    assert _check(dev, V, torch.float32, form, 0.5) + _check(dev, V, torch.bfloat16, form, 0.01, seed=1) >= 4


def test_tail_bits_wider_masks_and_row_strides(dev):
    """Garbage bits at positions >= V, mask_words larger than needed, and a row stride above mask_words (a column slice of a wider
    tensor): the ids of the tight clean mask."""
    for V in (33, 1000):
        n = 5
        logits = _logits(V, n, torch.float32, 3).to(dev)
        params = _params(n)
        bits = _bits(n, V, 0.3, 9)
        want = _masked(logits, params, _pack(bits).to(dev)).cpu()
        assert torch.equal(want, _oracle(logits, params, _pack(bits).to(dev)).cpu())
        W = (V + 31) // 32
        assert torch.equal(_masked(logits, params, _pack(bits, tail=True).to(dev)).cpu(), want)
        assert torch.equal(_masked(logits, params, _pack(bits, words=W + 3, tail=True).to(dev)).cpu(), want)
        wide = torch.full((n, W + 5), -1, dtype=torch.int32)
        wide[:, 2:2 + W] = _pack(bits, tail=True)
        sl = wide.to(dev)[:, 2:2 + W]
        assert sl.stride(0) == W + 5 and not sl.is_contiguous()
        assert torch.equal(_masked(logits, params, sl).cpu(), want)
        assert torch.equal(_oracle(logits, params, sl).cpu(), want)


@pytest.mark.parametrize("pen", [False, True])
def test_one_allowed_token_is_what_every_branch_returns(dev, pen):
    """Whatever the temperature, top-p or min-p, with and without a repetition penalty whose history holds the token."""
    V, n = 1000, 10
    logits = _logits(V, n, torch.bfloat16, 6).to(dev)
    settings = BRANCHES + [(20, 0.3, 0.05, 0.0), (64, 0.9, 7.0, 0.0), (0, 0.0, 0.05, 0.0), (0, 0.2, 9.0, 0.0), (0, 0.0, 4.0, 0.9)]
    params = _params(n, penalty=1.7 if pen else 1.0, settings=settings)
    only = torch.tensor([0, V - 1, 31, 32, 63, 64, 255, 256, 511, 999 - 32])
    bits = torch.zeros(n, V, dtype=torch.bool)
    bits[torch.arange(n), only] = True
    hist = (torch.cat([only[:, None], torch.zeros(n, 3, dtype=torch.int64)], 1).to(dev), torch.full((n,), 4, dtype=torch.int32).to(dev)) if pen else None
    got = _masked(logits, params, _pack(bits).to(dev), None, hist).cpu()
    assert torch.equal(got, only), (got.tolist(), only.tolist())


def test_the_mask_is_applied_last(dev):
    """A masked-out token with a +30 bias entry is never drawn; an allow-only row draws only from allowed AND mask; with frequency /
    presence the path is penalty_edits -> the masked launch and the ids equal the copy path's."""
    from omnimamba_amd import _capi as K
    from omnimamba_amd.sampling import apply_logit_edits, apply_token_mask, pack_rows, sample_rows
    import omnimamba_amd.sampling as S
    V, n = 1000, 5
    logits_h = _logits(V, n, torch.float32, 8)
    logits = logits_h.to(dev)
    order = torch.argsort(logits_h, descending=True, stable=True)
    boosted = order[:, 40]
    allowed = order[:, :10]
    ids = torch.cat([boosted[:, None], allowed], 1)
    vals = torch.zeros(n, 11)
    vals[:, 0] = 30.0
    bits = _bits(n, V, 0.5, 13)
    bits[torch.arange(n), boosted] = False
    for b in range(n):                      # half of the allowed set is masked out, at least one member stays
        bits[b, allowed[b, ::2]] = False
        bits[b, allowed[b, 1]] = True
    mask = _pack(bits).to(dev)
    for seed in range(6):
        params = _params(n, settings=[(0, 0.0, 1.5, 0.0), (20, 0.0, 1.5, 0.0)])
        params = [replace(p, seed=p.seed + 1000 * seed) for p in params]
        bias = {"edit_ids": ids[:, :1].contiguous().to(dev), "edit_vals": vals[:, :1].contiguous().to(dev),
                "edit_lens": torch.ones(n, dtype=torch.int32).to(dev), "edit_mode": torch.zeros(n, dtype=torch.int32).to(dev)}
        unm = sample_rows(logits, **{k: v for k, v in pack_rows(params, dev).items() if k != "penalty"}, **bias).cpu()
        got = _masked(logits, params, mask, bias).cpu()
        assert torch.equal(unm, boosted), "without the mask the +30 token is what every row draws"
        assert not (got == boosted).any() and torch.equal(got, _oracle(logits, params, mask, bias).cpu())
        allow = {"edit_ids": ids.to(dev), "edit_vals": vals.to(dev), "edit_lens": torch.full((n,), 11, dtype=torch.int32).to(dev),
                 "edit_mode": torch.ones(n, dtype=torch.int32).to(dev)}
        got = _masked(logits, params, mask, allow).cpu()
        for b in range(n):
            assert int(got[b]) in allowed[b].tolist() and bool(bits[b, int(got[b])]), (b, int(got[b]))
        assert torch.equal(got, _oracle(logits, params, mask, allow).cpu())
    # frequency / presence: two library launches (penalty_edits, the masked launch), and the ids of the copy path
    params = _params(n)
    hist = tuple(t.to(dev) for t in _history(logits_h))
    pk, rep = _settings(params, dev, hist)
    fr, pr = torch.full((n,), 0.7).to(dev), torch.full((n,), 0.4).to(dev)
    cs = torch.full((n,), 2, dtype=torch.int32).to(dev)
    calls, run0, try_run0 = [], K.run, K.try_run
    try:
        K.run = lambda lib, name, *a, **k: (calls.append(name), run0(lib, name, *a, **k))[1]
        K.try_run = lambda lib, name, *a, **k: (calls.append(name), try_run0(lib, name, *a, **k))[1]
        got = sample_rows(logits, **pk, **rep, **bias, frequency=fr, presence=pr, count_start=cs, token_mask=mask).cpu()
    finally:
        K.run, K.try_run = run0, try_run0
    assert calls == ["omk_penalty_edits", "omk_sample_rows_masked"], calls
    work = apply_token_mask(apply_logit_edits(logits, **bias, **rep, frequency=fr, presence=pr, count_start=cs), mask)
    assert torch.equal(got, sample_rows(work, **pk).cpu())
    assert S.sample_rows_form(logits, **pk, **rep, token_mask=mask) == 4       # (a history and a mask without a list: edit_cap 0)
    assert torch.equal(_masked(logits, params, mask, None, hist).cpu(), _oracle(logits, params, mask, None, hist).cpu())


def test_mask_on_and_active(dev):
    """Rows with mask_on 0 draw the unmasked launch's ids and inactive rows write nothing; the mask rows of both hold all zeros (a row
    that consulted them would be left without a finite logit)."""
    from omnimamba_amd.sampling import sample_rows
    V, n = 1000, 8
    logits_h = _logits(V, n, torch.bfloat16, 10)
    logits = logits_h.to(dev)
    for form in (3, 4):
        params = _params(n, penalty=1.3 if form == 4 else 1.0)
        ed = _to(_edits(logits_h), dev) if form == 4 else None
        hist = tuple(t.to(dev) for t in _history(logits_h)) if form == 4 else None
        on_h = torch.tensor([1, 0, 1, 0, 7, 0, 1, 0], dtype=torch.int32)         # (anything but 0 counts as 1)
        act_h = torch.tensor([1, 1, 1, 1, 1, 1, 0, 0], dtype=torch.int32)
        bits = _bits(n, V, 0.5, 21)
        words = _pack(bits)
        words[(on_h == 0) | (act_h == 0)] = 0
        mask, on, act = words.to(dev), on_h.to(dev), act_h.to(dev)
        pk, rep = _settings(params, dev, hist)
        unmasked = sample_rows(logits, **pk, **rep, **(ed or {})).cpu()
        allmasked = _masked(logits, params, _pack(bits).to(dev), ed, hist).cpu()
        out = torch.full((n,), -7, dtype=torch.int64, device=dev)
        got = _masked(logits, params, mask, ed, hist, mask_on=on, active=act, out=out).cpu()
        for b in range(n):
            want = -7 if not act_h[b] else int(allmasked[b] if on_h[b] else unmasked[b])
            assert int(got[b]) == want, (form, b, got.tolist())
        assert (allmasked != unmasked).sum() >= 3
        want = _oracle(logits, params, mask, ed, hist, mask_on=on).cpu()
        assert torch.equal(got[:6], want[:6])


def test_placement_invariance(dev):
    """A row's id does not depend on its index or its neighbours."""
    V, n = 4099, 5
    logits_h = _logits(V, n, torch.float16, 14)
    for form in (3, 4):
        params = _params(n, penalty=1.3 if form == 4 else 1.0)
        ed = _to(_edits(logits_h), dev) if form == 4 else None
        hist = tuple(t.to(dev) for t in _history(logits_h)) if form == 4 else None
        logits, mask = logits_h.to(dev), _pack(_bits(n, V, 0.5, 15)).to(dev)
        ids = _masked(logits, params, mask, ed, hist).cpu()
        perm = torch.tensor([3, 0, 4, 2, 1])
        pd = perm.to(dev)
        got = _masked(logits[pd].contiguous(), [params[i] for i in perm.tolist()], mask[pd].contiguous(),
                      None if ed is None else {k: v[pd].contiguous() for k, v in ed.items()},
                      None if hist is None else tuple(t[pd].contiguous() for t in hist)).cpu()
        assert torch.equal(got, ids[perm])
        for b in range(n):      # alone
            one = _masked(logits[b:b + 1], params[b:b + 1], mask[b:b + 1], None if ed is None else {k: v[b:b + 1] for k, v in ed.items()},
                          None if hist is None else tuple(t[b:b + 1] for t in hist)).cpu()
            assert int(one[0]) == int(ids[b])


def test_never_outside_the_mask(dev):
    """64 seeds x 4 rows, the whole vocabulary at temperature 1.5, ~50 % masks: every id has its bit set."""
    from omnimamba_amd.sampling import SamplingParams
    V, n = 1000, 4
    logits = _logits(V, n, torch.float32, 16).to(dev)
    seen = set()
    for seed in range(64):
        bits = _bits(n, V, 0.5, 100 + seed)
        params = [SamplingParams(top_k=0, temperature=1.5, seed=5000 + 13 * seed + b, step0=seed) for b in range(n)]
        got = _masked(logits, params, _pack(bits).to(dev)).cpu()
        for b in range(n):
            assert 0 <= int(got[b]) < V and bool(bits[b, int(got[b])]), (seed, b, int(got[b]))
            seen.add(int(got[b]))
    assert len(seen) > 100, "the rows hardly sample: the case does not test the mask"


def _status(lib, logits, params, mask, words=None, stride=None):
    from omnimamba_amd import _capi as K
    from omnimamba_amd.sampling import _rows_call
    pk, _ = _settings(params, logits.device, None)
    p, out = _rows_call(logits, **pk)
    pm = K.SampleRowsMasked(rows=p, mask=None if mask is None else mask.data_ptr(), mask_stride=(mask.stride(0) if mask is not None else 0) if stride is None else stride,
                            mask_words=(mask.shape[1] if mask is not None else 0) if words is None else words)
    return int(lib.omk_sample_rows_masked_form(ctypes.byref(pm))), pm, out


def test_form_and_refusals(dev):
    from omnimamba_amd import _capi as K
    from omnimamba_amd._lib import get_lib
    from omnimamba_amd.sampling import sample_rows, sample_rows_form
    lib = get_lib()
    V, n = 1000, 3
    logits_h = _logits(V, n, torch.float32, 17)
    logits = logits_h.to(dev)
    params = _params(n)
    mask = _pack(_bits(n, V, 0.5, 18)).to(dev)
    pk, _ = _settings(params, dev, None)
    hist = tuple(t.to(dev) for t in _history(logits_h))
    _, rep = _settings(_params(n, penalty=1.3), dev, hist)
    ed = _to(_edits(logits_h), dev)
    assert sample_rows_form(logits, **pk, token_mask=mask) == K.SAMPLE_ROWS_MASK == 3
    assert sample_rows_form(logits, **pk, **ed, token_mask=mask) == K.SAMPLE_ROWS_EDIT_MASK == 4
    assert sample_rows_form(logits, **pk, **rep, token_mask=mask) == 4
    assert [sample_rows_form(logits, **pk), sample_rows_form(logits, **pk, **rep), sample_rows_form(logits, **pk, **ed)] == [0, 1, 2]
    # mask == NULL through the masked entry point: the base call's form and ids
    for extra, form in (({}, 0), (rep, 1), (ed, 2)):
        from omnimamba_amd.sampling import _rows_call
        p, out = _rows_call(logits, **pk, **extra)
        pm = K.SampleRowsMasked(rows=p)
        assert int(lib.omk_sample_rows_masked_form(ctypes.byref(pm))) == form
        K.run(lib, "omk_sample_rows_masked", pm, logits)
        assert torch.equal(out.cpu(), sample_rows(logits, **pk, **extra).cpu())
    # refusals
    W = (V + 31) // 32
    assert _status(lib, logits, params, mask, words=W - 1)[0] == -1                  # too few words
    assert _status(lib, logits, params, mask, words=-1)[0] == -1                     # a negative width
    assert _status(lib, logits, params, mask, stride=W - 1)[0] == -1                 # rows that overlap
    assert _status(lib, logits[:1], params[:1], mask[:1], stride=0)[0] == 3          # (one row: its stride is not read)
    assert _status(lib, logits, params, mask)[0] == 3
    with pytest.raises(ValueError):
        sample_rows(logits, **pk, token_mask=mask.float())
    with pytest.raises(ValueError):
        sample_rows(logits, **pk, mask_on=torch.ones(n, dtype=torch.int32).to(dev))
    with pytest.raises(RuntimeError):
        sample_rows(logits, **pk, token_mask=mask[:, :W - 1].contiguous())


def test_a_vocabulary_above_the_bound_is_masked_on_a_copy(dev):
    """V = 65 537: the library refuses with OMK_EUNSUPPORTED (-4), and sample_rows returns the copy path's ids."""
    from omnimamba_amd._lib import get_lib
    V, n = 65537, 2
    logits = _logits(V, n, torch.float32, 19).to(dev)
    params = _params(n, settings=[(1, 0.0, 1.0, 0.0), (8, 0.0, 1.0, 0.0)])
    bits = _bits(n, V, 0.5, 20)
    bits[torch.arange(n), logits.cpu().argmax(1)] = False
    mask = _pack(bits).to(dev)
    assert _status(get_lib(), logits, params, mask)[0] == -4
    got = _masked(logits, params, mask).cpu()
    assert torch.equal(got, _oracle(logits, params, mask).cpu())
    assert all(bool(bits[b, int(got[b])]) for b in range(n))


def test_abi_is_additive(dev):
    from omnimamba_amd import _capi as K
    from omnimamba_amd._lib import get_lib
    lib = get_lib()
    assert lib.omk_abi_version() == 17 and K.OMK_ABI_VERSION == 17
    assert lib.omk_sizeof(b"OmkSampleRowsMasked") == ctypes.sizeof(K.SampleRowsMasked) == OMK_SAMPLE_ROWS_BYTES + 32
    assert lib.omk_sizeof(b"OmkSampleRows") == ctypes.sizeof(K.SampleRows) == OMK_SAMPLE_ROWS_BYTES
    assert K.SampleRowsMasked.rows.offset == 0 and K.SampleRowsMasked.mask.offset == OMK_SAMPLE_ROWS_BYTES
