"""Per-row logit edits in the row-wise sampler (omk_sample_rows ABI 16; sampling.sample_rows(edit_ids=, edit_vals=, edit_lens=, edit_mode=)):
logit_bias, banned ids and allowed token sets applied inside the launch, behind the repetition penalty.

The oracle needs no tolerance: the fused launch returns, bit for bit, the ids of sample_rows WITHOUT edits on
sampling.apply_logit_edits(logits, ...) -- the unchanged plain instantiation on a torch-edited copy, same random stream.
  * every branch (greedy, top-k with and without top-p, whole vocabulary plain / top-p / min_p) x every kind of list (bias only, bans only,
    allow-only, allow-only with biases, empty, none) x fp32 / bf16 / f16, with and without a penalty whose history overlaps the edited ids;
  * vocabularies: 2999 (emulator) / 4001, 50 288 and 65 536 (GPU), 5 and 257 (both); edits on token 0, token V - 1 and on the first and last
    lane of a stride;
  * what the kernel defines for contents the host cannot check; placement invariance; the copy fall-back; omk_sample_rows_form;
    capture and replay with rewritten edit tensors; SamplingParams validation and the merge rule of pack_edits."""
import math

import pytest
import torch

# (top_k, top_p, temperature, min_p): greedy | top-k 20 behind top-p | top-k 64 | whole vocabulary plain | behind top-p | behind min_p
SETTINGS = [(1, 0.0, 1.0, 0.0), (20, 0.9, 0.8, 0.0), (64, 0.0, 1.0, 0.0), (0, 0.0, 1.0, 0.0), (0, 0.9, 1.0, 0.0), (0, 0.0, 1.0, 0.05)]
KINDS = 6      # of edit lists: bias only | bans only | allow-only, 4 ids | allow-only with biases | empty (allow-only) | none
CAP = 24
NINF = float("-inf")


def _params(settings, n, penalty=1.0):
    from omnimamba_amd.sampling import SamplingParams
    seeds = [1000 + 37 * b for b in range(n)]
    seeds[-1] = 2 ** 64 - 5
    return [SamplingParams(top_k=k, top_p=tp, temperature=t, min_p=mp, seed=seeds[b], step0=3 + 11 * b, repetition_penalty=penalty)
            for b, (k, tp, t, mp) in enumerate(settings[b % len(settings)] for b in range(n))]


def _logits(V, n, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(n, V, generator=g) * 2.0).to(dtype)


def _special(V):
    """Token 0, token V - 1, and the first and last lane of a stride of the wave (64), of the emulator's workgroup (256), of the GPU's (1024)
    and of its four-deep pass (4096)."""
    return [i for i in dict.fromkeys([0, V - 1, 63, 64, 255, 256, 1023, 1024, 4095, 4096]) if 0 <= i < V]


def _edits(logits, shift):
    """Row b gets the list of kind (b + shift) % KINDS, built from the row's own ranking so that the edits change what is drawn.  Behind a
    row's length the arrays hold the row's arg max with +50: must not be read."""
    n, V = logits.shape
    g = torch.Generator().manual_seed(100 + shift)
    ids = torch.zeros(n, CAP, dtype=torch.int64)
    vals = torch.zeros(n, CAP, dtype=torch.float32)
    lens = torch.zeros(n, dtype=torch.int32)
    mode = torch.zeros(n, dtype=torch.int32)
    sp = _special(V)
    for b in range(n):
        kind = (b + shift) % KINDS
        order = torch.argsort(logits[b].float(), descending=True, stable=True).tolist()
        top = order[:6]
        mid = order[min(V - 1, 30): 36]
        if kind == 0:      # bias only: the top tokens down, a few special and middling ones up
            l = [(t, -4.0 - j) for j, t in enumerate(top[:3])] + [(t, 3.0 + 0.37 * j) for j, t in enumerate(sp + mid[:3])]
        elif kind == 1:    # bans only (at V = 5 two of the top tokens: a token must stay)
            l = [(t, NINF) for t in top[:min(5, V - 3)] + sp[:2]]
        elif kind == 2:    # allow-only, 4 ids, no biases
            l = [(t, 0.0) for t in list(dict.fromkeys([order[min(2, V - 1)], sp[0], sp[1], order[min(40, V - 2)], order[1]]))[:4]]
        elif kind == 3:    # allow-only with biases and one banned member
            l = [(t, float(torch.randn((), generator=g)) * 2.0) for t in dict.fromkeys(top[:3] + sp[:4] + mid[:2])]
            l[0] = (l[0][0], NINF)
        else:
            l = []
        l = list({t: v for t, v in reversed(l)}.items())[::-1]      # (an id once; small vocabularies repeat)
        ids[b] = order[0]
        vals[b] = 50.0
        for j, (t, v) in enumerate(l):
            ids[b, j], vals[b, j] = t, v
        lens[b] = len(l)
        mode[b] = 1 if kind in (2, 3, 4) else 0
    return {"edit_ids": ids, "edit_vals": vals, "edit_lens": lens, "edit_mode": mode}


def _history(logits, cap=40):
    """A history per row that holds the row's top tokens (which the lists of _edits bias, ban or allow), token 0 and token V - 1."""
    n, V = logits.shape
    g = torch.Generator().manual_seed(5)
    h = torch.zeros(n, cap, dtype=torch.int64)
    for b in range(n):
        top = torch.topk(logits[b].float(), min(8, V)).indices
        h[b] = torch.cat([top, torch.tensor([0, V - 1]), torch.randint(0, V, (cap,), generator=g)])[:cap]
    return h, torch.full((n,), cap - 3, dtype=torch.int32)


def _to(d, dev):
    return {k: v.to(dev) for k, v in d.items()}


def _fused(logits, params, ed, hist=None, **kw):
    from omnimamba_amd.sampling import pack_rows, sample_rows
    pk = pack_rows(params, logits.device)
    if hist is None:
        pk.pop("penalty")
        return sample_rows(logits, **pk, **ed, **kw)
    return sample_rows(logits, **pk, **ed, history=hist[0], history_lens=hist[1], **kw)


def _oracle(logits, params, ed, hist=None, **kw):
    """The plain launch on a copy edited with torch."""
    from omnimamba_amd.sampling import apply_logit_edits, pack_rows, sample_rows, sample_rows_form
    pk = pack_rows(params, logits.device)
    pen = pk.pop("penalty")
    work = apply_logit_edits(logits, **ed) if hist is None else apply_logit_edits(logits, **ed, penalty=pen, history=hist[0], history_lens=hist[1])
    assert sample_rows_form(work, **pk) == 0
    return sample_rows(work, **pk, **kw)


def _check(dev, V, dtype, shift, pen, n=8, seed=0):
    from omnimamba_amd.sampling import sample_rows_form, pack_rows
    logits_h = _logits(V, n, dtype, seed)
    params = _params(SETTINGS, n, penalty=1.3 if pen else 1.0)
    ed_h = _edits(logits_h, shift)
    logits, ed = logits_h.to(dev), _to(ed_h, dev)
    hist = tuple(t.to(dev) for t in _history(logits_h)) if pen else None
    before = logits.clone()
    assert sample_rows_form(logits, **{k: v for k, v in pack_rows(params, dev).items() if k != "penalty"}, **ed) == 2
    got = _fused(logits, params, ed, hist).cpu()
    assert torch.equal(logits.view(torch.uint8), before.view(torch.uint8)), "the launch wrote to logits"
    want = _oracle(logits, params, ed, hist).cpu()
    assert torch.equal(got, want), (V, dtype, shift, pen, got.tolist(), want.tolist())
    # the lists mean what they say, and the case tests something
    plain = _fused(logits, params, {}, hist).cpu()
    for b in range(n):
        kind, L = (b + shift) % KINDS, int(ed_h["edit_lens"][b])
        row_ids, row_vals = ed_h["edit_ids"][b, :L].tolist(), ed_h["edit_vals"][b, :L].tolist()
        if kind in (2, 3):
            assert int(got[b]) in [t for t, v in zip(row_ids, row_vals) if v != NINF], (b, kind)
        if kind == 1:
            assert int(got[b]) not in row_ids
        if kind in (4, 5):
            assert int(got[b]) == int(plain[b])
    return int((got != plain).sum())


@pytest.mark.parametrize("pen", [False, True])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_every_branch_and_every_kind_of_list_equal_the_plain_launch_on_an_edited_copy(dev, dtype, pen):
    """Six shifts: every one of the six branches meets every one of the six kinds of list."""
    V = 4001 if dev.type == "cuda" else 2999
    changed = sum(_check(dev, V, dtype, shift, pen) for shift in range(KINDS))
    assert changed >= 16, "the edits changed almost nothing: the case does not test them"


@pytest.mark.gpu
@pytest.mark.parametrize("V,dtype", [(50288, torch.float32), (50288, torch.bfloat16), (65536, torch.float32)])
def test_the_mmu_vocabulary_and_the_largest_map(V, dtype):
    """50 288: the MMU vocabulary with the full LDS budget (map + list + the 44 792 static bytes), one case per dtype width; 65 536: the
    largest id map.  With a penalty, so every part of the preamble runs."""
    dev = torch.device("cuda:0")
    assert _check(dev, V, dtype, 0, True) + _check(dev, V, dtype, 3, False) >= 4


@pytest.mark.parametrize("V", [5, 257])
@pytest.mark.parametrize("pen", [False, True])
def test_a_row_shorter_than_the_workgroup_and_the_first_size_past_a_lane_stride(dev, V, pen):
    for dtype in (torch.float32, torch.bfloat16):
        for shift in range(KINDS):
            _check(dev, V, dtype, shift, pen)


def test_contents_the_kernel_defines(dev):
    """A duplicated id: the first entry wins.  Ids -1, V and +-2^40 are skipped.  edit_lens below 0 and above the cap are clamped.  A mode
    other than 1 counts as 0.  An allow-only list of invalid ids only leaves the row unconstrained.  An inactive row with garbage in its
    edit arrays writes nothing.  Every row is greedy or top-k 8 at a fixed seed; `dirty` must draw what `clean` draws."""
    V, n, cap = 1501, 8, 6
    logits_h = _logits(V, n, torch.float32, 4)
    top = torch.topk(logits_h, 3).indices            # (n, 3)
    t0, t1, t2 = top[:, 0].tolist(), top[:, 1].tolist(), top[:, 2].tolist()
    params = _params([(1, 0.0, 1.0, 0.0), (8, 0.0, 1.0, 0.0)], n)
    G = 2 ** 40
    dirty = {
        "edit_ids": torch.tensor([[t0[0], t0[0], 0, 0, 0, 0],              # 0: duplicate, ban first then +50: banned
                                  [t1[1], t1[1], t0[1], 0, 0, 0],          # 1: duplicate, +60 first then ban: boosted; the arg max banned
                                  [-1, V, G, -G, t0[2], V + 7],            # 2: invalid ids around one valid ban
                                  [t0[3], t1[3], 0, 0, 0, 0],              # 3: length -3: nothing applies
                                  [t0[4]] * 6,                             # 4: length 1000: clamped to the cap
                                  [t0[5], 0, 0, 0, 0, 0],                  # 5: mode 7 is mode 0: a ban, not an allowed set
                                  [-1, V, G, 0, 0, 0],                     # 6: allow-only, no valid id: unconstrained
                                  [G, -G, 7, 7, 7, 7]], dtype=torch.int64),  # 7: inactive
        "edit_vals": torch.tensor([[NINF, 50.0, 0, 0, 0, 0], [60.0, NINF, NINF, 0, 0, 0], [NINF] * 6, [NINF, NINF, 0, 0, 0, 0], [NINF] * 6,
                                   [NINF, 0, 0, 0, 0, 0], [0.0] * 6, [float("nan")] * 6], dtype=torch.float32),
        "edit_lens": torch.tensor([2, 3, 6, -3, 1000, 1, 3, 10 ** 6], dtype=torch.int32),
        "edit_mode": torch.tensor([0, 0, 0, 0, 0, 7, 1, 99], dtype=torch.int32),
    }
    clean = {
        "edit_ids": torch.tensor([[t0[0], 0, 0], [t1[1], t0[1], 0], [t0[2], 0, 0], [0, 0, 0], [t0[4], 0, 0], [t0[5], 0, 0], [0, 0, 0], [0, 0, 0]], dtype=torch.int64),
        "edit_vals": torch.tensor([[NINF, 0, 0], [60.0, NINF, 0], [NINF, 0, 0], [0, 0, 0], [NINF, 0, 0], [NINF, 0, 0], [0, 0, 0], [0, 0, 0]], dtype=torch.float32),
        "edit_lens": torch.tensor([1, 2, 1, 0, 1, 1, 0, 0], dtype=torch.int32),
        "edit_mode": torch.zeros(n, dtype=torch.int32),
    }
    logits = logits_h.to(dev)
    active = torch.tensor([1] * 7 + [0], dtype=torch.int32).to(dev)
    out = torch.full((n,), -7, dtype=torch.int64, device=dev)
    got = _fused(logits, params, _to(dirty, dev), active=active, out=out).cpu()
    want = _fused(logits, params, _to(clean, dev)).cpu()
    plain = _fused(logits, params, {}).cpu()
    assert torch.equal(got[:7], want[:7]) and int(got[7]) == -7, (got.tolist(), want.tolist())
    assert torch.equal(got[:7], _oracle(logits, params, _to(dirty, dev)).cpu()[:7])
    assert int(got[0]) == t1[0] and int(got[1]) == t1[1] and int(got[2]) == t1[2] and int(got[4]) == t1[4]
    assert int(got[3]) == int(plain[3]) and int(got[6]) == int(plain[6])
    assert int(got[5]) != t0[5] and int(got[5]) == int(want[5])
    # without the flags the neighbours are what they were
    assert torch.equal(_fused(logits[:7], params[:7], {k: v[:7].contiguous() for k, v in _to(dirty, dev).items()}).cpu(), got[:7])


def test_placement_invariance(dev):
    """A row's id is the same alone, at another row index, and beside other neighbours."""
    V = 4001 if dev.type == "cuda" else 2999
    n = 8
    logits_h = _logits(V, n, torch.bfloat16, 11)
    params = _params(SETTINGS, n, penalty=1.3)
    ed_h = _edits(logits_h, 1)
    hist_h = _history(logits_h)
    logits, ed, hist = logits_h.to(dev), _to(ed_h, dev), tuple(t.to(dev) for t in hist_h)
    ids = _fused(logits, params, ed, hist).cpu()
    perm = torch.tensor([5, 2, 7, 0, 3, 6, 1, 4])
    pd = perm.to(dev)
    got = _fused(logits[pd].contiguous(), [params[i] for i in perm.tolist()], {k: v[pd].contiguous() for k, v in ed.items()},
                 tuple(t[pd].contiguous() for t in hist)).cpu()
    assert torch.equal(got, ids[perm])
    # among other rows (other logits, other lists, other histories) ...
    o_logits_h = _logits(V, 5, torch.bfloat16, 12)
    o_ed, o_hist, o_params = _edits(o_logits_h, 4), _history(o_logits_h), _params(SETTINGS[::-1], 5, penalty=1.7)
    place = [1, 2, 4, 5, 6, 9, 10, 12]
    src = [("m", place.index(r)) if r in place else ("o", r - sum(p < r for p in place)) for r in range(n + 5)]
    pick = lambda a, b: torch.stack([(a if w == "m" else b)[j] for w, j in src])
    mixed = _fused(pick(logits_h, o_logits_h).to(dev), [(params if w == "m" else o_params)[j] for w, j in src],
                   _to({k: pick(ed_h[k], o_ed[k]) for k in ed_h}, dev), tuple(pick(a, b).to(dev) for a, b in zip(hist_h, o_hist))).cpu()
    assert torch.equal(mixed[torch.tensor(place)], ids)
    # ... and each of them alone
    for b in range(n):
        one = _fused(logits[b:b + 1], params[b:b + 1], {k: v[b:b + 1] for k, v in ed.items()}, tuple(t[b:b + 1] for t in hist))
        assert int(one[0]) == int(ids[b]), b


def test_a_list_or_a_vocabulary_too_large_for_the_kernel_edits_a_copy(dev):
    """edit_cap = MAX_EDITS + 1 and V = 65 600 (deliberately above the other sizes: the id map holds 65 536 tokens) are declined by the
    library (omk_sample_rows_form < 0) and sample_rows draws from a copy: the oracle's ids, and those of the fused launch on the same lists
    in arrays the kernel takes."""
    from omnimamba_amd.sampling import MAX_EDITS, pack_rows, sample_rows_form
    assert MAX_EDITS >= 256
    V, n = 1501, 4
    logits_h = _logits(V, n, torch.float32, 8)
    params = _params(SETTINGS, n, penalty=1.3)
    small = _edits(logits_h, 0)
    wide = {k: (torch.cat([v, torch.zeros(n, MAX_EDITS + 1 - CAP, dtype=v.dtype)], 1) if v.dim() == 2 else v) for k, v in small.items()}
    logits, hist = logits_h.to(dev), tuple(t.to(dev) for t in _history(logits_h))
    pk = pack_rows(params, dev)
    assert sample_rows_form(logits, **pk, **_to(wide, dev), history=hist[0], history_lens=hist[1]) == -4
    assert sample_rows_form(logits, **pk, **_to(small, dev), history=hist[0], history_lens=hist[1]) == 2
    got = _fused(logits, params, _to(wide, dev), hist).cpu()
    assert torch.equal(got, _oracle(logits, params, _to(wide, dev), hist).cpu())
    assert torch.equal(got, _fused(logits, params, _to(small, dev), hist).cpu())
    # the vocabulary: two rows, greedy and top-k 20
    V = 65600
    logits_h = _logits(V, 2, torch.float32, 9)
    params = _params(SETTINGS, 2)
    ed = _edits(logits_h, 1)                     # row 0 bans its top tokens, row 1 is allow-only
    logits = logits_h.to(dev)
    pk = pack_rows(params, dev)
    pk.pop("penalty")
    assert sample_rows_form(logits, **pk, **_to(ed, dev)) == -4
    got = _fused(logits, params, _to(ed, dev)).cpu()
    assert torch.equal(logits.cpu(), logits_h)
    assert torch.equal(got, _oracle(logits, params, _to(ed, dev)).cpu())
    assert int(got[0]) == int(torch.topk(logits_h[0], 6).indices[5]) and int(got[1]) in ed["edit_ids"][1, :4].tolist()


def test_the_form_of_a_launch(dev):
    """omk_sample_rows_form: 0 plain, 1 penalty map, 2 edits, < 0 the status of a refused call.  No edit array, or an edit_cap of 0, is the
    parent's launch."""
    from omnimamba_amd.sampling import pack_rows, sample_rows, sample_rows_form
    V, n = 257, 3
    logits = _logits(V, n, torch.float32, 1).to(dev)
    pk = pack_rows(_params(SETTINGS, n, penalty=1.3), dev)
    pen = pk.pop("penalty")
    ed = _to(_edits(logits.cpu(), 0), dev)
    hist = tuple(t.to(dev) for t in _history(logits.cpu()))
    hk = dict(penalty=pen, history=hist[0], history_lens=hist[1])
    assert sample_rows_form(logits, **pk) == 0
    assert sample_rows_form(logits, **pk, penalty=pen) == 0                  # (no history: nothing to penalise)
    assert sample_rows_form(logits, **pk, **hk) == 1
    assert sample_rows_form(logits, **pk, **ed) == 2
    assert sample_rows_form(logits, **pk, **ed, **hk) == 2
    empty = {**ed, "edit_ids": ed["edit_ids"][:, :0], "edit_vals": ed["edit_vals"][:, :0]}
    assert sample_rows_form(logits, **pk, **empty) == 0 and sample_rows_form(logits, **pk, **empty, **hk) == 1
    assert torch.equal(sample_rows(logits, **pk, **empty, **hk), sample_rows(logits, **pk, **hk))
    assert sample_rows_form(logits, **pk, **{**ed, "edit_lens": None}) == -1
    assert sample_rows_form(logits, **pk, **{**ed, "edit_vals": None}) == -1
    assert sample_rows_form(logits, **{**pk, "top_k": None}) == -1
    with pytest.raises(RuntimeError, match="omk_status -1"):
        sample_rows(logits, **pk, **{**ed, "edit_lens": None})
    no_mode = {k: v for k, v in ed.items() if k != "edit_mode"}                # edit_mode is optional: 0 everywhere
    assert sample_rows_form(logits, **pk, **no_mode) == 2
    assert torch.equal(sample_rows(logits, **pk, **no_mode), sample_rows(logits, **pk, **{**ed, "edit_mode": torch.zeros_like(ed["edit_mode"])}))


def test_a_row_with_every_token_banned_returns_an_id_of_the_vocabulary():
    """V = 5, every token -inf, every branch: an unspecified id in [0, 5), in bounded time.  Under the emulator only."""
    from emu.loader import use_emulator
    with use_emulator():
        V, n = 5, 6
        logits = _logits(V, n, torch.float32, 2)
        ed = {"edit_ids": torch.arange(V).repeat(n, 1), "edit_vals": torch.full((n, V), NINF), "edit_lens": torch.full((n,), V, dtype=torch.int32),
              "edit_mode": torch.tensor([0, 1] * 3, dtype=torch.int32)}
        got = _fused(logits, _params(SETTINGS, n), ed)
        assert ((got >= 0) & (got < V)).all(), got.tolist()


@pytest.mark.gpu
@torch.inference_mode()
def test_capture_and_replay_with_rewritten_edits():
    """The launch inside a captured graph (the capture pattern of tests/test_sampling_rows.py's replay test): the edit tensors are rewritten
    between two replays and the ids follow the new contents."""
    from omnimamba_amd.sampling import pack_rows, sample_rows
    dev = torch.device("cuda:0")
    V, n = 4001, 8
    logits_h = _logits(V, n, torch.float32, 0)
    params = _params(SETTINGS, n, penalty=1.3)
    ed1, ed2 = _to(_edits(logits_h, 0), dev), _to(_edits(logits_h, 3), dev)
    logits, hist = logits_h.to(dev), tuple(t.to(dev) for t in _history(logits_h))
    ed = {k: v.clone() for k, v in ed1.items()}
    out = torch.full((n,), -1, dtype=torch.int64, device=dev)
    pk = pack_rows(params, dev)                    # (static across the replays: the captured launch reads these tensors)
    run = lambda: sample_rows(logits, **pk, **ed, history=hist[0], history_lens=hist[1], out=out)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            run()
        s.synchronize()
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run()
    out.fill_(-1)
    graph.replay()
    got1 = out.clone()
    for k in ed:
        ed[k].copy_(ed2[k])
    graph.replay()
    got2 = out.clone()
    torch.cuda.synchronize()
    e1 = _fused(logits, params, ed1, hist).clone()
    e2 = _fused(logits, params, ed2, hist).clone()
    assert torch.equal(got1, e1) and torch.equal(got2, e2)
    assert not torch.equal(got1, got2)


def test_sampling_params_constraints_validate_on_construction():
    from omnimamba_amd.sampling import SamplingParams as SP
    p = SP()
    assert (p.logit_bias, p.allowed_token_ids, p.banned_token_ids, p.min_new_tokens) == ((), None, (), 0)
    for bad in (dict(allowed_token_ids=[]), dict(logit_bias={3: math.inf}), dict(logit_bias={3: math.nan}), dict(logit_bias=[(3, math.inf)]),
                dict(min_new_tokens=-1)):
        with pytest.raises(ValueError):
            SP(**bad)
    p = SP(logit_bias={7: 1.5, 9: -math.inf}, allowed_token_ids=[4, 7], banned_token_ids=[9], min_new_tokens=2)
    assert p.logit_bias == ((7, 1.5), (9, -math.inf)) and p.allowed_token_ids == (4, 7) and p.banned_token_ids == (9,)
    assert SP(logit_bias=[(7, 1.5)]).logit_bias == ((7, 1.5),)
    hash(p)


def test_pack_edits_follows_the_merge_rule():
    from omnimamba_amd.sampling import SamplingParams as SP, pack_edits
    params = [SP(),                                                                       # nothing
              SP(logit_bias={5: 1.0, 6: -2.0}, banned_token_ids=[6, 8, 8]),               # bias keys + banned ids, a banned id is -inf
              SP(allowed_token_ids=[3, 4, 3, 9], logit_bias={4: 0.5, 77: 9.0}, banned_token_ids=[9, 100]),   # the set; bias outside it dropped
              SP(allowed_token_ids=[2]),
              SP(logit_bias=[(5, 1.0), (5, 2.0)])]
    e = pack_edits(params, torch.device("cpu"), extra_bans=[[], [11], [4], [50], []])
    rows = [list(zip(e["edit_ids"][b, :n].tolist(), e["edit_vals"][b, :n].tolist())) for b, n in enumerate(e["edit_lens"].tolist())]
    assert e["edit_mode"].tolist() == [0, 0, 1, 1, 0]
    assert e["edit_ids"].dtype == torch.int64 and e["edit_vals"].dtype == torch.float32 and e["edit_lens"].dtype == torch.int32 and e["edit_mode"].dtype == torch.int32
    assert e["edit_ids"].shape == e["edit_vals"].shape == (5, 4)
    assert rows[0] == []
    assert rows[1] == [(11, NINF), (5, 1.0), (6, NINF), (8, NINF)]
    assert rows[2] == [(4, NINF), (3, 0.0), (9, NINF)]
    assert rows[3] == [(50, NINF), (2, 0.0)]
    assert rows[4] == [(5, 1.0)]
    assert pack_edits(params[:1], torch.device("cpu"))["edit_ids"].shape == (1, 1)
