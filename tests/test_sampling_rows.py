"""The row-wise sampler (omk_sample_rows, ABI 14; omnimamba_amd.sampling.sample_rows): every row of one launch is sampled with its own
settings, seed and stream position, and -- optionally -- behind its own repetition penalty.
  * a row equals the scalar launch (omk_sample) of that row alone with seed = seeds[b], offset = steps[b], for every branch, as exact ids;
  * a row's id does not depend on its place in the batch or on its neighbours;
  * the fused penalty equals the scalar launch on generation.modify_logit_for_repetition_penalty(clone) and never writes the logits;
  * distinct steps of one seed are independent streams (chi-square against the reference's probabilities);
  * inactive rows write nothing; values in the device arrays that the host cannot check are clamped / skipped by the kernel;
  * the launch is capturable and replays with rewritten setting tensors."""
import math

import pytest
import torch

from test_sampling import ref_distribution

# (top_k, top_p, temperature, min_p): argmax | 2..64 candidates, with and without top-p | plain whole vocabulary | whole vocabulary behind top-p | min_p
SETTINGS = [(1, 0.0, 1.0, 0.0), (8, 0.0, 0.7, 0.0), (64, 0.6, 1.0, 0.0), (3, 0.999, 1.0, 0.0), (0, 0.0, 1.0, 0.0), (0, 0.9, 1.0, 0.0), (0, 0.0, 1.0, 0.05)]


def _params(settings, seeds, steps, penalty=None):
    from omnimamba_amd.sampling import SamplingParams
    return [SamplingParams(top_k=k, top_p=tp, temperature=t, min_p=mp, seed=sd, step0=st, repetition_penalty=1.0 if penalty is None else penalty[i])
            for i, ((k, tp, t, mp), sd, st) in enumerate(zip(settings, seeds, steps))]


def _rows(logits, params, **kw):
    from omnimamba_amd.sampling import pack_rows, sample_rows
    pk = pack_rows(params, logits.device)
    if "history" not in kw:
        pk.pop("penalty")
    return sample_rows(logits, **pk, **kw)


def _scalar(logits_row, p):
    from omnimamba_amd.sampling import sample_device
    return int(sample_device(logits_row, top_k=p.top_k, top_p=p.top_p, temperature=p.temperature, min_p=p.min_p, seed=p.seed, offset=p.step0)[0])


def _case(dev, dtype, big=True, nrow=8, seed=0):
    """nrow rows of different random logits, the settings cycling through SETTINGS, distinct seeds and steps."""
    g = torch.Generator().manual_seed(seed)
    V = (50288 if big else 4001) if dev.type == "cuda" else 2999
    logits = (torch.randn(nrow, V, generator=g) * 2.0).to(dtype)
    settings = [SETTINGS[b % len(SETTINGS)] for b in range(nrow)]
    if dtype != torch.float32:           # (16-bit rows tie: the kernel takes the lowest index, torch.argmax any)
        for b in range(nrow):
            if settings[b][0] == 1:
                logits[b, 17 * (b + 1)] = 11.0
    seeds = [1000 + 37 * b for b in range(nrow)]
    seeds[-1] = 2 ** 64 - 5              # (the whole 64 bits of a seed reach the key)
    steps = [3 + 11 * b for b in range(nrow)]
    steps[-2] = 2 ** 33 + 1              # (and both counter words of a step)
    return logits.to(dev), _params(settings, seeds, steps)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_a_row_equals_its_scalar_launch_for_every_branch(dev, dtype):
    logits, params = _case(dev, dtype, big=dtype == torch.float32)
    ids = _rows(logits, params).cpu().tolist()
    want = [_scalar(logits[b:b + 1], p) for b, p in enumerate(params)]
    assert ids == want
    for b, p in enumerate(params):
        if p.top_k == 1:
            assert ids[b] == int(logits[b].float().argmax())


def test_placement_invariance(dev):
    logits, params = _case(dev, torch.float32, big=False)
    n = len(params)
    ids = _rows(logits, params).cpu()
    perm = torch.tensor([5, 2, 7, 0, 3, 6, 1, 4])
    assert torch.equal(_rows(logits[perm.to(dev)].contiguous(), [params[i] for i in perm.tolist()]).cpu(), ids[perm])
    # the same rows among other rows ...
    other, oparams = _case(dev, torch.float32, big=False, nrow=5, seed=9)
    place = [1, 2, 4, 5, 6, 9, 10, 12]
    mixed, mparams, o = [], [], 0
    for r in range(n + 5):
        if r in place:
            j = place.index(r)
            mixed.append(logits[j]); mparams.append(params[j])
        else:
            mixed.append(other[o]); mparams.append(oparams[o]); o += 1
    got = _rows(torch.stack(mixed), mparams).cpu()
    assert torch.equal(got[torch.tensor(place)], ids)
    # ... and each of them alone
    for b in range(n):
        assert int(_rows(logits[b:b + 1], params[b:b + 1])[0]) == int(ids[b])


def _penalty_case(dev, dtype, pen):
    """Per setting (top_k 1, top_k 20, top_k 0 behind top-p): histories of length 0, of length 1 (the arg max), with duplicates, and of 1100
    ids (more than one per thread of the workgroup); the largest logits of a row are in its history, so the penalty changes the candidates.
    The last row has penalty 1.0 and a history."""
    g = torch.Generator().manual_seed(3)
    V = (50288 if dtype == torch.float32 and pen != 2.0 else 4001) if dev.type == "cuda" else 2999
    cap = 1100
    settings, hists = [], []
    for st in [(1, 0.0, 1.0, 0.0), (20, 0.0, 0.8, 0.0), (0, 0.9, 1.0, 0.0)]:
        for kind in range(4):
            settings.append(st)
            hists.append(kind)
    settings.append((20, 0.0, 0.8, 0.0))
    hists.append(2)
    n = len(settings)
    logits = (torch.randn(n, V, generator=g) * 2.0).to(dtype)
    history = torch.zeros(n, cap, dtype=torch.int64)
    lens = torch.zeros(n, dtype=torch.int32)
    for b, kind in enumerate(hists):
        top = torch.topk(logits[b].float(), 12).indices
        low = torch.topk(-logits[b].float(), 4).indices
        if kind == 1:
            h = top[:1]
        elif kind == 2:
            h = torch.cat([top[:6], low, top[:3], top[:1], torch.randint(0, V, (9,), generator=g), top[:6]])
        elif kind == 3:
            h = torch.cat([top, low, torch.randint(0, V, (cap - 16,), generator=g)])[torch.randperm(cap, generator=g)]
        else:
            h = top[:0]
        history[b, :h.numel()] = h
        history[b, h.numel():] = int(top[0])            # behind the length: must not be read as history
        lens[b] = h.numel()
        if h.numel():
            sc = logits[b].float()[h]
            assert (sc > 0).any() and (kind == 1 or (sc < 0).any())
    pens = [pen] * (n - 1) + [1.0]
    params = _params(settings, [77 + b for b in range(n)], [5 * b for b in range(n)], penalty=pens)
    return logits, history, lens, params


@pytest.mark.parametrize("pen", [2.0, 1.3])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_repetition_penalty_equals_the_scalar_launch_on_penalised_logits(dev, dtype, pen):
    from omnimamba_amd.generation import modify_logit_for_repetition_penalty
    logits_h, history, lens, params = _penalty_case(dev, dtype, pen)
    logits = logits_h.to(dev)
    before = logits.clone()
    ids = _rows(logits, params, history=history.to(dev), history_lens=lens.to(dev)).cpu().tolist()
    assert torch.equal(logits.view(torch.uint8), before.view(torch.uint8)), "the launch wrote to logits"
    changed = 0
    for b, p in enumerate(params):
        mod = modify_logit_for_repetition_penalty(logits_h[b:b + 1].clone(), history[b:b + 1, :int(lens[b])], p.repetition_penalty)
        assert ids[b] == _scalar(mod.to(dev), p), (b, p)
        changed += ids[b] != _scalar(logits[b:b + 1], p)
    assert changed >= 4, "the penalty changed almost nothing: the case does not test it"
    # penalty 1.0 with a history: the launch without history
    assert ids[-1] == int(_rows(logits[-1:], params[-1:])[0])
    # ... and no penalty array at all is penalty 1.0 everywhere
    from omnimamba_amd.sampling import pack_rows, sample_rows
    pk = pack_rows(params, dev)
    pk.pop("penalty")
    assert torch.equal(sample_rows(logits, **pk, history=history.to(dev), history_lens=lens.to(dev)), _rows(logits, params))


def test_array_contents_are_clamped_by_the_kernel(dev):
    """What the host cannot check: top_k outside [0, 64], history ids outside [0, V), history_lens outside [0, cap]."""
    from omnimamba_amd.sampling import pack_rows, sample_rows
    g = torch.Generator().manual_seed(4)
    V = 1501
    logits = (torch.randn(4, V, generator=g) * 2.0).to(dev)
    params = _params([(64, 0.0, 1.0, 0.0), (0, 0.0, 1.0, 0.0), (1, 0.0, 1.0, 0.0), (1, 0.0, 1.0, 0.0)], [1, 2, 3, 4], [5, 6, 7, 8], penalty=[1.0, 1.0, 1.5, 1.5])
    top = logits.cpu().argmax(-1)
    hist = torch.tensor([[0] * 6, [0] * 6, [-1, V, 2 ** 40, -2 ** 40, int(top[2]), V + 7], [int(top[3])] * 6], dtype=torch.int64)
    lens = torch.tensor([0, -4, 6, 1000], dtype=torch.int32)
    clean_hist = torch.tensor([[0] * 6, [0] * 6, [int(top[2])] * 6, [int(top[3])] * 6], dtype=torch.int64)
    clean = _rows(logits, params, history=clean_hist.to(dev), history_lens=torch.tensor([0, 0, 6, 6], dtype=torch.int32).to(dev))
    pk = pack_rows(params, dev)
    pk["top_k"] = torch.tensor([1000, -3, 1, 1], dtype=torch.int32).to(dev)
    got = sample_rows(logits, **pk, history=hist.to(dev), history_lens=lens.to(dev))
    assert torch.equal(got, clean)
    assert int(got[2]) != int(top[2]) and int(got[3]) != int(top[3])      # (the one valid id was penalised)


def test_vocabulary_too_large_for_the_id_map_is_penalised_on_a_copy(dev):
    from omnimamba_amd.generation import modify_logit_for_repetition_penalty
    g = torch.Generator().manual_seed(6)
    # Deliberately larger than the sizes of the other tests (V <= 3000 under the emulator): the id map of the penalty launch holds 65 536
    # tokens, so the path that penalises a copy exists only above that.  Two rows, top_k 1 and 5: well under a second on the CPU.
    V = 65600
    logits_h = torch.randn(2, V, generator=g) * 2.0
    params = _params([(1, 0.0, 1.0, 0.0), (5, 0.0, 1.0, 0.0)], [1, 2], [3, 4], penalty=[1.3, 1.3])
    history = torch.zeros(2, 8, dtype=torch.int64)
    for b in range(2):
        history[b, :5] = torch.topk(logits_h[b], 3).indices[[0, 1, 2, 0, 0]]
    lens = torch.tensor([5, 5], dtype=torch.int32)
    logits = logits_h.to(dev)
    ids = _rows(logits, params, history=history.to(dev), history_lens=lens.to(dev)).cpu().tolist()
    assert torch.equal(logits.cpu(), logits_h)
    for b, p in enumerate(params):
        mod = modify_logit_for_repetition_penalty(logits_h[b:b + 1].clone(), history[b:b + 1, :5], 1.3)
        assert ids[b] == _scalar(mod.to(dev), p)
    assert ids[0] != int(logits_h[0].argmax())


def test_steps_of_one_seed_are_independent_streams(dev):
    """The (20, 0.9, 0.7) chi-square case of test_sampling.test_topk_topp_distribution_matches_reference, drawn through the row-wise entry
    with steps 0 .. n - 1 of ONE seed (the row index is no longer in the Philox counter: the step alone separates the draws)."""
    from omnimamba_amd.sampling import SamplingParams, pack_rows, sample_rows
    top_k, top_p, temp = 20, 0.9, 0.7
    g = torch.Generator().manual_seed(1)
    V = 16384 if dev.type == "cuda" else 700
    row = torch.randn(V, generator=g) * 2.0
    p_ref = ref_distribution(row, top_k, top_p, temp)
    support = (p_ref > 0).nonzero().squeeze(-1)
    nrow, nlaunch = (256, 16) if dev.type == "cuda" else (48, 14)
    logits = row[None].repeat(nrow, 1).contiguous().to(dev)
    pk = pack_rows([SamplingParams(top_k=top_k, top_p=top_p, temperature=temp, seed=1234)] * nrow, dev)
    pk.pop("penalty")
    counts = torch.zeros(V, dtype=torch.float64)
    for i in range(nlaunch):
        pk["steps"] = torch.arange(i * nrow, (i + 1) * nrow, dtype=torch.int64).to(dev)
        counts += torch.bincount(sample_rows(logits, **pk).cpu(), minlength=V).double()
    n = nrow * nlaunch
    assert counts.sum() == n
    assert (counts[p_ref == 0] == 0).all(), "a token outside the reference's candidate set was drawn"
    exp = p_ref[support] * n
    obs = counts[support]
    big = exp >= 5
    chi = (((obs[big] - exp[big]) ** 2) / exp[big]).sum().item()
    dof = int(big.sum().item()) - 1
    if (~big).any():
        e, o = exp[~big].sum().item(), obs[~big].sum().item()
        if e > 0:
            chi += (o - e) ** 2 / e
            dof += 1
    print(f"chi-square {chi:.2f} at {dof} degrees of freedom")
    assert chi < dof + 5 * math.sqrt(2 * max(dof, 1)) + 5, (chi, dof)


def test_inactive_rows_write_nothing(dev):
    from omnimamba_amd.sampling import pack_rows, sample_rows
    logits, params = _case(dev, torch.float32, big=False)
    ids = _rows(logits, params)
    active = torch.tensor([1, 0, 1, 1, 0, 0, 1, 0], dtype=torch.int32)
    pk = pack_rows(params, dev)
    pk.pop("penalty")
    for name in ("top_k", "top_p", "min_p", "seeds", "steps"):        # what a retired row leaves behind may be anything representable
        pk[name][active.to(dev) == 0] = 0
    pk["temperature"][active.to(dev) == 0] = 1.0
    out = torch.full((8,), -7, dtype=torch.int64, device=dev)
    got = sample_rows(logits, **pk, active=active.to(dev), out=out)
    assert got is out
    assert torch.equal(out.cpu(), torch.where(active == 1, ids.cpu(), torch.full((8,), -7)))


def test_sampling_params_validate_on_construction():
    from omnimamba_amd.sampling import SamplingParams
    p = SamplingParams()
    assert (p.top_k, p.top_p, p.min_p, p.temperature, p.repetition_penalty, p.seed, p.step0) == (1, 0.0, 0.0, 1.0, 1.0, 0, 0)
    with pytest.raises(Exception):
        p.top_k = 2                                                    # frozen
    for bad in (dict(top_k=65), dict(top_k=-1), dict(temperature=0.0), dict(temperature=-1.0), dict(top_p=1.5), dict(min_p=-0.1, top_k=0),
                dict(min_p=1.0, top_k=0), dict(min_p=0.1, top_k=4), dict(repetition_penalty=0.0), dict(repetition_penalty=-2.0)):
        with pytest.raises(ValueError):
            SamplingParams(**bad)
    SamplingParams(top_k=0, min_p=0.1, top_p=1.0, temperature=0.5, repetition_penalty=1.3, seed=2 ** 64 - 1, step0=9)


def test_missing_arrays_are_refused(dev):
    from omnimamba_amd.sampling import pack_rows, sample_rows
    logits, params = _case(dev, torch.float32, big=False)
    pk = pack_rows(params, dev)
    pk.pop("penalty")
    for name in ("top_k", "top_p", "temperature", "min_p", "seeds", "steps"):
        with pytest.raises(RuntimeError, match="omk_status -1"):
            sample_rows(logits, **{**pk, name: None})
    with pytest.raises(RuntimeError, match="omk_status -1"):
        sample_rows(logits, **pk, history=torch.zeros(8, 4, dtype=torch.int64, device=dev))


@pytest.mark.gpu
@torch.inference_mode()
def test_capture_and_replay_with_rewritten_steps():
    """The launch inside a captured graph (the capture pattern of batch_decode._Bucket): the steps tensor is rewritten between two replays,
    and both replays equal the eager launches.  Runs with the process's default hardware queues.  Under inference_mode, as _Bucket
    captures inside decode_ragged: a capture registers the CUDA generator's graph state, and once an earlier capture of the process has
    made that state under inference_mode, a capture outside it is refused by torch."""
    from omnimamba_amd.sampling import pack_rows, sample_rows
    dev = torch.device("cuda:0")
    logits, params = _case(dev, torch.float32, big=False)
    pk = pack_rows(params, dev)
    history = torch.randint(0, logits.shape[1], (8, 40), device=dev)
    lens = torch.full((8,), 40, dtype=torch.int32, device=dev)
    pk["penalty"] = torch.full((8,), 1.3, device=dev)
    steps1, steps2 = pk["steps"].clone(), pk["steps"] + 100
    out = torch.full((8,), -1, dtype=torch.int64, device=dev)
    run = lambda: sample_rows(logits, **pk, history=history, history_lens=lens, out=out)
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
    pk["steps"].copy_(steps2)
    graph.replay()
    got2 = out.clone()
    torch.cuda.synchronize()
    e2 = sample_rows(logits, **pk, history=history, history_lens=lens).clone()
    pk["steps"].copy_(steps1)
    e1 = sample_rows(logits, **pk, history=history, history_lens=lens)
    assert torch.equal(got1, e1) and torch.equal(got2, e2)
    assert not torch.equal(got1, got2)
