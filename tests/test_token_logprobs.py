"""Log-probabilities behind the sampler (omk_token_logprobs, ABI 15; omnimamba_amd.sampling.token_logprobs): per row of logits the
log-probability of a given token, its rank, and the top_n most likely tokens, all of the raw row.

Reference: torch.log_softmax of the logits viewed as fp64; top_n and rank from a stable descending sort of the same values (ties in index
order).  Bound on every log-probability: |got - ref| <= 1e-5 + 2^-22 max(|x_id|, |lse|) -- the second term is two fp32 roundings (of lse and
of the difference), the first covers the fp32 sum and the hardware exp / log.  top_ids and rank are compared exactly.  All inputs are free
of -0 and NaN.

Shapes: V in {1, 5, 63, 64, 65, 1000, 4097, 16 384, 50 288} -- below, at and above a wave; more tokens than threads; the MMU vocabulary --
and 61 441, one more token than a 1024-thread workgroup keeps in registers (the emulator's 256 threads keep 15 360: there 16 384 and
50 288 take the form that re-reads the row, on the GPU 61 441 does)."""
import math

import pytest
import torch

VOCABS = [1, 5, 63, 64, 65, 1000, 4097, 16384, 50288, 61441]
TOP_NS = [0, 1, 5, 20, 64]
DTYPES = [torch.float32, torch.bfloat16, torch.float16]


def _tl(*a, **kw):
    from omnimamba_amd.sampling import token_logprobs
    return token_logprobs(*a, **kw)


def _logits(rows, V, dtype, scale, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(rows, V, generator=g) * scale).to(dtype) + 0.0          # (+ 0.0: no -0)


def _reference(x, ids, top_n):
    """x (rows, V) on the host, any dtype -> fp64 logprob (rows,), rank (rows,), top ids (rows, min(top_n, V)), their logprobs, lse."""
    x64 = x.double()
    lp = torch.log_softmax(x64, -1)
    order = torch.sort(x64, dim=-1, descending=True, stable=True).indices
    pos = torch.empty_like(order).scatter_(1, order, torch.arange(x.shape[1]).expand_as(order))
    k = min(top_n, x.shape[1])
    out = {"lse": torch.logsumexp(x64, -1), "top_ids": order[:, :k], "top_logprobs": lp.gather(1, order[:, :k]), "x": x64}
    if ids is not None:
        out["logprob"] = lp.gather(1, ids[:, None])[:, 0]
        out["rank"] = pos.gather(1, ids[:, None])[:, 0] + 1
        out["xid"] = x64.gather(1, ids[:, None])[:, 0]
    return out


def _close(got, ref, xval, lse, what):
    """The bound of the module docstring; a reference of -inf must be met exactly."""
    got, inf = got.double().cpu(), torch.isinf(ref)
    assert torch.equal(got[inf], ref[inf]), what
    lse = lse.reshape(-1, *([1] * (ref.dim() - 1))).expand_as(ref)
    bound = 1e-5 + 2.0 ** -22 * torch.maximum(xval.abs(), lse.abs())
    err = (got - ref).abs()
    fin = ~inf
    worst = (err[fin] / bound[fin]).max().item() if fin.any() else 0.0
    print(f"{what}: max error {err[fin].max().item() if fin.any() else 0.0:.3e}, {worst:.3f} of the bound")
    assert (err[fin] <= bound[fin]).all(), (what, err[fin].max().item())


def _check(x_host, ids_host, top_n, got, what=""):
    ref = _reference(x_host, ids_host, top_n)
    V = x_host.shape[1]
    k = min(top_n, V)
    if ids_host is not None:
        _close(got.logprob, ref["logprob"], ref["xid"], ref["lse"], what + " logprob")
        assert got.rank.dtype == torch.int32 and torch.equal(got.rank.cpu().long(), ref["rank"]), what + " rank"
    else:
        assert got.logprob is None and got.rank is None
    if top_n > 0:
        assert got.top_ids.shape == (x_host.shape[0], top_n) and got.top_ids.dtype == torch.int64
        assert torch.equal(got.top_ids.cpu()[:, :k], ref["top_ids"]), what + " top_ids"
        _close(got.top_logprobs[:, :k], ref["top_logprobs"], ref["x"].gather(1, ref["top_ids"]), ref["lse"], what + " top_logprobs")
        assert (got.top_ids.cpu()[:, k:] == -1).all() and (got.top_logprobs.cpu()[:, k:] == -math.inf).all(), what + " entries past the vocabulary"
    else:
        assert got.top_ids is None and got.top_logprobs is None


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16", "f16"])
@pytest.mark.parametrize("V", VOCABS)
def test_matches_the_fp64_reference(dev, V, dtype):
    """Every top_n at every vocabulary size and dtype; rows 1, 3 and 8 and the standard deviations 0.1, 2 and 12 (f16: 0.1, 2, 6) in turn.
    bf16 rows at V = 50 288 are dense in equal values: the index tie-break of top_ids and rank."""
    big = V >= 50288 and dev.type == "cpu"
    for j, top_n in enumerate(TOP_NS):
        rows = min((1, 3, 8)[(j + V) % 3], 2) if big else (1, 3, 8)[(j + V) % 3]
        scale = (0.1, 2.0, 6.0 if dtype == torch.float16 else 12.0)[(j + VOCABS.index(V)) % 3]
        x = _logits(rows, V, dtype, scale, seed=1000 * j + V)
        g = torch.Generator().manual_seed(j)
        ids = torch.randint(0, V, (rows,), generator=g)
        ids[0] = int(x[0].float().argmax()) if j % 2 else V - 1
        got = _tl(x.to(dev), ids.to(dev), top_n=top_n)
        _check(x, ids, top_n, got, f"V={V} rows={rows} top_n={top_n} scale={scale}")
    # top_n alone: no ids, nothing but the top_n fields
    x = _logits(2, V, dtype, 2.0, seed=V + 7)
    _check(x, None, 5, _tl(x.to(dev), top_n=5), f"V={V} top_n only")


def test_row_stride_and_strided_outputs(dev):
    from omnimamba_amd.sampling import TokenLogprobs
    V, rows, n = 1000, 3, 5
    g = torch.Generator().manual_seed(5)
    wide = (torch.randn(rows, V + 37, generator=g) * 2).to(dev)
    x = wide[:, :V]
    assert x.stride(0) == V + 37
    ids = torch.tensor([3, 999, 500])
    out = TokenLogprobs(logprob=torch.full((rows, 3), 7.0, device=dev)[:, 1], rank=torch.full((rows, 2), 7, dtype=torch.int32, device=dev)[:, 0],
                        top_ids=torch.full((2 * rows, 2 * n), 7, dtype=torch.int64, device=dev)[::2, 1::2],
                        top_logprobs=torch.full((n, rows), 7.0, device=dev).t())
    bases = [t._base.clone() for t in (out.logprob, out.rank, out.top_ids, out.top_logprobs)]
    got = _tl(x, ids.to(dev), top_n=n, out=out)
    assert got.logprob is out.logprob and got.rank is out.rank and got.top_ids is out.top_ids and got.top_logprobs is out.top_logprobs
    _check(x.cpu(), ids, n, got, "strided")
    # nothing outside the views was written
    for t, before in zip((out.logprob, out.rank, out.top_ids, out.top_logprobs), bases):
        after = t._base.clone()
        t.fill_(7)
        assert torch.equal(t._base, before)
        assert not torch.equal(after, before)


def test_ties_and_extremes(dev):
    V = 300
    # all equal: logprob -log V, top ids 0 .. N - 1, rank id + 1
    x = torch.full((3, V), 0.5)
    ids = torch.tensor([0, 7, V - 1])
    got = _tl(x.to(dev), ids.to(dev), top_n=20)
    _check(x, ids, 20, got, "all equal")
    assert torch.equal(got.top_ids.cpu(), torch.arange(20).expand(3, 20)) and torch.equal(got.rank.cpu().long(), ids + 1)
    assert (got.logprob.cpu() + math.log(V)).abs().max() <= 1e-5
    # one logit of 1e4 over zeros
    x = torch.zeros(2, V)
    x[0, 17] = 1e4
    x[1, V - 1] = 1e4
    ids = torch.tensor([17, 3])
    got = _tl(x.to(dev), ids.to(dev), top_n=5)
    _check(x, ids, 5, got, "1e4 over zeros")
    assert got.logprob.cpu().tolist() == [0.0, -1e4] and got.rank.cpu().tolist() == [1, 5]
    # -inf entries, a chosen id whose logit is -inf among them
    x = _logits(4, V, torch.float32, 2.0, seed=8)
    x[0, ::2] = -math.inf
    x[1, 5] = -math.inf
    x[2, :V - 3] = -math.inf                      # (fewer finite logits than top_n)
    x[3, 100:] = -math.inf
    ids = torch.tensor([4, 5, V - 1, 250])
    got = _tl(x.to(dev), ids.to(dev), top_n=20)
    _check(x, ids, 20, got, "-inf entries")
    assert got.logprob.cpu()[:2].tolist() == [-math.inf, -math.inf] and got.logprob[3].item() == -math.inf


def test_ids_are_not_trusted(dev):
    V = 1000
    x = _logits(6, V, torch.float32, 2.0, seed=9)
    ids = torch.tensor([5, -1, V, 2 ** 62, 999, -2 ** 63])
    got = _tl(x.to(dev), ids.to(dev), top_n=5)
    bad = torch.tensor([False, True, True, True, False, True])
    assert torch.isnan(got.logprob.cpu()[bad]).all() and (got.rank.cpu()[bad] == 0).all()
    good = torch.tensor([0, 4])
    alone = _tl(x[good].to(dev), ids[good].to(dev), top_n=5)
    _check(x[good], ids[good], 5, alone, "valid rows alone")
    assert torch.equal(got.logprob[good.to(dev)].view(torch.int32), alone.logprob.view(torch.int32)) and torch.equal(got.rank[good.to(dev)], alone.rank)
    # the top_n of a row does not depend on its id
    clean = _tl(x.to(dev), torch.zeros(6, dtype=torch.int64, device=dev), top_n=5)
    assert torch.equal(got.top_ids, clean.top_ids) and torch.equal(got.top_logprobs.view(torch.int32), clean.top_logprobs.view(torch.int32))


def test_inactive_rows_write_nothing(dev):
    from omnimamba_amd.sampling import TokenLogprobs
    V, n = 1000, 5
    x = _logits(8, V, torch.float32, 2.0, seed=10)
    ids = torch.randint(0, V, (8,), generator=torch.Generator().manual_seed(1))
    want = _tl(x.to(dev), ids.to(dev), top_n=n)
    active = torch.tensor([1, 0, 1, 1, 0, 0, 1, 0], dtype=torch.int32)
    off = active == 0
    x2, ids2 = x.clone(), ids.clone()
    x2[off] = math.nan                                   # what a retired row leaves behind may be anything
    ids2[off] = torch.tensor([-5, 2 ** 40, V, 0])
    out = TokenLogprobs(logprob=torch.full((8,), -7.0, device=dev), rank=torch.full((8,), -7, dtype=torch.int32, device=dev),
                        top_ids=torch.full((8, n), -7, dtype=torch.int64, device=dev), top_logprobs=torch.full((8, n), -7.0, device=dev))
    got = _tl(x2.to(dev), ids2.to(dev), top_n=n, active=active.to(dev), out=out)
    for name in ("logprob", "rank", "top_ids", "top_logprobs"):
        g, w = getattr(got, name).cpu(), getattr(want, name).cpu()
        assert (g[off] == -7).all(), name
        assert torch.equal(g[~off], w[~off]), name


def test_rows_are_independent_of_their_place(dev):
    V, n = 4097, 20
    x = _logits(8, V, torch.bfloat16, 2.0, seed=11)
    ids = torch.randint(0, V, (8,), generator=torch.Generator().manual_seed(2))
    got = _tl(x.to(dev), ids.to(dev), top_n=n)
    bits = lambda r: [r.logprob.view(torch.int32).cpu(), r.rank.cpu(), r.top_ids.cpu(), r.top_logprobs.view(torch.int32).cpu()]
    perm = torch.tensor([5, 2, 7, 0, 3, 6, 1, 4])
    pg = _tl(x[perm].contiguous().to(dev), ids[perm].to(dev), top_n=n)
    for a, b in zip(bits(pg), bits(got)):
        assert torch.equal(a, b[perm])
    for b in (0, 3, 7):
        one = _tl(x[b:b + 1].to(dev), ids[b:b + 1].to(dev), top_n=n)
        for a, w in zip(bits(one), bits(got)):
            assert torch.equal(a[0], w[b])


def test_arguments_are_validated(dev):
    x = _logits(2, 100, torch.float32, 1.0, seed=12).to(dev)
    ids = torch.zeros(2, dtype=torch.int64, device=dev)
    for bad in (dict(top_n=65), dict(top_n=-1)):
        with pytest.raises(ValueError):
            _tl(x, ids, **bad)
    with pytest.raises(ValueError):
        _tl(x)                                            # neither ids nor top_n
    with pytest.raises(ValueError):
        _tl(x, ids.int())
    with pytest.raises(ValueError):
        _tl(x, ids[:1])
    with pytest.raises(ValueError):
        _tl(x.t().contiguous().t(), ids)                  # no unit last stride
    assert _tl(x[:0], ids[:0], top_n=3).top_ids.shape == (0, 3)
    # the library's own checks (what a caller of the C entry meets)
    from omnimamba_amd import _capi as K
    from omnimamba_amd._lib import get_lib
    p = K.TokenLogprobs(logits=K.T(x), top_n=0)
    assert get_lib().omk_token_logprobs(__import__("ctypes").byref(p), None) == -1
    p = K.TokenLogprobs(logits=K.T(x), top_n=3)
    assert get_lib().omk_token_logprobs(__import__("ctypes").byref(p), None) == -1


@pytest.mark.gpu
@torch.inference_mode()
def test_capture_and_replay_with_rewritten_inputs():
    """The launch inside a captured graph with static buffers (the capture pattern of test_sampling_rows): logits and ids are rewritten
    between two replays, and both replays equal the eager calls bit for bit."""
    from omnimamba_amd.sampling import TokenLogprobs
    dev = torch.device("cuda:0")
    V, n = 50288, 5
    x1, x2 = _logits(8, V, torch.float32, 2.0, seed=13).to(dev), _logits(8, V, torch.float32, 3.0, seed=14).to(dev)
    i1 = torch.randint(0, V, (8,), generator=torch.Generator().manual_seed(3)).to(dev)
    i2 = torch.randint(0, V, (8,), generator=torch.Generator().manual_seed(4)).to(dev)
    x, ids = x1.clone(), i1.clone()
    out = TokenLogprobs(logprob=torch.zeros(8, device=dev), rank=torch.zeros(8, dtype=torch.int32, device=dev),
                        top_ids=torch.zeros(8, n, dtype=torch.int64, device=dev), top_logprobs=torch.zeros(8, n, device=dev))
    run = lambda: _tl(x, ids, top_n=n, out=out)
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
    snap = lambda r: [r.logprob.view(torch.int32).clone(), r.rank.clone(), r.top_ids.clone(), r.top_logprobs.view(torch.int32).clone()]
    for t in (out.logprob, out.top_logprobs):
        t.fill_(-1.0)
    graph.replay()
    got1 = snap(out)
    x.copy_(x2)
    ids.copy_(i2)
    graph.replay()
    got2 = snap(out)
    torch.cuda.synchronize()
    e1, e2 = snap(_tl(x1, i1, top_n=n)), snap(_tl(x2, i2, top_n=n))
    for a, b in zip(got1, e1):
        assert torch.equal(a, b)
    for a, b in zip(got2, e2):
        assert torch.equal(a, b)
    assert not torch.equal(got1[0], got2[0])
