"""Presence and frequency penalties as device-built logit edits (omk_penalty_edits, ABI 17; sampling.penalty_edits and
sampling.sample_rows(frequency=, presence=, count_start=)).

Two oracles, neither with a tolerance:
  * the kernel's output against `penalty_edit_list` below, the output definition of include/omk.h restated in plain Python with
    numpy.float32 arithmetic (every operation rounds on its own: the product and the sum of a delta are two roundings): ids, the BITS of the
    values, lengths and modes are equal, and nothing behind a row's length (or in an inactive row) is written;
  * the fused path (penalty_edits + the edit launch of omk_sample_rows) against the plain launch on the copy that
    sampling.apply_logit_edits(..., frequency=, presence=, count_start=) edits with torch: the same ids, bit for bit, in every branch of the
    sampler, fp32 and bf16, with and without a repetition penalty and user edits."""
import math
from collections import Counter

import numpy as np
import pytest
import torch

V = 1501
NINF = float("-inf")
SENT_ID, SENT_VAL, SENT_LEN, SENT_MODE = -77, 123.5, -5, -9
f32 = np.float32


def penalty_edit_list(hist, hist_len, count_start, freq, pres, vocab, user=None, out_cap=1 << 30):
    """(ids, values as numpy.float32, length, mode) of one row.  hist: the row of the history buffer, all history_cap entries;
    user: None or (ids, values, edit_len, edit_mode), the row of the user arrays, all edit_cap entries."""
    cap = len(hist)
    L = min(max(int(hist_len), 0), cap)
    s = min(max(int(count_start), 0), L)
    fr = f32(freq) if math.isfinite(freq) else f32(0.0)
    pr = f32(pres) if math.isfinite(pres) else f32(0.0)
    counted = [t for t in hist[s:L] if 0 <= t < vocab] if (fr != 0 or pr != 0) else []
    cnt = Counter(counted)

    def delta(c):
        prod = f32(fr * f32(c))
        return f32(-f32(prod + pr))

    uids, uvals, ulen, umode = user if user is not None else ([], [], 0, 0)
    n_user = min(max(int(ulen), 0), len(uids))
    ids, vals, valid = [], [], set()
    with np.errstate(all="ignore"):
        for j in range(n_user):
            i, v = int(uids[j]), f32(uvals[j])
            ok = 0 <= i < vocab
            if ok:
                valid.add(i)
            ids.append(i)
            vals.append(f32(v + delta(cnt[i])) if ok and cnt.get(i, 0) > 0 else v)
        allow = umode == 1 and bool(valid)
        if not allow:
            for t in dict.fromkeys(counted):
                if t not in valid:
                    ids.append(t)
                    vals.append(delta(cnt[t]))
    n = min(len(ids), int(out_cap))
    return ids[:n], vals[:n], n, int(allow)


def _bits(vals):
    return np.asarray(vals, dtype=np.float32).view(np.int32).tolist()


def _run_rows(dev, rows, *, vocab=V, out_cap=None, hist_pad=0, active=None):
    """rows: dicts with hist (list), len, start, freq, pres and optionally user = (ids, vals, len, mode).  Runs the kernel over all of them
    in one launch with sentinel-filled outputs and compares every row with penalty_edit_list."""
    from omnimamba_amd.sampling import penalty_edits
    n = len(rows)
    hcap = max(1, max(len(r["hist"]) for r in rows))
    ecap = max([len(r["user"][0]) for r in rows if r.get("user")] + [0])
    full = torch.full((n, hcap + hist_pad), 7, dtype=torch.int64)          # (what lies behind a row's width is never read: token 7 is valid)
    for b, r in enumerate(rows):
        full[b, :len(r["hist"])] = torch.tensor(r["hist"], dtype=torch.int64)
        r["hist_row"] = full[b, :hcap].tolist()
    hist = full.to(dev)[:, :hcap]                                          # a view whose row stride exceeds its width when hist_pad > 0
    kw = {}
    if ecap:
        ids = torch.full((n, ecap), 3, dtype=torch.int64)
        vals = torch.full((n, ecap), 50.0, dtype=torch.float32)
        lens = torch.zeros(n, dtype=torch.int32)
        mode = torch.zeros(n, dtype=torch.int32)
        for b, r in enumerate(rows):
            if r.get("user"):
                ui, uv, ul, um = r["user"]
                ids[b, :len(ui)] = torch.tensor(ui, dtype=torch.int64)
                vals[b, :len(uv)] = torch.tensor(uv, dtype=torch.float32)
                lens[b], mode[b] = ul, um
            r["user_row"] = (ids[b].tolist(), vals[b].tolist(), int(lens[b]), int(mode[b]))
        kw = dict(edit_ids=ids.to(dev), edit_vals=vals.to(dev), edit_lens=lens.to(dev), edit_mode=mode.to(dev))
    ocap = out_cap if out_cap is not None else max(1, ecap + hcap)
    out = {"edit_ids": torch.full((n, ocap), SENT_ID, dtype=torch.int64, device=dev), "edit_vals": torch.full((n, ocap), SENT_VAL, dtype=torch.float32, device=dev),
           "edit_lens": torch.full((n,), SENT_LEN, dtype=torch.int32, device=dev), "edit_mode": torch.full((n,), SENT_MODE, dtype=torch.int32, device=dev)}
    i32 = lambda k: torch.tensor([r[k] for r in rows], dtype=torch.int32).to(dev)
    f = lambda k: torch.tensor([r[k] for r in rows], dtype=torch.float32).to(dev)
    act = None if active is None else torch.tensor(active, dtype=torch.int32).to(dev)
    got = penalty_edits(hist, i32("len"), i32("start"), f("freq"), f("pres"), vocab, active=act, out=out, **kw)
    assert got is out
    oi, ov = out["edit_ids"].cpu(), out["edit_vals"].cpu()
    ol, om = out["edit_lens"].cpu().tolist(), out["edit_mode"].cpu().tolist()
    res = []
    for b, r in enumerate(rows):
        if active is not None and not active[b]:
            assert ol[b] == SENT_LEN and om[b] == SENT_MODE and (oi[b] == SENT_ID).all() and (ov[b] == SENT_VAL).all(), ("inactive row written", b)
            res.append(None)
            continue
        wi, wv, wl, wm = penalty_edit_list(r["hist_row"], r["len"], r["start"], r["freq"], r["pres"], vocab, r.get("user_row"), ocap)
        assert ol[b] == wl and om[b] == wm, (b, ol[b], wl, om[b], wm)
        assert oi[b, :wl].tolist() == wi, (b, oi[b, :wl].tolist(), wi)
        assert _bits(ov[b, :wl].numpy()) == _bits(wv), (b, ov[b, :wl].tolist(), [float(x) for x in wv])
        assert (oi[b, wl:] == SENT_ID).all() and (ov[b, wl:] == SENT_VAL).all(), ("written behind the row's length", b)
        res.append((wi, wv, wl, wm))
    return res


def _row(hist, start, freq, pres, user=None, hlen=None):
    return {"hist": list(hist), "len": len(hist) if hlen is None else hlen, "start": start, "freq": freq, "pres": pres, "user": user}


def _counted(n, seed):
    """n counted ids with repeats, in no particular id order."""
    g = torch.Generator().manual_seed(seed)
    pool = torch.randperm(V, generator=g)[:max(1, n // 3)]
    return pool[torch.randint(0, len(pool), (n,), generator=g)].tolist()


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257])
def test_counted_lengths_around_the_wave_and_the_workgroup_edge(dev, n):
    """A prompt of three ids in front of the counted range (two of them tokens of the range: they do not count).  Row 0 without a user list,
    row 1 with one that names two counted tokens (one twice), an uncounted one, an invalid id and a banned counted token."""
    c = _counted(n, n)
    prompt = [c[0] if c else 5, 9, c[-1] if c else 6]
    a, b = (c[0], c[n // 2]) if c else (11, 12)
    user = ([a, 1400, a, -1, b], [0.25, -1.5, 9.0, 2.0, NINF], 5, 0)
    res = _run_rows(dev, [_row(prompt + c, 3, 0.3, 0.7), _row(prompt + c, 3, 1.1, -0.2, user)])
    assert res[0][2] == len(set(c)) and res[1][2] == 5 + len(set(c) - {a, b})
    if n > 1:
        assert res[0][0] == list(dict.fromkeys(c)) and res[0][0] != sorted(res[0][0]), "first-occurrence order is id order here: the case does not test it"


def test_512_distinct_ids_and_a_range_longer_than_a_tile(dev):
    """512 distinct ids fill the list of the sampler (one tile); 1030 entries of five distinct ids loop over three tiles, own by compared."""
    g = torch.Generator().manual_seed(1)
    distinct = torch.randperm(V, generator=g)[:512].tolist()
    five = [distinct[i] for i in torch.randint(0, 5, (1030,), generator=g).tolist()]
    res = _run_rows(dev, [_row([2, 3] + distinct, 2, 0.5, 0.25)])
    assert res[0][2] == 512 and res[0][0] == distinct
    user = ([five[0], 8], [1.0, 2.0], 2, 0)
    res = _run_rows(dev, [_row(five, 0, 0.01, 0.5), _row(five, 0, 0.01, 0.5, user), _row(distinct + five, 100, 0.125, 0.0)])
    assert res[0][2] == 5 and res[1][2] == 2 + 4 and res[2][2] == 412 + len(set(five) - set(distinct[100:]))
    cnt = Counter(five)
    assert [float(v) for v in res[0][1]] == [float(f32(-f32(f32(f32(0.01) * f32(cnt[t])) + f32(0.5)))) for t in res[0][0]]


def test_contents_the_kernel_defines(dev):
    """Batch 5 and batch 1; all ids equal; ids -1, vocab and 2^40 in the range; count_start negative, equal to the length and beyond it;
    history_lens beyond history_cap and negative; a frequency of NaN (counts as 0) and a negative presence; both penalties off; a history
    view whose row stride exceeds its width."""
    G = 2 ** 40
    mixed = [4, -1, V, 4, G, 9, -G, 4, V - 1, 0, 9]
    rows = [_row([6] * 40, 0, 0.5, 0.5),
            _row(mixed, 0, 0.25, 1.0),
            _row(mixed, -3, float("nan"), -0.75),
            _row(mixed, len(mixed), 1.0, 1.0),
            _row(mixed, len(mixed) + 5, 1.0, 1.0)]
    res = _run_rows(dev, rows, hist_pad=5)
    assert res[0][:3:2] == ([6], 1) and float(res[0][1][0]) == -20.5
    assert res[1][0] == [4, 9, V - 1, 0] and [float(v) for v in res[1][1]] == [-1.75, -1.5, -1.25, -1.25]
    assert res[2][0] == [4, 9, V - 1, 0] and [float(v) for v in res[2][1]] == [0.75] * 4
    assert res[3][2] == 0 and res[4][2] == 0
    # two roundings: float32(1.1) x 6 is a tie that rounds up to 6.6000004, and 6.6000004 - 0.2 rounds to 0x40CCCCCE; one rounding of the
    # exact 6.60000014... - 0.2 (a fused multiply-add) gives 0x40CCCCCD
    res = _run_rows(dev, [_row([5] * 6, 0, 1.1, -0.2)])
    assert _bits(res[0][1]) == [0xC0CCCCCE - (1 << 32)]
    res = _run_rows(dev, [_row(mixed, 2, 0.5, 0.0, hlen=1000)])
    assert res[0][0] == [4, 9, V - 1, 0]
    res = _run_rows(dev, [_row(mixed, 0, 0.5, 0.0, hlen=-4), _row(mixed, 0, 0.0, 0.0, ([4, 9], [1.0, NINF], 2, 0)),
                          _row(mixed, 0, float("inf"), float("-inf"), ([4], [1.0], 1, 1))])
    assert res[0][2] == 0 and res[1][:2] == ([4, 9], [f32(1.0), f32(NINF)]) and res[2][:2] == ([4], [f32(1.0)]) and res[2][3] == 1


def test_user_lists(dev):
    """Empty lists; a repeated id (both entries move); an invalid id (kept, not moved); -inf stays -inf; an allow-only row (no entry is
    appended: the allowed set wins); an allow-only row without a valid id (unconstrained: it gets the penalties, mode 0); edit_lens below
    0 and above the cap; a mode other than 1; entries behind a row's length are not read."""
    h = [10, 11, 10, 12, 10, 13, 11]
    rows = [_row(h, 0, 0.5, 0.25, ([], [], 0, 0)),
            _row(h, 0, 0.5, 0.25, ([10, 10, 99, 11], [1.0, -2.0, 4.0, NINF], 4, 0)),
            _row(h, 0, 0.5, 0.25, ([-1, V, 2 ** 40, 12], [1.0, 2.0, 3.0, 0.0], 4, 0)),
            _row(h, 0, 0.5, 0.25, ([10, 500], [0.0, 0.5], 2, 1)),
            _row(h, 0, 0.5, 0.25, ([-1, V], [0.0, 0.0], 2, 1)),
            _row(h, 0, 0.5, 0.25, ([10, 11, 12, 13], [1.0] * 4, -2, 0)),
            _row(h, 0, 0.5, 0.25, ([10, 11, 12, 13], [1.0] * 4, 1000, 7)),
            _row(h, 0, 0.5, 0.25, ([13, 10, 11, 12], [1.0] * 4, 1, 0))]
    res = _run_rows(dev, rows)
    assert res[0][0] == [10, 11, 12, 13] and [float(v) for v in res[0][1]] == [-1.75, -1.25, -0.75, -0.75]
    assert res[1][0] == [10, 10, 99, 11, 12, 13] and [float(v) for v in res[1][1]] == [-0.75, -3.75, 4.0, NINF, -0.75, -0.75]
    assert res[2][0] == [-1, V, 2 ** 40, 12, 10, 11, 13] and [float(v) for v in res[2][1][:4]] == [1.0, 2.0, 3.0, -0.75]
    assert res[3][0] == [10, 500] and res[3][3] == 1 and [float(v) for v in res[3][1]] == [-1.75, 0.5]
    assert res[4][0] == [-1, V, 10, 11, 12, 13] and res[4][3] == 0
    assert res[5][0] == [10, 11, 12, 13] and res[5][2] == 4 and float(res[5][1][0]) == -1.75
    assert res[6][0] == [10, 11, 12, 13] and res[6][3] == 0 and [float(v) for v in res[6][1]] == [-0.75, -0.25, 0.25, 0.25]
    assert res[7][0] == [13, 10, 11, 12]


def test_a_user_list_longer_than_a_tile(dev):
    """600 user entries are two tiles of the user list: against a counted range of one tile (the user tiles are restaged while the range
    stays), and against one of 1030 entries (three tiles by two).  The list names counted and uncounted tokens, some twice, and an invalid
    id in each tile; the second row is allow-only."""
    g = torch.Generator().manual_seed(2)
    toks = torch.randperm(V, generator=g).tolist()
    short = [toks[i] for i in torch.randint(0, 300, (400,), generator=g).tolist()]
    long = [toks[i] for i in torch.randint(0, 700, (1030,), generator=g).tolist()]
    uids = toks[200:780] + toks[200:218] + [-1, V]
    uids[5], uids[530] = 2 ** 40, -7
    uvals = [0.01 * j - 3.0 for j in range(600)]
    for h in (short, long):
        res = _run_rows(dev, [_row(h, 0, 0.3, 0.2, (uids, uvals, 600, 0)), _row(h, 0, 0.3, 0.2, (uids, uvals, 600, 1)), _row(h, 0, 0.3, 0.2)])
        named = {t for t in uids if 0 <= t < V}
        assert res[0][2] == 600 + len(set(h) - named) > 700 and res[1][2] == 600 and res[1][3] == 1
        assert sum(1 for a, b in zip(res[0][1][:600], uvals) if float(a) != float(f32(b))) > 50, "few user values moved: the case does not test them"


def test_row_strides_below_the_width_are_refused(dev):
    from omnimamba_amd import _capi as K
    from omnimamba_amd._lib import get_lib
    hist = torch.zeros(2, 8, dtype=torch.int64, device=dev)
    i32, f = torch.zeros(2, dtype=torch.int32, device=dev), torch.zeros(2, dtype=torch.float32, device=dev)
    oi, ov = torch.zeros(2, 8, dtype=torch.int64, device=dev), torch.zeros(2, 8, device=dev)
    ol, om = i32.clone(), i32.clone()
    base = dict(history=hist.data_ptr(), history_lens=i32.data_ptr(), count_start=i32.data_ptr(), frequency=f.data_ptr(), presence=f.data_ptr(),
                history_stride=8, history_cap=8, out_ids=oi.data_ptr(), out_vals=ov.data_ptr(), out_lens=ol.data_ptr(), out_mode=om.data_ptr(),
                out_stride=8, out_cap=8, batch=2, vocab=V)
    K.run(get_lib(), "omk_penalty_edits", K.PenaltyEdits(**base), hist)
    for bad in (dict(history_stride=4), dict(history_stride=-8), dict(out_stride=7), dict(out_stride=0),
                dict(edit_ids=oi.data_ptr(), edit_vals=ov.data_ptr(), edit_lens=i32.data_ptr(), edit_cap=4, edit_stride=2)):
        with pytest.raises(RuntimeError, match="omk_status -1"):
            K.run(get_lib(), "omk_penalty_edits", K.PenaltyEdits(**{**base, **bad}), hist)


def test_truncation_and_inactive_rows(dev):
    """out_cap smaller than the result: the list is cut, the tail stays as it was (checked for every row in _run_rows), also inside the
    user entries.  Inactive rows next to active ones write nothing."""
    h = list(range(20, 60))
    user = ([25, 7, 8], [1.0, 2.0, 3.0], 3, 0)
    res = _run_rows(dev, [_row(h, 0, 0.5, 0.5), _row(h, 0, 0.5, 0.5, user)], out_cap=10)
    assert res[0][2] == 10 and res[0][0] == h[:10] and res[1][2] == 10 and res[1][0] == [25, 7, 8] + [t for t in h if t != 25][:7]
    res = _run_rows(dev, [_row(h, 0, 0.5, 0.5, user)], out_cap=2)
    assert res[0][0] == [25, 7]
    rows = [_row(h, 0, 0.5, 0.5, user), _row([2 ** 40] * 40, 0, float("nan"), 1.0, ([2 ** 40] * 3, [float("nan")] * 3, 10 ** 6, 99)),
            _row(h[::-1], 3, 0.5, 0.5), _row(h, 0, 1.0, 1.0), _row(h, 5, -0.5, 0.25, user)]
    res = _run_rows(dev, rows, active=[1, 0, 1, 0, 1])
    assert res[1] is None and res[3] is None and res[2][0] == h[::-1][3:]


def test_the_library_refuses_a_call_without_its_required_arrays(dev):
    from omnimamba_amd import _capi as K
    from omnimamba_amd._lib import get_lib
    from omnimamba_amd.sampling import penalty_edits
    assert get_lib().omk_abi_version() == 17 and K.OMK_ABI_VERSION == 17
    hist = torch.zeros(2, 8, dtype=torch.int64, device=dev)
    i32, f = torch.zeros(2, dtype=torch.int32, device=dev), torch.zeros(2, dtype=torch.float32, device=dev)
    for bad in ((hist, None, i32, f, f), (hist, i32, None, f, f), (hist, i32, i32, None, f), (hist, i32, i32, f, None)):
        with pytest.raises(RuntimeError, match="omk_status -1"):
            penalty_edits(*bad, V)
    ids = torch.zeros(2, 3, dtype=torch.int64, device=dev)
    with pytest.raises(RuntimeError, match="omk_status -1"):
        penalty_edits(hist, i32, i32, f, f, V, edit_ids=ids, edit_vals=ids.float(), edit_lens=None)
    with pytest.raises(RuntimeError, match="omk_status -1"):
        penalty_edits(hist, i32, i32, f, f, 0)
    p = K.PenaltyEdits(batch=1, vocab=V)                                              # (every pointer NULL)
    with pytest.raises(RuntimeError, match="omk_status -1"):
        K.run(get_lib(), "omk_penalty_edits", p, hist)
    empty = penalty_edits(hist[:0], i32[:0], i32[:0], f[:0], f[:0], V, out_cap=4)     # no row: OMK_OK, nothing launched
    assert empty["edit_ids"].shape == (0, 4)


def test_sampling_params_take_finite_penalties_only():
    from omnimamba_amd.sampling import SamplingParams as SP, has_count_penalties, pack_count_penalties, pack_rows
    assert (SP().presence_penalty, SP().frequency_penalty) == (0.0, 0.0) and not has_count_penalties(SP())
    assert has_count_penalties(SP(presence_penalty=0.5)) and has_count_penalties(SP(frequency_penalty=-0.25))
    for bad in (dict(presence_penalty=math.nan), dict(presence_penalty=math.inf), dict(frequency_penalty=-math.inf), dict(frequency_penalty=math.nan)):
        with pytest.raises(ValueError):
            SP(**bad)
    ps = [SP(presence_penalty=0.5, frequency_penalty=0.25), SP(), SP(frequency_penalty=-1.0)]
    pk = pack_count_penalties(ps, torch.device("cpu"))
    assert set(pk) == {"frequency", "presence"} and pk["frequency"].tolist() == [0.25, 0.0, -1.0] and pk["presence"].tolist() == [0.5, 0.0, 0.0]
    assert pk["frequency"].dtype == torch.float32 and pk["frequency"].is_contiguous() and pk["presence"].is_contiguous()
    assert set(pack_rows(ps, torch.device("cpu"))) == {"top_k", "top_p", "temperature", "min_p", "penalty", "seeds", "steps"}


# ---- the fused path against the statement ---------------------------------------------------------------------------------------------

# (top_k, top_p, temperature, min_p): arg max | top-k 20 behind top-p | whole vocabulary plain | behind top-p | behind min_p
SETTINGS = [(1, 0.0, 1.0, 0.0), (20, 0.9, 0.8, 0.0), (0, 0.0, 1.0, 0.0), (0, 0.9, 1.0, 0.0), (0, 0.0, 1.0, 0.05)]
PROMPT, HCAP = 6, 40


def _case(vocab, dtype, n, seed, rep, edits):
    """n rows of logits; a history per row of PROMPT prompt ids (the row's best tokens among them: they must not count) and 7 .. 7 + n sampled
    ids drawn from the row's 12 best tokens with repeats, so the penalties move what is drawn; frequency / presence vary over the rows, one
    row with both negative; user edits (optional): biases on counted and uncounted tokens, a ban, and an allow-only row."""
    from omnimamba_amd.sampling import SamplingParams
    g = torch.Generator().manual_seed(seed)
    logits = (torch.randn(n, vocab, generator=g) * 2.0).to(dtype)
    hist = torch.zeros(n, HCAP, dtype=torch.int64)
    lens = torch.zeros(n, dtype=torch.int32)
    for b in range(n):
        top = torch.topk(logits[b].float(), 12).indices
        samp = top[torch.randint(0, 12, (7 + b,), generator=g)]
        row = torch.cat([top[:3], torch.randint(0, vocab, (PROMPT - 3,), generator=g), samp])
        hist[b, :len(row)] = row
        hist[b, len(row):] = top[0]                       # (behind the row's length: must not be read)
        lens[b] = len(row)
    start = torch.full((n,), PROMPT, dtype=torch.int32)
    freq = torch.tensor([[0.8, 0.0, 1.5, 0.3, -0.4, 2.0, 0.0, 0.6][b % 8] for b in range(n)], dtype=torch.float32)
    pres = torch.tensor([[0.5, 1.2, 0.0, 0.9, -0.6, 3.0, 0.0, 0.1][b % 8] for b in range(n)], dtype=torch.float32)
    seeds = [1000 + 37 * b for b in range(n)]
    params = [SamplingParams(top_k=k, top_p=tp, temperature=t, min_p=mp, seed=seeds[b], step0=3 + 11 * b, repetition_penalty=1.3 if rep else 1.0)
              for b, (k, tp, t, mp) in enumerate(SETTINGS[b % len(SETTINGS)] for b in range(n))]
    ed = {}
    if edits:
        E = 6
        ids = torch.zeros(n, E, dtype=torch.int64)
        vals = torch.zeros(n, E, dtype=torch.float32)
        el = torch.zeros(n, dtype=torch.int32)
        mode = torch.zeros(n, dtype=torch.int32)
        for b in range(n):
            top = torch.topk(logits[b].float(), 14).indices.tolist()
            if b % 3 == 0:      # biases on a counted token (twice: the first entry wins), an uncounted one; a ban
                l = [(int(hist[b, PROMPT]), 1.5), (int(hist[b, PROMPT]), -9.0), (top[13], 3.0), (top[0], NINF)]
            elif b % 3 == 1:    # allow-only: some of the best tokens, counted or not
                l = [(t, 0.25 * j) for j, t in enumerate(top[1:6])]
                mode[b] = 1
            else:
                l = []
            for j, (t, v) in enumerate(l):
                ids[b, j], vals[b, j] = t, v
            el[b] = len(l)
        ed = {"edit_ids": ids, "edit_vals": vals, "edit_lens": el, "edit_mode": mode}
    return logits, params, hist, lens, start, freq, pres, ed


def _statement(logits, pk, hist, lens, start, freq, pres, ed, **kw):
    """The plain launch on the copy apply_logit_edits makes."""
    from omnimamba_amd.sampling import apply_logit_edits, sample_rows, sample_rows_form
    pk = dict(pk)
    pen = pk.pop("penalty", None)
    work = apply_logit_edits(logits, **ed, penalty=pen, history=hist, history_lens=lens, frequency=freq, presence=pres, count_start=start)
    assert sample_rows_form(work, **pk) == 0
    return sample_rows(work, **pk, **kw)


@pytest.mark.parametrize("edits", [False, True])
@pytest.mark.parametrize("rep", [False, True])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_the_fused_path_equals_the_plain_launch_on_the_stated_copy(dev, dtype, rep, edits, monkeypatch):
    import omnimamba_amd.sampling as S
    from omnimamba_amd import _capi as K
    n = 10                                   # every branch twice
    logits, params, hist, lens, start, freq, pres, ed = (_to(x, dev) for x in _case(V, dtype, n, 3, rep, edits))
    pk = S.pack_rows(params, dev)
    if not rep:
        pk.pop("penalty")
    calls, pe0 = [], S.penalty_edits
    monkeypatch.setattr(S, "penalty_edits", lambda *a, **k: calls.append(1) or pe0(*a, **k))
    before = logits.clone()
    got = S.sample_rows(logits, **pk, **ed, history=hist, history_lens=lens, frequency=freq, presence=pres, count_start=start, count_max=HCAP - PROMPT).cpu()
    assert calls == [1], "the fused path was not taken"
    assert torch.equal(logits.view(torch.uint8), before.view(torch.uint8))
    want = _statement(logits, pk, hist, lens, start, freq, pres, ed).cpu()
    assert torch.equal(got, want), (dtype, rep, edits, got.tolist(), want.tolist())
    # the second launch is the edit instantiation
    merged = pe0(hist, lens, start, freq, pres, V, **ed)
    assert S.sample_rows_form(logits, **pk, **merged, history=hist, history_lens=lens) == K.SAMPLE_ROWS_EDIT
    # caller-owned merged buffers, and only one of the two penalties
    bufs = {k: torch.zeros_like(v) for k, v in pe0(hist, lens, start, freq, pres, V, **ed, out_cap=64).items()}
    again = S.sample_rows(logits, **pk, **ed, history=hist, history_lens=lens, frequency=freq, presence=pres, count_start=start, count_max=HCAP - PROMPT, merged=bufs).cpu()
    assert torch.equal(again, got) and int(bufs["edit_lens"].max()) > 6
    only = S.sample_rows(logits, **pk, **ed, history=hist, history_lens=lens, presence=pres, count_start=start, count_max=HCAP - PROMPT).cpu()
    assert torch.equal(only, _statement(logits, pk, hist, lens, start, None, pres, ed).cpu())
    # the case tests something: the penalties change what is drawn, and so does where the counted range starts
    off = S.sample_rows(logits, **pk, **ed, history=hist, history_lens=lens).cpu()
    assert int((got != off).sum()) >= 3, (got.tolist(), off.tolist())
    whole = S.sample_rows(logits, **pk, **ed, history=hist, history_lens=lens, frequency=freq, presence=pres).cpu()
    assert torch.equal(whole, _statement(logits, pk, hist, lens, None, freq, pres, ed).cpu())


def _to(x, dev):
    if isinstance(x, dict):
        return {k: v.to(dev) for k, v in x.items()}
    return x.to(dev) if isinstance(x, torch.Tensor) else x


def test_a_vocabulary_or_a_range_too_large_for_the_edit_launch_edits_a_copy(dev, monkeypatch):
    """count_max + the user width above MAX_EDITS (the default count_max is the width of the history), or 65 537 tokens: no penalty_edits
    launch, the ids of the statement -- and of the fused path where it can run.  Both arrays None: the call as it was."""
    import omnimamba_amd.sampling as S
    calls, pe0 = [], S.penalty_edits
    monkeypatch.setattr(S, "penalty_edits", lambda *a, **k: calls.append(1) or pe0(*a, **k))
    logits, params, hist, lens, start, freq, pres, ed = (_to(x, dev) for x in _case(V, torch.float32, 5, 4, True, True))
    wide = torch.cat([hist, torch.zeros(5, S.MAX_EDITS, dtype=torch.int64, device=dev)], 1)
    pk = S.pack_rows(params, dev)
    kw = dict(history_lens=lens, frequency=freq, presence=pres, count_start=start)
    got = S.sample_rows(logits, **pk, **ed, history=wide, **kw).cpu()
    assert calls == []
    assert torch.equal(got, _statement(logits, pk, wide, lens, start, freq, pres, ed).cpu())
    assert torch.equal(got, S.sample_rows(logits, **pk, **ed, history=wide, **kw, count_max=S.MAX_EDITS - 6).cpu()) and calls == [1]
    del calls[:]
    assert torch.equal(S.sample_rows(logits, **pk, **ed, history=wide, **kw, count_max=S.MAX_EDITS - 5).cpu(), got) and calls == []
    assert torch.equal(S.sample_rows(logits, **pk, **ed, history=hist, history_lens=lens, frequency=None, presence=None),
                       S.sample_rows(logits, **pk, **ed, history=hist, history_lens=lens))
    with pytest.raises(ValueError):
        S.sample_rows(logits, **pk, frequency=freq)
    big = 65537
    logits, params, hist, lens, start, freq, pres, ed = (_to(x, dev) for x in _case(big, torch.float32, 2, 5, False, False))
    pk = S.pack_rows(params, dev)
    pk.pop("penalty")
    hist[0, PROMPT] = logits[0].argmax()             # the greedy row has sampled its arg max before; -(5 x 0.8 c + 0.5) moves it away
    freq = freq * 5.0
    got = S.sample_rows(logits, **pk, history=hist, history_lens=lens, frequency=freq, presence=pres, count_start=start, count_max=HCAP).cpu()
    assert calls == []
    assert torch.equal(got, _statement(logits, pk, hist, lens, start, freq, pres, {}).cpu())
    assert int(got[0]) != int(logits[0].argmax()), "the arg max was counted and penalised: the case does not test the copy path otherwise"


@pytest.mark.gpu
@torch.inference_mode()
def test_capture_and_replay_of_the_two_launches():
    """penalty_edits and the edit launch in ONE captured graph with static merged buffers; history, history_lens and the penalties are
    rewritten between the replays, and each replay equals the eager call on the same contents."""
    import omnimamba_amd.sampling as S
    dev = torch.device("cuda:0")
    n = 10
    c1 = [_to(x, dev) for x in _case(V, torch.float32, n, 3, True, True)]
    logits, params, hist, lens, start, freq, pres, ed = c1
    hist2 = hist.clone()
    hist2[:, PROMPT:PROMPT + 5] = hist[:, PROMPT + 2:PROMPT + 7]
    lens2 = (lens - 2).contiguous()
    freq2, pres2 = (freq * 0.5 + 0.25).contiguous(), (1.0 - pres).contiguous()
    st = {"hist": hist.clone(), "lens": lens.clone(), "freq": freq.clone(), "pres": pres.clone()}
    pk = S.pack_rows(params, dev)
    out = torch.full((n,), -1, dtype=torch.int64, device=dev)
    bufs = {k: torch.zeros_like(v) for k, v in S.penalty_edits(hist, lens, start, freq, pres, V, **ed, out_cap=64).items()}
    run = lambda: S.sample_rows(logits, **pk, **ed, history=st["hist"], history_lens=st["lens"], frequency=st["freq"], presence=st["pres"],
                                count_start=start, count_max=HCAP - PROMPT, merged=bufs, out=out)
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
    for k, v in (("hist", hist2), ("lens", lens2), ("freq", freq2), ("pres", pres2)):
        st[k].copy_(v)
    graph.replay()
    got2 = out.clone()
    torch.cuda.synchronize()
    kw = dict(count_start=start, count_max=HCAP - PROMPT)
    e1 = S.sample_rows(logits, **pk, **ed, history=hist, history_lens=lens, frequency=freq, presence=pres, **kw)
    e2 = S.sample_rows(logits, **pk, **ed, history=hist2, history_lens=lens2, frequency=freq2, presence=pres2, **kw)
    assert torch.equal(got1, e1) and torch.equal(got2, e2) and not torch.equal(got1, got2)
    assert torch.equal(e2, _statement(logits, pk, hist2, lens2, start, freq2, pres2, ed))
