"""Multi-turn MMU decoding: turn 1 through mmu_generate_batch(return_states=True), turn 2 through mmu_continue (the states extended by
the pending id and the new question, never re-prefilled), several conversations at once with max_batch below their number.  The
turn-2 ids equal mmu_generate on the full prompt (image prompt + Q1 + A1 + Q2), greedy.

Why this is exact up to ties: the full-prompt run prefills the whole conversation through the fused conv1d + chunked-scan node, the
continued one extends a cached state (extend kernel, or the chunked scan with initial states for the long question); both compute the
same recurrence in fp32 with different association, so their logits differ at rounding level (~1e-6 relative).  The embeddings are
scaled up (test_batch_decode._separate) so that greedy choices are far apart; where the ids still differ, the full prompt's top-2
logit gap at that position must be below TIE_TOL, i.e. a genuine tie that no fp32 path could decide reliably.
Emulator on CPU, MI355X under -m gpu."""
import pytest
import torch

from test_batch_decode import _separate
from test_stack_decode_train import TINY_SPECIAL, tiny_cfg

TIE_TOL = 1e-3     # relative to the largest |logit| of the row: 10 x the module tolerance of test_mamba2_module.py (1e-4)


def model_on(dev, seed=11):
    from omnimamba_amd.omni import OmniMambaPath
    cfg = tiny_cfg()
    cfg.mmu_positions = 160
    torch.manual_seed(seed)
    m = OmniMambaPath(cfg, stage="inference", special_ids=TINY_SPECIAL).to(dev)
    _separate(m)
    return m


def conversations(dev, n, seed=12):
    g = torch.Generator().manual_seed(seed)
    q1 = [torch.randint(0, 50, (1, L), generator=g).to(dev) for L in [3, 9, 6, 4, 11][:n]]
    q2 = [torch.randint(0, 50, (1, L), generator=g).to(dev) for L in [5, 2, 70, 8, 3][:n]]   # 1 + 70 > EXTEND_SCAN_MAX_T: the chunked scan
    feats = [torch.randn(1, 5, 12, generator=g).to(dev) for _ in range(n)]
    return feats, q1, q2


def full_logits(model, feat, question):
    """Logits of the last position of the full prompt, no cache."""
    ids, emb = model._mmu_prompt(feat, question)
    lm = model.llm_backbone.mamba
    return lm(None, emb, task="mmu").mmu_logits[0, -1].float()


def check_turn(model, got, want, feat, question):
    """got / want: generated ids (lists).  Equal, or equal up to the first position where the full prompt's logits tie."""
    if got == want:
        return
    k = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
    prefix = torch.cat([question, torch.tensor([want[:k]], dtype=torch.long, device=question.device)], dim=1)
    with torch.no_grad():
        lg = full_logits(model, feat, prefix)
    top = lg.topk(2).values
    assert (top[0] - top[1]).item() < TIE_TOL * lg.abs().max().item(), (k, got, want)


@pytest.mark.parametrize("cg", [False, pytest.param(True, marks=pytest.mark.gpu)])
def test_mmu_continue_equals_full_prompt(dev, cg):
    if cg and dev.type == "cpu":
        pytest.skip("graphs: MI355X only")
    model = model_on(dev)
    n = 5
    feats, q1, q2 = conversations(dev, n)
    # an EOS that some answers of turn 1 reach
    free = [model.mmu_generate(f, q, max_length=26, cg=False) for f, q in zip(feats, q1)]
    gens = [s[0, 4 + q.shape[1]:].tolist() for s, q in zip(free, q1)]
    eos = next(t for t in (g[1] for g in gens if len(g) > 2) if sum(t in g for g in gens) < len(gens))
    max1 = [26, 30, 28, 25, 32]
    ids1, st1 = model.mmu_generate_batch(feats, q1, max_length=max1, eos_token_id=eos, max_batch=2, cg=cg, return_states=True)
    for i in range(n):
        want1 = model.mmu_generate(feats[i], q1[i], max_length=max1[i], eos_token_id=eos, cg=False)
        assert torch.equal(ids1[i], want1)
        a1 = ids1[i][:, 4 + q1[i].shape[1]:]
        # positions consumed: 4 + 5 image + question + every answer id but the last, which is pending
        assert st1[i].seqlen == 9 + q1[i].shape[1] + a1.shape[1] - 1 and st1[i].pending_id == int(a1[0, -1])
    max2 = [m + 30 + q.shape[1] for m, q in zip(max1, q2)]
    ids2, st2 = model.mmu_continue(st1, q2, max_length=max2, eos_token_id=eos, max_batch=2, cg=cg)
    assert len(ids2) == len(st2) == n
    for i in range(n):
        assert torch.equal(ids2[i][:, :q2[i].shape[1]], q2[i])
        a1 = ids1[i][:, 4 + q1[i].shape[1]:]
        full_q = torch.cat([q1[i], a1, q2[i]], dim=1)
        want = model.mmu_generate(feats[i], full_q, max_length=max2[i], eos_token_id=eos, cg=False)
        check_turn(model, ids2[i][0, q2[i].shape[1]:].tolist(), want[0, 4 + full_q.shape[1]:].tolist(), feats[i], full_q)
        n_gen = ids2[i].shape[1] - q2[i].shape[1]
        assert st2[i].seqlen == st1[i].seqlen + 1 + q2[i].shape[1] + n_gen - 1


def test_mmu_continue_position_table_raises(dev):
    model = model_on(dev)
    feats, q1, _ = conversations(dev, 1)
    _, st = model.mmu_generate_batch(feats, q1, max_length=20, max_batch=1, cg=False, return_states=True)
    room = model.cfg.mmu_positions - st[0].seqlen          # positions left: the pending id + room - 1 question ids fit
    with pytest.raises(IndexError):
        model.mmu_continue(st, [torch.zeros(1, room, dtype=torch.long, device=dev)], max_length=10_000, cg=False)
    ids, _ = model.mmu_continue(st, [torch.zeros(1, room - 1, dtype=torch.long, device=dev)], max_length=model.cfg.mmu_positions + 1,
                                cg=False)
    assert ids[0].shape[1] == room                          # the question and one sampled id: the table is full


def test_two_tuple_requests_unchanged_by_return_states(dev):
    model = model_on(dev)
    feats, q1, _ = conversations(dev, 3)
    plain = model.mmu_generate_batch(feats, q1, max_length=[20, 26, 23], max_batch=2, cg=False)
    ids, states = model.mmu_generate_batch(feats, q1, max_length=[20, 26, 23], max_batch=2, cg=False, return_states=True)
    assert isinstance(plain, list) and all(torch.equal(a, b) for a, b in zip(plain, ids))
    assert all(s.task == "mmu" and len(s.layers) == model.cfg.n_layer for s in states)
