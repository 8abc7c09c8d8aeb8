"""mmu_continue(extend_batch=N): the follow-up turns of the conversations that find a free slot at the same moment are extended by ONE
right-padded pass on their pool slots (InferenceParams.state_indices + extend_lens) instead of one batch-1 pass each.

The five conversations, the model and check_turn of test_mmu_continue.py.  With extend_batch=4 and max_batch=4 the first four second
turns (1 + 5 / 2 / 70 / 8 positions: the padded pass is long enough for the chunked scan) go through one grouped call and the fifth
through today's batch-1 extend when a slot frees up; ids and state lengths agree with the extend_batch=1 run and with mmu_generate on the
full prompt under check_turn, whose tie excuse at most one conversation may need.  Emulator on CPU, MI355X under -m gpu."""
import torch

from test_mmu_continue import check_turn, conversations, model_on


def spy_on_forward(lm, calls):
    real = lm.forward

    def forward(input_ids, input_embeddings, *a, **k):
        ip = k.get("inference_params")
        if input_embeddings is not None and ip is not None and ip.seqlen_offset > 0:
            calls.append((tuple(input_embeddings.shape[:2]), getattr(ip, "extend_lens", None) is not None))
        return real(input_ids, input_embeddings, *a, **k)
    lm.forward = forward


def test_mmu_continue_extend_batch(dev):
    model = model_on(dev)
    n = 5
    feats, q1, q2 = conversations(dev, n)
    free = [model.mmu_generate(f, q, max_length=26, cg=False) for f, q in zip(feats, q1)]
    gens = [s[0, 4 + q.shape[1]:].tolist() for s, q in zip(free, q1)]
    eos = next(t for t in (g[1] for g in gens if len(g) > 2) if sum(t in g for g in gens) < len(gens))
    max1 = [26, 30, 28, 25, 32]
    ids1, st1 = model.mmu_generate_batch(feats, q1, max_length=max1, eos_token_id=eos, max_batch=2, cg=False, return_states=True)
    max2 = [m + 30 + q.shape[1] for m, q in zip(max1, q2)]
    calls = []
    spy_on_forward(model.llm_backbone.mamba, calls)
    ids_a, st_a = model.mmu_continue(st1, q2, max_length=max2, eos_token_id=eos, max_batch=4, cg=False, extend_batch=1)
    turns = [1 + q.shape[1] for q in q2]
    assert calls == [((1, t), False) for t in turns], "extend_batch=1 admits every conversation alone and runs no grouped call"
    calls.clear()
    ids_b, st_b = model.mmu_continue(st1, q2, max_length=max2, eos_token_id=eos, max_batch=4, cg=False, extend_batch=4)
    assert calls == [((4, max(turns[:4])), True), ((1, turns[4]), False)], "one grouped extend for the first four, the fifth alone"
    excused = 0
    for i in range(n):
        a1 = ids1[i][:, 4 + q1[i].shape[1]:]
        full_q = torch.cat([q1[i], a1, q2[i]], dim=1)
        want = model.mmu_generate(feats[i], full_q, max_length=max2[i], eos_token_id=eos, cg=False)[0, 4 + full_q.shape[1]:].tolist()
        for ids, st in ((ids_a, st_a), (ids_b, st_b)):
            assert torch.equal(ids[i][:, :q2[i].shape[1]], q2[i])
            got = ids[i][0, q2[i].shape[1]:].tolist()
            check_turn(model, got, want, feats[i], full_q)
            assert st[i].seqlen == st1[i].seqlen + 1 + q2[i].shape[1] + len(got) - 1
        got_a, got_b = ids_a[i][0, q2[i].shape[1]:].tolist(), ids_b[i][0, q2[i].shape[1]:].tolist()
        check_turn(model, got_b, got_a, feats[i], full_q)
        if got_b == got_a:
            assert st_b[i].seqlen == st_a[i].seqlen and st_b[i].pending_id == st_a[i].pending_id
        excused += got_b != want
    assert excused <= 1, f"{excused} of {n} conversations needed check_turn's tie excuse"
