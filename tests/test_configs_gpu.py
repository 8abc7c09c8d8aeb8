"""Every BASELINE.json config at its FULL size on the MI355X (-m gpu), against the CPU oracle where the domain lets a
slice be checked in seconds (heads / channels / rows are independent), plus finite-loss / gradient checks for the two
1.3B training configs.  Complements the small-shape parity tests: the XCD-aware workgroup order (grids of 512), 64-chunk
carries (L = 4096) and 64-head group sharing only exist at these sizes."""
import math

import pytest
import torch

import oracle as O

pytestmark = pytest.mark.gpu
from tolerances import ARITH_BUDGET, Q_BF16, arith_part, direct_bound, forward_budget, training_budget   # the tolerance rules (tests/tolerances.py)


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


SLOW_HEADS = (5, 40)   # forced to the slow corner of the module's init range: A in [1, 2], dt0 ~ 1e-3 (state-dominated outputs)


def _cfg2_inputs(seed=0):
    g = torch.Generator().manual_seed(seed)
    Bsz, L, H, P, N = 8, 4096, 64, 64, 128
    x = torch.randn(Bsz, L, H, P, generator=g).bfloat16()
    dt = (torch.randn(Bsz, L, H, generator=g) * 0.5).bfloat16()
    A = -(torch.rand(H, generator=g) * 15 + 1)
    Bm, Cm = torch.randn(Bsz, L, 1, N, generator=g).bfloat16(), torch.randn(Bsz, L, 1, N, generator=g).bfloat16()
    D = torch.randn(H, generator=g)
    # module-style dt bias: softplus^-1 of a log-uniform dt in [1e-3, 0.1]
    dt0 = torch.exp(torch.rand(H, generator=g) * (math.log(0.1) - math.log(1e-3)) + math.log(1e-3))
    # two heads in the slow-decay corner: their output is the carried state, where the bf16 operands of the
    # state update and of S_in^T Q^T cost the most
    for i, h in enumerate(SLOW_HEADS):
        A[h] = -(1.0 + 0.7 * i)
        dt0[h] = 1e-3 * (1.0 + i)
    dtb = dt0 + torch.log(-torch.expm1(-dt0))
    return x, dt, A, Bm, Cm, D, dtb


def _write_parity_table(name, lines):
    """The per-head table the production-shape tests print, kept under gpurun_out/ (copied to profiles/ per round)."""
    import os
    d = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gpurun_out", "parity")
    os.makedirs(d, exist_ok=True)
    with open(os.path.join(d, name), "w") as f:
        f.write("\n".join(lines) + "\n")


def test_cfg2_scan_forward_production_shape_vs_oracle():
    """configs[1] scan shape B 8, L 4096, H 64, P 64, N 128 bf16: (b, h) slices of y and the final state vs the fp64 recurrence on the
    same bf16 inputs under the rule of tests/tolerances.py -- for BOTH instantiations of the kernel: the one that keeps the final
    state (hi + lo operand of the state update) and the one a training step and bench.py launch (no final state, window-state
    images saved: single bf16 operand) -- and for the PRECISE instantiation (OmkSsdFwd.flags & OMK_SSD_PRECISE), which must meet the
    BARE 1e-3 on every slice.  Two of the sampled heads sit in the slow-decay corner (A in [1, 2], dt0 ~ 1e-3)."""
    from omnimamba_amd import _capi as K
    from omnimamba_amd.ssd_combined import ssd_scan_fwd
    dev = torch.device("cuda:0")
    x, dt, A, Bm, Cm, D, dtb = _cfg2_inputs()
    args = (x.to(dev), dt.to(dev), A.to(dev), Bm.to(dev), Cm.to(dev))
    kw = dict(D=D.to(dev), dt_bias=dtb.to(dev), dt_softplus=True)
    y, _, fin = ssd_scan_fwd(*args, return_final_states=True, **kw)
    yt, _, _, wst = ssd_scan_fwd(*args, return_final_states=False, save_window_states=True, **kw)     # as Stage2Step / bench.py launch it
    yp, _, finp = ssd_scan_fwd(*args, return_final_states=True, flags=K.SSD_PRECISE, **kw)
    torch.cuda.synchronize()
    assert wst is not None
    assert torch.isfinite(y.float()).all() and torch.isfinite(yt.float()).all()
    rows = ["# b h A_h dt0 | y arithmetic error vs fp64: keep-final kernel, training kernel, PRECISE kernel, upstream-rounding oracle, rule "
            "| direct distance to the upstream-rounding oracle: keep-final, training | final state: ours, PRECISE, upstream"]
    bad = []
    for b, h in ((0, 0), (0, 63), (3, 17), (7, 5), (7, 63), (4, 32), (1, 1), (6, 40), (2, 5), (5, 40)):
        sl = (x[b:b + 1, :, h:h + 1], dt[b:b + 1, :, h:h + 1], A[h:h + 1], Bm[b:b + 1], Cm[b:b + 1])
        y64, f64, by, bf, (eu, efu), (yu, fu) = forward_budget(*sl, D=D[h:h + 1], dt_bias=dtb[h:h + 1], dt_softplus=True, return_upstream=True)
        q = rel(y64[0, :, 0].bfloat16().float(), y64[0, :, 0])        # what one rounding of the exact result to bf16 costs on this slice
        e, et = arith_part(rel(y[b, :, h], y64[0, :, 0]), q), arith_part(rel(yt[b, :, h], y64[0, :, 0]), q)
        ep, efp = arith_part(rel(yp[b, :, h], y64[0, :, 0]), q), rel(finp[b, h], f64[0, 0])
        ef = rel(fin[b, h], f64[0, 0])
        dy_, dyt_, df_ = rel(y[b, :, h], yu[0, :, 0]), rel(yt[b, :, h], yu[0, :, 0]), rel(fin[b, h], fu[0, 0])   # DIRECT distances
        dt0 = float(torch.nn.functional.softplus(dtb[h]))
        rows.append(f"{b} {h:2d} {float(A[h]):7.2f} {dt0:.4f} | {e:.3e} {et:.3e} {ep:.3e} {eu:.3e} {by:.3e} | {arith_part(dy_, q):.3e} {arith_part(dyt_, q):.3e} "
                    f"| {ef:.3e} {efp:.3e} {efu:.3e}")
        # keep-final kernel: the shared rule; training kernel: training_budget; PRECISE: the bare north-star number (tests/tolerances.py)
        byt = training_budget(eu)
        if et > by:
            rows[-1] += "   <- training kernel above 1.05 x upstream"
        ok = (e <= by and et <= byt and ef <= ARITH_BUDGET and dy_ <= direct_bound(by, eu, q) and dyt_ <= direct_bound(byt, eu, q)
              and df_ <= direct_bound(ARITH_BUDGET, efu) and ep <= ARITH_BUDGET and efp <= ARITH_BUDGET)
        if not ok:
            bad.append(rows[-1])
    _write_parity_table("cfg2_forward.txt", rows)
    print("\n".join(rows))
    assert not bad, bad


def test_scan_b1_l8192_split_sequence_prefill_hand_off():
    """The north star's B = 1 shape (H 64, L 8192): 64 (batch, head) pairs leave CUs idle, so the sequence is SPLIT into segments whose
    start states come from a zero-start state pass + fold.  A prefill that keeps its final state (models/stage2/generation.py:195-211
    decodes from it) must hand over a state exact to fp32 accumulation here too (9.3e-4 .. 9.8e-4 on a slow head
    when the segment pass rounded its operand to bf16), and y must meet the rule of tests/tolerances.py."""
    from omnimamba_amd.ssd_combined import ssd_scan_fwd
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(21)
    Bsz, L, H, P, N = 1, 8192, 64, 64, 128
    x = torch.randn(Bsz, L, H, P, generator=g).bfloat16()
    dt = (torch.randn(Bsz, L, H, generator=g) * 0.5).bfloat16()
    A = -(torch.rand(H, generator=g) * 15 + 1)
    Bm, Cm = torch.randn(Bsz, L, 1, N, generator=g).bfloat16(), torch.randn(Bsz, L, 1, N, generator=g).bfloat16()
    D = torch.randn(H, generator=g)
    dt0 = torch.exp(torch.rand(H, generator=g) * (math.log(0.1) - math.log(1e-3)) + math.log(1e-3))
    A[9], dt0[9] = -1.0, 1e-3       # slow heads: the state remembers the whole sequence
    A[50], dt0[50] = -2.0, 2e-3
    dtb = dt0 + torch.log(-torch.expm1(-dt0))
    y, _, fin = ssd_scan_fwd(x.to(dev), dt.to(dev), A.to(dev), Bm.to(dev), Cm.to(dev), D=D.to(dev), dt_bias=dtb.to(dev),
                             dt_softplus=True, return_final_states=True)
    torch.cuda.synchronize()
    rows = ["# h A_h dt0 | final state vs fp64 (ours, upstream-rounding oracle) | y arithmetic error (ours, upstream-rounding oracle, rule)"]
    bad = []
    for h in (9, 50, 0, 33):
        sl = (x[:, :, h:h + 1], dt[:, :, h:h + 1], A[h:h + 1], Bm, Cm)
        y64, f64, by, bf, (eu, efu) = forward_budget(*sl, D=D[h:h + 1], dt_bias=dtb[h:h + 1], dt_softplus=True)
        q = rel(y64[0, :, 0].bfloat16().float(), y64[0, :, 0])
        e, ef = arith_part(rel(y[0, :, h], y64[0, :, 0]), q), rel(fin[0, h], f64[0, 0])
        rows.append(f"{h:2d} {float(A[h]):7.2f} {float(dt0[h]):.4f} | {ef:.3e} {efu:.3e} | {e:.3e} {eu:.3e} {by:.3e}")
        if not (ef <= 2e-5 and e <= by):
            bad.append(rows[-1])
    _write_parity_table("b1_l8192_split.txt", rows)
    print("\n".join(rows))
    assert not bad, bad


def test_cfg2_scan_backward_production_shape_vs_oracle():
    """Same shape, backward: dx / ddt of sampled heads and the full-group sums dB, dC, and dA / dD / d(dt_bias), for one
    batch element against autograd of the fp32 oracle (the other seven run the same code on other data)."""
    from omnimamba_amd.ssd_combined import mamba_chunk_scan_combined
    dev = torch.device("cuda:0")
    x, dt, A, Bm, Cm, D, dtb = _cfg2_inputs(1)
    g = torch.Generator().manual_seed(5)
    dy = torch.randn(x.shape, generator=g).bfloat16()
    leaves = [t.to(dev).requires_grad_() for t in (x, dt, A, Bm, Cm, D, dtb)]
    y = mamba_chunk_scan_combined(leaves[0], leaves[1], leaves[2], leaves[3], leaves[4], 256, D=leaves[5], dt_bias=leaves[6], dt_softplus=True)
    y.backward(dy.to(dev))
    torch.cuda.synchronize()
    b = 5
    ref = [t[b:b + 1].float().requires_grad_() if t.dim() >= 3 else t.clone().float().requires_grad_() for t in (x, dt, A, Bm, Cm, D, dtb)]
    y0 = O.ssd_ref_chunked(ref[0], ref[1], ref[2], ref[3], ref[4], 256, D=ref[5], dt_bias=ref[6], dt_softplus=True)
    y0.backward(dy[b:b + 1].float())
    # the forward this backward belongs to is the training instantiation (no final state, window states saved): its y too
    assert rel(y[b], y0[0]) < math.sqrt(Q_BF16 ** 2 + (2.2e-3) ** 2), rel(y[b], y0[0])
    assert rel(leaves[0].grad[b], ref[0].grad[0]) < 5e-3           # dx
    assert rel(leaves[3].grad[b], ref[3].grad[0]) < 4e-3           # dB: sum over the 64 heads of the group
    assert rel(leaves[4].grad[b], ref[4].grad[0]) < 4e-3           # dC
    assert rel(leaves[1].grad[b], ref[1].grad[0]) < 4e-3           # d(dt)
    for t in leaves:
        assert torch.isfinite(t.grad.float()).all()
    # dA, dD, d(dt_bias) are sums over the whole batch and every token of a head: the oracle on all 8 batch elements for four
    # sampled heads (heads are independent; B and C enter as shared inputs)
    hs = [0, 17, 40, 63]
    got = {n: leaves[i].grad.float().cpu() for n, i in (("A", 2), ("D", 5), ("dtb", 6))}
    want = {n: [] for n in got}
    for h in hs:
        r = [x[:, :, h:h + 1].float().requires_grad_(), dt[:, :, h:h + 1].float().requires_grad_(), A[h:h + 1].clone().requires_grad_(),
             Bm.float(), Cm.float(), D[h:h + 1].clone().requires_grad_(), dtb[h:h + 1].clone().requires_grad_()]
        O.ssd_ref_chunked(r[0], r[1], r[2], r[3], r[4], 256, D=r[5], dt_bias=r[6], dt_softplus=True).backward(dy[:, :, h:h + 1].float())
        want["A"].append(r[2].grad); want["D"].append(r[5].grad); want["dtb"].append(r[6].grad)
    for n in got:
        w_ = torch.cat(want[n])
        assert rel(got[n][hs], w_) < 5e-3, (n, got[n][hs], w_)


def test_cfg2_conv_and_gated_norm_rows_production_shape():
    """conv1d + SiLU over the 4352 xBC channels (channel-last, the zxbcdt view) and the 4096-wide gated RMSNorm at
    B 8 L 4096, two batch elements / 2048 rows against the oracle."""
    from omnimamba_amd.causal_conv1d import causal_conv1d_fn
    from omnimamba_amd.layernorm_gated import rmsnorm_fn
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(2)
    zx = torch.randn(8, 4096, 8512, generator=g).bfloat16()
    w, bias = torch.randn(4352, 4, generator=g) * 0.5, torch.randn(4352, generator=g) * 0.1
    xBC = zx.to(dev)[..., 4096:4096 + 4352]
    out = causal_conv1d_fn(xBC.transpose(1, 2), w.to(dev), bias.to(dev), activation="silu").transpose(1, 2)
    for b in (0, 7):
        ref = O.causal_conv1d_ref(zx[b:b + 1, :, 4096:4096 + 4352].transpose(1, 2).float(), w, bias, activation="silu").transpose(1, 2)
        assert rel(out[b], ref[0]) < 6e-3
    yv, wn = torch.randn(8 * 4096, 4096, generator=g).bfloat16(), torch.randn(4096, generator=g)
    z2 = zx.reshape(-1, 8512)[:, :4096]
    on = rmsnorm_fn(yv.to(dev), wn.to(dev), None, z=z2.to(dev), eps=1e-5, group_size=4096, norm_before_gate=False)
    rows = slice(30000, 32048)
    refn = O.rmsnorm_gated_ref(yv[rows].float(), wn, None, z=z2[rows].float(), eps=1e-5, group_size=4096, norm_before_gate=False)
    assert rel(on[rows], refn) < 6e-3


def test_cfg1_selective_scan_vs_ref():
    """configs[0]: Mamba-1 selective_scan_fn at B 2, L 1024, D 768, d_state 16 fp32 (SURVEY.md section 8d inputs) against
    the host restatement of selective_scan_ref, forward and backward."""
    from omnimamba_amd.selective_scan import selective_scan_fn
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    Bsz, Dm, L, N = 2, 768, 1024, 16
    u, delta = torch.randn(Bsz, Dm, L), torch.rand(Bsz, Dm, L) * 0.5
    A = -(torch.rand(Dm, N) + 0.1)
    Bm, Cm = torch.randn(Bsz, N, L), torch.randn(Bsz, N, L)
    D, z, db = torch.randn(Dm), torch.randn(Bsz, Dm, L), 0.1 * torch.randn(Dm)
    dout = torch.randn(Bsz, Dm, L)
    cpu = [t.clone().requires_grad_() for t in (u, delta, A, Bm, Cm, D, z, db)]
    ref, last = O.selective_scan_ref(*cpu[:5], cpu[5], cpu[6], cpu[7], True, True)
    ref.backward(dout)
    gpu = [t.to(dev).requires_grad_() for t in (u, delta, A, Bm, Cm, D, z, db)]
    out, glast = selective_scan_fn(*gpu[:5], gpu[5], gpu[6], gpu[7], True, True)
    out.backward(dout.to(dev))
    assert rel(out, ref) < 1e-3 and rel(glast, last) < 1e-3
    for name, a, b in zip("u delta A B C D z delta_bias".split(), gpu, cpu):
        assert rel(a.grad, b.grad) < 1e-3, name


@pytest.fixture(scope="module")
def lm_1p3b():
    from omnimamba_amd.stack import OmniMambaLM, StackConfig
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = OmniMambaLM(StackConfig.omnimamba_1_3b(), device=dev, dtype=torch.float32).eval()   # fp32 like scripts/inference_t2i.py:21-26
    yield model
    del model
    torch.cuda.empty_cache()


def test_cfg3_1p3b_t2i_decode_256_tokens(lm_1p3b):
    """configs[2]: 72-token prompt + 256 greedy image tokens on the random-init 1.3B stack: hipGraph replay == eager, ids
    inside the VQ codebook, exactly 256 sampled tokens, the reference's integer trace."""
    from omnimamba_amd.generation import decode
    dev = torch.device("cuda:0")
    model = lm_1p3b
    Pn, new = 72, 256
    ids = torch.zeros(1, Pn, dtype=torch.long, device=dev)
    emb = torch.randn(1, Pn, 2048, device=dev) * 0.02 + model.backbone.pos_embed[:, :Pn]
    tr_e, tr_g = [], []
    a = decode(ids, emb, model, Pn + new, top_k=1, task="t2i", cg=False, trace=tr_e)
    b = decode(ids, emb, model, Pn + new, top_k=1, task="t2i", cg=True, trace=tr_g)
    assert a.shape == (1, Pn + new) and torch.equal(a, b)
    assert int(a[:, Pn:].min()) >= 0 and int(a[:, Pn:].max()) < 16384
    assert tr_e == tr_g == [(0, None)] + [(o, o) for o in range(Pn, Pn + new - 1)]
    with torch.no_grad():
        lg = model(None, emb, task="t2i", num_last_tokens=1).t2i_logits
    assert torch.isfinite(lg).all() and int(lg[0, 0].argmax()) == int(a[0, Pn])


def test_decode_graph_follows_in_place_weight_updates(lm_1p3b):
    """a captured step must not keep a stale copy of -exp(A_log) after the weights change in place."""
    from omnimamba_amd.generation import decode
    dev = torch.device("cuda:0")
    model = lm_1p3b
    ids = torch.zeros(1, 8, dtype=torch.long, device=dev)
    emb = torch.randn(1, 8, 2048, device=dev) * 0.02
    decode(ids, emb, model, 24, top_k=1, task="t2i", cg=True)                 # captures the graph
    with torch.no_grad():
        for blk in model.backbone.layers:
            blk.mixer.A_log.add_(0.7)
    b = decode(ids, emb, model, 24, top_k=1, task="t2i", cg=True)             # replay of the SAME graph after the update
    a = decode(ids, emb, model, 24, top_k=1, task="t2i", cg=False)
    with torch.no_grad():
        for blk in model.backbone.layers:
            blk.mixer.A_log.sub_(0.7)
    assert torch.equal(a, b)


def _one_step(stage, tasks, seqlen, batch, cfg_kw):
    from omnimamba_amd.omni import OmniMambaPath
    from omnimamba_amd.stack import StackConfig
    from omnimamba_amd.train import Stage2Step, TrainConfig, synthetic_batch
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    cfg = StackConfig.omnimamba_1_3b(t2i_positions=max(seqlen, 329), mmu_positions=max(seqlen, 1500), **cfg_kw)
    model = OmniMambaPath(cfg, stage=stage, device=dev, dtype=torch.float32)
    step = Stage2Step(model, TrainConfig())
    before = {n: p.detach().clone() for n, p in list(model.named_parameters())[-4:] if p.requires_grad}
    data = synthetic_batch(cfg, batch, seqlen, dev, torch.bfloat16, tasks=tasks)
    total = step(data)
    torch.cuda.synchronize()
    assert math.isfinite(float(total))
    for t in tasks:                                    # random init: the loss of a uniform guess over the head's vocabulary
        v = float(step.last[t])
        assert 0.5 * math.log(16384) < v < 3.0 * math.log(50288), (t, v)
    missing = [n for n, p in model.named_parameters() if p.requires_grad and p.grad is None]
    assert not missing, missing[:5]
    gn = torch.sqrt(sum((p.grad.float() ** 2).sum() for p in model.parameters() if p.grad is not None))
    assert math.isfinite(float(gn)) and float(gn) > 0
    changed = [n for n, p in model.named_parameters() if n in before and not torch.equal(p.detach(), before[n])]
    assert changed                                      # the optimizer step moved the weights
    del step, model
    torch.cuda.empty_cache()


def test_cfg4_1p3b_stage1_mmu_step_L2048():
    """configs[3]: stage 'align', MMU only: images_feat (B, 729, 2176) -> FusedMLPProjector 2176 -> 8704 -> 2048 -> 2048,
    text ids of length 2048 - 733, projector + MMU LoRA train."""
    _one_step("align", ("mmu",), 2048, 8, dict(t2i_task=False, mmu_task=True))      # batch 8: the shape bench.py times (56 GB)


def test_cfg5_1p3b_stage2_step_L8192():
    """configs[4]: stage 'finetune', one T2I + one MMU forward of L = 8192 each, one backward, every parameter trains."""
    _one_step("finetune", ("t2i", "mmu"), 8192, 2, dict())      # batch 2 per task: the shape bench.py times (split sequences, B H = 128)


def test_device_loop_greedy_decode_equals_host_loop(lm_1p3b):
    """f3: argmax + id write-back + counters inside the captured step (GreedyLoopGraph) give the ids of the reference-shaped
    host loop, at the 1.3B size, 72-token prompt + 64 tokens."""
    from omnimamba_amd.generation import decode
    dev = torch.device("cuda:0")
    model = lm_1p3b
    Pn, new = 72, 64
    ids = torch.zeros(2, Pn, dtype=torch.long, device=dev)
    emb = torch.randn(2, Pn, 2048, device=dev) * 0.02 + model.backbone.pos_embed[:, :Pn]
    a = decode(ids, emb, model, Pn + new, top_k=1, task="t2i", cg=True)
    model._decoding_cache = None
    b = decode(ids, emb, model, Pn + new, top_k=1, task="t2i", cg=True, device_loop=True)
    c = decode(ids, emb, model, Pn + new, top_k=1, task="t2i", cg=True, device_loop=True)       # cached graph again
    model._decoding_cache = None
    assert a.shape == b.shape == (2, Pn + new) and torch.equal(a, b) and torch.equal(a, c)


def test_device_loop_sampled_decode_is_reproducible_and_in_range(lm_1p3b):
    """cfg 3 with sampling (the reference's inference default is top_k > 1 for T2I): omk_sample inside the captured step, the
    Philox stream position advanced by the graph itself.  Same torch seed -> same 256 ids; another seed -> other ids; every id is
    a VQ code; the greedy loop differs."""
    from omnimamba_amd.generation import decode
    model = lm_1p3b
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    Pn, new = 72, 64
    ids = torch.zeros(1, Pn, dtype=torch.long, device=dev)
    emb = torch.randn(1, Pn, model.cfg.d_model, device=dev) * 0.02 + model.backbone.pos_embed[:, :Pn]
    torch.manual_seed(11)
    a = decode(ids, emb, model, Pn + new, top_k=20, top_p=0.9, temperature=0.8, task="t2i", cg=True, device_loop=True)
    torch.manual_seed(11)
    b = decode(ids, emb, model, Pn + new, top_k=20, top_p=0.9, temperature=0.8, task="t2i", cg=True, device_loop=True)
    torch.manual_seed(12)
    c = decode(ids, emb, model, Pn + new, top_k=20, top_p=0.9, temperature=0.8, task="t2i", cg=True, device_loop=True)
    c2 = decode(ids, emb, model, Pn + new, top_k=20, top_p=0.9, temperature=0.8, task="t2i", cg=True, device_loop=True)   # no re-seed: a new stretch of the stream
    g = decode(ids, emb, model, Pn + new, top_k=1, task="t2i", cg=True, device_loop=True)
    # the default arguments of the reference's t2i_generate (top_k = 0, top_p = 1.0): full-vocabulary multinomial, also inside the graph
    torch.manual_seed(11)
    f1 = decode(ids, emb, model, Pn + new, top_k=0, top_p=1.0, task="t2i", cg=True, device_loop=True)
    torch.manual_seed(11)
    f2 = decode(ids, emb, model, Pn + new, top_k=0, top_p=1.0, task="t2i", cg=True, device_loop=True)
    model._decoding_cache = None
    assert a.shape == (1, Pn + new) and torch.equal(a, b)
    assert not torch.equal(a, c) and not torch.equal(a, g)
    assert not torch.equal(c, c2)      # successive calls are independent draws, as with the reference's torch.multinomial
    assert int(a[:, Pn:].min()) >= 0 and int(a[:, Pn:].max()) < model.cfg.vqvae_vocab_size
    assert torch.equal(f1, f2) and not torch.equal(f1, g) and int(f1[:, Pn:].min()) >= 0 and int(f1[:, Pn:].max()) < model.cfg.vqvae_vocab_size


# ---------------------------------------------------------------------------------------------------------------------------------
# Production-shape backward parity of the non-scan ops (1.3B geometry: B 8, L 4096, d_model 2048, d_ssm 4096, xBC 4352, zxbcdt 8512),
# bounds of tolerances.op_bound: fp64 references from exactly the tensors each kernel reads, computed on the device in row chunks.
# ---------------------------------------------------------------------------------------------------------------------------------
from tolerances import OP_ARITH, op_bound  # noqa: E402


class _Err:
    """Relative L2 error, and the op_bound quantisation term, accumulated over row chunks of one output."""

    def __init__(self, dtype):
        self.dtype, self.d2, self.r2, self.q2 = dtype, 0.0, 0.0, 0.0

    def add(self, got, ref):
        ref = ref.double()
        self.d2 += (got.double() - ref).pow(2).sum().item()
        self.r2 += ref.pow(2).sum().item()
        if self.dtype not in (torch.float32, torch.float64):
            self.q2 += (ref.to(self.dtype).double() - ref).pow(2).sum().item()

    def result(self):
        r2 = max(self.r2, 1e-300)
        e, q = math.sqrt(self.d2 / r2), math.sqrt(self.q2 / r2)
        return e, 1.1 * math.sqrt(q * q + OP_ARITH * OP_ARITH)


def _assert_table(name, errs, extra=()):
    """errs: {output: (error, bound)}; writes the table first, so that a failing run still leaves every number."""
    lines = [f"{'output':28s} {'rel-L2 error':>12s} {'bound':>10s}"] + [f"{k:28s} {e:12.3e} {b:10.3e}" for k, (e, b) in errs.items()]
    _write_parity_table(name, lines + list(extra))
    bad = {k: v for k, v in errs.items() if not v[0] <= v[1]}
    assert not bad, bad


def test_prod_conv1d_bwd_on_the_xbc_view():
    """causal_conv1d backward on the xBC view of zxbcdt (B 8, L 4096, C 4352, W 4, channel-last): conv1d_bwd_cl4_kernel over 34 channel
    blocks and the fold of B x 16 partial rows.  dx on sampled channel slices (channels are independent), dw / db over all 8 batch
    elements for those channels, against fp64."""
    from omnimamba_amd.causal_conv1d import causal_conv1d_fn
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(21)
    zx = torch.randn(8, 4096, 8512, generator=g).bfloat16()
    w, bias = torch.randn(4352, 4, generator=g) * 0.5, torch.randn(4352, generator=g) * 0.1
    gout = torch.randn(8, 4096, 4352, generator=g).bfloat16()
    zxd = zx.clone().to(dev).requires_grad_()
    wr, br = w.clone().to(dev).requires_grad_(), bias.clone().to(dev).requires_grad_()
    out = causal_conv1d_fn(zxd[..., 4096:4096 + 4352].transpose(1, 2), wr, br, activation="silu")
    out.backward(gout.to(dev).transpose(1, 2))
    torch.cuda.synchronize()
    dzx, dw, db = zxd.grad, wr.grad.cpu(), br.grad.cpu()
    assert float(dzx[..., :4096].abs().max()) == 0.0 and float(dzx[..., 4096 + 4352:].abs().max()) == 0.0   # z and dt untouched
    chans = torch.cat([torch.arange(0, 64), torch.arange(2100, 2164), torch.arange(4096, 4352)])   # x, the middle, B and C
    errs = {k: _Err(dt_) for k, dt_ in (("out", torch.bfloat16), ("dx", torch.bfloat16), ("dweight", torch.float32), ("dbias", torch.float32))}
    xs = zx[..., 4096 + chans].transpose(1, 2).double().requires_grad_()
    ws, bs = w[chans].double().requires_grad_(), bias[chans].double().requires_grad_()
    od = O.causal_conv1d_ref(xs, ws, bs, activation="silu", compute_dtype=torch.float64)
    od.backward(gout[..., chans].transpose(1, 2).double())
    errs["out"].add(out.detach()[:, chans].cpu(), od.detach())
    errs["dx"].add(dzx[..., 4096 + chans].transpose(1, 2).cpu(), xs.grad)
    errs["dweight"].add(dw[chans], ws.grad)
    errs["dbias"].add(db[chans], bs.grad)
    _assert_table("prod_conv1d_bwd.txt", {k: v.result() for k, v in errs.items()}, [f"channels: {len(chans)} of 4352, all 8 x 4096 tokens"])


@pytest.mark.parametrize("rows", [32768, 32768 + 3])
def test_prod_gated_norm_bwd_w8(rows):
    """The 4096-wide gated RMSNorm (one group, bf16, gate after the norm): forward lean kernel and norm_gated_bwd_w8_kernel at the
    production row count (every one of 512 workgroups walks 64 rows; + 3: a ragged last round) and its 512-row fold.  dx, dz of every
    row and dw over all rows against fp64."""
    from omnimamba_amd.layernorm_gated import rmsnorm_fn
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(22)
    x = torch.randn(rows, 4096, generator=g, device=dev).bfloat16()
    z = torch.randn(rows, 4096, generator=g, device=dev).bfloat16()
    w = torch.randn(4096, generator=g, device=dev)
    gy = torch.randn(rows, 4096, generator=g, device=dev).bfloat16()
    xr, zr, wr = x.clone().requires_grad_(), z.clone().requires_grad_(), w.clone().requires_grad_()
    y = rmsnorm_fn(xr, wr, None, z=zr, eps=1e-5, group_size=None, norm_before_gate=False)
    y.backward(gy)
    torch.cuda.synchronize()
    errs = {k: _Err(torch.bfloat16 if k != "dweight" else torch.float32) for k in ("y", "dx", "dz", "dweight")}
    wd = w.double().requires_grad_()
    for r0 in range(0, rows, 4096):
        s = slice(r0, min(rows, r0 + 4096))
        xd, zd = x[s].double().requires_grad_(), z[s].double().requires_grad_()
        yd = O.rmsnorm_gated_ref(xd, wd, None, z=zd, eps=1e-5, group_size=None, norm_before_gate=False, compute_dtype=torch.float64)
        yd.backward(gy[s].double())
        errs["y"].add(y[s].detach(), yd.detach())
        errs["dx"].add(xr.grad[s], xd.grad)
        errs["dz"].add(zr.grad[s], zd.grad)
    errs["dweight"].add(wr.grad, wd.grad)
    _assert_table(f"prod_gated_norm_bwd_{rows}.txt", {k: v.result() for k, v in errs.items()})


def test_prod_add_norm_fwd_bwd_residual_in_fp32():
    """add + RMSNorm at 32 768 x 2048 as the model runs it (bf16 x, fp32 residual stream): the {8,1,4} plan, the wvec forward's
    two-block-row grid (32 768 rows > 2048 workgroups), the backward's 1024 partial rows and their fold.  The backward's reference
    takes the forward's saved residual_out and rstd."""
    from omnimamba_amd.layer_norm import layer_norm_fn
    dev = torch.device("cuda:0")
    rows, cols = 32768, 2048
    g = torch.Generator(device=dev).manual_seed(23)
    x = torch.randn(rows, cols, generator=g, device=dev).bfloat16()
    res = torch.randn(rows, cols, generator=g, device=dev) * 2
    w = torch.randn(cols, generator=g, device=dev)
    gy = torch.randn(rows, cols, generator=g, device=dev).bfloat16()
    gr = torch.randn(rows, cols, generator=g, device=dev)
    xr, rr, wr = x.clone().requires_grad_(), res.clone().requires_grad_(), w.clone().requires_grad_()
    y, ro = layer_norm_fn(xr, wr, None, residual=rr, eps=1e-5, prenorm=True, residual_in_fp32=True, is_rms_norm=True)
    xsum, _, _, _, rstd = y.grad_fn.saved_tensors
    torch.autograd.backward([y, ro], [gy, gr])
    torch.cuda.synchronize()
    errs = {k: _Err(dt_) for k, dt_ in (("y", torch.bfloat16), ("residual_out", torch.float32), ("rstd", torch.float32),
                                        ("dx", torch.bfloat16), ("dresidual", torch.float32), ("dweight", torch.float32),
                                        ("dx end-to-end", torch.bfloat16))}
    dw64 = torch.zeros(cols, dtype=torch.float64, device=dev)
    for r0 in range(0, rows, 4096):
        s = slice(r0, r0 + 4096)
        r64 = x[s].double() + res[s].double()
        rs64 = torch.rsqrt(r64.pow(2).mean(-1, keepdim=True) + 1e-5)
        errs["y"].add(y[s].detach(), r64 * rs64 * w.double())
        errs["residual_out"].add(ro[s].detach(), r64)
        errs["rstd"].add(rstd[s], rs64[:, 0])
        # backward from its own inputs: saved xsum (fp32 residual_out) and rstd
        xhat = xsum[s].double() * rstd[s].double()[:, None]
        wdy = w.double() * gy[s].double()
        dx64 = (wdy - xhat * (xhat * wdy).mean(-1, keepdim=True)) * rstd[s].double()[:, None] + gr[s].double()
        errs["dx"].add(xr.grad[s], dx64)
        errs["dresidual"].add(rr.grad[s], dx64)
        dw64 += (gy[s].double() * xhat).sum(0)
        # end to end (the old 1.5e-2 regime): from x and residual alone
        xh = r64 * rs64
        errs["dx end-to-end"].add(xr.grad[s], (wdy - xh * (xh * wdy).mean(-1, keepdim=True)) * rs64 + gr[s].double())
    errs["dweight"].add(wr.grad, dw64)
    table = {k: v.result() for k, v in errs.items()}
    table["dx end-to-end"] = (table["dx end-to-end"][0], 1.5e-2)
    _assert_table("prod_add_norm.txt", table)


def test_prod_lora_add_and_up_bwd():
    """omk_lora_add and omk_lora_up_bwd at the training shape (T 16 384, N 8 512, r 8: 34 column blocks x 15 token chunks, a ragged
    last chunk): the output, dh and the folded dB against fp64."""
    from omnimamba_amd import lora_add as LA
    dev = torch.device("cuda:0")
    T, N = 16384, 8512
    g = torch.Generator(device=dev).manual_seed(24)
    res = torch.randn(T, N, generator=g, device=dev).bfloat16()
    h = torch.randn(T, 8, generator=g, device=dev).bfloat16()
    Bw = torch.randn(N, 8, generator=g, device=dev) * 0.1
    dy = torch.randn(T, N, generator=g, device=dev).bfloat16()
    out = res.clone()
    assert LA.applies(out, h, Bw) and LA.up_bwd_applies(dy, h, Bw)
    LA.lora_add_(out, h, Bw, 2.0)
    dh, dB = LA.lora_up_bwd(dy, h, Bw)
    torch.cuda.synchronize()
    errs = {"lora_add out": _Err(torch.bfloat16), "up_bwd dh": _Err(torch.float32), "up_bwd dB": _Err(torch.float32)}
    for t0 in range(0, T, 2048):
        s = slice(t0, t0 + 2048)
        errs["lora_add out"].add(out[s], res[s].double() + 2.0 * h[s].double() @ Bw.double().t())
        errs["up_bwd dh"].add(dh[s], dy[s].double() @ Bw.bfloat16().double())   # (lora_b as bf16 MFMA fragments)
    errs["up_bwd dB"].add(dB, dy.double().t() @ h.double())
    table = {k: v.result() for k, v in errs.items()}
    for k in ("up_bwd dh", "up_bwd dB"):                 # test_lora_up_bwd's bound, tighter than op_bound's fp32 allowance
        table[k] = (table[k][0], min(table[k][1], 1e-5))
    _assert_table("prod_lora.txt", table)


def test_prod_fused_split_conv_scan_backward():
    """MambaSplitConv1dScanCombinedFn backward with the gated norm at the 1.3B width (B 8, L 4096, H 64, P 64, N 128, G 1, W 4) against
    autograd through the oracle composition (conv -> scan -> gated norm, fp32, with the pipeline's two bf16 rounding points:
    conv output and pre-norm y).  The z / xBC / dt slices of d zxbcdt of one batch
    element of the B 8 call; the parameter gradients (conv weight / bias, A, D, dt_bias, norm weight: sums over the batch) from a call
    on that element alone.  Wiring errors are O(1): gradients through the scan keep the bounds of
    test_cfg2_scan_backward_production_shape_vs_oracle (5e-3 / 4e-3)."""
    import omnimamba_amd.ssd_combined as S
    dev = torch.device("cuda:0")
    Bsz, L, H, P, N, G, W = 8, 4096, 64, 64, 128, 1, 4
    d_ssm, Ct = H * P, H * P + 2 * G * N
    g = torch.Generator().manual_seed(25)
    zxbcdt = (torch.randn(Bsz, L, 2 * d_ssm + 2 * G * N + H, generator=g) * 0.8).bfloat16()
    cw, cb = torch.randn(Ct, W, generator=g) * 0.4, torch.randn(Ct, generator=g) * 0.2
    dtb, A, D = torch.randn(H, generator=g) * 0.5 - 2.0, -(torch.rand(H, generator=g) * 8 + 0.5), torch.randn(H, generator=g)
    nw = torch.rand(d_ssm, generator=g) + 0.5
    gy = torch.randn(Bsz, L, d_ssm, generator=g).bfloat16()
    b = 3

    def fused(zx, gout):
        leaves = [t.clone().to(dev).requires_grad_() for t in (zx, cw, cb, dtb, A, D, nw)]
        out = S.mamba_split_conv1d_scan_combined(leaves[0], leaves[1], leaves[2], leaves[3], leaves[4], leaves[5], 256, rmsnorm_weight=leaves[6],
                                                 rmsnorm_eps=1e-5, headdim=P, ngroups=G, norm_before_gate=False)
        out.backward(gout.to(dev))
        torch.cuda.synchronize()
        return [t.grad.float().cpu() for t in leaves]

    full = fused(zxbcdt, gy)
    one = fused(zxbcdt[b:b + 1], gy[b:b + 1])
    ref = [t.float().requires_grad_() for t in (zxbcdt[b:b + 1], cw, cb, dtb, A, D, nw)]
    yr = O.mamba_split_conv1d_scan_combined_ref(ref[0], ref[1], ref[2], ref[3], ref[4], ref[5], 256, rmsnorm_weight=ref[6], rmsnorm_eps=1e-5,
                                                headdim=P, ngroups=G, norm_before_gate=False, round_intermediates=True)
    yr.backward(gy[b:b + 1].float())
    dz_ref = ref[0].grad[0]
    sl = {"d zxbcdt: z": slice(0, d_ssm), "d zxbcdt: xBC": slice(d_ssm, d_ssm + Ct), "d zxbcdt: dt": slice(d_ssm + Ct, None)}
    table = {}
    for k, s in sl.items():
        table[k] = (rel(full[0][b][:, s], dz_ref[:, s]), 4e-3 if k.endswith("dt") else 5e-3)
        table[k + " (B 1 call)"] = (rel(one[0][0][:, s], dz_ref[:, s]), table[k][1])
    for i, k in ((1, "conv weight"), (2, "conv bias"), (3, "dt_bias"), (4, "A"), (5, "D"), (6, "norm weight")):
        table[k] = (rel(one[i], ref[i].grad), 5e-3)
    _assert_table("prod_fused_split_conv_scan_bwd.txt", table, [f"d zxbcdt of batch element {b} of the B 8 call; parameters from a B 1 call on it"])
