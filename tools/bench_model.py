"""BASELINE.json configs[2..4] on the synthetic OmniMamba-1.3B stack (random init, synthetic data), 1 GPU or N GPUs via
torch.distributed.run:   python tools/bench_model.py [decode|train|decode_mmu_batch|step_index_cost|mmu_followup|ragged_prefill] [--batch B] [--seqlen L] [--steps K]
Prints one JSON line per workload (rank 0)."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from omnimamba_amd.generation import decode  # noqa: E402
from omnimamba_amd.omni import OmniMambaPath  # noqa: E402
from omnimamba_amd.stack import OmniMambaLM, StackConfig  # noqa: E402
from omnimamba_amd.train import Stage2Step, TrainConfig, init_distributed, synthetic_batch, wrap_ddp  # noqa: E402


class _ProjectionForms:
    """Which kernel each fused decode-step projection took (norm_linear.form), by projection and number of sequences: active around a
    warm-up run, asks once per (projection, sequences) and launches nothing itself.  -> {"in_proj": {"8": "matrix"}, ...}"""

    def __enter__(self):
        from omnimamba_amd import norm_linear as NL
        self.NL, self.real, self.forms = NL, NL.norm_linear, {}

        def logging(x, *a, **k):
            role, nseq = ("out_proj" if k.get("z") is not None else "in_proj"), str(x.shape[0])
            if nseq not in self.forms.setdefault(role, {}):
                f = NL.form(x, *a, **k)
                self.forms[role][nseq] = NL.FORM_NAMES.get(f, f"status {f}")
            return self.real(x, *a, **k)

        NL.norm_linear = logging
        return self

    def __exit__(self, *exc):
        self.NL.norm_linear = self.real

    def sorted(self):
        return {r: dict(sorted(d.items(), key=lambda kv: int(kv[0]))) for r, d in sorted(self.forms.items())}


def bench_decode(args, dev):
    """configs[2]: T2I autoregressive decode, 72-token prompt + 256 image tokens, greedy, hipGraph replay, fp32 weights
    (the reference inference scripts never cast the model: scripts/inference_t2i.py:21-26)."""
    torch.manual_seed(0)
    cfg = StackConfig.omnimamba_1_3b()
    # the reference keeps fp32; bf16 = a model cast by the user; fp8 = bf16 activations with e4m3 in_proj / out_proj in the fused step
    # (omnimamba_amd.quant), --weights f32 --quant fp8 = fp32 activations with them
    quant = "fp8" if args.weights == "fp8" else args.quant
    wdt = torch.bfloat16 if args.weights in ("bf16", "fp8") else torch.float32
    model = OmniMambaLM(cfg, device=dev, dtype=wdt).eval()
    if quant == "fp8":
        from omnimamba_amd.quant import quantize_decode_weights
        quantize_decode_weights(model)
    B, P, new = args.batch, 72, 256
    ids = torch.zeros(B, P, dtype=torch.long, device=dev)
    emb = torch.randn(B, P, cfg.d_model, device=dev, dtype=wdt) * 0.02 + model.backbone.pos_embed[:, :P].to(wdt)
    out = {}
    forms = _ProjectionForms()
    for cg in (True, False) if args.eager_too else (True,):
        with forms:
            decode(ids, emb, model, P + new, top_k=1, task="t2i", cg=cg)      # warm-up (captures the graph)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        seq = decode(ids, emb, model, P + new, top_k=1, task="t2i", cg=cg)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        assert seq.shape == (B, P + new)
        out["graph" if cg else "eager"] = dt
    n_param = sum(p.numel() for p in model.parameters())
    n_bytes = n_param * (2 if wdt == torch.bfloat16 else 4)
    if quant == "fp8":   # the step streams the e4m3 codes and row scales of the projections instead of their master weights
        from omnimamba_amd.quant import decode_weights
        for m in model.modules():
            qw = decode_weights(m) if isinstance(m, torch.nn.Linear) else None
            if qw is not None:
                n_bytes += qw[0].numel() + 4 * qw[1].numel() - m.weight.numel() * m.weight.element_size()
    ms_tok = out["graph"] / new * 1e3
    print(json.dumps({"workload": "OmniMamba-1.3B T2I decode (configs[2])", "batch": B, "prompt": P, "new_tokens": new,
                      "ms_per_token": round(ms_tok, 3), "tokens_per_s": round(B * new / out["graph"], 1),
                      "weights_GBs": round(n_bytes / (ms_tok * 1e-3) / 1e9, 1), "params": n_param,
                      "dtype": "bf16" if wdt == torch.bfloat16 else "f32", "decode_projections": "fp8_e4m3" if quant == "fp8" else None,
                      "projection_forms": forms.sorted(), "eager_ms_per_token": round(out["eager"] / new * 1e3, 3) if "eager" in out else None}), flush=True)


def bench_decode_mmu(args, dev):
    """MMU generation the way scripts/inference_mmu.py runs it: <|mmu|> <|soi|> [729 projected image positions] <|eoi|> <|sot|> + a 47-token
    question = 780 prompt positions (but 51 prompt ids), greedy, hipGraph replay of the step, fp32 weights; 128 new tokens."""
    from omnimamba_amd.omni import OmniMambaPath
    torch.manual_seed(0)
    cfg = StackConfig.omnimamba_1_3b()
    model = OmniMambaPath(cfg, stage="inference", device=dev, dtype=torch.float32)
    B, Q, new = args.batch, 47, 128
    q = torch.randint(0, 50000, (B, Q), device=dev)
    feat = torch.randn(B, 729, cfg.fused_vision_dim, device=dev)
    P = 4 + 729 + Q
    res = {}
    for n in (1, new):
        model.mmu_generate(feat, q, max_length=P + n, cg=True)                # warm-up (captures)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        seq = model.mmu_generate(feat, q, max_length=P + n, cg=True)
        torch.cuda.synchronize()
        res[n] = time.perf_counter() - t0
        assert seq.shape == (B, 4 + Q + n)
    print(json.dumps({"workload": "OmniMamba-1.3B MMU generation (scripts/inference_mmu.py shape)", "batch": B, "prompt_positions": P,
                      "prompt_ids": 4 + Q, "new_tokens": new, "time_to_first_token_ms": round(res[1] * 1e3, 2),
                      "ms_per_token": round((res[new] - res[1]) / (new - 1) * 1e3, 3), "dtype": "f32"}), flush=True)


def bench_train(args, dev, rank, world):
    """configs[3]/[4]-style Stage-2 step: one T2I + one MMU forward, one backward, clip, AdamW; bf16 autocast over fp32
    master weights; DDP over RCCL when world > 1."""
    torch.manual_seed(0)
    L = args.seqlen
    tasks = tuple(args.tasks.split(","))
    cfg = StackConfig.omnimamba_1_3b(t2i_positions=max(L, 329), mmu_positions=max(L, 1500), t2i_task="t2i" in tasks, mmu_task="mmu" in tasks)
    model = OmniMambaPath(cfg, stage=args.stage, device=dev, dtype=torch.float32)
    tc = TrainConfig()
    net = wrap_ddp(model, tc, device_ids=[dev.index]) if world > 1 else None
    step = Stage2Step(model, tc, ddp_model=net)
    batch = synthetic_batch(cfg, args.batch, L, dev, torch.bfloat16, rank=rank, tasks=tasks)
    losses = []
    for _ in range(args.warmup):
        losses.append(step(batch))
    torch.cuda.synchronize()
    if world > 1:
        torch.distributed.barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        losses.append(step(batch))
    torch.cuda.synchronize()
    if world > 1:
        torch.distributed.barrier()
    dt = (time.perf_counter() - t0) / args.steps
    if world > 1:
        t = torch.tensor([dt], device=dev, dtype=torch.float64)
        torch.distributed.all_reduce(t, op=torch.distributed.ReduceOp.MAX)
        dt = t.item()
    if rank == 0:
        trainable = sum(p.numel() for p in model.parameters() if p.requires_grad)
        print(json.dumps({"workload": f"OmniMamba-1.3B step (stage {args.stage}), tasks {tasks} x L={L}", "n_gpus": world,
                          "batch_per_gpu": args.batch, "ms_per_step": round(dt * 1e3, 2),
                          "tokens_per_s": round(world * len(tasks) * args.batch * L / dt, 1), "trainable_params": trainable,
                          "peak_mem_GB": round(torch.cuda.max_memory_allocated() / 1e9, 2), "dtype": "bf16 autocast",
                          "losses": [round(float(x["loss"] if isinstance(x, dict) else x), 4) for x in losses]}), flush=True)


def _mmu_batch_workload(cfg, dev, n_req=32):
    """32 MMU requests: 729 image positions, questions of 8 - 120 ids, answers of 16 - 256 ids set by per-request max_length (random
    weights give no usable EOS)."""
    g = torch.Generator().manual_seed(1)
    qlen = torch.randint(8, 121, (n_req,), generator=g).tolist()
    new = [int(x) for x in torch.linspace(16, 256, n_req)]
    new = [new[i] for i in torch.randperm(n_req, generator=g).tolist()]
    qs = [torch.randint(0, 50000, (1, L), generator=g).to(dev) for L in qlen]
    feats = [torch.randn(1, 729, cfg.fused_vision_dim, generator=g).to(dev) for _ in range(n_req)]
    lens = [4 + 729 + L + n for L, n in zip(qlen, new)]         # decode samples max_length - prompt positions ids (no EOS)
    return feats, qs, lens, new


class _AdmissionClock:
    """Times the admissions of one decode_ragged call from outside the library: batch_decode's _prefill / _prefill_group / _extend are
    wrapped with a device synchronisation on both sides.  seconds: time spent in them (prefill or extend + state copy);
    first_token_s: per request in admission (FIFO) order, seconds from entering the context to the end of its admission, which is when
    its first id can be sampled.  The run it times is slower than an untimed one: do not take tokens / s from it."""

    def __enter__(self):
        from omnimamba_amd import batch_decode as BD
        self.BD, self.real, self.seconds, self.first_token_s = BD, {}, 0.0, []
        self.t_enter = time.perf_counter()
        for name in ("_prefill", "_prefill_group", "_extend"):
            self.real[name] = getattr(BD, name)
            setattr(BD, name, self._timed(name))
        return self

    def _timed(self, name):
        def fn(model, c, slot, *a, **k):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = self.real[name](model, c, slot, *a, **k)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            self.seconds += t1 - t0
            self.first_token_s += [t1 - self.t_enter] * (len(slot) if name == "_prefill_group" else 1)
            return out
        return fn

    def __exit__(self, *exc):
        for name, fn in self.real.items():
            setattr(self.BD, name, fn)


def bench_decode_mmu_batch(args, dev):
    """Continuous batching of MMU requests (omnimamba_amd/batch_decode.py): generated tokens / s of mmu_generate_batch (max_batch 8) against
    the same requests through sequential mmu_generate calls, OmniMamba-1.3B with fp32 weights (as the reference runs it) and with bf16
    weights; every bucket / graph is warmed up first, prefills are part of both timings.
    --prefill-batch / --prefill-bucket: the ragged-prefill options of decode_ragged.  --reps N: the ragged run N times (every time is
    printed: the spread is the point).  One more run under _AdmissionClock gives the time spent in admission (prefill + state copy)
    and the time to the first token of the first and of the last request of the opening burst; that run synchronises around every
    admission and is not one of the timed ones.  --no-sequential: skip the sequential baseline.
    --weights fp8: the bf16 model alone with e4m3 in_proj / out_proj in the fused step; --quant fp8: every dtype of --dtypes with them."""
    cfg = StackConfig.omnimamba_1_3b()
    opts = dict(prefill_batch=args.prefill_batch, prefill_bucket=args.prefill_bucket)
    quant = "fp8" if args.weights == "fp8" else args.quant
    for wdt in [dict(f32=torch.float32, bf16=torch.bfloat16)[d] for d in ("bf16" if args.weights == "fp8" else args.dtypes).split(",")]:
        torch.manual_seed(0)
        model = OmniMambaPath(cfg, stage="inference", device=dev, dtype=wdt)
        if quant == "fp8":
            from omnimamba_amd.quant import quantize_decode_weights
            quantize_decode_weights(model)
        feats, qs, lens, new = _mmu_batch_workload(cfg, dev)
        feats = [f.to(wdt) for f in feats]
        n_tok = sum(new)
        # warm-ups: the sequential step graph at the largest max_length (later calls reuse it), every bucket of the ragged step
        if not args.no_sequential:
            model.mmu_generate(feats[0], qs[0], max_length=max(lens), cg=True)
        with _ProjectionForms() as forms:
            model.mmu_generate_batch(feats, qs, max_length=lens, max_batch=args.max_batch, cg=True, **opts)
        torch.cuda.synchronize()
        seq, t_seq = None, None
        if not args.no_sequential:
            t0 = time.perf_counter()
            seq = [model.mmu_generate(f, q, max_length=L, cg=True) for f, q, L in zip(feats, qs, lens)]
            torch.cuda.synchronize()
            t_seq = time.perf_counter() - t0
        t_rags = []
        for _ in range(max(args.reps, 1)):
            t0 = time.perf_counter()
            rag = model.mmu_generate_batch(feats, qs, max_length=lens, max_batch=args.max_batch, cg=True, **opts)
            torch.cuda.synchronize()
            t_rags.append(time.perf_counter() - t0)
        t_rag = sorted(t_rags)[len(t_rags) // 2]
        with _AdmissionClock() as clk:
            model.mmu_generate_batch(feats, qs, max_length=lens, max_batch=args.max_batch, cg=True, **opts)
        burst = clk.first_token_s[:min(args.max_batch, len(qs))]
        samp = _sampling_variants(args, model, feats, qs, lens, n_tok, opts) if args.sampling in ("mixed", "constrained", "penalties", "guided") else {}
        if args.logprobs is not None:
            samp.update(_logprobs_variant(args, model, feats, qs, lens, n_tok, opts, rag))
        got = [r.shape[1] for r in rag]
        assert got == [4 + q.shape[1] + n for q, n in zip(qs, new)], got
        same = None if seq is None else sum(int(torch.equal(r, s_)) for r, s_ in zip(rag, seq))
        print(json.dumps({"workload": "OmniMamba-1.3B MMU continuous batching", "dtype": "bf16" if wdt == torch.bfloat16 else "f32",
                          "decode_projections": "fp8_e4m3" if quant == "fp8" else None, "projection_forms": forms.sorted(),
                          "requests": len(qs), "generated_tokens": n_tok, "max_batch": args.max_batch, **opts,
                          "sequential_s": None if t_seq is None else round(t_seq, 3), "ragged_s": round(t_rag, 3),
                          "ragged_s_all": [round(t, 3) for t in t_rags],
                          "sequential_tokens_per_s": None if t_seq is None else round(n_tok / t_seq, 1),
                          "ragged_tokens_per_s": round(n_tok / t_rag, 1), "ragged_tokens_per_s_all": [round(n_tok / t, 1) for t in t_rags],
                          "speedup": None if t_seq is None else round(t_seq / t_rag, 2), "requests_with_identical_ids": same,
                          "admission_s": round(clk.seconds, 3), "first_token_first_request_ms": round(burst[0] * 1e3, 1),
                          "first_token_last_of_burst_ms": round(burst[-1] * 1e3, 1), **samp}), flush=True)
        del model
        torch.cuda.empty_cache()


def _sampling_variants(args, model, feats, qs, lens, n_tok, opts):
    """--sampling mixed: the ragged run (same requests, no EOS: the same number of tokens) with (1) top_k = 20 for the whole call through
    the old path (generation.sample: one omk_sample launch per step), (2) top_k = 20 for every request through the row-wise launch
    (sampling=SamplingParams: the cost of the new path alone) and (3) mixed per-request settings -- greedy, top-k 20 with top-p, the
    whole vocabulary behind top-p, top-k 20 with a repetition penalty, the whole vocabulary behind min_p, in turn.  The variants
    alternate, --reps times each (every time is printed); ragged_tokens_per_s of the same line is the greedy run.
    --sampling constrained: (3) against (4) the same mixed requests, every second one with a 4-id allowed set and a logit_bias on 16 ids
    (the edit launch of the row-wise sampler in every draw of the call; the set is the first four of the biased ids, and the merge rule
    of sampling.pack_edits drops the biases outside it: lists of four entries); the ids differ, the number of tokens does not (no EOS).
    --sampling penalties: (3) against (5) the same mixed requests, every one with presence_penalty 0.5 and frequency_penalty 0.3 (every
    draw of the call: omk_penalty_edits + the edit launch while a request has sampled at most 512 ids, a torch-edited copy past that).
    --sampling guided: (3) against the same mixed requests with guides (decode_ragged(guides=...): the masked row-wise launch in every draw
    and a host read of the ids per step) -- (6) every request a sampling.ChoiceGuide over four fixed sequences (no EOS is given to the
    call: a request that has finished its choice goes on emitting the guide's EOS id, so the number of tokens is the same) and (7) every
    request a dense guide that allows a pseudo-random half of the vocabulary, one of 16 precomputed masks in turn.  Fresh guides for every
    run; the time spent inside the guides' mask() and advance() is reported per run (guide_s_all)."""
    from omnimamba_amd.sampling import SamplingParams as SP
    kinds = [SP(), SP(top_k=20, top_p=0.9), SP(top_k=0, top_p=0.9), SP(top_k=20, repetition_penalty=1.3), SP(top_k=0, min_p=0.05)]
    from dataclasses import replace
    mixed = [replace(kinds[i % len(kinds)], seed=1000 + i) for i in range(len(qs))]
    uni = [SP(top_k=20, seed=1000 + i) for i in range(len(qs))]
    runs = {"uniform_top_k20_old_path": dict(top_k=20), "uniform_top_k20_row_wise": dict(sampling=uni), "mixed_row_wise": dict(sampling=mixed)}
    if args.sampling == "constrained":
        V = model.cfg.vocab_size
        cons = [replace(p, allowed_token_ids=[(997 * (i + 1) + 131 * j) % V for j in range(4)],
                        logit_bias={(997 * (i + 1) + 131 * j) % V: 0.25 * j - 2.0 for j in range(16)}) if i % 2 else p for i, p in enumerate(mixed)]
        runs = {"mixed_row_wise": dict(sampling=mixed), "constrained_row_wise": dict(sampling=cons)}
    if args.sampling == "penalties":
        pens = [replace(p, presence_penalty=0.5, frequency_penalty=0.3) for p in mixed]
        runs = {"mixed_row_wise": dict(sampling=mixed), "penalties_row_wise": dict(sampling=pens)}
    guide_s = {}
    if args.sampling == "guided":
        from omnimamba_amd.sampling import ChoiceGuide, pack_token_mask
        V = model.cfg.vocab_size
        spent = [0.0]

        class Timed:      # (the guide's own Python time, apart from the launches)
            def __init__(self, g):
                self.g = g

            def mask(self):
                t0 = time.perf_counter()
                m = self.g.mask()
                spent[0] += time.perf_counter() - t0
                return m

            def advance(self, tok):
                t0 = time.perf_counter()
                self.g.advance(tok)
                spent[0] += time.perf_counter() - t0

        gen = torch.Generator().manual_seed(7)
        dense_masks = [pack_token_mask(torch.randperm(V, generator=gen)[: V // 2].tolist(), V) for _ in range(16)]

        class Dense:
            def __init__(self, i):
                self.n = i

            def mask(self):
                return dense_masks[self.n % 16]

            def advance(self, tok):
                self.n += 1

        choices = lambda i: [[(101 * (i + 1) + 17 * c + 3 * j) % (V - 1) for j in range(2 + 3 * c)] for c in range(4)]
        runs = {"mixed_row_wise": dict(sampling=mixed),
                "guided_choice_row_wise": lambda: dict(sampling=mixed, guides=[Timed(ChoiceGuide(choices(i), V, V - 1)) for i in range(len(qs))]),
                "guided_dense_row_wise": lambda: dict(sampling=mixed, guides=[Timed(Dense(i)) for i in range(len(qs))])}
        guide_s = {k: [] for k in runs if k != "mixed_row_wise"}
    times = {k: [] for k in runs}
    kwargs = lambda kw: kw() if callable(kw) else kw      # (guides are stateful: a fresh set for every run)
    for k, kw in runs.items():       # warm-up: the setting tensors of every bucket, the history buffer
        model.mmu_generate_batch(feats, qs, max_length=lens, max_batch=args.max_batch, cg=True, **opts, **kwargs(kw))
    torch.cuda.synchronize()
    for _ in range(max(args.reps, 1)):
        for k, kw in runs.items():
            kw = kwargs(kw)
            if k in guide_s:
                spent[0] = 0.0
            t0 = time.perf_counter()
            model.mmu_generate_batch(feats, qs, max_length=lens, max_batch=args.max_batch, cg=True, **opts, **kw)
            torch.cuda.synchronize()
            times[k].append(time.perf_counter() - t0)
            if k in guide_s:
                guide_s[k].append(spent[0])
    out = {}
    for k, ts in times.items():
        out[k + "_tokens_per_s"] = round(n_tok / sorted(ts)[len(ts) // 2], 1)
        out[k + "_tokens_per_s_all"] = [round(n_tok / t, 1) for t in ts]
        out[k + "_s_all"] = [round(t, 4) for t in ts]
    for k, ts in guide_s.items():
        out[k + "_guide_s_all"] = [round(t, 4) for t in ts]
    return {"sampling": out}


def _logprobs_variant(args, model, feats, qs, lens, n_tok, opts, rag):
    """--logprobs N: the greedy ragged run with logprobs=N for every request (one token_logprobs launch behind every draw, the records
    assembled at the end) alternating with the same run without, --reps times each (every time is printed).  The ids must be those of
    the run without."""
    kw = dict(max_length=lens, max_batch=args.max_batch, cg=True, **opts)
    ids, recs = model.mmu_generate_batch(feats, qs, logprobs=args.logprobs, **kw)       # warm-up
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(ids, rag)) and all(r.logprob.shape[0] == n for r, n in zip(recs, [o.shape[1] - 4 - q.shape[1] for o, q in zip(ids, qs)]))
    times = {"without": [], "with": []}
    for _ in range(max(args.reps, 1)):
        for k, extra in (("without", {}), ("with", dict(logprobs=args.logprobs))):
            t0 = time.perf_counter()
            model.mmu_generate_batch(feats, qs, **kw, **extra)
            torch.cuda.synchronize()
            times[k].append(time.perf_counter() - t0)
    med = {k: sorted(ts)[len(ts) // 2] for k, ts in times.items()}
    return {"logprobs": {"top_n": args.logprobs, "tokens_per_s": round(n_tok / med["with"], 1),
                         "tokens_per_s_all": [round(n_tok / t, 1) for t in times["with"]],
                         "without_tokens_per_s": round(n_tok / med["without"], 1),
                         "without_tokens_per_s_all": [round(n_tok / t, 1) for t in times["without"]],
                         "ms_per_call": round((med["with"] - med["without"]) * 1e3, 1)}}


def bench_step_index_cost(args, dev):
    """The cost of state_indices on the decode step: the captured bf16 batch-B step of OmniMamba-1.3B with identity slot indices against
    today's captured step without them, replays alternating in blocks of 20 (``--steps`` replays each).  ``--only plain|indexed`` captures
    and replays one of the two (for a kernel-trace run of each)."""
    from omnimamba_amd.batch_decode import _Bucket
    from omnimamba_amd.generation import InferenceParams
    torch.manual_seed(0)
    cfg = StackConfig.omnimamba_1_3b()
    model = OmniMambaLM(cfg, device=dev, dtype=torch.bfloat16).eval()
    B = args.batch
    pool = model.allocate_inference_cache(B, 4096, torch.bfloat16)
    for c, s_ in pool.values():
        c.normal_(std=0.1), s_.normal_(std=0.1)
    model.prepare_decode("mmu")
    graphs = {}
    with torch.inference_mode():
        if args.only in (None, "indexed"):
            bk = _Bucket(model, pool, B, 4096, "mmu", True, None)
            bk.slots.copy_(torch.arange(B, dtype=torch.int32))
            bk.position_ids.fill_(800)
            graphs["indexed"] = bk.graph
        if args.only in (None, "plain"):
            ip = InferenceParams(max_seqlen=4096, max_batch_size=B, seqlen_offset=1, key_value_memory_dict=pool)
            ids, pos = torch.zeros(B, 1, dtype=torch.long, device=dev), torch.full((B, 1), 800, dtype=torch.long, device=dev)
            s = torch.cuda.Stream()
            s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s):
                for _ in range(2):
                    model(ids, None, position_ids=pos, task="mmu", inference_params=ip, num_last_tokens=1)
                s.synchronize()
            torch.cuda.current_stream().wait_stream(s)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                model(ids, None, position_ids=pos, task="mmu", inference_params=ip, num_last_tokens=1)
            graphs["plain"] = g
    for g in graphs.values():
        for _ in range(20):
            g.replay()
    torch.cuda.synchronize()
    times = {k: [] for k in graphs}
    blk = 20
    for _ in range((args.steps + blk - 1) // blk):
        for k, g in graphs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(blk):
                g.replay()
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1) / blk)
    med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
    out = {"workload": "OmniMamba-1.3B captured decode step, bf16 weights", "batch": B, "replays_each": len(next(iter(times.values()))) * blk}
    out.update({f"{k}_ms_median": round(v, 4) for k, v in med.items()})
    out.update({f"{k}_ms_min": round(min(times[k]), 4) for k in times})
    if len(med) == 2:
        out["indexed_over_plain_pct"] = round((med["indexed"] / med["plain"] - 1) * 100, 2)
    print(json.dumps(out), flush=True)


def _time_ms(fn, reps):
    """Median of `reps` event-timed calls after two warm-up calls."""
    for _ in range(2):
        fn()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return sorted(ts)[len(ts) // 2]


def bench_mmu_followup(args, dev):
    """Multi-turn MMU.  (1) Per layer (1.3B shapes: H 64, P 64, N 128, batch 1): omk_selective_state_extend against the chunked scan
    with initial states for T in {1, 8, 32, 64, 128, 256} -- the sweep behind mamba2.EXTEND_SCAN_MAX_T.  (2) Time to the first token of
    turn 2 for --batch conversations (729 image positions, Q1 of 24 ids, A1 of 32 ids, Q2 of --turn2-ids ids, 24 unless given): mmu_continue from the turn-1
    states against re-prefilling the whole conversation with mmu_generate_batch.  fp32 and bf16 weights, eager both ways.
    --extend-batch N > 1: mmu_continue is timed twice, at extend_batch 1 (every conversation extended on its own) and at N (those that
    find a slot together extended by one right-padded pass), and the JSON line names both."""
    from omnimamba_amd.selective_state_update import selective_state_extend
    from omnimamba_amd.ssd_combined import mamba_chunk_scan_combined
    H, P, N = 64, 64, 128
    g = torch.Generator().manual_seed(2)
    for wdt in (torch.float32, torch.bfloat16):
        name = "bf16" if wdt == torch.bfloat16 else "f32"
        A = -(torch.rand(H, generator=g) * 15 + 1).to(dev)
        D, dtb = torch.randn(H, generator=g).to(dev), (torch.randn(H, generator=g) - 2).to(dev)
        rows = []
        with torch.inference_mode():
            for T in (1, 8, 32, 64, 128, 256):
                x = torch.randn(1, T, H, P, generator=g).to(wdt).to(dev)
                dt = torch.randn(1, T, H, generator=g).to(wdt).to(dev)
                Bm, Cm = torch.randn(1, T, 1, N, generator=g).to(wdt).to(dev), torch.randn(1, T, 1, N, generator=g).to(wdt).to(dev)
                st = torch.randn(1, H, P, N, generator=g).to(wdt).to(dev)
                work = st.clone()
                t_ext = _time_ms(lambda: (work.copy_(st), selective_state_extend(work, x, dt, A, Bm, Cm, D=D, dt_bias=dtb, dt_softplus=True)), 50)
                t_copy = _time_ms(lambda: work.copy_(st), 50)
                t_scan = _time_ms(lambda: mamba_chunk_scan_combined(x, dt, A, Bm, Cm, chunk_size=256, D=D, dt_bias=dtb, initial_states=st,
                                                                    dt_softplus=True, return_final_states=True), 50)
                rows.append({"T": T, "extend_us": round((t_ext - t_copy) * 1e3, 1), "chunk_scan_us": round(t_scan * 1e3, 1)})
        print(json.dumps({"workload": "per-layer state extend vs chunked scan with initial states", "dtype": name, "H": H, "P": P, "N": N,
                          "rows": rows}), flush=True)
    cfg = StackConfig.omnimamba_1_3b()
    n = args.batch
    for wdt in (torch.float32, torch.bfloat16):
        torch.manual_seed(0)
        model = OmniMambaPath(cfg, stage="inference", device=dev, dtype=wdt)
        g = torch.Generator().manual_seed(3)
        feats = [torch.randn(1, 729, cfg.fused_vision_dim, generator=g).to(dev).to(wdt) for _ in range(n)]
        q1 = [torch.randint(0, 50000, (1, 24), generator=g).to(dev) for _ in range(n)]
        q2 = [torch.randint(0, 50000, (1, args.turn2_ids), generator=g).to(dev) for _ in range(n)]
        ids1, st1 = model.mmu_generate_batch(feats, q1, max_length=4 + 729 + 24 + 32, max_batch=args.max_batch, cg=False, return_states=True)
        full = [torch.cat([a, i[:, 4 + a.shape[1]:], b], dim=1) for a, i, b in zip(q1, ids1, q2)]
        L2 = [s.seqlen + 1 + b.shape[1] + 1 for s, b in zip(st1, q2)]          # one sampled id: the first token of turn 2

        def cont(extend_batch=1):
            return model.mmu_continue(st1, q2, max_length=L2, max_batch=args.max_batch, cg=False, extend_batch=extend_batch)

        def again():
            return model.mmu_generate_batch(feats, full, max_length=L2, max_batch=args.max_batch, cg=False)
        t_cont = _time_ms(cont, args.steps)
        t_full = _time_ms(again, args.steps)
        same = sum(int(a[0, -1]) == int(b[0, -1]) for a, b in zip(cont()[0], again()))
        grouped = {}
        if args.extend_batch > 1:
            t_grp = _time_ms(lambda: cont(args.extend_batch), args.steps)
            grouped = {"extend_batch": args.extend_batch, "continue_extend_batch_1_ms": round(t_cont, 2),
                       f"continue_extend_batch_{args.extend_batch}_ms": round(t_grp, 2), "extend_batch_speedup": round(t_cont / t_grp, 2),
                       "first_ids_equal_grouped": sum(int(a[0, -1]) == int(b[0, -1]) for a, b in zip(cont(args.extend_batch)[0], cont()[0]))}
        print(json.dumps({"workload": "OmniMamba-1.3B MMU turn 2, time to first token", "dtype": "bf16" if wdt == torch.bfloat16 else "f32",
                          "conversations": n, "max_batch": args.max_batch, "turn2_positions": L2[0] - 1, "turn2_ids": args.turn2_ids,
                          "continue_ms": round(t_cont, 2), "reprefill_ms": round(t_full, 2), "speedup": round(t_full / t_cont, 2),
                          "first_ids_equal": same, **grouped}), flush=True)
        del model
        torch.cuda.empty_cache()


def bench_ragged_prefill(args, dev):
    """Ragged prefill of MMU prompts, per 1.3B layer (the first ResidualBlock) and for the whole stack, eager unless said otherwise:
    ONE prefill of 8 right-padded rows of 741 .. 853 positions (InferenceParams.seq_lens) against the 8 batch-1 prefills at exact length
    it replaces; and a CAPTURED batch-1 prefill of the 896-position bucket holding an 853-position prompt against the eager batch-1
    prefill of that prompt.  Medians of --steps event-timed calls after two warm-up calls."""
    from omnimamba_amd.generation import InferenceParams
    cfg = StackConfig.omnimamba_1_3b()
    lens = [int(x) for x in torch.linspace(741, 853, 8)]
    for wdt in [dict(f32=torch.float32, bf16=torch.bfloat16)[d] for d in args.dtypes.split(",")]:
        torch.manual_seed(0)
        model = OmniMambaLM(cfg, device=dev, dtype=wdt).eval()
        blk = model.backbone.layers[0]
        if hasattr(blk.mixer.in_proj, "task_types"):
            model.backbone.set_lora_mode("mmu")
        embs = [torch.randn(1, n, cfg.d_model, device=dev, dtype=wdt) * 0.02 for n in lens]
        buf = torch.zeros(8, max(lens), cfg.d_model, device=dev, dtype=wdt)
        for j, e in enumerate(embs):
            buf[j, :lens[j]] = e[0]
        lens_t = torch.tensor(lens, dtype=torch.int32, device=dev)
        bucket = torch.zeros(1, 896, cfg.d_model, device=dev, dtype=wdt)
        bucket[:, :lens[-1]] = embs[-1]
        one = torch.tensor([lens[-1]], dtype=torch.int32, device=dev)
        row = {"workload": "ragged prefill of MMU prompts, OmniMamba-1.3B", "dtype": "bf16" if wdt == torch.bfloat16 else "f32", "lens": lens}
        with torch.inference_mode():
            for scope in ("layer", "stack"):
                if scope == "layer":
                    cache = lambda b: {0: blk.allocate_inference_cache(b, 0, dtype=wdt)}
                    run = lambda x, ip: blk(x, None, inference_params=ip)[0]
                else:
                    cache = lambda b: model.allocate_inference_cache(b, 1024, wdt)
                    run = lambda x, ip: model(None, x, position_ids=None, task="mmu", inference_params=ip, num_last_tokens=1).mmu_logits
                ip8 = InferenceParams(max_seqlen=1024, max_batch_size=8, key_value_memory_dict=cache(8), seq_lens=lens_t)
                ip1 = InferenceParams(max_seqlen=1024, max_batch_size=1, key_value_memory_dict=cache(1))
                ipb = InferenceParams(max_seqlen=1024, max_batch_size=1, key_value_memory_dict=cache(1), seq_lens=one)
                row[f"{scope}_one_prefill_of_8_rows_ms"] = round(_time_ms(lambda: run(buf, ip8), args.steps), 3)
                row[f"{scope}_8_batch1_prefills_ms"] = round(_time_ms(lambda: [run(e, ip1) for e in embs], args.steps), 3)
                row[f"{scope}_eager_batch1_853_ms"] = round(_time_ms(lambda: run(embs[-1], ip1), args.steps), 3)
                row[f"{scope}_eager_bucket_896_ms"] = round(_time_ms(lambda: run(bucket, ipb), args.steps), 3)
                side = torch.cuda.Stream()
                side.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(side):
                    for _ in range(2):
                        run(bucket, ipb)
                    side.synchronize()
                torch.cuda.current_stream().wait_stream(side)
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph):
                    keep = run(bucket, ipb)  # noqa: F841
                row[f"{scope}_captured_bucket_896_ms"] = round(_time_ms(graph.replay, args.steps), 3)
                del graph, keep
        print(json.dumps(row), flush=True)
        del model
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["decode", "train", "decode_mmu_batch", "step_index_cost", "mmu_followup", "ragged_prefill"])
    ap.add_argument("--max-batch", type=int, default=8, help="decode_mmu_batch: slots of the ragged decoder")
    ap.add_argument("--prefill-batch", type=int, default=1, help="decode_mmu_batch: requests admitted by one right-padded prefill (1 = off)")
    ap.add_argument("--prefill-bucket", type=int, default=0, help="decode_mmu_batch: length bucket of the captured prefill graphs (0 = off; 128 for MMU)")
    ap.add_argument("--turn2-ids", type=int, default=24, help="mmu_followup: ids of the second question (with the pending id: up to mamba2.EXTEND_SCAN_MAX_T "
                                                                  "positions take the extend kernel, more the chunked scan)")
    ap.add_argument("--extend-batch", type=int, default=1, help="mmu_followup: also time mmu_continue with this many turns per grouped extend (1 = off)")
    ap.add_argument("--sampling", choices=["greedy", "mixed", "constrained", "penalties", "guided"], default="greedy",
                    help="decode_mmu_batch: mixed = also time uniform top_k 20 (old path) and per-request settings (row-wise launch); "
                         "constrained = the mixed settings against the same with an allowed set and a logit_bias on every second request; "
                         "penalties = the mixed settings against the same with a presence and a frequency penalty on every request; "
                         "guided = the mixed settings against the same with a ChoiceGuide / a dense pseudo-random guide on every request")
    ap.add_argument("--logprobs", type=int, default=None, help="decode_mmu_batch: also time the greedy run with logprobs=N (token_logprobs behind every draw)")
    ap.add_argument("--reps", type=int, default=1, help="decode_mmu_batch: timed repetitions of the ragged run")
    ap.add_argument("--dtypes", default="f32,bf16", help="decode_mmu_batch: weight dtypes to run")
    ap.add_argument("--no-sequential", action="store_true", help="decode_mmu_batch: skip the sequential mmu_generate baseline")
    ap.add_argument("--only", choices=["plain", "indexed"], default=None, help="step_index_cost: capture and replay one step only")
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--seqlen", type=int, default=2048)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)   # one warm-up step is not enough: optimizer state and GEMM heuristics settle in the second
    ap.add_argument("--stage", default="finetune")
    ap.add_argument("--tasks", default="t2i,mmu", help="t2i,mmu (stage 2) or mmu (stage-1 MMU pretrain, BASELINE configs[3])")
    ap.add_argument("--eager-too", action="store_true")
    ap.add_argument("--task", default="t2i", choices=["t2i", "mmu"], help="decode: T2I (configs[2]) or the MMU generation of scripts/inference_mmu.py")
    ap.add_argument("--weights", choices=["f32", "bf16", "fp8"], default="f32",
                    help="decode / decode_mmu_batch: fp8 = bf16 activations with e4m3 in_proj / out_proj in the fused decode step")
    ap.add_argument("--quant", choices=["none", "fp8"], default="none",
                    help="decode / decode_mmu_batch: e4m3 in_proj / out_proj under the chosen --weights / --dtypes (f32: fp32 activations)")
    args = ap.parse_args()
    rank, local, world = init_distributed()
    dev = torch.device("cuda", local)
    torch.cuda.set_device(dev)
    if args.what == "decode":
        (bench_decode_mmu if args.task == "mmu" else bench_decode)(args, dev)
    elif args.what == "decode_mmu_batch":
        bench_decode_mmu_batch(args, dev)
    elif args.what == "ragged_prefill":
        bench_ragged_prefill(args, dev)
    elif args.what == "step_index_cost":
        bench_step_index_cost(args, dev)
    elif args.what == "mmu_followup":
        bench_mmu_followup(args, dev)
    else:
        bench_train(args, dev, rank, world)


if __name__ == "__main__":
    main()
