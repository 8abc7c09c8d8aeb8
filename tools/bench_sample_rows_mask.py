"""Launches for a kernel trace of the masked row-wise sampler (profiles/sample_rows_mask.txt).

    rocprofv3 --kernel-trace --output-format csv -d DIR -o NAME -- python tools/bench_sample_rows_mask.py run
    python tools/bench_sample_rows_mask.py summarise DIR/**/NAME_kernel_trace.csv

run: ONE process, every variant in turn and the whole round --reps times (interleaved: all numbers of a table come from one session), on
--rows x --vocab fp32 logits (randn x 2), the same settings in every row.  In front of every segment one token_logprobs launch, which no
variant uses: the separator `summarise` cuts the trace at.  A segment is --warmup + --timed calls; the first half of a round runs with
top_k 20 / top_p 0.9, the second with top_k 0 / top_p 0.9 (the whole vocabulary).  The variants:
  plain          omk_sample_rows, no id map
  edit4          the edit launch with a 4-id allowed set (what a caller had for "one of these tokens")
  mask_ones      form 3, an all-ones mask: what the mask costs where it cuts nothing
  mask_half      form 3, a ~50 % mask
  mask_4tok      form 3, four tokens allowed
  hist_mask      form 4, a 300-id history with a repetition penalty of 1.3 and the ~50 % mask
  copy_half      what mask_ones / mask_half replace: apply_token_mask on a copy + the plain launch
  copy_4tok      ... for the 4-token mask
  copy_hist      what hist_mask replaces: apply_logit_edits (the penalty) + apply_token_mask on a copy + the plain launch
summarise: kernel time per call (the sum of End - Start over the kernels of a call, launch gaps not counted) of the last --timed calls of
every segment: per variant and setting the median of each repetition, and their min - max; kernels per call."""
import argparse
import csv
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

VARIANTS = ["plain", "edit4", "mask_ones", "mask_half", "mask_4tok", "hist_mask", "copy_half", "copy_4tok", "copy_hist"]
SETTINGS = ["top_k20", "whole_vocab"]


def run(args):
    import torch
    from omnimamba_amd import _capi as K
    from omnimamba_amd.sampling import (SamplingParams as SP, apply_logit_edits, apply_token_mask, pack_edits, pack_rows, pack_token_mask, sample_rows,
                                        sample_rows_form, token_logprobs)
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    n, V = args.rows, args.vocab
    logits = (torch.randn(n, V, generator=g) * 2.0).to(dev)
    ids = torch.zeros(n, dtype=torch.int64, device=dev)
    history = torch.randint(0, V, (n, 300), generator=g).to(dev)
    lens = torch.full((n,), 300, dtype=torch.int32).to(dev)
    four = [[int(t) for t in torch.randperm(V, generator=g)[:4]] for _ in range(n)]
    ones = torch.full((n, (V + 31) // 32), -1, dtype=torch.int32, device=dev)
    half = torch.stack([pack_token_mask(torch.randperm(V, generator=g)[: V // 2].tolist(), V) for _ in range(n)]).to(dev)
    tok4 = torch.stack([pack_token_mask(f, V) for f in four]).to(dev)
    allow4 = pack_edits([SP(allowed_token_ids=f) for f in four], dev)
    pen = torch.full((n,), 1.3, device=dev)
    rep = dict(penalty=pen, history=history, history_lens=lens)
    torch.cuda.synchronize()
    for _ in range(args.reps):
        for top_k in (20, 0):
            pk = pack_rows([SP(top_k=top_k, top_p=0.9, seed=100 + b) for b in range(n)], dev)
            pk.pop("penalty")
            assert sample_rows_form(logits, **pk, **allow4) == K.SAMPLE_ROWS_EDIT and sample_rows_form(logits, **pk, token_mask=half) == K.SAMPLE_ROWS_MASK
            assert sample_rows_form(logits, **pk, **rep, token_mask=half) == K.SAMPLE_ROWS_EDIT_MASK
            calls = {
                "plain": lambda: sample_rows(logits, **pk),
                "edit4": lambda: sample_rows(logits, **pk, **allow4),
                "mask_ones": lambda: sample_rows(logits, **pk, token_mask=ones),
                "mask_half": lambda: sample_rows(logits, **pk, token_mask=half),
                "mask_4tok": lambda: sample_rows(logits, **pk, token_mask=tok4),
                "hist_mask": lambda: sample_rows(logits, **pk, **rep, token_mask=half),
                "copy_half": lambda: sample_rows(apply_token_mask(logits, half), **pk),
                "copy_4tok": lambda: sample_rows(apply_token_mask(logits, tok4), **pk),
                "copy_hist": lambda: sample_rows(apply_token_mask(apply_logit_edits(logits, **rep), half), **pk),
            }
            for name in VARIANTS:
                token_logprobs(logits, ids)        # the separator
                for _ in range(args.warmup + args.timed):
                    calls[name]()
                torch.cuda.synchronize()


def summarise(args):
    rows = [r for r in csv.DictReader(open(args.trace)) if not r["Kernel_Name"].startswith("__amd_rocclr_")]   # (the runtime's copy kernels: the inputs)
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    cuts = [i for i, r in enumerate(rows) if "token_logprobs" in r["Kernel_Name"]]
    assert len(cuts) == args.reps * len(SETTINGS) * len(VARIANTS), (len(cuts), "separators")
    dur = lambda r: (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
    calls = args.warmup + args.timed
    med = {}
    per_call = {}
    for s, c in enumerate(cuts):
        seg = rows[c + 1: cuts[s + 1] if s + 1 < len(cuts) else len(rows)]
        name, setting = VARIANTS[s % len(VARIANTS)], SETTINGS[(s // len(VARIANTS)) % len(SETTINGS)]
        per = len(seg) // calls
        assert per * calls == len(seg), (name, setting, len(seg), calls)
        t = sorted(sum(dur(r) for r in seg[k * per:(k + 1) * per]) for k in range(args.warmup, calls))
        med.setdefault((name, setting), []).append(round(t[len(t) // 2], 2))
        per_call[name] = per
    out = {"trace": args.trace, "timed_calls": args.timed, "kernels_per_call": per_call}
    for setting in SETTINGS:
        out[setting] = {name: {"median_us_per_rep": med[(name, setting)], "min_us": min(med[(name, setting)]), "max_us": max(med[(name, setting)])}
                        for name in VARIANTS}
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["run", "summarise"])
    ap.add_argument("trace", nargs="?")
    ap.add_argument("--rows", type=int, default=8)
    ap.add_argument("--vocab", type=int, default=50288)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--timed", type=int, default=100)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    summarise(a) if a.what == "summarise" else run(a)
