"""Launches for a kernel trace of the row-wise sampler with per-row logit edits (profiles/sample_rows_edits.txt).

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o NAME -- python tools/bench_sample_rows_edits.py VARIANT
    python tools/bench_sample_rows_edits.py summarise DIR/**/NAME_kernel_trace.csv

VARIANT, on --rows x --vocab fp32 logits (randn x 2), the same settings in every row:
  plain      no penalty, no edits (the plain instantiation)
  penalty    penalty 1.3 and a 300-id history per row (the penalty instantiation)
  allow4     the edit instantiation: an allow-only list of 4 ids per row
  bias16     ... a logit_bias on 16 ids per row
  biasmax    ... a logit_bias on MAX_EDITS ids per row
  bias16pen  ... bias16 with the penalty and the 300-id history
  torch      what a caller has without the edit launch: apply_logit_edits(logits, bias16) on a copy, then the plain launch
Every process runs --warmup + --timed calls with top_k 20 / top_p 0.9 and then as many with top_k 0 / top_p 0.9 (the whole vocabulary).
The inputs are made on the host and copied: every kernel of the trace but the runtime's copy kernels belongs to one of the calls.
summarise: kernel time per call (the sum of End - Start over the kernels of a call, launch gaps not counted) of the last --timed calls of
each half: median, min, p90 in us."""
import argparse
import csv
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

VARIANTS = ["plain", "penalty", "allow4", "bias16", "biasmax", "bias16pen", "torch"]


def launches(args):
    import torch
    from omnimamba_amd.sampling import MAX_EDITS, SamplingParams as SP, apply_logit_edits, pack_edits, pack_rows, sample_rows, sample_rows_form
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    n, V, what = args.rows, args.vocab, args.what
    logits = (torch.randn(n, V, generator=g) * 2.0).to(dev)
    history = torch.randint(0, V, (n, 300), generator=g).to(dev)
    hist = dict(history=history, history_lens=torch.full((n,), 300, dtype=torch.int32).to(dev))
    ids = lambda b, k: [(7919 * (b + 1) + 6151 * j) % V for j in range(k)]
    if what == "allow4":
        con = [dict(allowed_token_ids=ids(b, 4)) for b in range(n)]
    else:
        k = MAX_EDITS if what == "biasmax" else 16
        con = [dict(logit_bias={i: 0.01 * (j % 400) - 2.0 for j, i in enumerate(ids(b, k))}) for b in range(n)]
    want = {"plain": 0, "penalty": 1, "torch": 0}.get(what, 2)
    torch.cuda.synchronize()
    for top_k in (20, 0):
        params = [SP(top_k=top_k, top_p=0.9, seed=100 + b, repetition_penalty=1.3 if what in ("penalty", "bias16pen") else 1.0, **con[b]) for b in range(n)]
        pk = pack_rows(params, dev)
        pen = pk.pop("penalty")
        ed = pack_edits(params, dev)
        kw = dict(pk)
        if what in ("penalty", "bias16pen"):
            kw.update(hist, penalty=pen)
        if want == 2:
            kw.update(ed)
        assert sample_rows_form(logits, **kw) == want
        torch.cuda.synchronize()
        for _ in range(args.warmup + args.timed):
            if what == "torch":
                sample_rows(apply_logit_edits(logits, **ed), **kw)
            else:
                sample_rows(logits, **kw)
        torch.cuda.synchronize()


def summarise(args):
    rows = [r for r in csv.DictReader(open(args.trace)) if not r["Kernel_Name"].startswith("__amd_rocclr_")]   # (the runtime's copy kernels: the inputs)
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    calls = 2 * (args.warmup + args.timed)
    per = len(rows) // calls
    assert per * calls == len(rows), (len(rows), calls)
    out = {"trace": args.trace, "kernels_per_call": per}
    for half, name in enumerate(("top_k20", "whole_vocab")):
        first = half * (calls // 2) + args.warmup
        t = sorted(sum(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) for r in rows[c * per:(c + 1) * per]) / 1e3 for c in range(first, first + args.timed))
        out[name] = {"median_us": round(t[len(t) // 2], 2), "min_us": round(t[0], 2), "p90_us": round(t[int(0.9 * len(t))], 2)}
    out["kernels"] = sorted({r["Kernel_Name"][:70] for r in rows[-per:]})
    print(json.dumps(out))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=VARIANTS + ["summarise"])
    ap.add_argument("trace", nargs="?")
    ap.add_argument("--rows", type=int, default=8)
    ap.add_argument("--vocab", type=int, default=50288)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--timed", type=int, default=120)
    a = ap.parse_args()
    summarise(a) if a.what == "summarise" else launches(a)
