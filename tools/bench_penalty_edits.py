"""Launches for a kernel trace of the presence / frequency penalties (profiles/penalty_edits.txt).

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o NAME -- python tools/bench_penalty_edits.py VARIANT --counted K
    python tools/bench_penalty_edits.py summarise DIR/**/NAME_kernel_trace.csv

VARIANT, on --rows x --vocab fp32 logits (randn x 2), the same settings in every row, a history of 300 prompt ids and --counted sampled
ids per row (random tokens: almost all distinct), frequency 0.5 and presence 0.5, no repetition penalty, no user list:
  pair   sampling.sample_rows(frequency=, presence=, count_start=, count_max=K, merged=static buffers): omk_penalty_edits, then the edit
         launch of omk_sample_rows -- two kernels
  copy   what a caller has without them: apply_logit_edits(..., frequency=, presence=, count_start=) on a copy, then the plain launch
Every process runs --warmup + --timed calls with top_k 20 / top_p 0.9 and then as many with top_k 0 / top_p 0.9 (the whole vocabulary).
summarise: kernel time per call (the sum of End - Start over the kernels of a call, launch gaps not counted) of the last --timed calls of
each half: median, min, p90 in us; for `pair` also the median of the penalty_edits kernel alone."""
import argparse
import csv
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def launches(args):
    import torch
    from omnimamba_amd import _capi as K
    from omnimamba_amd.sampling import SamplingParams as SP, apply_logit_edits, pack_rows, penalty_edits, sample_rows, sample_rows_form
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    n, V, k = args.rows, args.vocab, args.counted
    logits = (torch.randn(n, V, generator=g) * 2.0).to(dev)
    history = torch.randint(0, V, (n, 300 + k), generator=g).to(dev)
    lens = torch.full((n,), 300 + k, dtype=torch.int32).to(dev)
    start = torch.full((n,), 300, dtype=torch.int32).to(dev)
    freq, pres = torch.full((n,), 0.5).to(dev), torch.full((n,), 0.5).to(dev)
    w = 1
    while w < k:
        w *= 2
    bufs = penalty_edits(history, lens, start, freq, pres, V, out_cap=w)
    torch.cuda.synchronize()
    for top_k in (20, 0):
        pk = pack_rows([SP(top_k=top_k, top_p=0.9, seed=100 + b) for b in range(n)], dev)
        pk.pop("penalty")
        assert sample_rows_form(logits, **pk, **bufs) == K.SAMPLE_ROWS_EDIT
        torch.cuda.synchronize()
        for _ in range(args.warmup + args.timed):
            if args.what == "copy":
                sample_rows(apply_logit_edits(logits, history=history, history_lens=lens, frequency=freq, presence=pres, count_start=start), **pk)
            else:
                sample_rows(logits, **pk, history=history, history_lens=lens, frequency=freq, presence=pres, count_start=start, count_max=k, merged=bufs)
        torch.cuda.synchronize()


def summarise(args):
    rows = [r for r in csv.DictReader(open(args.trace)) if not r["Kernel_Name"].startswith("__amd_rocclr_")]   # (the runtime's copy kernels: the inputs)
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    first_call = next(i for i, r in enumerate(rows) if "sample_rows_kernel" in r["Kernel_Name"])             # (in front: the set-up launch of the buffers)
    lead = [i for i, r in enumerate(rows[:first_call]) if "penalty_edits_kernel" in r["Kernel_Name"]]
    rows = rows[lead[0] + 1:]
    calls = 2 * (args.warmup + args.timed)
    per = len(rows) // calls
    assert per * calls == len(rows), (len(rows), calls)
    dur = lambda r: (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
    out = {"trace": args.trace, "kernels_per_call": per}
    for half, name in enumerate(("top_k20", "whole_vocab")):
        first = half * (calls // 2) + args.warmup
        t = sorted(sum(dur(r) for r in rows[c * per:(c + 1) * per]) for c in range(first, first + args.timed))
        out[name] = {"median_us": round(t[len(t) // 2], 2), "min_us": round(t[0], 2), "p90_us": round(t[int(0.9 * len(t))], 2)}
        pe = sorted(dur(r) for c in range(first, first + args.timed) for r in rows[c * per:(c + 1) * per] if "penalty_edits_kernel" in r["Kernel_Name"])
        if pe:
            out[name]["penalty_edits_median_us"] = round(pe[len(pe) // 2], 2)
    out["kernels"] = sorted({r["Kernel_Name"][:70] for r in rows[-per:]})
    print(json.dumps(out))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["pair", "copy", "summarise"])
    ap.add_argument("trace", nargs="?")
    ap.add_argument("--counted", type=int, default=128)
    ap.add_argument("--rows", type=int, default=8)
    ap.add_argument("--vocab", type=int, default=50288)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--timed", type=int, default=120)
    a = ap.parse_args()
    summarise(a) if a.what == "summarise" else launches(a)
