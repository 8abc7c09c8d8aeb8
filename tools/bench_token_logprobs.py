"""Launches for a kernel trace of sampling.token_logprobs and of the torch composition it replaces (profiles/token_logprobs.txt).

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o NAME -- python tools/bench_token_logprobs.py new   --top-n 5
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o NAME -- python tools/bench_token_logprobs.py torch --top-n 5
    python tools/bench_token_logprobs.py summarise DIR/**/NAME_kernel_trace.csv --calls 130 --timed 120

new:   --warmup + --timed calls of token_logprobs(logits, ids, top_n=N) on --rows x --vocab fp32 logits (randn x 2).
torch: the same number of calls of what a caller has without the kernel: log_softmax(logits.float(), -1), gather of the ids, topk(N)
       of the log-probabilities (N > 0), and the rank as a compare-and-sum (value greater, or equal with a smaller index).
The inputs are made on the host and copied: every kernel of the trace but the runtime's copy kernels belongs to one of the calls, the same number to each.
summarise: kernel time per call (the sum of End - Start over the kernels of a call, launch gaps not counted) of the last --timed calls:
median, min, p90 in us, and the kernels of one call."""
import argparse
import csv
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def torch_chain(logits, ids, top_n, idx):
    import torch
    lp = torch.log_softmax(logits.float(), -1)
    chosen = lp.gather(1, ids[:, None])
    top = torch.topk(lp, top_n, dim=-1) if top_n > 0 else None
    x = logits.gather(1, ids[:, None])
    rank = ((logits > x) | ((logits == x) & (idx < ids[:, None]))).sum(-1) + 1
    return chosen, top, rank


def launches(args):
    import torch
    from omnimamba_amd.sampling import token_logprobs
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    logits = (torch.randn(args.rows, args.vocab, generator=g) * 2.0).to(dev)
    ids = torch.randint(0, args.vocab, (args.rows,), generator=g).to(dev)
    idx = torch.arange(args.vocab)[None].to(dev)          # (the index row of the rank's tie-break: made once, not part of a call)
    torch.cuda.synchronize()
    for _ in range(args.warmup + args.timed):
        if args.what == "new":
            token_logprobs(logits, ids, top_n=args.top_n)
        else:
            torch_chain(logits, ids, args.top_n, idx)
    torch.cuda.synchronize()


def summarise(args):
    rows = [r for r in csv.DictReader(open(args.trace)) if not r["Kernel_Name"].startswith("__amd_rocclr_")]   # (the runtime's copy kernels: the inputs)
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    per = len(rows) // args.calls
    assert per * args.calls == len(rows), (len(rows), args.calls)
    t = sorted(sum(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) for r in rows[c * per:(c + 1) * per]) / 1e3
               for c in range(args.calls - args.timed, args.calls))
    print(json.dumps({"trace": os.path.basename(args.trace), "kernels_per_call": per, "median_us": round(t[len(t) // 2], 2), "min_us": round(t[0], 2),
                      "p90_us": round(t[int(0.9 * len(t))], 2), "kernels": [r["Kernel_Name"][:60] for r in rows[-per:]]}))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["new", "torch", "summarise"])
    ap.add_argument("trace", nargs="?")
    ap.add_argument("--top-n", type=int, default=5)
    ap.add_argument("--rows", type=int, default=8)
    ap.add_argument("--vocab", type=int, default=50288)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--timed", type=int, default=120)
    ap.add_argument("--calls", type=int, default=130)
    a = ap.parse_args()
    summarise(a) if a.what == "summarise" else launches(a)
