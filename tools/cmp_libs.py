"""Developer tool: do several builds of the library compute the SAME bits on the scan (forward with final state, training forward + backward)?
usage: python tools/cmp_libs.py [--selscan] tag=lib.so[:ENV=V,...] ...   (first = reference; empty path = the product library)
--selscan: the Mamba-1 selective scan instead -- forward with last state and pass / tile states, then backward, on the smallest row
of tests/test_selscan_slices.py for every distinct kernel string and on the shapes tools/bench_selscan.py times."""
import os
import subprocess
import sys
import tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CODE = r'''
import os, sys, torch
sys.path.insert(0, %r)
import omnimamba_amd._lib as LB
if os.environ.get("AB_LIB"):
    LB.LIB_PATH = os.environ["AB_LIB"]
    LB._LIB = LB.load(LB.LIB_PATH)
import omnimamba_amd.ssd_combined as S
dev = torch.device("cuda:0")
out = {}
for (B, L, H) in [(2, 1000, 8), (1, 2100, 4), (8, 300, 64)]:
    torch.manual_seed(B * 1000 + L)
    P, N, G = 64, 128, 1
    x = torch.randn(B, L, H, P, device=dev).bfloat16(); Bm = torch.randn(B, L, G, N, device=dev).bfloat16(); Cm = torch.randn(B, L, G, N, device=dev).bfloat16()
    dt = (torch.randn(B, L, H, device=dev) * 0.5).bfloat16(); A = -(torch.rand(H, device=dev) * 15 + 1); D = torch.ones(H, device=dev)
    dtb = torch.randn(H, device=dev) * 0.5 - 3
    y, _, fin = S.ssd_scan_fwd(x, dt, A, Bm, Cm, D=D, dt_bias=dtb, dt_softplus=True, return_final_states=True)
    out[f"y{B}x{L}"] = y.cpu(); out[f"fin{B}x{L}"] = fin.cpu()
    lv = [t.clone().requires_grad_() for t in (x, dt, A, Bm, Cm, D, dtb)]
    yy = S.mamba_chunk_scan_combined(lv[0], lv[1], lv[2], lv[3], lv[4], 256, D=lv[5], dt_bias=lv[6], dt_softplus=True)
    yy.backward(torch.ones_like(yy))
    out[f"yt{B}x{L}"] = yy.detach().cpu()
    for n, t in zip(["dx", "ddt", "dA", "dB", "dC", "dD", "ddtb"], lv):
        out[f"{n}{B}x{L}"] = t.grad.cpu()
torch.save(out, os.environ["AB_OUT"])
''' % ROOT
# the selective scan: tensors above 16 MB travel as their SHA-256 (they are required bit-equal; the atomic sums are all small)
CODE_SELSCAN = r'''
import hashlib, os, sys, torch
sys.path[:0] = [%r, %r]
import omnimamba_amd._lib as LB
if os.environ.get("AB_LIB"):
    LB.LIB_PATH = os.environ["AB_LIB"]
    LB._LIB = LB.load(LB.LIB_PATH)
import test_selscan_slices as TS
dev, lib = torch.device("cuda:0"), LB.get_lib()
out = {}
def keep(key, t):
    if t is not None:
        t = t.detach().contiguous().cpu()
        out[key] = t if t.numel() * t.element_size() <= (16 << 20) else hashlib.sha256(t.view(torch.uint8).numpy().tobytes()).hexdigest()
def run(tag, r, src):
    torch.manual_seed(1)
    g = torch.randn(src[0].shape).to(src[0].dtype)
    o, last, grads, kf, kb, states = TS._launch(r, src, g, dev, lib)
    print(f"  {tag}: {kf} | {kb}", flush=True)
    for n, t in [("out", o), ("last_state", last), ("states", states)] + [("d" + n, t) for n, t in zip(TS.NAMES, grads)]:
        keep(f"{tag}/{n}", t)
size = lambda k: (TS.ROWS[k]["batch"] * TS.ROWS[k]["D"] * TS.ROWS[k]["L"] * TS.ROWS[k]["N"], k)
picked = {}
for k in sorted(TS.ROWS, key=size):
    for f in ("fwd", "bwd", "twin"):
        if TS.ROWS[k][f]:
            picked.setdefault(TS.ROWS[k][f], (k, f))
for k in sorted({k for k, _ in picked.values()}, key=size):
    r = TS.ROWS[k]
    os.environ.update(r["env"] or {})
    os.environ.pop(TS.NO_PS, None)
    src = TS._inputs(r)
    run(k, r, src)
    if (k, "twin") in picked.values():
        os.environ[TS.NO_PS] = "1"
        run(k + "/twin", r, src)
        del os.environ[TS.NO_PS]
    for e in r["env"] or {}:
        del os.environ[e]
from tools.bench_selscan import inputs      # the timed shapes, as that tool builds them
for dtype in (torch.float32, torch.bfloat16):
    for bld in (False, True):
        for Bsz in (2, 16, 64):
            run(f"bench-{str(dtype)[6:]}-{'bld' if bld else 'bdl'}-B{Bsz}", dict(bwd=True, softplus=True), list(inputs(Bsz, 768, dtype, bld, "cpu")))
torch.save(out, os.environ["AB_OUT"])
''' % (ROOT, os.path.join(ROOT, "tests"))
ARGS = [a for a in sys.argv[1:] if a != "--selscan"]
SELSCAN = len(ARGS) < len(sys.argv) - 1
# sums formed with float atomics: equal to rounding
LOOSE = ("dA", "dB", "dC", "dD", "ddelta_bias") if SELSCAN else ("dA", "dD", "ddtb", "ddt")
specs = []
for a in ARGS:
    tag, rest = a.split("=", 1)
    path, _, envs = rest.partition(":")
    specs.append((tag, os.path.abspath(path) if path else "", dict(e.split("=", 1) for e in envs.split(",") if e)))
import torch
ref = None
with tempfile.TemporaryDirectory() as td:
    for tag, lib, env in specs:
        f = os.path.join(td, tag + ".pt")
        subprocess.run([sys.executable, "-c", CODE_SELSCAN if SELSCAN else CODE], env=dict(os.environ, AB_LIB=lib, AB_OUT=f, **env), check=True)
        cur = torch.load(f)
        if ref is None:
            ref = cur
            print(f"{tag}: reference ({len(cur)} tensors)")
            continue
        bad = []
        for k in ref:
            if isinstance(ref[k], str):
                if ref[k] != cur.get(k):
                    bad.append((k, "sha256"))
            elif k not in cur or not torch.equal(ref[k], cur[k]):
                e = ((ref[k].double() - cur[k].double()).norm() / ref[k].double().norm().clamp_min(1e-30)).item() if k in cur else float("inf")
                if not (k.rsplit("/", 1)[-1].startswith(LOOSE) and e < 1e-5):
                    bad.append((k, e))
        print(f"{tag}: " + ("bit-identical" if not bad else f"DIFFERENT {bad}"), flush=True)
