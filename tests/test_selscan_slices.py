"""Mamba-1 selective scan: every kernel instantiation against autograd of the fp64 recurrence, per slice (tolerances.slice_check).

One table drives one forward + backward test.  A row holds the shape, the layout, the dtypes, the test hooks and the exact
omk_ssd_last_kernels() string after the forward and after the backward: both are asserted on the emulator and on the MI355X, so a number
in this file belongs to the kernel that made it (tests/test_selscan_dispatch.py pins the same strings without numbers;
test_every_dispatched_kernel_has_numbers compares the two sets).

The reference is oracle.selective_scan_ref(..., compute_dtype=float64) under autograd, fed the very bf16 / fp32 tensors the kernel reads,
cast to double before the call.  The bound of a slice is tolerances.op_bound on that slice: 1.1 sqrt(q^2 + 1e-4^2) with q the one rounding
of the exact slice to the output dtype (0 for the fp32 sums dA, dD, ddelta_bias, last_state and for constant dB / dC).  Where the forward
hands pass states (in front of every 512-token pass) or tile states (in front of every 16-token tile) to the backward, each is checked
the same way against the fp64 last state of the prefix in front of it, and the gradients of the backward that was handed none (its own
state-only pass / forward sweep) must equal the first ones to 1e-6 per slice.

Inputs.  The upstream gradient is g = 0.3 noise + k / rms(k) + 2 J / rms(J) with k = d out / d D and J = d out / d delta_bias of every
(batch, channel, token), normalised per (batch, channel) row: the per-element outputs dD = sum g k and ddelta_bias = sum g J are then sums with a
mean, not differences of noise of which 8 % would land under a tenth of their RMS.  ddelta of a channel scales with its dt and dA with
dt^2, so the channels of one row draw dt from a window of half a decade (`dt`): with two decades in one row a quarter of the ddelta rows
would be judged on the scale of the others.  Every row asserts that at most 5 % of the slices of any output met the floor of
slice_check; the seed of a row (`seed`) was chosen on the fp64 reference alone for that to hold.

Decay regimes (`regime`; softplus and delta_bias on):
  suite   A in -[0.1, 1.1], softplus(delta) 0.7 .. 1: what tests/test_ops_selscan.py draws
  module  A[d, n] = -(n + 1), delta_bias = softplus^-1(dt), raw delta 0.3 N(0, 1); dt log-uniform in one half-decade window of the
          module's own range [1e-3, 0.1]: -lo [1e-3, 3e-3], -mid [3e-3, 1e-2], -hi [3e-2, 0.1] ([1e-2, 3e-2]: the mixed rows)
  small   the same in [1e-5, 1e-3]: -lo [1e-5, 3e-5], -mid [3e-5, 1e-4], -hi [3e-4, 1e-3] ([1e-4, 3e-4]: the mixed rows).  softplus(v) =
          log(1 + e^v) without a repair of the rounding of 1 + e^v is off by 6e-8 ABSOLUTE, up to 6e-3 of such a dt
  slow    |A| dt ~ 1e-3: state and adjoint cross every pass / tile boundary undamped
  fast    |A| dt of 20 .. 22, 60 and 90 per token: exp2 underflows, the reverse scans see zeros
  mixed   channel d is of regime d % 4 = module, small, slow, fast: the lanes of one wave (lanes kernels) and the waves of one workgroup
          (the others) take different branches of the softplus, of the sigmoid from it and of exp2 side by side.  The last state and dA
          of the slow channels are more than ten times those of the others and ddelta of the small-dt channels 1e-2 of the rest, so the
          floor of a slice is taken inside its regime (slice_check(groups=...)) where that is smaller than the tensor's.
A row with L = 1 has one element per slice: its u, z and g stay away from zero and its B, C are positive (`_inputs`), or a tenth of all
slices would be small by the draw alone.

Rows marked heavy take more than about 20 s on the emulator: they run there with OMK_FULL_EMU=1 only, and always under -m gpu.
"""
import math
import os

import pytest
import torch

import oracle as O
from tolerances import slice_check

BF16, F32 = torch.bfloat16, torch.float32
LANES = {"OMK_SELSCAN_LANES": "1"}
NO_PS = "OMK_SELSCAN_NO_PASS_STATES"

PC, PCB = "selscan_fwd<nreg=16>", "selscan_fwd<nreg=16>;selscan_bwd"
CH8, CH16 = "selscan_fwd_chunked<lc=8>", "selscan_fwd_chunked<lc=16>"
SH2, SH16, SH1S = ("selscan_fwd_shared<lc=8,nu=2,state_only=0>", "selscan_fwd_shared<lc=16,nu=1,state_only=0>",
                   "selscan_fwd_shared<lc=8,nu=1,state_only=1>")
LN0, LN1, LNB = "selscan_fwd_lanes<lc=0>", "selscan_fwd_lanes<lc=1>", "selscan_bwd_lanes"


def BC(nw, nb=16, noct=1):
    return f"selscan_bwd_chunked<nw={nw},nb={nb},noct={noct}>"


def row(D, L, N, fwd, bwd=None, twin=None, G=1, dtype=BF16, cl=False, bvar=True, cvar=True, bc_dtype=None, bc_state_contig=False, z=True,
        skip=True, bias=True, softplus=True, par_dtype=F32, env=None, regime="suite", dt=None, seed=0, batch=2, heavy=False):
    """fwd / bwd: the kernel strings after the forward / the backward (bwd None: forward only).  twin: the string of the backward when
    the forward handed over no pass / tile states (OMK_SELSCAN_NO_PASS_STATES=1) -- its gradients must equal the first backward's."""
    return dict(locals())


# the module's dt range [1e-3, 0.1] and the small one [1e-5, 1e-3] in windows of half a decade (module docstring); the fourth window of
# each, [1e-2, 3e-2] and [1e-4, 3e-4], is what the module and small-dt channels of the mixed rows draw from
REGIMES = {"module-lo": dict(regime="module", dt=(1e-3, 3e-3)), "module-mid": dict(regime="module", dt=(3e-3, 1e-2)),
           "module-hi": dict(regime="module", dt=(3e-2, 1e-1)),
           "small-lo": dict(regime="small", dt=(1e-5, 3e-5)), "small-mid": dict(regime="small", dt=(3e-5, 1e-4)),
           "small-hi": dict(regime="small", dt=(3e-4, 1e-3)),
           "slow": dict(regime="slow"), "fast": dict(regime="fast"), "mixed": dict(regime="mixed")}

# id -> row.  Batch 2 unless stated.
ROWS = {
    # ---- per-channel forward and backward (forward tile 32 tokens, backward tile 16)
    "pc-constBC-L1": row(6, 1, 4, PC, PCB, bvar=False, cvar=False, dtype=F32),
    "pc-constB-L31": row(6, 31, 4, PC, PCB, bvar=False),
    "pc-constB-L32": row(6, 32, 4, PC, PCB, bvar=False, dtype=F32, z=False, par_dtype=BF16),
    "pc-constBC-L33": row(6, 33, 4, PC, PCB, bvar=False, cvar=False, softplus=False, skip=False),
    "pc-nreg64-L33": row(130, 33, 24, "selscan_fwd<nreg=64>"),
    "pc-nreg64-L32-f32": row(130, 32, 24, "selscan_fwd<nreg=64>", dtype=F32, bias=False),
    "pc-G2-L1": row(12, 1, 8, LN0, LNB, LN0 + ";" + LNB, G=2),       # (one token: (B, D, 1) rows are channel-last too, so lanes take them)
    "pc-G2-L31": row(12, 31, 8, LN1, PCB, G=2, dtype=F32),
    "pc-G2-L32": row(12, 32, 8, LN1, PCB, G=2, bias=False),
    "pc-G2-L33": row(12, 33, 8, LN1, PCB, G=2, dtype=F32, par_dtype=BF16),
    # ---- chunked forward, own B / C rows per channel (10 or 3 channels per group: no sharing, per-channel backward)
    "ch8-L64": row(10, 64, 16, CH8, PCB),
    "ch8-L65": row(10, 65, 16, CH8, PCB, dtype=F32, z=False),
    "ch8-L513": row(10, 513, 16, CH8, softplus=False),
    "ch16-L1024": row(6, 1024, 16, CH16, G=2),
    "ch16-L1025": row(6, 1025, 16, CH16, G=2, dtype=F32, skip=False),
    "ch8-bc_f32": row(16, 130, 16, CH8, PCB, bc_dtype=F32, bias=False),
    "ch8-constB-N64-f32": row(8, 130, 64, CH8, bvar=False, dtype=F32),
    # ---- shared B / C rows (8 | channels per group) and the chunked backward
    "sh2-L64": row(16, 64, 16, SH2, BC(8), SH1S + ";" + BC(8), G=2),
    "sh2-L511": row(16, 511, 16, SH2, BC(8), SH1S + ";" + BC(8), G=2, dtype=F32, heavy=True),
    "sh2-L512": row(16, 512, 16, SH2, BC(8), SH1S + ";" + BC(8), G=2, heavy=True),
    "sh2-L513": row(16, 513, 16, SH2, BC(8), SH1S + ";" + BC(8), G=2, softplus=False, heavy=True),
    "sh2-L1023": row(8, 1023, 8, SH2),                                # (16 tokens per lane from L = 1024 on)
    "sh16-L1024": row(8, 1024, 8, SH16),
    "sh16-L1025": row(8, 1025, 8, SH16, dtype=F32, par_dtype=BF16),
    "bw-nw8-L65": row(8, 65, 16, SH2, BC(8), SH1S + ";" + BC(8), dtype=F32, bias=False),
    "bw-nw16-L130": row(16, 130, 16, SH2, BC(16), SH1S + ";" + BC(16), z=False, par_dtype=BF16),
    "bw-nb8-L64": row(16, 64, 8, SH2, BC(16, 8), SH1S + ";" + BC(16, 8), skip=False),
    "bw-nb8-L513": row(16, 513, 8, SH2, BC(16, 8), SH1S + ";" + BC(16, 8), dtype=F32, heavy=True),
    "bw-N24-L64": row(16, 64, 24, SH2, BC(16), SH1S + ";" + BC(16)),
    "bw-N64-f32-L64": row(8, 64, 64, CH8, BC(8), CH8 + ";" + BC(8), dtype=F32),
    "bw-N64-f32-L513": row(8, 513, 64, CH8, BC(8), CH8 + ";" + BC(8), dtype=F32, heavy=True),
    "bw-oct1-D32-L513": row(32, 513, 16, SH2, BC(16, 16, 1), SH1S + ";" + BC(16, 16, 1), batch=1, dtype=F32, env={"OMK_SELSCAN_BWD_OCT": "1"},
                            heavy=True),
    "bw-oct1-D32-L64": row(32, 64, 16, SH2, BC(16, 16, 1), SH1S + ";" + BC(16, 16, 1), batch=1, env={"OMK_SELSCAN_BWD_OCT": "1"}),
    "bw-oct2-D32-L64": row(32, 64, 16, SH2, BC(16, 16, 2), SH1S + ";" + BC(16, 16, 2), batch=1, dtype=F32, env={"OMK_SELSCAN_BWD_OCT": "2"}),
    "bw-oct4-D64-L64": row(64, 64, 16, SH2, BC(16, 16, 4), SH1S + ";" + BC(16, 16, 4), batch=1, env={"OMK_SELSCAN_BWD_OCT": "4"}),
    "bw-oct2-D32-L513": row(32, 513, 16, SH2, BC(16, 16, 2), SH1S + ";" + BC(16, 16, 2), batch=1, env={"OMK_SELSCAN_BWD_OCT": "2"}, heavy=True),
    "bw-oct4-D64-L513": row(64, 513, 16, SH2, BC(16, 16, 4), SH1S + ";" + BC(16, 16, 4), batch=1, dtype=F32, env={"OMK_SELSCAN_BWD_OCT": "4"},
                            heavy=True),
    # ---- lanes = channels, channel-last storage read as it lies (test hook: no minimum number of waves)
    "ln-D70-L1": row(70, 1, 16, LN0, LNB, LN0 + ";" + LNB, cl=True, env=LANES),
    "ln-D70-L15": row(70, 15, 16, LN0, LNB, LN0 + ";" + LNB, cl=True, env=LANES, dtype=F32, bc_state_contig=True),
    "ln-D70-L16": row(70, 16, 5, LN0, LNB, LN0 + ";" + LNB, cl=True, env=LANES, z=False),
    "ln-D70-L17": row(70, 17, 16, LN0, LNB, LN0 + ";" + LNB, cl=True, env=LANES, bc_state_contig=True, par_dtype=BF16),
    "ln-D70-L33": row(70, 33, 5, LN0, LNB, LN0 + ";" + LNB, cl=True, env=LANES, dtype=F32, softplus=False),
    "ln-D96-G2-L17": row(96, 17, 5, LN0, LNB, LN0 + ";" + LNB, G=2, cl=True, env=LANES, dtype=F32, bias=False, bc_state_contig=True),
    "ln-D96-G2-L33": row(96, 33, 16, LN0, LNB, LN0 + ";" + LNB, G=2, cl=True, env=LANES, skip=False),
    "ln-lc1-D70-L33": row(70, 33, 16, LN1, PCB, env=LANES),
    "ln-lc1-D96-G2-L17": row(96, 17, 5, LN1, PCB, G=2, env=LANES, dtype=F32),
    # ---- decay regimes on the cheapest shape of each form, L across a tile / pass boundary
    # (the mixed rows take more channels: four regimes in turn, d % 4, and a floored slice must stay under 5 % of the tensor's)
    **{f"pc-{k}": row(32 if k == "mixed" else 6, 33, 4, PC, PCB, bvar=False, dtype=F32, **v) for k, v in REGIMES.items()},
    **{f"ch8-{k}": row(20 if k == "mixed" else 10, 65, 16, CH8, PCB, dtype=F32, **v) for k, v in REGIMES.items()},
    **{f"sh2-{k}-L130": row(16, 130, 16, SH2, BC(16), SH1S + ";" + BC(16), dtype=F32, **v) for k, v in REGIMES.items() if k[0] in "ms"},       # (module, small, slow, mixed)
    **{f"sh2-{k}-L513": row(16, 513, 16, SH2, BC(16), SH1S + ";" + BC(16), dtype=F32, heavy=True, **v) for k, v in REGIMES.items()},
    "sh2-small-hi-L513-bf16": row(16, 513, 16, SH2, BC(16), SH1S + ";" + BC(16), heavy=True, **REGIMES["small-hi"]),
    **{f"ln-{k}": row(70, 33, 16, LN0, LNB, LN0 + ";" + LNB, cl=True, env=LANES, dtype=F32, **v) for k, v in REGIMES.items()},
    "ln-small-lo-bf16": row(70, 33, 16, LN0, LNB, LN0 + ";" + LNB, cl=True, env=LANES, **REGIMES["small-lo"]),
}
# the seed of a row's inputs where 0 leaves more than 5 % of the slices of some output of the fp64 reference under the floor
SEEDS = {"bw-N24-L64": 5, "bw-nw8-L65": 1, "bw-oct1-D32-L64": 6, "bw-oct2-D32-L64": 6, "bw-oct4-D64-L64": 4, "ch8-fast": 2, "ch8-module-hi": 1,
         "ln-D70-L15": 9, "ln-D70-L17": 4, "ln-D70-L33": 3, "ln-D96-G2-L17": 18, "ln-lc1-D70-L33": 1, "ln-lc1-D96-G2-L17": 18, "ln-slow": 1,
         "pc-G2-L31": 5, "pc-constB-L31": 15, "pc-constB-L32": 4, "pc-constBC-L33": 26, "pc-fast": 1, "pc-module-hi": 18, "pc-module-lo": 1,
         "pc-slow": 7, "pc-small-hi": 1, "pc-small-lo": 1, "sh2-L64": 3,
         "pc-mixed": 17, "pc-module-mid": 3, "pc-small-mid": 1, "sh2-module-mid-L513": 2}
for _k, _s in SEEDS.items():
    ROWS[_k]["seed"] = _s


MIXED = (("module", (1e-2, 3e-2)), ("small", (1e-4, 3e-4)), ("slow", None), ("fast", None))


def _groups(r):
    """Regime of every channel of a mixed row (slice_check(groups=...)), None for the others."""
    return torch.arange(r["D"]) % 4 if r["regime"] == "mixed" else None


def _inv_softplus(dt):
    return torch.log(torch.expm1(dt.double())).float()


def _log_uniform(g, n, lo, hi):
    return torch.exp(torch.rand(n, generator=g) * (math.log(hi) - math.log(lo)) + math.log(lo))


def _regime(r, g, Dm, N, win):
    """(A (D, N) fp32, delta_bias (D) fp32, scale of the raw delta N(0, 1)); 'suite' draws delta its own way."""
    n1 = torch.arange(1, N + 1, dtype=torch.float32)
    # |A| dt of the fast channels: 20 .. 22, and 60 and 90 for the last two states (e^-90 is below the smallest fp32 number).  A dA row
    # is then a norm over several comparable elements and not the one sum of random signs that a steep ladder of decays leaves
    spread = torch.cat([20.0 + 2.0 * torch.rand(N - 2, generator=g), torch.tensor([60.0, 90.0])])
    if r in ("module", "small"):
        dt = _log_uniform(g, Dm, *win)
        return -n1.repeat(Dm, 1), _inv_softplus(dt), 0.3
    if r == "slow":
        dt = _log_uniform(g, Dm, 7e-3, 1.5e-2)
        return -(1e-3 / dt)[:, None] * (0.5 + torch.rand(Dm, N, generator=g)), _inv_softplus(dt), 0.3
    if r == "fast":
        return -spread.repeat(Dm, 1), _inv_softplus(torch.ones(Dm)), 0.05
    assert r == "mixed"      # channel d is of regime d % 4 (MIXED): every wave of the lanes kernels and every workgroup of the others holds all four
    parts = [_regime(k, g, Dm, N, w) for k, w in MIXED]
    pick = lambda i: torch.stack([parts[d % 4][i][d] if parts[d % 4][i].dim() else parts[d % 4][i] for d in range(Dm)])
    return pick(0), pick(1), torch.tensor([parts[d % 4][2] for d in range(Dm)])


def _inputs(r):
    """CPU tensors exactly as the kernel reads them: [u, delta, A, B, C, D, z, delta_bias] (None where absent)."""
    g = torch.Generator().manual_seed(r["seed"])
    Bsz, Dm, L, N, G, dt = r["batch"], r["D"], r["L"], r["N"], r["G"], r["dtype"]

    def rows(t):     # (B, L, D) storage -> (B, D, L): a view (channel-last) or L-contiguous
        t = t.to(dt).transpose(1, 2)
        return t if r["cl"] else t.contiguous()

    def bc(var):
        if not var:
            return 0.5 + torch.rand(Dm, N, generator=g) if one else torch.randn(Dm, N, generator=g)
        t = (0.5 + torch.rand(Bsz, G, L, N, generator=g) if one else torch.randn(Bsz, G, L, N, generator=g)).to(r["bc_dtype"] or dt).transpose(2, 3)   # (B, G, N, L), the state contiguous
        t = t if r["bc_state_contig"] else t.contiguous()
        return t[:, 0] if G == 1 else t

    one = L == 1     # one element per slice: u 0.75 .. 1.25 with random signs, z, B and C positive
    if one:      # (z positive: silu'(z) = 0 at z = -1.28)
        u = rows((0.75 + 0.5 * torch.rand(Bsz, L, Dm, generator=g)) * (2.0 * torch.randint(0, 2, (Bsz, L, Dm), generator=g) - 1.0))
        z = rows(0.75 + 0.5 * torch.rand(Bsz, L, Dm, generator=g))
    else:
        u, z = rows(torch.randn(Bsz, L, Dm, generator=g)), rows(torch.randn(Bsz, L, Dm, generator=g))
    if r["regime"] == "suite":
        delta = rows(0.5 * torch.rand(Bsz, L, Dm, generator=g))
        A, db = -(torch.rand(Dm, N, generator=g) + 0.1), 0.1 * torch.randn(Dm, generator=g)
    else:
        assert r["softplus"] and r["bias"]
        A, db, sc = _regime(r["regime"], g, Dm, N, r["dt"])
        delta = rows(sc * torch.randn(Bsz, L, Dm, generator=g))
        fast = {"fast": torch.ones(Dm, dtype=torch.bool), "mixed": torch.arange(Dm) % 4 == 3}.get(r["regime"])
        if fast is not None:           # the last state is the last token's dt B u alone: a u of that token near zero is a row near zero
            u = rows(torch.where(fast, 1.0 + 0.5 * torch.randn(Bsz, L, Dm, generator=g), u.transpose(1, 2).float()))
    Bm, Cm = bc(r["bvar"]), bc(r["cvar"])
    D = (1.0 + 0.3 * torch.randn(Dm, generator=g)).to(r["par_dtype"])
    return [u, delta, A, Bm, Cm, D if r["skip"] else None, z if r["z"] else None, db.to(r["par_dtype"]) if r["bias"] else None]


def _reference(r, src):
    """fp64 oracle on the tensors of _inputs: (leaves, out, last_state, upstream gradient g in the kernel's dtype)."""
    lv = [None if t is None else t.detach().double().requires_grad_() for t in src]
    out, last = O.selective_scan_ref(*lv, r["softplus"], True, compute_dtype=torch.float64)
    o = out.detach()
    # d out / d D and d out / d delta_bias of every (batch, channel, token), the latter by a central difference (g is an input: any will do)
    with torch.no_grad():
        s64 = [None if t is None else t.detach().double() for t in src]
        k = s64[0] if s64[6] is None else s64[0] * s64[6] * torch.sigmoid(s64[6])
        db, h = (torch.zeros(r["D"], dtype=torch.float64) if s64[7] is None else s64[7]), 1e-6
        side = lambda e: O.selective_scan_ref(*s64[:7], db + e, r["softplus"], compute_dtype=torch.float64)
        J = (side(h) - side(-h)) / (2 * h)
        unit = lambda t: t / t.pow(2).mean(dim=2, keepdim=True).sqrt().clamp_min(1e-300)
        noise = torch.randn(o.shape, generator=torch.Generator().manual_seed(r["seed"] + 1), dtype=torch.float64)
        g = (0.3 * noise + unit(k) + 2.0 * unit(J)).to(r["dtype"])      # (weights 1 and 2: no row where the two cancel)
    if r["bwd"]:
        out.backward(g.double())
    return lv, o, last.detach(), g


NAMES = ["u", "delta", "A", "B", "C", "D", "z", "delta_bias"]


def _keep(name, t):
    return {"u": 2, "delta": 2, "z": 2, "A": 1, "D": 1, "delta_bias": 1}.get(name, t.dim() - 1)


def _chan(name, t):
    return name not in ("B", "C") or t.dim() == 2


def _launch(r, src, g, dev, lib):
    """Forward (+ backward) through the autograd function: (out, last, gradients, kernels after the forward, after the backward)."""
    from omnimamba_amd.selective_scan import selective_scan_fn
    need = bool(r["bwd"])
    lv = [None if t is None else t.detach().to(dev).requires_grad_(need) for t in src]
    for a, b in zip(lv, src):
        assert a is None or a.stride() == b.stride()
    out, last = selective_scan_fn(*lv, r["softplus"], True)
    kf, kb, states = lib.omk_ssd_last_kernels().decode(), None, None
    if need:
        states = out.grad_fn.saved_tensors[8]      # what the forward kept for the backward: pass states, tile states or None
        # (the record is per thread and autograd runs the backward of device tensors on a thread of its own: read it from a hook there)
        seen = []
        lv[0].register_hook(lambda _: seen.append(lib.omk_ssd_last_kernels().decode()))
        out.backward(g.to(dev))
        kb, = seen
    return out.detach(), last, [None if t is None or t.grad is None else t.grad for t in lv], kf, kb, states


@pytest.mark.parametrize("case", sorted(ROWS))
def test_selscan_slices(dev, monkeypatch, case):
    from omnimamba_amd._lib import get_lib
    r = ROWS[case]
    if r["heavy"] and dev.type == "cpu" and not os.environ.get("OMK_FULL_EMU"):
        pytest.skip("more than 20 s on the emulator: runs on the GPU (-m gpu) or with OMK_FULL_EMU=1")
    for k, v in (r["env"] or {}).items():
        monkeypatch.setenv(k, v)
    monkeypatch.delenv(NO_PS, raising=False)
    lib = get_lib()
    src = _inputs(r)
    ref, o0, l0, g = _reference(r, src)
    out, last, grads, kf, kb, states = _launch(r, src, g, dev, lib)
    assert (kf, kb) == (r["fwd"], r["bwd"])
    if r["cl"]:
        assert out.stride(1) == 1            # read and written as it lies
    report, shares = [], {}

    def check(name, got, want, dtype, keep, kernel, chan=True):
        """chan: the last slice dimension is the channel (all but input-dependent dB / dC): the regime groups of a mixed row apply."""
        e, q, b, share = slice_check(f"{case} {name} [{kernel}]", got, want, dtype, keep, groups=_groups(r) if chan else None)
        report.append(f"{name}={e:.1e}/{b:.1e}")
        shares[name] = share

    check("out", out, o0, r["dtype"], 2, kf)
    check("last", last, l0, F32, 2, kf)
    if r["twin"]:
        # the states the forward handed to the backward, against the fp64 state of the prefix in front of each: (B, D, passes, N) in
        # front of every 512-token pass, or (B, tiles, N, D) in front of every 16-token tile of the lanes form
        assert states is not None
        tiles = states.shape[-1] == r["D"] and states.shape[1] == (r["L"] + 15) // 16
        step, n = (16, states.shape[1]) if tiles else (512, states.shape[2])
        assert n == (r["L"] + step - 1) // step
        for j in range(n):
            got = states[:, j].transpose(1, 2) if tiles else states[:, :, j]
            if j == 0:
                assert bool((got == 0).all())
                continue
            with torch.no_grad():
                cut = [t[..., :j * step] if t is not None and t.dim() >= 3 else t for t in ref]
                _, want = O.selective_scan_ref(*cut, r["softplus"], True, compute_dtype=torch.float64)
            check(f"state{j}", got, want, F32, 2, kf)
    if kb:
        for name, a, b, s in zip(NAMES, grads, ref, src):
            if s is None:
                continue
            assert a is not None and a.shape == s.shape and a.dtype == s.dtype, name
            # dA, dD, ddelta_bias and constant dB / dC are fp32 sums cast to the parameter's dtype by the wrapper
            check("d" + name, a, b.grad, a.dtype, _keep(name, s), kb, chan=_chan(name, s))
    print(f"\n[slices] {case} {dev.type} {kf} | {kb}: " + " ".join(report))
    assert max(shares.values()) <= 0.05, shares
    if r["twin"]:
        # the same gradients from the backward's own state-only pass / forward sweep instead of the states the forward saved
        monkeypatch.setenv(NO_PS, "1")
        out2, _, grads2, kf2, kb2, states2 = _launch(r, src, g, dev, lib)
        assert (kf2, kb2) == (r["fwd"], r["twin"]) and torch.equal(out2.cpu(), out.cpu()) and states2 is None
        for name, a, b, w, s in zip(NAMES, grads2, grads, ref, src):
            if s is not None:
                check("d" + name, a, w.grad, a.dtype, _keep(name, s), kb2, chan=_chan(name, s))
                slice_check(f"{case} d{name} [{kb2}] against [{kb}]", a, b, F32, _keep(name, s), bound=1e-6,
                            groups=_groups(r) if _chan(name, s) else None)


def test_every_dispatched_kernel_has_numbers():
    """Every kernel string of tests/test_selscan_dispatch.py that launches something is the forward, backward or twin string of a row
    here, and a row that is not heavy on the emulator carries it: a later dispatch row without numbers fails."""
    from test_selscan_dispatch import EXPECTED
    want = {k for _, _, k in EXPECTED.values() if k}
    have = {r[f] for r in ROWS.values() for f in ("fwd", "bwd", "twin") if r[f]}
    light = {r[f] for r in ROWS.values() if not r["heavy"] for f in ("fwd", "bwd", "twin") if r[f]}
    assert not want - have, sorted(want - have)
    assert not want - light, sorted(want - light)
