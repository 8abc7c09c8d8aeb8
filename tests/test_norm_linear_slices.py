"""omk_norm_linear (norm + projection + LoRA + conv tail of the decode step) over every form of its selector and every template
instantiation of its kernels, bf16 / fp32 / f16 weights: emulator on CPU, MI355X under -m gpu.  (fp8 weights: test_fp8_decode*.py.)

Reference: fp64, from exactly the tensors the kernel reads, already rounded to their storage dtypes:

    q = x + residual | x silu(z) | x;   u = q w;   out = rstd (W u + scale B (A u)) + bias      (rstd per norm group)

with the kernel's two documented rounding points and nothing else (tolerances.py, module docstring): u as bf16 in the BATCHED / MATRIX
forms under bf16 weights (formed in fp32 in the kernel's order; gated inputs are drawn away from bf16 midpoints of u and each gated row
asserts that), and the projected value of a conv channel rounded to the activation dtype before it enters the tap sum (the conv reference
takes the newest state column as the kernel stored it, which is itself checked against the unrounded projection).

Bound: tolerances.slice_check with the project's OP_ARITH, per (sequence, block of 16 output rows) -- outside the conv range aligned to
row 0, inside it aligned to conv_offset -- and per (sequence, 16 channels) of the newest conv-state column; at most 5 % of the slices of any
output may meet the floor (the row's seed is chosen on the reference for that).  Exact: residual_out, the rolled conv-state columns, every
pool row no sequence addresses, the zeros in the conv columns of a padding sequence.

Guards: strided rows are column slices of NaN-filled parents (x, residual, z, out, residual_out, weight, lora_a, lora_b, and the conv
state as (rows, S, C) transposed) whose elements outside the slice must still be NaN after the call; out and residual_out start as NaN
everywhere; the conv state is rows of a pool with two rows more than the batch.

Dispatch: `plan` below repeats nl_plan's rules for 256 compute units (what the emulator and the MI355X report); every row names its
form, the test asserts norm_linear.form(...) == that before it runs, and the row id carries the template parameters the row reaches:

    form - TW (weights) - TR (residual) - NQ (in / 1024) - RMAX (0 / 8) - NB (sequences rounded up) - gate - ROWS per tile - k (nbatch,
    row batches per wave; matrix form: the largest number of tiles one workgroup walks)

Each row prints its worst slice as a fraction of the bound and the share of floored slices (`pytest -s`; profiles/norm_linear_slices.txt).
No row takes more than about 5 s on the emulator (the nbatch rows, 8 - 17 M weights), so none is marked heavy and none skips there."""
from types import SimpleNamespace

import pytest
import torch

from tolerances import column_blocks, near_bf16_midpoint, slice_check

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
NAME = {F32: "f32", BF16: "bf16", F16: "f16", None: "none"}
EPS, SCALE = 1e-5, 4.0
CUS = 256
NAN = float("nan")


def row(name, form, B=1, In=1024, Out=40, w=BF16, x=None, res=None, ro=None, nw="w", bias=None, R=0, ldt=None, odt=None, G=1, gate=False,
        nbg=False, conv=None, cbias=True, silu=True, idx=None, pool=None, steps=1, strided=False, lb_unaligned=False, wgs=None, seed=1):
    """One call.  w / x / res / ro / nw / bias / ldt / odt: dtypes of the weight, the activations (default: the weight's), the residual
    and residual_out (None: absent), the norm weight ("w": the weight's; None: no norm), the bias (None: absent), the LoRA factors and
    the output (default: x's).  R: LoRA rank.  G: norm groups.  conv: (W, S, conv_offset, C).  idx: conv_state_indices (None: the state
    is pool rows 1 .. B); pool: its rows (default B + 2).  steps: consecutive calls on the same state.  strided: the operands are column
    slices of NaN-filled parents.  lb_unaligned: rows of lora_b 24 bytes apart.  wgs: OMK_NL_MFMA_WGS.  seed: chosen on the reference."""
    x = x or w
    return SimpleNamespace(name=name, form=form, B=B, In=In, Out=Out, w=w, x=x, res=res, ro=ro, nw=w if nw == "w" else nw, bias=bias, R=R,
                           ldt=ldt or w, odt=odt or x, G=G, gate=gate, nbg=nbg, conv=conv, cbias=cbias, silu=silu, idx=idx,
                           pool=pool or B + 2, steps=steps, strided=strided, lb_unaligned=lb_unaligned, wgs=wgs, seed=seed)


# ------------------------------------------------------------------------------------------------------------------------------
# the selector's rules (nl_plan in csrc/norm_linear.hip), for CUS compute units
# ------------------------------------------------------------------------------------------------------------------------------
def plan(r):
    """(form, TW, TR, NQ, RMAX, NB, GATE, ROWS, k) the library's selector reaches for row r; None where a parameter does not exist."""
    uniform = (r.w in (F32, BF16) and r.x == r.w and r.nw == r.w and r.odt == r.w and (r.bias in (None, r.w)) and (r.R == 0 or r.ldt == r.w)
               and r.G == 1 and r.R <= 8 and r.In in (1024, 2048, 4096) and (r.res in (None, F32, r.w))
               and (r.ro is None or r.res is None or r.ro == r.res))
    trdt = r.res or r.ro or r.w
    uniform = uniform and trdt in (F32, r.w)
    nq, es = r.In // 1024, 4 if r.w == F32 else 2
    rw = 16 // (r.In // (64 * (16 // es)))                     # rows per batch: 16 loads of 16 bytes per lane
    rmax = 8 if r.R else 0
    if r.B > 1:
        assert uniform and not (r.gate and r.res), "two to eight sequences: the uniform-dtype kernels, gate or residual"
        nb = 2 if r.B <= 2 else (4 if r.B <= 4 else 8)
        lora16 = r.R == 0 or (r.R == 8 and not r.lb_unaligned)            # (the parents of strided rows keep 16-byte alignment)
        if lora16 and (r.w == BF16 or (nq <= 2 and nb == 8 and r.R > 0)):
            wgs = r.wgs or CUS
            rows = 8 if (r.Out + 15) // 16 < wgs else 16
            ntile = (r.Out + rows - 1) // rows
            return ("matrix", r.w, trdt, nq, rmax, nb, r.gate, rows, (ntile + min(ntile, wgs) - 1) // min(ntile, wgs))
        bsmem = nb * r.In * es + 4 * nb * 73 * 4
        assert bsmem <= 150 * 1024
        maxw = (2 if bsmem <= 76 * 1024 else 1) * CUS * 4
        k = (r.Out + rw * maxw - 1) // (rw * maxw)
        assert k * rw <= 64
        return ("batched", r.w, trdt, nq, rmax, nb, r.gate, None, k)
    if uniform:
        k = (r.Out + rw * 2 * CUS * 4 - 1) // (rw * 2 * CUS * 4)
        if k * rw <= 64:
            return ("fast", r.w, trdt, nq, rmax, None, None, None, k)
    assert r.conv is None
    return ("generic", r.w, None, None, None, None, None, None, None)


def rid(r):
    f, tw, tr, nq, rmax, nb, gate, rows, k = plan(r)
    parts = [f, NAME[tw]] + ([] if f == "generic" else ["r" + NAME[tr], f"nq{nq}", f"rmax{rmax}"])
    if nb:
        parts += [f"nb{nb}", "gate" if gate else "nogate"]
    if rows:
        parts.append(f"rows{rows}")
    if k:
        parts.append(f"k{k}")
    return r.name + ":" + "-".join(parts)


# ------------------------------------------------------------------------------------------------------------------------------
# the table
# ------------------------------------------------------------------------------------------------------------------------------
CONVS = [(2, 1), (2, 4), (3, 2), (3, 3), (4, 3), (4, 4)]          # (W, S) of the conv tail


def _rows():
    T = []
    add = lambda *a, **k: T.append(row(*a, **k))
    # ---- GENERIC: one sequence, run-time dtypes (anything the uniform-dtype rule refuses)
    add("g-mixed-lora8-out-f16", "generic", w=F32, x=BF16, res=F32, ro=F32, nw=F32, bias=BF16, R=8, ldt=F16, odt=F16, Out=40, strided=True)
    add("g-bf16w-in3072-lora9", "generic", w=BF16, x=F32, res=BF16, ro=F32, nw=BF16, R=9, ldt=F32, In=3072, Out=7)
    add("g-f16-lora16", "generic", w=F16, res=F16, ro=F16, bias=F16, R=16, Out=9, strided=True)
    add("g-f32-in8192-lora1-ro-alone", "generic", w=F32, ro=F32, bias=F32, R=1, In=8192, Out=8)
    add("g-f16w-in8192", "generic", w=F16, x=BF16, nw=F32, In=8192, Out=40, strided=True)
    add("g-plain-linear", "generic", w=BF16, nw=None, Out=1)
    add("g-plain-linear-f32-bias", "generic", w=F32, x=F16, nw=None, bias=F32, Out=70, strided=True)
    add("g-ro-alone-bf16-from-f32", "generic", w=F32, ro=BF16, Out=33)
    for j, (G, nbg) in enumerate([(1, False), (1, True), (2, False), (2, True), (4, False), (8, False), (8, True)]):
        add(f"g-gate-G{G}{'-nbg' if nbg else ''}", "generic", w=[BF16, F16, F32][j % 3], nw=F32 if G == 1 else "w", G=G, gate=True, nbg=nbg,
            In=[1024, 3072, 2048][j % 3], Out=[40, 8, 70][j % 3], bias=[None, F32][j % 2], strided=j % 2 == 1)
    # ---- FAST: one sequence, one dtype: {f32, bf16} x residual {f32, same dtype, none} x NQ, the LoRA ranks and the bias cycled
    j = 0
    for w in (F32, BF16):
        for res in ((F32, None) if w == F32 else (F32, BF16, None)):
            for nq in (1, 2, 4):
                add(f"f-{NAME[w]}-res-{NAME[res]}", "fast", w=w, res=res, ro=res if j % 4 else (res or w), In=1024 * nq, Out=[40, 70, 200][j % 3],
                    R=[0, 1, 3, 7, 8][j % 5], bias=w if j % 2 == 0 else None, strided=j % 2 == 1)
                j += 1
    add("f-f32-gate", "fast", w=F32, gate=True, R=8, Out=70, strided=True)
    add("f-f32-gate-nbg", "fast", w=F32, gate=True, nbg=True, In=2048, Out=40, bias=F32)
    add("f-bf16-gate", "fast", w=BF16, gate=True, In=4096, Out=70)
    add("f-bf16-gate-nbg-res", "fast", w=BF16, gate=True, nbg=True, res=F32, ro=F32, R=3, Out=200, strided=True)
    for j, (W, S) in enumerate(CONVS):
        Out = [70, 200][j % 2]
        off, C = [(0, 24), (Out - 37, 37), (8, 20)][j % 3]          # from row 0; up to the last row; inside, ragged blocks on both sides
        add(f"f-conv-w{W}s{S}", "fast", w=[F32, BF16][j % 2], res=F32 if j % 2 == 0 else [F32, None, BF16][j % 3], R=[8, 0][j % 2],
            In=[1024, 2048][j // 3], Out=Out, conv=(W, S, off, C), cbias=j % 2 == 0, silu=j % 3 != 1, strided=j % 2 == 0)
    add("f-conv-two-steps", "fast", w=BF16, res=F32, ro=F32, R=8, Out=200, conv=(4, 4, 48, 120), steps=2, strided=True)
    add("f-conv-two-steps-f32", "fast", w=F32, Out=70, conv=(3, 2, 16, 50), cbias=False, steps=2)
    add("f-conv-one-row-pool", "fast", w=BF16, Out=70, conv=(4, 3, 8, 40), idx=[0], pool=1)
    add("f-conv-pool-slot", "fast", w=F32, Out=70, conv=(4, 4, 8, 40), idx=[2], pool=4, silu=False, strided=True)
    add("f-conv-negative-index", "fast", w=BF16, R=8, Out=70, conv=(4, 4, 8, 40), idx=[-1], strided=True)
    add("f-conv-index-past-pool", "fast", w=F32, Out=70, conv=(2, 1, 0, 60), idx=[3], pool=3)
    # nbatch: fp32, 4096 features: 16 loads per lane = one row per batch (rw = 1), 2 x 256 x 4 = 2048 waves: Out 2050 -> k = 2, 4100 -> k = 3
    add("f-f32-nbatch2", "fast", w=F32, res=F32, ro=F32, R=8, bias=F32, In=4096, Out=2050)
    add("f-f32-nbatch3", "fast", w=F32, In=4096, Out=4100, strided=True)
    # bf16, 2048 features: rw = 4 rows per batch: Out 8200 > 4 x 2048 -> k = 2 (the shape class of the 1.3B in_proj)
    add("f-bf16-nbatch2", "fast", w=BF16, res=F32, ro=F32, R=8, In=2048, Out=8200, conv=(4, 4, 4096, 4100))
    # ---- BATCHED: two to eight sequences on the vector pipe: fp32 outside the matrix case; bf16 with LoRA rank 1 .. 7 or unaligned B rows
    for B in range(2, 9):
        nq = [1, 2, 4][B % 3]
        res = [F32, None, F32][B % 3]
        gate = B in (3, 6)
        add(f"b-f32-B{B}", "batched", w=F32, B=B, In=1024 * nq, Out=[40, 70, 200][B % 3], res=None if gate else res, ro=None if gate else res,
            gate=gate, nbg=B == 6, R=[0, 4, 7][B % 3], bias=F32 if B % 2 else None, strided=B % 2 == 0)
        nq = [2, 4, 1][B % 3]
        res = [BF16, F32, None][B % 3]
        gate = B in (3, 8)
        add(f"b-bf16-B{B}", "batched", w=BF16, B=B, In=1024 * nq, Out=[70, 200, 40][B % 3], res=None if gate else res, ro=None if gate else res,
            gate=gate, nbg=B == 8, R=[4, 7, 1, 8][B % 4], lb_unaligned=B % 4 == 3, bias=BF16 if B % 2 == 0 else None, strided=B % 2 == 1)
    add("b-f32-B8-nq2-nolora", "batched", w=F32, B=8, In=2048, Out=70, res=F32, ro=F32)
    add("b-f32-conv-pool-padding", "batched", w=F32, B=3, Out=70, R=4, res=F32, ro=F32, conv=(4, 4, 8, 40), idx=[4, -1, 1], pool=5, steps=2,
        strided=True)
    add("b-bf16-conv-pool-padding", "batched", w=BF16, B=5, In=2048, Out=200, R=7, conv=(3, 2, 60, 100), idx=[6, 0, 9, 3, 2], pool=7, cbias=False)
    add("b-bf16-conv-no-indices", "batched", w=BF16, B=2, Out=70, R=8, lb_unaligned=True, res=BF16, ro=BF16, conv=(4, 3, 0, 70), silu=False,
        strided=True)
    # nbatch: fp32, 4096 features, eight sequences: 140 KB of LDS = one workgroup per CU = 1024 waves, rw = 1: Out 1030 -> k = 2
    add("b-f32-nbatch2", "batched", w=F32, B=8, In=4096, Out=1030, R=4, res=F32, ro=F32)
    # bf16, 1024 features: rw = 8, 2 x 256 x 4 waves: Out 16400 -> k = 2
    add("b-bf16-nbatch2", "batched", w=BF16, B=2, Out=16400, R=7, gate=True)
    # ---- MATRIX: bf16 at every B x NQ; ROWS 16 and several tiles per workgroup through OMK_NL_MFMA_WGS
    j = 0
    for B in range(2, 9):
        for nq in (1, 2, 4):
            mode = ["res-f32", "gate", "res-bf16", "none", "gate-nbg"][j % 5]
            res = {"res-f32": F32, "res-bf16": BF16}.get(mode)
            Out, wgs = [(70, None), (70, 2), (65, 5), (5, None), (70, 6), (129, 3), (70, 3)][j % 7]
            add(f"m-bf16-B{B}", "matrix", w=BF16, B=B, In=1024 * nq, Out=Out, wgs=wgs, res=res, ro=res, gate="gate" in mode, nbg=mode == "gate-nbg",
                R=[8, 0][j % 2], bias=BF16 if j % 3 == 0 else None, strided=j % 2 == 1)
            j += 1
    for B, nq, Out, wgs in [(8, 1, 70, None), (8, 2, 70, 2), (5, 2, 65, 5), (6, 1, 200, 4), (7, 1, 5, None)]:
        add(f"m-f32-B{B}", "matrix", w=F32, B=B, In=1024 * nq, Out=Out, wgs=wgs, R=8, res=F32 if B != 6 else None, ro=F32 if B != 6 else None,
            gate=B == 6, bias=F32 if B == 8 else None, strided=B % 2 == 1)
    add("m-bf16-conv-pool-padding", "matrix", w=BF16, B=5, In=2048, Out=200, wgs=3, R=8, res=F32, ro=F32, conv=(4, 3, 60, 100),
        idx=[6, 0, -1, 3, 2], pool=7, steps=2, strided=True)
    add("m-bf16-conv-rows8", "matrix", w=BF16, B=3, Out=70, conv=(2, 4, 0, 33), idx=[0, 7, 1], pool=5, cbias=False, silu=False)
    add("m-f32-conv-pool-padding", "matrix", w=F32, B=8, Out=70, wgs=2, R=8, res=F32, ro=F32, conv=(3, 3, 37, 33), idx=[1, 2, 3, 4, 5, -2, 7, 8],
        pool=10)
    names = [r.name for r in T]
    for r in T:                                                       # names repeat across NQ: number them
        if names.count(r.name) > 1:
            r.name = f"{r.name}-in{r.In}"
    return T


ROWS = {}
for _r in _rows():
    assert _r.name not in ROWS, _r.name
    ROWS[_r.name] = _r
# rows whose seed 1 leaves more than 5 % of some output's slices on the floor (a last tile of one row: a single element is often small)
SEEDS = {"m-bf16-B5-in1024": 2, "m-bf16-B7-in2048": 2, "m-f32-B5": 3, "m-bf16-conv-pool-padding": 2}
for _k, _s in SEEDS.items():
    ROWS[_k].seed = _s


# ------------------------------------------------------------------------------------------------------------------------------
# inputs: parents own the memory, the call's operands are views of them
# ------------------------------------------------------------------------------------------------------------------------------
def rounded_u(r):
    """The kernel keeps u as bf16 in LDS: the BATCHED / MATRIX forms under bf16 weights."""
    return r.B > 1 and r.w == BF16


def held(t, dtype, lead, trail):
    """t rounded to dtype inside a NaN-filled parent with `lead` / `trail` more columns (0, 0: t itself).  Returns (parent, column range)."""
    n = t.shape[-1]
    p = torch.full(t.shape[:-1] + (lead + n + trail,), NAN)
    p[..., lead:lead + n] = t
    return p.to(dtype), (lead, lead + n)


def view(P, k):
    """Operand k of the parents P (None where the call has none)."""
    if k not in P["_cols"]:
        return None
    a, b = P["_cols"][k]
    return P[k][..., a:b]


def exact_u(r, x, res, z, nw):
    x, g = x.double(), None if z is None else z.double() * torch.sigmoid(z.double())
    s = x if res is None else x + res.double()
    return s * nw.double() if g is None else s * g * nw.double()


def make_inputs(r, step):
    """The parents of one step, on the CPU (the weights, LoRA factors and conv parameters depend on the seed alone: the same every step)."""
    g = torch.Generator().manual_seed(1000 * r.seed + 7)
    gs = torch.Generator().manual_seed(1000 * r.seed + 100 + step)
    rn = lambda gen, *s: torch.randn(*s, generator=gen)
    pad = (8, 8) if r.strided else (0, 0)
    P, cols = {}, {}

    def put(k, t, dtype, lead=pad[0], trail=pad[1]):
        P[k], cols[k] = held(t, dtype, lead, trail)

    put("weight", rn(g, r.Out, r.In) * 0.05, r.w)
    if r.nw is not None:
        put("norm_weight", torch.rand(r.In, generator=g) + 0.5, r.nw, 0, 0)
    if r.bias is not None:
        put("bias", rn(g, r.Out), r.bias, 0, 0)
    if r.R:
        put("lora_a", rn(g, r.R, r.In) * 0.05, r.ldt)
        if r.lb_unaligned:
            put("lora_b", rn(g, r.Out, r.R) * 0.05, r.ldt, 4, 0)      # rows of 12 elements = 24 bytes
        else:
            put("lora_b", rn(g, r.Out, r.R) * 0.05, r.ldt)
    if r.conv:
        W, S, off, C = r.conv
        put("conv_weight", rn(g, C, W) * 0.5, r.w, 0, 0)
        if r.cbias:
            put("conv_bias", rn(g, C) * 0.2, r.w, 0, 0)
        if step == 0:
            put("pool", rn(g, r.pool, S, C), r.w, 4 if r.strided else 0, 4 if r.strided else 0)      # (rows, S, C): channel-contiguous
        if r.idx is not None:
            P["idx"] = torch.tensor(r.idx, dtype=torch.int32)
    put("x", rn(gs, r.B, r.In), r.x)
    if r.res is not None:
        put("residual", rn(gs, r.B, r.In), r.res)
    if r.gate:
        z = rn(gs, r.B, r.In).to(r.x)
        if rounded_u(r):
            # elements of z whose exact u lies next to a bf16 rounding midpoint are drawn again (silu_fast differs from the exact sigmoid by
            # a few fp32 ulps: such an element might round the other way in the kernel) -- on the reference alone
            xv, nwv = P["x"][..., cols["x"][0]:cols["x"][1]], P["norm_weight"]
            for _ in range(8):
                m = near_bf16_midpoint(exact_u(r, xv, None, z, nwv))
                if not m.any():
                    break
                z[m] = rn(gs, int(m.sum())).to(r.x)
        put("z", z.float(), r.x)
    put("out", torch.full((r.B, r.Out), NAN), r.odt, 3 if r.strided else 0, 5 if r.strided else 0)
    if r.ro is not None:
        put("residual_out", torch.full((r.B, r.In), NAN), r.ro)
    P["_cols"] = cols
    return P


def conv_state_of(r, P):
    """The conv_state argument: (rows, C, S) over the channel-contiguous pool; without indices the pool's rows 1 .. B."""
    st = view(P, "pool").transpose(1, 2)
    return st if r.idx is not None else st[1:r.B + 1]


def slots_of(r):
    """Pool row of every sequence (None: a padding sequence)."""
    if r.idx is None:
        return [b + 1 for b in range(r.B)]
    return [s if 0 <= s < r.pool else None for s in r.idx]


def kwargs_of(r, P):
    kw = dict(norm_weight=view(P, "norm_weight"), eps=EPS, residual=view(P, "residual"), z=view(P, "z"), out=view(P, "out"),
              residual_out=view(P, "residual_out"), norm_before_gate=r.nbg)
    if r.G > 1:
        kw["group_size"] = r.In // r.G
    if r.R:
        kw.update(lora_a=view(P, "lora_a"), lora_b=view(P, "lora_b"), lora_scale=SCALE)
    if r.conv:
        kw.update(conv_state=conv_state_of(r, P), conv_weight=view(P, "conv_weight"), conv_bias=view(P, "conv_bias"), conv_offset=r.conv[2],
                  conv_silu=r.silu, conv_state_indices=P.get("idx"))
    return (view(P, "x"), view(P, "weight"), view(P, "bias")), kw


# ------------------------------------------------------------------------------------------------------------------------------
# the fp64 reference
# ------------------------------------------------------------------------------------------------------------------------------
def reference(r, P):
    """(out before the conv tail, unrounded fp64 (B, Out); residual_out as the kernel must store it, or None)."""
    d = lambda k: None if view(P, k) is None else view(P, k).double()
    x, res, z, nw, W, bias = d("x"), d("residual"), d("z"), d("norm_weight"), d("weight"), d("bias")
    s = x if res is None else x + res
    g = None if z is None else z * torch.sigmoid(z)
    q = s * g if (g is not None and not r.nbg) else s
    if nw is None:
        u, rstd = q if (g is None or not r.nbg) else q * g, torch.ones(r.B, 1, dtype=torch.float64)
    else:
        rstd = torch.rsqrt((q * q).view(r.B, r.G, -1).mean(-1) + EPS)
        u = q * nw if (g is None or not r.nbg) else q * nw * g
        if rounded_u(r):
            # the kernel's u: fp32, its order of operations -- (x + res) * w, x * g * w, or x * w * g under norm_before_gate -- rounded to bf16
            xf, nf = view(P, "x").float(), view(P, "norm_weight").float()
            if g is None:
                u32 = (xf if res is None else xf + view(P, "residual").float()) * nf
            else:
                zf = view(P, "z").float()
                gf = zf * torch.sigmoid(zf)
                u32 = xf * nf * gf if r.nbg else xf * gf * nf
                assert not near_bf16_midpoint(u).any(), "a gated element of u lies next to a bf16 rounding midpoint"
            u = u32.to(BF16).double()
    un = (u.view(r.B, rstd.shape[1], -1) * rstd[:, :, None]).view(r.B, r.In)
    out = un @ W.t()
    if r.R:
        out = out + SCALE * (un @ d("lora_a").t()) @ d("lora_b").t()
    if bias is not None:
        out = out + bias
    ro = None
    if r.ro is not None:
        xf = view(P, "x").float()
        ro = (xf if res is None else xf + view(P, "residual").float()).to(r.ro)
    return out, ro


def same_bits(a, b):
    """torch.equal with NaN == NaN (the parents' margins)."""
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(torch.nan_to_num(a.float(), nan=12345.0), torch.nan_to_num(b.float(), nan=12345.0))


def margins_are_nan(P, k):
    a, b = P["_cols"][k]
    p = P[k]
    return bool(p[..., :a].isnan().all()) and bool(p[..., b:].isnan().all())


# ------------------------------------------------------------------------------------------------------------------------------
# one row
# ------------------------------------------------------------------------------------------------------------------------------
def check_row(r, cpu, dev_P, report):
    """Everything the call on dev_P (the copies of the parents `cpu`, after the call, back on the CPU) must satisfy."""
    out64, ro_want = reference(r, cpu)
    got = view(dev_P, "out")
    assert got.dtype == r.odt and torch.isfinite(got).all(), "an output element was not written, or an element outside a view was used"
    shares = {}

    def check(name, g3, r3, sizes, dtype):
        e, q, b, share = slice_check(f"{r.name} {name}", g3, r3, dtype, 2, sizes=sizes)
        report.append(f"{name} {e / b:.3f} floor {share:.3f}")
        shares[name] = share

    if r.ro is not None:
        assert torch.equal(view(dev_P, "residual_out"), ro_want), "residual_out is not the one rounding of x + residual"
    if not r.conv:
        check("out", *column_blocks(got, out64, 0, r.Out), r.odt)
    else:
        W, S, off, C = r.conv
        slots = slots_of(r)
        live = [b for b in range(r.B) if slots[b] is not None]
        dead = [b for b in range(r.B) if slots[b] is None]
        before, after = view(cpu, "pool"), view(dev_P, "pool")                      # (rows, S, C)
        used = [slots[b] for b in live]
        for p_ in range(r.pool):
            if p_ not in used:
                assert same_bits(dev_P["pool"][p_], cpu["pool"][p_]), f"pool row {p_}, which no sequence addresses, was written"
        for b in dead:
            assert bool((got[b, off:off + C] == 0).all()), f"conv columns of padding sequence {b} are not zeros"
        # outside the conv range: every sequence, padding ones included
        parts = [column_blocks(got, out64, lo, hi) for lo, hi in ((0, off), (off + C, r.Out)) if lo < hi]
        if parts:
            check("out", torch.cat([t[0] for t in parts], 1), torch.cat([t[1] for t in parts], 1), torch.cat([t[2] for t in parts]), r.odt)
        if live:
            new = torch.stack([after[slots[b], S - 1] for b in live])                   # (live, C): the newest column as stored
            proj = out64[live][:, off:off + C]
            check("newest", *column_blocks(new, proj, 0, C), r.w)
            for b in live:
                assert torch.equal(after[slots[b], :S - 1], before[slots[b], 1:]), f"sequence {b}: the rolled conv-state columns are not raw copies"
            cw, cb = view(cpu, "conv_weight").double(), view(cpu, "conv_bias")
            old = torch.stack([before[slots[b]] for b in live]).double()                # (live, S, C)
            cv = new.double() * cw[:, W - 1]
            for j in range(W - 1):
                cv = cv + old[:, S - (W - 1) + j] * cw[:, j]
            if cb is not None:
                cv = cv + cb.double()
            want = cv * torch.sigmoid(cv) if r.silu else cv
            full = torch.zeros(len(live), r.Out, dtype=torch.float64)
            full[:, off:off + C] = want
            check("conv", *column_blocks(got[live], full, off, off + C, align=off), r.odt)
    assert max(shares.values(), default=0.0) <= 0.05, f"more than 5 % of the slices met the floor: {shares}"
    # the kernel writes out, residual_out and the pool, nothing else; the margins of every parent are still NaN
    for k in cpu["_cols"]:
        if k not in ("out", "residual_out", "pool"):
            assert same_bits(dev_P[k], cpu[k]), f"operand {k} was written"
        assert margins_are_nan(dev_P, k), f"an element of {k}'s parent outside the view was written"


@pytest.mark.parametrize("case", [pytest.param(k, id=rid(r)) for k, r in ROWS.items()])
def test_norm_linear_slices(dev, monkeypatch, case):
    from omnimamba_amd import norm_linear as NL
    r = ROWS[case]
    if r.wgs:
        monkeypatch.setenv("OMK_NL_MFMA_WGS", str(r.wgs))
    else:
        monkeypatch.delenv("OMK_NL_MFMA_WGS", raising=False)
    want_form = {"generic": NL.GENERIC, "fast": NL.FAST, "batched": NL.BATCHED, "matrix": NL.MATRIX}
    assert plan(r)[0] == r.form, "the row's parameters do not belong to the form it names"
    pool = None
    for step in range(r.steps):
        cpu = make_inputs(r, step)
        if r.conv and step:
            cpu["pool"], cpu["_cols"]["pool"] = pool, pool_cols                      # the state the step before left
        P = {k: (v if k == "_cols" else v.to(dev, copy=True)) for k, v in cpu.items()}
        args, kw = kwargs_of(r, P)
        if r.strided:
            assert all(t.stride(0) > t.shape[1] for t in (args[0], args[1], kw["out"]))
        got_form = NL.form(*args, **kw)
        if NL.applies(args[0], args[1], kw["norm_weight"], *[t for t in (kw["z"], kw.get("lora_a"), args[2]) if t is not None]):
            assert got_form >= 0, "applies() says yes and the library refuses the call"
        assert got_form == want_form[r.form], f"reaches {NL.FORM_NAMES.get(got_form, got_form)}, meant for {r.form}"
        NL.norm_linear(*args, **kw)
        back = {k: (v if k == "_cols" else v.cpu()) for k, v in P.items()}
        report = []
        check_row(r, cpu, back, report)
        print(f"\n[norm-linear-slices] {rid(r)} {dev.type} step {step}: worst slice / bound  " + "  ".join(report))
        if r.conv:
            pool, pool_cols = back["pool"], cpu["_cols"]["pool"]


# ------------------------------------------------------------------------------------------------------------------------------
# the table covers every cell of the list it was written from
# ------------------------------------------------------------------------------------------------------------------------------
def _cells():
    C = []
    cell = lambda name, pred: C.append((name, pred))
    P = {k: plan(r) for k, r in ROWS.items()}
    f = lambda form: (lambda r: r.form == form)
    both = lambda a, b: (lambda r: a(r) and b(r))
    for form in ("generic", "fast", "batched", "matrix"):
        cell(f"{form}: contiguous", both(f(form), lambda r: not r.strided))
        cell(f"{form}: strided", both(f(form), lambda r: r.strided))
    G = f("generic")
    for w in (F32, BF16, F16):
        cell(f"generic: weights {NAME[w]}", both(G, lambda r, w=w: r.w == w))
    cell("generic: out_dtype different from x", both(G, lambda r: r.odt != r.x))
    cell("generic: mixed x / residual / norm weight / bias / LoRA dtypes", both(G, lambda r: len({r.x, r.res, r.nw, r.bias, r.ldt, r.w} - {None}) >= 3))
    for In in (1024, 3072, 8192):
        cell(f"generic: In {In}", both(G, lambda r, In=In: r.In == In))
    cell("generic: no norm weight", both(G, lambda r: r.nw is None))
    for Gn in (1, 2, 4, 8):
        for nbg in ((False, True) if Gn != 4 else (False,)):
            cell(f"generic: gate G {Gn} nbg {nbg}", both(G, lambda r, Gn=Gn, nbg=nbg: r.gate and r.G == Gn and r.nbg == nbg))
    cell("generic: grouped norm with 16-bit inputs", both(G, lambda r: r.G > 1 and r.x != F32))
    for R in (1, 8, 9, 16):
        cell(f"generic: LoRA rank {R}", both(G, lambda r, R=R: r.R == R))
    cell("generic: residual with residual_out", both(G, lambda r: r.res is not None and r.ro is not None))
    cell("generic: residual_out alone", both(G, lambda r: r.res is None and r.ro is not None))
    for Out in (1, 7, 8, 9):
        cell(f"generic: Out {Out}", both(G, lambda r, Out=Out: r.Out == Out))
    Fa = f("fast")
    for w in (F32, BF16):
        for res in ((F32, None) if w == F32 else (F32, BF16, None)):
            for nq in (1, 2, 4):
                cell(f"fast: {NAME[w]} residual {NAME[res]} NQ {nq}", both(Fa, lambda r, w=w, res=res, nq=nq: r.w == w and r.res == res and r.In == 1024 * nq))
    for R in (0, 1, 3, 7, 8):
        cell(f"fast: LoRA rank {R}", both(Fa, lambda r, R=R: r.R == R))
    for nbg in (False, True):
        cell(f"fast: gate nbg {nbg}", both(Fa, lambda r, nbg=nbg: r.gate and r.nbg == nbg))
    for b in (False, True):
        cell(f"fast: bias {b}", both(Fa, lambda r, b=b: (r.bias is not None) == b))
        cell(f"fast: conv_bias {b}", both(Fa, lambda r, b=b: r.conv and r.cbias == b))
        cell(f"fast: conv_silu {b}", both(Fa, lambda r, b=b: r.conv and r.silu == b))
    for ws in CONVS:
        cell(f"fast: conv (W, S) {ws}", both(Fa, lambda r, ws=ws: r.conv and r.conv[:2] == ws))
    cell("fast: conv offset 0", both(Fa, lambda r: r.conv and r.conv[2] == 0))
    cell("fast: conv range ends at Out", both(Fa, lambda r: r.conv and r.conv[2] + r.conv[3] == r.Out))
    cell("fast: two steps on one state", both(Fa, lambda r: r.conv and r.steps == 2))
    cell("fast: single-row pool through indices", both(Fa, lambda r: r.conv and r.idx == [0] and r.pool == 1))
    cell("fast: pool larger than the batch through indices", both(Fa, lambda r: r.conv and r.idx is not None and r.pool > 1 and r.idx[0] >= 0))
    cell("fast: negative index", both(Fa, lambda r: r.conv and r.idx is not None and r.idx[0] < 0))
    cell("fast: index past the pool", both(Fa, lambda r: r.conv and r.idx is not None and r.idx[0] >= r.pool))
    for k in (2, 3):
        cell(f"fast: nbatch {k}", both(Fa, lambda r, k=k: P[r.name][8] == k))
    cell("fast: nbatch 2 under bf16", both(Fa, lambda r: P[r.name][8] == 2 and r.w == BF16))
    Ba = f("batched")
    for w in (F32, BF16):
        for B in range(2, 9):
            cell(f"batched: {NAME[w]} B {B}", both(Ba, lambda r, w=w, B=B: r.w == w and r.B == B))
        for nq in (1, 2, 4):
            cell(f"batched: {NAME[w]} NQ {nq}", both(Ba, lambda r, w=w, nq=nq: r.w == w and r.In == 1024 * nq))
        for nb in (2, 4, 8):
            cell(f"batched: {NAME[w]} NB {nb}", both(Ba, lambda r, w=w, nb=nb: r.w == w and P[r.name][5] == nb))
        cell(f"batched: {NAME[w]} gate", both(Ba, lambda r, w=w: r.w == w and r.gate and not r.nbg))
        cell(f"batched: {NAME[w]} gate nbg", both(Ba, lambda r, w=w: r.w == w and r.gate and r.nbg))
        cell(f"batched: {NAME[w]} conv with pool, indices and a padding sequence in the middle",
             both(Ba, lambda r, w=w: r.w == w and r.conv and r.idx is not None and None in slots_of(r)[1:-1] and r.pool > r.B))
        cell(f"batched: {NAME[w]} nbatch 2", both(Ba, lambda r, w=w: r.w == w and P[r.name][8] == 2))
    for res in (F32, BF16, None):
        cell(f"batched: bf16 residual {NAME[res]}", both(Ba, lambda r, res=res: r.w == BF16 and r.res == res and not r.gate))
    for res in (F32, None):
        cell(f"batched: f32 residual {NAME[res]}", both(Ba, lambda r, res=res: r.w == F32 and r.res == res and not r.gate))
    for R in (0, 4, 7):
        cell(f"batched: LoRA rank {R}", both(Ba, lambda r, R=R: r.R == R))
    cell("batched: bf16 LoRA rank 8 with unaligned rows", both(Ba, lambda r: r.w == BF16 and r.R == 8 and r.lb_unaligned))
    Ma = f("matrix")
    for B in range(2, 9):
        for nq in (1, 2, 4):
            cell(f"matrix: bf16 B {B} NQ {nq}", both(Ma, lambda r, B=B, nq=nq: r.w == BF16 and r.B == B and r.In == 1024 * nq))
    for nq in (1, 2):
        cell(f"matrix: f32 eight sequences with LoRA NQ {nq}", both(Ma, lambda r, nq=nq: r.w == F32 and r.B == 8 and r.R == 8 and r.In == 1024 * nq))
    for w in (F32, BF16):
        for rows_ in (8, 16):
            cell(f"matrix: {NAME[w]} ROWS {rows_}", both(Ma, lambda r, w=w, rows_=rows_: r.w == w and P[r.name][7] == rows_))
        cell(f"matrix: {NAME[w]} conv with indices and padding", both(Ma, lambda r, w=w: r.w == w and r.conv and r.idx is not None and None in slots_of(r)))
        cell(f"matrix: {NAME[w]} gate", both(Ma, lambda r, w=w: r.w == w and r.gate))
    for k in (1, 2, 3):
        for rows_ in (8, 16):
            if (k, rows_) != (3, 8):
                cell(f"matrix: {k} tiles per workgroup, ROWS {rows_}", both(Ma, lambda r, k=k, rows_=rows_: P[r.name][8] == k and P[r.name][7] == rows_))
    cell("matrix: last tile of 1 row", both(Ma, lambda r: r.Out % P[r.name][7] == 1))
    cell("matrix: Out smaller than one tile", both(Ma, lambda r: r.Out < 8))
    cell("matrix: gate nbg", both(Ma, lambda r: r.gate and r.nbg))
    for res in (F32, BF16, None):
        cell(f"matrix: bf16 residual {NAME[res]}", both(Ma, lambda r, res=res: r.w == BF16 and r.res == res and not r.gate))
    for R in (0, 8):
        cell(f"matrix: bf16 LoRA rank {R}", both(Ma, lambda r, R=R: r.w == BF16 and r.R == R))
    for nb in (2, 4, 8):
        for gate in (False, True):
            cell(f"matrix: bf16 NB {nb} gate {gate}", both(Ma, lambda r, nb=nb, gate=gate: r.w == BF16 and P[r.name][5] == nb and r.gate == gate))
    return C


def test_table_covers_every_cell():
    """Every cell of the list the table was written from has a row (so a dropped row fails), and every row belongs to the form it names."""
    missing = [name for name, pred in _cells() if not any(pred(r) for r in ROWS.values())]
    assert not missing, missing
    for r in ROWS.values():
        assert plan(r)[0] == r.form, r.name
