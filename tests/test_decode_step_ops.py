"""The two kernels every generated token goes through, omk_selective_state_update and omk_causal_conv1d_update, over every branch of
their dispatch: emulator on CPU, MI355X under -m gpu.

Reference: the fp64 recurrence (oracle.selective_state_update_ref with compute_dtype=float64 on an fp64 copy of the initial state; for the
convolution an fp64 window dot product written here), built from exactly the tensors the kernel reads, already rounded to their storage
dtypes.  Bound: tolerances.op_bound with the project's OP_ARITH, per slice -- y and the new state per (batch, head), the convolution's
output per (batch, block of 64 channels); the new convolution state is a copy and must be bit-exact.

Guards: the state is rows 1 .. B of a pool of B + 2 rows whose other rows must come back bit-unchanged.  Where operands are views, they are
column slices of one NaN-filled row per sequence, laid out as Mamba2.step_from_zxbcdt slices xBC and dt out of zxbcdt:

    [ off | x: H P | pad | B: G N | C: G N | dt: H | 8 | pad ]

(the two pads, 0 .. 3 columns of NaN each, exist only where H P or the row length is no multiple of 4: the first makes B start at
column off mod 4 so that `off` alone decides the alignment of B / C, the second keeps the row stride a multiple of 4; at the production
shapes both are empty).  off = 8 keeps the vector path, off = 3 or 1 forces the element-wise kernel.  A kernel that uses an element
outside its view produces a NaN and fails.

Every case names the kernel it is meant to reach; su_branch below repeats the library's dispatch on the very tensors of the call and the
test asserts that the two agree, so that a change of the dispatch cannot silently move a case to another kernel.

Each case prints its worst slice as a fraction of the bound (`pytest -s`)."""
from types import SimpleNamespace

import pytest
import torch

import oracle as O
from tolerances import op_bound, rel

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
NAME = {F32: "f32", BF16: "bf16", F16: "f16"}


def on(t, dev):
    """A copy on `dev` with the same strides (on the emulator `dev` is the CPU: .to() alone would hand the kernel the reference's tensor)."""
    return None if t is None else t.to(dev, copy=True)


# ------------------------------------------------------------------------------------------------------------------------------
# selective_state_update: inputs
# ------------------------------------------------------------------------------------------------------------------------------
def su_case(branch, Bsz, H, P, N, G, sdt, xdt, pdt=F32, tied=True, opts="zDb", mode="softplus", off=None, d_hp=False, seed=0):
    """opts: which of z, D, dt_bias (b) are passed.  mode: 'softplus' (dt, dt_bias standard normal), 'thresh' (dt 15 x standard normal:
    dt + dt_bias spans about -40 .. +40, past softplus's pass-through threshold on one side and into exp's underflow on the other),
    'plain' (dt_softplus=False, dt in 0.05 .. 1.05 and dt_bias >= 0).  off: None for contiguous operands, else x / B / C / dt are views
    (module docstring).  tied: A, dt, D, dt_bias are stride-0 expansions of per-head tensors (d_hp: D a real (H, P)); else (H, P[, N])."""
    return SimpleNamespace(branch=branch, Bsz=Bsz, H=H, P=P, N=N, G=G, sdt=sdt, xdt=xdt, pdt=pdt, tied=tied, opts=opts, mode=mode, off=off,
                           d_hp=d_hp, seed=seed)


def view_cols(c):
    """Column offsets (x, B, C, dt) and the row length of the view layout."""
    HP, GN = c.H * c.P, c.G * c.N
    ox = c.off
    oB = ox + HP + (-HP) % 4
    oC = oB + GN
    odt = oC + GN
    end = odt + c.H + 8
    return ox, oB, oC, odt, end + (-end) % 4


def su_bases(c):
    """The tensors that own memory, on the CPU.  su_operands turns them (or their copies on a device) into the call's operands."""
    g = torch.Generator().manual_seed(c.seed)
    r = lambda *s: torch.randn(*s, generator=g)
    u = lambda *s: torch.rand(*s, generator=g)
    Bsz, H, P, N, G = c.Bsz, c.H, c.P, c.N, c.G
    b = {"pool": r(Bsz + 2, H, P, N).to(c.sdt)}
    x, Bm, Cm = r(Bsz, H * P), r(Bsz, G * N), r(Bsz, G * N)
    dt = r(Bsz, H) if (c.tied or c.off is not None) else r(Bsz, H, P)      # a view of zxbcdt has one dt per head
    if c.mode == "thresh":
        dt = dt * 15
    elif c.mode == "plain":
        dt = u(*dt.shape) + 0.05
    if c.off is None:
        b["x"], b["B"], b["C"], b["dt"] = x.to(c.xdt), Bm.to(c.xdt), Cm.to(c.xdt), dt.to(c.xdt)
    else:
        ox, oB, oC, odt, width = view_cols(c)
        buf = torch.full((Bsz, width), float("nan"))
        buf[:, ox:ox + H * P], buf[:, oB:oB + G * N], buf[:, oC:oC + G * N], buf[:, odt:odt + H] = x, Bm, Cm, dt
        b["buf"] = buf.to(c.xdt)
    if "z" in c.opts:
        b["z"] = r(Bsz, H, P).to(c.xdt)
    b["A"] = (-(1 + 15 * u(H)) if c.tied else -(0.1 + u(H, P, N))).to(c.pdt)
    if "D" in c.opts:
        b["D"] = (r(H) if (c.tied and not c.d_hp) else r(H, P)).to(c.pdt)
    if "b" in c.opts:
        tb = r(H) if c.tied else r(H, P)
        b["dt_bias"] = (tb.abs() if c.mode == "plain" else tb).to(c.pdt)
    return b


def su_operands(c, b, rows=None):
    """rows: use the first `rows` sequences only (their state is pool rows 1 .. rows)."""
    Bsz, H, P, N, G = c.Bsz, c.H, c.P, c.N, c.G
    n = Bsz if rows is None else rows
    if c.off is None:
        x, Bm, Cm, dt = b["x"].view(Bsz, H, P), b["B"].view(Bsz, G, N), b["C"].view(Bsz, G, N), b["dt"]
    else:
        ox, oB, oC, odt, _ = view_cols(c)
        buf = b["buf"]
        x, Bm, Cm = buf[:, ox:ox + H * P].view(Bsz, H, P), buf[:, oB:oB + G * N].view(Bsz, G, N), buf[:, oC:oC + G * N].view(Bsz, G, N)
        dt = buf[:, odt:odt + H]
    if dt.dim() == 2:
        dt = dt[:, :, None].expand(Bsz, H, P)
    A, D, tb, z = b["A"], b.get("D"), b.get("dt_bias"), b.get("z")
    if A.dim() == 1:
        A = A[:, None, None].expand(H, P, N)
    if D is not None and D.dim() == 1:
        D = D[:, None].expand(H, P)
    if tb is not None and tb.dim() == 1:
        tb = tb[:, None].expand(H, P)
    return SimpleNamespace(state=b["pool"][1:n + 1], x=x[:n], dt=dt[:n], A=A, B=Bm[:n], C=Cm[:n], D=D, z=None if z is None else z[:n], dt_bias=tb)


def su_branch(o):
    """The kernel omk_selective_state_update picks for these operands (its dispatch, repeated on the tensors of the call)."""
    Bsz, H, P, N = o.state.shape
    aligned = lambda t: t.data_ptr() % (4 * t.element_size()) == 0
    strides = o.state.stride()[:3] + o.B.stride()[:2] + o.C.stride()[:2]
    vec = (N % 4 == 0 and o.state.stride(3) == 1 and o.B.stride(2) == 1 and o.C.stride(2) == 1 and aligned(o.state) and aligned(o.B)
           and aligned(o.C) and all(s % 4 == 0 for s in strides))
    lpr = N // 4
    tied = (vec and o.A.stride(2) == 0 and o.A.stride(1) == 0 and o.dt.stride(2) == 0 and (o.dt_bias is None or o.dt_bias.stride(1) == 0)
            and lpr in (16, 32) and Bsz * H * P * N >= 2 ** 21)
    if tied and P % ((64 // lpr) * 16) == 0:
        return f"tied/LPR{lpr}"
    if not vec:
        return "row/VEC1"
    return "row/VEC4/LPR32" if N >= 128 else ("row/VEC4/LPR16" if N >= 64 else "row/VEC4/LPR4")


# ------------------------------------------------------------------------------------------------------------------------------
# selective_state_update: run and check
# ------------------------------------------------------------------------------------------------------------------------------
def worst_ratio(got, ref, dtype, slices):
    """max over the slices of rel(slice, ref slice) / op_bound(ref slice, dtype)."""
    worst = 0.0
    for ix in slices:
        worst = max(worst, rel(got[ix], ref[ix]) / op_bound(ref[ix], dtype))
    return worst


def run_su(c, dev, name, rows=None):
    """One call of the kernel on `dev` against the fp64 recurrence; returns (y, new state) on the CPU."""
    from omnimamba_amd.selective_state_update import selective_state_update
    cpu = su_bases(c)
    bases = {k: on(v, dev) for k, v in cpu.items()}
    o = su_operands(c, bases, rows)
    assert su_branch(o) == c.branch, "the case does not reach the kernel it names"
    soft = c.mode != "plain"
    y = selective_state_update(o.state, o.x, o.dt, o.A, o.B, o.C, D=o.D, z=o.z, dt_bias=o.dt_bias, dt_softplus=soft)
    r = su_operands(c, cpu, rows)
    dbl = lambda t: None if t is None else t.double()
    s64 = r.state.double().clone()
    y64 = O.selective_state_update_ref(s64, r.x.double(), r.dt.double(), r.A.double(), r.B.double(), r.C.double(), D=dbl(r.D), z=dbl(r.z),
                                       dt_bias=dbl(r.dt_bias), dt_softplus=soft, compute_dtype=torch.float64)
    y, pool = y.cpu(), bases["pool"].cpu()
    n = r.state.shape[0]
    new = pool[1:n + 1]
    assert y.dtype == c.xdt and y.shape == r.x.shape
    assert torch.isfinite(y).all() and torch.isfinite(new).all(), "an element outside a view was used"
    slices = [(b, h) for b in range(n) for h in range(c.H)]
    ry, rs = worst_ratio(y, y64, c.xdt, slices), worst_ratio(new, s64, c.sdt, slices)
    print(f"\n[decode-step-ops] {c.branch:15s} {name}: worst slice / bound  y {ry:.3f}  state {rs:.3f}")
    assert ry <= 1.0, f"y: worst (batch, head) slice at {ry:.3f} of op_bound"
    assert rs <= 1.0, f"state: worst (batch, head) slice at {rs:.3f} of op_bound"
    assert torch.equal(pool[0], cpu["pool"][0]) and torch.equal(pool[n + 1:], cpu["pool"][n + 1:]), "a pool row outside the batch was written"
    for k in ("x", "B", "C", "dt", "buf", "z", "A", "D", "dt_bias"):                      # the kernel writes the state and y, nothing else
        if k in cpu:
            got, want = bases[k].cpu(), cpu[k]
            assert torch.equal(torch.nan_to_num(got.float(), nan=7.0), torch.nan_to_num(want.float(), nan=7.0)), f"operand {k} was written"
    return y, new


# ---- the row kernel (state_update_kernel): one row per dispatch branch, crossed with the axes below -----------------------------------
ROWS = [  # (id, (H, P, N, G), kernel, view offsets the branch allows)
    ("v4l32-1step-deadrows", (2, 5, 128, 1), "row/VEC4/LPR32", (None, 8)),
    ("v4l32-2steps", (2, 9, 256, 1), "row/VEC4/LPR32", (None, 8)),
    ("v4l32-2steps-partial", (2, 9, 192, 2), "row/VEC4/LPR32", (None, 8)),
    ("v4l16", (2, 9, 64, 2), "row/VEC4/LPR16", (None, 8)),
    ("v4l4-2steps", (3, 17, 20, 1), "row/VEC4/LPR4", (None, 8)),
    ("v4l4-clamped", (3, 17, 12, 1), "row/VEC4/LPR4", (None, 8)),
    ("v1-n6", (3, 7, 6, 1), "row/VEC1", (None, 8, 3)),            # N % 4 != 0: element-wise whatever the alignment
    ("v1-viewoff", (2, 9, 64, 2), "row/VEC1", (3, 1)),             # N 64 would take VEC 4 / LPR 16: B / C start off 4-element alignment
]
DTYPES = [(F32, F32), (F32, BF16), (BF16, BF16), (F16, F16), (F32, F16)]     # (state, activations)
PDTYPES = [F32, BF16, F16]                                                    # A, D, dt_bias
OPTS = ["zDb", "", "Db"]                                                      # all, none, the production set (gate applied by the fused norm)
MODES = ["softplus", "plain", "thresh"]
PER_ROW = 6


def row_cases():
    """Six cases per row of ROWS, the axes cycled at different periods and shifted by the row's index: within a row every value of every
    axis occurs (test_row_cases_cover_every_axis), across rows the pairs vary.  An unaligned view would move a VEC 4 row to the
    element-wise kernel, so those rows alternate between contiguous operands and the aligned view; the element-wise rows take the rest."""
    out = []
    for r, (rid, (H, P, N, G), branch, offs) in enumerate(ROWS):
        for j in range(PER_ROW):
            sdt, xdt = DTYPES[(j + r) % 5]
            tied = (j // 3 + r) % 2 == 0
            c = su_case(branch, 2 + (j + r) % 2, H, P, N, G, sdt, xdt, pdt=PDTYPES[j % 3], tied=tied, opts=OPTS[(j // 2 + r) % 3],
                        mode=MODES[(2 * j + r) % 3], off=offs[(j + j // 3) % len(offs)], d_hp=j % 2 == 1, seed=100 * r + j)
            cid = (f"{rid}-{NAME[sdt]}/{NAME[xdt]}-{'tied' if tied else 'untied'}-p{NAME[c.pdt]}-{c.opts or 'noopt'}-{c.mode}-"
                   f"{'contig' if c.off is None else 'view%d' % c.off}")
            out.append(pytest.param(c, cid, id=cid))
    return out


def test_row_cases_cover_every_axis():
    """Every row of ROWS meets every value of each axis at least once (layouts: the ones its branch allows)."""
    cases = [p.values[0] for p in row_cases()]
    for r, (rid, _, branch, offs) in enumerate(ROWS):
        mine = cases[r * PER_ROW:(r + 1) * PER_ROW]
        assert all(c.branch == branch for c in mine)
        assert {(c.sdt, c.xdt) for c in mine} == set(DTYPES), rid
        assert {c.pdt for c in mine} == set(PDTYPES), rid
        assert {c.tied for c in mine} == {True, False}, rid
        assert {c.opts for c in mine} == set(OPTS), rid
        assert {c.mode for c in mine} == set(MODES), rid
        assert {c.off for c in mine} == set(offs), rid
        assert {c.Bsz for c in mine} == {2, 3}, rid
    assert any(c.tied and c.d_hp and "D" in c.opts for c in cases)


@pytest.mark.parametrize("c,name", row_cases())
def test_state_update_row_kernel(dev, c, name):
    run_su(c, dev, name)


@pytest.mark.parametrize("sdt,xdt", [(F32, BF16), (F16, F16)])
def test_state_update_no_heads_16bit(dev, sdt, xdt):
    """Mamba-1's layout: state (B, dim, N), A (dim, N), dt_bias and z present, no D, 16-bit activations."""
    from omnimamba_amd.selective_state_update import selective_state_update
    g = torch.Generator().manual_seed(7)
    r = lambda *s: torch.randn(*s, generator=g)
    Bsz, Dm, N = 3, 40, 16
    pool0 = r(Bsz + 2, Dm, N).to(sdt)
    x, dt, z = r(Bsz, Dm).to(xdt), r(Bsz, Dm).to(xdt), r(Bsz, Dm).to(xdt)
    A, Bm, Cm, tb = -(0.1 + torch.rand(Dm, N, generator=g)), r(Bsz, N).to(xdt), r(Bsz, N).to(xdt), r(Dm)
    pool = on(pool0, dev)
    y = selective_state_update(pool[1:Bsz + 1], on(x, dev), on(dt, dev), on(A, dev), on(Bm, dev), on(Cm, dev), z=on(z, dev), dt_bias=on(tb, dev),
                               dt_softplus=True)
    s64 = pool0[1:Bsz + 1].double().clone()
    y64 = O.selective_state_update_ref(s64, x.double(), dt.double(), A.double(), Bm.double(), Cm.double(), z=z.double(), dt_bias=tb.double(),
                                       dt_softplus=True, compute_dtype=torch.float64)
    y, pool = y.cpu(), pool.cpu()
    assert y.shape == x.shape and y.dtype == xdt
    rows = [(b,) for b in range(Bsz)]
    ry, rs = worst_ratio(y, y64, xdt, rows), worst_ratio(pool[1:Bsz + 1], s64, sdt, rows)
    print(f"\n[decode-step-ops] row/VEC4/LPR4   no-heads-{NAME[sdt]}/{NAME[xdt]}: worst slice / bound  y {ry:.3f}  state {rs:.3f}")
    assert ry <= 1.0 and rs <= 1.0, (ry, rs)
    assert torch.equal(pool[0], pool0[0]) and torch.equal(pool[Bsz + 1], pool0[Bsz + 1])


# ---- the tied-rows kernel (state_update_tied_kernel): B H P N >= 2^21, the smallest shapes that reach it ------------------------------
PRODUCTION = dict(Bsz=4, H=64, P=64, N=128, G=2, opts="Db", seed=11)
TIED = [
    ("lpr32-production-g2", su_case("tied/LPR32", sdt=BF16, xdt=BF16, **PRODUCTION)),
    ("lpr32-no-options", su_case("tied/LPR32", 4, 64, 64, 128, 1, F32, BF16, opts="", seed=12)),
    ("lpr32-views-Dhp-f16", su_case("tied/LPR32", 4, 64, 64, 128, 1, F16, F16, pdt=F16, opts="Db", off=8, d_hp=True, seed=13)),
    ("lpr16-all-options", su_case("tied/LPR16", 8, 64, 64, 64, 1, F32, F32, opts="zDb", seed=14)),
    ("p96-three-passes", su_case("tied/LPR32", 3, 64, 96, 128, 1, BF16, BF16, pdt=BF16, opts="zDb", seed=15)),
    ("p48-falls-through", su_case("row/VEC4/LPR32", 6, 64, 48, 128, 1, BF16, BF16, opts="Db", seed=16)),   # 48 % 32 != 0: the row kernel
]


@pytest.mark.parametrize("name,c", TIED, ids=[t[0] for t in TIED])
def test_state_update_tied_kernel(dev, name, c):
    run_su(c, dev, name)


def test_state_update_both_kernels_same_bits(dev):
    """The production case with an fp32 state and fp32 activations, and its first two sequences alone: half the elements, just under the
    2^21 threshold, so the row kernel.  Both kernels evaluate the same expression in the same order: y and the state are bit-equal."""
    big = su_case("tied/LPR32", sdt=F32, xdt=F32, **PRODUCTION)
    small = su_case("row/VEC4/LPR32", sdt=F32, xdt=F32, **PRODUCTION)
    y4, s4 = run_su(big, dev, "production-f32-4-sequences")
    y2, s2 = run_su(small, dev, "production-f32-first-2-sequences", rows=2)
    assert torch.equal(y2, y4[:2]), "y of the row kernel and of the tied-rows kernel differ"
    assert torch.equal(s2, s4[:2]), "state of the row kernel and of the tied-rows kernel differ"


def test_state_update_refuses_bad_shapes(dev):
    from omnimamba_amd.selective_state_update import selective_state_update
    Bsz, H, P, N = 2, 3, 4, 8
    t = lambda *s: torch.zeros(*s, device=dev)
    with pytest.raises(RuntimeError):                  # H 3 is no multiple of G 2
        selective_state_update(t(Bsz, H, P, N), t(Bsz, H, P), t(Bsz, H, P), t(H, P, N), t(Bsz, 2, N), t(Bsz, 2, N))
    with pytest.raises(RuntimeError):                  # x's P differs from the state's
        selective_state_update(t(Bsz, H, P, N), t(Bsz, H, P + 1), t(Bsz, H, P + 1), t(H, P, N), t(Bsz, 1, N), t(Bsz, 1, N))


# ------------------------------------------------------------------------------------------------------------------------------
# causal_conv1d_update
# ------------------------------------------------------------------------------------------------------------------------------
CONV = [  # id, B, C, W, S, T, (x, state, weight) dtypes, activation, bias, layout of the state, layout of x
    ("workgroups-production", 3, 200, 4, 4, 1, (BF16, BF16, BF16), "silu", True, "channel-last", "column-slice"),
    ("w3-minimal-state", 3, 200, 3, 2, 1, (F16, F16, F16), "silu", False, "channel-first", "contig"),
    ("w2-long-state-3-tokens", 2, 300, 2, 4, 3, (F32, F32, F32), None, True, "channel-first", "contig"),
    ("t6-longer-than-state", 2, 130, 4, 3, 6, (BF16, BF16, F32), "silu", True, "channel-last", "column-slice"),
]


@pytest.mark.parametrize("name,Bsz,C,W,S,T,dts,act,use_bias,slay,xlay", CONV, ids=[c[0] for c in CONV])
def test_conv1d_update_cases(dev, name, Bsz, C, W, S, T, dts, act, use_bias, slay, xlay):
    """state: rows 1 .. B of a pool of B + 2 rows, random; channel-last as Mamba2.allocate_inference_cache makes it, or channel-first.
    x: contiguous, or the columns 8 .. 8 + C of NaN-filled rows of C + 16 (the xBC columns of zxbcdt; T > 1: one such row per token)."""
    from omnimamba_amd.causal_conv1d import causal_conv1d_update
    xdt, sdt, wdt = dts
    g = torch.Generator().manual_seed(C + W + T)
    r = lambda *s: torch.randn(*s, generator=g)
    pool0 = (r(Bsz + 2, S, C).to(sdt).transpose(1, 2) if slay == "channel-last" else r(Bsz + 2, C, S).to(sdt))
    w0, b0 = r(C, W).to(wdt), (r(C).to(wdt) if use_bias else None)
    if xlay == "column-slice":
        xbase0 = torch.full((Bsz, T, C + 16), float("nan"))
        xbase0[:, :, 8:8 + C] = r(Bsz, T, C)
        xbase0 = xbase0.to(xdt)
        view = (lambda t: t[:, 0, 8:8 + C]) if T == 1 else (lambda t: t[:, :, 8:8 + C].transpose(1, 2))
    else:
        xbase0 = r(Bsz, C, T).to(xdt)
        view = (lambda t: t[:, :, 0]) if T == 1 else (lambda t: t)
    pool, xbase = on(pool0, dev), on(xbase0, dev)
    assert pool.stride() == pool0.stride()
    out = causal_conv1d_update(view(xbase), pool[1:Bsz + 1], on(w0, dev), on(b0, dev), activation=act)
    # fp64: the last W - 1 state columns and x, dot the weight, + bias, SiLU; the new state is the last S columns of (state ++ x)
    x64 = view(xbase0).double().reshape(Bsz, C, T)
    full = torch.cat([pool0[1:Bsz + 1].double(), x64], -1)
    o64 = torch.stack([(full[:, :, S + t + 1 - W:S + t + 1] * w0.double()[None]).sum(-1) for t in range(T)], -1)
    if b0 is not None:
        o64 = o64 + b0.double()[None, :, None]
    if act is not None:
        o64 = o64 * torch.sigmoid(o64)
    out, pool = out.cpu().reshape(Bsz, C, T), pool.cpu()
    assert out.dtype == xdt and torch.isfinite(out).all()
    blocks = [(b, slice(c0, min(c0 + 64, C))) for b in range(Bsz) for c0 in range(0, C, 64)]
    ro = worst_ratio(out, o64, xdt, blocks)
    print(f"\n[decode-step-ops] conv1d_update   {name}: worst (batch, 64 channels) / bound  out {ro:.3f}")
    assert ro <= 1.0, f"out: worst (batch, 64-channel block) at {ro:.3f} of op_bound"
    assert torch.equal(pool[1:Bsz + 1], full[:, :, -S:].to(sdt)), "the new state is not the shifted window"
    assert torch.equal(pool[0], pool0[0]) and torch.equal(pool[Bsz + 1], pool0[Bsz + 1]), "a pool row outside the batch was written"
    assert torch.equal(torch.nan_to_num(xbase.cpu().float(), nan=7.0), torch.nan_to_num(xbase0.float(), nan=7.0)), "x was written"
