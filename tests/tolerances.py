"""The forward-scan tolerance rule of round 3, shared by the parity tests.

North star: the MFMA scan matches the reference's scan within 1e-3 (relative L2) of ARITHMETIC error -- on top of the one
rounding of the bf16 output itself (Q_BF16: no bf16-output kernel can go below it), hence every bound has the form
sqrt(arith^2 + q^2) with q measured on the oracle's own output.

The reference's scan (mamba_ssm 2.2.2, absent from /root/reference) is itself not exact: with 16-bit activations it rounds
three tl.dot operands to the activation dtype (oracle.ssd_ref_chunked(..., emulate_upstream_rounding=True)).
Its own arithmetic error against the fp64 recurrence is 0.4e-3 .. 1.7e-3 depending on the head's decay (heads whose output
is mostly intra-chunk suffer the bf16 C.B^T operand, slow-decay heads the bf16 chunk states), so "within 1e-3 of the
reference" is not a fixed distance from the exact answer.  The rule the tests apply per (batch, head) slice:

    arith(ours vs fp64)  <=  max(ARITH_BUDGET, 1.05 * arith(upstream-rounding oracle at the reference's chunk size 256 vs fp64))

i.e. inside the north-star budget wherever the reference pipeline itself is, and never further from the exact result than
the reference pipeline where its own rounding points exceed the budget.

Two more rules live here and nowhere else (round 6):

  * PRECISE (OmkSsdFwd.flags & OMK_SSD_PRECISE, ssd_combined.scan_options(precise=True)): the BARE 1e-3 on every head -- no
    reference-relative term.  tests/test_configs_gpu.py asserts it on all ten slices of the production shape, slow heads included.
  * the TRAINING instantiation of the default kernel (no final state kept, window-state images saved: what Stage2Step and
    bench.py launch) enters the scaled operand of the state update as ONE bf16 value, like the reference pipeline's chunk-state
    kernel, where the keep-final instantiation uses hi + lo.  It therefore rounds at exactly the reference's two points (that
    operand, and the state that meets C) and ties with it on state-dominated heads: measured 0.94 .. 1.13 x the upstream-rounding
    oracle's own error on heads with A dt0 < 0.01, 0.2 .. 0.6 x elsewhere.  A tie cannot be asserted at 1.05 x of a quantity that
    is itself one draw of a rounding error, so its bound is TRAIN_FACTOR = 1.15 x; callers who need more take KHILO (+ 15 %) or
    PRECISE (+ 37 %) per call (profiles/r06_precise.txt).

The rule of the NON-SCAN streaming ops (norms, conv1d, LoRA add; op_bound below).  These kernels keep every intermediate in fp32
and round once, at the store.  For an output o of dtype T and an fp64 reference r computed from exactly the tensors the kernel
reads (a backward reference takes the forward's saved tensors -- residual_out, rstd, mean -- as its inputs, so that only the
backward's own arithmetic is measured):

    rel(o, r)  <=  1.1 * sqrt(q^2 + a^2),    q = rel(r.to(T), r) on the compared slice (0 for fp32 outputs)

with a = OP_ARITH = 1e-4, the allowance of fp32 arithmetic with fast exp / rcp / rsqrt and long fp32 sums.  dw / db of the norms
and the conv are fp32 sums: q = 0, so a dropped row (1 / sqrt(rows) of rel-L2) or a double-counted partial is far outside the
bound, where the flat 1.5e-2 of rounds 1 - 6 hid it.

omk_norm_linear (tests/test_norm_linear_slices.py) comes under the same rule, per (sequence, block of 16 output rows), with its two
documented internal rounding points reproduced by the reference and nothing else.  (1) With bf16 weights the kernels for two to eight
sequences (BATCHED and MATRIX) keep u = (x + residual | x silu(z)) * w in LDS as bf16, and the LoRA input is the same rounded u: the
reference forms u in fp32 in the kernel's order of operations, rounds it to bf16 and goes on in fp64 (the sum of squares takes the
unrounded q, as the kernel does).  Without a gate that u is bit-identical to the kernel's.  With a gate the kernel's silu_fast differs from
the exact sigmoid by a few fp32 ulps, so an element of u next to a bf16 rounding midpoint could round the other way; the bound is NOT
widened for that: the inputs are chosen on the reference alone -- every element of z whose exact u lies within relative
MIDPOINT_REL = 2^-19 (about 16 fp32 ulps: three roundings, a hardware exp2 and a reciprocal) of a midpoint is drawn again, and each
gated row asserts that none is left (near_bf16_midpoint).  (2) The conv tail rounds the projected value to the activation dtype before it
enters the tap sum and becomes the newest state column: that stored column is checked against the unrounded projection (one rounding of
the exact value), and the conv reference takes it as stored, like a backward reference takes the forward's saved tensors."""
import math

import torch

import oracle as O

Q_BF16 = 1.65e-3
ARITH_BUDGET = 1e-3
TRAIN_FACTOR = 1.15
OP_ARITH = 1e-4


def training_budget(upstream_arith):
    """y arithmetic bound of the training instantiation (module docstring)."""
    return max(ARITH_BUDGET, TRAIN_FACTOR * upstream_arith)


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def arith_part(e, q):
    return math.sqrt(max(e * e - q * q, 0.0))


def forward_budget(x, dt, A, Bm, Cm, return_upstream=False, **kw):
    """Returns (y_exact fp64 unrounded, final_exact, budget_y, budget_final, (upstream arithmetic error of y, of the final state))
    for one slice of inputs; kw: D, z, dt_bias, initial_states, dt_softplus, dt_limit.  return_upstream: a sixth element, the
    (unrounded) output and final state of the upstream-rounding oracle, for the DIRECT distance (direct_bound below)."""
    kw = dict(kw, return_final_states=True, round_output=False)
    y64, f64 = O.ssd_ref_chunked(x, dt, A, Bm, Cm, 64, compute_dtype=torch.float64, **kw)
    yu, fu = O.ssd_ref_chunked(x, dt, A, Bm, Cm, 256, emulate_upstream_rounding=True, **kw)
    eu, ef = rel(yu, y64), rel(fu, f64)
    r = (y64, f64, max(ARITH_BUDGET, 1.05 * eu), max(ARITH_BUDGET, 1.05 * ef), (eu, ef))
    return r + ((yu, fu),) if return_upstream else r


def direct_bound(own_arith_budget, upstream_arith, q=0.0):
    """Round 4: the distance of this kernel's output to the upstream-rounding oracle ITSELF (not each one's
    distance to the exact result).  Two independent arithmetic errors a (ours, <= own_arith_budget) and u (the reference
    pipeline's own, measured) are at most a + u apart and sqrt(a^2 + u^2) apart when uncorrelated; the tests assert the
    uncorrelated form with 10 % slack, on top of the quantisation q of a bf16 output compared with an unrounded one.  Where the
    reference pipeline's own error is small (u << 1e-3) this IS the north-star 1e-3; where u ~ 1.7e-3 no kernel that does not
    reproduce upstream's rounding errors bit for bit can be closer to it than u."""
    return math.sqrt(q * q + 1.21 * (own_arith_budget ** 2 + upstream_arith ** 2))


def op_bound(ref, dtype, arith=OP_ARITH):
    """Bound of a non-scan op's output of dtype `dtype` against its fp64 reference `ref` (module docstring): one rounding of the
    exact answer to `dtype`, measured on this slice, plus the fp32 arithmetic allowance, with 10 % slack."""
    q = 0.0 if dtype in (torch.float32, torch.float64) else rel(ref.to(dtype), ref)
    return 1.1 * math.sqrt(q * q + arith * arith)


SLICE_FLOOR = 0.1


def slice_check(name, got, ref, dtype, keep, arith=OP_ARITH, bound=None, groups=None, sizes=None):
    """op_bound on every slice of one output (the selective scan; module docstring for the rule).  The first `keep` dimensions index
    the slices, the others are reduced: out / du / ddelta / dz (B, D, L) keep 2 = a (batch, channel) row over L; input-dependent
    dB / dC (B, G, N, L) keep 3; dA and constant dB / dC (D, N) keep 1; states (B, D, N) keep 2; dD / ddelta_bias (D) keep 1 = each
    element.  `ref` is the unrounded fp64 answer, `dtype` the dtype the kernel stored (fp32 sums: q = 0).

    The relative error of slice s is |got_s - ref_s| / max(|ref_s|, SLICE_FLOOR * RMS over the tensor's slices of |ref_s|): a
    slice that is small by cancellation (or belongs to a channel whose regime makes it small) is judged on an absolute scale and
    none is left out.  q_s, the one rounding of ref_s to `dtype`, is measured with the same denominator; for a slice of ONE element of
    a 16-bit dtype it is half an ulp instead (the measured rounding of a single number can be anything down to 0, and a sum that is off
    by 1e-6 may round the other way).  `groups` (a tensor of ids over the last slice dimension, i.e. per channel): the RMS of the floor
    is taken inside each group where that is SMALLER than the tensor's -- channels of different decay regimes in one launch, whose
    slices differ by orders of magnitude, are each judged on their own scale and never on a larger one than without groups.
    `sizes` (a tensor over the slices): the number of real elements of each slice where ragged slices were padded with zeros on both
    sides (column_blocks below) -- a slice of one real element takes the half-ulp q like a slice of one element.
    `bound`: a flat number per slice in place of op_bound (two launches that must agree).  Fails naming the tensor, the slice, its error, q and bound; returns
    (worst error, q of that slice, its bound, share of slices that met the floor)."""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape, (name, tuple(got.shape), tuple(ref.shape))
    assert torch.isfinite(got).all(), f"{name}: not finite"
    lead = tuple(ref.shape[:keep])
    g2, r2 = got.reshape(*lead, -1), ref.reshape(*lead, -1)
    norms = r2.norm(dim=-1)
    floor = SLICE_FLOOR * norms.pow(2).mean().sqrt()
    if groups is not None:
        gl, floor = groups.expand(lead), floor.expand(lead).clone()
        for gid in groups.unique():
            m = gl == gid
            floor[m] = torch.minimum(floor[m], SLICE_FLOOR * norms[m].pow(2).mean().sqrt())
    den = torch.maximum(norms, floor).clamp_min(1e-300)
    err = (g2 - r2).norm(dim=-1) / den
    if dtype in (torch.float32, torch.float64):
        q = torch.zeros_like(err)
    else:
        half, meas = 0.5 * torch.finfo(dtype).eps * norms / den, (r2.to(dtype).double() - r2).norm(dim=-1) / den
        q = half if r2.shape[-1] == 1 else (meas if sizes is None else torch.where(sizes.expand(lead) == 1, half, meas))
    lim = torch.full_like(err, bound) if bound is not None else 1.1 * (q * q + arith * arith).sqrt()
    share = (norms < floor).double().mean().item()
    i = int((err / lim).argmax())
    idx = tuple(int(v) for v in torch.unravel_index(torch.tensor(i), lead)) if lead else ()
    e, qq, b = err.flatten()[i].item(), q.flatten()[i].item(), lim.flatten()[i].item()
    assert e <= b, f"{name}: slice {idx} error {e:.3e} q {qq:.3e} bound {b:.3e} ({int((err > lim).sum())} of {err.numel()} slices over)"
    return e, qq, b, share


def column_blocks(got, ref, lo, hi, align=0, width=16):
    """Columns [lo, hi) of two (rows, columns) tensors cut into blocks of `width` columns whose edges lie at align + k * width, for
    slice_check: returns (got, ref) as (rows, blocks, width) in fp64, ragged first / last blocks padded with zeros in both (a zero adds
    nothing to a slice's norm, error or rounding), and the number of real columns of every block (slice_check's `sizes`)."""
    first = lo - (lo - align) % width
    edges = [(max(a, lo), min(a + width, hi)) for a in range(first, hi, width)]
    g3, r3 = (torch.zeros(ref.shape[0], len(edges), width, dtype=torch.float64) for _ in range(2))
    for j, (a, b) in enumerate(edges):
        g3[:, j, :b - a], r3[:, j, :b - a] = got[:, a:b].double().cpu(), ref[:, a:b].double().cpu()
    return g3, r3, torch.tensor([b - a for a, b in edges])


MIDPOINT_REL = 2.0 ** -19


def near_bf16_midpoint(u, rel_dist=MIDPOINT_REL):
    """Mask of the elements of the fp64 tensor u that lie within rel_dist * |u| of the midpoint of two neighbouring bf16 values (module
    docstring, norm_linear): |u| = t * 2^e with t in [128, 256) has the bf16 grid at the integers of t."""
    mant, _ = torch.frexp(u.abs().double())
    t = mant * 256.0
    return ((t - t.floor() - 0.5).abs() <= t * rel_dist) & (u != 0)
