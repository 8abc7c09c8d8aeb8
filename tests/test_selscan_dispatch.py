"""Which kernels a Mamba-1 selective scan call launches: a table of calls through the C ABI (K.SelScanFwd / K.SelScanBwd, so that no
copy of the Python wrapper hides the layout) and, for each, what omk_selective_scan_{fwd,bwd}_form answers, the status of the call
and the exact omk_ssd_last_kernels() string -- on the emulator (the host code that chooses and launches is the same in both builds).

Every row was recorded from the commit BEFORE ss_fwd_plan / ss_bwd_plan existed, not from the code under test.  That commit recorded
no selscan kernel, so its host section (selscan.hip behind `using namespace omk;`) got these ten lines, in a scratch copy that was
never committed, and the case table below ran against its emulator build:

  * `kernels_reset();` as the first statement of omk_selective_scan_fwd and of omk_selective_scan_bwd;
  * in ss_launch_fwd, in front of the two selscan_fwd_lanes_kernel launches (`form` = what ss_lanes_form returned, 2 channel-last / 3 L-contiguous):
    `kernels_note("selscan_fwd_lanes<lc=%d>", form == 2 ? 0 : 1);`
  * in front of the three selscan_fwd_shared_kernel launches (<T, 8, 1, true> for pass_ckpt, <T, 16, 1> for lc16, else <T, 8, 2>):
    `kernels_note("selscan_fwd_shared<lc=%d,nu=%d,state_only=%d>", lc, pass_ckpt || lc16 ? 1 : 2, (int)pass_ckpt);`
  * in front of the two selscan_fwd_chunked_kernel launches: `kernels_note("selscan_fwd_chunked<lc=%d>", lc);`
  * in front of the selscan_fwd_kernel launch: `kernels_note("selscan_fwd<nreg=%d>", a.N <= 16 ? 16 : 64);`
  * in omk_selective_scan_bwd, in front of the lanes backward's own selscan_fwd_lanes_kernel<T, false> launch:
    `kernels_note("selscan_fwd_lanes<lc=0>");` and in front of selscan_bwd_lanes_kernel: `kernels_note("selscan_bwd_lanes");`
  * in front of selscan_bwd_chunked_kernel: `kernels_note("selscan_bwd_chunked<nw=%d,nb=%d,noct=%d>", NW, q.NB, q.nOct);`
  * in front of selscan_bwd_kernel: `kernels_note("selscan_bwd");`

A row is (answer of the _form query, status of the call, kernel string); the query is asked on the very descriptor the call gets.
Where the first entry is a pair, it is (that commit's answer, the answer now): omk_selective_scan_bwd_form used to say 1 ("chunked")
from a looser condition than the one the call launched by, and now says what the call launches.  These are the classes of input where
L-contiguous rows with input-dependent B / C and L >= 64 do NOT run the chunked scan, one row each: channels per group not a multiple
of 8 (bwd-bdl-dpg6); B / C of another dtype than u (bwd-b_dtype); A not fp32 (bwd-a_dtype); du / ddelta / dz without unit stride
along L (bwd-grads_cl); and the two refusals of the same class (bwd-refused-N24: d_state > 16, bwd-refused-pass_states).  No 2 changed.

Some things the table shows that one might not expect: with L < 64 the lanes = channels form takes every call that meets its layout and
dtype conditions, whatever the number of waves (fwd-bdl-var_b, bwd-cl-L33); omk_selective_scan_fwd_form does not look at the form of
pass_states, so it answers 2 for tile states on (B, D, L) storage and the call refuses them (fwd-tile_states-refused-bdl); B + C rows
of exactly 64 KiB are still shared (fwd-shared-lds_bound-N32-bf16).  An empty tensor has no data pointer in torch, and the ABI takes
such a tensor for absent: the two empty cases hand in a dummy pointer to reach the early return.

The backward cases run the real kernels on the emulator and take one to three seconds each there; the forward cases well under one.
"""
import ctypes

import pytest
import torch

BF16, F32 = torch.bfloat16, torch.float32
LANES = {"OMK_SELSCAN_LANES": "1"}    # the test hook: no minimum number of waves for the lanes = channels form


def _inputs(D, L, N, G=1, dtype=BF16, cl=False, const_b=False, b_dtype=None, a_dtype=F32, batch=2):
    """u / delta / z (B, D, L) and B / C (B, G, N, L): L-contiguous, or with cl views of token-major (B, L, D) / (B, L, G, N) storage.
    batch 0: empty slices of a batch of one."""
    g = torch.Generator().manual_seed(0)
    empty, batch = batch == 0, max(batch, 1)

    def rows(scale=1.0):
        t = (torch.rand(batch, L, D, generator=g) * scale).to(dtype).transpose(1, 2)
        return t if cl else t.contiguous()

    def bc():
        t = torch.randn(batch, L, G, N, generator=g).to(b_dtype or dtype).permute(0, 2, 3, 1)
        return t if cl else t.contiguous()

    u, delta, z = rows(), rows(0.5), rows()
    A = -(torch.rand(D, N, generator=g) + 0.1).to(a_dtype)
    Bm, Cm = bc(), bc()
    if empty:
        u, delta, z, Bm, Cm = (t[:0] for t in (u, delta, z, Bm, Cm))
    return u, delta, z, A, torch.randn(D, N, generator=g) if const_b else Bm, Cm


_SOMEWHERE = torch.zeros(4)


def _desc(K, t):
    """K.T(t); an empty tensor gets a data pointer (torch gives it none, and the ABI takes a tensor without one for absent)."""
    d = K.T(t)
    if t is not None and t.numel() == 0:
        d.data = _SOMEWHERE.data_ptr()
    return d


def _states(kind, u, N):
    """pass_states: the 512-token form (B, D, ceil(L / 512), N), the tile form (B, ceil(L / 16), N, D), or none."""
    Bsz, D, L = u.shape
    if kind == "pass":
        return torch.zeros(Bsz, D, (L + 511) // 512, N)
    if kind == "tile":
        return torch.zeros(Bsz, (L + 15) // 16, N, D)
    assert kind is None
    return None


def _fwd(lib, K, states=None, out_cl=None, **shape):
    u, delta, z, A, Bm, Cm = _inputs(**shape)
    T = lambda t: _desc(K, t)
    cl = shape.get("cl", False) if out_cl is None else out_cl
    out = torch.empty(u.shape[0], u.shape[2], u.shape[1], dtype=u.dtype).transpose(1, 2) if cl else torch.empty(u.shape, dtype=u.dtype)
    ps = _states(states, u, A.shape[1])
    p = K.SelScanFwd(u=T(u), delta=T(delta), A=T(A), Bm=T(Bm), Cm=T(Cm), D=T(None), z=T(z), delta_bias=T(None),
                     out=T(out), last_state=T(None), pass_states=T(ps), delta_softplus=1)
    return lib.omk_selective_scan_fwd_form(ctypes.byref(p)), lib.omk_selective_scan_fwd(ctypes.byref(p), None)


def _bwd(lib, K, states=None, grads_cl=False, **shape):
    u, delta, z, A, Bm, Cm = _inputs(**shape)
    T = lambda t: _desc(K, t)
    # du / ddelta / dz laid out like u (empty_like keeps the strides of a dense view), or channel-last whatever u is
    like = lambda t: torch.empty_like(t.transpose(1, 2).contiguous().transpose(1, 2) if grads_cl else t)
    dout, du, ddelta, dz = torch.ones_like(u), like(u), like(delta), like(z)
    dA, dB, dC = torch.zeros(A.shape), torch.zeros(Bm.shape), torch.zeros(Cm.shape)
    ps = _states(states, u, A.shape[1])
    p = K.SelScanBwd(u=T(u), delta=T(delta), A=T(A), Bm=T(Bm), Cm=T(Cm), D=T(None), z=T(z), delta_bias=T(None),
                     dout=T(dout), du=T(du), ddelta=T(ddelta), dA=T(dA), dB=T(dB), dC=T(dC), dD=T(None), dz=T(dz),
                     ddelta_bias=T(None), pass_states=T(ps), delta_softplus=1)
    ws = K.workspace(lib, "omk_selective_scan_bwd_workspace_bytes", p, u)  # noqa: F841
    if ws is None:
        p.workspace = _SOMEWHERE.data_ptr()    # (nothing to keep for an empty call, but the pointer is required)
    return lib.omk_selective_scan_bwd_form(ctypes.byref(p)), lib.omk_selective_scan_bwd(ctypes.byref(p), None)


# id -> (function, keyword arguments, environment)
CASES = {
    # ---- forward: the per-channel kernel
    "fwd-bdl-const_b": (_fwd, dict(D=6, L=20, N=4, const_b=True), {}),
    "fwd-bdl-const_b-f32": (_fwd, dict(D=6, L=20, N=4, const_b=True, dtype=F32), {}),
    "fwd-bdl-var_b": (_fwd, dict(D=6, L=20, N=4), {}),
    "fwd-bdl-var_b-f32": (_fwd, dict(D=6, L=20, N=4, dtype=F32), {}),
    "fwd-nreg64": (_fwd, dict(D=130, L=37, N=24), {}),
    "fwd-cl-L200": (_fwd, dict(D=12, L=200, N=16, cl=True), {}),
    "fwd-cl-D1": (_fwd, dict(D=1, L=200, N=16, cl=True), {}),
    "fwd-cl-L100": (_fwd, dict(D=70, L=100, N=16, cl=True), {}),
    # ---- forward: the chunked scan, own B / C rows per channel or shared by 8 channels of a group
    "fwd-chunked-dpg10": (_fwd, dict(D=10, L=200, N=16), {}),
    "fwd-chunked-lc16": (_fwd, dict(D=6, G=2, L=1100, N=16), {}),
    "fwd-chunked-const_b": (_fwd, dict(D=24, L=130, N=16, const_b=True), {}),
    "fwd-chunked-b_dtype": (_fwd, dict(D=16, L=130, N=16, b_dtype=F32), {}),
    "fwd-chunked-a_dtype": (_fwd, dict(D=16, L=130, N=16, a_dtype=BF16), {}),
    "fwd-shared-nu2": (_fwd, dict(D=16, G=2, L=600, N=16), {}),
    "fwd-shared-lc16": (_fwd, dict(D=8, L=1100, N=16), {}),
    "fwd-shared-lds_bound-f32": (_fwd, dict(D=8, L=64, N=64, dtype=F32), {}),
    "fwd-shared-lds_bound-bf16": (_fwd, dict(D=8, L=64, N=64), {}),
    "fwd-shared-lds_bound-N32-f32": (_fwd, dict(D=8, L=64, N=32, dtype=F32), {}),
    "fwd-shared-lds_bound-N32-bf16": (_fwd, dict(D=8, L=64, N=32), {}),    # B + C rows of exactly 64 KiB
    # ---- forward: lanes = channels
    "fwd-lanes-cl-L45": (_fwd, dict(D=70, L=45, N=16, cl=True), {}),
    "fwd-lanes-cl-hook": (_fwd, dict(D=96, G=2, L=200, N=16, cl=True), LANES),
    "fwd-lanes-bdl-hook": (_fwd, dict(D=96, G=2, L=200, N=16), LANES),
    "fwd-lanes-no-N24-hook": (_fwd, dict(D=96, G=2, L=200, N=24, cl=True), LANES),
    "fwd-lanes-no-b_dtype-hook": (_fwd, dict(D=96, G=2, L=200, N=16, cl=True, b_dtype=F32), LANES),
    # ---- forward: pass_states
    "fwd-pass_states-chunked": (_fwd, dict(D=16, L=600, N=16, states="pass"), {}),
    "fwd-pass_states-L1100": (_fwd, dict(D=8, L=1100, N=16, states="pass"), {}),    # (512-token passes: no lc=16)
    "fwd-pass_states-lanes-hook": (_fwd, dict(D=96, G=2, L=200, N=16, cl=True, states="pass"), LANES),
    "fwd-pass_states-refused-cl": (_fwd, dict(D=96, G=2, L=200, N=16, cl=True, states="pass"), {}),
    "fwd-tile_states-lanes-cl": (_fwd, dict(D=70, L=45, N=16, cl=True, states="tile"), {}),
    "fwd-tile_states-refused-bdl": (_fwd, dict(D=70, L=45, N=16, states="tile"), {}),
    "fwd-empty": (_fwd, dict(D=6, L=20, N=4, batch=0), {}),
    # ---- backward: lanes = channels
    "bwd-lanes-hook": (_bwd, dict(D=70, L=45, N=16, cl=True), LANES),
    "bwd-lanes-tile_states-hook": (_bwd, dict(D=70, L=45, N=16, cl=True, states="tile"), LANES),
    "bwd-cl-D1": (_bwd, dict(D=1, L=45, N=16, cl=True), LANES),
    # ---- backward: the chunked scan
    "bwd-chunked": (_bwd, dict(D=16, L=600, N=16), {}),
    "bwd-chunked-pass_states": (_bwd, dict(D=16, L=600, N=16, states="pass"), {}),
    "bwd-chunked-nw8": (_bwd, dict(D=8, L=64, N=16, states="pass"), {}),
    "bwd-chunked-oct1": (_bwd, dict(D=32, L=64, N=16, states="pass"), {"OMK_SELSCAN_BWD_OCT": "1"}),
    "bwd-chunked-oct2": (_bwd, dict(D=32, L=64, N=16, states="pass"), {"OMK_SELSCAN_BWD_OCT": "2"}),
    "bwd-chunked-oct4": (_bwd, dict(D=32, L=64, N=16, states="pass"), {"OMK_SELSCAN_BWD_OCT": "4"}),
    "bwd-chunked-oct4-D64": (_bwd, dict(D=64, L=64, N=16, states="pass", batch=1), {"OMK_SELSCAN_BWD_OCT": "4"}),
    "bwd-chunked-N24": (_bwd, dict(D=16, L=64, N=24, states="pass"), {}),
    "bwd-chunked-N64-f32": (_bwd, dict(D=8, L=64, N=64, dtype=F32), {}),
    "bwd-chunked-tile_states": (_bwd, dict(D=16, L=64, N=16, states="tile"), {}),
    # ---- backward: the per-channel kernel, and what it refuses
    "bwd-bdl-dpg6": (_bwd, dict(D=6, L=200, N=16), {}),
    "bwd-cl-L33": (_bwd, dict(D=12, L=33, N=8, G=2, cl=True), {}),
    "bwd-cl-L33-const_b": (_bwd, dict(D=12, L=33, N=8, cl=True, const_b=True), {}),
    "bwd-cl-L64": (_bwd, dict(D=12, L=64, N=8, G=2, cl=True, batch=1), {}),
    "bwd-b_dtype": (_bwd, dict(D=8, L=64, N=16, b_dtype=F32, batch=1), {}),
    "bwd-a_dtype": (_bwd, dict(D=8, L=64, N=16, a_dtype=BF16, batch=1), {}),
    "bwd-grads_cl": (_bwd, dict(D=8, L=64, N=16, grads_cl=True, batch=1), {}),
    "bwd-refused-N24": (_bwd, dict(D=6, L=200, N=24), {}),
    "bwd-refused-N24-cl": (_bwd, dict(D=16, L=100, N=24, cl=True), {}),
    "bwd-empty": (_bwd, dict(D=6, L=20, N=4, batch=0), {}),
    "bwd-refused-pass_states": (_bwd, dict(D=6, L=200, N=16, states="pass"), {}),
}


def launched(case, setenv):
    """Run one case on the emulator: (what the _form query answers, the status of the call, omk_ssd_last_kernels())."""
    from emu.loader import use_emulator
    fn, kw, env = CASES[case]
    for k, v in env.items():
        setenv(k, v)
    with use_emulator() as lib:
        from omnimamba_amd import _capi as K
        form, rc = fn(lib, K, **kw)
        return form, rc, lib.omk_ssd_last_kernels().decode()


EXPECTED = {
    "bwd-a_dtype": ((1, 0), 0, 'selscan_fwd<nreg=16>;selscan_bwd'),
    "bwd-b_dtype": ((1, 0), 0, 'selscan_fwd<nreg=16>;selscan_bwd'),
    "bwd-bdl-dpg6": ((1, 0), 0, 'selscan_fwd<nreg=16>;selscan_bwd'),
    "bwd-chunked": (1, 0, 'selscan_fwd_shared<lc=8,nu=1,state_only=1>;selscan_bwd_chunked<nw=16,nb=16,noct=1>'),
    "bwd-chunked-N24": (1, 0, 'selscan_bwd_chunked<nw=16,nb=16,noct=1>'),
    "bwd-chunked-N64-f32": (1, 0, 'selscan_fwd_chunked<lc=8>;selscan_bwd_chunked<nw=8,nb=16,noct=1>'),
    "bwd-chunked-nw8": (1, 0, 'selscan_bwd_chunked<nw=8,nb=16,noct=1>'),
    "bwd-chunked-oct1": (1, 0, 'selscan_bwd_chunked<nw=16,nb=16,noct=1>'),
    "bwd-chunked-oct2": (1, 0, 'selscan_bwd_chunked<nw=16,nb=16,noct=2>'),
    "bwd-chunked-oct4": (1, 0, 'selscan_bwd_chunked<nw=16,nb=16,noct=1>'),
    "bwd-chunked-oct4-D64": (1, 0, 'selscan_bwd_chunked<nw=16,nb=16,noct=4>'),
    "bwd-chunked-pass_states": (1, 0, 'selscan_bwd_chunked<nw=16,nb=16,noct=1>'),
    "bwd-chunked-tile_states": (1, -1, ''),
    "bwd-cl-D1": (0, 0, 'selscan_fwd<nreg=16>;selscan_bwd'),
    "bwd-cl-L33": (2, 0, 'selscan_fwd_lanes<lc=0>;selscan_bwd_lanes'),
    "bwd-cl-L33-const_b": (0, 0, 'selscan_fwd<nreg=16>;selscan_bwd'),
    "bwd-cl-L64": (0, 0, 'selscan_fwd<nreg=16>;selscan_bwd'),
    "bwd-empty": (0, 0, ''),
    "bwd-grads_cl": ((1, 0), 0, 'selscan_fwd<nreg=16>;selscan_bwd'),
    "bwd-lanes-hook": (2, 0, 'selscan_fwd_lanes<lc=0>;selscan_bwd_lanes'),
    "bwd-lanes-tile_states-hook": (2, 0, 'selscan_bwd_lanes'),
    "bwd-refused-N24": ((1, 0), -4, ''),
    "bwd-refused-N24-cl": (0, -4, ''),
    "bwd-refused-pass_states": ((1, 0), -1, ''),
    "fwd-bdl-const_b": (0, 0, 'selscan_fwd<nreg=16>'),
    "fwd-bdl-const_b-f32": (0, 0, 'selscan_fwd<nreg=16>'),
    "fwd-bdl-var_b": (2, 0, 'selscan_fwd_lanes<lc=1>'),
    "fwd-bdl-var_b-f32": (2, 0, 'selscan_fwd_lanes<lc=1>'),
    "fwd-chunked-a_dtype": (1, 0, 'selscan_fwd_chunked<lc=8>'),
    "fwd-chunked-b_dtype": (1, 0, 'selscan_fwd_chunked<lc=8>'),
    "fwd-chunked-const_b": (1, 0, 'selscan_fwd_chunked<lc=8>'),
    "fwd-chunked-dpg10": (1, 0, 'selscan_fwd_chunked<lc=8>'),
    "fwd-chunked-lc16": (1, 0, 'selscan_fwd_chunked<lc=16>'),
    "fwd-cl-D1": (0, 0, 'selscan_fwd<nreg=16>'),
    "fwd-cl-L100": (0, 0, 'selscan_fwd<nreg=16>'),
    "fwd-cl-L200": (0, 0, 'selscan_fwd<nreg=16>'),
    "fwd-empty": (2, 0, ''),
    "fwd-lanes-bdl-hook": (2, 0, 'selscan_fwd_lanes<lc=1>'),
    "fwd-lanes-cl-L45": (2, 0, 'selscan_fwd_lanes<lc=0>'),
    "fwd-lanes-cl-hook": (2, 0, 'selscan_fwd_lanes<lc=0>'),
    "fwd-lanes-no-N24-hook": (0, 0, 'selscan_fwd<nreg=64>'),
    "fwd-lanes-no-b_dtype-hook": (0, 0, 'selscan_fwd<nreg=16>'),
    "fwd-nreg64": (0, 0, 'selscan_fwd<nreg=64>'),
    "fwd-pass_states-L1100": (1, 0, 'selscan_fwd_shared<lc=8,nu=2,state_only=0>'),
    "fwd-pass_states-chunked": (1, 0, 'selscan_fwd_shared<lc=8,nu=2,state_only=0>'),
    "fwd-pass_states-lanes-hook": (2, 0, 'selscan_fwd_lanes<lc=0>'),
    "fwd-pass_states-refused-cl": (0, -4, ''),
    "fwd-shared-lc16": (1, 0, 'selscan_fwd_shared<lc=16,nu=1,state_only=0>'),
    "fwd-shared-lds_bound-N32-bf16": (1, 0, 'selscan_fwd_shared<lc=8,nu=2,state_only=0>'),
    "fwd-shared-lds_bound-N32-f32": (1, 0, 'selscan_fwd_chunked<lc=8>'),
    "fwd-shared-lds_bound-bf16": (1, 0, 'selscan_fwd_chunked<lc=8>'),
    "fwd-shared-lds_bound-f32": (1, 0, 'selscan_fwd_chunked<lc=8>'),
    "fwd-shared-nu2": (1, 0, 'selscan_fwd_shared<lc=8,nu=2,state_only=0>'),
    "fwd-tile_states-lanes-cl": (2, 0, 'selscan_fwd_lanes<lc=0>'),
    "fwd-tile_states-refused-bdl": (2, -4, ''),
}


def test_every_case_has_an_expected_row():
    assert sorted(CASES) == sorted(EXPECTED)


@pytest.mark.parametrize("case", sorted(CASES))
def test_selscan_dispatch(case, monkeypatch):
    form, rc, kernels = EXPECTED[case]
    if isinstance(form, tuple):    # (what the query answered before it asked the plan, what it answers now): the form of the launch
        form = form[1]
        assert form == (2 if "bwd_lanes" in kernels else 1 if "bwd_chunked" in kernels else 0)
    assert launched(case, monkeypatch.setenv) == (form, rc, kernels)
