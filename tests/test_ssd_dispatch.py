"""Which kernels an SSD scan call launches: a table of calls and the exact omk_ssd_last_kernels() string of each, on the emulator
(the host code that chooses and launches the kernels is the same in both builds).

The expected strings were recorded from the commit BEFORE the class A selector (ssd_class_a_plan) and the launch helper
(ssd_launch) existed, not from the code under test.  Where that commit's string named every launch, the string here is the
recorded one unchanged.  It left some launches out; for those cases the string here is the recorded one with exactly the missing
launches inserted in launch order:

  * fwd-window-odd, fwd-window-hg: the row-strip scan that writes window states -- `ssd_mfma_a3<...,dump=1>` appended
    (recorded: "ssd_dt_prep");
  * final_state_raw-odd, final_state_raw-hg: the row-strip state-only pass -- `ssd_mfma_a3<state_only>` appended
    (recorded: "ssd_dt_prep"); split-final_state_raw-odd, split-final_state_raw-hg: the same behind the segment state pass and fold;
  * bwd-sequential-pair, bwd-sequential-window-pair, split-bwd-sequential-pair: both class B scans `ssd_mfma_b3<mode,dmode>`, each
    followed by `ssd_reduce_partials`, inserted between the segment preparation (if any) and the dx scan
    (recorded for bwd-sequential-pair: "ssd_dt_prep;ssd_a8<mode=2,dump=0,khilo=0,precise=0>;ssd_bwd_finish_par").

(The row-strip state-dump pass `ssd_mfma_a3<state_dump>` is recorded now as well; no call through the C ABI reaches it -- the
chunk-parallel backward that asks for it needs head pairs, which the column-slice kernel takes.)
"""
import pytest
import torch

LAYOUTS = {"pair": (2, 1), "odd": (3, 1), "hg": (2, 2)}    # (nheads, ngroups): paired heads, odd head count, one head per group


def _inputs(H, G, L=70, P=64, N=128, dtype=torch.bfloat16):
    g = torch.Generator().manual_seed(0)
    x = torch.randn(1, L, H, P, generator=g).to(dtype)
    dt = torch.randn(1, L, H, generator=g).to(dtype)
    A = -torch.rand(H, generator=g) - 0.5
    Bm, Cm = torch.randn(1, L, G, N, generator=g).to(dtype), torch.randn(1, L, G, N, generator=g).to(dtype)
    return x, dt, A, Bm, Cm


def _fwd(S, K, H, G, variant, L=70, **shape):
    x, dt, A, Bm, Cm = _inputs(H, G, L, **shape)
    kw = {
        "plain": {},
        "gate_outx": dict(z=torch.randn_like(x), want_out_x=True),
        "final": dict(return_final_states=True),
        "D_hp": dict(D=torch.randn(H, x.shape[-1])),
        "window": dict(save_window_states=True),
        "precise": dict(flags=K.SSD_PRECISE),
        "khilo": dict(flags=K.SSD_KHILO),
        "column_slice": dict(flags=K.SSD_COLUMN_SLICE),
        "every_chunk": dict(flags=K.SSD_EVERY_CHUNK),
        "force_generic": dict(force_generic=True),
    }[variant]
    S.ssd_scan_fwd(x, dt, A, Bm, Cm, dt_softplus=True, **kw)


def _final_state_raw(S, K, H, G, L=70):
    x, dt, A, Bm, _ = _inputs(H, G, L)
    S.ssd_final_state_raw(x, dt, A, Bm, dt_softplus=True)


def _bwd(S, K, H, G, sequential=False, window=False, L=70):
    x, dt, A, Bm, Cm = _inputs(H, G, L)
    ws = S.ssd_scan_fwd(x, dt, A, Bm, Cm, D=torch.ones(H), dt_softplus=True, save_window_states=True)[3] if window else None
    assert not window or ws is not None
    S.ssd_scan_bwd(torch.randn_like(x), x, dt, A, Bm, Cm, D=torch.ones(H), dt_bias=torch.zeros(H), dt_softplus=True, window_states=ws,
                   flags=K.SSD_SEQUENTIAL_BWD if sequential else 0)


def _fused_conv(S, K, H, G, taken):
    P, N, W, L = 64, 128, 4, 70
    Ct = H * P + 2 * G * N
    g = torch.Generator().manual_seed(0)
    xBC = (torch.randn(1, L, Ct, generator=g) * 0.8).bfloat16()
    dt = torch.randn(1, L, H, generator=g).bfloat16()
    r = S.ssd_scan_fwd_fused_conv(xBC, dt, -torch.rand(H, generator=g) - 0.5, torch.randn(Ct, W, generator=g) * 0.4, torch.randn(Ct, generator=g) * 0.2,
                                  H, P, G, N, D=torch.ones(H))
    assert (r is not None) == taken


def _cases():
    c = {}    # id -> (function, positional and keyword arguments behind (S, K), environment)
    for lay, (H, G) in LAYOUTS.items():
        for v in ("plain", "gate_outx", "final", "D_hp", "window", "precise", "khilo", "column_slice", "every_chunk", "force_generic"):
            c[f"fwd-{v}-{lay}"] = (_fwd, (H, G, v), {}, {})
        c[f"final_state_raw-{lay}"] = (_final_state_raw, (H, G), {}, {})
        c[f"bwd-default-{lay}"] = (_bwd, (H, G), {}, {})
        c[f"bwd-sequential-{lay}"] = (_bwd, (H, G), dict(sequential=True), {})
        c[f"bwd-window-{lay}"] = (_bwd, (H, G), dict(window=True), {})
        # a split sequence (the test hook lets 64-token segments exist): three segments of 150 tokens
        split = {"OMK_SSD_SEG_CHUNKS": "1"}
        c[f"split-fwd-{lay}"] = (_fwd, (H, G, "plain"), dict(L=150), split)
        c[f"split-fwd-final-{lay}"] = (_fwd, (H, G, "final"), dict(L=150), split)
        c[f"split-final_state_raw-{lay}"] = (_final_state_raw, (H, G), dict(L=150), split)
        c[f"split-bwd-default-{lay}"] = (_bwd, (H, G), dict(L=150), split)
    c["bwd-sequential-window-pair"] = (_bwd, (2, 1), dict(sequential=True, window=True), {})
    c["split-fwd-gate_outx-pair"] = (_fwd, (2, 1, "gate_outx"), dict(L=150), split)
    c["split-fwd-window-pair"] = (_fwd, (2, 1, "window"), dict(L=150), split)
    c["split-bwd-sequential-pair"] = (_bwd, (2, 1), dict(sequential=True, L=150), split)
    c["split-bwd-window-pair"] = (_bwd, (2, 1), dict(window=True, L=150), split)
    k2 = {"OMK_K2_MIN_WGS": "1"}
    c["fused_conv-taken"] = (_fused_conv, (2, 1, True), {}, k2)
    c["fused_conv-refused-odd"] = (_fused_conv, (3, 1, False), {}, k2)
    c["fused_conv-refused-split"] = (_fused_conv, (2, 1, False), {}, dict(k2, **split))
    for v in ("plain", "gate_outx", "final"):
        c[f"fp32-{v}"] = (_fwd, (2, 1, v), dict(dtype=torch.float32), {})
        c[f"non_mfma-{v}"] = (_fwd, (2, 1, v), dict(P=32, N=16), {})
    c["fp32-bwd"] = (_bwd_plain, (), dict(dtype=torch.float32), {})
    c["non_mfma-bwd"] = (_bwd_plain, (), dict(P=32, N=16), {})
    return c


def _bwd_plain(S, K, **shape):
    x, dt, A, Bm, Cm = _inputs(2, 1, **shape)
    S.ssd_scan_bwd(torch.randn_like(x), x, dt, A, Bm, Cm, dt_softplus=True)


CASES = _cases()


def launched(case, setenv):
    """Run one case on the emulator and return omk_ssd_last_kernels()."""
    from emu.loader import use_emulator
    fn, args, kw, env = CASES[case]
    for k, v in env.items():
        setenv(k, v)
    with use_emulator():
        import omnimamba_amd.ssd_combined as S
        from omnimamba_amd import _capi as K
        from omnimamba_amd._lib import get_lib
        fn(S, K, *args, **kw)
        return get_lib().omk_ssd_last_kernels().decode()


EXPECTED = {
    "bwd-default-hg": "ssd_dt_prep;ssd_generic<mode=1>;ssd_generic<mode=2>;ssd_generic<mode=3>;ssd_bwd_finish",
    "bwd-default-odd": "ssd_dt_prep;ssd_generic<mode=1>;ssd_generic<mode=2>;ssd_generic<mode=3>;ssd_bwd_finish",
    "bwd-default-pair": "ssd_dt_prep;ssd_a6<state_dump>;ssd_a8<mode=2,dump=1,khilo=0,precise=0>;ssd_cp<direct=1,nhs=1>;ssd_bwd_finish_par",
    "bwd-sequential-hg": "ssd_dt_prep;ssd_generic<mode=1>;ssd_generic<mode=2>;ssd_generic<mode=3>;ssd_bwd_finish",
    "bwd-sequential-odd": "ssd_dt_prep;ssd_generic<mode=1>;ssd_generic<mode=2>;ssd_generic<mode=3>;ssd_bwd_finish",
    "bwd-sequential-pair": "ssd_dt_prep;ssd_mfma_b3<mode=1,dmode=0>;ssd_reduce_partials;ssd_mfma_b3<mode=3,dmode=1>;ssd_reduce_partials;ssd_a8<mode=2,dump=0,khilo=0,precise=0>;ssd_bwd_finish_par",
    "bwd-sequential-window-pair": "ssd_dt_prep;ssd_mfma_b3<mode=1,dmode=0>;ssd_reduce_partials;ssd_mfma_b3<mode=3,dmode=1>;ssd_reduce_partials;ssd_a8<mode=2,dump=0,khilo=0,precise=0>;ssd_bwd_finish_par",
    "bwd-window-hg": "ssd_dt_prep;ssd_generic<mode=1>;ssd_generic<mode=2>;ssd_generic<mode=3>;ssd_bwd_finish",
    "bwd-window-odd": "ssd_dt_prep;ssd_generic<mode=1>;ssd_generic<mode=2>;ssd_generic<mode=3>;ssd_bwd_finish",
    "bwd-window-pair": "ssd_dt_prep;ssd_a8<mode=2,dump=1,khilo=0,precise=0>;ssd_cp<direct=1,nhs=1>;ssd_bwd_finish_par",
    "final_state_raw-hg": "ssd_dt_prep;ssd_mfma_a3<state_only>",
    "final_state_raw-odd": "ssd_dt_prep;ssd_mfma_a3<state_only>",
    "final_state_raw-pair": "ssd_dt_prep;ssd_a6<state_only>",
    "fp32-bwd": "ssd_dt_prep;ssd_generic<mode=1>;ssd_generic<mode=2>;ssd_generic<mode=3>;ssd_bwd_finish",
    "fp32-final": "ssd_dt_prep;ssd_f32_mfma",
    "fp32-gate_outx": "ssd_dt_prep;ssd_f32_mfma",
    "fp32-plain": "ssd_dt_prep;ssd_f32_mfma",
    "fused_conv-refused-odd": "ssd_dt_prep",
    "fused_conv-refused-split": "ssd_dt_prep",
    "fused_conv-taken": "ssd_dt_prep;ssd_a8<mode=0,dump=0,khilo=0,precise=0,conv=1>",
    "fwd-D_hp-hg": "ssd_dt_prep;ssd_mfma_a3<mode=0,ex=0,state=0,dfold=0,khilo=0>",
    "fwd-D_hp-odd": "ssd_dt_prep;ssd_mfma_a3<mode=0,ex=0,state=0,dfold=0,khilo=0>",
    "fwd-D_hp-pair": "ssd_dt_prep;ssd_a6<mode=0,ex=0,dfold=0,dump=0,khilo=0>",
    "fwd-column_slice-hg": "ssd_dt_prep;ssd_mfma_a3<mode=0,ex=0,state=0,dfold=1,khilo=0>",
    "fwd-column_slice-odd": "ssd_dt_prep;ssd_mfma_a3<mode=0,ex=0,state=0,dfold=1,khilo=0>",
    "fwd-column_slice-pair": "ssd_dt_prep;ssd_a6<mode=0,ex=0,dfold=1,dump=0,khilo=0>",
    "fwd-every_chunk-hg": "ssd_dt_prep;ssd_mfma_a3<mode=0,ex=0,state=0,dfold=1,khilo=0>",
    "fwd-every_chunk-odd": "ssd_dt_prep;ssd_mfma_a3<mode=0,ex=0,state=0,dfold=1,khilo=0>",
    "fwd-every_chunk-pair": "ssd_dt_prep;ssd_a8<mode=0,dump=0,khilo=0,precise=0>",
    "fwd-final-hg": "ssd_dt_prep;ssd_mfma_a3<mode=0,ex=0,state=0,dfold=1,khilo=0>",
    "fwd-final-odd": "ssd_dt_prep;ssd_mfma_a3<mode=0,ex=0,state=0,dfold=1,khilo=0>",
    "fwd-final-pair": "ssd_dt_prep;ssd_a8<mode=0,dump=0,khilo=1,precise=0>",
    "fwd-force_generic-hg": "ssd_dt_prep;ssd_generic<mode=0>",
    "fwd-force_generic-odd": "ssd_dt_prep;ssd_generic<mode=0>",
    "fwd-force_generic-pair": "ssd_dt_prep;ssd_generic<mode=0>",
    "fwd-gate_outx-hg": "ssd_dt_prep;ssd_mfma_a3<mode=0,ex=1,state=0,dfold=1,khilo=0>",
    "fwd-gate_outx-odd": "ssd_dt_prep;ssd_mfma_a3<mode=0,ex=1,state=0,dfold=1,khilo=0>",
    "fwd-gate_outx-pair": "ssd_dt_prep;ssd_a6<mode=0,ex=1,dfold=1,dump=0,khilo=0>",
    "fwd-khilo-hg": "ssd_dt_prep;ssd_mfma_a3<mode=0,ex=0,state=0,dfold=1,khilo=1>",
    "fwd-khilo-odd": "ssd_dt_prep;ssd_mfma_a3<mode=0,ex=0,state=0,dfold=1,khilo=1>",
    "fwd-khilo-pair": "ssd_dt_prep;ssd_a8<mode=0,dump=0,khilo=1,precise=0>",
    "fwd-plain-hg": "ssd_dt_prep;ssd_mfma_a3<mode=0,ex=0,state=0,dfold=1,khilo=0>",
    "fwd-plain-odd": "ssd_dt_prep;ssd_mfma_a3<mode=0,ex=0,state=0,dfold=1,khilo=0>",
    "fwd-plain-pair": "ssd_dt_prep;ssd_a8<mode=0,dump=0,khilo=0,precise=0>",
    "fwd-precise-hg": "ssd_dt_prep;ssd_generic<mode=0>",
    "fwd-precise-odd": "ssd_dt_prep;ssd_generic<mode=0>",
    "fwd-precise-pair": "ssd_dt_prep;ssd_a8<mode=0,dump=0,khilo=1,precise=1>",
    "fwd-window-hg": "ssd_dt_prep;ssd_mfma_a3<mode=0,ex=0,state=0,dfold=1,khilo=0,dump=1>",
    "fwd-window-odd": "ssd_dt_prep;ssd_mfma_a3<mode=0,ex=0,state=0,dfold=1,khilo=0,dump=1>",
    "fwd-window-pair": "ssd_dt_prep;ssd_a8<mode=0,dump=1,khilo=0,precise=0>",
    "non_mfma-bwd": "ssd_dt_prep;ssd_generic<mode=1>;ssd_generic<mode=2>;ssd_generic<mode=3>;ssd_bwd_finish",
    "non_mfma-final": "ssd_dt_prep;ssd_generic<mode=0>",
    "non_mfma-gate_outx": "ssd_dt_prep;ssd_generic<mode=0>",
    "non_mfma-plain": "ssd_dt_prep;ssd_generic<mode=0>",
    "split-bwd-default-hg": "ssd_dt_prep;ssd_generic<mode=1>;ssd_generic<mode=2>;ssd_generic<mode=3>;ssd_bwd_finish",
    "split-bwd-default-odd": "ssd_dt_prep;ssd_generic<mode=1>;ssd_generic<mode=2>;ssd_generic<mode=3>;ssd_bwd_finish",
    "split-bwd-default-pair": "ssd_dt_prep;ssd_mfma_a3<segment state pass,khilo=0>;ssd_seg_fold;ssd_mfma_a3<segment state pass,khilo=0>;ssd_seg_fold;ssd_a6<state_dump>;ssd_a8<mode=2,dump=1,khilo=0,precise=0>;ssd_cp<direct=1,nhs=1>;ssd_bwd_finish_par",
    "split-bwd-sequential-pair": "ssd_dt_prep;ssd_mfma_a3<segment state pass,khilo=0>;ssd_seg_fold;ssd_mfma_a3<segment state pass,khilo=0>;ssd_seg_fold;ssd_mfma_b3<mode=1,dmode=0>;ssd_reduce_partials;ssd_mfma_b3<mode=3,dmode=1>;ssd_reduce_partials;ssd_a8<mode=2,dump=0,khilo=0,precise=0>;ssd_bwd_finish_par",
    "split-bwd-window-pair": "ssd_dt_prep;ssd_mfma_a3<segment state pass,khilo=0>;ssd_seg_fold;ssd_a8<mode=2,dump=1,khilo=0,precise=0>;ssd_cp<direct=1,nhs=1>;ssd_bwd_finish_par",
    "split-final_state_raw-hg": "ssd_dt_prep;ssd_mfma_a3<segment state pass,khilo=1>;ssd_seg_fold;ssd_mfma_a3<state_only>",
    "split-final_state_raw-odd": "ssd_dt_prep;ssd_mfma_a3<segment state pass,khilo=1>;ssd_seg_fold;ssd_mfma_a3<state_only>",
    "split-final_state_raw-pair": "ssd_dt_prep;ssd_mfma_a3<segment state pass,khilo=1>;ssd_seg_fold;ssd_a6<state_only>",
    "split-fwd-final-hg": "ssd_dt_prep;ssd_mfma_a3<segment state pass,khilo=1>;ssd_seg_fold;ssd_mfma_a3<mode=0,ex=0,state=0,dfold=1,khilo=0>",
    "split-fwd-final-odd": "ssd_dt_prep;ssd_mfma_a3<segment state pass,khilo=1>;ssd_seg_fold;ssd_mfma_a3<mode=0,ex=0,state=0,dfold=1,khilo=0>",
    "split-fwd-final-pair": "ssd_dt_prep;ssd_mfma_a3<segment state pass,khilo=1>;ssd_seg_fold;ssd_a8<mode=0,dump=0,khilo=1,precise=0>",
    "split-fwd-gate_outx-pair": "ssd_dt_prep;ssd_mfma_a3<segment state pass,khilo=0>;ssd_seg_fold;ssd_a6<mode=0,ex=1,dfold=1,dump=0,khilo=0>",
    "split-fwd-hg": "ssd_dt_prep;ssd_mfma_a3<segment state pass,khilo=0>;ssd_seg_fold;ssd_mfma_a3<mode=0,ex=0,state=0,dfold=1,khilo=0>",
    "split-fwd-odd": "ssd_dt_prep;ssd_mfma_a3<segment state pass,khilo=0>;ssd_seg_fold;ssd_mfma_a3<mode=0,ex=0,state=0,dfold=1,khilo=0>",
    "split-fwd-pair": "ssd_dt_prep;ssd_mfma_a3<segment state pass,khilo=0>;ssd_seg_fold;ssd_a8<mode=0,dump=0,khilo=0,precise=0>",
    "split-fwd-window-pair": "ssd_dt_prep;ssd_mfma_a3<segment state pass,khilo=0>;ssd_seg_fold;ssd_a8<mode=0,dump=1,khilo=0,precise=0>",
}


def test_every_case_has_an_expected_string():
    assert sorted(CASES) == sorted(EXPECTED)


@pytest.mark.parametrize("case", sorted(CASES))
def test_ssd_dispatch(case, monkeypatch):
    assert launched(case, monkeypatch.setenv) == EXPECTED[case]
