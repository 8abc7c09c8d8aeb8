"""Drop-in check against the reference's OWN Block (models/stage2/block.py): tests/golden/reference_block.npz holds its state dicts,
inputs and outputs, captured by tests/golden/make_golden.py from the unmodified Block running on the oracle-backed `mamba_ssm`
provider.  The Block reaches its operators through `mamba_ssm.ops.triton.layer_norm` and the mixer / MLP classes it is handed; this
repo's facade of those names -- run on the HIP sources under the emulator -- must load the Block's state dict and reproduce its numbers."""
import os

import numpy as np
import torch

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_block.npz")


def rel(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30)).item()


def load(key):
    g = np.load(GOLD)
    t = lambda name: torch.from_numpy(g[f"{key}.{name}"])
    sd = {k[len(key) + 4:]: torch.from_numpy(g[k]) for k in g.files if k.startswith(f"{key}.sd.")}
    return g, t, sd


def test_reference_block_runs_on_our_operators():
    from emu.loader import use_emulator
    from omnimamba_amd.stack import ResidualBlock, StackConfig
    g, t, sd = load("mixer")
    with use_emulator():
        ours = ResidualBlock(32, 0, StackConfig(d_model=32, n_layer=1, ssm_cfg=dict(d_state=16, headdim=8, chunk_size=16)))
        ours.load_state_dict(sd, strict=True)
        with torch.no_grad():
            y, r = ours(t("h"), t("res"))
            assert r.dtype == torch.float32 and torch.equal(r, t("r")) and rel(y, t("y")) < 2e-5
            with torch.autocast("cpu", dtype=torch.bfloat16):   # training runs under bf16 AMP (train_stage2.py:21,37)
                y, r = ours(t("h").bfloat16(), None)             # first block: residual=None, bf16 activations, fp32 residual out
        assert r.dtype == torch.float32 and y.dtype == torch.bfloat16
        assert torch.equal(r, t("amp_r")) and rel(y.float(), t("amp_y")) < 4e-3


def test_reference_block_with_a_gated_mlp():
    """d_intermediate > 0 (no shipped config, but create_block builds it: mixer_seq_simple.py:168-230): the reference's Block with a
    GatedMLP as mlp_cls -- second fused add + norm, then the MLP -- against the same composition on this repo's facade."""
    from functools import partial
    from emu.loader import use_emulator
    from mamba_ssm.modules.mamba2 import Mamba2
    from mamba_ssm.modules.mlp import GatedMLP
    from mamba_ssm.ops.triton.layer_norm import RMSNorm, layer_norm_fn
    g, t, sd = load("mlp")
    with use_emulator():
        blk = torch.nn.Module()
        blk.norm, blk.norm2 = RMSNorm(32, eps=1e-5), RMSNorm(32, eps=1e-5)
        blk.mixer = Mamba2(32, layer_idx=0, d_state=16, headdim=8, chunk_size=16)
        blk.mlp = GatedMLP(32, hidden_features=40, out_features=32, multiple_of=16)
        assert blk.mlp.fc1.weight.shape == (96, 32) and blk.mlp.fc2.weight.shape == (32, 48)      # 40 -> 48 = next multiple of 16
        blk.load_state_dict(sd, strict=True)
        add_norm = partial(layer_norm_fn, prenorm=True, residual_in_fp32=True, eps=1e-5, is_rms_norm=True)
        with torch.no_grad():
            hn, r = add_norm(t("h"), blk.norm.weight, None, residual=t("res"))
            hn2, r = add_norm(blk.mixer(hn), blk.norm2.weight, None, residual=r)
            y = blk.mlp(hn2, task_types=None)
    assert r.dtype == torch.float32 and rel(r, t("r")) < 2e-5 and rel(y, t("y")) < 2e-5
