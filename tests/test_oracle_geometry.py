"""CPU: pins oracle/ref_cpu.py to the reference's own DiT at patch geometries other than (patch 2, 16 channels) — fixture G14
(tools/make_golden.py g14_geometry -> tests/golden/g14_geometry.safetensors): forward, loss, autograd gradients and one denoise_step.
fp32 against fp32 on the same ATen kernels: the bound of tests/test_oracle_golden.py, 2e-5 relative L2."""
import os

import pytest
import torch
from safetensors.torch import load_file

from oracle import ref_cpu as O
import gtav_amd.weights as W

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g14_geometry.safetensors")
TOL = 2e-5
SMALL = dict(hidden_size=256, depth=2, num_heads=4, external_cond_dim=25)
G14_GEOMETRIES = {"p4c4": dict(input_h=16, input_w=32, patch_size=4, in_channels=4), "p2c8": dict(input_h=8, input_w=16, patch_size=2, in_channels=8)}
GEOMETRY_WEIGHTS = ("x_embedder.proj.weight", "final_layer.linear.weight")


def rel(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30)).item()


def g14_sel(name, v):
    """The elements G14 keeps of a gradient (tools/make_golden.py g14_sel)."""
    if v.numel() <= 512:
        return v.reshape(-1)
    return v.reshape(-1)[::97 if name in GEOMETRY_WEIGHTS else 997]


def test_fixture_holds_data_only_and_is_small():
    assert os.path.getsize(GOLD) < 300 * 1024
    g = load_file(GOLD)
    assert all(torch.is_tensor(v) for v in g.values()) and {k.split(".")[0] for k in g} == set(G14_GEOMETRIES)


@pytest.mark.parametrize("tag", sorted(G14_GEOMETRIES))
def test_g14_oracle_matches_the_reference_at_other_patch_geometries(tag):
    g = {k[len(tag) + 1:]: v for k, v in load_file(GOLD).items() if k.startswith(tag + ".")}
    kw = dict(SMALL, **G14_GEOMETRIES[tag])
    sd = W.synth_state_dict(W.dit_param_shapes(**kw), seed=3)
    cfg = O.DiTConfig(**kw)
    loss, v_pred, grads = O.dit_loss_and_grads(sd, cfg, g["x"], g["t"], g["actions"], g["v_target"])
    assert v_pred.shape == g["x"].shape
    assert rel(v_pred, g["v_pred"]) < TOL and abs(float(loss) - float(g["loss"])) < TOL * float(g["loss"])
    names = sorted(grads)
    assert len(names) == int(g["names_check"])
    assert rel(torch.stack([grads[k].norm() for k in names]), g["grad_norms"]) < TOL
    for k in names:
        assert rel(g14_sel(k, grads[k]), g["grad." + k]) < TOL, k
    ac = O.alphas_cumprod_table(1e-4)[:, None, None, None]
    fn = lambda x, t, a: O.dit_forward(sd, cfg, x, t, a)
    with torch.no_grad():
        xp, _ = O.denoise_step(fn, g["x"], g["actions"], 50, 15, torch.linspace(0, 999, 51), ac, start_frame=0)
    assert rel(xp[:, -1:], g["x_pred_last_50"]) < TOL
