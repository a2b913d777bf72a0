"""Dropout in the forward of a plain trunk (reference model/common/mlp.py:59-60: ``nn.Dropout`` behind every Linear but the last, in
front of the activation), the actor of seven of the eight shipped IBRL cfgs: csrc/ibrl.h's row kernel behind the unchanged GEMM,
``dppo_gaussian_sample_drop`` and ``GaussianModel._sample``'s use of it.

CPU: the plain ``MLP`` and ``Gaussian_MLP(plain_fixed_std=True)`` carry the reference's state dict (``nn.Dropout`` has no
parameters), the per-call struct follows the module's mode, and a mask of the wrong shape is refused.
GPU: the mask drawn in the kernel (Philox4x32-10, counter (l M + m) H + h, keep iff u >= p) on one small shape, 64 rows x 1024 wide
x 2 hidden layers: the same seed gives the same mask and the same bits, another seed another mask, the written-out mask fed back as
the given mask reproduces the output bit for bit, the kept share lies within 5 binomial standard deviations of 1 - p (computed here
from the count), and p = 0 under ``train()`` or any p under ``eval()`` is ``dppo_gaussian_sample`` bit for bit.  The given-mask
parity against float64 is tests/test_ibrl.py's.
"""
import ctypes as C
import math

import pytest
import torch

from dppo_amd import hip

DEV = "cuda:0"
ROWS, WIDTH, OBS, DA = 64, 1024, 23, 7


def make_actor(p=0.5, act="ReLU", prec="fp32", dims=(WIDTH, WIDTH)):
    from dppo_amd.model.common.mlp_gaussian import Gaussian_MLP
    torch.manual_seed(11)
    return Gaussian_MLP(DA, 1, OBS, mlp_dims=list(dims), activation_type=act, dropout=p, fixed_std=0.1, precision=prec,
                        plain_fixed_std=True)


def make_model(net):
    from dppo_amd.model.common.gaussian import GaussianModel
    return GaussianModel(network=net, horizon_steps=1, device=net.mlp_mean.moduleList[0].linear_1.weight.device, randn_clip_value=3)


# ------------------------------------------------------------------------------------------------------------------ CPU
def test_dropout_trunk_carries_the_references_state_dict():
    from dppo_amd.model.common.mlp import MLP
    plain, dropped = MLP([14, 64, 64, 3], activation_type="Mish"), MLP([14, 64, 64, 3], activation_type="Mish", dropout=0.25)
    assert list(plain.state_dict()) == list(dropped.state_dict()) == [f"moduleList.{i}.linear_1.{w}" for i in range(3) for w in ("weight", "bias")]
    drops = [m for m in dropped.modules() if isinstance(m, torch.nn.Dropout)]
    assert [d.p for d in drops] == [0.25, 0.25] and not hasattr(dropped.moduleList[2], "dropout_1") and dropped.dropout == 0.25
    assert plain.dropout == 0.0 and not any(isinstance(m, torch.nn.Dropout) for m in plain.modules())
    with pytest.raises(ValueError):
        MLP([14, 64, 64, 3], activation_type="Mish", dropout=1.0)
    a = make_actor(0.5, dims=(64, 64))
    # (a module's own parameters come before its children's in a state dict, in the reference's too)
    assert list(a.state_dict()) == ["logvar_min", "logvar_max"] + [f"mlp_mean.moduleList.{i}.linear_1.{w}" for i in range(3) for w in ("weight", "bias")]
    d = a.net_desc()
    assert (d.kind, d.plain, d.use_layernorm, d.in_dim, d.hidden, d.n_blocks, d.out_dim) == (1, 1, 0, OBS, 64, 1, DA)
    assert a.flat_params().numel() == hip.load().dppo_net_param_count(C.byref(d))
    cfg = a.gaussian_cfg(randn_clip=3.0)
    assert cfg.tanh_mean == 1 and cfg.std_mode == 0 and abs(cfg.fixed_std - 0.1) < 1e-7


def test_the_per_call_struct_follows_the_modules_mode():
    a = make_actor(0.5, dims=(64, 64))
    m = make_model(a)
    drop, keep, out = m._dropout_of(a, 5, "cpu", want_mask=False)
    assert drop is not None and drop.p == 0.5 and drop.mask is None and drop.mask_out is None and (drop.seed_lo or drop.seed_hi)
    mask = torch.ones(2, 5, 64, dtype=torch.uint8)
    drop, keep, out = m._dropout_of(a, 5, "cpu", mask, want_mask=True)
    assert drop.mask == keep[0].data_ptr() and drop.mask_out == out.data_ptr() and tuple(out.shape) == (2, 5, 64)
    with pytest.raises(ValueError, match="drop_mask must be"):
        m._dropout_of(a, 5, "cpu", torch.ones(2, 4, 64, dtype=torch.uint8))
    a.eval()
    assert m._dropout_of(a, 5, "cpu")[0] is None
    with pytest.raises(ValueError, match="dropout is off"):
        m._dropout_of(a, 5, "cpu", mask)
    z = make_actor(0.0, dims=(64, 64))
    assert z.training and make_model(z)._dropout_of(z, 5, "cpu")[0] is None
    with pytest.raises(NotImplementedError, match="sampled through GaussianModel"):
        make_actor(0.5, dims=(64, 64))({"state": torch.zeros(2, 1, OBS)})


# ------------------------------------------------------------------------------------------------------------------ GPU
def drawn(m, obs, noise, seed):
    torch.manual_seed(seed)
    a, mu = m._sample(m.network, {"state": obs}, False, noise, want_mean=True, want_mask=True)
    return a.clone(), mu.clone(), m.last_drop_mask.clone()


@pytest.mark.gpu
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("act,p", [("ReLU", 0.5), ("Mish", 0.25)])
def test_hip_dropout_drawn_in_the_kernel(act, p, prec):
    m = make_model(make_actor(p, act, prec).to(DEV))
    g = torch.Generator().manual_seed(3)
    obs, noise = torch.randn(ROWS, 1, OBS, generator=g).to(DEV), torch.randn(ROWS, 1, DA, generator=g).to(DEV)
    a1, mu1, k1 = drawn(m, obs, noise, 5)
    a2, mu2, k2 = drawn(m, obs, noise, 5)
    assert torch.equal(k1, k2) and torch.equal(a1, a2) and torch.equal(mu1, mu2)
    a3, mu3, k3 = drawn(m, obs, noise, 6)
    assert not torch.equal(k1, k3) and not torch.equal(mu1, mu3)
    assert tuple(k1.shape) == (2, ROWS, WIDTH) and int(k1.max()) == 1 and set(k1.unique().tolist()) == {0, 1}
    a4, mu4 = m._sample(m.network, {"state": obs}, False, noise, want_mean=True, drop_mask=k1, want_mask=True)
    assert torch.equal(a4, a1) and torch.equal(mu4, mu1) and torch.equal(m.last_drop_mask, k1)
    for k in (k1, k3):
        count, total = int(k.sum()), k.numel()
        sd = math.sqrt(total * p * (1 - p))
        print(f"{act} p={p} {prec}: kept {count} of {total}: {(count - total * (1 - p)) / sd:+.2f} standard deviations")
        assert abs(count - total * (1 - p)) <= 5 * sd
        per_layer = k.reshape(2, -1).sum(dim=1).double()
        assert ((per_layer - total / 2 * (1 - p)).abs() <= 5 * math.sqrt(total / 2 * p * (1 - p))).all()
    assert (k1[0] != k1[1]).any() and (k1[:, 0] != k1[:, 1]).any()  # layers and rows draw their own


@pytest.mark.gpu
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_hip_dropout_off_is_the_sample_without_it(prec):
    """``eval()`` with any p, and p = 0 under ``train()``, are ``dppo_gaussian_sample`` bit for bit: through the model (which then
    makes that very call) and through ``dppo_gaussian_sample_drop`` handed p = 0 and no mask."""
    net = make_actor(0.5, "Mish", prec).to(DEV)
    m = make_model(net)
    g = torch.Generator().manual_seed(4)
    obs, noise = torch.randn(ROWS, 1, OBS, generator=g).to(DEV), torch.randn(ROWS, 1, DA, generator=g).to(DEV)
    lib, d, cfg = hip.load(), net.net_desc(), net.gaussian_cfg(randn_clip=3.0)
    ws = torch.zeros(lib.dppo_gaussian_workspace_bytes(C.byref(d), None, m.prec, ROWS), dtype=torch.uint8, device=DEV)
    flat_obs, flat_noise = obs.reshape(ROWS, -1).contiguous(), noise.reshape(ROWS, -1).contiguous()

    def call(drop):
        a, mu = torch.empty(ROWS, DA, device=DEV), torch.empty(ROWS, DA, device=DEV)
        common = (C.byref(d), m.prec, net.flat_params().data_ptr(), net.packed(m.prec, 0).data_ptr(), C.byref(cfg), None,
                  flat_obs.data_ptr(), flat_noise.data_ptr(), ROWS, a.data_ptr(), mu.data_ptr())
        if drop is None:
            hip.check(lib.dppo_gaussian_sample(*common, ws.data_ptr(), ws.numel(), hip.stream()), "dppo_gaussian_sample")
        else:
            hip.check(lib.dppo_gaussian_sample_drop(*common, C.byref(drop), ws.data_ptr(), ws.numel(), hip.stream()), "dppo_gaussian_sample_drop")
        return a, mu
    want_a, want_mu = call(None)
    zero = hip.Dropout(p=0.0, seed_lo=1, seed_hi=2, pad=0, mask=None, mask_out=None)
    got_a, got_mu = call(zero)
    assert torch.equal(got_a, want_a) and torch.equal(got_mu, want_mu)
    ones = torch.ones(2, ROWS, WIDTH, dtype=torch.uint8, device=DEV)  # a given all-keep mask at p = 0 runs the row kernel: the same values
    kept = hip.Dropout(p=0.0, seed_lo=0, seed_hi=0, pad=0, mask=ones.data_ptr(), mask_out=None)
    ka, kmu = call(kept)
    assert (ka - want_a).abs().max() <= (1e-5 if prec == "fp32" else 2e-2) and (kmu - want_mu).abs().max() <= (1e-5 if prec == "fp32" else 2e-2)
    net.eval()
    ea, emu = m._sample(net, {"state": obs}, False, noise, want_mean=True)
    assert torch.equal(ea.reshape(ROWS, -1), want_a) and torch.equal(emu, want_mu)
    net.train()
    da, dmu = m._sample(net, {"state": obs}, False, noise, want_mean=True)
    assert not torch.equal(dmu, want_mu)
    z = make_actor(0.0, "Mish", prec).to(DEV)
    z.load_state_dict(net.state_dict())
    za, zmu = make_model(z)._sample(z, {"state": obs}, False, noise, want_mean=True)
    assert z.training and torch.equal(za.reshape(ROWS, -1), want_a) and torch.equal(zmu, want_mu)
