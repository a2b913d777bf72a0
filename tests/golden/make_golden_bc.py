"""Generate the behaviour-cloning fixtures by running the REFERENCE's GaussianModel.loss / GMMModel.loss on the CPU:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_bc.py <checkout of the reference (the directory holding dppo/)>

Writes tests/golden/g22_gaussian_bc.npz and g23_gmm_bc.npz: per case the inputs (state, true_action), the reference's loss and
entropy, and every parameter gradient of loss.backward() (large tensors as flat[::61] + norm + sum, like make_golden.py's
put_grad).  Weights are never stored: both sides rebuild them from ``oracle.dppo_oracle.init_params`` and the logvar recipes
in make_golden_bc_cases.py.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.dont_write_bytecode = True

from oracle import dppo_oracle as O  # noqa: E402  (seeded weight recipe + specs only)
from tests.golden.make_golden_bc_cases import (BC_CLAMPED, BC_GAUSS_CASES, BC_GMM_KINDS, BC_GMM_NETS, BC_LOGVAR_SEED,  # noqa: E402
                                               BC_N, BC_WEIGHT_SEED, clamp_mask, gauss_logvar, gmm_logvar)
from tests.golden.make_golden_cases import GAUSS_CASES  # noqa: E402

torch.set_num_threads(4)
GRAD_STRIDE = 61
T = torch.from_numpy


def save(name, out):
    arrays = {k: np.asarray(v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in out.items()}
    np.savez_compressed(os.path.join(HERE, name + ".npz"), **arrays)
    print(f"wrote {name}.npz: {len(arrays)} arrays, {sum(v.nbytes for v in arrays.values())} bytes raw")


def put_grad(out, key, g):
    g = g.detach().cpu().numpy()
    if g.size > 4096:
        out[key + "__sub"] = g.reshape(-1)[::GRAD_STRIDE].copy()
        out[key + "__norm"] = np.float64(np.sqrt((g.astype(np.float64) ** 2).sum()))
        out[key + "__sum"] = np.float64(g.astype(np.float64).sum())
    else:
        out[key] = g


def put_case(out, name, state, action, loss, info, net):
    assert torch.isfinite(loss), name
    loss.backward()
    out.update({f"{name}_state": state, f"{name}_true_action": action, f"{name}_loss": np.float64(loss.item()),
                f"{name}_entropy": np.float64(info["entropy"].item())})
    for k, p in net.named_parameters():
        if p.grad is not None:
            assert torch.isfinite(p.grad).all(), (name, k)
            put_grad(out, f"{name}_g_{k}", p.grad)
    print(f"  {name}: loss {loss.item():.4f} entropy {info['entropy'].item():.4f}")


def g22_gaussian_bc():
    from dppo.model.common.gaussian import GaussianModel
    from dppo.model.common.mlp_gaussian import Gaussian_MLP
    out = {}
    rs = np.random.RandomState(2200)
    N = BC_N
    for cname, ent_coef in BC_GAUSS_CASES.items():
        sname, kw = GAUSS_CASES[cname]
        a, _ = O.named_specs(sname)
        Ta, Da = a.horizon_steps, a.action_dim
        actor = Gaussian_MLP(action_dim=Da, horizon_steps=Ta, cond_dim=a.cond_dim, mlp_dims=list(a.mlp_dims),
                             activation_type=a.activation, residual_style=True, fixed_std=kw["fixed_std"],
                             learn_fixed_std=kw["learn_fixed_std"], std_min=kw["std_min"], std_max=kw["std_max"])
        sd = dict(O.init_params(a, BC_WEIGHT_SEED))
        sd["logvar_min"], sd["logvar_max"] = actor.logvar_min.data.clone(), actor.logvar_max.data.clone()
        lv = gauss_logvar(cname, Da, kw, BC_LOGVAR_SEED)
        if lv is not None:
            sd["logvar"] = T(lv)
        actor.load_state_dict(sd, strict=True)
        m = GaussianModel(network=actor, horizon_steps=Ta, device="cpu")
        if lv is not None:  # the reference module's own clamp mask: zeros exactly in the BC_CLAMPED cases
            inside = (actor.logvar >= actor.logvar_min) & (actor.logvar <= actor.logvar_max)
            assert (cname in BC_CLAMPED) == (not bool(inside.all())) and np.array_equal(inside.numpy(), clamp_mask(lv, kw)), cname
        state = T(rs.uniform(-1, 1, size=(N, 1, a.cond_dim)).astype(np.float32))
        with torch.no_grad():
            mean, scale = actor({"state": state})
        # first half: expert-like actions around the policy's mean (2 sigma); second half: anywhere in the action box
        near = mean + 2.0 * scale * T(rs.randn(N, Ta * Da).astype(np.float32))
        far = T(rs.uniform(-1, 1, size=(N, Ta * Da)).astype(np.float32))
        action = torch.where(torch.arange(N).view(N, 1) < N // 2, near, far).clamp(-1, 1).view(N, Ta, Da)
        loss, info = m.loss(action, {"state": state}, ent_coef)
        out[f"{cname}_ent_coef"] = np.float64(ent_coef)
        put_case(out, cname, state, action, loss, info, actor)
    save("g22_gaussian_bc", out)


def g23_gmm_bc():
    from dppo.model.common.gmm import GMMModel
    from dppo.model.common.mlp_gmm import GMM_MLP
    out = {}
    rs = np.random.RandomState(2300)
    N = BC_N
    for nname in sorted(BC_GMM_NETS):
        cond, tkw, Ta, Da, gkw = BC_GMM_NETS[nname]
        M = gkw["num_modes"]
        ms, ws = O.gmm_specs(cond, tkw["mlp_dims"], tkw["activation"], tkw["residual"], Da, Ta, M)
        for kind in BC_GMM_KINDS:
            actor = GMM_MLP(action_dim=Da, horizon_steps=Ta, cond_dim=cond, mlp_dims=list(tkw["mlp_dims"]), num_modes=M,
                            activation_type=tkw["activation"], residual_style=tkw["residual"], fixed_std=gkw["fixed_std"],
                            learn_fixed_std=gkw["learn_fixed_std"], std_min=gkw["std_min"], std_max=gkw["std_max"])
            sd = dict(O.gmm_init_params(ms, ws, BC_WEIGHT_SEED))
            sd["logvar_min"], sd["logvar_max"] = actor.logvar_min.data.clone(), actor.logvar_max.data.clone()
            lv = gmm_logvar(nname, Da, gkw, BC_LOGVAR_SEED)
            if lv is not None:
                sd["logvar"] = T(lv)
            actor.load_state_dict(sd, strict=True)
            m = GMMModel(network=actor, horizon_steps=Ta, device="cpu")
            if lv is not None:
                inside = (actor.logvar >= actor.logvar_min) & (actor.logvar <= actor.logvar_max)
                assert (nname in BC_CLAMPED) == (not bool(inside.all())) and np.array_equal(inside.numpy(), clamp_mask(lv, gkw)), nname
            state = T(rs.uniform(-1, 1, size=(N, 1, cond)).astype(np.float32))
            with torch.no_grad():
                means, _, _ = actor({"state": state})  # (N, M, Ta*Da)
            rows = torch.arange(N)
            if kind == "near":
                k = T(rs.randint(0, M, size=N))
                action = means[rows, k] + 0.02 * T(rs.randn(N, Ta * Da).astype(np.float32))
            elif kind == "between":
                k1 = T(rs.randint(0, M, size=N))
                k2 = (k1 + T(rs.randint(1, M, size=N))) % M  # a different component
                action = 0.5 * (means[rows, k1] + means[rows, k2])
            else:
                action = T(rs.uniform(-1, 1, size=(N, Ta * Da)).astype(np.float32))
            action = action.clamp(-1, 1).view(N, Ta, Da)
            loss, info = m.loss(action, {"state": state})
            put_case(out, f"{nname}_{kind}", state, action, loss, info, actor)
    save("g23_gmm_bc", out)


if __name__ == "__main__":
    sys.path.insert(0, os.path.abspath(sys.argv[1]))
    only = sys.argv[2:]
    for fn in (g22_gaussian_bc, g23_gmm_bc):
        if not only or fn.__name__ in only:
            fn()
