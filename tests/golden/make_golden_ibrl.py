"""Generate the IBRL fixture by running the REFERENCE's IBRL_Gaussian / Gaussian_MLP / CriticObsAct on the CPU:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_ibrl.py <checkout of the reference (the directory holding dppo/)>

Writes tests/golden/g31_ibrl.npz.  Per case (make_golden_ibrl_cases.CASES): ``loss_critic`` with ``get_random_indices`` pinned to the
case's pair (the loss, {loss, mean q, mean y} and y rebuilt from the reference's own modules, every member's gradients as ONE flat
vector per member, in state-dict order: its row of the [E][P] image) and ``forward``, greedy and soft (the chosen actions, both
proposals and took_bc).  Draws are replaced: ``Normal.sample`` / ``rsample`` hand back the recipe's noise (make_golden_sac.
recorded_draws), every ``nn.Dropout`` of the three actors is swapped for a module that multiplies by the recorded mask over 1 - p
-- after one tensor showed that this is ``nn.Dropout``'s own output for its mask -- and ``torch.multinomial`` of the soft choice
takes index 0 iff u < weights[:, 0].  Where both weights overflow the softmax is NaN and the real ``torch.multinomial`` raises
(asserted here): that row's took_bc is stored as 2.  The state-dict keys and shapes.  Large tensors as flat[::61] + norm
(make_golden_bc.put_grad).  Weights and inputs are never stored: both sides rebuild them from make_golden_ibrl_cases.py.

The reference stacks ``ensemble_params`` at construction and differentiates THOSE: after the members are loaded they are stacked
again here.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.dont_write_bytecode = True

from tests.golden import make_golden_ibrl_cases as K  # noqa: E402
from tests.golden.make_golden_bc import put_grad, save  # noqa: E402
from tests.golden.make_golden_rlpd import member_flat  # noqa: E402
from tests.golden.make_golden_sac import recorded_draws  # noqa: E402

torch.set_num_threads(4)


class MaskMul(torch.nn.Module):
    """Stands in for nn.Dropout(p) in train(): x * (mask / (1 - p)) with the mask set before the call."""

    def __init__(self, p):
        super().__init__()
        self.p, self.mask = p, None

    def forward(self, x):
        return x * (self.mask.to(x.dtype) / (1 - self.p))


def check_mask_mul_is_dropout(p=0.25):
    x = torch.randn(33, 128)
    torch.manual_seed(7)
    y = torch.nn.Dropout(p)(x)
    mask = (y != 0).to(torch.uint8)  # (no entry of x is 0)
    m = MaskMul(p)
    m.mask = mask
    assert (x != 0).all() and 0 < int(mask.sum()) < mask.numel() and torch.equal(m(x), y)


def swap_dropout(actor):
    """[MaskMul per hidden layer], in layer order."""
    out = []
    for layer in actor.mlp_mean.moduleList:
        if hasattr(layer, "dropout_1"):
            assert isinstance(layer.dropout_1, torch.nn.Dropout)
            layer.dropout_1 = MaskMul(layer.dropout_1.p)
            out.append(layer.dropout_1)
    return out


def set_masks(mods, mask):
    for i, m in enumerate(mods):
        m.mask = mask[i]


def ref_model(case, soft):
    from dppo.model.common.critic import CriticObsAct
    from dppo.model.common.mlp_gaussian import Gaussian_MLP
    from dppo.model.rl.gaussian_ibrl import IBRL_Gaussian
    od, ta, da, dims, act, p, qdims, qact, E = K.IBRL_NETS[case]
    actor = Gaussian_MLP(action_dim=da, horizon_steps=ta, cond_dim=od, mlp_dims=list(dims), activation_type=act, dropout=p,
                         fixed_std=K.FIXED_STD)
    q = CriticObsAct(cond_dim=od, mlp_dims=list(qdims), action_dim=da, action_steps=ta, activation_type=qact, use_layernorm=True,
                     double_q=False)
    m = IBRL_Gaussian(actor=actor, critic=q, n_critics=E, soft_action_sample=soft, soft_action_sample_beta=K.BETA, horizon_steps=ta,
                      device="cpu", randn_clip_value=K.RANDN_CLIP)
    m.train()  # as the reference's agent leaves it: dropout is live in all three actors
    for name, net in (("bc", m.bc_policy), ("rl", m.network), ("target", m.target_actor)):
        net.load_state_dict(K.actor_state_dict(case, name), strict=True)
    for e in range(E):
        m.critic_networks[e].load_state_dict(K.member_params(case, e), strict=True)
        m.target_networks[e].load_state_dict(K.member_params(case, e, K.TARGET_EPS), strict=True)
    m.ensemble_params, m.ensemble_buffers = torch.func.stack_module_state(m.critic_networks)
    m.get_random_indices = lambda *a, **k: torch.tensor(K.pair_of(case))
    mods = {name: swap_dropout(net) for name, net in (("bc", m.bc_policy), ("rl", m.network), ("target", m.target_actor))}
    return m, mods


class given_uniform:
    """``torch.multinomial(weights, 1)`` takes index 0 iff u < weights[:, 0]; the rows whose weights are NaN are recorded (the
    real one raises on them) and take index 1."""

    def __init__(self, u):
        self.u, self.nan_rows = u, None

    def __enter__(self):
        self.real = torch.multinomial

        def stand_in(w, k):
            assert k == 1 and w.shape[1] == 2
            self.nan_rows = torch.isnan(w).any(dim=1)
            if self.nan_rows.any():
                try:
                    self.real(w, 1)
                    raise AssertionError("torch.multinomial took NaN weights")
                except RuntimeError:
                    pass
            self.index = (~(self.u < w[:, 0])).long()[:, None]
            return self.index
        torch.multinomial = stand_in
        return self

    def __exit__(self, *a):
        torch.multinomial = self.real


def one_forward(out, case, n, soft):
    from dppo.model.common.gaussian import GaussianModel
    b = K.forward_inputs(case, n)
    m, mods = ref_model(case, soft)
    cond = {"state": b["obs"]}
    set_masks(mods["bc"], b["mask_bc"])
    set_masks(mods["rl"], b["mask_rl"])
    with torch.no_grad(), recorded_draws([b["noise_bc"], b["noise_rl"]]), given_uniform(b["u"]) as gu:
        action = m(cond, deterministic=False)
    with torch.no_grad(), recorded_draws([b["noise_bc"], b["noise_rl"]]):
        a_bc = GaussianModel.forward(m, cond=cond, deterministic=True, network_override=m.bc_policy)
        a_rl = GaussianModel.forward(m, cond=cond, deterministic=False)
    action, a_bc, a_rl = (t.reshape(n, -1) for t in (action, a_bc, a_rl))
    is_bc, is_rl = (action == a_bc).all(dim=1), (action == a_rl).all(dim=1)
    assert (is_bc | is_rl).all()
    took = (is_bc & ~is_rl).to(torch.uint8)  # a row whose proposals are equal took RL: torch.where's else branch
    if soft:  # the index the model drew, which on the tie row the actions cannot tell
        assert torch.equal(took[~(is_bc & is_rl)], (gu.index[:, 0] == 0).to(torch.uint8)[~(is_bc & is_rl)])
        took = (gu.index[:, 0] == 0).to(torch.uint8)
        took[gu.nan_rows] = 2
    key = f"{case}_{n}_{'soft' if soft else 'greedy'}"
    out.update({f"{key}_action": action.numpy().copy(), f"{key}_took_bc": took.numpy().copy()})
    if not soft:
        out.update({f"{case}_{n}_a_bc": a_bc.numpy().copy(), f"{case}_{n}_a_rl": a_rl.numpy().copy()})
    print(f"  {key}: took BC in {int((took == 1).sum())} of {n} rows, {int((took == 2).sum())} NaN rows")


def one_critic(out, case, n):
    b = K.inputs(case, n)
    m, mods = ref_model(case, False)
    cond, ncond = {"state": b["obs"]}, {"state": b["next_obs"]}
    set_masks(mods["bc"], b["mask_bc"])
    set_masks(mods["target"], b["mask_rl"])
    with recorded_draws([b["noise_bc"], b["noise_rl"]]):
        lc = m.loss_critic(cond, ncond, b["actions"], b["reward"], b["terminated"], K.GAMMA)
    lc.backward()
    grads = [p.grad for p in m.ensemble_params.values()]
    assert all(g is not None and torch.isfinite(g).all() for g in grads)
    name = f"{case}_{n}"
    for e in range(len(m.critic_networks)):
        put_grad(out, f"{name}_gq_{e}", member_flat(grads, e))
    # the target and the statistics, rebuilt from the reference's own modules on the same draws
    from dppo.model.common.gaussian import GaussianModel
    with torch.no_grad(), recorded_draws([b["noise_bc"], b["noise_rl"]]):
        a_bc = GaussianModel.forward(m, cond=ncond, deterministic=True, network_override=m.bc_policy)
        a_rl = GaussianModel.forward(m, cond=ncond, deterministic=False, network_override=m.target_actor)
        i, j = K.pair_of(case)
        mb = torch.min(m.target_networks[i](ncond, a_bc), m.target_networks[j](ncond, a_bc))
        mr = torch.min(m.target_networks[i](ncond, a_rl), m.target_networks[j](ncond, a_rl))
        y = b["reward"] + K.GAMMA * (1 - b["terminated"]) * torch.where(mb > mr, mb, mr)
        q = torch.stack([net(cond, b["actions"]) for net in m.critic_networks])
        rebuilt = torch.mean((q - y[None]) ** 2).item()  # (vmap's batched products round differently from the modules' own)
        assert abs(rebuilt - lc.item()) <= 1e-6 * abs(lc.item()), (rebuilt, lc.item())
    out.update({f"{name}_c_loss": np.float64(lc.item()), f"{name}_stats": np.array([lc.item(), q.mean().item(), y.mean().item()]),
                f"{name}_y": y.numpy().copy(), f"{name}_bc_share": np.float64((mb > mr).double().mean().item())})
    print(f"  {name}: critic {lc.item():.6f} bc share {(mb > mr).double().mean().item():.3f}")


def main():
    check_mask_mul_is_dropout()
    out = {}
    for case, n in K.CASES:
        one_critic(out, case, n)
        for soft in (False, True):
            one_forward(out, case, n, soft)
    m, _ = ref_model("tiny", False)
    sd = m.state_dict()
    out["state_dict_keys"] = np.array(list(sd))
    out["state_dict_shapes"] = np.array([",".join(str(s) for s in v.shape) for v in sd.values()])
    save("g31_ibrl", out)


if __name__ == "__main__":
    sys.path.insert(0, os.path.abspath(sys.argv[1]))
    main()
