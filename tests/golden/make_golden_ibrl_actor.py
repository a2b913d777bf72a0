"""Generate the fixture of IBRL's actor loss by running the REFERENCE's IBRL_Gaussian.loss_actor on the CPU:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_ibrl_actor.py <checkout of the reference (the directory holding dppo/)>

Writes tests/golden/g32_ibrl_actor.npz.  Per case of make_golden_ibrl_actor_cases.CASES: the loss, d_a (the gradient at the sampled
action, retained where ``GaussianModel.forward`` hands it over), every actor gradient (large tensors as flat[::61] + norm, make_golden_bc.put_grad)
and the selected member per row, recomputed in float64 from the reference's own modules.  The draws are replaced as in
make_golden_ibrl.py (imported, not edited): ``rsample`` hands back the recipe's noise, every ``nn.Dropout`` of the online actor is a
``MaskMul`` with the recorded mask, and the members are restacked into ``ensemble_params`` after loading.  The conditions on the cases
(make_golden_ibrl_actor_cases.check_conditions) are asserted before anything is written.  Then one update sequence on tiny, N = 77, in
the agent's order (reference train_ibrl_agent.py:245-297): two critic AdamW steps on ``ensemble_params`` (both updates' member gradients are
kept: a member's two-step bound needs both), each followed by ``update_target_critic``, one actor step, ``update_target_actor``.  Weights and inputs are never stored.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.dont_write_bytecode = True

from tests.golden import make_golden_ibrl_actor_cases as A  # noqa: E402
from tests.golden.make_golden_bc import put_grad, save  # noqa: E402
from tests.golden.make_golden_ibrl import check_mask_mul_is_dropout, set_masks, swap_dropout  # noqa: E402
from tests.golden.make_golden_rlpd import member_flat  # noqa: E402
from tests.golden.make_golden_sac import recorded_draws  # noqa: E402

K = A.K
torch.set_num_threads(4)


def ref_model(case):
    from dppo.model.common.critic import CriticObsAct
    from dppo.model.common.mlp_gaussian import Gaussian_MLP
    from dppo.model.rl.gaussian_ibrl import IBRL_Gaussian
    od, ta, da, dims, act, p, qdims, qact, E = A.net_of(case)
    actor = Gaussian_MLP(action_dim=da, horizon_steps=ta, cond_dim=od, mlp_dims=list(dims), activation_type=act, dropout=p,
                         fixed_std=A.FIXED_STD)
    q = CriticObsAct(cond_dim=od, mlp_dims=list(qdims), action_dim=da, action_steps=ta, activation_type=qact, use_layernorm=True,
                     double_q=False)
    m = IBRL_Gaussian(actor=actor, critic=q, n_critics=E, horizon_steps=ta, device="cpu", randn_clip_value=A.RANDN_CLIP)
    m.train()
    m.network.load_state_dict(A.actor_state_dict(case), strict=True)
    for e in range(E):
        m.critic_networks[e].load_state_dict(A.member_params(case, e), strict=True)
    m.ensemble_params, m.ensemble_buffers = torch.func.stack_module_state(m.critic_networks)
    return m, swap_dropout(m.network)


class catch_action:
    """Keeps the action ``loss_actor`` samples (what ``GaussianModel.forward`` returns to it) and has its gradient retained."""

    def __init__(self):
        self.a = None

    def __enter__(self):
        from dppo.model.common.gaussian import GaussianModel
        self.cls, self.real = GaussianModel, GaussianModel.forward

        def forward(model, *args, **kw):
            a = self.real(model, *args, **kw)
            a.retain_grad()
            self.a = a
            return a
        GaussianModel.forward = forward
        return self

    def __exit__(self, *a):
        self.cls.forward = self.real


def one_actor(out, case, n):
    A.check_conditions(case, n)
    b = A.inputs(case, n)
    m, mods = ref_model(case)
    set_masks(mods, b["mask"])
    cond = {"state": b["obs"]}
    with recorded_draws([b["noise"]]), catch_action() as ca:
        la = m.loss_actor(cond)
    la.backward()
    name = f"{case}_{n}"
    trunk = [(k, p) for k, p in m.network.named_parameters() if p.requires_grad and p.grad is not None]
    assert [k for k, _ in trunk] == list(A.actor_params(case)), [k for k, _ in trunk]
    for k, p in trunk:
        assert torch.isfinite(p.grad).all()
        put_grad(out, f"{name}_ga_{k}", p.grad)
    assert all(p.grad is None for net in m.critic_networks for p in net.parameters())
    put_grad(out, f"{name}_d_a", ca.a.grad.reshape(n, -1))
    # the selected member per row, in float64 from the reference's own modules at the reference's own action
    with torch.no_grad():
        a64 = ca.a.detach().double()
        q = torch.stack([net.double()({"state": b["obs"].double()}, a64).reshape(-1) for net in m.critic_networks])
    sel = A.argmin_lowest(q).numpy().astype(np.uint8)
    want = A.restate(case, n)
    assert np.array_equal(sel, want["sel"]), (name, np.flatnonzero(sel != want["sel"]))
    assert abs(la.item() - float(want["loss"])) <= 1e-5 * max(1.0, abs(la.item())), (la.item(), float(want["loss"]))
    out.update({f"{name}_a_loss": np.float64(la.item()), f"{name}_sel": sel})
    print(f"  {name}: actor loss {la.item():.6f}, wins per member {np.bincount(sel, minlength=q.shape[0]).tolist()}")


def update_sequence(out):
    case, n = A.SEQ_CASE, A.SEQ_N
    b = K.inputs(case, n)
    m, mods = ref_model(case)
    m.target_actor.load_state_dict(K.actor_state_dict(case, "target"), strict=True)
    m.bc_policy.load_state_dict(K.actor_state_dict(case, "bc"), strict=True)
    for e in range(len(m.target_networks)):
        m.target_networks[e].load_state_dict(K.member_params(case, e, K.TARGET_EPS), strict=True)
    tmods, bmods = swap_dropout(m.target_actor), swap_dropout(m.bc_policy)
    set_masks(mods, b["mask_rl"])
    set_masks(bmods, b["mask_bc"])
    set_masks(tmods, b["mask_rl"])
    opt_c = torch.optim.AdamW(m.ensemble_params.values(), lr=A.SEQ_LR, weight_decay=A.SEQ_WEIGHT_DECAY)
    opt_a = torch.optim.AdamW(m.network.parameters(), lr=A.SEQ_ACTOR_LR, weight_decay=A.SEQ_WEIGHT_DECAY)
    cond, ncond = {"state": b["obs"]}, {"state": b["next_obs"]}
    c_losses, grads = [], []
    for pair in A.SEQ_PAIRS:
        m.get_random_indices = lambda *a, pair=pair, **k: torch.tensor(pair)
        with recorded_draws([b["noise_bc"], b["noise_rl"]]):
            lc = m.loss_critic(cond, ncond, b["actions"], b["reward"], b["terminated"], K.GAMMA)
        opt_c.zero_grad()
        lc.backward()
        grads.append([p.grad.clone() for p in m.ensemble_params.values()])
        opt_c.step()
        m.update_target_critic(A.SEQ_TAU)
        c_losses.append(lc.item())
    with recorded_draws([b["noise_rl"]]):
        la = m.loss_actor(cond)
    opt_a.zero_grad()
    la.backward()
    opt_a.step()
    m.update_target_actor(A.SEQ_TAU)
    keys = list(m.ensemble_params)
    for i, gs in enumerate(grads):  # both critic updates' gradients, one flat vector per member: its row of the [E][P] image
        for e in range(len(m.critic_networks)):
            put_grad(out, f"seq_gq{i}_{e}", member_flat(gs, e))
    names = list(A.actor_params(case))
    for k in names:
        p = dict(m.network.named_parameters())[k]
        put_grad(out, f"seq_ga_{k}", p.grad)
        put_grad(out, f"seq_actor_{k}", p.detach())
        put_grad(out, f"seq_target_actor_{k}", dict(m.target_actor.named_parameters())[k].detach())
    for e in range(len(m.critic_networks)):
        put_grad(out, f"seq_q_{e}", member_flat([m.ensemble_params[k] for k in keys], e))
        put_grad(out, f"seq_target_{e}", torch.cat([p.detach().reshape(-1) for p in m.target_networks[e].parameters()]))
    out.update(seq_c_losses=np.array(c_losses), seq_a_loss=np.float64(la.item()), seq_member_keys=np.array(keys))
    print(f"  sequence: critic {c_losses}, actor {la.item():.6f}")


def main():
    check_mask_mul_is_dropout()
    out = {}
    for case, n in A.CASES:
        one_actor(out, case, n)
    A.check_conditions("wide", 3)
    update_sequence(out)
    save("g32_ibrl_actor", out)


if __name__ == "__main__":
    sys.path.insert(0, os.path.abspath(sys.argv[1]))
    main()
