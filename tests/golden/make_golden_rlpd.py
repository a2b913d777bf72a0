"""Generate the RLPD fixture by running the REFERENCE's RLPD_Gaussian / Gaussian_MLP / CriticObsAct on the CPU:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_rlpd.py <checkout of the reference (the directory holding dppo/)>

Writes tests/golden/g28_rlpd.npz.  Per case (make_golden_rlpd_cases.CASES): ``loss_actor`` with ``rsample``'s draw replaced by the
recipe's (the loss, d mean(-q_mean) / d a, every actor gradient) and ``loss_critic`` with ``get_random_indices`` handing back
``pair_of`` and ``forward`` handing back the recipe's next actions and log-probabilities (the loss, every member's gradients as ONE
flat vector per member, in state-dict order: its row of the [E][P] image).  The state-dict keys.  One update sequence on cheetah,
N = 77: two critic AdamW steps with Polyak (the first one's gradients are cheetah_77's own, not stored twice), one actor step, one
temperature step; the stepped members and targets as flat vectors too.  Large tensors as flat[::61] + norm (make_golden_bc.put_grad).  Weights and inputs are never stored: both sides rebuild them from
make_golden_rlpd_cases.py / make_golden_sac_cases.py.

The reference stacks ``ensemble_params`` at construction and optimises THOSE: after the members are loaded they are stacked again
here, and the sequence steps ``ensemble_params``; ``critic_networks.*`` would record the initial weights.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.dont_write_bytecode = True

from tests.golden import make_golden_rlpd_actor_cases as A  # noqa: E402
from tests.golden import make_golden_rlpd_cases as K  # noqa: E402
from tests.golden import make_golden_sac_cases as S  # noqa: E402
from tests.golden.make_golden_bc import put_grad, save  # noqa: E402
from tests.golden.make_golden_sac import put_grads, recorded_draws  # noqa: E402

torch.set_num_threads(4)


def ref_model(case, backup=True):
    from dppo.model.common.critic import CriticObsAct
    from dppo.model.common.mlp_gaussian import Gaussian_MLP
    from dppo.model.rl.gaussian_rlpd import RLPD_Gaussian
    od, ta, da, dims, act, E = K.RLPD_NETS[case]
    base = A.sac_case(case)
    actor = Gaussian_MLP(action_dim=da, horizon_steps=ta, cond_dim=od, mlp_dims=S.dims(base), activation_type=S.activation(base),
                         tanh_output=False, std_min=S.STD_MIN, std_max=S.STD_MAX)
    actor.load_state_dict(A.actor_params(case), strict=True)
    q = CriticObsAct(cond_dim=od, mlp_dims=list(dims), action_dim=da, action_steps=ta, activation_type=act, use_layernorm=True,
                     double_q=False)
    m = RLPD_Gaussian(actor=actor, critic=q, n_critics=E, backup_entropy=backup, horizon_steps=ta, device="cpu",
                      randn_clip_value=S.RANDN_CLIP, tanh_output=True)
    for e in range(E):
        m.critic_networks[e].load_state_dict(K.member_params(case, e), strict=True)
        m.target_networks[e].load_state_dict(K.member_params(case, e, K.TARGET_EPS), strict=True)
    m.ensemble_params, m.ensemble_buffers = torch.func.stack_module_state(m.critic_networks)  # (see the module docstring)
    return m


def given_critic_inputs(m, case, n):
    """``loss_critic`` then takes the pair, the sample at next_obs and its log-probability from the recipe."""
    b = K.inputs(case, n)
    m.get_random_indices = lambda *a, **k: torch.tensor(K.pair_of(case, n))
    m.forward = lambda *a, **k: (b["next_actions"], b["next_logp"])


def ensemble_q(m, cond, a):
    return torch.vmap(m.critic_wrapper, in_dims=(0, 0, None))(m.ensemble_params, m.ensemble_buffers, (cond, a))


def member_flat(tensors, e):
    """Member e's slices of the stacked tensors back to back, in state-dict order: its row of the flat [E][P] image."""
    return torch.cat([t[e].detach().reshape(-1) for t in tensors])


def put_member_grads(out, key, m):
    """One flat [P] vector per member (a fixture of per-tensor entries for E members and ten cases outgrows a committed file)."""
    grads = [p.grad for p in m.ensemble_params.values()]
    assert all(g is not None and torch.isfinite(g).all() for g in grads), key
    for e in range(m.n_critics):
        put_grad(out, f"{key}_{e}", member_flat(grads, e))


def zero_member_grads(m):
    for p in m.ensemble_params.values():
        p.grad = None


def one_case(out, case, n):
    name, b, ab = f"{case}_{n}", K.inputs(case, n), A.inputs(case, n)
    m = ref_model(case, K.backup_entropy(case, n))
    cond = {"state": b["obs"]}
    # actor
    with recorded_draws([ab["noise"]]):
        la = m.loss_actor(cond, K.ALPHA)
    la.backward()
    put_grads(out, f"{name}_ga", m.network)
    zero_member_grads(m)
    with recorded_draws([ab["noise"]]):
        a2, _ = m(cond, deterministic=False, reparameterize=True, get_logprob=True)
    ad = a2.detach().clone().requires_grad_(True)
    (-ensemble_q(m, cond, ad).mean(dim=0)).mean().backward()
    out[f"{name}_a_loss"] = np.float64(la.item())
    put_grad(out, f"{name}_d_a", ad.grad.reshape(n, -1))
    zero_member_grads(m)
    # critic
    given_critic_inputs(m, case, n)
    lc = m.loss_critic(cond, {"state": b["next_obs"]}, b["actions"], b["reward"], b["terminated"], K.GAMMA, K.ALPHA)
    lc.backward()
    out[f"{name}_c_loss"] = np.float64(lc.item())
    put_member_grads(out, f"{name}_gq", m)
    print(f"  {name}: actor {la.item():.6f} critic {lc.item():.6f}")


def update_sequence(out, case=A.SEQ_CASE, n=A.SEQ_N):
    """The reference agent's update (train_rlpd_agent.py:246-347) with its optimisers, on one batch."""
    b, sb = K.inputs(case, n), S.inputs(A.sac_case(case), n)
    m = ref_model(case, K.backup_entropy(case, n))
    real_forward = m.forward
    cond, ncond = {"state": b["obs"]}, {"state": b["next_obs"]}
    opt_a = torch.optim.AdamW(m.network.parameters(), lr=A.SEQ_ACTOR_LR, weight_decay=A.SEQ_WEIGHT_DECAY)
    opt_c = torch.optim.AdamW(m.ensemble_params.values(), lr=A.SEQ_LR, weight_decay=A.SEQ_WEIGHT_DECAY)
    log_alpha = torch.tensor(A.SEQ_LOG_ALPHA, dtype=torch.float64, requires_grad=True)
    opt_t = torch.optim.Adam([log_alpha], lr=A.SEQ_LR)
    c_loss = []
    given_critic_inputs(m, case, n)
    for i in range(A.SEQ_CRITIC_UPDATES):
        alpha = log_alpha.exp().item()
        lc = m.loss_critic(cond, ncond, b["actions"], b["reward"], b["terminated"], K.GAMMA, alpha)
        opt_c.zero_grad()
        lc.backward()
        opt_c.step()
        if i == 0:  # the first update is cheetah_77's loss_critic: same batch, pair and alpha
            assert lc.item() == float(out[f"{case}_{n}_c_loss"])
        else:
            put_member_grads(out, f"seq_gq{i}", m)
        m.update_target_critic(A.SEQ_TAU)
        c_loss.append(lc.item())
    del m.forward  # the instance's stand-in: the class's own again
    assert m.forward.__func__ is type(m).forward and real_forward.__func__ is type(m).forward
    with recorded_draws([sb["noise"]]):
        la = m.loss_actor(cond, alpha)
    opt_a.zero_grad()
    la.backward()
    opt_a.step()
    put_grads(out, "seq_ga", m.network)
    opt_t.zero_grad()
    with recorded_draws([sb["noise_t"]]):
        lt = m.loss_temperature(cond, log_alpha.exp(), S.target_entropy(A.sac_case(case)))
    lt.backward()
    opt_t.step()
    out.update(seq_c_loss=np.array(c_loss), seq_a_loss=np.float64(la.item()), seq_t_loss=np.float64(lt.item()),
               seq_log_alpha=np.float64(log_alpha.item()))
    for e, t in enumerate(m.target_networks):
        put_grad(out, f"seq_q_{e}", member_flat(list(m.ensemble_params.values()), e))
        put_grad(out, f"seq_target_{e}", torch.cat([p.detach().reshape(-1) for p in t.parameters()]))
    for k, p in m.network.named_parameters():
        if p.requires_grad:
            put_grad(out, f"seq_actor_{k}", p)
    print(f"  seq: critic {c_loss} actor {la.item():.6f} temperature {lt.item():.6f} log_alpha {log_alpha.item():.8f}")


def main():
    out = {}
    for case, n in K.CASES:
        one_case(out, case, n)
    update_sequence(out)
    sd = ref_model("tiny").state_dict()
    out["state_dict_keys"] = np.array(list(sd))
    save("g28_rlpd", out)


if __name__ == "__main__":
    sys.path.insert(0, os.path.abspath(sys.argv[1]))
    main()
