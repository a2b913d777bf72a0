"""Generate the fixture of Cal-QL's actor loss by running the REFERENCE's CalQL_Gaussian / Gaussian_MLP / CriticObsAct on the CPU:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_calql_actor.py <checkout of the reference (the directory holding dppo/)>

Writes tests/golden/g30_calql_actor.npz.  Per case (make_golden_calql_actor_cases.CASES), with ``Normal.rsample``'s draw replaced
by the recipe's: ``loss_actor``, d mean(-min(q1, q2)) / d a and every actor gradient (large ones as flat[::61] + norm,
make_golden_bc.put_grad).  Then one update on K's ``tiny`` at N = 77 in the agent's order with the reference's optimisers: critic
loss and AdamW step, Polyak, actor loss and AdamW step, temperature loss and Adam step -- both losses, every critic and actor
gradient, the stepped critic, target and actor, and ``log_alpha``.  Weights and inputs are never stored: both sides rebuild them from
make_golden_calql_cases.py and make_golden_calql_actor_cases.py.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.dont_write_bytecode = True

from tests.golden import make_golden_calql_actor_cases as A  # noqa: E402
from tests.golden.make_golden_bc import put_grad, save  # noqa: E402
from tests.golden.make_golden_sac import put_grads, recorded_draws  # noqa: E402

K, S = A.K, A.S
torch.set_num_threads(4)


def ref_model(case, twin, actor_p, clips=(-np.inf, np.inf), n_next=10):
    from dppo.model.common.critic import CriticObsAct
    from dppo.model.common.mlp_gaussian import Gaussian_MLP
    from dppo.model.rl.gaussian_calql import CalQL_Gaussian
    od, ta, da, dims, act = A.net_of(case)
    actor = Gaussian_MLP(action_dim=da, horizon_steps=ta, cond_dim=od, mlp_dims=A.actor_dims(case), activation_type=act,
                         tanh_output=False, std_min=S.STD_MIN, std_max=S.STD_MAX)
    actor.load_state_dict(actor_p, strict=True)
    q = CriticObsAct(cond_dim=od, mlp_dims=list(dims), action_dim=da, action_steps=ta, activation_type=act, use_layernorm=True,
                     double_q=True)
    q.load_state_dict(twin, strict=True)
    return CalQL_Gaussian(actor=actor, critic=q, cql_clip_diff_min=clips[0], cql_clip_diff_max=clips[1],
                          cql_min_q_weight=K.MIN_Q_WEIGHT, cql_n_actions=n_next, horizon_steps=ta, device="cpu",
                          randn_clip_value=A.RANDN_CLIP, tanh_output=True)


def one_case(out, case):
    b, n = A.inputs(case), A.parts(case)[1]
    m = ref_model(case, A.twin_params(case), A.actor_params(case))
    cond = {"state": b["obs"]}
    with recorded_draws([b["noise"]]):
        la = m.loss_actor(cond, A.ALPHA)
    la.backward()
    put_grads(out, f"{case}_ga", m.network)
    with recorded_draws([b["noise"]]):
        a2, _ = m(cond, deterministic=False, reparameterize=True, get_logprob=True)
    ad = a2.detach().clone().requires_grad_(True)
    (-torch.min(*m.critic(cond, ad))).mean().backward()
    out[f"{case}_a_loss"] = np.float64(la.item())
    put_grad(out, f"{case}_d_a", ad.grad.reshape(n, -1))
    print(f"  {case}: actor {la.item():.6f}")


def update_sequence(out, case=A.SEQ_CASE, n=A.SEQ_N):
    """The reference agent's update (train_calql_agent.py:408-445) with its optimisers, on one batch."""
    b = K.inputs(case, n)
    R, Sn = K.n_samples(case)
    name = f"{case}_{n}"
    m = ref_model(name, K.twin_params(case), K.actor_params(case), K.clips_of(case, n), Sn)
    m.target_critic.load_state_dict(K.twin_params(case, K.TARGET_EPS), strict=True)
    cond, ncond = {"state": b["obs"]}, {"state": b["next_obs"]}
    opt_a = torch.optim.AdamW(m.network.parameters(), lr=A.SEQ_ACTOR_LR, weight_decay=A.SEQ_WEIGHT_DECAY)
    opt_c = torch.optim.AdamW(m.critic.parameters(), lr=A.SEQ_LR, weight_decay=A.SEQ_WEIGHT_DECAY)
    log_alpha = torch.tensor(A.SEQ_LOG_ALPHA, dtype=torch.float64, requires_grad=True)
    opt_t = torch.optim.Adam([log_alpha], lr=A.SEQ_LR)
    z = b["noise"]
    alpha = log_alpha.exp().item()
    with recorded_draws([z[:n * Sn], z[n * Sn:n * Sn + n], z[n * Sn + n:]]):
        lc = m.loss_critic(cond, ncond, b["actions"], b["random_actions"], b["reward"], K.returns_of(case, n), b["terminated"], K.GAMMA)
    opt_c.zero_grad()
    lc.backward()
    opt_c.step()
    put_grads(out, "seq_gq", m.critic)
    m.update_target_critic(A.SEQ_TAU)
    with recorded_draws([z[n * Sn:n * Sn + n]]):
        la = m.loss_actor(cond, alpha)
    opt_a.zero_grad()
    la.backward()
    opt_a.step()
    put_grads(out, "seq_ga", m.network)
    opt_t.zero_grad()
    with recorded_draws([A.temperature_noise(case, n)]):
        lt = m.loss_temperature(cond, log_alpha.exp(), -float(np.prod(K.shapes(case)[1:])))
    lt.backward()
    opt_t.step()
    out.update(seq_c_loss=np.float64(lc.item()), seq_a_loss=np.float64(la.item()), seq_t_loss=np.float64(lt.item()),
               seq_log_alpha=np.float64(log_alpha.item()))
    for key, mod in (("seq_q", m.critic), ("seq_target", m.target_critic), ("seq_actor", m.network)):
        for k, p in mod.named_parameters():
            if p.requires_grad or key != "seq_actor":
                put_grad(out, f"{key}_{k}", p)
    print(f"  seq: critic {lc.item():.6f} actor {la.item():.6f} temperature {lt.item():.6f} log_alpha {log_alpha.item():.8f}")


def main():
    out = {}
    for case in A.CASES:
        one_case(out, case)
    update_sequence(out)
    save("g30_calql_actor", out)


if __name__ == "__main__":
    sys.path.insert(0, os.path.abspath(sys.argv[1]))
    main()
