"""Generate the QSM fixture by running the REFERENCE's QSMDiffusion / CriticObsAct / DiffusionMLP on the CPU:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_qsm.py <checkout of the reference (the directory holding dppo/)>

Writes tests/golden/g25_qsm.npz.  Per critic case (make_golden_qsm_cases.CRITIC_CASES): the reference's ``loss_critic`` with
``forward`` replaced by the recipe's next_actions, its statistics (mean q1, mean y) and every Q gradient.  Per actor case
(ACTOR_CASES): ``loss_actor`` with its two draws replaced by the recipe's noise and t, the mean action gradient g it forms on the
way (in full for N = 77; for N = 1000 flat[::61] + norm, like every large tensor here: make_golden_bc.put_grad) and every
actor gradient.  One update sequence on hopper, N = 77 (critic AdamW step, actor loss with the updated critic, actor step,
Polyak).  The state-dict keys and shapes of QSMDiffusion.  Weights and inputs are never stored: both sides rebuild them from
make_golden_qsm_cases.py.
"""
import os
import sys
from contextlib import contextmanager

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.dont_write_bytecode = True

from tests.golden import make_golden_qsm_cases as K  # noqa: E402
from tests.golden.make_golden import recorded_noise  # noqa: E402
from tests.golden.make_golden_bc import put_grad, save  # noqa: E402

torch.set_num_threads(4)


def ref_model(net):
    from dppo.model.common.critic import CriticObsAct
    from dppo.model.diffusion.diffusion_qsm import QSMDiffusion
    from dppo.model.diffusion.mlp_diffusion import DiffusionMLP
    od, ta, da, steps = K.shapes(net)
    a = K.actor_spec(net)
    actor = DiffusionMLP(action_dim=da, horizon_steps=ta, cond_dim=od, time_dim=a.time_dim, mlp_dims=list(a.mlp_dims),
                         activation_type=a.activation, residual_style=True)
    actor.load_state_dict(K.actor_params(net), strict=True)
    q = CriticObsAct(cond_dim=od, mlp_dims=[256, 256, 256], action_dim=da, action_steps=ta, activation_type="Mish",
                     residual_tyle=K.QSM_NETS[net][4], residual_style=True)  # (the last one is swallowed, as shipped)
    q.load_state_dict(K.twin_params(net), strict=True)
    m = QSMDiffusion(actor=actor, critic=q, horizon_steps=ta, obs_dim=od, action_dim=da, device="cpu", denoising_steps=steps,
                     **K.SAMPLING_KW)
    m.target_q.load_state_dict(K.twin_params(net, K.TARGET_EPS), strict=True)
    return m


@contextmanager
def recorded_draws(m, b):
    """``loss_actor``'s two draws (torch.randn_like, torch.randint) and ``loss_critic``'s ``forward`` return the recipe's tensors;
    the gradient the actor loss forms is kept in ``m.recorded_g``."""
    real_randint, real_grad, real_forward = torch.randint, torch.autograd.grad, m.forward
    grads = []

    def grad(*a, **k):
        out = real_grad(*a, **k)
        grads.append(out[0].detach().clone())
        return out
    torch.randint = lambda *a, **k: b["t"].clone()
    torch.autograd.grad = grad
    m.forward = lambda cond, deterministic=False: b["next_actions"].clone()
    try:
        with recorded_noise([b["noise"]]):
            yield
    finally:
        torch.randint, torch.autograd.grad = real_randint, real_grad
        m.forward = real_forward
        m.recorded_g = torch.stack(grads[-2:], 0).mean(0) if len(grads) >= 2 else None


def put_grads(out, key, module):
    for k, p in module.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), (key, k)
        put_grad(out, f"{key}_{k}", p.grad)


def critic_stats(m, b):
    with torch.no_grad():
        q1, _ = m.critic_q({"state": b["obs"]}, b["actions"])
        nq = torch.min(*m.target_q({"state": b["next_obs"]}, b["next_actions"]))
        y = b["reward"] + K.GAMMA * nq.view(-1) * (1 - b["terminated"])
    return np.float64(q1.double().mean().item()), np.float64(y.double().mean().item())


def critic_case(out, net, n):
    name, b, m = f"{net}_{n}", K.inputs(net, n), ref_model(net)
    with recorded_draws(m, b):
        lc = m.loss_critic({"state": b["obs"]}, {"state": b["next_obs"]}, b["actions"], b["reward"], b["terminated"], K.GAMMA)
    lc.backward()
    q1m, ym = critic_stats(m, b)
    out.update({f"{name}_c_loss": np.float64(lc.item()), f"{name}_q1_mean": q1m, f"{name}_y_mean": ym})
    put_grads(out, f"{name}_gq", m.critic_q)
    print(f"  {name}: critic loss {lc.item():.5f} mean q1 {q1m:.4f} mean y {ym:.4f}")


def actor_case(out, net, n):
    name, b, m = f"{net}_{n}", K.inputs(net, n), ref_model(net)
    with recorded_draws(m, b):
        la = m.loss_actor({"state": b["obs"]}, b["actions"], K.coeff(net))
    la.backward()
    g = m.recorded_g
    assert g.shape == b["actions"].shape and torch.isfinite(g).all()
    out[f"{name}_a_loss"] = np.float64(la.item())
    if n == 77:  # in full: g is per row, and the small case is where a tail-row or column-range error would show
        out[f"{name}_g"] = g.reshape(n, -1).numpy().copy()
    else:
        put_grad(out, f"{name}_g", g.reshape(n, -1))
    put_grads(out, f"{name}_ga", m.actor)
    print(f"  {name}: actor loss {la.item():.5f} |g| rms {g.pow(2).mean().sqrt():.4f} max {g.abs().max():.4f}")


def update_sequence(out, net="hopper", n=77):
    """The reference agent's minibatch (:246-275): critic loss, AdamW step; actor loss WITH THE UPDATED critic, AdamW step; Polyak."""
    b, m = K.inputs(net, n), ref_model(net)
    opt_c = torch.optim.AdamW(m.critic_q.parameters(), lr=K.SEQ_LR, weight_decay=0)
    opt_a = torch.optim.AdamW(m.actor.parameters(), lr=K.SEQ_ACTOR_LR, weight_decay=0)
    with recorded_draws(m, b):
        lc = m.loss_critic({"state": b["obs"]}, {"state": b["next_obs"]}, b["actions"], b["reward"], b["terminated"], K.GAMMA)
    opt_c.zero_grad()
    lc.backward()
    opt_c.step()
    put_grads(out, "seq_gq", m.critic_q)
    with recorded_draws(m, b):
        la = m.loss_actor({"state": b["obs"]}, b["actions"], K.coeff(net))
    opt_a.zero_grad()
    la.backward()
    opt_a.step()
    put_grads(out, "seq_ga", m.actor)
    m.update_target_critic(K.SEQ_TAU)
    out.update(seq_c_loss=np.float64(lc.item()), seq_a_loss=np.float64(la.item()))
    for key, mod in (("seq_q", m.critic_q), ("seq_actor", m.actor), ("seq_target", m.target_q)):
        for k, p in mod.named_parameters():  # the stepped weights, stored like the gradients (same entries of each tensor)
            put_grad(out, f"{key}_{k}", p)
    print(f"  seq: critic loss {lc.item():.5f} actor loss (updated critic) {la.item():.5f}")


def main():
    out = {}
    for net, n in K.CRITIC_CASES:
        critic_case(out, net, n)
    for net, n in K.ACTOR_CASES:
        actor_case(out, net, n)
    update_sequence(out)
    sd = ref_model("hopper").state_dict()
    out["state_dict_keys"] = np.array(list(sd))
    out["state_dict_shapes"] = np.array([",".join(str(int(x)) for x in v.shape) for v in sd.values()])
    save("g25_qsm", out)


if __name__ == "__main__":
    sys.path.insert(0, os.path.abspath(sys.argv[1]))
    main()
