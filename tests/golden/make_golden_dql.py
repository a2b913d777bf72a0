"""Generate the DQL fixture by running the REFERENCE's DQLDiffusion / CriticObsAct / DiffusionMLP on the CPU:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_dql.py <checkout of the reference (the directory holding dppo/)>

Writes tests/golden/g26_dql.npz.  Per case (make_golden_dql_cases.CASES): ``loss_actor`` with ``torch.randn`` / ``randn_like`` /
``randint`` and the coin replaced by the recipe's draws; the loss, the statistics {loss, bc, q_loss, mean q1, mean q2}, the chain
(in full for make_golden_dql_cases.FULL_CHAINS; otherwise flat[::61] of it and its norm: the file stays below g25's size), the clamp masks (bit-packed), the list of near-tie elements,
d loss / d action and every actor gradient (make_golden_bc.put_grad: flat[::61] + norm above 4096 entries).  One update sequence on
hopper, N = 77.  The state-dict keys and shapes of DQLDiffusion.  Weights and inputs are never stored.
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

from tests.golden import make_golden_dql_cases as K  # noqa: E402
from tests.golden import make_golden_qsm_cases as Q  # noqa: E402
from tests.golden.make_golden import recorded_noise  # noqa: E402
from tests.golden.make_golden_bc import put_grad, save  # noqa: E402

torch.set_num_threads(4)


def ref_model(case):
    from dppo.model.common.critic import CriticObsAct
    from dppo.model.diffusion.diffusion_dql import DQLDiffusion
    from dppo.model.diffusion.mlp_diffusion import DiffusionMLP
    net = K.net_of(case)
    od, ta, da, steps = K.shapes(case)
    a = Q.actor_spec(net)
    actor = DiffusionMLP(action_dim=da, horizon_steps=ta, cond_dim=od, time_dim=a.time_dim, mlp_dims=list(a.mlp_dims),
                         activation_type=a.activation, residual_style=True)
    actor.load_state_dict(Q.actor_params(net), strict=True)
    q = CriticObsAct(cond_dim=od, mlp_dims=[256, 256, 256], action_dim=da, action_steps=ta, activation_type="Mish",
                     residual_style=True)  # (swallowed, as shipped: plain trunks)
    q.load_state_dict(Q.twin_params(net), strict=True)
    m = DQLDiffusion(actor=actor, critic=q, horizon_steps=ta, obs_dim=od, action_dim=da, device="cpu", denoising_steps=steps,
                     **K.SAMPLING_KW, **K.model_kw(case))
    m.critic_target.load_state_dict(Q.twin_params(net, Q.TARGET_EPS), strict=True)
    return m


@contextmanager
def recorded_draws(m, b, coin, rec):
    """forward_train's K + 1 draws, the BC term's t and noise and the coin come from the recipe; ``loss_critic``'s ``forward``
    returns the recipe's next_actions.  rec collects every step's input, its x0 before the clamp, and the action (with its
    gradient kept)."""
    real_randint, real_uniform, real_pmv, real_ft, real_fwd = torch.randint, np.random.uniform, m.p_mean_var, m.forward_train, m.forward
    rec.update(chain=[], x0_raw=[])

    def pmv(x, t, cond, **kw):
        rec["chain"].append(x.detach().clone())
        with torch.no_grad():
            eps = m.network(x, t, cond=cond)
            s = (len(x), 1, 1)
            rec["x0_raw"].append(m.sqrt_recip_alphas_cumprod[t].reshape(s) * x - m.sqrt_recipm1_alphas_cumprod[t].reshape(s) * eps)
        return real_pmv(x, t, cond, **kw)

    def ft(cond, deterministic=False):
        x = real_ft(cond=cond, deterministic=deterministic)
        x.retain_grad()
        rec["a"] = x
        return x
    torch.randint = lambda *a, **k: b["t_bc"].clone()
    np.random.uniform = lambda *a, **k: coin
    m.p_mean_var, m.forward_train = pmv, ft
    m.forward = lambda cond, deterministic=False: b["next_actions"].clone()
    try:
        with recorded_noise(list(b["noise"]) + [b["noise_bc"]]):
            yield
    finally:
        torch.randint, np.random.uniform = real_randint, real_uniform
        m.p_mean_var, m.forward_train, m.forward = real_pmv, real_ft, real_fwd


def put_grads(out, key, module):
    for k, p in module.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), (key, k)
        put_grad(out, f"{key}_{k}", p.grad.clone())  # (a copy: small tensors are stored as they are, and later backwards add to .grad)


def run_actor(m, case, b, rec):
    coin = 0.75 if K.which(case) == 0 else 0.25  # `> 0.5` picks -mean(q1) / mean|q2|
    with recorded_draws(m, b, coin, rec):
        la = m.loss_actor({"state": b["obs"]}, K.ETA, K.shapes(case)[1])
    la.backward()
    return la


def actor_case(out, case, n):
    name, b, m, rec = f"{case}_{n}", K.inputs(case, n), ref_model(case), {}
    od, ta, da, steps = K.shapes(case)
    la = run_actor(m, case, b, rec)
    a = rec["a"]
    with torch.no_grad():
        q1, q2 = m.critic({"state": b["obs"]}, a)
        bc_in = m.q_sample(a, b["t_bc"], b["noise_bc"])
        bc = torch.nn.functional.mse_loss(m.network(bc_in, b["t_bc"], cond={"state": b["obs"]}), b["noise_bc"])
    qa, qb = (q1, q2) if K.which(case) == 0 else (q2, q1)
    ql = -qa.mean() / qb.abs().mean()
    assert abs((bc + K.ETA * ql).item() - la.item()) <= 1e-6 * max(1.0, abs(la.item())), name
    chain = torch.stack(rec["chain"] + [a.detach()], 1).reshape(n, steps + 1, -1).numpy()
    x0 = torch.stack(rec["x0_raw"], 1).reshape(n, steps, -1).numpy()
    clip = K.model_kw(case)["denoised_clip_value"]
    masks = np.ones(x0.shape, dtype=bool) if clip is None else np.abs(x0) <= clip
    ties = K.near_ties(x0, steps, clip)
    assert ties.size <= K.NEAR_TIE_CAP * x0.size, (name, ties.size, x0.size)
    out[f"{name}_loss"] = np.float64(la.item())
    out[f"{name}_stats"] = np.array([la.item(), bc.item(), ql.item(), q1.double().mean().item(), q2.double().mean().item()])
    out[f"{name}_masks"] = np.packbits(masks.reshape(-1))
    out[f"{name}_ties"] = ties.astype(np.int32)
    if (case, n) in K.FULL_CHAINS:
        out[f"{name}_chain"] = chain.copy()
    else:  # (the file-size limit: the restatement rebuilds these chains, and is pinned to the entries stored here)
        put_grad(out, f"{name}_chain", torch.from_numpy(chain))
    put_grad(out, f"{name}_d_a", a.grad.reshape(n, -1))
    put_grads(out, f"{name}_ga", m.actor)
    print(f"  {name}: loss {la.item():.5f} bc {bc.item():.5f} q_loss {ql.item():.5f} clamped {1 - masks.mean():.3f} "
          f"near ties {ties.size} of {x0.size}")


def update_sequence(out, n=77):
    """The reference agent's minibatch (:232-260): critic loss, AdamW step; actor loss WITH THE UPDATED critic, AdamW step; Polyak."""
    b, m, rec = K.critic_batch(n), ref_model("hopper"), {}
    opt_c = torch.optim.AdamW(m.critic.parameters(), lr=K.SEQ_LR, weight_decay=0)
    opt_a = torch.optim.AdamW(m.actor.parameters(), lr=K.SEQ_ACTOR_LR, weight_decay=0)
    with recorded_draws(m, b, 0.75, rec):
        lc = m.loss_critic({"state": b["obs"]}, {"state": b["next_obs"]}, b["actions"], b["reward"], b["terminated"], K.GAMMA)
    opt_c.zero_grad()
    lc.backward()
    opt_c.step()
    put_grads(out, "seq_gq", m.critic)
    opt_a.zero_grad()
    la = run_actor(m, "hopper", b, rec)
    opt_a.step()
    put_grads(out, "seq_ga", m.actor)
    m.update_target_critic(K.SEQ_TAU)
    out.update(seq_c_loss=np.float64(lc.item()), seq_a_loss=np.float64(la.item()))
    for key, mod in (("seq_q", m.critic), ("seq_actor", m.actor), ("seq_target", m.critic_target)):
        for k, p in mod.named_parameters():
            put_grad(out, f"{key}_{k}", p.detach().clone())
    print(f"  seq: critic loss {lc.item():.5f} actor loss (updated critic) {la.item():.5f}")


def main():
    out = {}
    for case, n in K.CASES:
        actor_case(out, case, n)
    update_sequence(out)
    sd = ref_model("hopper").state_dict()
    out["state_dict_keys"] = np.array(list(sd))
    out["state_dict_shapes"] = np.array([",".join(str(int(x)) for x in v.shape) for v in sd.values()])
    save("g26_dql", out)


if __name__ == "__main__":
    sys.path.insert(0, os.path.abspath(sys.argv[1]))
    main()
