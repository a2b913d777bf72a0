"""Generate the SAC fixture by running the REFERENCE's SAC_Gaussian / Gaussian_MLP / CriticObsAct on the CPU:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_sac.py <checkout of the reference (the directory holding dppo/)>

Writes tests/golden/g27_sac.npz.  Per case (make_golden_sac_cases.CASES), with every draw of ``Normal.sample`` / ``rsample``
replaced by the recipe's: the sample and its log-probability (stochastic and deterministic), ``loss_critic`` with its statistics
and every Q gradient, ``loss_actor`` with its statistics, ``sel`` (1 where Q2 is the smaller), d mean(-q_sel) / d a and every
actor gradient, ``loss_temperature`` and its derivative by log_alpha.  One update sequence on cheetah, N = 77 (critic Adam step,
Polyak, two actor + temperature steps).  The state-dict keys and shapes of SAC_Gaussian.  Large tensors as flat[::61] + norm
(make_golden_bc.put_grad).  Weights and inputs are never stored: both sides rebuild them from make_golden_sac_cases.py.
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

from tests.golden import make_golden_sac_cases as K  # noqa: E402
from tests.golden.make_golden_bc import put_grad, save  # noqa: E402

torch.set_num_threads(4)


def ref_model(case):
    from dppo.model.common.critic import CriticObsAct
    from dppo.model.common.mlp_gaussian import Gaussian_MLP
    from dppo.model.rl.gaussian_sac import SAC_Gaussian
    od, ta, da = K.shapes(case)
    actor = Gaussian_MLP(action_dim=da, horizon_steps=ta, cond_dim=od, mlp_dims=K.dims(case), activation_type=K.activation(case),
                         tanh_output=False, std_min=K.STD_MIN, std_max=K.STD_MAX)
    actor.load_state_dict(K.actor_params(case), strict=True)
    q = CriticObsAct(cond_dim=od, mlp_dims=K.dims(case), action_dim=da, action_steps=ta, activation_type=K.activation(case))
    q.load_state_dict(K.twin_params(case), strict=True)
    m = SAC_Gaussian(actor=actor, critic=q, horizon_steps=ta, device="cpu", randn_clip_value=K.RANDN_CLIP, tanh_output=True)
    m.target_critic.load_state_dict(K.twin_params(case, K.TARGET_EPS), strict=True)
    return m


@contextmanager
def recorded_draws(noises):
    """``Normal.sample`` / ``rsample`` return loc + the next recorded draw * scale (their own arithmetic: distributions/normal.py)."""
    it = iter(noises)
    N = torch.distributions.Normal
    real_s, real_r = N.sample, N.rsample

    def rsample(self, sample_shape=torch.Size()):
        return self.loc + next(it).reshape(self.loc.shape) * self.scale

    def sample(self, sample_shape=torch.Size()):
        with torch.no_grad():
            return rsample(self)
    N.sample, N.rsample = sample, rsample
    try:
        yield
    finally:
        N.sample, N.rsample = real_s, real_r


def put_grads(out, key, module):
    for k, p in module.named_parameters():
        if not p.requires_grad:
            continue
        assert p.grad is not None and torch.isfinite(p.grad).all(), (key, k)
        put_grad(out, f"{key}_{k}", p.grad.clone())


def one_case(out, case, n):
    name, b, m = f"{case}_{n}", K.inputs(case, n), ref_model(case)
    cond, ncond = {"state": b["obs"]}, {"state": b["next_obs"]}
    with recorded_draws([b["noise"], b["noise"]]):
        a, logp = m(cond, deterministic=False, get_logprob=True)
        a_det, logp_det = m(cond, deterministic=True, get_logprob=True)
    out.update({f"{name}_a": a.reshape(n, -1).detach().numpy().copy(), f"{name}_logp": logp.detach().numpy().copy(),
                f"{name}_a_det": a_det.reshape(n, -1).detach().numpy().copy(), f"{name}_logp_det": logp_det.detach().numpy().copy()})
    # critic
    with recorded_draws([b["noise_next"]]):
        lc = m.loss_critic(cond, ncond, b["actions"], b["reward"], b["terminated"], K.GAMMA, K.ALPHA)
    lc.backward()
    with torch.no_grad(), recorded_draws([b["noise_next"]]):
        na, nlp = m(ncond, deterministic=False, get_logprob=True)
        nq = torch.min(*m.target_critic(ncond, na)) - K.ALPHA * nlp
        y = b["reward"] + K.GAMMA * nq * (1 - b["terminated"])
        q1, _ = m.critic(cond, b["actions"])
    out[f"{name}_c_stats"] = np.array([lc.item(), q1.double().mean().item(), y.double().mean().item()])
    put_grads(out, f"{name}_gq", m.critic)
    m.critic.zero_grad()
    # actor
    with recorded_draws([b["noise"]]):
        la = m.loss_actor(cond, K.ALPHA)
    la.backward()
    with recorded_draws([b["noise"]]):
        a2, lp2 = m(cond, deterministic=False, reparameterize=True, get_logprob=True)
    ad = a2.detach().clone().requires_grad_(True)
    q1, q2 = m.critic(cond, ad)
    qs = torch.min(q1, q2)
    (-qs).mean().backward()
    with torch.no_grad():
        _, scale = m.network(cond)
    out[f"{name}_a_stats"] = np.array([la.item(), qs.detach().double().mean().item(), lp2.detach().double().mean().item(),
                                       scale.double().mean().item()])
    out[f"{name}_sel"] = (q2 < q1).detach().numpy().astype(np.uint8)
    out[f"{name}_qgap"] = (q1 - q2).detach().numpy().copy()
    put_grad(out, f"{name}_d_a", ad.grad.reshape(n, -1))
    put_grads(out, f"{name}_ga", m.network)
    # temperature
    la_t = torch.tensor(K.SEQ_LOG_ALPHA, dtype=torch.float64, requires_grad=True)
    with recorded_draws([b["noise_t"]]):
        lt = m.loss_temperature(cond, la_t.exp(), K.target_entropy(case))
    lt.backward()
    out[f"{name}_t"] = np.array([lt.item(), la_t.grad.item()])
    print(f"  {name}: critic {lc.item():.5f} actor {la.item():.5f} temperature {lt.item():.5f} sel share {out[f'{name}_sel'].mean():.2f}")


def update_sequence(out, case="cheetah", n=77):
    """The reference agent's update (:242-280) with its optimisers: critic step, Polyak, two actor + temperature steps."""
    b, m = K.inputs(case, n), ref_model(case)
    cond, ncond = {"state": b["obs"]}, {"state": b["next_obs"]}
    opt_a = torch.optim.Adam(m.network.parameters(), lr=K.SEQ_ACTOR_LR)
    opt_c = torch.optim.Adam(m.critic.parameters(), lr=K.SEQ_LR)
    log_alpha = torch.tensor(K.SEQ_LOG_ALPHA, dtype=torch.float64, requires_grad=True)
    opt_t = torch.optim.Adam([log_alpha], lr=K.SEQ_LR)
    alpha = log_alpha.exp().item()
    with recorded_draws([b["noise_next"]]):
        lc = m.loss_critic(cond, ncond, b["actions"], b["reward"], b["terminated"], K.GAMMA, alpha)
    opt_c.zero_grad()
    lc.backward()
    opt_c.step()
    put_grads(out, "seq_gq", m.critic)
    m.update_target_critic(K.SEQ_TAU)
    a_loss, t_loss, las = [], [], []
    for i, (nk, tk) in enumerate((("noise", "noise_t"), ("noise2", "noise_t2"))):
        with recorded_draws([b[nk]]):
            la = m.loss_actor(cond, alpha)
        opt_a.zero_grad()
        la.backward()
        opt_a.step()
        put_grads(out, f"seq_ga{i}", m.network)
        opt_t.zero_grad()
        with recorded_draws([b[tk]]):
            lt = m.loss_temperature(cond, log_alpha.exp(), K.target_entropy(case))
        lt.backward()
        opt_t.step()
        a_loss.append(la.item()), t_loss.append(lt.item()), las.append(log_alpha.item())
    out.update(seq_c_loss=np.float64(lc.item()), seq_a_loss=np.array(a_loss), seq_t_loss=np.array(t_loss), seq_log_alpha=np.array(las))
    for key, mod in (("seq_q", m.critic), ("seq_actor", m.network), ("seq_target", m.target_critic)):
        for k, p in mod.named_parameters():
            if p.requires_grad:
                put_grad(out, f"{key}_{k}", p)
    print(f"  seq: critic {lc.item():.5f} actor {a_loss} temperature {t_loss} log_alpha {las}")


def main():
    out = {}
    for case, n in K.CASES:
        one_case(out, case, n)
    update_sequence(out)
    sd = ref_model("cheetah").state_dict()
    out["state_dict_keys"] = np.array(list(sd))
    out["state_dict_shapes"] = np.array([",".join(str(int(x)) for x in v.shape) for v in sd.values()])
    save("g27_sac", out)


if __name__ == "__main__":
    sys.path.insert(0, os.path.abspath(sys.argv[1]))
    main()
