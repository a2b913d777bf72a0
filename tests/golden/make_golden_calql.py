"""Generate the Cal-QL fixture by running the REFERENCE's CalQL_Gaussian / Gaussian_MLP / CriticObsAct on the CPU:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_calql.py <checkout of the reference (the directory holding dppo/)>

Writes tests/golden/g29_calql.npz.  Per case (make_golden_calql_cases.CASES), with every draw of ``Normal.sample`` replaced by the
recipe's (make_golden_sac.recorded_draws) in the reference's call order -- next x S, pi, pi_next: ``loss_critic`` and every critic
gradient (large ones as flat[::61] + norm, make_golden_bc.put_grad), and the statistics {loss, td_1 + td_2, mean diff_1, mean diff_2,
mean q1, mean y} rebuilt from the reference's own modules on the same draws.  The state-dict keys and shapes of CalQL_Gaussian.
Weights and inputs are never stored: both sides rebuild them from make_golden_calql_cases.py.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.dont_write_bytecode = True

from tests.golden import make_golden_calql_cases as K  # noqa: E402
from tests.golden.make_golden_bc import save  # noqa: E402
from tests.golden.make_golden_sac import put_grads, recorded_draws  # noqa: E402

torch.set_num_threads(4)


def ref_model(case, n):
    from dppo.model.common.critic import CriticObsAct
    from dppo.model.common.mlp_gaussian import Gaussian_MLP
    from dppo.model.rl.gaussian_calql import CalQL_Gaussian
    od, ta, da, dims, act, R, S = K.CALQL_NETS[case]
    actor = Gaussian_MLP(action_dim=da, horizon_steps=ta, cond_dim=od, mlp_dims=dims, activation_type=act, tanh_output=False,
                         std_min=K.S.STD_MIN, std_max=K.S.STD_MAX)
    actor.load_state_dict(K.actor_params(case), strict=True)
    q = CriticObsAct(cond_dim=od, mlp_dims=dims, action_dim=da, action_steps=ta, activation_type=act, use_layernorm=True, double_q=True)
    q.load_state_dict(K.twin_params(case), strict=True)
    lo, hi = K.clips_of(case, n)
    m = CalQL_Gaussian(actor=actor, critic=q, cql_clip_diff_min=lo, cql_clip_diff_max=hi, cql_min_q_weight=K.MIN_Q_WEIGHT,
                       cql_n_actions=S, horizon_steps=ta, device="cpu", randn_clip_value=K.S.RANDN_CLIP, tanh_output=True)
    m.target_critic.load_state_dict(K.twin_params(case, K.TARGET_EPS), strict=True)
    return m


def draws(case, n, b):
    _, S = K.n_samples(case)
    z = b["noise"]
    return [z[:n * S], z[n * S:n * S + n], z[n * S + n:]]


def one_case(out, case, n):
    name, b, m = f"{case}_{n}", K.inputs(case, n), ref_model(case, n)
    R, S = K.n_samples(case)
    cond, ncond, ret = {"state": b["obs"]}, {"state": b["next_obs"]}, K.returns_of(case, n)
    with recorded_draws(draws(case, n, b)):
        lc = m.loss_critic(cond, ncond, b["actions"], b["random_actions"], b["reward"], ret, b["terminated"], K.GAMMA)
    lc.backward()
    lo, hi = K.clips_of(case, n)
    with torch.no_grad(), recorded_draws(draws(case, n, b)):  # the statistics, from the reference's modules on the same draws
        rep = {"state": b["next_obs"].repeat_interleave(S, dim=0)}
        na, _ = m(rep, deterministic=False, get_logprob=True)
        pa, lp = m(cond, deterministic=False, get_logprob=True)
        pna, lpn = m(ncond, deterministic=False, get_logprob=True)
        y = b["reward"] + K.GAMMA * (1 - b["terminated"]) * torch.min(*m.target_critic(rep, na)).view(n, S).max(dim=1).values
        qd = m.critic(cond, b["actions"])
        qr = m.critic({"state": b["obs"].repeat_interleave(R, dim=0)}, b["random_actions"].reshape(n * R, *b["actions"].shape[1:]))
        qp, qn = m.critic(cond, pa), m.critic(ncond, pna)
        td, diffs = 0.0, []
        for i in range(2):
            cat = torch.cat([qr[i].view(n, R) - K.log_rand_pi(case), torch.max(qp[i], ret)[:, None] - lp,
                             torch.max(qn[i], ret)[:, None] - lpn], dim=-1)  # the reference's (n, R + 2 n) matrix
            diffs.append(torch.clamp(torch.logsumexp(cat, dim=-1) - qd[i], min=lo, max=hi).double().mean().item())
            td = td + ((qd[i] - y) ** 2).double().mean().item()
    out[f"{name}_stats"] = np.array([lc.item(), td, diffs[0], diffs[1], qd[0].double().mean().item(), y.double().mean().item()])
    put_grads(out, f"{name}_gq", m.critic)
    print(f"  {name}: loss {lc.item():.6f} td {td:.6f} diffs {diffs[0]:.6f} {diffs[1]:.6f}")


def main():
    out = {}
    for case, n in K.CASES:
        one_case(out, case, n)
    sd = ref_model("kitchen", 256).state_dict()
    out["state_dict_keys"] = np.array(list(sd))
    out["state_dict_shapes"] = np.array([",".join(str(int(x)) for x in v.shape) for v in sd.values()])
    save("g29_calql", out)


if __name__ == "__main__":
    sys.path.insert(0, os.path.abspath(sys.argv[1]))
    main()
