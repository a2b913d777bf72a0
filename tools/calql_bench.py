"""Time Cal-QL's critic loss at the shipped kitchen shape (batch 256, obs 60, Ta*Da = 9, twin of [256, 256, 256] ReLU LayerNorm
trunks, 10 random actions and 10 policy samples per row), bf16 and fp32:

    python3 tools/calql_bench.py profiles/calql_loss_critic.json

  hip     CalQL_Gaussian.loss_critic out of plain tensors with the policy's three samples given (dppo_calql_q_loss_fwd_bwd: the row
          builder, the two target trunks on N S rows, both trunks forward and backward ONCE on N (R + 3) rows, the target, loss and
          statistics kernels) -- the gradient is left in critic.flat_grads(); no optimiser step on either side;
  draws   the same with random_actions=None: the kernel draws them (one CPU-generator seed per call);
  eager   the restatement of tests/golden/make_golden_calql_cases.py (loss_critic, fp32) as plain torch on the same GPU with the
          same samples given, and torch.autograd.grad over both trunks' parameters.
Every arm is warmed, each pass times >= 0.5 s of work between two device events, the median of ten passes is reported
(tools/idql_bench.timed).  The launch count of a call is csrc/calql.h's (read off the code).  First measurements of a new path: no
threshold is set."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from tests.golden import make_golden_calql_cases as K  # noqa: E402
from tools.idql_bench import measured_on, timed  # noqa: E402

DEV, CASE, N = "cuda:0", "kitchen", 256


def make_model(prec):
    from dppo_amd.model.common.critic import CriticObsAct
    from dppo_amd.model.common.mlp_gaussian import Gaussian_MLP
    from dppo_amd.model.rl.gaussian_calql import CalQL_Gaussian
    od, ta, da, dims, act, R, S = K.CALQL_NETS[CASE]
    actor = Gaussian_MLP(da, ta, od, mlp_dims=dims, activation_type=act, tanh_output=False, fixed_std=None, std_min=K.S.STD_MIN,
                         std_max=K.S.STD_MAX, precision=prec)
    critic = CriticObsAct(cond_dim=od, mlp_dims=dims, action_dim=da, action_steps=ta, activation_type=act, use_layernorm=True,
                          double_q=True, twin_layernorm=True, precision=prec)
    m = CalQL_Gaussian(actor=actor, critic=critic, cql_min_q_weight=K.MIN_Q_WEIGHT, cql_n_actions=S, horizon_steps=ta, device=DEV,
                       randn_clip_value=K.S.RANDN_CLIP, tanh_output=True)
    m.critic.load_state_dict(K.twin_params(CASE), strict=True)
    m.target_critic.load_state_dict(K.twin_params(CASE, K.TARGET_EPS), strict=True)
    m.n_random_actions = R
    return m


def hip_step(model, b, sm, ret, draws=False):
    def step():
        model.loss_critic({"state": b["obs"]}, {"state": b["next_obs"]}, b["actions"], None if draws else b["random_actions"], b["reward"],
                          ret, b["terminated"], K.GAMMA, samples=sm)
    return step


def eager_step(b, sm, ret):
    q = {k: v.to(DEV).clone().requires_grad_(True) for k, v in K.twin_params(CASE).items()}
    tq = {k: v.to(DEV) for k, v in K.twin_params(CASE, K.TARGET_EPS).items()}

    def step():
        K.loss_critic(q, tq, CASE, b, sm, ret, host_stats=False)
    return step


def main(path):
    b = {k: v.to(DEV) for k, v in K.inputs(CASE, N).items()}
    sm = {k: v.to(DEV) for k, v in K.samples(CASE, N).items()}
    ret = K.returns_of(CASE, N).to(DEV)
    R, S = K.n_samples(CASE)
    out = dict(device=torch.cuda.get_device_name(0), torch=torch.__version__, measured_on=measured_on(), batch=N, n_random=R, n_next=S,
               critic_rows=N * (R + 3), target_rows=N * S, launches_per_call_read_off_the_code=84,
               method="median of 10 passes of >= 0.5 s between device events, every arm warmed")
    eag, reps = timed(eager_step(b, sm, ret))
    out["eager_torch_fp32"] = dict(ms_per_call=eag, calls_per_pass=reps)
    print("eager", eag, flush=True)
    for prec in ("bf16", "fp32"):
        for draws in (False, True):
            ms, reps = timed(hip_step(make_model(prec), b, sm, ret, draws))
            out[f"{prec}{'/draws' if draws else ''}"] = dict(ms_per_call=ms, calls_per_pass=reps, eager_over_hip=eag / ms)
            print(prec, "draws" if draws else "given", ms, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main(sys.argv[1])
