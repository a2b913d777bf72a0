"""One behaviour-cloning pre-training step (GaussianModel.loss / GMMModel.loss + fused AdamW) in a loop, for a kernel trace:

    rocprofv3 --kernel-trace --stats --output-format csv -d out -- python3 tools/bc_step_bench.py --steps 20

Default shape: cfg/robomimic/pretrain/can/pre_gaussian_mlp.yaml (23 -> residual 512 x 3 -> Ta 4 x Da 7, 256 rows, bf16);
``--gmm`` runs pre_gmm_mlp.yaml's two trunks (5 modes).  Prints one JSON line with the event-timed step."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from dppo_amd.util.optim import FlatAdamW, step_many  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rows", type=int, default=256)
    ap.add_argument("--precision", default="bf16")
    ap.add_argument("--gmm", action="store_true")
    a = ap.parse_args()
    dev, cond, Ta, Da = "cuda:0", 23, 4, 7
    if a.gmm:
        from dppo_amd.model.common.gmm import GMMModel
        from dppo_amd.model.common.mlp_gmm import GMM_MLP
        net = GMM_MLP(action_dim=Da, horizon_steps=Ta, cond_dim=cond, mlp_dims=[512, 512, 512], num_modes=5, residual_style=True,
                      fixed_std=0.1, precision=a.precision)
        model = GMMModel(network=net, horizon_steps=Ta, device=dev)
    else:
        from dppo_amd.model.common.gaussian import GaussianModel
        from dppo_amd.model.common.mlp_gaussian import Gaussian_MLP
        net = Gaussian_MLP(action_dim=Da, horizon_steps=Ta, cond_dim=cond, mlp_dims=[512, 512, 512], residual_style=True,
                           fixed_std=0.1, precision=a.precision)
        model = GaussianModel(network=net, horizon_steps=Ta, device=dev)
    torch.manual_seed(0)
    state = torch.rand(a.rows, 1, cond, device=dev) * 2 - 1
    action = torch.rand(a.rows, Ta, Da, device=dev) * 2 - 1
    opt = FlatAdamW(net.flat_params(), lr=1e-4, weight_decay=1e-6)

    def step():
        loss, _ = model.loss(action, {"state": state}, ent_coef=0.0)
        step_many([opt.slot(model.last_loss_grad)])
        net.mark_updated()
        return loss

    for _ in range(a.warmup):
        step()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(a.steps):
        loss = step()
    e1.record()
    torch.cuda.synchronize()
    print(json.dumps({"what": "gmm_bc_step" if a.gmm else "gaussian_bc_step", "rows": a.rows, "precision": a.precision,
                      "steps": a.steps, "ms_per_step": e0.elapsed_time(e1) / a.steps, "loss": float(loss.detach())}))


if __name__ == "__main__":
    main()
