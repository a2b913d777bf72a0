"""Measure the behaviour-cloning losses (GaussianModel.loss / GMMModel.loss) against the reference fixtures g22 / g23 in fp32
and bf16 on the GPU, per case and worst per family -> the JSON the bf16 bounds of tests/test_pretrain_gaussian.py come from:

    python3 tools/bc_parity_report.py profiles/bc_gaussian_parity.json

Uses that test module's own helpers (family_setup / run_loss / bf16_errors), so the test and the record measure the same thing."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from tests import test_pretrain_gaussian as Tm  # noqa: E402
from tests.conftest import load_golden  # noqa: E402


def main(path):
    cache = {}

    def golden(name):
        if name not in cache:
            cache[name] = load_golden(name)
        return cache[name]

    out = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "cases": {}}
    for prec in ("fp32", "bf16"):
        for family, case in Tm.ALL_CASES:
            model, g, prefix, ent_coef = Tm.family_setup(family, case, prec, golden)
            state, action = torch.from_numpy(g[f"{prefix}_state"]).cuda(), torch.from_numpy(g[f"{prefix}_true_action"]).cuda()
            loss, entropy, named, _ = Tm.run_loss(model, state, action, ent_coef)
            m = Tm.bf16_errors(g, prefix, named, loss, entropy)
            m.update(family=family, precision=prec, loss_value=loss, loss_ref=float(g[f"{prefix}_loss"]), entropy_value=entropy,
                     entropy_ref=float(g[f"{prefix}_entropy"]))
            out["cases"][f"{prefix}/{prec}"] = m
            print(prefix, prec, {k: v for k, v in m.items() if k != "per_tensor"}, flush=True)
    for prec in ("fp32", "bf16"):
        for family in ("gaussian", "gmm"):
            rows = [v for v in out["cases"].values() if v["family"] == family and v["precision"] == prec]
            out[f"worst/{family}/{prec}"] = dict(
                loss=max(r["loss"] for r in rows), entropy=max(r["entropy"] for r in rows), grad=max(r["grad"] for r in rows),
                grad_unfiltered=max(max(r["per_tensor"].values()) for r in rows), cos=min(r["cos"] for r in rows),
                cos_trunk=min(r["cos_trunk"] for r in rows))
            print("WORST", family, prec, out[f"worst/{family}/{prec}"], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main(sys.argv[1])
