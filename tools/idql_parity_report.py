"""Measure IDQL's critic losses (IDQLDiffusion.loss_critic_v / loss_critic_q) against the reference fixture g24 in fp32 and
bf16 on the GPU, per case and worst per loss -> the JSON the bf16 bounds of tests/test_idql.py come from:

    python3 tools/idql_parity_report.py profiles/idql_parity.json

Uses that test module's own helpers (build_model / run_losses / case_errors), so the test and the record measure the same thing."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def measured_on():
    """The accelerator the numbers were taken on, from the device itself: its gfx architecture, and the product it is."""
    arch = torch.cuda.get_device_properties(0).gcnArchName.split(":")[0]
    return {"gfx950": "MI355X (gfx950)"}.get(arch, arch)

from tests import test_idql as Tm  # noqa: E402
from tests.conftest import load_golden  # noqa: E402


def main(path):
    g = load_golden("g24_idql")
    out = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "measured_on": measured_on(), "cases": {}}
    for prec in ("fp32", "bf16"):
        for net, n in Tm.K.IDQL_CASES:
            m = Tm.build_model(net, prec, float(g[f"{net}_{n}_v_bias"]))
            res = Tm.run_losses(m, Tm.case_batch(g, net, n))
            sign_ok, errs = Tm.case_errors(g, net, n, m, res)
            adv_err = float((res["adv"].cpu() - torch.from_numpy(g[f"{net}_{n}_adv"])).abs().max())
            for which, e in errs.items():
                e.update(precision=prec, sign_adv_agrees=sign_ok, max_adv_error=adv_err)
                out["cases"][f"{net}_{n}/{which}/{prec}"] = e
            print(net, n, prec, sign_ok, errs, flush=True)
    for prec in ("fp32", "bf16"):
        for which in ("v", "q"):
            rows = [v for k, v in out["cases"].items() if k.endswith(f"/{which}/{prec}")]
            out[f"worst/{which}/{prec}"] = dict(loss=max(r["loss"] for r in rows), grad=max(r["grad"] for r in rows),
                                                cos=min(r["cos"] for r in rows), sign_adv_agrees=all(r["sign_adv_agrees"] for r in rows),
                                                max_adv_error=max(r["max_adv_error"] for r in rows))
            print("WORST", which, prec, out[f"worst/{which}/{prec}"], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main(sys.argv[1])
