"""Measure QSM's two losses and the critic's action gradient g (QSMDiffusion.loss_critic / loss_actor) against the reference
fixture g25 in fp32 and bf16 on the GPU, per case and worst per quantity -> the JSON the bf16 bounds of tests/test_qsm.py come from:

    python3 tools/qsm_parity_report.py profiles/qsm_parity.json

Uses that test module's own helpers (make_model / run_critic / run_actor / qsm_errors), so the test and the record measure the
same thing."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from tools.idql_bench import measured_on  # noqa: E402
from tests import test_qsm as Tm  # noqa: E402
from tests.conftest import load_golden  # noqa: E402


def main(path):
    g = load_golden("g25_qsm")
    out = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "measured_on": measured_on(), "cases": {}}
    for prec in ("fp32", "bf16"):
        for net, n in Tm.K.CRITIC_CASES:
            m, b = Tm.make_model(net, prec, Tm.DEV), Tm.dev_batch(net, n)
            crit = Tm.run_critic(m, b)
            act = Tm.run_actor(m, net, b) if (net, n) in Tm.K.ACTOR_CASES else None
            errs = Tm.qsm_errors(g, net, n, m, crit, act)
            for which, e in errs.items():
                e.update(precision=prec)
                out["cases"][f"{net}_{n}/{which}/{prec}"] = e
            print(net, n, prec, errs, flush=True)
    for prec in ("fp32", "bf16"):
        for which in ("critic", "actor", "g"):
            rows = [v for k, v in out["cases"].items() if k.endswith(f"/{which}/{prec}")]
            out[f"worst/{which}/{prec}"] = dict(loss=max(r["loss"] for r in rows), grad=max(r["grad"] for r in rows),
                                                cos=min(r["cos"] for r in rows))
            print("WORST", which, prec, out[f"worst/{which}/{prec}"], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main(sys.argv[1])
