"""Measure DQL's actor loss (DQLDiffusion.loss_actor, differentiated through the sampling chain) in bf16 on the GPU against the
bf16 rounding yardstick of tests/test_dql.py, per case -> the record beside that test (the test reads nothing from it):

    python3 tools/dql_parity_report.py profiles/dql_parity.json

Per case: e_y, the error of the restatement with every Linear's operands rounded to bf16 against the fp32 restatement on the chain
and masks the bf16 call returned, and the call's own errors against that fp32 restatement (loss, d_a, worst tensor, 1 - cosine of
the whole gradient), plus the number of clamp-mask elements on which the call, and the yardstick run with its own masks, disagree
with the reference.  Uses that test module's own helper (bf16_figures), so the test and the record measure the same thing."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from tools.idql_bench import measured_on  # noqa: E402
from tests import test_dql as Tm  # noqa: E402
from tests.conftest import load_golden  # noqa: E402


def main(path):
    g = load_golden("g26_dql")
    out = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "measured_on": measured_on(), "cases": {}}
    for case, n in Tm.K.CASES:
        e_y, e_c, mism, mism_y = Tm.bf16_figures(g, case, n)
        worst = max(e_c["per"], key=lambda k: e_c["per"][k] / (e_y["per"][k] + 1e-30))
        out["cases"][f"{case}_{n}"] = dict(yardstick=e_y, call=e_c, worst_tensor=worst, masks_off_call=mism, masks_off_yardstick=mism_y)
        print(case, n, {k: v for k, v in e_y.items() if k != "per"}, {k: v for k, v in e_c.items() if k != "per"}, worst, mism, mism_y,
              flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main(sys.argv[1])
