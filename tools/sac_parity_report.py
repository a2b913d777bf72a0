"""Measure SAC's actor loss (SAC_Gaussian.loss_actor) in bf16 on the GPU against the bf16 rounding yardstick of tests/test_sac.py,
per case, and the saturated sample's error beside the reference's own -> the record beside that test (the test reads nothing from
it):

    python3 tools/sac_parity_report.py profiles/sac_parity.json

Per case: e_y, the error of the restatement with every Linear's operands rounded to bf16 against the fp32 restatement on the ``sel``
the bf16 call returned, and the call's own errors against that fp32 restatement (loss, d_a, worst tensor, 1 - cosine of the whole
gradient), plus the number of rows whose ``sel`` differs from the fp32 restatement's.  ``saturated``: for the ``tiny_sat`` case the
fp32 call's sample and log-probability against the float64 restatement, and e_ref, the same error of the reference's fp32 values in
g27.  Uses that test module's own helpers, so the test and the record measure the same thing."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from tools.idql_bench import measured_on  # noqa: E402
from tests import test_sac as Tm  # noqa: E402
from tests.conftest import load_golden  # noqa: E402


def saturated(g):
    (case, n), K = Tm.K.SAT_CASES[0], Tm.K
    m, b, r = Tm.make_model(case, "fp32", Tm.DEV), Tm.dev_batch(case, n), Tm.restated(case, n)
    a, logp, _ = Tm.run_sample(m, b)
    ea, el = Tm.sample_errors(case, n, a, logp, r["actor"])
    return dict(case=f"{case}_{n}", u_abs_max=float(r["actor"]["u"].abs().max()), randn_clip=K.RANDN_CLIP,
                call=dict(sample=ea, logp=el),
                e_ref=dict(sample=float(np.abs(g[f"{case}_{n}_a"].astype(np.float64) - r["actor"]["a"].numpy()).max()),
                           logp=float(np.abs(g[f"{case}_{n}_logp"].astype(np.float64) - r["actor"]["logp"].numpy()).max())))


def main(path):
    g = load_golden("g27_sac")
    out = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "measured_on": measured_on(), "cases": {}}
    out["saturated"] = saturated(g)
    print(out["saturated"], flush=True)
    for case, n in Tm.K.CASES:
        e_y, e_c, flips = Tm.bf16_figures(case, n)
        worst = max(e_c["per"], key=lambda k: e_c["per"][k] / (e_y["per"][k] + 1e-30))
        out["cases"][f"{case}_{n}"] = dict(yardstick=e_y, call=e_c, worst_tensor=worst, sel_off_fp32=flips)
        print(case, n, {k: v for k, v in e_y.items() if k != "per"}, {k: v for k, v in e_c.items() if k != "per"}, worst,
              e_c["per"][worst], e_y["per"][worst], flips, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main(sys.argv[1])
