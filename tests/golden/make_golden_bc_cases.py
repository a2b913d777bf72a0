"""Case tables and seeded recipes shared by make_golden_bc.py (generator, needs the reference) and
tests/test_pretrain_gaussian.py (no reference needed): behaviour-cloning loss of the Gaussian / mixture policies."""
import numpy as np

from tests.golden.make_golden_cases import GAUSS_CASES, GMM_CASES

BC_N = 64
BC_WEIGHT_SEED, BC_LOGVAR_SEED = 71, 73  # as g12 / g20 build their networks

# name -> ent_coef; the specs are GAUSS_CASES'
BC_GAUSS_CASES = {"gauss_d3il_fixed": 0.0, "gauss_furniture_learned": 0.01, "gauss_nonorm": 0.01}

# mixture networks: name -> (cond_dim, trunk kwargs, Ta, Da, GmmCfg kwargs); gmm_can_fixed01 is the gmm_can networks with the
# std every shipped pre_gmm_mlp.yaml sets; gmm_d3il_learned is the gmm_d3il networks with a learned std
BC_GMM_NETS = {k: v[:5] for k, v in GMM_CASES.items()}
BC_GMM_NETS["gmm_can_fixed01"] = GMM_CASES["gmm_can"][:4] + (dict(GMM_CASES["gmm_can"][4], fixed_std=0.1, learn_fixed_std=False),)
BC_GMM_NETS["gmm_d3il_learned"] = GMM_CASES["gmm_d3il"][:4] + (dict(GMM_CASES["gmm_d3il"][4], fixed_std=0.2, learn_fixed_std=True,
                                                                    std_min=0.1, std_max=0.3),)
# The cases whose learned logvar has entries OUTSIDE the clamp range [log std_min^2, log std_max^2] (at least one below and one
# above), so that the clamp's pass-through mask in the loss and in the entropy bonus is exercised with zeros.  g12 / g20's own
# recipe (log fixed_std^2 + U(-0.4, 0.4)) stays inside the range in every case, so these entries are placed by hand.
BC_CLAMPED = ("gauss_nonorm", "gmm_d3il_learned")
# kinds of true_action (all clamped to [-1, 1]):
#   near    one component's mean + 0.02 N(0, 1): one responsibility ~ 1
#   between midpoint of two components' means
#   far     uniform in [-1, 1], independent of the state: with std 0.1 every component's log-density is hundreds of nats below 0
BC_GMM_KINDS = ("near", "between", "far")
BC_GMM_CASES = [(net, kind) for net in sorted(BC_GMM_NETS) for kind in BC_GMM_KINDS]


def _logvar(name, size, kw, seed):
    if not kw["learn_fixed_std"]:
        return None
    rs = np.random.RandomState(seed)
    lv = np.log(kw["fixed_std"] ** 2) + rs.uniform(-0.4, 0.4, size=size)
    if name in BC_CLAMPED:
        lv[0] = np.log(kw["std_min"] ** 2) - 0.3   # below the range: sigma = std_min, no gradient
        lv[-1] = np.log(kw["std_max"] ** 2) + 0.3  # above the range: sigma = std_max, no gradient
    lv = lv.astype(np.float32)
    inside = clamp_mask(lv, kw)
    assert (name in BC_CLAMPED) == (not inside.all()), (name, lv)  # a later change of seed or range cannot lose the zeros
    return lv


def clamp_mask(logvar, kw):
    """True where torch.clamp(logvar, log std_min^2, log std_max^2) passes the gradient (closed interval, fp32 bounds as the
    networks hold them)."""
    lo, hi = np.log(np.float32(kw["std_min"] ** 2)), np.log(np.float32(kw["std_max"] ** 2))
    return (logvar >= lo) & (logvar <= hi)


def gauss_logvar(case, action_dim, kw, seed=BC_LOGVAR_SEED):
    """Seeded per-dimension log-variance of a learned-std Gaussian head (None for a fixed std)."""
    return _logvar(case, action_dim, kw, seed)


def gmm_logvar(net, action_dim, kw, seed=BC_LOGVAR_SEED):
    """The same for a mixture head: one entry per (mode, action dimension)."""
    return _logvar(net, action_dim * kw["num_modes"], kw, seed)
