"""Gaussian policy head on the observation trunk.  Mirrors ``dppo/model/common/mlp_gaussian.py:283-362`` (reference
``Gaussian_MLP``): mean = [tanh](ResidualMLP(state)); sigma fixed, or learned per action dimension (``logvar``, clamped
to [log std_min^2, log std_max^2]).  Parameter names match the reference state dict (``mlp_mean.layers.*``, ``logvar``,
``logvar_min``, ``logvar_max``).  The arithmetic is the HIP library's (``dppo_gaussian_*``, csrc/gaussian.hip around the
fused trunk kernels); this class owns parameters only.

Built: ``residual_style=True`` with ``fixed_std`` given -- the d3il / furniture fine-tuning cfgs (7 of the 10 shipped
PPO_Gaussian cfgs) -- and the SAC actor: the state-dependent ``mlp_logvar`` head on a plain ``MLP`` base (``fixed_std=None``,
``tanh_output=False``, ``residual_style=False``; reference :304-321, 370-379), and IBRL's actor: a fixed std on a plain ``MLP``
trunk, with dropout behind every hidden Linear where the cfg asks for it, under the keyword ``plain_fixed_std=True`` (which
``IBRL_Gaussian``'s cfg node sets): sampling only, no BC / PPO loss.  Not built (raises): the state-dependent head with
``tanh_output=True`` (walker2d pre-training, the three gym ``scratch`` PPO cfgs: no BC / PPO loss exists for it) and plain
(non-residual) trunks with a fixed std outside that keyword.
"""
from __future__ import annotations

import math

import torch
from torch import nn

from dppo_amd import hip
from dppo_amd.model.common.mlp import MLP, SUPPORTED_ACT, HipNet, ResidualMLP
from dppo_amd.model.common.vit import VisionMixin


class Gaussian_MLP(HipNet):
    def __init__(self, action_dim, horizon_steps, cond_dim, mlp_dims=[256, 256, 256], activation_type="Mish",
                 tanh_output=True, residual_style=False, use_layernorm=False, dropout=0.0, fixed_std=None,
                 learn_fixed_std=False, std_min=0.01, std_max=1, precision="bf16", plain_fixed_std=False):
        super().__init__()
        self.plain_fixed_std, self.dropout = False, 0.0
        if plain_fixed_std:
            self._init_plain_fixed_std(action_dim, horizon_steps, cond_dim, list(mlp_dims), activation_type, tanh_output,
                                       residual_style, use_layernorm, dropout, fixed_std, learn_fixed_std, std_min, std_max, precision)
            return
        if fixed_std is None and (tanh_output or residual_style):
            raise NotImplementedError("dppo_amd: Gaussian_MLP with a state-dependent logvar head (fixed_std=None) is built for "
                                      "tanh_output=False on a plain trunk only (the SAC actor); no BC / PPO loss exists for it")
        if fixed_std is not None and not residual_style:
            raise NotImplementedError("dppo_amd: Gaussian_MLP needs residual_style=True (plain MLP trunk not built)")
        if dropout:
            raise NotImplementedError("Dropout not implemented for residual MLP!")
        self.action_dim, self.horizon_steps, self.cond_dim = action_dim, horizon_steps, cond_dim
        out_dim = action_dim * horizon_steps
        if fixed_std is None:
            self._init_state_dependent(cond_dim, list(mlp_dims), out_dim, activation_type, use_layernorm, std_min, std_max,
                                       precision)
            return
        self.mlp_mean = ResidualMLP([cond_dim] + list(mlp_dims) + [out_dim], activation_type=activation_type,
                                    out_activation_type="Identity", use_layernorm=use_layernorm)
        if learn_fixed_std:  # initialised to fixed_std (reference :331-336)
            self.logvar = nn.Parameter(torch.log(torch.tensor([fixed_std ** 2 for _ in range(action_dim)])),
                                       requires_grad=True)
        self.logvar_min = nn.Parameter(torch.log(torch.tensor(std_min ** 2)), requires_grad=False)
        self.logvar_max = nn.Parameter(torch.log(torch.tensor(std_max ** 2)), requires_grad=False)
        self.use_fixed_std, self.fixed_std, self.learn_fixed_std = True, fixed_std, learn_fixed_std
        self.tanh_output = tanh_output
        self.prec = hip.PREC_BY_NAME[precision]
        self._cache_clamp_bounds()

    def _init_plain_fixed_std(self, action_dim, horizon_steps, cond_dim, mlp_dims, activation_type, tanh_output, residual_style,
                              use_layernorm, dropout, fixed_std, learn_fixed_std, std_min, std_max, precision):
        """IBRL's actor (reference :323-329 with ``residual_style=False``): ``mlp_mean`` = plain [cond] + mlp_dims + [Ta*Da],
        names ``mlp_mean.moduleList.{i}.linear_1.*``, a tanh mean per ``tanh_output``, a fixed std, ``nn.Dropout(dropout)`` behind
        every hidden Linear.  The library samples from it (``dppo_gaussian_sample_drop``, ``dppo_ibrl_act``); nothing trains it yet."""
        if fixed_std is None or residual_style:
            raise NotImplementedError("dppo_amd: plain_fixed_std is the plain (residual_style=False) trunk with fixed_std given")
        if use_layernorm or learn_fixed_std:
            raise NotImplementedError("dppo_amd: plain_fixed_std is built without LayerNorm and without a learned std "
                                      "(no shipped IBRL cfg sets either)")
        self.action_dim, self.horizon_steps, self.cond_dim = action_dim, horizon_steps, cond_dim
        self.mlp_mean = MLP([cond_dim] + mlp_dims + [action_dim * horizon_steps], activation_type=activation_type,
                            out_activation_type="Identity", dropout=dropout)
        self.logvar_min = nn.Parameter(torch.log(torch.tensor(std_min ** 2)), requires_grad=False)
        self.logvar_max = nn.Parameter(torch.log(torch.tensor(std_max ** 2)), requires_grad=False)
        self.use_fixed_std, self.fixed_std, self.learn_fixed_std = True, fixed_std, False
        self.tanh_output, self.plain_fixed_std, self.dropout = tanh_output, True, float(dropout)
        self.prec = hip.PREC_BY_NAME[precision]
        self._cache_clamp_bounds()

    def _init_state_dependent(self, cond_dim, mlp_dims, out_dim, activation_type, use_layernorm, std_min, std_max, precision):
        """The state-dependent std (reference :304-321, 370-379): ``mlp_base`` = plain [cond] + mlp_dims with the hidden
        activation on its last layer too, ``mlp_mean`` and ``mlp_logvar`` one Linear(H, Ta*Da) each.  To the library this is ONE
        plain trunk with out_dim = 2 Ta*Da whose last layer is the two heads stacked (rows [0, AF) the mean's, [AF, 2 AF) the raw
        logvar's); the squash of the SAMPLE and the log-probability are the caller's (``SAC_Gaussian``, csrc/sac.hip)."""
        if use_layernorm:
            raise NotImplementedError("dppo_amd: plain MLP with LayerNorm / dropout / appended inputs is not built")
        H = mlp_dims[-1]
        if len(mlp_dims) < 2 or any(d != H for d in mlp_dims) or H % 64:
            raise NotImplementedError("dppo_amd: plain MLP needs >= 2 hidden layers of one width (a multiple of 64)")
        if activation_type not in SUPPORTED_ACT:
            raise NotImplementedError(f"dppo_amd: activation {activation_type!r} not built (ReLU, Mish are)")

        def stack(dims):  # reference MLP's module names: moduleList.{i}.linear_1
            m = nn.Module()
            m.moduleList = nn.ModuleList()
            for i in range(len(dims) - 1):
                layer = nn.Module()
                layer.linear_1 = nn.Linear(dims[i], dims[i + 1])
                m.moduleList.append(layer)
            return m
        # (registration order is the reference's state-dict order: logvar_min, logvar_max come first there)
        self.logvar_min = nn.Parameter(torch.log(torch.tensor(std_min ** 2)), requires_grad=False)
        self.logvar_max = nn.Parameter(torch.log(torch.tensor(std_max ** 2)), requires_grad=False)
        self.mlp_base = stack([cond_dim] + mlp_dims)
        self.mlp_mean = stack([H, out_dim])
        self.mlp_logvar = stack([H, out_dim])
        self.hidden, self.n_blocks, self.act = H, len(mlp_dims) - 1, SUPPORTED_ACT[activation_type]
        self.use_fixed_std, self.fixed_std, self.learn_fixed_std, self.tanh_output = False, None, False, False
        self.prec = hip.PREC_BY_NAME[precision]
        self._cache_clamp_bounds()

    def _cache_clamp_bounds(self):
        """The clamp bounds as Python floats for the per-call cfg struct: they are constants, and reading them from the
        (device) parameters on every call would be two host synchronisations per step."""
        object.__setattr__(self, "_lv_bounds", (float(self.logvar_min), float(self.logvar_max)))

    def _load_from_state_dict(self, *args, **kwargs):
        super()._load_from_state_dict(*args, **kwargs)
        self._cache_clamp_bounds()  # a checkpoint carries logvar_min / logvar_max

    def trunk_parameters(self):
        if not self.use_fixed_std:  # the plain layout wants W (2 AF x H) then b (2 AF): [..., Wm, Wl, bm, bl]
            m, l = self.mlp_mean.moduleList[0].linear_1, self.mlp_logvar.moduleList[0].linear_1
            return list(self.mlp_base.parameters()) + [m.weight, l.weight, m.bias, l.bias]
        return list(self.mlp_mean.parameters())

    def net_desc(self) -> hip.NetDesc:
        d = self.__dict__.get("_desc_cache")
        if d is None and not self.use_fixed_std:
            d = hip.NetDesc(kind=1, in_dim=self.cond_dim, hidden=self.hidden, n_blocks=self.n_blocks,
                            out_dim=2 * self.action_dim * self.horizon_steps, act=self.act, time_dim=0, act_flat=0,
                            cond_dim=self.cond_dim, cond_hidden=0, cond_out=0, use_layernorm=0, plain=1)
            object.__setattr__(self, "_desc_cache", d)
        if d is None:
            m = self.mlp_mean
            d = hip.NetDesc(kind=1, in_dim=self.cond_dim, hidden=m.hidden, n_blocks=m.n_blocks, out_dim=m.out_dim, act=m.act,
                            time_dim=0, act_flat=0, cond_dim=self.cond_dim, cond_hidden=0, cond_out=0,
                            use_layernorm=m.use_layernorm, plain=m.plain)
            object.__setattr__(self, "_desc_cache", d)
        return d

    def sac_cfg(self, deterministic=False, randn_clip=10.0, squash=True) -> hip.SacCfg:
        return hip.SacCfg(horizon_steps=self.horizon_steps, action_dim=self.action_dim, deterministic=int(bool(deterministic)),
                          squash=int(bool(squash)), logvar_min=self._lv_bounds[0], logvar_max=self._lv_bounds[1],
                          randn_clip=float(randn_clip), pad=0.0, seed_lo=0, seed_hi=0)

    def gaussian_cfg(self, deterministic=False, randn_clip=10.0) -> hip.GaussianCfg:
        if not self.use_fixed_std:
            raise NotImplementedError("dppo_amd: no BC / PPO loss exists for a state-dependent std (SAC_Gaussian samples it)")
        return hip.GaussianCfg(
            horizon_steps=self.horizon_steps, action_dim=self.action_dim, tanh_mean=int(bool(self.tanh_output)),
            std_mode=1 if self.learn_fixed_std else 0, norm_adv=1, has_vclip=0, deterministic=int(bool(deterministic)), pad=0,
            fixed_std=float(self.fixed_std), logvar_min=self._lv_bounds[0], logvar_max=self._lv_bounds[1],
            randn_clip=float(randn_clip), clip_ploss_coef=0.0, clip_vloss_coef=0.0, seed_lo=0, seed_hi=0)

    def logvar_ptr(self):
        return self.logvar.data_ptr() if self.learn_fixed_std else None

    @torch.no_grad()
    def forward(self, cond):
        """cond {"state": (B,To,Do)} -> (mean (B,Ta*Da), scale (B,Ta*Da)), like the reference's forward (inference only:
        the differentiable evaluation is fused into ``PPO_Gaussian.loss``)."""
        import ctypes as C
        if not self.use_fixed_std:
            raise NotImplementedError("dppo_amd: the state-dependent head is evaluated inside SAC_Gaussian (dppo_sac_sample)")
        if self.plain_fixed_std and self.training and self.dropout > 0:
            raise NotImplementedError("dppo_amd: a dropout actor in train() is sampled through GaussianModel (its mask is per call)")
        state = cond["state"]
        hip.require_gpu(state, "Gaussian_MLP.forward")
        B = state.shape[0]
        obs = state.reshape(B, -1).contiguous().float()
        AF = self.action_dim * self.horizon_steps
        lib, d = hip.load(), self.net_desc()
        cfg = self.gaussian_cfg()
        zeros = torch.zeros(B, AF, device=state.device)
        actions = torch.empty(B, AF, device=state.device)
        mean = torch.empty(B, AF, device=state.device)
        wsb = lib.dppo_gaussian_workspace_bytes(C.byref(d), None, self.prec, B)
        ws = self.__dict__.setdefault("_ws", hip.Workspace()).get(wsb, state.device)
        hip.check(lib.dppo_gaussian_sample(C.byref(d), self.prec, self.flat_params().data_ptr(),
                                           self.packed(self.prec, 0).data_ptr(), C.byref(cfg), self.logvar_ptr(),
                                           obs.data_ptr(), zeros.data_ptr(), B, actions.data_ptr(), mean.data_ptr(),
                                           ws.data_ptr(), ws.numel(), hip.stream()), "dppo_gaussian_sample")
        if self.learn_fixed_std:
            lv = torch.clamp(self.logvar.detach(), self.logvar_min, self.logvar_max)
            scale = torch.exp(0.5 * lv).view(1, self.action_dim).repeat(B, self.horizon_steps)
        else:
            scale = torch.full_like(mean, self.fixed_std)
        return mean, scale


class Gaussian_VisionMLP(VisionMixin, Gaussian_MLP):
    """ViT backbone + SpatialEmb, then the Gaussian head's trunk on cat[feat, state]; the mean is always tanh-squashed.
    Mirrors ``dppo/model/common/mlp_gaussian.py:112-281``."""

    def __init__(self, backbone, action_dim, horizon_steps, cond_dim, img_cond_steps=1, mlp_dims=[256, 256, 256],
                 activation_type="Mish", residual_style=False, use_layernorm=False, fixed_std=None, learn_fixed_std=False,
                 std_min=0.01, std_max=1, spatial_emb=0, visual_feature_dim=128, dropout=0, num_img=1, augment=False,
                 precision="bf16"):
        Gaussian_MLP.__init__(self, action_dim, horizon_steps, cond_dim + spatial_emb * num_img, mlp_dims=mlp_dims,
                              activation_type=activation_type, tanh_output=True, residual_style=residual_style,
                              use_layernorm=use_layernorm, dropout=0.0, fixed_std=fixed_std, learn_fixed_std=learn_fixed_std,
                              std_min=std_min, std_max=std_max, precision=precision)
        self._init_vision(backbone, cond_dim, img_cond_steps, spatial_emb, num_img, augment, dropout, precision)
        self._vision_modules_first("backbone", "compress", "compress1", "compress2")

    @torch.no_grad()
    def forward(self, cond):
        return Gaussian_MLP.forward(self, {"state": self.encode_obs(cond)})
