"""Gaussian policy parameterisation.  Mirrors ``dppo/model/common/gaussian.py:14-121`` (reference ``GaussianModel``):
constructor surface, checkpoint loading, ``loss`` (behaviour cloning: one ``dppo_gaussian_bc_loss_fwd_bwd`` call), ``forward``
(sampling with the draw clipped to +-randn_clip_value sigma).
Sampling is one trunk forward + one epilogue kernel (``dppo_gaussian_sample``); noise is drawn in the kernel (Philox keyed
from torch's CPU generator) unless a recorded tensor is passed (parity tests)."""
from __future__ import annotations

import ctypes as C
import logging

import torch

from dppo_amd import hip
# _FusedDenoiseLoss: (value, gradient views, *parameters) -> scalar with a backward
from dppo_amd.model.diffusion.diffusion import _FusedDenoiseLoss, flat_views

log = logging.getLogger(__name__)


class GaussianModel(torch.nn.Module):
    _squash_built = False  # tanh applied to the SAMPLE, get_logprob, reparameterize: the SAC subclass's

    def __init__(self, network, horizon_steps, network_path=None, device="cuda:0", randn_clip_value=10,
                 tanh_output=False, precision=None):
        super().__init__()
        if tanh_output and not self._squash_built:  # (SAC_Gaussian, model/rl/gaussian_sac.py, builds it)
            raise NotImplementedError("dppo_amd: tanh applied to the SAMPLED action (SAC / RLPD) is out of scope")
        self.device = device
        self.network = network.to(device)
        if network_path is not None:
            checkpoint = torch.load(network_path, map_location=self.device, weights_only=True)  # safe loader only
            self.load_state_dict(checkpoint["model"], strict=False)
            log.info("Loaded actor from %s", network_path)
        self.horizon_steps = horizon_steps
        self.randn_clip_value = randn_clip_value
        self.tanh_output = tanh_output
        self.prec = hip.PREC_BY_NAME[precision] if precision is not None else network.prec
        object.__setattr__(self, "_ws_g", hip.Workspace())
        object.__setattr__(self, "_ws_bc", hip.Workspace())

    def loss(self, true_action, cond, ent_coef):
        """Behaviour cloning (reference :49-65): mean over the B*Ta*Da elements of -log N(a; mu, sigma) minus ``ent_coef`` times
        the mean element entropy -> (loss, {"entropy": entropy}), device scalars, no host sync.  Value and every gradient
        come from one library call (``dppo_gaussian_bc_loss_fwd_bwd``); the returned scalar carries them into
        ``.backward()``, and the flat d loss / d trunk parameters stays in ``last_loss_grad`` (d loss / d logvar in
        ``last_logvar_grad``) for callers that step a flat optimiser."""
        state = cond["state"]
        net = self.network
        if getattr(net, "plain_fixed_std", False):
            raise NotImplementedError("dppo_amd: behaviour cloning of the plain fixed-std actor (IBRL's pre-training, with the "
                                      "backward through dropout) is not built")
        hip.require_gpu(state, type(self).__name__ + ".loss")
        if getattr(net, "is_vision", False):
            raise NotImplementedError("dppo_amd: supervised pre-training of the pixel Gaussian policy is not built")
        B, dev = len(true_action), state.device
        AF = net.action_dim * net.horizon_steps
        obs = state.reshape(B, -1).contiguous().float()
        act = true_action.reshape(B, AF).contiguous().float()
        lib, d = hip.load(), net.net_desc()
        cfg = net.gaussian_cfg(randn_clip=self.randn_clip_value)
        flat = net.flat_params()
        grad = torch.empty_like(flat)
        lv_grad = torch.empty(net.action_dim, device=dev) if net.learn_fixed_std else None
        out = torch.empty(2, dtype=torch.float64, device=dev)
        wsb = lib.dppo_gaussian_bc_workspace_bytes(C.byref(d), self.prec, B)
        if wsb < 0:
            hip.check(int(wsb), "dppo_gaussian_bc_workspace_bytes")
        ws = self._ws_bc.get(wsb, dev)
        hip.check(lib.dppo_gaussian_bc_loss_fwd_bwd(
            C.byref(d), self.prec, flat.data_ptr(), net.packed(self.prec, 0).data_ptr(), C.byref(cfg), net.logvar_ptr(),
            obs.data_ptr(), act.data_ptr(), B, float(ent_coef), grad.data_ptr(), hip.ptr(lv_grad), out.data_ptr(), ws.data_ptr(),
            ws.numel(), hip.stream()), "dppo_gaussian_bc_loss_fwd_bwd")
        object.__setattr__(self, "last_loss_grad", grad)
        object.__setattr__(self, "last_logvar_grad", lv_grad)
        params = net.trunk_parameters()  # the flat image is their concatenation in this order
        views = flat_views(grad, params)
        if lv_grad is not None:
            params, views = params + [net.logvar], views + [lv_grad]
        return _FusedDenoiseLoss.apply(out[0], views, *params), {"entropy": out[1].float()}

    def _dropout_of(self, net, B, dev, drop_mask=None, want_mask=False):
        """(struct or None, tensors to keep alive, the mask buffer written or None): the per-call dropout of ``net``'s trunk
        (csrc/ibrl.h), live iff ``net.training`` and ``net.dropout > 0`` as in torch.  ``drop_mask`` (L, B, H) uint8, 1 = keep,
        replaces the draw; ``want_mask`` has the mask used written out."""
        p = float(getattr(net, "dropout", 0.0))
        if not (net.training and p > 0):
            if drop_mask is not None:
                raise ValueError("drop_mask given, but this actor's dropout is off (eval() or dropout = 0)")
            return None, (), None
        d = net.net_desc()
        shape = (d.n_blocks + 1, B, d.hidden)
        drop = hip.Dropout(p=p, seed_lo=0, seed_hi=0, pad=0, mask=None, mask_out=None)
        keep, out = [], None
        if drop_mask is not None:
            if tuple(drop_mask.shape) != shape:
                raise ValueError(f"drop_mask must be {shape} (hidden layers, rows, hidden), got {tuple(drop_mask.shape)}")
            m = drop_mask.to(device=dev, dtype=torch.uint8).contiguous()
            drop.mask = m.data_ptr()
            keep.append(m)
        else:
            seed = int(torch.randint(0, 2 ** 62, (1,)).item())  # CPU generator: no device sync
            drop.seed_lo, drop.seed_hi = seed & 0xFFFFFFFF, seed >> 32
        if want_mask:
            out = torch.empty(shape, dtype=torch.uint8, device=dev)
            drop.mask_out = out.data_ptr()
        return drop, keep, out

    @torch.no_grad()
    def _sample(self, net, cond, deterministic, noise=None, want_mean=False, drop_mask=None, want_mask=False):
        state = cond["state"]
        hip.require_gpu(state, type(self).__name__ + ".forward")
        B, dev = state.shape[0], state.device
        AF = net.action_dim * net.horizon_steps
        obs = net.encode_obs(cond) if getattr(net, "is_vision", False) else state.reshape(B, -1).contiguous().float()
        lib, d = hip.load(), net.net_desc()
        cfg = net.gaussian_cfg(deterministic=deterministic, randn_clip=self.randn_clip_value)
        if noise is None:
            seed = int(torch.randint(0, 2 ** 62, (1,)).item())  # CPU generator: no device sync
            cfg.seed_lo, cfg.seed_hi = seed & 0xFFFFFFFF, seed >> 32
        else:
            noise = noise.reshape(B, AF).contiguous().float()
        actions = torch.empty(B, AF, device=dev)
        mean = torch.empty(B, AF, device=dev) if want_mean else None
        wsb = lib.dppo_gaussian_workspace_bytes(C.byref(d), None, self.prec, B)
        ws = self._ws_g.get(wsb, dev)
        drop, keep, mask_out = self._dropout_of(net, B, dev, drop_mask, want_mask)
        if drop is not None:  # dropout live in the trunk (IBRL's actors in train())
            hip.check(lib.dppo_gaussian_sample_drop(
                C.byref(d), self.prec, net.flat_params().data_ptr(), net.packed(self.prec, 0).data_ptr(), C.byref(cfg),
                net.logvar_ptr(), obs.data_ptr(), hip.ptr(noise), B, actions.data_ptr(), hip.ptr(mean), C.byref(drop), ws.data_ptr(),
                ws.numel(), hip.stream()), "dppo_gaussian_sample_drop")
            object.__setattr__(self, "last_drop_mask", mask_out)
            return actions.view(B, self.horizon_steps, -1), mean
        hip.check(lib.dppo_gaussian_sample(
            C.byref(d), self.prec, net.flat_params().data_ptr(), net.packed(self.prec, 0).data_ptr(), C.byref(cfg),
            net.logvar_ptr(), obs.data_ptr(), hip.ptr(noise), B, actions.data_ptr(), hip.ptr(mean), ws.data_ptr(), ws.numel(),
            hip.stream()), "dppo_gaussian_sample")
        return actions.view(B, self.horizon_steps, -1), mean

    def forward(self, cond, deterministic=False, network_override=None, reparameterize=False, get_logprob=False, noise=None,
                drop_mask=None):
        """cond {"state": (B,To,Do)} -> sampled action chunk (B,Ta,Da) (reference :94-121).  ``drop_mask`` (L, B, H) uint8 hands a
        recorded dropout mask to an actor whose dropout is live (``_dropout_of``)."""
        if get_logprob or reparameterize:
            raise NotImplementedError("dppo_amd: get_logprob / reparameterize (SAC-style use) are out of scope")
        net = network_override if network_override is not None else self.network
        return self._sample(net, cond, deterministic, noise, drop_mask=drop_mask)[0]
