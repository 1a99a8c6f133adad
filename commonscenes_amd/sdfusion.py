"""Shape-diffusion model behind the reference's `SDFusionText2ShapeModel` interface (inference side).

Mirrors model/sdfusion_txt2shape_model.py:
  __init__ (:51-132)  builds df (DiffusionUNet), the DDPM schedule, the DDIM sampler, loads the VQ-VAE
  register_schedule (:184-236), apply_model (:275-291), set_input (:238-256), rel2shape (:459-516)
Like the reference's BaseModel (model/base_model.py:31) this is a plain class, not an nn.Module
(SURVEY F11): `.df` / `.vqvae` carry their own state and are saved under 'df' / 'vqvae' keys.

Extensions over the reference (SURVEY 8b "Extension the build adds"):
  * rel2shape(..., x_T=None, mini_B=None, launch_B=None): inject the shared initial noise (the reference seeds it
    from time.time(), F7) and choose the sampler mini-batch.  `mini_B` defaults to the reference's hard-coded 7
    (sdfusion_txt2shape_model.py:493): the objects are SLICED exactly as the reference slices them.  Since r4 the
    slices are then COALESCED: with the deterministic sampler (eta = 0: no per-mini-batch noise draw) consecutive
    mini-batches are launched as one sampler run of up to `launch_B` objects (default 32 -> ceil(32 / 7) = 5
    mini-batches per launch; `model.launch_B`, CS_LAUNCH_B; 0 = one sampler run per mini-batch, the r3 behaviour).
    Objects are independent -- batch dimensions never mix -- so a coalesced launch gives every object the result of
    its own mini-batch to ~1e-5 (different GEMM tilings add in a different order; gated by
    tests/test_parity_depth_gpu.py), and the default API delivers the benchmarked 32-object throughput
    (2.6 instead of 3.3 ms per object-step on an MI355X) instead of five sequential 7-object runs.
"""
from __future__ import annotations

import logging
import os

import time
from functools import partial
from pathlib import Path
from typing import Optional

import numpy as np
import torch
import yaml

from . import dist
from . import lib as L
from . import ops
from .ddim import DDIMSampler
from .unet import DiffusionUNet
from .unet_native import NativeDiffusionUNet
from .vqvae_native import NativeVQVAE
from .vqvae import VQVAE, load_vqvae

Tensor = torch.Tensor
_log = logging.getLogger("commonscenes_amd.sdfusion")


class AttrDict(dict):
    """OmegaConf-lite: attribute access over the YAML mapping (OmegaConf is not installed here)."""

    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError as e:
            raise AttributeError(k) from e

    def __setattr__(self, k, v):
        self[k] = v


def to_attr(o):
    if isinstance(o, dict):
        return AttrDict({k: to_attr(v) for k, v in o.items()})
    if isinstance(o, list):
        return [to_attr(v) for v in o]
    return o


def load_yaml(path) -> AttrDict:
    with open(path) as f:
        return to_attr(yaml.safe_load(f))


def make_beta_schedule(schedule, n_timestep, linear_start=1e-4, linear_end=2e-2, cosine_s=8e-3) -> np.ndarray:
    """ldm_diffusion_util.py:43-65 ('linear' is what the shipped config uses)."""
    if schedule == "linear":
        betas = torch.linspace(linear_start ** 0.5, linear_end ** 0.5, n_timestep, dtype=torch.float64) ** 2
    elif schedule == "sqrt_linear":
        betas = torch.linspace(linear_start, linear_end, n_timestep, dtype=torch.float64)
    elif schedule == "sqrt":
        betas = torch.linspace(linear_start, linear_end, n_timestep, dtype=torch.float64) ** 0.5
    else:
        raise ValueError(f"schedule '{schedule}' unknown.")
    return betas.numpy()


class SDFusionText2ShapeModel:
    def __init__(self, opt, resolve_dir: Optional[Path] = None):
        """`opt`: the v2_full.yaml mapping (hyper / network / misc sections).  Relative df_cfg / vq_cfg /
        vq_ckpt paths are resolved against `resolve_dir` (default: cwd, like the reference)."""
        self.opt = opt if isinstance(opt, AttrDict) else to_attr(opt)
        self.isTrain = False
        self.model_name = self.name()
        self.device = torch.device(self.opt.hyper.device)
        if self.device.type != "cuda":
            raise RuntimeError("commonscenes_amd runs on the HIP device only (hyper.device must be 'cuda')")
        base = Path(resolve_dir) if resolve_dir else Path.cwd()
        rp = lambda p: str(p) if Path(p).is_absolute() else str(base / p)
        assert self.opt.network.df_cfg is not None and self.opt.network.vq_cfg is not None
        df_conf = load_yaml(rp(self.opt.network.df_cfg))
        vq_conf = load_yaml(rp(self.opt.network.vq_cfg))

        ddconfig = vq_conf.model.params.ddconfig                       # :68-72
        shape_res = ddconfig.resolution
        z_ch, n_down = ddconfig.z_channels, len(ddconfig.ch_mult) - 1
        z_sp = shape_res // (2 ** n_down)
        self.z_shape = (z_ch, z_sp, z_sp, z_sp)

        # two interchangeable sequencers of the same HIP kernels: the Python ones (unet.py, vqvae.py) and the native
        # whole-forward drivers (csrc/cs_unet.hip cs_unet_step, csrc/cs_vqvae.hip cs_vqvae_decode); bit-identical
        driver = str(self.opt.network.get("unet_driver") or os.environ.get("CS_UNET_DRIVER", "python"))
        if driver not in ("python", "native"):
            raise ValueError(f"unet_driver must be 'python' or 'native', got {driver!r}")
        unet_cls = NativeDiffusionUNet if driver == "native" else DiffusionUNet
        self.df = unet_cls(df_conf.unet.params, vq_conf=vq_conf,
                           conditioning_key=df_conf.model.params.conditioning_key, device=self.device)
        self.init_diffusion_params(uc_scale=3., df_model_params=df_conf.model.params)
        self.ddim_sampler = DDIMSampler(self)
        ck = self.opt.network.get("vq_ckpt")
        mp = vq_conf.model.params
        if driver == "native":
            self.vqvae = NativeVQVAE(mp.ddconfig, mp.n_embed, mp.embed_dim, device=self.device)
            if ck is not None and Path(rp(ck)).exists():
                vsd = torch.load(rp(ck), map_location="cpu")
                self.vqvae.load_state_dict(vsd["vqvae"] if "vqvae" in vsd else vsd)
        elif ck is not None and Path(rp(ck)).exists():
            self.vqvae = load_vqvae(vq_conf, rp(ck), device=str(self.device))
        else:   # weights to be supplied through load_state_dict (e.g. a full checkpoint's 'vqvae' entry)
            self.vqvae = VQVAE(mp.ddconfig, mp.n_embed, mp.embed_dim, device=self.device)
        self.df_module = self.df
        self.vqvae_module = self.vqvae
        self.ddim_steps = 100                                           # :128 (hard-coded in the reference)
        self.mini_B = int(os.environ.get("CS_MINI_B", "7"))               # :493 (hard-coded 7 in the reference)
        # objects per sampler LAUNCH: consecutive mini-batches of the deterministic sampler run as one batch (see the
        # module docstring); 0 = never coalesce
        self._launch_B = int(os.environ.get("CS_LAUNCH_B", "32"))
        self._launch_B_explicit = "CS_LAUNCH_B" in os.environ      # (rel2shape_many's fill-the-chip default)
        # which fall-backs this model has taken (sticky, like the math mode itself): `unet_fp32` / `vqvae_fp32` = an F16X3
        # operand left the fp16 range and the module continues on the fp32-input MFMA kernels (4-5x slower);
        # `splitk_two_kernel` = a fused split-K launch was not resident.  Every rel2shape* call reports a copy in `last_meta`
        # (and returns it with return_meta=True); each transition is logged at WARNING.
        self.fell_back = {"unet_fp32": False, "vqvae_fp32": False, "splitk_two_kernel": False}
        self.last_meta = None

    @property
    def launch_B(self) -> int:
        return self._launch_B

    @launch_B.setter
    def launch_B(self, v):           # an assignment is an explicit cap: rel2shape_many honours it
        self._launch_B = int(v)
        self._launch_B_explicit = True

    def name(self):
        return "SDFusion-Text2Shape-Model"

    # ---- schedule (:152-236) ----
    def init_diffusion_params(self, uc_scale=3., df_model_params=None):
        self.parameterization = "eps"
        self.learn_logvar = False                                       # :165-170
        self.v_posterior = 0.
        self.original_elbo_weight = 0.
        self.l_simple_weight = 1.
        self.register_schedule(timesteps=df_model_params.timesteps, linear_start=df_model_params.linear_start,
                               linear_end=df_model_params.linear_end)
        self.logvar = torch.full(fill_value=0., size=(self.num_timesteps,))      # :178-179
        self.uc_scale = uc_scale
        self.scale = uc_scale     # the reference reads an undefined self.scale when uc_scale=None (:474)

    def register_schedule(self, beta_schedule="linear", timesteps=1000, linear_start=1e-4, linear_end=2e-2):
        betas = make_beta_schedule(beta_schedule, timesteps, linear_start=linear_start, linear_end=linear_end)
        alphas = 1. - betas
        alphas_cumprod = np.cumprod(alphas, axis=0)
        alphas_cumprod_prev = np.append(1., alphas_cumprod[:-1])
        self.num_timesteps = int(betas.shape[0])
        self.linear_start, self.linear_end = linear_start, linear_end
        to_torch = partial(torch.tensor, dtype=torch.float32)
        # kept on the host: the sampler only ever indexes them from Python (ddim.py:31-57)
        self.betas = to_torch(betas)
        self.alphas_cumprod = to_torch(alphas_cumprod)
        self.alphas_cumprod_prev = to_torch(alphas_cumprod_prev)
        self.sqrt_alphas_cumprod = to_torch(np.sqrt(alphas_cumprod))
        self.sqrt_one_minus_alphas_cumprod = to_torch(np.sqrt(1. - alphas_cumprod))
        # :210-235, the tables p_losses and the posterior read: float64 numpy, rounded to fp32 where the reference rounds
        self.log_one_minus_alphas_cumprod = to_torch(np.log(1. - alphas_cumprod))
        self.sqrt_recip_alphas_cumprod = to_torch(np.sqrt(1. / alphas_cumprod))
        self.sqrt_recipm1_alphas_cumprod = to_torch(np.sqrt(1. / alphas_cumprod - 1))
        v_posterior = getattr(self, "v_posterior", 0.)
        posterior_variance = (1 - v_posterior) * betas * (1. - alphas_cumprod_prev) / (1. - alphas_cumprod) + v_posterior * betas
        self.posterior_variance = to_torch(posterior_variance)
        self.posterior_log_variance_clipped = to_torch(np.log(np.maximum(posterior_variance, 1e-20)))
        self.posterior_mean_coef1 = to_torch(betas * np.sqrt(alphas_cumprod_prev) / (1. - alphas_cumprod))
        self.posterior_mean_coef2 = to_torch((1. - alphas_cumprod_prev) * np.sqrt(alphas) / (1. - alphas_cumprod))
        if getattr(self, "parameterization", "eps") != "eps":
            raise NotImplementedError("only the 'eps' parameterisation is shipped")
        lvlb_weights = self.betas ** 2 / (2 * self.posterior_variance * to_torch(alphas) * (1 - self.alphas_cumprod))   # fp32 ops
        lvlb_weights[0] = lvlb_weights[1]
        self.lvlb_weights = lvlb_weights
        assert not torch.isnan(self.lvlb_weights).all()
        self._dev_tables = {}         # device copies of the two tables cs_q_sample indexes, made on first use

    # ---- reference surface ----
    def set_input(self, input=None, max_sample=None):
        self.x = input["sdf"]
        self.rel = input["rel"]
        self.uc_rel = input["uc"]
        if self.df.conditioning_key == "concat":                        # :246-248: the condition is a volume
            B = self.rel.shape[0]
            C_, D, H, W = self.z_shape
            self.rel = self.rel.reshape(B, -1, D, H, W)
            self.uc_rel = self.uc_rel.reshape(B, -1, D, H, W)
        if max_sample is not None:
            self.x, self.rel, self.uc_rel = self.x[:max_sample], self.rel[:max_sample], self.uc_rel[:max_sample]

    def switch_eval(self):
        self.df.eval()
        self.vqvae.eval()

    def switch_train(self):
        raise NotImplementedError("training is out of scope (SURVEY 3.4)")

    def apply_model(self, x_noisy, t, cond, return_ids=False):
        """:275-291"""
        if isinstance(cond, dict):
            return self.df(x_noisy, t, **cond)
        if not isinstance(cond, list):
            cond = [cond]
        key = "c_concat" if self.df_module.conditioning_key == "concat" else "c_crossattn"
        return self.df(x_noisy, t, **{key: cond})

    def apply_model_cfg(self, x, t, c_in):
        """[eps_uc; eps_c] for the guidance pair batch (ddim.py:206-209) without duplicating (x, t)."""
        return self.df.forward_cfg(x, t, c_in)

    # ---- training-time losses, forward only (:268-345) --------------------------------------------------------------
    def _q_tables(self):
        dev = torch.device(self.device)
        key = (dev.type, dev.index if dev.index is not None else torch.cuda.current_device())
        tb = self._dev_tables.get(key)
        if tb is None:
            tb = self._dev_tables[key] = (self.sqrt_alphas_cumprod.to(dev).contiguous(),
                                          self.sqrt_one_minus_alphas_cumprod.to(dev).contiguous())
        return tb

    def _t_dev(self, t) -> Tensor:
        return torch.as_tensor(t, dtype=torch.int64).to(self.device).reshape(-1)

    @torch.no_grad()
    def q_sample(self, x_start, t, noise=None, src=None, nsrc=None):
        """:268-272: sqrt_alphas_cumprod[t] * x_start + sqrt_one_minus_alphas_cumprod[t] * noise with a per-sample timestep,
        one cs_q_sample launch (the reference's three roundings per element).  Extension: `src` / `nsrc` int32 row maps."""
        x_start = x_start.to(device=self.device, dtype=torch.float32)
        if noise is None:
            noise = torch.randn_like(x_start)
        sa, s1 = self._q_tables()
        return ops.q_sample(x_start, noise.to(device=self.device, dtype=torch.float32), self._t_dev(t), sa, s1, src, nsrc)

    @torch.no_grad()
    def get_loss(self, pred, target, loss_type='l2', mean=True):
        """:293-306, value only.  mean=True: the fp32 scalar of F.mse_loss / (target - pred).abs().mean().  mean=False: the
        reference returns the element-wise map, and its one caller reduces it with .mean([1, 2, 3, 4]) at once (:328, :339);
        here that per-sample mean is returned directly, fp32 [B].  Either way one cs_pair_stats launch: fp64 sums in a fixed
        order, divided once and rounded to fp32 once."""
        if loss_type not in ('l1', 'l2'):
            raise NotImplementedError(f"unknown loss type '{loss_type}'")
        pred = pred.to(device=self.device, dtype=torch.float32)
        target = target.to(device=self.device, dtype=torch.float32)
        sums, _ = ops.pair_stats(target, pred)
        col = sums[:, 0 if loss_type == 'l2' else 1]
        per = pred.numel() // pred.shape[0]
        if mean:
            return (col.sum() / float(pred.numel())).to(torch.float32)
        return (col / float(per)).to(torch.float32)

    def _loss_dict(self, loss_simple: Tensor, t: Tensor):
        """:328-343 from the per-sample loss_simple [B] (fp32) on: a handful of fp32 operations over B numbers, evaluated on the
        host in the reference's order (the schedule tables live there)."""
        ls = loss_simple.detach().to("cpu", torch.float32)
        tc = t.detach().to("cpu")
        loss_dict = {"loss_simple": ls.mean()}
        logvar_t = self.logvar[tc]
        loss = ls / torch.exp(logvar_t) + logvar_t
        if self.learn_logvar:
            raise NotImplementedError("learn_logvar is not shipped")
        loss = self.l_simple_weight * loss.mean()
        loss_vlb = (self.lvlb_weights[tc] * ls).mean()
        loss_dict["loss_vlb"] = loss_vlb
        loss = loss + self.original_elbo_weight * loss_vlb
        loss_dict["loss_total"] = loss.clone().detach().mean()
        return loss.to(self.device), {k: v.to(self.device) for k, v in loss_dict.items()}

    @torch.no_grad()
    def p_losses(self, x_start, cond, t, noise=None):
        """:311-345, forward only: (x_noisy, target, loss, loss_dict) with loss_simple / loss_vlb / loss_total as fp32 0-dim
        tensors.  x_start is the latent [B, 3, 16, 16, 16], t int64 [B]."""
        if self.parameterization != "eps":
            raise NotImplementedError("only the 'eps' parameterisation is shipped")
        self.switch_eval()
        x_start = x_start.to(device=self.device, dtype=torch.float32)
        if noise is None:
            noise = torch.randn_like(x_start)
        noise = noise.to(device=self.device, dtype=torch.float32)
        t = self._t_dev(t)
        x_noisy = self.q_sample(x_start=x_start, t=t, noise=noise)
        model_output = self._apply_checked(x_noisy, t, cond)
        self.last_model_output = model_output
        target = noise
        loss_simple = self.get_loss(model_output, target, mean=False)
        loss, loss_dict = self._loss_dict(loss_simple, t)
        return x_noisy, target, loss, loss_dict

    def _apply_checked(self, x_noisy, t, cond):
        """apply_model under the F16X3 overflow policy of the samplers (see _sample_minibatch)."""
        def run():
            if hasattr(self.df, "reset_run_cache"):
                self.df.reset_run_cache()
            ops.clear_status(self.device)
            out = self.apply_model(x_noisy, t, cond)
            ops.check_overflow(self.device, "denoising loss (UNet)")
            return out
        try:
            try:
                return run()
            except L.CsSplitKTimeout as e:
                _log.warning("fused split-K reduce timed out: re-running with no_fused_reduce=1 (%s)", e)
                L.debug_set(no_fused_reduce=1)
                self.fell_back["splitk_two_kernel"] = True
                return run()
        except L.CsOverflowError:
            if self.overflow_policy != "fp32" or getattr(self.df, "math", None) != L.MATH_F16X3:
                raise
            _log.warning("F16X3 activation overflow in the UNet: this model continues on the fp32-input MFMA kernels")
            self.df.set_math("fp32")
            self._df_fell_back = True
            self.fell_back["unet_fp32"] = True
            return run()

    @torch.no_grad()
    def denoising_loss_table(self, x, c, timesteps, noise=None, seed=None, batch=64, encoded=False, return_meta=False):
        """Extension (ours, not in the reference): the training loss of a held-out set at fixed timesteps.

        x: [N, 1, 64, 64, 64] SDFs, encoded with vqvae.encode_no_quant (raises when the checkpoint has no encoder), or with
        encoded=True the latents [N, 3, 16, 16, 16].  c: the condition of each shape, per the conditioning key.  Every shape is
        evaluated at every entry of `timesteps` (K of them): row k * N + n of the sweep is shape n at timesteps[k], noised by
        cs_q_sample through row maps (the latents are never repeated) and run through the UNet in launches of at most
        `batch` rows.  noise: [N, ...] shared over the timesteps, [N, K, ...] one per cell, or None = drawn from a device
        generator seeded with `seed` (None: the clock, like the reference's sampling).
        Returns {'per_sample': fp64 [N, K] per-shape loss_simple, 'loss_simple': fp32 [K], 'loss_vlb': fp32 [K], 'timesteps':
        int64 [K], 'fell_back': ...}: column k holds what p_losses reports for all N shapes at t = timesteps[k]."""
        if self.parameterization != "eps":
            raise NotImplementedError("only the 'eps' parameterisation is shipped")
        self.switch_eval()
        ts = torch.as_tensor(timesteps, dtype=torch.int64).reshape(-1).cpu()
        K = int(ts.numel())
        if K == 0 or int(ts.min()) < 0 or int(ts.max()) >= self.num_timesteps:
            raise ValueError(f"timesteps must be a non-empty list inside [0, {self.num_timesteps})")
        if int(batch) < 1:
            raise ValueError("batch must be at least 1")
        x = x.to(device=self.device, dtype=torch.float32)
        if encoded:
            z = x.contiguous()
        else:
            if not getattr(self.vqvae, "has_encoder", False):
                raise RuntimeError("denoising_loss_table: the VQ-VAE checkpoint has no encoder (encoder.* / quant_conv.*); "
                                   "pass latents with encoded=True")
            z = self.vqvae.encode_no_quant(x)
        N = int(z.shape[0])
        if tuple(z.shape[1:]) != tuple(self.z_shape) or N == 0:
            raise ValueError(f"latents {tuple(z.shape)} do not match the model's {self.z_shape}")
        c = c.to(device=self.device, dtype=torch.float32)
        if self.df.conditioning_key == "concat":
            c = c.reshape(N, -1, *self.z_shape[1:])
        if c.shape[0] != N:
            raise ValueError(f"{N} shapes but {c.shape[0]} conditions")
        if noise is None:
            g = torch.Generator(device=self.device)
            g.manual_seed(int(time.time()) if seed is None else int(seed))
            noise = torch.randn((N, K, *self.z_shape), generator=g, device=self.device, dtype=torch.float32)
        noise = noise.to(device=self.device, dtype=torch.float32)
        if tuple(noise.shape) == (N, *self.z_shape):
            per_cell = False
        elif tuple(noise.shape) == (N, K, *self.z_shape):
            per_cell = True
        else:
            raise ValueError(f"noise {tuple(noise.shape)}: expected [N, ...] or [N, K, ...] with N = {N}, K = {K}")
        nz = noise.reshape(-1, *self.z_shape).contiguous()
        rows = N * K
        r = torch.arange(rows)
        n_of, k_of = r % N, r // N
        src_all = n_of.to(torch.int32).to(self.device)
        nsrc_all = (n_of * K + k_of if per_cell else n_of).to(torch.int32).to(self.device)
        t_all = ts[k_of].to(self.device)
        sa, s1 = self._q_tables()
        per = z.numel() // N
        means = torch.empty((rows,), dtype=torch.float64, device=self.device)
        for lo in range(0, rows, int(batch)):
            hi = min(rows, lo + int(batch))
            x_noisy = ops.q_sample(z, nz, t_all[lo:hi], sa, s1, src_all[lo:hi], nsrc_all[lo:hi])
            eps = self._apply_checked(x_noisy, t_all[lo:hi], c[src_all[lo:hi].long()])
            target = nz[nsrc_all[lo:hi].long()]
            sums, _ = ops.pair_stats(target, eps)
            means[lo:hi] = sums[:, 0] / float(per)
        m = means.cpu().reshape(K, N)
        ls = m.to(torch.float32)                     # p_losses' per-sample loss_simple: the fp64 mean rounded once
        # (row by row, the very reductions of _loss_dict: column k is bit for bit what p_losses reports at timesteps[k])
        out = {"per_sample": m.t().contiguous(), "loss_simple": torch.stack([ls[k].mean() for k in range(K)]),
               "loss_vlb": torch.stack([(self.lvlb_weights[ts[k].expand(N)] * ls[k]).mean() for k in range(K)]),
               "timesteps": ts.clone(),
               "fell_back": dict(self.fell_back), "any_fell_back": any(self.fell_back.values())}
        self.last_meta = {"fell_back": dict(self.fell_back), "any_fell_back": any(self.fell_back.values()),
                          "launch_sizes": [min(int(batch), rows - lo) for lo in range(0, rows, int(batch))]}
        return (out, self.last_meta) if return_meta else out

    # ---- F16X3 overflow policy -------------------------------------------------------------------------------------
    # CS_MATH_F16X3 carries activations as fp16 pairs of a * 16: |a| >= ~4094 cannot be represented.  Every F16X3
    # kernel reports that in a sticky device word (CS_STATUS_F16X3_OVERFLOW); it is read back ONCE per sampler run /
    # decode.  'fp32' (default): re-run that mini-batch on the fp32-input MFMA kernels and stay there;
    # 'raise': propagate CsOverflowError.
    overflow_policy = os.environ.get("CS_OVERFLOW_POLICY", "fp32")

    def _sample_minibatch(self, sampler, ddim_steps, shape, c, uc, noise, uc_scale, ddim_eta, max_steps, **sample_kw):
        """`sample_kw`: further sampler.sample arguments of this run (shape_comp: mask, x0, q_noise and the row maps)."""
        def run():
            if hasattr(self.df, "reset_run_cache"):
                self.df.reset_run_cache()           # per-run caches (one-token context vectors) never outlive a run
            # the status word is sticky per device: clear what earlier, unchecked F16X3 launches (a direct decode, a
            # bench loop, a call that raised before its own check) may have left, so only THIS run is attributed.
            # Stream-ordered clear, no read-back: the one host sync per run is check_overflow's below.
            ops.clear_status(self.device)
            out, _ = sampler.sample(S=ddim_steps, batch_size=c.shape[0], shape=shape, conditioning=c, x_T=noise,
                                    verbose=False, unconditional_guidance_scale=uc_scale,
                                    unconditional_conditioning=uc, eta=ddim_eta, max_steps=max_steps, **sample_kw)
            ops.check_overflow(self.device, "DDIM sampling (UNet)")
            return out
        try:
            try:
                return run()
            except L.CsSplitKTimeout as e:
                # a fused split-K launch was not resident (CUs held by another stream / a CU mask): same arithmetic on the
                # two-kernel form, which needs no co-residency -- for the rest of the process
                import warnings
                warnings.warn(f"{e}; re-running with the two-kernel split-K")
                _log.warning("fused split-K reduce timed out: re-running this mini-batch with no_fused_reduce=1")
                L.debug_set(no_fused_reduce=1)
                self.fell_back["splitk_two_kernel"] = True
                return run()
        except L.CsOverflowError:
            if self.overflow_policy != "fp32" or getattr(self.df, "math", None) != L.MATH_F16X3:
                raise
            import warnings
            warnings.warn("F16X3 activation overflow in the UNet: re-running this mini-batch (and continuing) on the "
                          "fp32-input MFMA kernels (set_math('fp32'))")
            _log.warning("F16X3 activation overflow in the UNet: this model continues on the fp32-input MFMA kernels "
                         "(~4-5x slower); tools/check_checkpoint.py prints the per-layer bounds of a checkpoint")
            self.df.set_math("fp32")
            self._df_fell_back = True
            self.fell_back["unet_fp32"] = True
            return run()

    def _decode_checked(self, samples):
        ops.clear_status(self.device)               # see _sample_minibatch: attribute only this decode's kernels
        out = self.vqvae_module.decode_no_quant(samples)
        try:
            try:
                ops.check_overflow(self.device, "VQ-VAE decode")
            except L.CsSplitKTimeout as e:              # see _sample_minibatch
                _log.warning("fused split-K reduce timed out in the VQ-VAE decode: re-running with no_fused_reduce=1 (%s)", e)
                L.debug_set(no_fused_reduce=1)
                self.fell_back["splitk_two_kernel"] = True
                ops.clear_status(self.device)
                out = self.vqvae_module.decode_no_quant(samples)
                ops.check_overflow(self.device, "VQ-VAE decode")
        except L.CsOverflowError:
            if (self.overflow_policy != "fp32" or getattr(self.vqvae, "math", None) != L.MATH_F16X3
                    or not hasattr(self.vqvae, "set_math")):
                raise
            import warnings
            warnings.warn("F16X3 activation overflow in the VQ-VAE decoder: re-running on the fp32-input MFMA kernels")
            _log.warning("F16X3 activation overflow in the VQ-VAE decoder: this model continues on the fp32-input MFMA kernels")
            self.vqvae.set_math("fp32")
            self._vq_fell_back = True
            self.fell_back["vqvae_fp32"] = True
            out = self.vqvae_module.decode_no_quant(samples)
        return out

    def _sync_math_across_ranks(self):
        """Sharded runs: the fp32 fall-back is decided per rank (only the rank whose shard overflowed switches), which
        would leave the ranks on different numerics for every later call -- shards then stop matching the single-rank
        run bit for bit.  One tiny all-reduce after the shard is done: if ANY rank fell back, all do."""
        # (explicit fell-back flags, set where the fall-back is taken: a module without a `math` attribute, or one that
        # was STARTED in fp32 (CS_MATH=fp32), must not read as "fell back" and drag its peers to fp32 -- ADVICE r3)
        flags = torch.tensor([float(bool(getattr(self, "_df_fell_back", False))),
                              float(bool(getattr(self, "_vq_fell_back", False)))], device=self.device)
        flags = dist.all_reduce_max(flags)
        if flags[0] > 0 and getattr(self.df, "math", None) == L.MATH_F16X3:
            _log.warning("another rank's UNet fell back to fp32: this rank follows (all ranks stay on the same numerics)")
            self.df.set_math("fp32")
            self._df_fell_back = True
            self.fell_back["unet_fp32"] = True
        if flags[1] > 0 and getattr(self.vqvae, "math", None) == L.MATH_F16X3 and hasattr(self.vqvae, "set_math"):
            _log.warning("another rank's VQ-VAE decoder fell back to fp32: this rank follows")
            self.vqvae.set_math("fp32")
            self._vq_fell_back = True
            self.fell_back["vqvae_fp32"] = True

    def _launch_slices(self, lo: int, hi: int, mini_B: Optional[int], launch_B: Optional[int], ddim_eta: float):
        """The sampler launches over objects [lo, hi).  :493-511 slices the objects into ceil(B / 7) mini-batches and runs
        the sampler once per slice.  Every object starts from its scene's x_T and the batch dimension never mixes, so with
        eta = 0 (no noise draw inside the loop) the slices are independent of how they are grouped: WHOLE mini-batches
        are coalesced into launches.  launch_B counts objects and is rounded UP to whole mini-batches (launch_B = 32,
        mini_B = 7: up to five slices = 35 objects per launch -- a cap on memory should be given as a multiple of
        mini_B); the mini-batches are then dealt EVENLY over the fewest launches that respects it, so 40 objects run as
        21 + 19, not as 35 + 5 with an inefficient tail launch.  eta > 0 keeps one launch per slice: the
        sampler draws one noise tensor per slice and step (ddim.py:240), which grouping would re-order."""
        mb = max(1, int(mini_B or self.mini_B))
        lb = int(self.launch_B if launch_B is None else launch_B)
        n = hi - lo
        if n <= 0:
            return []
        n_mb = -(-n // mb)
        per = -(-lb // mb) if (lb > mb and float(ddim_eta) == 0.0) else 1
        n_launch = -(-n_mb // per)
        base, extra = divmod(n_mb, n_launch)
        out, i = [], lo
        for k in range(n_launch):
            cnt = (base + (1 if k < extra else 0)) * mb
            out.append(slice(i, min(i + cnt, hi)))
            i += cnt
        return out

    @torch.no_grad()
    def rel2shape_many(self, datas, ddim_steps=100, ddim_eta=0.0, uc_scale=None, x_Ts=None, mini_B: Optional[int] = None,
                       return_latents: bool = False, max_steps: Optional[int] = None, sampler: str = "ddim",
                       launch_B: Optional[int] = None, return_meta: bool = False):
        """Extension: rel2shape for SEVERAL scenes in one coalesced sampler + decode.
        Single-rank only (it has no object sharding: under torch.distributed with more than one rank it raises -- call
        rel2shape per scene there); `launch_B=None` = model.launch_B when that was set explicitly (attribute / CS_LAUNCH_B),
        else the fill-the-chip default of 64 objects per launch.

        The reference's evaluation loop calls rel2shape once per scene (scripts/eval_3dfront.py:484-513 ->
        VAEGAN_V2FULL.py:600-618 -> sdfusion_txt2shape_model.py:459-516) with 5-15 shaped objects each: small batches, the
        regime furthest from the roofline.  Objects never mix along the batch dimension (GroupNorm / LayerNorm /
        attention are per sample), so the scenes' objects are concatenated and sampled together; what is kept per scene is
        its SHARED x_T (:489-491: one noise volume repeated over the scene's objects) -- x_Ts[i] (or a fresh time-seeded
        draw per scene) is repeated over scene i's objects only.  Returns a list of per-scene gen_df (and latents).
        Per-object results equal the per-scene call bit for bit whenever the GEMM plan is the same (the plan depends on
        the launch's object count), within fp32 summation order otherwise.  Deterministic samplers only (eta = 0)."""
        if float(ddim_eta) != 0.0:
            raise ValueError("rel2shape_many coalesces scenes: deterministic sampling (ddim_eta = 0) only")
        if dist.world()[1] > 1:
            raise RuntimeError("rel2shape_many is single-rank (no object sharding / rank-failure agreement): call "
                               "rel2shape(sharded=True) per scene under torch.distributed")
        if x_Ts is not None and len(x_Ts) != len(datas):
            raise ValueError(f"rel2shape_many: {len(datas)} scenes but {len(x_Ts)} x_Ts (one per scene, or None)")
        self.switch_eval()
        if sampler == "ddim":
            smp = DDIMSampler(self)
        elif sampler == "plms":
            from .plms import PLMSSampler
            smp = PLMSSampler(self)
        else:
            raise ValueError(f"sampler must be 'ddim' or 'plms', got {sampler!r}")
        if ddim_steps is None:
            ddim_steps = self.ddim_steps
        if uc_scale is None:
            uc_scale = self.scale
        shape = self.z_shape
        C_, D, H, W = shape
        counts, cs, ucs, noises = [], [], [], []
        for i, data in enumerate(datas):
            self.set_input(data)
            c_i = self.rel.to(device=self.device, dtype=torch.float32)
            cs.append(c_i)
            ucs.append(self.uc_rel.to(device=self.device, dtype=torch.float32))
            counts.append(int(c_i.shape[0]))
            if x_Ts is None or x_Ts[i] is None:
                torch.manual_seed(int(time.time()) + i)                  # :489 (time-seeded in the reference), per scene
                n_i = torch.randn((1, C_, D, H, W), device=self.device)
            else:
                n_i = x_Ts[i].to(device=self.device, dtype=torch.float32).reshape(1, C_, D, H, W)
            noises.append(n_i.expand(counts[-1], C_, D, H, W))
        total = sum(counts)
        r = self.vqvae.cfg["resolution"] if hasattr(self.vqvae, "cfg") else 64
        och = self.vqvae.cfg.get("out_ch", 1) if hasattr(self.vqvae, "cfg") else 1
        self.last_launch_sizes = []
        if total == 0:
            gens = [torch.empty((0, och, r, r, r), dtype=torch.float32, device=self.device) for _ in counts]
            lat = [torch.empty((0, C_, D, H, W), dtype=torch.float32, device=self.device) for _ in counts]
            return (gens, lat) if return_latents else gens
        c_all, uc_all = torch.cat(cs, dim=0), torch.cat(ucs, dim=0)
        noise_all = torch.cat(noises, dim=0).contiguous()
        gen, lats = [], []
        if launch_B is None:
            # scenes are batched to fill the chip (up to 64 objects per launch) -- unless the operator capped launch_B
            # (memory): an explicit attribute / CS_LAUNCH_B is honoured, never silently raised
            launch_B = int(self.launch_B) if self._launch_B_explicit else 64
        for sl in self._launch_slices(0, total, mini_B, launch_B, ddim_eta):
            self.last_launch_sizes.append(sl.stop - sl.start)
            samples = self._sample_minibatch(smp, ddim_steps, shape, c_all[sl], uc_all[sl], noise_all[sl].contiguous(),
                                             uc_scale, ddim_eta, max_steps)
            lats.append(samples)
            gen.append(self._decode_checked(samples))
        g_all, l_all = torch.cat(gen, dim=0), torch.cat(lats, dim=0)
        gens = list(torch.split(g_all, counts, dim=0))
        lat = list(torch.split(l_all, counts, dim=0))
        self.last_latents, self.gen_df = l_all, g_all
        meta = self._meta(ddim_steps, sampler)
        out = (gens, lat) if return_latents else gens
        if return_meta:
            return (*out, meta) if return_latents else (out, meta)
        return out

    def _meta(self, ddim_steps, sampler):
        """what the last rel2shape* call ran as: kept in `last_meta`, returned with return_meta=True."""
        self.last_meta = {"fell_back": dict(self.fell_back), "any_fell_back": any(self.fell_back.values()),
                          "launch_sizes": list(self.last_launch_sizes), "ddim_steps": int(ddim_steps), "sampler": sampler,
                          "unet_math": {L.MATH_FP32: "fp32", L.MATH_F16X3: "f16x3"}.get(getattr(self.df, "math", None)),
                          "vqvae_math": {L.MATH_FP32: "fp32", L.MATH_F16X3: "f16x3"}.get(getattr(self.vqvae, "math", None))}
        return self.last_meta

    @torch.no_grad()
    def rel2shape(self, data, ddim_steps=100, ddim_eta=0.0, uc_scale=None, x_T: Optional[Tensor] = None,
                  mini_B: Optional[int] = None, return_latents: bool = False, max_steps: Optional[int] = None,
                  sharded: Optional[bool] = None, sampler: str = "ddim", launch_B: Optional[int] = None,
                  return_meta: bool = False):
        """:459-516.  data = {'sdf': (B,...) only its batch size is used, 'rel': (B,1,1280), 'uc': (B,1,1280)}.
        `return_meta=True` appends a dict (also kept as `self.last_meta`): `fell_back` (which fall-backs this model has taken:
        fp32 re-runs after an F16X3 range overflow, the two-kernel split-K), the launch sizes, the math modes.

        Extensions: `x_T` injection (the reference seeds from the clock), `mini_B` (reference: 7),
        `launch_B` (objects per sampler launch: consecutive mini-batches of the deterministic sampler are coalesced, see
        the module docstring; None = self.launch_B, 0 = one launch per mini-batch as in the reference),
        `sampler` ('ddim' | 'plms', samplers/plms.py), and `sharded`: with torch.distributed initialised (one process
        per GPU, RCCL) the objects are split contiguously over the ranks -- rank 0's (x_T, uc, c) is broadcast once,
        every rank samples + decodes its shard, one all-gather returns ALL objects on every rank.  No per-step
        collective.  Default (None): shard iff a process group with more than one rank exists and CS_SHARD != 0."""
        self.switch_eval()
        self.set_input(data)
        if sampler == "ddim":
            smp = DDIMSampler(self)
        elif sampler == "plms":
            from .plms import PLMSSampler
            smp = PLMSSampler(self)
        else:
            raise ValueError(f"sampler must be 'ddim' or 'plms', got {sampler!r}")
        if ddim_steps is None:
            ddim_steps = self.ddim_steps
        if uc_scale is None:
            uc_scale = self.scale
        uc = self.uc_rel.to(device=self.device, dtype=torch.float32)
        c_text = self.rel.to(device=self.device, dtype=torch.float32)
        B = c_text.shape[0]
        shape = self.z_shape
        C_, D, H, W = shape
        if x_T is None:
            torch.manual_seed(int(time.time()))                          # :489 (time-seeded in the reference)
            single_noise = torch.randn((1, C_, D, H, W), device=self.device)
        else:
            single_noise = x_T.to(device=self.device, dtype=torch.float32).reshape(1, C_, D, H, W)
        rank, ws = dist.world()
        if sharded is None:
            sharded = ws > 1 and os.environ.get("CS_SHARD", "1") != "0"
        multi = ws > 1 or dist._force()     # (_force: test-only, drives the collectives through a one-rank RCCL group)
        lo, hi = 0, B
        if sharded and multi:
            # one broadcast of the packed [x_T | uc | c] buffer: every rank then holds rank 0's bits (x_T is
            # time-seeded, and the GCN that produced uc / c ran on every rank or only on rank 0 -- either way)
            single_noise, uc, c_text = dist.broadcast_conditioning(
                single_noise, uc, c_text, B, self.device, src=0, latent_shape=shape,
                ctx_dim=int(c_text[0].numel()) if B else 0, cond_shape=tuple(c_text.shape[1:]))
            lo, hi = dist.shard_range(B, ws, rank)
        r = self.vqvae.cfg["resolution"] if hasattr(self.vqvae, "cfg") else 64
        och = self.vqvae.cfg.get("out_ch", 1) if hasattr(self.vqvae, "cfg") else 1
        self.last_launch_sizes = []
        gen, lats = [], []
        failure: Optional[BaseException] = None
        try:
            for sl in self._launch_slices(lo, hi, mini_B, launch_B, ddim_eta):
                self.last_launch_sizes.append(sl.stop - sl.start)
                num = sl.stop - sl.start
                noise = single_noise.repeat(num, 1, 1, 1, 1)             # every object shares one x_T (:491)
                samples = self._sample_minibatch(smp, ddim_steps, shape, c_text[sl], uc[sl], noise, uc_scale, ddim_eta,
                                                 max_steps)
                lats.append(samples)
                gen.append(self._decode_checked(samples))
        except Exception as e:              # noqa: BLE001 -- re-raised below, after the other ranks have been told
            if not (sharded and multi):
                raise
            failure = e
        if sharded and multi:
            # a rank that raised must not leave its peers blocked in the all-gather: agree on failure first
            bad = dist.any_rank_failed(failure is not None, self.device)
            if failure is not None:
                raise failure
            if bad:
                raise RuntimeError("rel2shape: another rank failed while sampling its shard (see its traceback); "
                                   "no SDFs were gathered")
            self._sync_math_across_ranks()
        if gen:
            local, llat = torch.cat(gen, dim=0), torch.cat(lats, dim=0)
        else:       # an empty shard (more ranks than objects) or B == 0: nothing to sample, still join the gather
            local = torch.empty((0, och, r, r, r), dtype=torch.float32, device=self.device)
            llat = torch.empty((0, C_, D, H, W), dtype=torch.float32, device=self.device)
        if sharded and multi:
            local = dist.all_gather_objects(local, B)
            if return_latents:
                llat = dist.all_gather_objects(llat, B)
        self.last_latents = llat            # this rank's (or, with return_latents, all) sampled latents: diagnostics
        self.gen_df = local
        meta = self._meta(ddim_steps, sampler)
        if return_latents:
            return (self.gen_df, llat, meta) if return_meta else (self.gen_df, llat)
        return (self.gen_df, meta) if return_meta else self.gen_df

    # ---- shape completion (sdfusion_model.py:399-446, on the conditioned model) -----------------------------------------------
    def _encode_checked(self, x):
        """vqvae.encode_no_quant under the overflow policy of _decode_checked (raises when the checkpoint has no encoder)."""
        ops.clear_status(self.device)
        z = self.vqvae_module.encode_no_quant(x)
        try:
            ops.check_overflow(self.device, "VQ-VAE encode")
        except L.CsOverflowError:
            if (self.overflow_policy != "fp32" or getattr(self.vqvae, "math", None) != L.MATH_F16X3
                    or not hasattr(self.vqvae, "set_math")):
                raise
            _log.warning("F16X3 activation overflow in the VQ-VAE encoder: this model continues on the fp32-input MFMA kernels")
            self.vqvae.set_math("fp32")
            self._vq_fell_back = True
            self.fell_back["vqvae_fp32"] = True
            z = self.vqvae_module.encode_no_quant(x)
        return z

    @torch.no_grad()
    def shape_comp(self, shape, xyz_dict, cond, uc=None, ngen=1, ddim_steps=100, ddim_eta=0.0, uc_scale=None,
                   x_T: Optional[Tensor] = None, q_noise: Optional[Tensor] = None, return_latents: bool = False,
                   return_meta: bool = False):
        """Shape completion: keep what lies inside the box `xyz_dict` of each SDF, generate the rest under that object's
        condition.  The reference has this on its unconditional model (sdfusion_model.py:399-446: encode, get_partial_shape,
        DDIMSampler.sample(x0=z, mask=z_mask), decode_no_quant); here it runs with the object's scene-graph condition and
        classifier-free guidance, as rel2shape does.

        shape: [N, 1, 64, 64, 64] SDFs (a 4-d input gains a batch axis).  cond / uc: what rel2shape hands the sampler for
        those N objects (crossattn [N, 1, 1280], or the concat volume); uc=None = the unconditional embedding of the last
        set_input (`self.uc_rel`).  ngen completions per object.  x_T: [N * ngen, C, d, h, w] start noise (None: drawn
        fresh per row, as the reference's sampler does); q_noise: [steps, N * ngen, C, d, h, w], the q_sample noise of every
        step (None: drawn on the device once per step).  Returns [N * ngen, 1, 64, 64, 64] SDFs, object-major (rows
        n * ngen .. n * ngen + ngen - 1 belong to object n), and sets self.x_part / self.x_missing (visualisation).
        The known region is re-noised before every step and not after the last one, so in the result it is what the last
        step made of q_sample(x0, t_min): close to the input there, not equal to it (the reference's behaviour).
        Rows run in sampler launches of at most `launch_B`; the ngen rows of an object read its latent and mask through row
        maps.  With q_noise and x_T given, a row's result does not depend on how the rows were sliced (bit for bit when the
        GEMM plan of the launch is the same, within fp32 summation order otherwise).  Single-rank."""
        if dist.world()[1] > 1:
            raise RuntimeError("shape_comp is single-rank (no object sharding): call it on one rank under torch.distributed")
        ngen = int(ngen)
        if ngen < 1:
            raise ValueError("ngen must be at least 1")
        self.switch_eval()
        if ddim_steps is None:
            ddim_steps = self.ddim_steps
        if uc_scale is None:
            uc_scale = self.scale
        if shape.dim() == 4:
            shape = shape.unsqueeze(0)
        shape = shape.to(device=self.device, dtype=torch.float32)
        from .demo_util import get_partial_shape
        z = self._encode_checked(shape)
        N = int(z.shape[0])
        if tuple(z.shape[1:]) != tuple(self.z_shape) or N == 0:
            raise ValueError(f"latents {tuple(z.shape)} do not match the model's {self.z_shape}")
        ret = get_partial_shape(shape, xyz_dict=xyz_dict, z=z)
        z_mask = ret["z_mask"]
        self.x_part, self.x_missing = ret["shape_part"], ret["shape_missing"]
        C_, D, H, W = self.z_shape
        cond = cond.to(device=self.device, dtype=torch.float32)
        if uc is None:
            uc = getattr(self, "uc_rel", None)
            if uc is None:
                raise ValueError("shape_comp: uc=None needs the unconditional embedding of an earlier set_input (uc_rel)")
        uc = uc.to(device=self.device, dtype=torch.float32)
        if self.df.conditioning_key == "concat":
            cond, uc = cond.reshape(cond.shape[0], -1, D, H, W), uc.reshape(uc.shape[0], -1, D, H, W)
        if cond.shape[0] != N or uc.shape[0] != N:
            raise ValueError(f"{N} shapes but {cond.shape[0]} conditions / {uc.shape[0]} unconditional embeddings")
        rows = N * ngen
        obj = torch.arange(rows) // ngen                                  # object-major: row r completes object r // ngen
        if x_T is not None:
            x_T = x_T.to(device=self.device, dtype=torch.float32)
            if tuple(x_T.shape) != (rows, C_, D, H, W):
                raise ValueError(f"x_T {tuple(x_T.shape)}: expected {(rows, C_, D, H, W)}")
        smp = DDIMSampler(self)
        smp.make_schedule(ddim_num_steps=ddim_steps, ddim_eta=ddim_eta, verbose=False)
        n_steps = int(smp.ddim_timesteps.shape[0])
        if q_noise is not None:
            q_noise = q_noise.to(device=self.device, dtype=torch.float32)
            if tuple(q_noise.shape) != (n_steps, rows, C_, D, H, W):
                raise ValueError(f"q_noise {tuple(q_noise.shape)}: expected {(n_steps, rows, C_, D, H, W)}")
        lb = int(self.launch_B) if int(self.launch_B) > 0 else max(1, int(self.mini_B))      # (0: the reference's mini-batch)
        self.last_launch_sizes = []
        gen, lats = [], []
        for lo in range(0, rows, lb):
            hi = min(rows, lo + lb)
            self.last_launch_sizes.append(hi - lo)
            o = obj[lo:hi]
            src = o.to(torch.int32)
            samples = self._sample_minibatch(
                smp, ddim_steps, self.z_shape, cond[o.to(self.device)], uc[o.to(self.device)],
                None if x_T is None else x_T[lo:hi].contiguous(), uc_scale, ddim_eta, None,
                mask=z_mask, x0=z, x0_src=src, mask_src=src,
                q_noise=None if q_noise is None else q_noise[:, lo:hi].contiguous())
            lats.append(samples)
            gen.append(self._decode_checked(samples))
        self.last_latents, self.gen_df = torch.cat(lats, dim=0), torch.cat(gen, dim=0)
        meta = self._meta(ddim_steps, "ddim")
        meta["ngen"], meta["masked_steps"] = ngen, n_steps
        out = (self.gen_df, self.last_latents) if return_latents else self.gen_df
        if return_meta:
            return (*out, meta) if return_latents else (out, meta)
        return out

    # ---- the other callers of the same sampler (sdfusion_txt2shape_model.py:368-457) -----------------------------------
    # The reference runs these over ALL objects in one sampler call (no mini-batching) with fresh noise per object
    # (DDIMSampler draws torch.randn when x_T is None); same here, plus the x_T / max_steps injection of rel2shape.
    def _sample_all(self, c, uc, ddim_steps, ddim_eta, uc_scale, x_T=None, max_steps=None):
        if ddim_steps is None:
            ddim_steps = self.ddim_steps
        if uc_scale is None:
            uc_scale = self.uc_scale
        c = c.to(device=self.device, dtype=torch.float32)
        uc = None if uc is None else uc.to(device=self.device, dtype=torch.float32)
        samples = self._sample_minibatch(self.ddim_sampler, ddim_steps, self.z_shape, c, uc, x_T, uc_scale, ddim_eta,
                                         max_steps)
        self.last_latents = samples
        self.gen_df = self._decode_checked(samples)
        return self.gen_df

    @torch.no_grad()
    def inference(self, data, ddim_steps=None, ddim_eta=0., uc_scale=None, infer_all=False, max_sample=16,
                  x_T: Optional[Tensor] = None, max_steps: Optional[int] = None):
        """:423-457: set_input (at most `max_sample` objects unless infer_all), one guided sampler run over all of them,
        decode into self.gen_df.  (The reference then calls switch_train(): training is out of scope here.)"""
        self.switch_eval()
        self.set_input(data, max_sample=None if infer_all else max_sample)
        return self._sample_all(self.rel, self.uc_rel, ddim_steps, ddim_eta, uc_scale, x_T, max_steps)

    @torch.no_grad()
    def graph2shape(self, num_obj=6, ddim_steps=100, ddim_eta=0.0, uc_scale=None, x_T: Optional[Tensor] = None,
                    max_steps: Optional[int] = None):
        """:390-421: the first num_obj objects of the CURRENT input (set_input must have run), sampled with
        unconditional_conditioning=None -- i.e. WITHOUT classifier-free guidance, whatever uc_scale says (ddim.py:200-201)
        -- and decoded.  Returns gen_df."""
        self.switch_eval()
        return self._sample_all(self.rel[:num_obj], None, ddim_steps, ddim_eta, uc_scale, x_T, max_steps)

    @torch.no_grad()
    def gen_shape_after_foward(self, num_obj, ddim_steps=None, uc_scale=None, ddim_eta=0., x_T: Optional[Tensor] = None,
                               max_steps: Optional[int] = None):
        """:368-386 (sic): guided sampling of the first num_obj objects of the current input, decode into self.gen_df."""
        self.switch_eval()
        return self._sample_all(self.rel[:num_obj], self.uc_rel[:num_obj], ddim_steps, ddim_eta, uc_scale, x_T, max_steps)

    @property
    def renderer(self):
        """sdfusion_txt2shape_model.py:110-112: init_mesh_renderer(image_size=256, dist=1.7, elev=20, azim=20), on first use"""
        if getattr(self, "_renderer", None) is None:
            from .object_views import init_mesh_renderer
            self._renderer = init_mesh_renderer(image_size=256, dist=1.7, elev=20, azim=20, device="cuda")
        return self._renderer

    @torch.no_grad()
    def get_current_visuals(self, vocab, obj_ids, num_obj=2):
        """:645-668: OrderedDict(img_gt, img_gen_df) of uint8 grids: the first num_obj input SDFs and the generated ones,
        rendered by object_views.  The reference's third panel, img_text (the object names drawn with cv2.putText), is not
        built: cv2 is not part of this package's image.  self.text_obj still holds the names."""
        from collections import OrderedDict
        from .object_views import render_sdf, tensor2im
        self.text_obj = [vocab.get(i) for i in obj_ids[:num_obj]]
        self.img_gt = render_sdf(self.renderer, self.x[:num_obj]).detach().cpu()
        self.img_gen_df = render_sdf(self.renderer, self.gen_df).detach().cpu()
        return OrderedDict((name, tensor2im(getattr(self, name))) for name in ("img_gt", "img_gen_df"))

    # ---- checkpoint surface (VAEGAN_V2FULL.py:687-699 stores these under 'df' / 'vqvae') ----
    def state_dict(self):
        return {"df": self.df.state_dict(), "vqvae": self.vqvae.state_dict()}

    def load_state_dict(self, sd):
        if "df" in sd:
            self.df.load_state_dict(sd["df"])
        if "vqvae" in sd:
            self.vqvae.load_state_dict(sd["vqvae"])
        return self
