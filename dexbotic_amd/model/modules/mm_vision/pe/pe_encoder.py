"""Perception Encoder vision tower on libdexbotic_amd kernels.

Mirror of dexbotic/model/modules/mm_vision/pe/pe_encoder.py:27-71 over the arithmetic of ``PerceptionEncoderWithDownsample``
(pe/pe_model.py:367-565): patch convolution without bias, CLS token, learned absolute positions (resampled bilinearly for an input
grid that is not the native one), ln_pre, pre-LN blocks with 2-D RoPE on q and k and LayerScale on both branches, optional ln_post,
CLS dropped, pooling, and the two 3x3 stride-2 convolutions that merge the T x T token grid down to ceil(ceil(T/2)/2)^2 tokens of
4 x width columns — which is why ``hidden_size`` is ``width`` while the output rows are four times as wide (DM0 projects them
with ``linear4x``).  Unlike the CLIP tower this one is trained by the reference (no ``no_grad``): every stage has a backward.

``pool_type`` "tok" / "avg" return the pooled [N, width] feature without the downsampler (the reference's ``forward`` cannot
unpack a pooled tensor into a grid and fails there); "attn" is not built.
"""
from __future__ import annotations

from typing import Dict, Tuple

import torch
import torch.nn as nn
import torch.nn.functional as F

from ..... import _lib as L
from ..... import functional as Fn
from ..... import kernels as K
from .....engine import ParamStore
from .pe_configuration import PerceptionEncoderConfig

LN_EPS = 1e-5           # norm_layer = partial(nn.LayerNorm, eps=1e-5), pe_model.py:376


class PEVisionTower(nn.Module):
    def __init__(self, vision_tower, store: ParamStore, prefix: str = "model.mm_vision_tower.", delay_load=False):
        super().__init__()
        self.is_loaded = True
        self.vision_tower_name = vision_tower
        self.cfg = c = PerceptionEncoderConfig.from_any(vision_tower)
        if c.pool_type == "attn":
            raise NotImplementedError("PEVisionTower: pool_type='attn' (the AttentionPooling head) is not built; no registered "
                                      "configuration uses it")
        if c.pool_type not in ("none", "tok", "avg"):
            raise ValueError(f"PEVisionTower: unknown pool_type {c.pool_type!r}")
        if not c.use_rope2d:
            raise ValueError("use_rope2d must be True")
        if not c.use_abs_posemb:
            raise NotImplementedError("PEVisionTower: use_abs_posemb=False is not built; no registered configuration uses it")
        if c.width % c.heads or (c.width // c.heads) % 4:
            raise ValueError(f"PEVisionTower: width {c.width} / heads {c.heads} must give a head width that is a multiple of 4")
        self._image_processor = None
        self.store = store
        self.p = p = prefix + "vision_tower."
        C_, P, I = c.width, c.patch_size, int(c.width * c.mlp_ratio)
        self.grid = c.image_size // P
        self.kpad = (3 * P * P + 7) // 8 * 8            # im2col row length: 16-byte aligned rows for bf16
        self._tables: Dict[Tuple[int, int], Tuple[torch.Tensor, torch.Tensor]] = {}
        store.new_bucket()
        if c.use_cls_token:
            store.register([(p + "class_embedding", (C_,))])
        store.register([(p + "positional_embedding", (int(c.use_cls_token) + self.grid ** 2, C_))])
        store.register([(p + "conv1.weight", (C_, 3, P, P))])
        if c.use_ln_pre:
            store.register([(p + "ln_pre.weight", (C_,)), (p + "ln_pre.bias", (C_,))], layernorm=True)
        ls = c.ls_init_value is not None
        self.layer_specs = []
        for j in range(c.layers):
            lp = f"{p}transformer.resblocks.{j}."
            store.new_bucket()
            store.register([(lp + "ln_1.weight", (C_,)), (lp + "ln_1.bias", (C_,))], layernorm=True)
            store.register([(lp + "attn.in_proj_weight", (3 * C_, C_))])
            store.register([(lp + "attn.in_proj_bias", (3 * C_,))])
            store.register([(lp + "attn.out_proj.weight", (C_, C_)), (lp + "attn.out_proj.bias", (C_,))])
            if ls:
                store.register([(lp + "ls_1.gamma", (C_,))])
            store.register([(lp + "ln_2.weight", (C_,)), (lp + "ln_2.bias", (C_,))], layernorm=True)
            store.register([(lp + "mlp.c_fc.weight", (I, C_)), (lp + "mlp.c_fc.bias", (I,))])
            store.register([(lp + "mlp.c_proj.weight", (C_, I)), (lp + "mlp.c_proj.bias", (C_,))])
            if ls:
                store.register([(lp + "ls_2.gamma", (C_,))])
            self.layer_specs.append(Fn.PeBlockSpec(
                ln1_w=lp + "ln_1.weight", ln1_b=lp + "ln_1.bias", qkv_w=lp + "attn.in_proj_weight", qkv_b=lp + "attn.in_proj_bias",
                out_w=lp + "attn.out_proj.weight", out_b=lp + "attn.out_proj.bias", ln2_w=lp + "ln_2.weight", ln2_b=lp + "ln_2.bias",
                fc1_w=lp + "mlp.c_fc.weight", fc1_b=lp + "mlp.c_fc.bias", fc2_w=lp + "mlp.c_proj.weight",
                fc2_b=lp + "mlp.c_proj.bias", ls1=lp + "ls_1.gamma" if ls else None, ls2=lp + "ls_2.gamma" if ls else None,
                eps=LN_EPS, H=c.heads, D=C_ // c.heads, I=I))
        store.new_bucket()
        if c.use_ln_post:
            store.register([(p + "ln_post.weight", (C_,)), (p + "ln_post.bias", (C_,))], layernorm=True)
        store.register([(p + "vit_downsampler1.weight", (2 * C_, C_, 3, 3)), (p + "vit_downsampler1.bias", (2 * C_,))])
        store.register([(p + "vit_downsampler2.weight", (4 * C_, 2 * C_, 3, 3)), (p + "vit_downsampler2.bias", (4 * C_,))])

    # parameters that never receive a gradient: the downsampler of a pooled tower (its output is the pooled feature)
    def unused_parameter_names(self):
        if self.cfg.pool_type == "none":
            return []
        return [n for n in self.store.slots if n.startswith(self.p + "vit_downsampler")]

    def load_model(self):
        return

    @property
    def image_processor(self):
        if self._image_processor is None:
            from transformers import SiglipImageProcessor    # host-side preprocessing only (pe_encoder.py:8-24)
            s = self.cfg.image_size
            self._image_processor = SiglipImageProcessor(
                do_convert_rgb=None, do_normalize=True, do_rescale=True, do_resize=True, image_mean=[0.5, 0.5, 0.5],
                image_std=[0.5, 0.5, 0.5], resample=3, rescale_factor=1 / 255, size={"height": s, "width": s})
        return self._image_processor

    # ------------------------------------------------------------------------------------------ per-grid pieces
    @staticmethod
    def tokens_out(T: int) -> int:
        """tokens per image after the two stride-2 convolutions over a T x T grid"""
        return K.conv_out_grid(K.conv_out_grid(T)) ** 2

    def _rope_tables(self, gh: int, gw: int):
        key = (gh, gw)
        if key not in self._tables:
            c = self.cfg
            self._tables[key] = K.rope2d_tables(gh, gw, c.width // c.heads, self.grid, self.grid, c.use_cls_token, self.store.device)
        return self._tables[key]

    def _resampled_positions(self, pos: torch.Tensor, gh: int, gw: int) -> torch.Tensor:
        """sample_abs_posemb (pe_model.py:475-500): the grid rows of the embedding resampled bilinearly to gh x gw, the CLS row kept
        apart.  torch's own interpolate under autograd, once per forward: a parameter-sized operation."""
        C_, G = self.cfg.width, self.grid
        ncls = int(self.cfg.use_cls_token)
        grid = pos[ncls:].reshape(1, G, G, C_).permute(0, 3, 1, 2).contiguous()
        grid = F.interpolate(grid, size=(gh, gw), mode="bilinear", align_corners=False)
        grid = grid.permute(0, 2, 3, 1).reshape(gh * gw, C_)
        return torch.cat([pos[:ncls], grid], dim=0).contiguous() if ncls else grid.contiguous()

    def forward(self, images: torch.Tensor) -> torch.Tensor:
        """images [N,3,H,W] -> [N, tokens_out(H // patch), 4 * width] in the compute dtype (pool_type "none"), or the pooled
        [N, width] feature ("tok" / "avg")"""
        if isinstance(images, list):
            images = torch.stack(images, 0)
        st, c, p = self.store, self.cfg, self.p
        N, _, H, W = images.shape
        C_, P = c.width, c.patch_size
        gh, gw = H // P, W // P
        if gh < 1 or gw < 1:
            raise ValueError(f"Input image size ({H}*{W}) is smaller than one patch ({P})")
        if c.pool_type == "none" and gh != gw:
            raise ValueError(f"PEVisionTower: the downsampler needs a square patch grid, got {gh} x {gw} (image {H}*{W}, patch {P})")
        np_ = gh * gw
        native = gh == self.grid and gw == self.grid
        rows = K.im2col(images.float().contiguous(), P, self.kpad, st.compute_dtype)          # [N*np, kpad]
        anchor = st.params[p + "conv1.weight"]
        patch = Fn.LinearFn.apply(rows, anchor, st, p + "conv1.weight", None, L.ACT_NONE, (C_, 3 * P * P))
        pos_n = p + "positional_embedding"
        if native and c.use_cls_token:
            x = Fn.VitEmbedFn.apply(patch, anchor, st, p + "class_embedding", pos_n, N, np_)
        elif native:
            x = Fn.AddPosFn.apply(patch.view(N, np_, C_), anchor, st, pos_n)
        else:
            pos = self._resampled_positions(Fn.ParamFn.apply(anchor, st, pos_n), gh, gw)
            if c.use_cls_token:
                x = Fn.VitEmbedTensorFn.apply(patch, Fn.ParamFn.apply(anchor, st, p + "class_embedding"), pos, N, np_)
            else:
                x = Fn.AddFn.apply(patch.view(N, np_, C_), Fn.BroadcastBatchFn.apply(pos, N))
        T = np_ + int(c.use_cls_token)
        if c.use_ln_pre:
            x = Fn.NormFn.apply(x.reshape(N * T, C_), anchor, st, "ln", p + "ln_pre.weight", p + "ln_pre.bias", LN_EPS)
        x = x.view(N, T, C_)
        cos_t, sin_t = self._rope_tables(gh, gw)
        for sp in self.layer_specs:
            sp.N, sp.T, sp.cos, sp.sin = N, T, cos_t, sin_t
            x = Fn.PeBlockFn.apply(x, st.params[sp.fc2_w], st, sp)
        if c.use_ln_post:
            x = Fn.NormFn.apply(x.reshape(N * T, C_), anchor, st, "ln", p + "ln_post.weight", p + "ln_post.bias", LN_EPS)
            x = x.view(N, T, C_)
        if c.use_cls_token:
            x = Fn.DropClsFn.apply(x)
        if c.pool_type == "tok":
            return x[:, 0]
        if c.pool_type == "avg":
            return Fn.TokenMeanFn.apply(x)
        w1 = p + "vit_downsampler1.weight"
        x = Fn.Conv3x3s2Fn.apply(x, st.params[w1], st, w1, p + "vit_downsampler1.bias", gh)
        return Fn.Conv3x3s2Fn.apply(x, st.params[w1], st, p + "vit_downsampler2.weight", p + "vit_downsampler2.bias",
                                    K.conv_out_grid(gh))

    @property
    def dummy_feature(self):
        return torch.zeros(1, 4 * self.hidden_size, device=self.device, dtype=self.dtype)

    @property
    def dtype(self):
        return self.store.compute_dtype

    @property
    def device(self):
        return self.store.device

    @property
    def config(self):
        return self.cfg

    @property
    def hidden_size(self):
        """``width``, as in the reference: the output rows have 4 * width columns"""
        return self.cfg.width

    @property
    def num_patches(self):
        """tokens per image at the native size: the reference's (image_size // patch_size // 4) ** 2 wherever the grid divides by 4,
        and the true count where it does not"""
        return self.tokens_out(self.grid)
