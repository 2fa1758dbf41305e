"""SwinIR (Liang et al. 2021, https://arxiv.org/abs/2108.10257) with the interface, module tree and ``state_dict`` of
``pssr.models.swinir.SwinIR``: checkpoints move between the two with ``strict=True``.

The convolutions, Linears, LayerNorms, the MLP and the pixel shuffle are torch modules.  The shifted-window attention of a block --
roll, window partition, ``q k^T``, bias, mask, softmax, ``P v``, window reverse, roll back -- runs as one HIP kernel pair
(csrc/window_attn.hip) on the output of the ``qkv`` Linear applied to the un-rolled, un-windowed tokens: the Linear is per token, so
the roll and the partition commute with it.  ``fused_attention=False``, a CPU tensor, a dtype or shape the kernel does not take, or
attention dropout in training select the torch composition of the same formula instead; that one also runs on the CPU.

timm is not a dependency: ``DropPath`` and ``to_2tuple`` are local, initialisation uses ``torch.nn.init.trunc_normal_``.  Initial
values and the stochastic-depth random stream are therefore not pinned to the reference's.
"""
from __future__ import annotations

import math

import torch
import torch.nn as nn
import torch.nn.functional as F
from torch.nn.init import trunc_normal_
from torch.utils.checkpoint import checkpoint

_MASK_VALUE = -100.0


def to_2tuple(v):
    return tuple(v) if isinstance(v, (tuple, list)) else (v, v)


def _as_list(v):
    return list(v) if isinstance(v, (list, tuple)) else [v]


class DropPath(nn.Module):
    """Stochastic depth: a per-sample keep mask scaled by 1 / keep; the identity in eval() or at rate 0."""

    def __init__(self, drop_prob: float = 0.0):
        super().__init__()
        self.drop_prob = float(drop_prob)

    def forward(self, x):
        if self.drop_prob == 0.0 or not self.training:
            return x
        keep = 1.0 - self.drop_prob
        mask = x.new_empty((x.shape[0],) + (1,) * (x.dim() - 1)).bernoulli_(keep)
        return x * (mask / keep)

    def extra_repr(self):
        return f"drop_prob={self.drop_prob:.3f}"


def window_partition(x, window_size):
    """[B, H, W, C] -> [B * nW, ws, ws, C], windows row-major, tokens row-major inside a window."""
    b, h, w, c = x.shape
    x = x.view(b, h // window_size, window_size, w // window_size, window_size, c)
    return x.permute(0, 1, 3, 2, 4, 5).reshape(-1, window_size, window_size, c)


def window_reverse(windows, window_size, h, w):
    """The inverse of ``window_partition``: [B * nW, ws, ws, C] -> [B, H, W, C]."""
    nh, nw = h // window_size, w // window_size
    b = windows.shape[0] // (nh * nw)
    x = windows.view(b, nh, nw, window_size, window_size, -1)
    return x.permute(0, 1, 3, 2, 4, 5).reshape(b, h, w, -1)


class _WindowAttnFn(torch.autograd.Function):
    """ops.window_attn_fwd / window_attn_bwd as one differentiable op over (qkv, bias_table)."""

    @staticmethod
    def forward(ctx, qkv, bias_table, heads, ws, shift, scale):
        from . import ops
        qkv = qkv.contiguous()
        bias = bias_table.detach().float().contiguous()
        out, lse = ops.window_attn_fwd(qkv, bias, heads, ws, shift, scale)
        ctx.save_for_backward(qkv, bias, lse)
        ctx.cfg = (heads, ws, shift, scale, bias_table.dtype)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dout):
        from . import ops
        qkv, bias, lse = ctx.saved_tensors
        heads, ws, shift, scale, bias_dtype = ctx.cfg
        dqkv, dbias = ops.window_attn_bwd(qkv, bias, lse, dout.contiguous(), heads, ws, shift, scale)
        return dqkv, dbias.to(bias_dtype), None, None, None, None


class Mlp(nn.Module):
    def __init__(self, in_features, hidden_features=None, out_features=None, act_layer=nn.GELU, drop=0.0):
        super().__init__()
        self.fc1 = nn.Linear(in_features, hidden_features or in_features)
        self.act = act_layer()
        self.fc2 = nn.Linear(hidden_features or in_features, out_features or in_features)
        self.drop = nn.Dropout(drop)

    def forward(self, x):
        return self.drop(self.fc2(self.drop(self.act(self.fc1(x)))))


class WindowAttention(nn.Module):
    """Multi-head self attention inside windows with a learnt relative-position bias.  ``forward`` is the torch composition over
    windowed tokens [B * nW, N, C]; ``fused`` is the HIP path over the token image [B, H, W, C]."""

    def __init__(self, dim, window_size, num_heads, qkv_bias=True, qk_scale=None, attn_drop=0.0, proj_drop=0.0):
        super().__init__()
        self.dim, self.window_size, self.num_heads = dim, window_size, num_heads
        self.scale = qk_scale or (dim // num_heads) ** -0.5
        wh, ww = window_size
        self.relative_position_bias_table = nn.Parameter(torch.zeros((2 * wh - 1) * (2 * ww - 1), num_heads))
        # index into the table for every (query, key) pair: (dy + wh - 1) * (2 ww - 1) + (dx + ww - 1)
        ys, xs = torch.meshgrid(torch.arange(wh), torch.arange(ww), indexing="ij")
        ys, xs = ys.flatten(), xs.flatten()
        dy, dx = ys[:, None] - ys[None, :], xs[:, None] - xs[None, :]
        self.register_buffer("relative_position_index", (dy + wh - 1) * (2 * ww - 1) + (dx + ww - 1))
        self.qkv = nn.Linear(dim, dim * 3, bias=qkv_bias)
        self.attn_drop = nn.Dropout(attn_drop)
        self.proj = nn.Linear(dim, dim)
        self.proj_drop = nn.Dropout(proj_drop)
        trunc_normal_(self.relative_position_bias_table, std=0.02)
        self.softmax = nn.Softmax(dim=-1)

    def forward(self, x, mask=None):
        bw, n, c = x.shape
        heads = self.num_heads
        q, k, v = self.qkv(x).reshape(bw, n, 3, heads, c // heads).permute(2, 0, 3, 1, 4).unbind(0)
        attn = (q * self.scale) @ k.transpose(-2, -1)
        bias = self.relative_position_bias_table[self.relative_position_index.view(-1)].view(n, n, heads)
        attn = attn + bias.permute(2, 0, 1).contiguous().unsqueeze(0)
        if mask is not None:
            nw = mask.shape[0]
            attn = (attn.view(bw // nw, nw, heads, n, n) + mask.unsqueeze(1).unsqueeze(0)).view(-1, heads, n, n)
        attn = self.attn_drop(self.softmax(attn))
        x = (attn @ v).transpose(1, 2).reshape(bw, n, c)
        return self.proj_drop(self.proj(x))

    def fused(self, x, shift):
        """x [B, H, W, C] (un-rolled, un-windowed) -> attention output [B, H, W, C]; None when the kernel does not take the case."""
        from . import ops
        b, h, w, c = x.shape
        ws = self.window_size[0]
        if self.window_size[0] != self.window_size[1] or not x.is_cuda:
            return None
        if self.attn_drop.p > 0 and self.training:
            return None
        if not ops.window_attn_supported(torch.float32, h, w, c, self.num_heads, ws, shift):
            return None
        qkv = self.qkv(x)
        if qkv.dtype not in (torch.float32, torch.bfloat16):
            return None
        out = _WindowAttnFn.apply(qkv, self.relative_position_bias_table, self.num_heads, ws, shift, float(self.scale))
        return self.proj_drop(self.proj(out))

    def extra_repr(self):
        return f"dim={self.dim}, window_size={self.window_size}, num_heads={self.num_heads}"


class SwinTransformerBlock(nn.Module):
    def __init__(self, dim, input_resolution, num_heads, window_size=7, shift_size=0, mlp_ratio=4.0, qkv_bias=True, qk_scale=None,
                 drop=0.0, attn_drop=0.0, drop_path=0.0, act_layer=nn.GELU, norm_layer=nn.LayerNorm, fused_attention=True):
        super().__init__()
        self.dim, self.input_resolution, self.num_heads, self.mlp_ratio = dim, input_resolution, num_heads, mlp_ratio
        self.window_size, self.shift_size = window_size, shift_size
        self.fused_attention = fused_attention
        if min(input_resolution) <= window_size:          # one window covers the image: no partition, no shift
            self.shift_size, self.window_size = 0, min(input_resolution)
        if not 0 <= self.shift_size < self.window_size:
            raise ValueError(f"shift_size must between 0 and window_size. Given values are {shift_size} and {window_size}.")
        self.norm1 = norm_layer(dim)
        self.attn = WindowAttention(dim, window_size=to_2tuple(self.window_size), num_heads=num_heads, qkv_bias=qkv_bias, qk_scale=qk_scale,
                                    attn_drop=attn_drop, proj_drop=drop)
        self.drop_path = DropPath(drop_path) if drop_path > 0.0 else nn.Identity()
        self.norm2 = norm_layer(dim)
        self.mlp = Mlp(in_features=dim, hidden_features=int(dim * mlp_ratio), act_layer=act_layer, drop=drop)
        self.register_buffer("attn_mask", self.calculate_mask(input_resolution) if self.shift_size > 0 else None)

    def calculate_mask(self, x_size):
        """[nW, N, N]: 0 where two tokens of a shifted window come from the same region of the image, -100 elsewhere."""
        h, w = x_size
        ws, s = self.window_size, self.shift_size

        def region(length):          # 0 | 1 | 2 for [0, L - ws) | [L - ws, L - s) | [L - s, L)
            ids = torch.zeros(length)
            ids[-ws:-s] = 1
            ids[-s:] = 2
            return ids

        img = (3 * region(h)[:, None] + region(w)[None, :]).view(1, h, w, 1)
        ids = window_partition(img, ws).view(-1, ws * ws)
        diff = ids.unsqueeze(1) - ids.unsqueeze(2)
        return torch.zeros_like(diff).masked_fill(diff != 0, _MASK_VALUE)

    def _attend(self, x, x_size):
        """x [B, H, W, C] normalised tokens -> attention output [B, H, W, C]."""
        h, w = x_size
        b, c = x.shape[0], x.shape[3]
        ws, s = self.window_size, self.shift_size
        if self.fused_attention:
            out = self.attn.fused(x, s)
            if out is not None:
                return out
        if s > 0:
            x = torch.roll(x, shifts=(-s, -s), dims=(1, 2))
        windows = window_partition(x, ws).view(-1, ws * ws, c)
        if tuple(self.input_resolution) == tuple(x_size):
            mask = self.attn_mask
        else:                        # another size than the one the buffer was made for
            mask = self.calculate_mask(x_size).to(x.device) if s > 0 else None
        out = window_reverse(self.attn(windows, mask=mask).view(-1, ws, ws, c), ws, h, w)
        if s > 0:
            out = torch.roll(out, shifts=(s, s), dims=(1, 2))
        return out

    def forward(self, x, x_size):
        h, w = x_size
        b, _, c = x.shape
        x = x + self.drop_path(self._attend(self.norm1(x).view(b, h, w, c), x_size).reshape(b, h * w, c))
        return x + self.drop_path(self.mlp(self.norm2(x)))

    def extra_repr(self):
        return (f"dim={self.dim}, input_resolution={self.input_resolution}, num_heads={self.num_heads}, window_size={self.window_size}, "
                f"shift_size={self.shift_size}, mlp_ratio={self.mlp_ratio}")


class BasicLayer(nn.Module):
    """``depth`` blocks, alternately un-shifted and shifted by half a window."""

    def __init__(self, dim, input_resolution, depth, num_heads, window_size, mlp_ratio=4.0, qkv_bias=True, qk_scale=None, drop=0.0,
                 attn_drop=0.0, drop_path=0.0, norm_layer=nn.LayerNorm, downsample=None, use_checkpoint=False, fused_attention=True):
        super().__init__()
        self.dim, self.input_resolution, self.depth, self.use_checkpoint = dim, input_resolution, depth, use_checkpoint
        self.blocks = nn.ModuleList([
            SwinTransformerBlock(dim=dim, input_resolution=input_resolution, num_heads=num_heads, window_size=window_size,
                                 shift_size=0 if i % 2 == 0 else window_size // 2, mlp_ratio=mlp_ratio, qkv_bias=qkv_bias, qk_scale=qk_scale,
                                 drop=drop, attn_drop=attn_drop, drop_path=drop_path[i] if isinstance(drop_path, list) else drop_path,
                                 norm_layer=norm_layer, fused_attention=fused_attention)
            for i in range(depth)])
        self.downsample = None if downsample is None else downsample(input_resolution, dim=dim, norm_layer=norm_layer)

    def forward(self, x, x_size):
        for block in self.blocks:
            x = checkpoint(block, x, x_size, use_reentrant=False) if self.use_checkpoint else block(x, x_size)
        return x if self.downsample is None else self.downsample(x)

    def extra_repr(self):
        return f"dim={self.dim}, input_resolution={self.input_resolution}, depth={self.depth}"


class PatchEmbed(nn.Module):
    """[B, C, H, W] -> tokens [B, H * W, C], normalised when a norm layer is given."""

    def __init__(self, img_size=224, patch_size=4, in_chans=3, embed_dim=96, norm_layer=None):
        super().__init__()
        self.img_size, self.patch_size = to_2tuple(img_size), to_2tuple(patch_size)
        self.patches_resolution = [self.img_size[0] // self.patch_size[0], self.img_size[1] // self.patch_size[1]]
        self.num_patches = self.patches_resolution[0] * self.patches_resolution[1]
        self.in_chans, self.embed_dim = in_chans, embed_dim
        self.norm = None if norm_layer is None else norm_layer(embed_dim)

    def forward(self, x):
        x = x.flatten(2).transpose(1, 2)
        return x if self.norm is None else self.norm(x)


class PatchUnEmbed(nn.Module):
    """Tokens [B, H * W, C] -> [B, C, H, W]."""

    def __init__(self, img_size=224, patch_size=4, in_chans=3, embed_dim=96, norm_layer=None):
        super().__init__()
        self.img_size, self.patch_size = to_2tuple(img_size), to_2tuple(patch_size)
        self.patches_resolution = [self.img_size[0] // self.patch_size[0], self.img_size[1] // self.patch_size[1]]
        self.num_patches = self.patches_resolution[0] * self.patches_resolution[1]
        self.in_chans, self.embed_dim = in_chans, embed_dim

    def forward(self, x, x_size):
        return x.transpose(1, 2).view(x.shape[0], self.embed_dim, x_size[0], x_size[1])


def _conv_tail(dim, resi_connection):
    """The convolution(s) that close a residual group or the deep-feature body; None for an unknown setting, as upstream leaves it."""
    if resi_connection == "1conv":
        return nn.Conv2d(dim, dim, 3, 1, 1)
    if resi_connection == "3conv":
        return nn.Sequential(nn.Conv2d(dim, dim // 4, 3, 1, 1), nn.LeakyReLU(negative_slope=0.2, inplace=True),
                             nn.Conv2d(dim // 4, dim // 4, 1, 1, 0), nn.LeakyReLU(negative_slope=0.2, inplace=True),
                             nn.Conv2d(dim // 4, dim, 3, 1, 1))
    return None


class RSTB(nn.Module):
    """Residual Swin Transformer block: a BasicLayer, a convolution, and the skip around both."""

    def __init__(self, dim, input_resolution, depth, num_heads, window_size, mlp_ratio=4.0, qkv_bias=True, qk_scale=None, drop=0.0,
                 attn_drop=0.0, drop_path=0.0, norm_layer=nn.LayerNorm, downsample=None, use_checkpoint=False, img_size=224, patch_size=4,
                 resi_connection="1conv", fused_attention=True):
        super().__init__()
        self.dim, self.input_resolution = dim, input_resolution
        self.residual_group = BasicLayer(dim=dim, input_resolution=input_resolution, depth=depth, num_heads=num_heads, window_size=window_size,
                                         mlp_ratio=mlp_ratio, qkv_bias=qkv_bias, qk_scale=qk_scale, drop=drop, attn_drop=attn_drop,
                                         drop_path=drop_path, norm_layer=norm_layer, downsample=downsample, use_checkpoint=use_checkpoint,
                                         fused_attention=fused_attention)
        conv = _conv_tail(dim, resi_connection)
        if conv is not None:
            self.conv = conv
        self.patch_embed = PatchEmbed(img_size=img_size, patch_size=patch_size, in_chans=0, embed_dim=dim, norm_layer=None)
        self.patch_unembed = PatchUnEmbed(img_size=img_size, patch_size=patch_size, in_chans=0, embed_dim=dim, norm_layer=None)

    def forward(self, x, x_size):
        y = self.patch_unembed(self.residual_group(x, x_size), x_size)
        return self.patch_embed(self.conv(y)) + x


class Upsample(nn.Sequential):
    """conv + PixelShuffle(2) per factor of two, or one conv + PixelShuffle(3)."""

    def __init__(self, scale, num_feat):
        layers = []
        if scale & (scale - 1) == 0:
            for _ in range(int(math.log(scale, 2))):
                layers += [nn.Conv2d(num_feat, 4 * num_feat, 3, 1, 1), nn.PixelShuffle(2)]
        elif scale == 3:
            layers += [nn.Conv2d(num_feat, 9 * num_feat, 3, 1, 1), nn.PixelShuffle(3)]
        else:
            raise ValueError(f"scale {scale} is not supported. Supported scales are 2^n and 3.")
        super().__init__(*layers)


class UpsampleOneStep(nn.Sequential):
    """One conv + one PixelShuffle(scale) straight to the output channels."""

    def __init__(self, scale, num_feat, num_out_ch, input_resolution=None):
        self.num_feat, self.input_resolution = num_feat, input_resolution
        super().__init__(nn.Conv2d(num_feat, scale ** 2 * num_out_ch, 3, 1, 1), nn.PixelShuffle(scale))


class SwinIR(nn.Module):
    def __init__(self, image_size: int = 128, channels: list[int] = 1, scale: int = 4, embed_dim: int = 96, mlp_ratio: int = 2,
                 depths: list[int] = [4, 4, 4, 4], num_heads: list[int] = [6, 6, 6, 6], window_size: int = 8, patch_size: int = 1,
                 upsampler: str = "pixelshuffle", qkv_bias: bool = True, qk_scale: float = None, drop_rate: float = 0,
                 attn_drop_rate: float = 0, drop_path_rate: float = 0.1, norm_layer: nn.Module = nn.LayerNorm, ape: bool = False,
                 patch_norm: bool = True, use_checkpoint: bool = False, resi_connection: str = "1conv", *, fused_attention: bool = True):
        """SwinIR as in ``pssr.models.swinir.SwinIR`` (same arguments, defaults and errors).  ``fused_attention`` (keyword only)
        selects the HIP window-attention kernel where it applies; False keeps the torch composition everywhere."""
        super().__init__()
        if len(depths) != len(num_heads):
            raise ValueError(f"Lengths of depths and num_heads must be equal. Given lengths are {len(depths)} and {len(num_heads)}.")
        channels = _as_list(channels)
        num_in_ch, num_out_ch = (channels * 2)[:2] if len(channels) == 1 else channels[:2]
        num_feat = 64
        self.img_range = 1
        self.mean = torch.zeros(1, 1, 1, 1)          # upstream's RGB mean is never enabled (it compares the channel list with 3)
        self.upscale, self.upsampler, self.window_size = scale, upsampler, window_size
        self.fused_attention = fused_attention

        self.conv_first = nn.Conv2d(num_in_ch, embed_dim, 3, 1, 1)

        self.num_layers, self.embed_dim, self.ape, self.patch_norm = len(depths), embed_dim, ape, patch_norm
        self.num_features, self.mlp_ratio = embed_dim, mlp_ratio
        self.patch_embed = PatchEmbed(img_size=image_size, patch_size=patch_size, in_chans=embed_dim, embed_dim=embed_dim,
                                      norm_layer=norm_layer if patch_norm else None)
        self.patches_resolution = self.patch_embed.patches_resolution
        res = (self.patches_resolution[0], self.patches_resolution[1])
        self.patch_unembed = PatchUnEmbed(img_size=image_size, patch_size=patch_size, in_chans=embed_dim, embed_dim=embed_dim,
                                          norm_layer=norm_layer if patch_norm else None)
        if ape:
            self.absolute_pos_embed = nn.Parameter(torch.zeros(1, self.patch_embed.num_patches, embed_dim))
            trunc_normal_(self.absolute_pos_embed, std=0.02)
        self.pos_drop = nn.Dropout(p=drop_rate)

        rates = [r.item() for r in torch.linspace(0, drop_path_rate, sum(depths))]          # stochastic depth grows with depth
        self.layers = nn.ModuleList()
        for i, depth in enumerate(depths):
            first = sum(depths[:i])
            self.layers.append(RSTB(dim=embed_dim, input_resolution=res, depth=depth, num_heads=num_heads[i], window_size=window_size,
                                    mlp_ratio=mlp_ratio, qkv_bias=qkv_bias, qk_scale=qk_scale, drop=drop_rate, attn_drop=attn_drop_rate,
                                    drop_path=rates[first:first + depth], norm_layer=norm_layer, downsample=None,
                                    use_checkpoint=use_checkpoint, img_size=image_size, patch_size=patch_size,
                                    resi_connection=resi_connection, fused_attention=fused_attention))
        self.norm = norm_layer(embed_dim)
        conv = _conv_tail(embed_dim, resi_connection)
        if conv is not None:
            self.conv_after_body = conv

        if upsampler == "pixelshuffle":
            self.conv_before_upsample = nn.Sequential(nn.Conv2d(embed_dim, num_feat, 3, 1, 1), nn.LeakyReLU(inplace=True))
            self.upsample = Upsample(scale, num_feat)
            self.conv_last = nn.Conv2d(num_feat, num_out_ch, 3, 1, 1)
        elif upsampler == "pixelshuffledirect":
            self.upsample = UpsampleOneStep(scale, embed_dim, num_out_ch, res)
        elif upsampler == "nearest+conv":
            self.conv_before_upsample = nn.Sequential(nn.Conv2d(embed_dim, num_feat, 3, 1, 1), nn.LeakyReLU(inplace=True))
            self.conv_up1 = nn.Conv2d(num_feat, num_feat, 3, 1, 1)
            if scale == 4:
                self.conv_up2 = nn.Conv2d(num_feat, num_feat, 3, 1, 1)
            self.conv_hr = nn.Conv2d(num_feat, num_feat, 3, 1, 1)
            self.conv_last = nn.Conv2d(num_feat, num_out_ch, 3, 1, 1)
            self.lrelu = nn.LeakyReLU(negative_slope=0.2, inplace=True)
        else:
            self.conv_last = nn.Conv2d(embed_dim, num_out_ch, 3, 1, 1)
        self.apply(self._init_weights)

    def _init_weights(self, m):
        if isinstance(m, nn.Linear):
            trunc_normal_(m.weight, std=0.02)
            if m.bias is not None:
                nn.init.constant_(m.bias, 0)
        elif isinstance(m, nn.LayerNorm):
            nn.init.constant_(m.bias, 0)
            nn.init.constant_(m.weight, 1.0)

    def check_image_size(self, x):
        """Reflect-pads the bottom and the right up to a multiple of the window size."""
        h, w = x.shape[2:]
        ws = self.window_size
        return F.pad(x, (0, -w % ws, 0, -h % ws), "reflect")

    def forward_features(self, x):
        x_size = (x.shape[2], x.shape[3])
        x = self.patch_embed(x)
        if self.ape:
            x = x + self.absolute_pos_embed
        x = self.pos_drop(x)
        for layer in self.layers:
            x = layer(x, x_size)
        return self.patch_unembed(self.norm(x), x_size)

    def _body(self, x):
        return self.conv_after_body(self.forward_features(x)) + x

    def forward(self, x):
        h, w = x.shape[2:]
        x = self.check_image_size(x)
        self.mean = self.mean.type_as(x)
        x = (x - self.mean) * self.img_range
        if self.upsampler == "pixelshuffle":
            x = self.conv_last(self.upsample(self.conv_before_upsample(self._body(self.conv_first(x)))))
        elif self.upsampler == "pixelshuffledirect":
            x = self.upsample(self._body(self.conv_first(x)))
        elif self.upsampler == "nearest+conv":
            x = self.conv_before_upsample(self._body(self.conv_first(x)))
            x = self.lrelu(self.conv_up1(F.interpolate(x, scale_factor=2, mode="nearest")))
            if self.upscale == 4:
                x = self.lrelu(self.conv_up2(F.interpolate(x, scale_factor=2, mode="nearest")))
            x = self.conv_last(self.lrelu(self.conv_hr(x)))
        else:
            x = x + self.conv_last(self._body(self.conv_first(x)))
        x = x / self.img_range + self.mean
        return x[:, :, :h * self.upscale, :w * self.upscale]

    def extra_repr(self):
        return f"SwinIR with {self.upscale}x upscaling\n{self.num_layers} Swin Transformer blocks with embedding size {self.embed_dim}"
