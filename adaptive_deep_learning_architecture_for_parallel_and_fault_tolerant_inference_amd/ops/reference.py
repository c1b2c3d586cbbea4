"""fp32 PyTorch oracle for the graph IR (test oracle + CPU plumbing path).

Implements Keras inference semantics layer by layer (NHWC tensors, HWIO
kernels, zero padding, BN with moving statistics, Dense (in,out)).  It is
what `test/local_infer.py` computes with `model.predict` in the reference,
and what every HIP kernel is checked against.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence

import numpy as np
import torch
import torch.nn.functional as F

from ..graph.ir import Graph, _pair, deconv_out_len, deconv_pad_before, mha_sources, same_pads


def _same(x: torch.Tensor, kh: int, kw: int, s: int, value: float = 0.0) -> torch.Tensor:
    """TF 'same' padding of an NCHW tensor (the odd pixel goes after)."""
    t, b = same_pads(x.shape[2], kh, s)
    l, r = same_pads(x.shape[3], kw, s)
    return F.pad(x, (l, r, t, b), value=value)


def _heads(b):
    """A (heads, d) projection bias broadcast over (windows, heads, tokens, d); 0.0 (no bias) stays as it is."""
    return b[:, None, :] if torch.is_tensor(b) else b


def _act(y: torch.Tensor, act, alpha: float = 0.3) -> torch.Tensor:
    """Keras activations by name (tf.keras 2.15 definitions)."""
    if act in (None, "linear"):
        return y
    if act == "relu":
        return torch.relu(y)
    if act == "relu6":
        return torch.clamp(y, 0.0, 6.0)
    if act == "softmax":
        return torch.softmax(y, dim=-1)
    if act in ("swish", "silu"):
        return y * torch.sigmoid(y)
    if act == "sigmoid":
        return torch.sigmoid(y)
    if act == "tanh":
        return torch.tanh(y)
    if act == "hard_sigmoid":
        return torch.clamp(0.2 * y + 0.5, 0.0, 1.0)
    if act == "hard_swish":
        return y * torch.clamp(y + 3.0, 0.0, 6.0) / 6.0
    if act == "gelu":
        return F.gelu(y)
    if act == "gelu_tanh":
        return F.gelu(y, approximate="tanh")
    if act == "elu":
        return F.elu(y)
    if act == "selu":
        return F.selu(y)
    if act == "softplus":
        return F.softplus(y)
    if act == "leaky_relu":
        return F.leaky_relu(y, alpha)
    raise ValueError(f"unsupported activation {act!r}")


def deconv_nhwc(x: torch.Tensor, kernel: torch.Tensor, bias, stride: int, padding: str) -> torch.Tensor:
    """Keras Conv2DTranspose (no output_padding, no dilation) on NHWC x with the Keras kernel
    (kh, kw, filters, cin): the full scatter F[i*s + t] += x[i] * w[t] (no kernel flip), of which the output is
    `deconv_out_len` elements from `deconv_pad_before`; positions past the end of F (k < s) are zero before
    the bias."""
    kh, kw = kernel.shape[:2]
    full = F.conv_transpose2d(x.permute(0, 3, 1, 2), kernel.permute(3, 2, 0, 1), None, stride=stride)
    oh, ow = deconv_out_len(x.shape[1], kh, stride, padding), deconv_out_len(x.shape[2], kw, stride, padding)
    pt, pl = deconv_pad_before(kh, stride, padding), deconv_pad_before(kw, stride, padding)
    full = F.pad(full, (0, max(pl + ow - full.shape[3], 0), 0, max(pt + oh - full.shape[2], 0)))
    y = full[:, :, pt:pt + oh, pl:pl + ow].permute(0, 2, 3, 1)
    return y if bias is None else y + bias


def upsample_nhwc(x: torch.Tensor, size, interpolation: str) -> torch.Tensor:
    """Keras UpSampling2D on NHWC x: 'nearest' repeats pixels, 'bilinear' is tf.image.resize's half-pixel
    centres (`align_corners=False`)."""
    sh, sw = size
    if interpolation == "nearest":
        return x.repeat_interleave(sh, dim=1).repeat_interleave(sw, dim=2)
    if interpolation != "bilinear":
        raise ValueError(f"unsupported interpolation {interpolation!r}")
    y = F.interpolate(x.permute(0, 3, 1, 2), size=(x.shape[1] * sh, x.shape[2] * sw), mode="bilinear",
                      align_corners=False)
    return y.permute(0, 2, 3, 1)


class ReferenceExecutor:
    def __init__(self, g: Graph, weights: Dict[str, np.ndarray], device="cpu", dtype=torch.float32):
        self.g = g
        self.device = torch.device(device)
        self.dtype = dtype
        self.w: Dict[str, torch.Tensor] = {}
        for n in g.order:
            L = g.layers[n]
            for wname, _ in L.weight_shapes(g.in_shapes(n)) if L.op != "input" else []:
                self.w[wname] = torch.from_numpy(np.asarray(weights[wname], np.float32)).to(self.device, dtype)
            if L.op == "rescale":           # per-channel Rescaling factors: device tensors made once (graph capture)
                for k in ("scale", "offset"):
                    if isinstance(L.attrs.get(k), (list, tuple)):
                        self.w[f"{n}/#{k}"] = torch.tensor(L.attrs[k], dtype=dtype, device=self.device)

    def _layer(self, L, ins: List[torch.Tensor]) -> torch.Tensor:
        a = L.attrs
        if L.op == "zeropad":
            (t, b), (l, r) = a["pad"]
            return F.pad(ins[0], (0, 0, l, r, t, b))
        if L.op == "conv":
            x = ins[0].permute(0, 3, 1, 2)
            k = self.w[f"{L.name}/kernel"].permute(3, 2, 0, 1)
            bias = self.w.get(f"{L.name}/bias")
            s = a.get("stride", 1)
            if a.get("padding", "valid") == "same":
                x = _same(x, *a["kernel"], s)
            y = F.conv2d(x, k, bias, stride=s, groups=a.get("groups", 1))
            return _act(y.permute(0, 2, 3, 1), a.get("activation"), a.get("alpha", 0.3))
        if L.op == "dwconv":
            x = ins[0].permute(0, 3, 1, 2)
            c = x.shape[1]
            k = self.w[f"{L.name}/depthwise_kernel"].permute(2, 3, 0, 1)      # (C, 1, kh, kw)
            bias = self.w.get(f"{L.name}/bias")
            s = a.get("stride", 1)
            if a.get("padding", "valid") == "same":
                x = _same(x, *a["kernel"], s)
            y = F.conv2d(x, k, bias, stride=s, groups=c)
            return _act(y.permute(0, 2, 3, 1), a.get("activation"))
        if L.op == "deconv":
            bias = self.w.get(f"{L.name}/bias")
            y = deconv_nhwc(ins[0], self.w[f"{L.name}/kernel"], bias, a.get("stride", 1), a.get("padding", "valid"))
            return _act(y, a.get("activation"), a.get("alpha", 0.3))
        if L.op == "upsample":
            return upsample_nhwc(ins[0], a["size"], a.get("interpolation", "nearest"))
        if L.op == "crop":
            (t, b), (l, r) = a["crop"]
            return ins[0][:, t:ins[0].shape[1] - b, l:ins[0].shape[2] - r, :]
        if L.op == "bn":
            m_, v_ = self.w[f"{L.name}/moving_mean"], self.w[f"{L.name}/moving_variance"]
            g_ = self.w.get(f"{L.name}/gamma", 1.0)         # scale=False / center=False defaults
            b_ = self.w.get(f"{L.name}/beta", 0.0)
            return (ins[0] - m_) / torch.sqrt(v_ + a.get("epsilon", 1e-3)) * g_ + b_
        if L.op == "layernorm":
            c = ins[0].shape[-1]
            return F.layer_norm(ins[0], (c,), self.w.get(f"{L.name}/gamma"), self.w.get(f"{L.name}/beta"),
                                a.get("epsilon", 1e-3))
        if L.op == "rmsnorm":
            return F.rms_norm(ins[0], (ins[0].shape[-1],), self.w.get(f"{L.name}/scale"), a.get("epsilon", 1e-6))
        if L.op == "groupnorm":
            # the library normalises over (C / G, H, W) of an NCHW tensor.  A contiguous copy: on the strided
            # (channels-last) view its CPU kernel takes a one-pass form that loses every digit at mean >> sigma
            # (error 1.0 against 1.4e-4 on the mean 100 / sigma 0.1 probe of tests/groupnorm_cases.py)
            y = F.group_norm(ins[0].permute(0, 3, 1, 2).contiguous(), int(a["groups"]), self.w.get(f"{L.name}/gamma"),
                             self.w.get(f"{L.name}/beta"), a.get("epsilon", 1e-3))
            return y.permute(0, 2, 3, 1)
        if L.op == "layerscale":
            return ins[0] * self.w[f"{L.name}/gamma"]
        if L.op == "mha":
            # Keras MultiHeadAttention(query, value, key): attention over all positions, the query scaled before the
            # dot product; one input is (x, x), a missing key is the value
            w = lambda p: self.w[f"{L.name}/{p}/kernel"]
            b = lambda p: self.w.get(f"{L.name}/{p}/bias", 0.0)
            x, xk, xv = (t.reshape(t.shape[0], -1, t.shape[-1]) for t in mha_sources(ins, bool(a.get("key_mask"))))      # (B, T, C) each
            q = (torch.einsum("btc,chd->bthd", x, w("query")) + b("query")) * (1.0 / float(a["key_dim"]) ** 0.5)
            k = torch.einsum("btc,chd->bthd", xk, w("key")) + b("key")
            v = torch.einsum("btc,chd->bthd", xv, w("value")) + b("value")
            if a.get("rope"):
                # rotary embedding, rotate-half convention, at position t of the image: the angles in float64,
                # rounded to the tensors' dtype (the 1/sqrt(d) scale above commutes with the rotation)
                d = int(a["key_dim"])
                inv = float(a["rope"]) ** (-2.0 * torch.arange(d // 2, dtype=torch.float64) / d)
                th = torch.arange(q.shape[1], dtype=torch.float64)[:, None] * inv[None, :]
                cs, sn = (f(th).to(q.dtype).to(q.device)[None, :, None, :] for f in (torch.cos, torch.sin))

                def rot(t):
                    t1, t2 = t[..., :d // 2], t[..., d // 2:]
                    return torch.cat([t1 * cs - t2 * sn, t2 * cs + t1 * sn], dim=-1)
                q, k = rot(q), rot(k)
            if k.shape[2] != q.shape[2]:        # grouped-query attention: head h reads K / V head h // g
                k = k.repeat_interleave(q.shape[2] // k.shape[2], dim=2)
                v = v.repeat_interleave(q.shape[2] // v.shape[2], dim=2)
            s = torch.einsum("bqhd,bkhd->bhqk", q, k)
            if a.get("causal"):                 # Keras _compute_causal_mask: query i attends keys j <= i
                t = s.shape[-1]
                s = s.masked_fill(torch.ones(t, t, dtype=torch.bool, device=s.device).triu(1), float("-inf"))
            keep = None
            if a.get("key_mask"):
                # the padding mask: token j is padding iff -1 < ids[j] < 1 (a NaN is kept).  A padded key gets the
                # score -inf; a padded query's context row, and every row of a sample with no kept key, is zeros
                ids = ins[-1].reshape(ins[-1].shape[0], -1)
                keep = ~((ids > -1) & (ids < 1))                                    # (B, T)
                s = s.masked_fill(~keep[:, None, None, :], float("-inf"))
                s = s.masked_fill(~keep.any(-1)[:, None, None, None], 0.0)          # no kept key: no NaN row
            p = torch.softmax(s, dim=-1)
            y = torch.einsum("bhqk,bkhd->bqhd", p, v)
            if keep is not None:
                y = y * (keep & keep.any(-1, keepdim=True))[:, :, None, None].to(y.dtype)
            y = torch.einsum("bqhd,hdc->bqc", y, w("attention_output")) + b("attention_output")
            return y.reshape(ins[0].shape)
        if L.op == "winattn":
            # Swin (Liu et al. 2021) the published way: roll, partition into windows, a gather of the bias table,
            # an explicit additive -100 mask between the regions of a shifted map, reverse, roll back
            w = lambda p: self.w[f"{L.name}/{p}/kernel"]
            b = lambda p: self.w.get(f"{L.name}/{p}/bias", 0.0)
            B, H, W, C = ins[0].shape
            M, s, h, d = int(a["window"]), int(a.get("shift", 0)), int(a["num_heads"]), int(a["key_dim"])

            def partition(t):                   # (B, H, W, c) -> (B * windows, M * M, c)
                c = t.shape[-1]
                return t.reshape(B, H // M, M, W // M, M, c).permute(0, 1, 3, 2, 4, 5).reshape(-1, M * M, c)

            x = torch.roll(ins[0], shifts=(-s, -s), dims=(1, 2)) if s else ins[0]
            xw = partition(x)
            q = (torch.einsum("ntc,chd->nhtd", xw, w("query")) + _heads(b("query"))) * (1.0 / float(d) ** 0.5)
            k = torch.einsum("ntc,chd->nhtd", xw, w("key")) + _heads(b("key"))
            v = torch.einsum("ntc,chd->nhtd", xw, w("value")) + _heads(b("value"))
            coords = torch.stack(torch.meshgrid(torch.arange(M), torch.arange(M), indexing="ij")).flatten(1)
            rel = (coords[:, :, None] - coords[:, None, :]).permute(1, 2, 0) + (M - 1)
            index = (rel[..., 0] * (2 * M - 1) + rel[..., 1]).to(ins[0].device)
            table = self.w[f"{L.name}/relative_position_bias_table"]
            attn = q @ k.transpose(-2, -1) + table[index.reshape(-1)].reshape(M * M, M * M, h).permute(2, 0, 1)
            if s:
                img = torch.zeros((1, H, W, 1), dtype=ins[0].dtype, device=ins[0].device)
                cnt = 0
                for hs in (slice(0, -M), slice(-M, -s), slice(-s, None)):
                    for ws in (slice(0, -M), slice(-M, -s), slice(-s, None)):
                        img[:, hs, ws, :] = cnt
                        cnt += 1
                mw = img.reshape(1, H // M, M, W // M, M, 1).permute(0, 1, 3, 2, 4, 5).reshape(-1, M * M)
                mask = mw[:, None, :] - mw[:, :, None]
                mask = torch.where(mask != 0, torch.full_like(mask, -100.0), torch.zeros_like(mask))
                nw = mask.shape[0]
                attn = (attn.reshape(B, nw, h, M * M, M * M) + mask[None, :, None]).reshape(-1, h, M * M, M * M)
            y = (torch.softmax(attn, dim=-1) @ v).permute(0, 2, 1, 3)                   # (n, t, h, d)
            y = y.reshape(B, H // M, W // M, M, M, h * d).permute(0, 1, 3, 2, 4, 5).reshape(B, H, W, h * d)
            if s:
                y = torch.roll(y, shifts=(s, s), dims=(1, 2))
            return (torch.einsum("bhwk,kc->bhwc", y, w("attention_output").reshape(h * d, -1))
                    + b("attention_output"))
        if L.op == "space_to_depth":
            x = ins[0]
            return torch.cat([x[:, 0::2, 0::2], x[:, 1::2, 0::2], x[:, 0::2, 1::2], x[:, 1::2, 1::2]], dim=-1)
        if L.op == "posembed":
            x = ins[0].reshape(ins[0].shape[0], -1, ins[0].shape[-1])
            if a.get("class_token"):
                x = torch.cat([self.w[f"{L.name}/class_token"].expand(x.shape[0], 1, -1), x], dim=1)
            return (x + self.w[f"{L.name}/position_embedding"]).unsqueeze(1)
        if L.op == "embedding":
            # the ids truncated toward zero, as Keras casts a float input; an id outside [0, V) yields a zero row
            table = self.w[f"{L.name}/embeddings"]
            ids = ins[0].to(torch.float64)
            ok = (ids > -1) & (ids < table.shape[0])
            idx = torch.where(ok, ids, torch.zeros_like(ids)).to(torch.int64)
            return table[idx] * ok.unsqueeze(-1).to(table.dtype)
        if L.op == "queries":
            return self.w[f"{L.name}/embeddings"].expand(ins[0].shape[0], 1, -1, -1)
        if L.op == "relu":
            y = torch.relu(ins[0])
            return y if a.get("max_value") is None else torch.clamp(y, max=float(a["max_value"]))
        if L.op == "identity":
            return ins[0]
        if L.op == "act":
            return _act(ins[0], a["fn"], a.get("alpha", 0.3))
        if L.op == "binary":
            x, y = ins
            if y.dim() != x.dim():                      # one channel row per image
                y = y.reshape((y.shape[0],) + (1,) * (x.dim() - 2) + (y.shape[-1],))
            fn = a["fn"]
            if fn == "mul":
                return x * y
            if fn == "sub":
                return x - y
            if fn == "max":
                return torch.maximum(x, y)
            if fn == "min":
                return torch.minimum(x, y)
            if fn == "avg":
                return 0.5 * (x + y)
            raise ValueError(f"binary {fn}")
        if L.op == "gmp":
            y = ins[0].amax(dim=(1, 2))
            return y.reshape(y.shape[0], 1, 1, -1) if a.get("keepdims") else y
        if L.op == "reshape":
            return ins[0].reshape((ins[0].shape[0],) + tuple(L.out_shape))
        if L.op == "rescale":
            sc, of = a.get("scale", 1.0), a.get("offset", 0.0)
            if isinstance(sc, (list, tuple)):
                sc = self.w[f"{L.name}/#scale"]
            if isinstance(of, (list, tuple)):
                of = self.w[f"{L.name}/#offset"]
            return ins[0] * sc + of
        if L.op == "normalization":
            m, v = self.w[f"{L.name}/mean"], self.w[f"{L.name}/variance"]
            return (ins[0] - m) / torch.clamp(torch.sqrt(v), min=1e-7)
        if L.op == "flatten":
            return ins[0].reshape(ins[0].shape[0], -1)
        if L.op == "concat":
            return torch.cat(ins, dim=-1)
        if L.op == "add":
            y = ins[0]
            for t in ins[1:]:
                y = y + t
            return y
        if L.op in ("maxpool", "avgpool"):
            x = ins[0].permute(0, 3, 1, 2)
            kh, kw = _pair(a["pool"])
            s = a["stride"]
            if L.op == "maxpool":
                if a.get("padding", "valid") == "same":
                    x = _same(x, kh, kw, s, value=float("-inf"))
                y = F.max_pool2d(x, (kh, kw), s)
            elif a.get("padding", "valid") == "same":
                # mean over the in-image part of each window (TF excludes the padding)
                ones = torch.ones_like(x[:, :1])
                num = F.avg_pool2d(_same(x, kh, kw, s), (kh, kw), s, divisor_override=1)
                den = F.avg_pool2d(_same(ones, kh, kw, s), (kh, kw), s, divisor_override=1)
                y = num / den
            else:
                y = F.avg_pool2d(x, (kh, kw), s)
            return y.permute(0, 2, 3, 1)
        if L.op == "gap":
            y = ins[0].mean(dim=(1, 2))
            return y.reshape(y.shape[0], 1, 1, -1) if a.get("keepdims") else y
        if L.op == "dense":
            y = ins[0] @ self.w[f"{L.name}/kernel"]
            if f"{L.name}/bias" in self.w:
                y = y + self.w[f"{L.name}/bias"]
            return _act(y, a.get("activation"))
        if L.op == "softmax":
            return torch.softmax(ins[0], dim=-1)
        raise ValueError(f"unsupported op {L.op}")

    @torch.no_grad()
    def run(self, inputs: Dict[str, torch.Tensor], outputs: Optional[Sequence[str]] = None,
            keep_all: bool = False) -> Dict[str, torch.Tensor]:
        g = self.g
        outputs = list(outputs or g.output_names)
        vals: Dict[str, torch.Tensor] = {}
        for n, t in inputs.items():
            vals[n] = t.to(self.device, self.dtype)
        cons = g.consumers()
        remaining = {n: len(cons[n]) for n in g.order}
        for n in g.order:
            if n in vals:
                continue
            L = g.layers[n]
            if L.op == "input":
                raise KeyError(f"missing input {n}")
            vals[n] = self._layer(L, [vals[i] for i in L.inputs])
            if not keep_all:
                for i in L.inputs:
                    remaining[i] -= 1
                    if remaining[i] == 0 and i not in outputs:
                        vals.pop(i, None)
        return {o: vals[o] for o in outputs} if not keep_all else vals

    def __call__(self, x: torch.Tensor) -> torch.Tensor:
        return self.run({self.g.input: x})[self.g.output]
