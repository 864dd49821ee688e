"""The FID variant of InceptionV3 on the HIP engine: the TF 2015-12-05 graph that torch-fidelity / torchmetrics ship as
``pt_inception-2015-12-05``, in fp32 on ``fm_conv2d_nhwc_f32`` (csrc/inception.hip).  Inference only.

``FidInceptionV3`` is a parameter holder.  Parameter names follow torchvision's ``Inception3`` - every conv unit ``X`` has
``X.conv.weight (Cout, Cin, KH, KW)`` and ``X.bn.{weight, bias, running_mean, running_var}`` (BatchNorm eps 1e-3, no conv bias); the head is
``fc.weight (1008, 2048)`` / ``fc.bias``.  That is what the published checkpoint uses to the best of our knowledge: the file was not available
when this was written, so loading it is untested, and parity with torchmetrics / torch-fidelity is NOT pinned ("FID and
Inception score").  The graph itself - unit table, concatenation order, the pools of the FID variant (3 x 3 averages with
count_include_pad=False, a max pool in Mixed_7c) - is ``UNITS`` / ``_features`` below and is the contract."""
from collections import OrderedDict

import torch
import torch.nn as nn

from . import ops

__all__ = ["FidInceptionV3", "UNITS", "BN_EPS"]

BN_EPS = 1e-3
NUM_CLASSES = 1008


def _unit_table():
    """name -> (Cin, Cout, (KH, KW), stride, (pad_h, pad_w)) of every conv + BN + ReLU unit, in graph order."""
    U = OrderedDict()

    def add(name, cin, cout, k=1, s=1, p=0):
        U[name] = (cin, cout, (k, k) if isinstance(k, int) else tuple(k), s, (p, p) if isinstance(p, int) else tuple(p))

    add("Conv2d_1a_3x3", 3, 32, 3, 2)
    add("Conv2d_2a_3x3", 32, 32, 3)
    add("Conv2d_2b_3x3", 32, 64, 3, 1, 1)
    add("Conv2d_3b_1x1", 64, 80)
    add("Conv2d_4a_3x3", 80, 192, 3)
    for name, cin, pf in (("Mixed_5b", 192, 32), ("Mixed_5c", 256, 64), ("Mixed_5d", 288, 64)):
        add(f"{name}.branch1x1", cin, 64)
        add(f"{name}.branch5x5_1", cin, 48)
        add(f"{name}.branch5x5_2", 48, 64, 5, 1, 2)
        add(f"{name}.branch3x3dbl_1", cin, 64)
        add(f"{name}.branch3x3dbl_2", 64, 96, 3, 1, 1)
        add(f"{name}.branch3x3dbl_3", 96, 96, 3, 1, 1)
        add(f"{name}.branch_pool", cin, pf)
    add("Mixed_6a.branch3x3", 288, 384, 3, 2)
    add("Mixed_6a.branch3x3dbl_1", 288, 64)
    add("Mixed_6a.branch3x3dbl_2", 64, 96, 3, 1, 1)
    add("Mixed_6a.branch3x3dbl_3", 96, 96, 3, 2)
    for name, c7 in (("Mixed_6b", 128), ("Mixed_6c", 160), ("Mixed_6d", 160), ("Mixed_6e", 192)):
        add(f"{name}.branch1x1", 768, 192)
        add(f"{name}.branch7x7_1", 768, c7)
        add(f"{name}.branch7x7_2", c7, c7, (1, 7), 1, (0, 3))
        add(f"{name}.branch7x7_3", c7, 192, (7, 1), 1, (3, 0))
        add(f"{name}.branch7x7dbl_1", 768, c7)
        add(f"{name}.branch7x7dbl_2", c7, c7, (7, 1), 1, (3, 0))
        add(f"{name}.branch7x7dbl_3", c7, c7, (1, 7), 1, (0, 3))
        add(f"{name}.branch7x7dbl_4", c7, c7, (7, 1), 1, (3, 0))
        add(f"{name}.branch7x7dbl_5", c7, 192, (1, 7), 1, (0, 3))
        add(f"{name}.branch_pool", 768, 192)
    add("Mixed_7a.branch3x3_1", 768, 192)
    add("Mixed_7a.branch3x3_2", 192, 320, 3, 2)
    add("Mixed_7a.branch7x7x3_1", 768, 192)
    add("Mixed_7a.branch7x7x3_2", 192, 192, (1, 7), 1, (0, 3))
    add("Mixed_7a.branch7x7x3_3", 192, 192, (7, 1), 1, (3, 0))
    add("Mixed_7a.branch7x7x3_4", 192, 192, 3, 2)
    for name, cin in (("Mixed_7b", 1280), ("Mixed_7c", 2048)):
        add(f"{name}.branch1x1", cin, 320)
        add(f"{name}.branch3x3_1", cin, 384)
        add(f"{name}.branch3x3_2a", 384, 384, (1, 3), 1, (0, 1))
        add(f"{name}.branch3x3_2b", 384, 384, (3, 1), 1, (1, 0))
        add(f"{name}.branch3x3dbl_1", cin, 448)
        add(f"{name}.branch3x3dbl_2", 448, 384, 3, 1, 1)
        add(f"{name}.branch3x3dbl_3a", 384, 384, (1, 3), 1, (0, 1))
        add(f"{name}.branch3x3dbl_3b", 384, 384, (3, 1), 1, (1, 0))
        add(f"{name}.branch_pool", cin, 192)
    return U


UNITS = _unit_table()


class _Conv(nn.Module):
    def __init__(self, cin, cout, kh, kw):
        super().__init__()
        self.weight = nn.Parameter(torch.zeros(cout, cin, kh, kw))


class _BN(nn.Module):
    def __init__(self, c):
        super().__init__()
        self.weight, self.bias = nn.Parameter(torch.ones(c)), nn.Parameter(torch.zeros(c))
        self.register_buffer("running_mean", torch.zeros(c))
        self.register_buffer("running_var", torch.ones(c))


class _Unit(nn.Module):
    def __init__(self, cin, cout, k):
        super().__init__()
        self.conv, self.bn = _Conv(cin, cout, *k), _BN(cout)


class _FC(nn.Module):
    def __init__(self, cin, cout):
        super().__init__()
        self.weight, self.bias = nn.Parameter(torch.zeros(cout, cin)), nn.Parameter(torch.zeros(cout))


def fold_bn(weight, gamma, beta, mean, var, eps=BN_EPS):
    """conv (no bias) + BatchNorm in inference mode as one conv: float64 on the host, -> (weight (Cout, Cin, KH, KW), bias (Cout,)) float64."""
    scale = gamma.double() / torch.sqrt(var.double() + eps)
    return weight.double() * scale[:, None, None, None], beta.double() - mean.double() * scale


def pack_weight(weight):
    """(Cout, Cin, KH, KW) -> (Cout, KH*KW*Cin): tap-major, channel-minor (k = (ky KW + kx) Cin + c)."""
    return weight.permute(0, 2, 3, 1).reshape(weight.shape[0], -1).contiguous()


class FidInceptionV3(nn.Module):
    """``forward(imgs, normalize=False)`` -> dict(pool (B, 2048), logits_unbiased (B, 1008), logits (B, 1008)), fp32 on the GPU.

    ``imgs``: (B, 3, H, W) uint8, or fp32 in [0, 1] with ``normalize=True`` (torchmetrics' convention).  ``chunk``: images per internal pass
    (bounds the workspace; the convolutions are batch-invariant, so the cut does not show in the result)."""

    def __init__(self, chunk=32):
        super().__init__()
        for name, (cin, cout, k, _, _) in UNITS.items():
            parent = self
            *path, leaf = name.split(".")
            for part in path:
                if not hasattr(parent, part):
                    parent.add_module(part, nn.Module())
                parent = getattr(parent, part)
            parent.add_module(leaf, _Unit(cin, cout, k))
        self.fc = _FC(2048, NUM_CLASSES)
        self.chunk = int(chunk)
        self.__dict__["_prepared"] = None

    # ---- parameters ---------------------------------------------------------------------------------------------------------------
    def load_state_dict(self, state_dict, strict=True, **kw):
        """Drops ``*.num_batches_tracked`` and ``AuxLogits.*`` (present in torchvision-style checkpoints, unused here); otherwise strict."""
        sd = OrderedDict((k, v) for k, v in state_dict.items() if not k.endswith("num_batches_tracked") and not k.startswith("AuxLogits."))
        return super().load_state_dict(sd, strict=strict, **kw)

    def _versions(self):
        return tuple((t.data_ptr(), t._version) for t in list(self.parameters()) + list(self.buffers()))

    def prepare(self):
        """Folds BatchNorm into every conv (float64, host), packs the weights tap-major and uploads them as fp32; cached on the parameter
        versions.  -> {unit: (weight (Cout, K), bias (Cout,))} plus ``"fc"``."""
        dev = self.fc.weight.device
        key = (dev, self._versions())
        cached = self.__dict__.get("_prepared")
        if cached is not None and cached[0] == key:
            return cached[1]
        if dev.type != "cuda":
            raise RuntimeError("FidInceptionV3 computes on an MI355X through libfourm_hip.so; move it to the GPU first (there is no CPU path)")
        sd = {k: v.detach().cpu() for k, v in self.state_dict().items()}
        out = {}
        for name in UNITS:
            w, b = fold_bn(sd[f"{name}.conv.weight"], sd[f"{name}.bn.weight"], sd[f"{name}.bn.bias"], sd[f"{name}.bn.running_mean"], sd[f"{name}.bn.running_var"])
            out[name] = (pack_weight(w).float().to(dev), b.float().to(dev))
        out["fc"] = (sd["fc.weight"].float().contiguous().to(dev), sd["fc.bias"].float().contiguous().to(dev))
        self.__dict__["_prepared"] = (key, out)
        return out

    # ---- forward ------------------------------------------------------------------------------------------------------------------
    def _refuse_grad(self):
        if torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()):
            raise NotImplementedError("FidInceptionV3 runs at inference only on the HIP engine (no backward): call under torch.no_grad() "
                                      "or freeze it with requires_grad_(False)")

    def forward(self, imgs, normalize=False, chunk=None):
        self._refuse_grad()
        if not torch.is_tensor(imgs):
            raise TypeError(f"FidInceptionV3: an image tensor is expected, got {type(imgs).__name__}")
        want = torch.float32 if normalize else torch.uint8
        if imgs.dtype != want:
            raise TypeError(f"FidInceptionV3: {want} images expected with normalize={bool(normalize)}, got {imgs.dtype}")
        if imgs.dim() != 4 or imgs.shape[1] != 3 or imgs.shape[0] < 1:
            raise ValueError(f"FidInceptionV3: images (B, 3, H, W) expected, got {tuple(imgs.shape)}")
        if not imgs.is_cuda:
            raise RuntimeError(f"FidInceptionV3: the images are on {imgs.device}; the tower runs on an MI355X only (there is no CPU path)")
        chunk = self.chunk if chunk is None else int(chunk)
        if chunk < 1:
            raise ValueError(f"FidInceptionV3: chunk={chunk}")
        B = imgs.shape[0]
        with torch.no_grad():
            P = self.prepare()
            if imgs.device != P["fc"][0].device:
                raise RuntimeError(f"input on {imgs.device}, model on {P['fc'][0].device}")
            pool = torch.empty(B, 2048, dtype=torch.float32, device=imgs.device)
            for b0 in range(0, B, chunk):
                part = imgs[b0:b0 + chunk]
                rows = ops.inception_preprocess(part, normalize)
                self._features(P, rows, part.shape[0], pool[b0:b0 + chunk])
            return self._head(P, pool)

    def features(self, rows_299, chunk=None):
        """The tower behind the preprocess: ``rows_299`` fp32 NHWC rows (B*299*299, 3) in (v - 128) / 128 -> the same dict as ``forward``."""
        self._refuse_grad()
        rows_299 = ops._rows(rows_299, "FidInceptionV3.features")
        n = ops.SIZE * ops.SIZE
        if rows_299.shape[1] != 3 or rows_299.shape[0] == 0 or rows_299.shape[0] % n:
            raise ValueError(f"FidInceptionV3.features: rows (B*299*299, 3) expected, got {tuple(rows_299.shape)}")
        chunk = self.chunk if chunk is None else int(chunk)
        B = rows_299.shape[0] // n
        with torch.no_grad():
            P = self.prepare()
            pool = torch.empty(B, 2048, dtype=torch.float32, device=rows_299.device)
            for b0 in range(0, B, chunk):
                b1 = min(B, b0 + chunk)
                self._features(P, rows_299[b0 * n:b1 * n], b1 - b0, pool[b0:b1])
            return self._head(P, pool)

    def _head(self, P, pool):
        B = pool.shape[0]
        unbiased = ops.conv2d_nhwc(pool, B, 1, 1, P["fc"][0], None, 1, 1, relu=False)      # the same kernel: one code path, one invariance argument
        return dict(pool=pool, logits_unbiased=unbiased, logits=unbiased + P["fc"][1])

    def _features(self, P, rows, B, pool_out):
        """rows (B*299*299, 3) -> pool_out (B, 2048).  A map is (rows tensor, H, W)."""
        dev = rows.device

        def cv(name, fm, out=None):
            x, H, W = fm
            _, _, (kh, kw), s, pad = UNITS[name]
            w, b = P[name]
            y = ops.conv2d_nhwc(x, B, H, W, w, b, kh, kw, s, pad, True, out)
            return y, ops.conv_out_size(H, kh, s, pad[0]), ops.conv_out_size(W, kw, s, pad[1])

        def pl(mode, fm, out=None):
            x, H, W = fm
            Ho, Wo = ops.pool_out_size(mode, H, W)
            return ops.pool2d_nhwc(x, B, H, W, mode, out), Ho, Wo

        def cat(H, W, C):
            return torch.empty(B * H * W, C, dtype=torch.float32, device=dev)

        x = cv("Conv2d_1a_3x3", (rows, ops.SIZE, ops.SIZE))
        x = cv("Conv2d_2a_3x3", x)
        x = cv("Conv2d_2b_3x3", x)
        x = pl("max_s2", x)
        x = cv("Conv2d_3b_1x1", x)
        x = cv("Conv2d_4a_3x3", x)
        x = pl("max_s2", x)
        for name, pf in (("Mixed_5b", 32), ("Mixed_5c", 64), ("Mixed_5d", 64)):
            _, H, W = x
            o = cat(H, W, 224 + pf)
            cv(f"{name}.branch1x1", x, o[:, 0:64])
            cv(f"{name}.branch5x5_2", cv(f"{name}.branch5x5_1", x), o[:, 64:128])
            cv(f"{name}.branch3x3dbl_3", cv(f"{name}.branch3x3dbl_2", cv(f"{name}.branch3x3dbl_1", x)), o[:, 128:224])
            cv(f"{name}.branch_pool", pl("avg_s1p1", x), o[:, 224:224 + pf])
            x = (o, H, W)
        _, H, W = x
        Ho, Wo = ops.pool_out_size("max_s2", H, W)
        o = cat(Ho, Wo, 768)
        cv("Mixed_6a.branch3x3", x, o[:, 0:384])
        cv("Mixed_6a.branch3x3dbl_3", cv("Mixed_6a.branch3x3dbl_2", cv("Mixed_6a.branch3x3dbl_1", x)), o[:, 384:480])
        pl("max_s2", x, o[:, 480:768])
        x = (o, Ho, Wo)
        for name in ("Mixed_6b", "Mixed_6c", "Mixed_6d", "Mixed_6e"):
            _, H, W = x
            o = cat(H, W, 768)
            cv(f"{name}.branch1x1", x, o[:, 0:192])
            cv(f"{name}.branch7x7_3", cv(f"{name}.branch7x7_2", cv(f"{name}.branch7x7_1", x)), o[:, 192:384])
            t = cv(f"{name}.branch7x7dbl_1", x)
            for i in (2, 3, 4):
                t = cv(f"{name}.branch7x7dbl_{i}", t)
            cv(f"{name}.branch7x7dbl_5", t, o[:, 384:576])
            cv(f"{name}.branch_pool", pl("avg_s1p1", x), o[:, 576:768])
            x = (o, H, W)
        _, H, W = x
        Ho, Wo = ops.pool_out_size("max_s2", H, W)
        o = cat(Ho, Wo, 1280)
        cv("Mixed_7a.branch3x3_2", cv("Mixed_7a.branch3x3_1", x), o[:, 0:320])
        t = cv("Mixed_7a.branch7x7x3_1", x)
        for i in (2, 3):
            t = cv(f"Mixed_7a.branch7x7x3_{i}", t)
        cv("Mixed_7a.branch7x7x3_4", t, o[:, 320:512])
        pl("max_s2", x, o[:, 512:1280])
        x = (o, Ho, Wo)
        for name, mode in (("Mixed_7b", "avg_s1p1"), ("Mixed_7c", "max_s1p1")):      # the max pool of Mixed_7c is the FID variant's difference
            _, H, W = x
            o = cat(H, W, 2048)
            cv(f"{name}.branch1x1", x, o[:, 0:320])
            t = cv(f"{name}.branch3x3_1", x)
            cv(f"{name}.branch3x3_2a", t, o[:, 320:704])
            cv(f"{name}.branch3x3_2b", t, o[:, 704:1088])
            t = cv(f"{name}.branch3x3dbl_2", cv(f"{name}.branch3x3dbl_1", x))
            cv(f"{name}.branch3x3dbl_3a", t, o[:, 1088:1472])
            cv(f"{name}.branch3x3dbl_3b", t, o[:, 1472:1856])
            cv(f"{name}.branch_pool", pl(mode, x), o[:, 1856:2048])
            x = (o, H, W)
        pl("global_avg", x, pool_out)
