"""MLP encoders / decoders of the one-vector-per-sample tokenizers (human poses, DINOv2 / ImageBind global features): parameter
owners in the upstream layout (``fourm/vq/models/mlp_models.py``: ``BottleneckBlock`` :19-32, ``StandardMLP`` :35-72, ``BottleneckMLP``
:75-115, ``build_mlp`` :118-165; the architectures of "Scaling MLPs: A Tale of Inductive Bias", arXiv 2306.13575).  The arithmetic runs
in ``fourm.vq.engine`` (``_mlp_rows``) on the exact-fp32 GEMM and LayerNorm kernels, point-wise over the rows (B h w, C)."""
from typing import Optional

from torch import nn

_NO_FORWARD = "{} computes inside VQ.encode / VQVAE.decode_quant (fourm.vq.engine); it has no stand-alone forward"


class BottleneckBlock(nn.Module):
    """Linear(thin -> wide), GELU, Linear(wide -> thin): state-dict names ``block.0.*`` / ``block.2.*``."""

    def __init__(self, thin, wide):
        super().__init__()
        self.block = nn.Sequential(nn.Linear(thin, wide), nn.GELU(), nn.Linear(wide, thin))

    def forward(self, x):
        raise RuntimeError(_NO_FORWARD.format("BottleneckBlock"))


class StandardMLP(nn.Module):
    """linear_in, then z = layers[i](layernorms[i](z)) for the len(widths) - 1 inner layers (no activation), linear_out."""

    def __init__(self, dim_in, dim_out, widths):
        super().__init__()
        self.dim_in, self.dim_out, self.widths = dim_in, dim_out, widths
        self.linear_in = nn.Linear(dim_in, widths[0])
        self.linear_out = nn.Linear(widths[-1], dim_out)
        self.layers = nn.ModuleList([nn.Linear(a, b) for a, b in zip(widths[:-1], widths[1:])])
        self.layernorms = nn.ModuleList([nn.LayerNorm(b) for b in widths[1:]])          # (upstream sizes the norm by the layer's OUTPUT width)

    def forward(self, x):
        raise RuntimeError(_NO_FORWARD.format("StandardMLP"))


class BottleneckMLP(nn.Module):
    """linear_in, then x = x + blocks[i](layernorms[i](x)) per [wide, thin] entry of block_dims, linear_out."""

    def __init__(self, dim_in, dim_out, block_dims):
        super().__init__()
        self.dim_in, self.dim_out, self.block_dims = dim_in, dim_out, block_dims
        self.linear_in = nn.Linear(dim_in, block_dims[0][1])
        self.linear_out = nn.Linear(block_dims[-1][1], dim_out)
        self.blocks = nn.ModuleList([BottleneckBlock(thin=thin, wide=wide) for wide, thin in block_dims])
        self.layernorms = nn.ModuleList([nn.LayerNorm(thin) for _, thin in block_dims])

    def forward(self, x):
        raise RuntimeError(_NO_FORWARD.format("BottleneckMLP"))


def build_mlp(model_id: str = "BottleneckMLP/B_6-Wi_1024", dim_in: Optional[int] = None, dim_out: Optional[int] = None, **kwargs) -> nn.Module:
    """"BottleneckMLP/B_<blocks>-Wi_<width>[-E_<expansion>]" or "MLP/B_<layers>-Wi_<width>" -> the model; dim_in / dim_out default to the
    width, the expansion factor to 4."""
    family, arch = model_id.split("/")
    assert family in ("BottleneckMLP", "MLP"), f"Model {family} not supported."
    fields = [int(part.split("_")[1]) for part in arch.split("-")]
    n, width = fields[0], fields[1]
    expansion = fields[2] if len(fields) == 3 else 4
    dim_in, dim_out = dim_in or width, dim_out or width
    if family == "BottleneckMLP":
        return BottleneckMLP(dim_in=dim_in, dim_out=dim_out, block_dims=[[expansion * width, width] for _ in range(n)])
    return StandardMLP(dim_in=dim_in, dim_out=dim_out, widths=[width] * n)


# names only upstream's same-named module defines resolve lazily (see fourm/_upstream.py)
from fourm import _upstream as _up
__getattr__ = _up.fallthrough(__name__, is_package=False)
