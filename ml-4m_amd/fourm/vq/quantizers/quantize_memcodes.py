"""``Memcodes``: the multi-head inner-product codebook of the pose / global-feature tokenizers, parameter owner in the upstream layout
(``fourm/vq/quantizers/quantize_memcodes.py`` :25-124; state-dict keys ``codes`` (H, K, d), ``to_k.weight`` / ``to_v.weight`` (H, d, d)).
Inference only: per head the token is the arg-max of <z_h, k_hj> with k_h = codes_h @ to_k.weight_h, the output v_h[token] with
v_h = codes_h @ to_v.weight_h.  The search runs in ``fourm.vq.engine`` on fm_memcodes_assign; keys and values are computed once by the
fp32 GEMM and cached there.  The training branch (straight-through gumbel-softmax) is not built."""
import torch
from torch import nn


class _HeadMix(nn.Module):
    """The parameter of upstream's einops ``EinMix('h n d -> h n c', weight_shape='h d c')``: ``weight`` (H, d, d), uniform in
    +-1 / sqrt(d) like EinMix initialises it, no bias."""

    def __init__(self, heads, dim):
        super().__init__()
        bound = dim ** -0.5
        self.weight = nn.Parameter(torch.zeros(heads, dim, dim).uniform_(-bound, bound), requires_grad=True)


class Memcodes(nn.Module):
    def __init__(self, *, dim, codebook_size, heads=1, temperature=1., channel_last=False, accept_image_fmap=True, **kwargs):
        super().__init__()
        assert dim % heads == 0, f"dim={dim} does not split into {heads} heads"
        if channel_last or not accept_image_fmap:
            raise NotImplementedError("Memcodes on sequences (channel_last / accept_image_fmap=False): only the image-feature-map form the "
                                      "tokenizers use is built")
        self.heads, self.dim, self.codebook_size = heads, dim, codebook_size
        self.scale = (dim // heads) ** -0.5               # (upstream's factor on the query: a positive scale, it cannot move the arg-max and is not applied)
        self.temperature = temperature
        self.accept_image_fmap, self.channel_last = accept_image_fmap, channel_last
        d = dim // heads
        self.codes = nn.Parameter(torch.randn(heads, codebook_size, d))
        self.to_k = _HeadMix(heads, d)
        self.to_v = _HeadMix(heads, d)

    def indices_to_embedding(self, indices):
        """tokens (B, H, 1, 1), H > 1 -> (B, H d, 1, 1): values[h][token] per head, heads concatenated (the same bits ``forward`` returns)."""
        if indices.dim() != 4 or self.heads == 1 or tuple(indices.shape[1:]) != (self.heads, 1, 1):
            raise NotImplementedError(
                f"Memcodes.indices_to_embedding of tokens shaped {tuple(indices.shape)} ({self.heads} heads): upstream's own result is not an "
                "image-shaped latent there (a transposed tensor on 1 x n grids, an error inside gather on larger ones, (B, 1, D) with one head); "
                "only one vector per sample, tokens (B, heads, 1, 1) with heads > 1, has a well-defined token -> embedding map")
        from fourm.vq.engine import memcodes_embedding
        return memcodes_embedding(self, indices)

    def forward(self, x):
        """(B, dim, h, w) -> (out (B, dim, h, w), zeros(1), tokens (B, H, h, w), or (B, h, w) with one head)   [quantize_memcodes.py:70-124]"""
        if self.training:
            raise NotImplementedError("Memcodes in training mode (straight-through gumbel-softmax) is not built: call .eval()")
        from fourm.vq.engine import memcodes_forward
        with torch.no_grad():
            return memcodes_forward(self, x)


# names only upstream's same-named module defines resolve lazily (see fourm/_upstream.py)
from fourm import _upstream as _up
__getattr__ = _up.fallthrough(__name__, is_package=False)
