"""``compute_codebook_usage`` of upstream's ``fourm/vq/vq_utils.py`` (:18-46) on the HIP engine; upstream's other public names of that module
resolve through the fall-through (fourm/_upstream.py)."""
import numpy as np
import torch

MAX_CODEBOOK_SIZE = 1 << 20          # FM_TOKEN_USAGE_MAX_K: the per-window bitmap is codebook_size bits of LDS (128 KB at the limit)


def compute_codebook_usage(all_tokens: torch.Tensor, codebook_size: int = 16_384, window_size: int = 65_536) -> float:
    """Average codebook usage: the fraction of ``codebook_size`` that appears in each full window of ``window_size`` consecutive tokens of
    ``all_tokens`` (n_tokens,), averaged over the full windows (a ragged tail is dropped; no full window: nan).  Upstream's signature and value.

    Tokens on the GPU (int64 / int32 / int16; other integer types are widened): one launch of fm_token_usage, a bitmap per window in LDS and
    its population count.  Tokens on the CPU: the same count on the host.  ValueError: ``codebook_size`` outside [1, 2^20], a non-positive
    window, tokens outside [0, codebook_size) (counted on the device; reading that flag is the one synchronisation of this evaluation-time call)."""
    codebook_size, window_size = int(codebook_size), int(window_size)
    if not 1 <= codebook_size <= MAX_CODEBOOK_SIZE:
        raise ValueError(f"codebook_size {codebook_size}: 1 .. {MAX_CODEBOOK_SIZE} (the window's bitmap lives in LDS)")
    if window_size < 1:
        raise ValueError(f"window_size {window_size}")
    if all_tokens.dim() != 1 or all_tokens.is_floating_point() or all_tokens.dtype == torch.bool:
        raise ValueError(f"all_tokens: a 1-D integer tensor expected, got {all_tokens.dtype} {tuple(all_tokens.shape)}")
    n_full_windows = all_tokens.shape[0] // window_size
    if n_full_windows == 0:
        return float("nan")
    tokens = all_tokens.detach()[:n_full_windows * window_size]
    if tokens.is_cuda:
        from fourm.hip import ops
        if tokens.dtype not in (torch.int64, torch.int32, torch.int16):
            tokens = tokens.to(torch.int64)
        tokens = tokens.contiguous()
        counts = torch.empty(n_full_windows, dtype=torch.int32, device=tokens.device)
        bad = torch.empty(1, dtype=torch.int32, device=tokens.device)
        with torch.cuda.device(tokens.device):
            ops.token_usage(tokens, n_full_windows, window_size, codebook_size, counts, bad)
        n_bad = int(bad.item())
        if n_bad:
            raise ValueError(f"{n_bad} tokens lie outside [0, {codebook_size})")
        counts = counts.tolist()
    else:
        tokens = tokens.to(torch.int64)
        if int(tokens.min()) < 0 or int(tokens.max()) >= codebook_size:
            raise ValueError(f"{int(((tokens < 0) | (tokens >= codebook_size)).sum())} tokens lie outside [0, {codebook_size})")
        counts = [int((torch.bincount(w, minlength=codebook_size) > 0).sum()) for w in tokens.split(window_size)]
    return np.mean([c / codebook_size for c in counts])


# names only upstream's same-named module defines (see fourm/_upstream.py)
from fourm import _upstream as _up
_up.merge(__name__, globals())
