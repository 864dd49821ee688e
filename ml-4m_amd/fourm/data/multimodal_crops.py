"""One aligned multi-modal sample batch from the device data stage: every modality of a sample goes through the SAME crop settings (upstream's
UnifiedDataTransform with one crop per sample draws one box and flip and applies them to all modalities), each through its own transform:

    rgb, normal    crop_resize, float32 (N, 3, S, S), mean = std = 0.5; ``normal`` with channel 0 inverted in flipped crops
    depth          crop_resize_depth, float32 (N, 1, S, S), truncated standardisation per crop (16-bit sources, fourm.data.crops.decode_depth)
    semseg*        crop_resize, int64 (N, S, S), always nearest
    mask_valid     crop_resize, bool (N, 1, S, S), always nearest; valid where the byte is 255 (upstream's ``to_tensor(mask) == 1.0``)

The result is the batch dict that ``fourm.vq.training.prepare_inputs`` takes.  Nothing is masked here: ``prepare_inputs`` and
``mask_out_samples`` do that with ``mask_value``."""
import numpy as np
import torch

from .crops import crop_resize, crop_resize_depth

HALF = (0.5, 0.5, 0.5)


def _mask_u8(m, i):
    """A decoded validity mask as uint8 (H, W): mode L arrives as uint8, mode 1 as bool (True -> 255, as to_tensor scales it)."""
    if isinstance(m, torch.Tensor):
        m = m.detach().cpu().numpy()
    m = np.asarray(m)
    if m.dtype == np.bool_:
        return m.astype(np.uint8) * np.uint8(255)
    if m.dtype != np.uint8:
        raise TypeError(f"mask_valid {i}: uint8 (mode 'L') or bool (mode '1') expected, got {m.dtype}")
    return m


def crop_modalities(samples, settings, size, resample_mode=None, mask_pool_size=1):
    """samples: {name: [decoded array per sample]} with names ``rgb``, ``normal`` (uint8 (H, W, 3)), ``depth`` (uint16 (H, W)), ``semseg*``
    (uint8 (H, W)) and ``mask_valid`` (uint8 or bool (H, W)); settings: one (n_i, 5) array of rows (top, left, h, w, flip) per sample, shared
    by all its modalities.  Returns {name: tensor of the sum(n_i) crops at size x size} on the current device, one crop_resize or
    crop_resize_depth call per modality.  resample_mode (None: bicubic) applies to rgb, normal and depth.  An unknown name, lists of unequal
    length or ``mask_pool_size`` > 1 (upstream's min-pooling of the mask is not built) raise before anything is launched."""
    if mask_pool_size != 1:
        raise NotImplementedError(f"mask_pool_size {mask_pool_size}: only 1 (no pooling of the valid mask) is supported")
    if not samples:
        raise ValueError("no modalities")
    for name, imgs in samples.items():
        if not (name in ("rgb", "normal", "depth", "mask_valid") or name.startswith("semseg")):
            raise ValueError(f"modality {name!r}: one of rgb, normal, depth, semseg*, mask_valid")
        if len(imgs) != len(settings):
            raise ValueError(f"modality {name!r}: {len(imgs)} samples for {len(settings)} settings arrays")
    out = {}
    for name, imgs in samples.items():
        if name == "rgb":
            out[name] = crop_resize(imgs, settings, size, resample=resample_mode, mean=HALF, std=HALF)
        elif name == "normal":
            out[name] = crop_resize(imgs, settings, size, resample=resample_mode, mean=HALF, std=HALF, invert_on_flip=(0,))
        elif name == "depth":
            out[name] = crop_resize_depth(imgs, settings, size, resample=resample_mode, standardize=True)
        elif name == "mask_valid":
            u8 = crop_resize([_mask_u8(m, i) for i, m in enumerate(imgs)], settings, size, resample="nearest", out="uint8")
            out[name] = (u8 == 255).permute(0, 3, 1, 2).contiguous()
        else:
            out[name] = crop_resize(imgs, settings, size, resample="nearest", out="int64")
    return out
