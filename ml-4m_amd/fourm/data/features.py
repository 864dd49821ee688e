"""Feature tasks of dataset pre-tokenization: the frozen feature network in front of a feature-map or global-embedding tokenizer
(upstream save_vq_tokens.py:37, 188-197, 270-286).  The extractors are the HIP towers of this package - CLIP's vision tower
(fourm/utils/clip/model.py) and DINOv2's (fourm/utils/dinov2/model.py; parity with the `facebookresearch/dinov2` package and with the real
checkpoints is unpinned) - built from a LOCAL state-dict file: nothing is fetched (no torch.hub, no clip.load)."""
import os

FEATURE_TASKS = ("CLIP-B16", "DINOv2-B14", "DINOv2-B14-global")
CKPT_ENV = "FOURM_FEATURE_EXTRACTOR_CKPT"


def checkpoint_path(task):
    """The state-dict file named by FOURM_FEATURE_EXTRACTOR_CKPT; refusals name the variable and are raised before anything is loaded."""
    if task not in FEATURE_TASKS:
        raise NotImplementedError(f"task {task!r}: the feature extractor tasks built here are {list(FEATURE_TASKS)}")
    path = os.environ.get(CKPT_ENV)
    if not path:
        raise NotImplementedError(f"task {task!r} needs the frozen feature extractor in front of the tokenizer: set {CKPT_ENV} to a local state-dict "
                                  "file of the network (nothing is downloaded)")
    if not os.path.isfile(path):
        raise FileNotFoundError(f"{CKPT_ENV}={path}: no such file (the feature extractor of task {task!r})")
    return path


def load_feature_extractor(task, path=None):
    """The tower of ``task`` from the state dict at ``path`` (default: checkpoint_path(task)), frozen, in eval mode, on the host."""
    import torch
    path = checkpoint_path(task) if path is None else path
    sd = torch.load(path, map_location="cpu", weights_only=True)
    if not isinstance(sd, dict) or not all(torch.is_tensor(v) for v in sd.values()):
        raise ValueError(f"{path}: a flat state dict of tensors expected")
    if task == "CLIP-B16":
        from fourm.utils.clip.model import build_visual
        return build_visual(sd)          # (a full CLIP dict with visual.* keys, or the visual tower's own)
    from fourm.utils.dinov2 import build_dinov2
    return build_dinov2(sd)


def feature_maps(task, extractor, images):
    """images (B, 3, H, W), already normalised -> the tokenizer's input, fp32: (B, D, nh, nw) patch features ('b (nh nw) d -> b d nh nw') for
    CLIP-B16 (return_final_tokens_no_cls) and DINOv2-B14 (x_norm_patchtokens), (B, D, 1, 1) for DINOv2-B14-global (x_norm_clstoken)."""
    import torch
    if task not in FEATURE_TASKS:
        raise NotImplementedError(f"task {task!r}: the feature extractor tasks built here are {list(FEATURE_TASKS)}")
    B, _, H, W = images.shape
    with torch.no_grad():
        if task == "CLIP-B16":
            P = extractor.conv1.kernel_size[0]
            tok = extractor(images, return_final_tokens_no_cls=True)
        else:
            P = extractor.patch_embed.proj.kernel_size[0]
            out = extractor(images, is_training=True)
            if task.endswith("global"):
                return out["x_norm_clstoken"].unsqueeze(2).unsqueeze(2).contiguous()
            tok = out["x_norm_patchtokens"]
        nh, nw = H // P, W // P
        return tok.reshape(B, nh, nw, tok.shape[-1]).permute(0, 3, 1, 2).contiguous()
