"""DINOv2's vision tower on the HIP engine (see model.py; parity with the `facebookresearch/dinov2` package and with the real checkpoints is
unpinned: the definition in INTEGRATION.md, "DINOv2 tower", is the contract)."""
from .model import (DinoVisionTransformer, build_dinov2, position_table, vit_base, vit_base_reg4, vit_giant2, vit_giant2_reg4, vit_large,
                    vit_large_reg4, vit_small, vit_small_reg4)

__all__ = ["DinoVisionTransformer", "build_dinov2", "position_table", "vit_small", "vit_base", "vit_large", "vit_giant2", "vit_small_reg4",
           "vit_base_reg4", "vit_large_reg4", "vit_giant2_reg4"]
