"""FID and Inception score on the HIP engine: the fp32 FID-InceptionV3 tower (model.py), its kernels on tensors (ops.py) and the two metrics
(metrics.py).  INTEGRATION.md, "FID and Inception score"."""
from .metrics import FrechetInceptionDistance, InceptionScore, fid_from_moments
from .model import BN_EPS, UNITS, FidInceptionV3

__all__ = ["FidInceptionV3", "FrechetInceptionDistance", "InceptionScore", "fid_from_moments", "UNITS", "BN_EPS"]
