"""Frechet Inception distance and Inception score on the HIP engine: the numbers upstream's ``run_generation.py`` (:668-694) and the tokenizer
trainers' ``eval_metrics`` judge generators and image tokenizers by, where they come from torchmetrics.  The definitions below (INTEGRATION.md,
"FID and Inception score") are the contract; torchmetrics / torch-fidelity are not dependencies and parity with them - and with the published
Inception checkpoint - is NOT pinned.

Both follow the ``update`` / ``compute`` / ``reset`` / ``.to`` pattern of ``fourm.vq.metrics``.  ``update`` never synchronises with the host;
``compute`` is where a number is asked for.  The FID state is ADDITIVE and lives in public device tensors (``real_sum`` f64 (d,),
``real_outer`` f64 (d, d), ``real_n`` int64 (1,), and ``fake_*``): a multi-rank caller all-reduces (sums) the six tensors before ``compute``;
nothing here talks to a process group (``sync_on_compute`` / ``compute_on_cpu`` are accepted and touch nothing).  There is no CPU path."""
import torch

from . import ops
from .model import FidInceptionV3

__all__ = ["FrechetInceptionDistance", "InceptionScore", "fid_from_moments"]

_IGNORED = ("sync_on_compute", "compute_on_cpu", "dist_sync_on_step", "process_group", "dist_sync_fn", "compute_with_cache")


def _common(kw, what):
    bad = [k for k in kw if k not in _IGNORED]
    if bad:
        raise TypeError(f"{what}: unexpected keyword argument(s) {', '.join(sorted(bad))}")


def _features_arg(feats, what):
    if not torch.is_tensor(feats):
        raise TypeError(f"{what}: a feature tensor is expected, got {type(feats).__name__}")
    if feats.dtype != torch.float32:
        raise TypeError(f"{what}: fp32 features expected, got {feats.dtype}")
    if feats.dim() != 2 or feats.shape[1] < 1:
        raise ValueError(f"{what}: features (n, d) expected, got {tuple(feats.shape)}")
    if not feats.is_cuda:
        raise RuntimeError(f"{what}: the features are on {feats.device}; the metric runs on the HIP kernels only (there is no CPU path)")
    feats = feats.detach()
    return feats if feats.stride(1) == 1 and feats.stride(0) >= feats.shape[1] else feats.contiguous()


def fid_from_moments(sum1, outer1, n1, sum2, outer2, n2):
    """FID from the additive moments, in float64 on the host:  mu = sum / n,  S = (outer - n mu mu^T) / (n - 1),
    FID = |mu1 - mu2|^2 + tr S1 + tr S2 - 2 sum(sqrt(eigvals(S1 S2)).real).  -> a 0-dim float64 tensor."""
    n1, n2 = int(n1), int(n2)
    if n1 < 2 or n2 < 2:
        raise RuntimeError(f"FrechetInceptionDistance: at least 2 samples on either side are needed (real {n1}, fake {n2})")
    stats = []
    for s, o, n in ((sum1, outer1, n1), (sum2, outer2, n2)):
        s, o = s.detach().double().cpu(), o.detach().double().cpu()
        mu = s / n
        stats.append((mu, (o - n * torch.outer(mu, mu)) / (n - 1)))
    (mu1, S1), (mu2, S2) = stats
    ev = torch.linalg.eigvals(S1 @ S2)
    d = mu1 - mu2
    return (d * d).sum() + torch.trace(S1) + torch.trace(S2) - 2.0 * torch.sqrt(ev).real.sum()


class FrechetInceptionDistance:
    def __init__(self, feature=2048, reset_real_features=True, normalize=False, inception=None, **kw):
        """Upstream's keywords verbatim.  ``feature``: 2048 (the pool features; 64 / 192 / 768 are not built) or a ``FidInceptionV3``;
        ``inception``: the ``FidInceptionV3`` ``update`` runs (None: only ``update_features`` is available)."""
        _common(kw, "FrechetInceptionDistance")
        if isinstance(feature, FidInceptionV3):
            feature, inception = 2048, feature
        if isinstance(feature, bool) or not isinstance(feature, int):
            raise TypeError(f"FrechetInceptionDistance: feature={feature!r}: 2048 or a FidInceptionV3 is expected")
        if feature != 2048:
            raise ValueError(f"FrechetInceptionDistance: feature={feature} is not built (2048, the pool features, only)")
        if inception is not None and not isinstance(inception, FidInceptionV3):
            raise TypeError("FrechetInceptionDistance: inception must be a fourm.utils.inception.FidInceptionV3")
        self.feature, self.inception = feature, inception
        self.reset_real_features, self.normalize = bool(reset_real_features), bool(normalize)
        self.real_sum = self.real_outer = self.real_n = self.fake_sum = self.fake_outer = self.fake_n = None

    _STATE = ("real_sum", "real_outer", "real_n", "fake_sum", "fake_outer", "fake_n")

    def _alloc(self, d, dev):
        for side in ("real", "fake"):
            setattr(self, f"{side}_sum", torch.zeros(d, dtype=torch.float64, device=dev))
            setattr(self, f"{side}_outer", torch.zeros(d, d, dtype=torch.float64, device=dev))
            setattr(self, f"{side}_n", torch.zeros(1, dtype=torch.int64, device=dev))

    def update(self, imgs, real):
        """imgs (B, 3, H, W): uint8, or fp32 in [0, 1] when ``normalize``; ``real``: which side they belong to."""
        if self.inception is None:
            raise RuntimeError("FrechetInceptionDistance.update needs the tower (inception=FidInceptionV3); update_features takes features")
        with torch.no_grad():
            self.update_features(self.inception(imgs, normalize=self.normalize)["pool"], real)

    def update_features(self, feats, real):
        """feats (n, d) fp32 on the GPU, any width d (the first call fixes it)."""
        feats = _features_arg(feats, "FrechetInceptionDistance.update_features")
        d = feats.shape[1]
        if d > 4096:
            raise ValueError(f"FrechetInceptionDistance: feature width {d} exceeds FM_MOMENTS_MAX_D = 4096")
        if self.real_sum is None:
            self._alloc(d, feats.device)
        elif self.real_sum.shape[0] != d:
            raise ValueError(f"FrechetInceptionDistance: features of width {d}, the state holds width {self.real_sum.shape[0]}")
        elif self.real_sum.device != feats.device:
            self.to(feats.device)
        side = "real" if real else "fake"
        ops.feature_moments(feats, getattr(self, f"{side}_sum"), getattr(self, f"{side}_outer"), getattr(self, f"{side}_n"))

    def reset(self):
        for name in self._STATE:
            t = getattr(self, name)
            if t is not None and (self.reset_real_features or name.startswith("fake")):
                t.zero_()

    def to(self, device):
        """Moves the accumulated state (the tower is the caller's)."""
        for name in self._STATE:
            t = getattr(self, name)
            if t is not None:
                setattr(self, name, t.to(device))
        return self

    def compute(self):
        """The FID of everything seen since ``reset`` as a 0-dim fp32 tensor: the one host synchronisation, float64 on the host."""
        if self.real_sum is None:
            raise RuntimeError("FrechetInceptionDistance: at least 2 samples on either side are needed (nothing was seen)")
        return fid_from_moments(self.real_sum, self.real_outer, self.real_n.item(), self.fake_sum, self.fake_outer, self.fake_n.item()).float()


class InceptionScore:
    def __init__(self, feature="logits_unbiased", splits=10, normalize=False, inception=None, generator=None, **kw):
        """Upstream's keywords verbatim.  ``feature``: ``"logits_unbiased"`` or a ``FidInceptionV3``; ``generator``: the CPU
        ``torch.Generator`` the permutation of ``compute`` is drawn from (None: the global one)."""
        _common(kw, "InceptionScore")
        if isinstance(feature, FidInceptionV3):
            feature, inception = "logits_unbiased", feature
        if feature != "logits_unbiased":
            raise ValueError(f"InceptionScore: feature={feature!r} is not built ('logits_unbiased' only)")
        if isinstance(splits, bool) or not isinstance(splits, int) or splits < 1:
            raise ValueError(f"InceptionScore: splits={splits!r}: an integer >= 1 is expected")
        if inception is not None and not isinstance(inception, FidInceptionV3):
            raise TypeError("InceptionScore: inception must be a fourm.utils.inception.FidInceptionV3")
        self.feature, self.splits, self.normalize, self.inception, self.generator = feature, splits, bool(normalize), inception, generator
        self.features, self.n = None, 0

    def update(self, imgs):
        if self.inception is None:
            raise RuntimeError("InceptionScore.update needs the tower (inception=FidInceptionV3); update_features takes logits")
        with torch.no_grad():
            self.update_features(self.inception(imgs, normalize=self.normalize)["logits_unbiased"])

    def update_features(self, logits):
        """logits (n, classes) fp32 on the GPU, appended to a device buffer that doubles (``features[:n]`` are the rows seen)."""
        logits = _features_arg(logits, "InceptionScore.update_features")
        m, c = logits.shape
        if self.features is not None and self.features.shape[1] != c:
            raise ValueError(f"InceptionScore: logits of width {c}, the buffer holds width {self.features.shape[1]}")
        if self.features is not None and self.features.device != logits.device:
            self.to(logits.device)
        cap = 0 if self.features is None else self.features.shape[0]
        if self.n + m > cap:
            buf = torch.empty(max(self.n + m, 2 * cap), c, dtype=torch.float32, device=logits.device)
            if self.n:
                buf[:self.n].copy_(self.features[:self.n])
            self.features = buf
        self.features[self.n:self.n + m].copy_(logits)
        self.n += m

    def reset(self):
        self.n = 0

    def to(self, device):
        if self.features is not None:
            self.features = self.features.to(device)
        return self

    def compute(self):
        """(mean, std) over ``splits`` chunks of the permuted rows of exp(mean_i sum_c p (log p - log mean_i p)), 0-dim fp32 tensors; the
        arithmetic is float64.  The std is the unbiased one (nan with one split)."""
        if self.n == 0:
            raise RuntimeError("InceptionScore: nothing was seen")
        idx = torch.randperm(self.n, generator=self.generator)
        x = self.features[:self.n][idx.to(self.features.device)].double()
        prob, log_prob = x.softmax(dim=1), x.log_softmax(dim=1)
        scores = []
        for p, lp in zip(prob.chunk(self.splits, dim=0), log_prob.chunk(self.splits, dim=0)):
            mean_p = p.mean(dim=0, keepdim=True)
            scores.append((p * (lp - mean_p.log())).sum(dim=1).mean().exp())
        scores = torch.stack(scores)
        return scores.mean().float(), scores.std().float()
