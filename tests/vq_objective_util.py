"""Float64 references and error bounds for the tokenizer training objective (fourm.vq.training, csrc/train_objective.hip).

The references are upstream's expressions (run_training_vqvae.py:961-1003) written against torch's own F.* functions, evaluated in float64 on
the CPU on the same fp32 inputs, with the gradient from torch's autograd.  The bounds are first-order bounds of the kernels' fp32 arithmetic,
built from float64 quantities only, doubled for the second-order terms; U = 2^-24 is the fp32 unit roundoff and a chain of n fp32 additions
errs by at most n U sum |terms|.  Nothing here looks at what the kernels return.

Summation depth of a loss value: a term passes through at most 16 sequential additions in its thread, 6 + 3 in the workgroup (shuffle tree, the
four wavefronts), ceil(parts / 256) + 6 + 3 in the final launch: DEPTH(parts) = 40 + parts / 256 covers every mode."""
import torch
import torch.nn.functional as F

U = 2.0 ** -24
ETA = 2.0 ** -126          # fp32 values below the normal range may be flushed to zero

LOSS_FNS = ("mse", "l1", "smooth_l1", "cross_entropy", "binary_cross_entropy", "cosine", "cosine_1d")
SHAPES = [(2, 3, 8, 8), (3, 5, 7, 9), (4, 6, 1, 1), (2, 70, 33, 31)]


def gen(seed):
    return torch.Generator().manual_seed(seed)


def reference_loss(x, target, loss_fn):
    """upstream's compute_reconst_loss on whatever dtype it is given (float64 here)."""
    if loss_fn == "mse":
        return F.mse_loss(x, target)
    if loss_fn == "l1":
        return F.l1_loss(x, target)
    if loss_fn == "smooth_l1":
        return F.smooth_l1_loss(x, target)
    if loss_fn == "cross_entropy":
        return F.cross_entropy(x, target)
    if loss_fn == "cosine":
        return 1 - F.cosine_similarity(x.flatten(2), target.flatten(2), dim=-1).mean()
    if loss_fn == "cosine_1d":
        return 1 - F.cosine_similarity(x.flatten(2), target.flatten(2), dim=1).mean()
    if loss_fn == "binary_cross_entropy":
        s = torch.sigmoid(x)
        return F.cross_entropy(torch.cat([s, 1 - s], dim=1), torch.cat([target, 1 - target], dim=1))
    raise ValueError(loss_fn)


def reference(x, target, loss_fn):
    """-> (loss, d loss / d x) in float64 from fp32 (or int64) CPU inputs."""
    xd = x.double().requires_grad_(True)
    td = target if loss_fn == "cross_entropy" else target.double()
    loss = reference_loss(xd, td, loss_fn)
    grad, = torch.autograd.grad(loss, xd)
    return loss.detach(), grad


def make_inputs(loss_fn, shape, seed, K=None):
    """fp32 CPU (model_output, target) of a mode.  l1 / smooth_l1 get some exactly equal elements (sign(0) = 0) and differences on both sides of
    1; the cosine modes one all-zero row of model_output (row 0 along the reduced axis)."""
    g = gen(seed)
    B, C, H, W = shape
    x = torch.randn(shape, generator=g)
    if loss_fn == "cross_entropy":
        return x, torch.randint(0, C, (B, H, W), generator=g)
    if loss_fn == "binary_cross_entropy":
        return 2.0 * x, torch.rand(shape, generator=g)
    t = torch.randn(shape, generator=g)
    if loss_fn in ("l1", "smooth_l1"):
        same = torch.rand(shape, generator=g) < 0.1
        t = torch.where(same, x, t)
    if loss_fn == "cosine":
        x[0, 0] = 0.0
    if loss_fn == "cosine_1d":
        x[0, :, 0, 0] = 0.0
    return x, t


def parts_of(loss_fn, shape):
    B, C, H, W = shape
    if loss_fn in ("mse", "l1", "smooth_l1"):
        return -(-B * C * H * W // 4096)
    if loss_fn == "cosine":
        return -(-B * C // 4)
    return -(-B * H * W // 256)


def depth(parts):
    return 40 + parts / 256


def _cos_bounds(x, t, dim, n_rows, D):
    """Cosine modes: dot, |x|^2, |t|^2 are chains of at most L + 8 additions over the reduced axis (L its length; sequential per thread or per
    lane plus the shuffle tree); sqrt, the clamp-free product of the norms and its reciprocal add 4 U, the product with the dot 1 U:
        E_cos = (L + 8) U (sum |x t| / (|x| |t|) + |cos|) + 6 U |cos|
    loss = 1 - mean cos: mean E_cos + D U mean |cos| + 3 U (1 + |loss|).
    gradient (b x - a t) / R with a = 1 / (|x| |t|), b = cos / |x|^2: |x| (E_cos + (L + 12) U |cos|) / |x|^2 + (L + 14) U |a t| + 4 U (|b x| + |a t|),
    over R.  Norms are clamped at eps = 1e-8 as the installed torch does; gradients are only compared on rows of norm >= 1e-3."""
    x, t = x.double(), t.double()
    L = x.shape[dim]
    nx = x.norm(dim=dim, keepdim=True).clamp_min(1e-8)
    nt = t.norm(dim=dim, keepdim=True).clamp_min(1e-8)
    cos = (x * t).sum(dim, keepdim=True) / (nx * nt)
    mag = (x * t).abs().sum(dim, keepdim=True) / (nx * nt)
    E_cos = (L + 8) * U * (mag + cos.abs()) + 6 * U * cos.abs()
    loss = 1 - cos.mean()
    loss_tol = 2 * (E_cos.mean() + D * U * cos.abs().mean() + 3 * U * (1 + loss.abs()))
    a, b = 1 / (nx * nt), cos / nx ** 2
    grad_tol = 2 * (x.abs() * (E_cos + (L + 12) * U * cos.abs()) / nx ** 2 + (L + 14) * U * (a * t).abs() + 4 * U * ((b * x).abs() + (a * t).abs())) / n_rows
    live = (x.norm(dim=dim, keepdim=True) >= 1e-3).expand_as(x)
    return loss_tol, grad_tol, live


def bounds(x, target, loss_fn):
    """-> (loss_tol (0-dim), grad_tol (x's shape), live (bool mask of the gradient elements that are compared)); see the docstrings of the tests."""
    B, C = x.shape[0], x.shape[1]
    D = depth(parts_of(loss_fn, tuple(x.shape)))
    xd = x.double()
    live = torch.ones_like(xd, dtype=torch.bool)
    if loss_fn in ("mse", "l1", "smooth_l1"):
        n = xd.numel()
        d = xd - target.double()
        a = d.abs()
        if loss_fn == "mse":          # d rounds by U |d|, d * d by U: 3 U d^2 per term; gradient 2 d / n: d, the product, 1 / n and its float(n): 4 U |g|
            term, e_term, g_tol = d * d, 3 * U * d * d, 4 * U * (2 * a / n)
        elif loss_fn == "l1":         # |d|: U |d|; gradient +- 1 / n: 2 U / n
            term, e_term, g_tol = a, U * a, 2 * U * torch.ones_like(a) / n
        else:                         # 0.5 d^2 or |d| - 0.5: 3 U (term + |d|); gradient d / n or +- 1 / n: 4 U |g|, + U / n where rounding moves |d| across 1
            term = torch.where(a < 1, 0.5 * d * d, a - 0.5)
            e_term, g_tol = 3 * U * (term + a), (4 * U * torch.minimum(a, torch.ones_like(a)) + U) / n
        loss = term.mean()
        return 2 * (e_term.mean() + D * U * term.mean() + 3 * U * loss.abs()), 2 * g_tol, live
    if loss_fn == "cosine":
        lt, gt, lv = _cos_bounds(x.flatten(2), target.flatten(2), 2, B * C, D)
        return lt, gt.reshape(x.shape), lv.reshape(x.shape)
    if loss_fn == "cosine_1d":
        lt, gt, lv = _cos_bounds(x.flatten(2), target.flatten(2), 1, B * x[0, 0].numel(), D)
        return lt, gt.reshape(x.shape), lv.reshape(x.shape)
    if loss_fn == "cross_entropy":
        # as tests/test_fp32_kernels_gpu.py::test_cross_entropy_f32, with K sequential terms in the sum of exponentials:
        #   E_lse = 2 (sum_c e_c (|t_c| + 3) U / sum_c e_c + (K + 10) U + 2 U |log S| + 2 U |lse|);  loss_pix = lse - x_l: E_lse + U |loss_pix|
        #   d = (exp(x - lse) - onehot) / count: (p (E_lse + (|x - lse| + 3) U) + U |p - onehot|) / count + 4 U |d| + ETA
        K = C
        valid = (target != -100)
        m = xd.amax(1, keepdim=True)
        e = torch.exp(xd - m)
        S = e.sum(1, keepdim=True)
        lse = m + S.log()
        E_lse = 2 * ((e * ((xd - m).abs() + 3)).sum(1, keepdim=True) * U / S + (K + 10) * U + 2 * U * S.log().abs() + 2 * U * lse.abs())
        lab = target.clamp(0, K - 1).unsqueeze(1)
        loss_pix = (lse - xd.gather(1, lab)) * valid.unsqueeze(1)
        cnt = max(int(valid.sum()), 1)
        E_pix = (E_lse + U * loss_pix.abs()) * valid.unsqueeze(1)
        loss = loss_pix.sum() / cnt
        loss_tol = E_pix.sum() / cnt + D * U * loss_pix.abs().sum() / cnt + 3 * U * loss.abs()
        p = torch.exp(xd - lse)
        p_oh = p - F.one_hot(lab.squeeze(1), K).movedim(-1, 1)
        g_tol = ((p * (E_lse + ((xd - lse).abs() + 3) * U) + U * p_oh.abs()) / cnt + 4 * U * p_oh.abs() / cnt + ETA) * valid.unsqueeze(1)
        return loss_tol, g_tol, live
    if loss_fn == "binary_cross_entropy":
        # s = 1 / (1 + exp(-x)) and u = 1 - s: absolute errors <= 5 U and 6 U (expf 3 U, the sum, the reciprocal, the difference); dz = 6 U for both.
        #   exp(z) with z in [0, 1]: relative dz + 3 U = 9 U; S = the 2 C of them added in order: relative (9 + 2 C) U;
        #   E_lse = (9 + 2 C) U + 3 U |lse|  (logf 2 U);   A = sum_k q_k z_k: E_A = sum_k |q_k| (dz + 2 U) + 2 C U + 2 C U sum_k |q_k z_k|
        #   loss_pix = C lse - A: E_pix = C E_lse + E_A + 2 U (C |lse| + |A|)
        #   p_k = exp(z_k - lse): relative rp = dz + E_lse + 4 U;  g_k = C p_k - q_k: C p_k (rp + U) + U |q_k| + U |g_k|
        #   d / d x = (g_c - g_{C + c}) s u / N: (dg1 + dg2 + U |g1 - g2|) s u + |g1 - g2| (5 U u + 6 U s + U s u), over N, + 4 U |d|
        td = target.double()
        N = xd.numel() // C
        s = torch.sigmoid(xd)
        u = 1 - s
        z = torch.cat([s, u], 1)
        q = torch.cat([td, 1 - td], 1)
        dz = 6 * U
        lse = torch.logsumexp(z, 1, keepdim=True)
        E_lse = (9 + 2 * C) * U + 3 * U * lse.abs()
        A = (q * z).sum(1, keepdim=True)
        E_A = q.abs().sum(1, keepdim=True) * (dz + 2 * U) + 2 * C * U + 2 * C * U * (q * z).abs().sum(1, keepdim=True)
        loss_pix = C * lse - A
        E_pix = C * E_lse + E_A + 2 * U * (C * lse.abs() + A.abs())
        loss = loss_pix.mean()
        loss_tol = 2 * (E_pix.mean() + D * U * loss_pix.abs().mean() + 3 * U * loss.abs())
        p = torch.exp(z - lse)
        gk = C * p - q
        dgk = C * p * (dz + E_lse + 5 * U) + U * q.abs() + U * gk.abs()
        g1, g2, dg1, dg2 = gk[:, :C], gk[:, C:], dgk[:, :C], dgk[:, C:]
        gs = g1 - g2
        d_su = 5 * U * u + 6 * U * s + U * s * u
        want = gs * s * u / N
        g_tol = 2 * (((dg1 + dg2 + U * gs.abs()) * s * u + gs.abs() * d_su) / N + 4 * U * want.abs())
        return loss_tol, g_tol, live
    raise ValueError(loss_fn)


def bce_closed_form(x, target, sum_q):
    """d loss / d x of upstream's binary_cross_entropy in float64 by the chain rule, with the softmax gradient (sum_q p_k - q_k) / N: sum_q = C is
    the formulation's own (its 2 C target probabilities add up to C), sum_q = 1 what a softmax over proper probabilities would give."""
    xd, td = x.double(), target.double()
    C, N = xd.shape[1], xd.numel() // xd.shape[1]
    s = torch.sigmoid(xd)
    z = torch.cat([s, 1 - s], 1)
    q = torch.cat([td, 1 - td], 1)
    gk = (sum_q * torch.softmax(z, 1) - q) / N
    return (gk[:, :C] - gk[:, C:]) * s * (1 - s)


def within(name, got, ref, tol, live=None):
    err = (got.detach().double().cpu() - ref.double()).abs()
    tol = tol.double().expand_as(err)
    bad = ~(err <= tol)
    if live is not None:
        bad = bad & live
    worst = float((err / (tol + 1e-300))[live if live is not None else torch.ones_like(bad)].max()) if err.numel() else 0.0
    assert not bool(bad.any()), f"{name}: {int(bad.sum())} of {err.numel()} outside the bound, worst err/tol {worst:.3g}"
    return worst
