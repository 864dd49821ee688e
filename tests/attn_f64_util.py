"""Float64 reference, per-element error bounds, mask builders and a CPU emulation of the bf16 attention kernels
(``csrc/attention.hip``: fm_attn_fwd / fm_attn_bwd).  Importable without a GPU; every function runs on the device of its inputs.

Layout: q / k / v / o / dO are 2-D ``(B * N, >= 64 H)`` row-major tensors (row ``b * N + t``, head h in columns [64 h, 64 h + 64)), as
the kernels take them; the reference works on ``(B, H, N, 64)`` float64 views of them.  ``blocked`` is a ``(B, Nq, Nk)`` bool tensor
(or None), shared by the heads.

The reference forward is the definition (scores -> masked_fill(-finfo(bf16).max) -> softmax / softmax1 -> @ v) in float64 from the
bf16 inputs.  The reference backward is the float64 value of the function fm_attn_bwd is specified to compute from ITS inputs
(q, k, v, o, dO, stat_m, stat_l): the forward tests prove o / m / l, the backward tests then take them as given.

The emulation restates the kernels' rounding points in torch on the CPU (fp32 matmul accumulation, P and dS through bf16, outputs
through bf16).  It validates the bounds (tests/test_attention_ref_cpu.py) and is NOT the reference.
"""
import math
from dataclasses import dataclass, field
from typing import Optional

import torch

HD = 64
NEG_FILL = -float(torch.finfo(torch.bfloat16).max)       # what a blocked score is replaced by (attention.hip: NEG_FILL)
LOG2E = 1.4426950408889634
LN2 = math.log(2.0)
U = 2.0 ** -24                                           # fp32 unit roundoff
U_BF = 2.0 ** -8                                         # bf16: 8 significant bits, round to nearest is within 2^-8 relative
FLUSH = 2.0 ** -125                                      # absolute floor: an fp32 value below 2^-126 (v_exp_f32 result, MFMA operand) may be flushed to zero


def heads(x2d, B, N, H):
    """(B * N, >= 64 H) -> (B, H, N, 64) float64."""
    return x2d[:, :H * HD].reshape(B, N, H, HD).permute(0, 2, 1, 3).double()


def unheads(x4d):
    """(B, H, N, 64) -> (B * N, 64 H)."""
    B, H, N, _ = x4d.shape
    return x4d.permute(0, 2, 1, 3).reshape(B * N, H * HD)


# ------------------------------------------------------------------------------------------------
# masks
# ------------------------------------------------------------------------------------------------
@dataclass
class Mask:
    kind: str                                            # none | keypad | decoder | dense   (the kernel's mask kind)
    causal: bool = False
    kpad: Optional[torch.Tensor] = None                  # (B, Nk) bool
    cs: Optional[torch.Tensor] = None                    # (B, Nq) int32
    modq: Optional[torch.Tensor] = None                  # (B, Nq) int16
    modk: Optional[torch.Tensor] = None                  # (B, Nk) int16
    dense: Optional[torch.Tensor] = None                 # (B, Nq, Nk) bool
    blocked: Optional[torch.Tensor] = field(default=None, repr=False)      # (B, Nq, Nk) bool: the rule spelled out

    def to(self, dev):
        mv = lambda t: None if t is None else t.to(dev)
        return Mask(self.kind, self.causal, mv(self.kpad), mv(self.cs), mv(self.modq), mv(self.modk), mv(self.dense), mv(self.blocked))


def largest_modality_id():
    """The largest modality id fourm/data/modality_info.py defines (ids are 15-bit hashes of the modality names)."""
    from fourm.data.modality_info import MODALITY_INFO
    return max(int(v["id"]) for v in MODALITY_INFO.values())


def decoder_blocked(cs, modq, modk, Nq, Nk, causal=False, off_by_one=False):
    """blocked[b][q][k] = k >= cs[b][q] || modq[b][q] != modk[b][k]  (causal: k > q).  off_by_one: the WRONG rule k > cs (a mutation)."""
    B = (cs if cs is not None else modq).shape[0] if (cs is not None or modq is not None) else 1
    kk = torch.arange(Nk)[None, None, :]
    if causal:
        blk = (kk > torch.arange(Nq)[None, :, None]).expand(B, Nq, Nk).clone()
    elif cs is not None:
        blk = (kk > cs[:, :, None].long()) if off_by_one else (kk >= cs[:, :, None].long())
    else:
        blk = torch.zeros(B, Nq, Nk, dtype=torch.bool)
    if modq is not None:
        blk = blk | (modq[:, :, None] != modk[:, None, :])
    return blk


def make_mask(variant, B, Nq, Nk, seed):
    """The mask fixtures (all on the CPU):
      none
      keypad       30 % of the keys padded; sample 0 has EVERY key padded (a whole fully blocked sample); in the other samples at least
                   one key is padded (blocked for every query) and one is not
      dec          the decoder rule with cs and modalities: cs = cumsum of a sparse 0..3 mask, so the leading rows have cs = 0 (fully
                   blocked); in the last sample the increments are tripled so cs passes Nk, and its last row holds 5000 (beyond every
                   clamp of the packed forms); modality ids from {1, 7, 300, the largest defined id}, sorted per sample
      dec_nomod    cs alone (modq = modk = None)
      dec_modonly  modalities alone (cs = None)
      causal       k > q
      dense        40 % blocked at random; rows 0, 5 and the last one fully blocked in every sample; keys 1 and the last one blocked for
                   every query
    """
    g = torch.Generator().manual_seed(seed)
    if variant == "none":
        return Mask("none")
    if variant == "keypad":
        kp = torch.rand(B, Nk, generator=g) < 0.3
        kp[0] = True
        for b in range(1, B):
            kp[b, int(torch.randint(0, Nk, (1,), generator=g))] = False
            if Nk > 1:
                free = (~kp[b]).nonzero().flatten()
                cand = [i for i in range(Nk) if i != int(free[0])]
                kp[b, cand[int(torch.randint(0, len(cand), (1,), generator=g))]] = True
        return Mask("keypad", kpad=kp, blocked=kp[:, None, :].expand(B, Nq, Nk).clone())
    if variant == "causal":
        return Mask("decoder", causal=True, blocked=decoder_blocked(None, None, None, Nq, Nk, causal=True).expand(B, Nq, Nk).clone())
    if variant in ("dec", "dec_nomod", "dec_modonly"):
        dam = (torch.rand(B, Nq, generator=g) < 0.5).int() * torch.randint(1, 4, (B, Nq), generator=g).int()
        dam[:, :min(3, Nq)] = 0
        dam[B - 1] *= 3
        cs = dam.cumsum(-1).int()
        cs[B - 1, Nq - 1] = 5000
        ids = torch.tensor([1, 7, 300, largest_modality_id()], dtype=torch.int16)
        modq = ids[torch.randint(0, 4, (B, Nq), generator=g)].sort(-1).values
        modk = modq.clone() if Nq == Nk else ids[torch.randint(0, 4, (B, Nk), generator=g)].sort(-1).values
        if variant == "dec_nomod":
            modq = modk = None
        if variant == "dec_modonly":
            cs = None
        return Mask("decoder", cs=cs, modq=modq, modk=modk, blocked=decoder_blocked(cs, modq, modk, Nq, Nk))
    if variant == "dense":
        d = torch.rand(B, Nq, Nk, generator=g) < 0.4
        for r in {0, min(5, Nq - 1), Nq - 1}:
            d[:, r, :] = True
        for c in {min(1, Nk - 1), Nk - 1}:
            d[:, :, c] = True
        return Mask("dense", dense=d, blocked=d.clone())
    raise ValueError(variant)


# ------------------------------------------------------------------------------------------------
# inputs
# ------------------------------------------------------------------------------------------------
def make_inputs(B, H, Nq, Nk, seed, ramp="flat", kpad=None):
    """q, k, v, dO ~ N(0, 1.5^2) rounded to bf16, as contiguous (B * N, 64 H) CPU tensors.
    ramp = rise / fall: the K rows are scaled geometrically from 1/16 to 4 (or 4 to 2^-20) along the key index - rising, the running maximum
    of the online softmax moves in every key tile; falling, it is met in the first tile and every later rescale factor is exactly 1.
    kpad: the padded keys' V rows hold 1e4 and their K rows are 4 x larger - a leak is far outside any bound, the reference does not move."""
    g = torch.Generator().manual_seed(seed)
    D = H * HD
    q = torch.randn(B * Nq, D, generator=g) * 1.5
    k = torch.randn(B * Nk, D, generator=g) * 1.5
    v = torch.randn(B * Nk, D, generator=g) * 1.5
    do = torch.randn(B * Nq, D, generator=g) * 1.5
    if ramp != "flat":
        x = torch.arange(Nk, dtype=torch.float64) / max(Nk - 1, 1)
        f = (2.0 ** (-4 + 6 * x)) if ramp == "rise" else (2.0 ** (2 - 22 * x))
        k = (k.reshape(B, Nk, D) * f.float()[None, :, None]).reshape(B * Nk, D)
    if kpad is not None:
        kp = kpad.reshape(B * Nk)
        k[kp] *= 4.0
        v[kp] = 1e4
    return q.bfloat16(), k.bfloat16(), v.bfloat16(), do.bfloat16()


# ------------------------------------------------------------------------------------------------
# float64 reference
# ------------------------------------------------------------------------------------------------
def ref_forward(q, k, v, B, H, Nq, Nk, scale, blocked=None, zero_attn=False):
    """-> dict(O, P (B, H, Nq, Nk), m, l (B, H, Nq)) in float64.  m / l in the kernel's convention: m = row maximum of t = s * log2 e
    (a blocked t is REPLACED by -finfo(bf16).max: a fully blocked row has m = -finfo.max, P = 1 / Nk, l = Nk); zero_attn: one zero logit
    joins the maximum and the sum (m = max(m, 0), l += exp2(-m)) and its probability is dropped."""
    qh, kh, vh = heads(q, B, Nq, H), heads(k, B, Nk, H), heads(v, B, Nk, H)
    t = (qh @ kh.transpose(-1, -2)) * (scale * LOG2E)
    if blocked is not None:
        t = torch.where(blocked[:, None], torch.full_like(t, NEG_FILL), t)
    m = t.max(-1).values
    if zero_attn:
        m = m.clamp_min(0.0)
    p = torch.exp2(t - m[..., None])
    l = p.sum(-1)
    if zero_attn:
        l = l + torch.exp2(-m)
    P = p / l[..., None]
    return dict(O=P @ vh, P=P, m=m, l=l)


def ref_backward(q, k, v, o, do, m, l, B, H, Nq, Nk, scale, blocked=None):
    """float64 value of what fm_attn_bwd is specified to compute from its inputs.  m, l: (B, H, Nq).
    P = exp2(t - m) / l at unblocked scores; at blocked scores 0, or 1 / l in a row with m < -1e38 (the forward's fully-blocked marker);
    delta = sum_d dO o;  dV = P^T dO;  dS = P (dO V^T - delta), ZERO at every blocked score (masked_fill stops the gradient);
    dQ = scale dS K;  dK = scale dS^T Q.   -> dict(dQ, dK, dV, P, dS (unscaled), dPd = dO V^T - delta)."""
    qh, kh, vh = heads(q, B, Nq, H), heads(k, B, Nk, H), heads(v, B, Nk, H)
    oh, gh = heads(o, B, Nq, H), heads(do, B, Nq, H)
    m, l = m.double(), l.double()
    full = m < -1e38
    t = (qh @ kh.transpose(-1, -2)) * (scale * LOG2E)
    P = torch.exp2(t - torch.where(full, torch.zeros_like(m), m)[..., None]) / l[..., None]
    if blocked is not None:
        blk = blocked[:, None].expand_as(P)
        P = torch.where(blk, torch.where(full[..., None], 1.0 / l[..., None], torch.zeros_like(P)).expand_as(P), P)
    delta = (gh * oh).sum(-1)
    dPd = gh @ vh.transpose(-1, -2) - delta[..., None]
    dS = P * dPd
    if blocked is not None:
        dS = torch.where(blk, torch.zeros_like(dS), dS)
    return dict(dQ=scale * (dS @ kh), dK=scale * (dS.transpose(-1, -2) @ qh), dV=P.transpose(-1, -2) @ gh, P=P, dS=dS, dPd=dPd)


# ------------------------------------------------------------------------------------------------
# bounds: every term is one rounding point of attention.hip
# ------------------------------------------------------------------------------------------------
def _live(blocked, shape, dev):
    if blocked is None:
        return torch.ones(shape, dtype=torch.bool, device=dev)
    return (~blocked)[:, None].expand(shape)


def fwd_bounds(q, k, v, B, H, Nq, Nk, scale, ref, blocked=None):
    """-> tol_O (B, H, Nq, 64), tol_m, tol_l (B, H, Nq).  Every term of tol_O is proportional to a probability that is exactly 0.0 in
    float64 at a blocked score: where the reference is structurally zero the bound is exactly zero."""
    qh, kh, vh = heads(q, B, Nq, H), heads(k, B, Nk, H), heads(v, B, Nk, H)
    c2 = scale * LOG2E
    NT = (Nk + 63) // 64                                  # key tiles of the online softmax (64 keys; the tiled kernel's 128 give fewer)
    # exponent t - m of one score.  t: 64-term fp32 MFMA accumulation of exact bf16 products (64 u), c2 = fp32(scale log2 e) (u), the
    # product / FMA with it (u), the subtraction of the maximum (u): 67 u c2 sum_d |q_d k_d|, taken at the row's largest key since the
    # maximum is another key's score; the online softmax re-bases on m_run - m_new once per key tile (u |dm|, |dm| <= 2 max |t|): 2 NT u.
    eps_t = (67 + 2 * NT) * U * c2 * (qh.abs() @ kh.abs().transpose(-1, -2)).max(-1).values
    # probability before normalisation: the errors of t and of m both move the exponent (2 ln2 eps_t), v_exp_f32 is good to 1 ulp (2 u)
    eps_p = torch.expm1(2 * LN2 * eps_t) + 2 * U
    # row sum l: fp32 additions of Nk positive terms (Nk u); per key tile one exp2 (2 u), one multiply and one add (2 u) of the rescale;
    # softmax1 adds exp2(-m) through one more exp2, multiply and add (8 u with the final cross-lane add)
    eps_l = (Nk + 4 * NT + 8) * U
    # gamma: P = p / l carries eps_p twice (numerator, row sum) and eps_l; O accumulates Nk products in fp32 (Nk u) with the same per-tile
    # rescale (4 NT u), then one reciprocal-multiply (2 u)
    gamma = 2 * eps_p + eps_l + (Nk + 4 * NT + 2) * U
    live = _live(blocked, ref["P"].shape, ref["P"].device)
    # P is rounded to bf16 in front of the P V MFMA (U_BF) while l sums the unrounded values; FLUSH: a p below 2^-126 becomes 0
    eP = ref["P"] * (U_BF + gamma)[..., None] + FLUSH * live
    A = eP @ vh.abs()
    # the output is rounded to bf16 once: U_BF |O|, and (1 + U_BF): that rounding acts on the value that already carries A
    tol_O = U_BF * ref["O"].abs() + (1 + U_BF) * A + FLUSH * live.any(-1)[..., None]
    tol_m = eps_t                                         # the maximum of perturbed scores moves by at most the perturbation
    tol_l = (eps_l + eps_p) * ref["l"]
    return tol_O, tol_m, tol_l


def bwd_bounds(q, k, v, o, do, m, l, B, H, Nq, Nk, scale, ref, blocked=None):
    """-> tol_dQ (B, H, Nq, 64), tol_dK, tol_dV (B, H, Nk, 64) around ref_backward's values.  Exactly zero where the reference is
    structurally zero: dQ of a fully blocked query, dK of a key no query may see, dV of such a key unless a fully blocked row (P = 1 / l)
    sees it."""
    qh, kh, vh = heads(q, B, Nq, H), heads(k, B, Nk, H), heads(v, B, Nk, H)
    oh, gh = heads(o, B, Nq, H), heads(do, B, Nq, H)
    m, l = m.double(), l.double()
    c2 = scale * LOG2E
    full = m < -1e38
    lg = torch.log2(l).abs()
    # exponent of one probability.  DIET / 128 kernels: fma(s, c2, nm), nm = -(m + log2 l): the 64-term MFMA accumulation, c2 and the FMA
    # (67 u c2 sum_d |q_d k_d|, with |t| <= c2 sum_d |q_d k_d| inside the FMA's own rounding), v_log_f32 to 1 ulp and the fp32 sum
    # m + log2 l (2 u |m| + 4 u |log2 l| with the FMA's share of |nm|).  A fully blocked row selects pb = -log2 l alone (4 u |log2 l|).
    # The chunked kernel's exp2(s c2 - m) * (1 / l) has the same score terms and no logarithm.
    eps_e = U * (67 * c2 * (qh.abs() @ kh.abs().transpose(-1, -2)).max(-1).values + 2 * torch.where(full, torch.zeros_like(m), m.abs()) + 4 * lg)
    eps_e = torch.where(full, 4 * U * lg, eps_e)
    # probability: exponent error (ln2 eps_e), v_exp_f32 (2 u); chunked kernel: the reciprocal of l and two multiplies (4 u)
    eps_p = torch.expm1(LN2 * eps_e) + 6 * U
    P, dS, dPd = ref["P"], ref["dS"], ref["dPd"]
    live = _live(blocked, P.shape, P.device)
    Pu = P * live                                        # the probabilities that carry a gradient (zero at blocked scores, also in full rows)
    # dV = P^T dO: P rounded to bf16 (U_BF), its own error (eps_p), Nq-term fp32 MFMA accumulation ((Nq + 2) u); FLUSH as in the forward
    ePv = P * (U_BF + eps_p + (Nq + 2) * U)[..., None] + FLUSH * live
    tol_dV = U_BF * ref["dV"].abs() + (1 + U_BF) * (ePv.transpose(-1, -2) @ gh.abs()) + FLUSH * (P > 0).any(-2)[..., None]
    # dP - delta: dP is a 64-term fp32 MFMA accumulation of exact bf16 products, delta a 64-term fp32 dot of bf16 values (v_dot2c_f32_bf16
    # + cross-lane adds), one subtraction: 67 u (sum_d |dO V_k| + sum_d |dO o|)
    e_dpd = 67 * U * (gh.abs() @ vh.abs().transpose(-1, -2) + (gh.abs() * oh.abs()).sum(-1)[..., None])
    # dS = P (dP - delta) is rounded to bf16 in front of dS K / dS^T Q (U_BF), carries eps_p and the product's rounding (chunked kernel:
    # also the multiply by scale in front of the rounding; 3 u); FLUSH: p or dS below 2^-126 flushed
    e_dS = dS.abs() * (U_BF + eps_p + 3 * U)[..., None] + Pu * e_dpd + FLUSH * live * (1 + dPd.abs())
    # dK = scale dS^T Q: Nq-term fp32 accumulation and the multiply by scale at the store ((Nq + 2) u); dQ = scale dS K alike with Nk
    tol_dK = U_BF * ref["dK"].abs() + (1 + U_BF) * scale * ((e_dS + dS.abs() * (Nq + 2) * U).transpose(-1, -2) @ qh.abs()) + FLUSH * live.any(-2)[..., None]
    tol_dQ = U_BF * ref["dQ"].abs() + (1 + U_BF) * scale * ((e_dS + dS.abs() * (Nk + 2) * U) @ kh.abs()) + FLUSH * (live & ~full[..., None]).any(-1)[..., None]
    # (a fully blocked row has dS = 0 in every column, so e_dS = 0 there except through FLUSH * live, which `full` rows only have with
    # an unblocked key - then they are not full.  The explicit & ~full keeps the zero exact whatever m holds.)
    return tol_dQ, tol_dK, tol_dV


def within(name, got, ref, tol):
    """Every element of ``got`` within ``tol`` of ``ref`` (NaN fails); -> the worst err / tol.  The message names the first element outside."""
    err = (got.double() - ref).abs()
    tol = tol.expand_as(err)
    bad = ~(err <= tol)
    ratio = float(torch.where(err == 0, torch.zeros_like(err), err / (tol + 1e-300)).max()) if err.numel() else 0.0
    if bool(bad.any()):
        i = tuple(bad.nonzero()[0].tolist())
        raise AssertionError(f"{name}: {int(bad.sum())} of {bad.numel()} outside the bound, worst err/tol {ratio:.3g}, first at {i}: "
                             f"got {float(got[i])!r}, want {float(ref[i])!r} +- {float(tol[i]):.3g}")
    return ratio


# ------------------------------------------------------------------------------------------------
# CPU emulation of the kernels' rounding points (validates the bounds; not the reference)
# ------------------------------------------------------------------------------------------------
def _h32(x2d, B, N, H):
    return x2d[:, :H * HD].reshape(B, N, H, HD).permute(0, 2, 1, 3).float()


def emu_forward(q, k, v, B, H, Nq, Nk, scale, blocked=None, zero_attn=False, *, full_row_zero=False, zero_attn_not_in_l=False):
    """-> O (B * Nq, 64 H) bf16, m, l (B, H, Nq) fp32.  fp32 matmul for the MFMA accumulation, t = s * fp32(scale log2 e), exp2 in fp32,
    l from the unrounded p, P through bf16 in front of P V, O through bf16.  The keyword flags are deliberately WRONG variants."""
    qh, kh, vh = _h32(q, B, Nq, H), _h32(k, B, Nk, H), _h32(v, B, Nk, H)
    c2 = torch.tensor(scale * LOG2E, dtype=torch.float32)
    t = (qh @ kh.transpose(-1, -2)) * c2
    if blocked is not None:
        t = torch.where(blocked[:, None], torch.full_like(t, NEG_FILL), t)
    m = t.max(-1).values
    p = torch.exp2(t - m[..., None])
    l = p.sum(-1)
    acc = p.bfloat16().float() @ vh
    oscale = torch.ones_like(m)
    if zero_attn:
        m_fin = m.clamp_min(0.0)
        oscale = torch.exp2(m - m_fin)
        l = l * oscale if zero_attn_not_in_l else l * oscale + torch.exp2(-m_fin)
        m = m_fin
    O = acc * (oscale / l)[..., None]
    if full_row_zero and blocked is not None:
        O = torch.where(blocked.all(-1)[:, None, :, None], torch.zeros_like(O), O)
    return unheads(O.bfloat16()), m, l


def emu_backward(q, k, v, o, do, m, l, B, H, Nq, Nk, scale, blocked=None, *, ds_in_full_rows=False, no_delta=False, scale_twice_dk=False):
    """-> dQ, dK, dV (2-D bf16).  The DIET arithmetic: p = exp2(fma(s, c2, -(m + log2 l))) in fp32, a blocked score selects the exponent
    -inf (or -log2 l in a fully blocked row), delta from the ROUNDED o, P and dS through bf16, scale applied after the products."""
    qh, kh, vh = _h32(q, B, Nq, H), _h32(k, B, Nk, H), _h32(v, B, Nk, H)
    oh, gh = _h32(o, B, Nq, H), _h32(do, B, Nq, H)
    m, l = m.float(), l.float()
    c2 = torch.tensor(scale * LOG2E, dtype=torch.float32)
    full = (m < -1e38) if blocked is not None else torch.zeros_like(m, dtype=torch.bool)
    nm = torch.where(full, torch.zeros_like(m), -(m + torch.log2(l)))
    e = (qh @ kh.transpose(-1, -2)) * c2 + nm[..., None]
    blk = None
    if blocked is not None:
        blk = blocked[:, None].expand_as(e)
        pb = torch.where(full, -torch.log2(l), torch.full_like(l, -math.inf))
        e = torch.where(blk, pb[..., None].expand_as(e), e)
    p = torch.exp2(e)
    delta = torch.zeros_like(m) if no_delta else (gh * oh).sum(-1)
    ds = p * (gh @ vh.transpose(-1, -2) - delta[..., None])
    if blk is not None:
        keep = (blk & full[..., None]) if ds_in_full_rows else torch.zeros_like(blk)
        ds = torch.where(blk & ~keep, torch.zeros_like(ds), ds)
    dsb, pbf = ds.bfloat16().float(), p.bfloat16().float()
    dV = pbf.transpose(-1, -2) @ gh
    dK = (dsb.transpose(-1, -2) @ qh) * (scale * scale if scale_twice_dk else scale)
    dQ = (dsb @ kh) * scale
    return unheads(dQ.bfloat16()), unheads(dK.bfloat16()), unheads(dV.bfloat16())


# ------------------------------------------------------------------------------------------------
# the case table shared by the GPU test and the CPU validation of the bounds
# ------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Case:
    Nq: int
    Nk: int
    mask: str                     # make_mask variant
    tr: int                       # force_tr
    fwd: str                      # forward kernel reached (dispatch rule of fm_attn_fwd)
    bwd: str                      # backward kernel reached (dispatch rule of fm_attn_bwd); "-" = forward only
    zero_attn: bool = False
    ramp: str = "flat"
    o_layout: int = 0             # 0: rows 16-byte aligned; 1: ldo % 8 == 4; 2: first column 8 bytes off alignment (1, 2: o16 = wide_o = 0)
    g_layout: int = 0             # dq / dk / dv: 0 aligned, 1: ld % 8 == 4 (rows16 = 0)
    kvr: int = 0                  # kv_batch_rows (> Nk: a K/V cache, forward only)

    @property
    def id(self):
        s = f"{self.Nq}x{self.Nk}-{self.mask}-tr{self.tr}"
        s += "-z" if self.zero_attn else ""
        s += f"-{self.ramp}" if self.ramp != "flat" else ""
        s += f"-o{self.o_layout}" if self.o_layout else ""
        s += f"-g{self.g_layout}" if self.g_layout else ""
        s += f"-kvr{self.kvr}" if self.kvr else ""
        return s

    @property
    def math_key(self):           # cases with the same key have the same inputs, mask and reference
        return (self.Nq, self.Nk, self.mask, self.zero_attn, self.ramp)

    @property
    def seed(self):
        return 1000 * self.Nq + self.Nk


B, H = 2, 3
KINDS4 = ("none", "keypad", "dec", "dense")


def fwd_route(Nq, Nk, mask, tr):
    """The dispatch rule of fm_attn_fwd with no FOURM_ATTN_* variable set and scale > 0."""
    if tr and mask != "dense" and Nq == 128 and Nk == 128:
        return "attn_fwd128_kernel"
    if tr and mask != "dense" and Nq % 128 == 0 and Nk % 128 == 0 and Nk <= 512:
        return "attn_fwdt_kernel"
    return f"attn_fwd_kernel<{'true' if tr else 'false'},.>"


def bwd_route(Nq, Nk, mask, tr, g_layout):
    """The dispatch rule of fm_attn_bwd with no FOURM_ATTN_* variable set."""
    NqP, NkP = (Nq + 31) & ~31, (Nk + 31) & ~31
    NPmax = max(NqP, NkP)
    if tr and g_layout == 0 and Nq == 128 and Nk == 128 and mask != "dense":
        return "attn_bwd128o_kernel" if mask in ("dec", "dec_nomod", "dec_modonly", "causal") else "attn_bwd128_kernel"
    t = "true" if tr else "false"
    if NPmax > 512:
        return f"attn_bwd_kernel<{t},.,true,false>"
    if (NqP + 63) // 64 * NkP * 128 <= 32 * 1024:
        return f"attn_bwd_kernel<{t},.,false,true>"
    return f"attn_bwd_kernel<{t},.,false,false>"


def build_cases():
    out, seen = [], set()

    def add(Nq, Nk, mask, tr, *, bwd=True, **kw):
        bwd = bwd and not kw.get("o_layout") and not kw.get("kvr")
        for z in (False, True):
            c = Case(Nq, Nk, mask, tr, fwd_route(Nq, Nk, mask, tr), bwd_route(Nq, Nk, mask, tr, kw.get("g_layout", 0)) if bwd else "-",
                     zero_attn=z, **kw)
            if c.id not in seen:
                seen.add(c.id)
                out.append(c)

    decs = ("dec", "dec_nomod", "dec_modonly", "causal")
    # ---- 128 x 128, force_tr = 1 -----------------------------------------------------------------------------------------------
    for mk in ("none", "keypad") + decs:
        add(128, 128, mk, 1)                          # fwd: attn_fwd128_kernel (o16 = 1)   bwd: attn_bwd128_kernel (none -> the keypad instantiation with kpad = NULL, keypad) / attn_bwd128o_kernel (decoder, causal)
        add(128, 128, mk, 1, o_layout=1)              # fwd: attn_fwd128_kernel, o16 = 0 (ldo % 8 == 4)
    for mk in ("none", "keypad", "dec", "causal"):
        add(128, 128, mk, 1, g_layout=1)              # bwd: rows16 false -> attn_bwd_kernel<true,.,false,true>
    for mk in ("none", "keypad"):
        add(128, 128, mk, 1, o_layout=2)              # fwd: attn_fwd128_kernel, o16 = 0 (first column 8 bytes off)
    for mk in ("none", "keypad", "dec"):
        add(128, 128, mk, 1, kvr=160)                 # fwd: attn_fwd128_kernel on a K/V cache of 160 rows per sample
    add(128, 128, "none", 1, ramp="rise")
    add(128, 128, "none", 1, ramp="fall")
    # ---- 128 x 128 on the general kernels: force_tr = 0, and the dense mask for both ---------------------------------------------
    for mk in ("none", "keypad") + decs:
        add(128, 128, mk, 0)                          # fwd: attn_fwd_kernel<false,.>   bwd: attn_bwd_kernel<false,.,false,true> (DS)
    for tr in (1, 0):
        add(128, 128, "dense", tr)                    # fwd: attn_fwd_kernel<tr,DENSE>  bwd: attn_bwd_kernel<tr,DENSE,false,true> (DS)
    # ---- multiples of 128 up to 512 keys, force_tr = 1: the tiled forward ----------------------------------------------------------
    for Nq, Nk in ((256, 128), (128, 256), (128, 512)):
        for mk in ("none", "keypad"):
            add(Nq, Nk, mk, 1)                        # fwd: attn_fwdt_kernel   bwd: attn_bwd_kernel<true,.,false,false>
    for mk in ("none", "keypad"):
        add(256, 128, mk, 1, o_layout=1)              # fwd: attn_fwdt_kernel, o16 = 0
        add(128, 512, mk, 1, ramp="rise", bwd=False)  # fwd: attn_fwdt_kernel, the maximum moves in every 128-key tile
        add(128, 512, mk, 1, ramp="fall", bwd=False)  # fwd: attn_fwdt_kernel, alpha == 1 in every later tile
    for mk in ("dec", "dec_nomod", "causal"):
        add(256, 256, mk, 1)                          # fwd: attn_fwdt_kernel   bwd: attn_bwd_kernel<true,DECODER,false,false>
    add(256, 256, "dec", 1, o_layout=1)               # fwd: attn_fwdt_kernel, o16 = 0
    # ---- the general kernels, both transpose-read settings ---------------------------------------------------------------------------
    for tr in (1, 0):
        for Nq, Nk in ((1, 1), (33, 70), (64, 64)):
            for mk in KINDS4:
                add(Nq, Nk, mk, tr)                   # fwd: attn_fwd_kernel<tr,.>   bwd: attn_bwd_kernel<tr,.,false,true> (DS)
        for mk in ("causal", "dec_modonly"):
            add(64, 64, mk, tr)
        add(1, 1, "causal", tr)
        for mk in KINDS4:
            add(64, 256, mk, tr)                      # bwd: attn_bwd_kernel<tr,.,false,true> (DS, the largest key count it takes)
        add(64, 256, "none", tr, ramp="rise")         # fwd: attn_fwd_kernel, the maximum moves in every 64-key tile
        add(64, 256, "none", tr, ramp="fall")         # fwd: attn_fwd_kernel, the rescale is skipped in every later tile
        for mk in ("dec", "dec_nomod", "dec_modonly", "causal"):
            add(96, 96, mk, tr)                       # bwd: attn_bwd_kernel<tr,DECODER,false,true> (DS)
            add(160, 160, mk, tr)                     # bwd: attn_bwd_kernel<tr,DECODER,false,false>
        for Nq, Nk in ((160, 96), (130, 65), (512, 40)):
            for mk in KINDS4:
                add(Nq, Nk, mk, tr)                   # bwd: attn_bwd_kernel<tr,.,false,false> (one chunk, no dS^T)
        for mk in ("none", "keypad"):
            add(128, 640, mk, tr, bwd=False)          # fwd: attn_fwd_kernel<tr,.> (Nk > 512 leaves the tiled kernel)
        add(128, 640, "none", tr, ramp="rise", bwd=False)
        add(128, 640, "none", tr, ramp="fall", bwd=False)
        for mk in ("none", "keypad"):
            add(33, 70, mk, tr, kvr=96)               # fwd: attn_fwd_kernel on a K/V cache of 96 rows per sample
        for Nq, Nk in ((520, 40), (40, 530)):
            for mk in KINDS4:
                add(Nq, Nk, mk, tr)                   # bwd: attn_bwd_kernel<tr,.,true,false> (chunks of 256 rows re-staged)
        for mk in ("dec", "keypad", "causal"):
            add(544, 544, mk, tr)                     # bwd: attn_bwd_kernel<tr,.,true,false>, both sides chunked
        add(130, 65, "none", tr, o_layout=1)          # fwd: attn_fwd_kernel, wide_o = 0
        add(130, 65, "keypad", tr, g_layout=1)        # bwd: attn_bwd_kernel<tr,KEYPAD,false,false>, wide_q / wide_k / wide_v = 0
    return out


CASES = build_cases()


class Fixture:
    """Inputs and mask of one (shape, mask, ramp), built once on the CPU and shared by the cases that use them."""

    def __init__(self, c: Case):
        self.mask = make_mask(c.mask, B, c.Nq, c.Nk, seed=c.seed + 7)
        self.scale = HD ** -0.5
        self.q, self.k, self.v, self.do = make_inputs(B, H, c.Nq, c.Nk, c.seed, c.ramp, self.mask.kpad)


_FIX = {}


def fixture(c: Case) -> Fixture:
    key = (c.Nq, c.Nk, c.mask, c.ramp)
    if key not in _FIX:
        _FIX[key] = Fixture(c)
    return _FIX[key]
