"""fm_attn_decode (csrc/attn_decode.hip) on a real MI355X, element by element against a float64 restatement on the same inputs.

The operands live where the decoder keeps them: a (B, kv_batch_rows, q | k | v) cache with a padded row stride, the query being the q
block of row Nk - 1 of every sample.  Rows >= Nk, the trailing rows and the pad columns hold NaN, o sits in a sentinel-filled buffer.

Bounds (u = 2^-24, the fp32 unit roundoff; everything first order, with a factor 1 + 2^-10 on the total for the products of two of
these terms, each of which is below 2^-10):
  written key   the kernel evaluates the LayerNorm in double and rounds once: it must be within ONE unit in the last place (of the
                storage type, in the binade of the reference) of the float64 LayerNorm rounded to the storage type.
  q             with the norm: the double result rounded to fp32, dq = u |qn| + 2^-46 (max |xhat w| + max |b|) (64 double operations
                on terms of that size); without: exact.
  score s_j     64 fused multiply-adds and the scale: E_s = scale (66 u sum_d |qn_d k_jd| + sum_d dq_d |k_jd|); a blocked score is the
                exact constant.
  e_j           exp(s_j - m) with m the maximum of the kernel's own scores (softmax does not depend on the shift): the subtraction
                rounds once and expf is good to 2 ulp = 4 u, so e_j carries the relative error rho_j = expm1(E_s) + u (|s_j - m| +
                2 max E_s) + 4 u; rho_j = 0 where the score is blocked (e_j is exactly 0, or exactly 1 in a fully blocked row).
  sum           positive terms: ceil(Nk / 256) additions in a thread, 6 shuffle levels, 2 additions over the waves and 1 for softmax1's
                zero logit (itself an expf: 4 u more): relative error sum_j p_j rho_j + (ceil(Nk / 256) + 9 [+ 4]) u = eps_sum.
  o_d           numerator: n_v = ceil(Nk / (4 KPW)) fused multiply-adds in a thread (KPW = 8 value rows per wave in bf16, 4 in fp32),
                log2(KPW) shuffle levels, 2 additions over the waves, then the division:
                E = sum_j p_j |v_jd| (rho_j + (n_v + log2 KPW + 3) u) + |o_d| eps_sum
                    + Nk 2^-126 max |v|   (an e_j below the normal range may be flushed),
                plus half a bf16 ulp of (|o_d| + E) for a bf16 store.
The reference uses the key as STORED after the call (the kernel must use the rounded value it wrote)."""
import ctypes as C
import itertools
import math

import pytest
import torch

from tests.test_divae_kernels_gpu import ETA, U, bf16_rne, check, hulp

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")
SENT = 7.0
BF, F32 = torch.bfloat16, torch.float32
EPS = 1e-6
NEG = {BF: -3.3895313892515355e38, F32: -3.4028234663852886e38}
NKS = (1, 2, 63, 64, 65, 129, 300)


def _ops():
    from fourm.hip import _lib, ops
    return ops, _lib


def gen(seed):
    g = torch.Generator(device="cpu")
    g.manual_seed(seed)
    return g


def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF else torch.int32).clone()


def ulp(ref, dtype):
    """Spacing of ``dtype`` in the binade of ``ref`` (float64): 2^(e - 7) for bf16, 2^(e - 23) for fp32, 2^e <= |ref| < 2^(e + 1)."""
    e = torch.frexp(ref.abs())[1].double() - 1
    return torch.where(ref != 0, torch.exp2(e - (7 if dtype == BF else 23)), torch.zeros_like(ref))


def layer_norm64(x, w, b):
    """(..., 64) float64 LayerNorm with the eps the kernel receives (a float); -> (y, max |xhat w| + max |b| per vector)."""
    eps = float(torch.tensor(EPS, dtype=F32))
    mu = x.mean(-1, keepdim=True)
    xh = (x - mu) / torch.sqrt(((x - mu) ** 2).mean(-1, keepdim=True) + eps)
    y = xh * w.double()
    mag = y.abs().amax(-1, keepdim=True)
    if b is not None:
        y = y + b.double()
        mag = mag + b.double().abs().max()
    return y, mag


def decode_case(Nk, B, H, extra, dtype, norm, knew, zero_attn, kpad_mode, seed):
    """One launch against float64.  norm: "off" | "bias" | "nobias"; knew: -1 | 0 | "last"; kpad_mode: None | "few" | "all" (the last
    sample fully blocked, the others a few keys).  -> worst err / bound of o."""
    ops, _ = _ops()
    D, kvr = 64 * H, Nk + extra
    ld = 3 * D + 8
    knew = Nk - 1 if knew == "last" else knew
    scale = 64 ** -0.5
    buf = torch.full((B * kvr + 2, ld), NAN, dtype=dtype, device=DEV)
    for b in range(B):
        buf[b * kvr:b * kvr + Nk, :3 * D] = (torch.randn(Nk, 3 * D, generator=gen(seed + b)) * 1.5 + 0.25).to(DEV).to(dtype)
    q = buf[Nk - 1:Nk + (B - 1) * kvr:kvr, :D]
    k, v = buf[:, D:2 * D], buf[:, 2 * D:3 * D]
    assert q.shape == (B, D)
    o_buf = torch.full((B + 1, D + 8), SENT, dtype=dtype, device=DEV)
    qn = kn = None
    if norm != "off":
        mk = lambda s, bias: ((1.0 + 0.2 * torch.randn(64, generator=gen(s))).to(DEV),
                              (0.1 * torch.randn(64, generator=gen(s + 1))).to(DEV) if bias else None)
        qn, kn = mk(seed + 50, norm == "bias"), mk(seed + 60, norm == "bias")
    kpad = None
    if kpad_mode is not None:
        kpad = torch.rand(B, Nk, generator=gen(seed + 70)) < 0.3
        kpad[:, Nk // 2] = False                                         # "a few": never the whole row
        if kpad_mode == "all":
            kpad[B - 1] = True
        kpad = kpad.to(DEV)
    before = bits(buf)
    ops.attn_decode(q, k, v, o_buf[:, :D], B, H, Nk, scale, kv_batch_rows=kvr, k_new_row=knew, q_norm=qn, k_norm=kn, eps=EPS, kpad=kpad,
                    zero_attn=zero_attn)
    torch.cuda.synchronize()
    name = f"Nk={Nk} B={B} H={H} kvr={kvr} {dtype} norm={norm} knew={knew} zero={zero_attn} kpad={kpad_mode}"
    # ---- memory discipline ----
    after = bits(buf)
    changed = torch.zeros_like(after, dtype=torch.bool)
    rows = torch.arange(B, device=DEV) * kvr
    writes_key = norm != "off" and knew >= 0
    if writes_key:
        changed[rows + knew, D:2 * D] = True
    assert torch.equal(after[~changed], before[~changed]), f"{name}: q / k / v written outside the new key row"
    assert bool((o_buf[B] == SENT).all()) and bool((o_buf[:, D:] == SENT).all()), f"{name}: o written outside (B, 64 H)"
    o = o_buf[:B, :D]
    assert bool(torch.isfinite(o.float()).all()), f"{name}: o is not finite"
    # ---- float64 reference ----
    sample = lambda t: torch.stack([t[b * kvr:b * kvr + Nk] for b in range(B)]).double().reshape(B, Nk, H, 64)      # (B, Nk, H, 64)
    q64 = q.double().reshape(B, H, 64)
    dq = torch.zeros_like(q64)
    if norm != "off":
        q64, mag = layer_norm64(q64, *qn)
        dq = U * q64.abs() + 2.0 ** -46 * mag
    if writes_key:
        pre = torch.stack([before.view(buf.dtype)[b * kvr + knew, D:2 * D] for b in range(B)]).double().reshape(B, H, 64)
        want_k, _ = layer_norm64(pre, *kn)
        want_k = bf16_rne(want_k) if dtype == BF else want_k.float().double()
        got_k = torch.stack([k[b * kvr + knew] for b in range(B)]).double().reshape(B, H, 64)
        check(f"stored key {name}", got_k, want_k, ulp(want_k, dtype))
        assert not torch.equal(got_k, pre), f"{name}: the key was not normalised"
    k64, v64 = sample(k), sample(v)                                       # (the stored key)
    s = scale * torch.einsum("bhd,bjhd->bhj", q64, k64)
    E_s = scale * (66 * U * torch.einsum("bhd,bjhd->bhj", q64.abs(), k64.abs()) + torch.einsum("bhd,bjhd->bhj", dq, k64.abs()))
    blocked = torch.zeros(B, 1, Nk, dtype=torch.bool, device=DEV) if kpad is None else kpad[:, None, :]
    blocked = blocked.expand(B, H, Nk)
    s = torch.where(blocked, torch.full_like(s, NEG[dtype]), s)
    m = s.amax(-1, keepdim=True)
    if zero_attn:
        m = m.clamp(min=0.0)
    e = torch.exp(s - m)
    den = e.sum(-1, keepdim=True) + (torch.exp(-m) if zero_attn else 0.0)
    p = e / den
    rho = torch.expm1(E_s) + U * ((s - m).abs() + 2 * E_s.amax(-1, keepdim=True)) + 4 * U
    rho = torch.where(blocked, torch.zeros_like(rho), rho)
    want = torch.einsum("bhj,bjhd->bhd", p, v64)
    kpw = 8 if dtype == BF else 4
    n_t, n_v = math.ceil(Nk / 256), math.ceil(Nk / (4 * kpw))
    pr = (p * rho).sum(-1, keepdim=True)
    E = (torch.einsum("bhj,bjhd->bhd", p * (rho + (n_v + math.log2(kpw) + 3) * U), v64.abs()) + want.abs() * (pr + (n_t + 9 + (4 if zero_attn else 0)) * U)
         + Nk * ETA * v64.abs().max())
    E = E * (1 + 2.0 ** -10)
    if dtype == BF:
        E = E + hulp(want.abs() + E)
    if kpad_mode == "all" and not zero_attn:                             # a fully blocked sample attends uniformly
        uni = v64[B - 1].mean(0)
        assert float((want[B - 1] - uni).abs().max()) <= 1e-12 * float(uni.abs().max())
    return check(f"o {name}", o.reshape(B, H, 64), want, E)


@pytest.mark.parametrize("norm", ["off", "bias", "nobias"])
@pytest.mark.parametrize("dt", ["bf16", "fp32"])
def test_attn_decode_against_float64(dt, norm):
    """Nk in {1, 2, 63, 64, 65, 129, 300} (one key, one short of / exactly / one past a wave, two PV sweeps of every wave, a second
    score sweep of the 256 threads), B in {1, 3}, H in {1, 6}, kv_batch_rows in {Nk, Nk + 5}, k_new_row in {-1, 0, Nk - 1},
    softmax and softmax1, no mask / a few blocked keys / one fully blocked sample."""
    dtype = BF if dt == "bf16" else F32
    worst = 0.0
    for n, (Nk, B, H, extra) in enumerate(itertools.product(NKS, (1, 3), (1, 6), (0, 5))):
        for i, (knew, zero_attn, kpad_mode) in enumerate(itertools.product((-1, 0, "last"), (False, True), (None, "few", "all"))):
            worst = max(worst, decode_case(Nk, B, H, extra, dtype, norm, knew, zero_attn, kpad_mode, seed=1000 * n + 17 * i))
    print(f"attn_decode {dt} norm={norm}: worst err / bound {worst:.3g}")


def test_attn_decode_eager_reread_sees_the_stored_key():
    """A later token reads the normalised key as it is: decoding row p with k_new_row = p, then the same query with k_new_row = -1 over
    the now normalised cache, gives the same output bit for bit (the first call used the rounded value it stored)."""
    ops, _ = _ops()
    B, H, Nk, kvr = 3, 6, 65, 70
    D = 64 * H
    for dtype in (BF, F32):
        buf = (torch.randn(B * kvr, 3 * D, generator=gen(5)) * 1.5).to(DEV).to(dtype)
        q, k, v = buf[Nk - 1::kvr, :D], buf[:, D:2 * D], buf[:, 2 * D:]
        w = (1.0 + 0.2 * torch.randn(64, generator=gen(6))).to(DEV)
        o1, o2 = torch.zeros(B, D, dtype=dtype, device=DEV), torch.zeros(B, D, dtype=dtype, device=DEV)
        ops.attn_decode(q, k, v, o1, B, H, Nk, 0.125, kv_batch_rows=kvr, k_new_row=Nk - 1, q_norm=(w, None), k_norm=(w, None), eps=EPS)
        ops.attn_decode(q, k, v, o2, B, H, Nk, 0.125, kv_batch_rows=kvr, k_new_row=-1, q_norm=(w, None), eps=EPS)
        assert torch.equal(bits(o1), bits(o2)), dtype


REFUSALS = [
    ("null q", dict(q=None), "null pointer"),
    ("null k", dict(k=None), "null pointer"),
    ("null v", dict(v=None), "null pointer"),
    ("null o", dict(o=None), "null pointer"),
    ("Nk < 1", dict(Nk=0, k_new_row=-1), "Nk=0"),
    ("Nk too large", dict(Nk=8193, kv_batch_rows=8193), "Nk=8193"),
    ("kv_batch_rows < Nk", dict(kv_batch_rows=9), "kv_batch_rows=9 < Nk=10"),
    ("k_new_row >= Nk", dict(k_new_row=10), "k_new_row=10"),
    ("norm on the new key without k_w", dict(k_w=None), "needs k_w"),
    ("ldq < 64 H", dict(ldq=120), "row stride"),
    ("ldk < 64 H", dict(ldk=120), "row stride"),
    ("ldv < 64 H", dict(ldv=120), "row stride"),
    ("ldo < 64 H", dict(ldo=120), "row stride"),
    ("k not 16-byte aligned", dict(k_offset=2), "misaligned k / v"),
    ("v not 16-byte aligned", dict(v_offset=8), "misaligned k / v"),
    ("ldk not a multiple of 16 bytes", dict(ldk=396), "misaligned k / v"),
    ("q not aligned to its element", dict(q_offset=1), "misaligned q / o"),
]


@pytest.mark.parametrize("what,change,text", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_attn_decode_refusals(what, change, text):
    """Every argument check returns -1 with its reason in fm_last_error() and launches nothing (o keeps its bits)."""
    _, L = _ops()
    change = dict(change)
    B, H, Nk = 2, 2, 10
    D = 64 * H
    buf = torch.zeros(B * Nk, 3 * D, dtype=BF, device=DEV)
    o = torch.full((B, D), SENT, dtype=BF, device=DEV)
    w = torch.ones(64, device=DEV)
    a = L.AttnDecodeArgs()
    ptr = dict(q=buf.data_ptr(), k=buf.data_ptr() + 2 * D, v=buf.data_ptr() + 4 * D, o=o.data_ptr(), q_w=w.data_ptr(), k_w=w.data_ptr())
    for f in ("q", "k", "v"):
        ptr[f] += change.pop(f + "_offset", 0)
    a.ldq, a.ldk, a.ldv, a.ldo = Nk * 3 * D, 3 * D, 3 * D, D
    a.B, a.H, a.Nk, a.kv_batch_rows, a.k_new_row, a.is_f32, a.zero_attn, a.scale, a.eps = B, H, Nk, Nk, Nk - 1, 0, 0, 0.125, EPS
    for f, val in {**ptr, **change}.items():
        setattr(a, f, val)
    rc = L.attn_decode(C.byref(a), None)
    torch.cuda.synchronize()
    assert rc == -1, (what, rc)
    assert text in L.lib.fm_last_error().decode(), (what, L.lib.fm_last_error().decode())
    assert bool((o == SENT).all())
