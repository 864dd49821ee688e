"""Dispatch restatement, case tables, float64 reference, per-element bounds and a CPU emulation of the dense bf16 GEMMs
(``fm_gemm_nt`` / ``fm_gemm_tn``: csrc/gemm.hip, gemm_nt3.hip, gemm_nt4.hip, gemm_nt_flat.hip, gemm_skinny.hip).
Importable without a GPU; every function runs on the device of its inputs.

Routes.  ``nt_route`` / ``tn_route`` restate the host-side dispatch (fm_gemm_nt with launch_nt, fm_launch_nt_skinny, fm_launch_nt4,
fm_launch_nt3, fm_launch_nt_flat; fm_gemm_tn) for a given number of compute units.  Reading that dispatch for the table below showed one
rule the shapes have to be read against: the SMALL-GRID policy (fm_lab_set 9, on by default) sits IN FRONT of gemm_nt4 / gemm_nt3 / the
flat kernel and takes every plain bf16 launch (no bias-less condition: any FM_EPI_BF16 launch without out2 / res and N % 4 == 0) whose
256 x 256 tiling covers at most half of the CUs: ceil(M / 256) * ceil(N / 256) <= 128.  A (2050, 256, 128) bf16 launch therefore runs on
the 128 x 128 tiles, not on gemm_nt3, and (2048, 384, 192) never reaches gemm_nt4.  The rows that are meant for nt3 / nt4 / flat at such
small shapes carry ``(9, 0)`` in their lab state (policy off for the launch, restored afterwards): the smallest shape that passes the policy
by itself is 129 row tiles (M > 32768 at N <= 256), which the rows "nt3 more tiles than CUs" and "nt4 default mode" use.

Reference.  Everything is float64 from the bf16-rounded operands.  Where a kernel output feeds a later stage of the same epilogue the
reference of the later stage is a function of the kernel's OWN earlier output (GELU: out = gelu(out2); SwiGLU: act = silu(g) u from the
saved g | u); without that copy the bound of the earlier stage is carried through the activation's Lipschitz constant.

Bounds (per element; U = 2^-24, gamma(n) = n U / (1 - n U); v = float64 result, S = the same sum over absolute values):
  accumulation   t_acc = gamma(K + 4) S          any summation order of K products + bias + the split-K partial sums (IEEE adds)
  bf16 output    hu(|v| + t_acc) + t_acc         one round-to-nearest of the accumulated value; hu(x) = 2^(floor(log2 x) - 8) is HALF AN
                                                 ULP of bf16 at x (8 significant bits), i.e. between 2^-9 x and 2^-8 x.  A relative constant
                                                 of 2^-9 is NOT a bound of round-to-nearest (0.5608 rounds to 0.5625: 2^-8.3 relative - the
                                                 faithful restatement fails it at once), 2^-8 is one but lets a truncation pass at large
                                                 mantissas; half an ulp is exactly what a correct conversion guarantees, and a truncating
                                                 or off-by-one-ulp conversion exceeds it
  fp32 output    t_acc                           (+ U (|res| + |v|) for the fp32 residual addition)
  activations    E_act = FN (|f(p)| + |p|), FN = 2^-20: erf_fast (Abramowitz-Stegun 7.1.26, 1.5e-7 absolute), __expf and rcpf
Two numbers are not derivable from the code: the matrix cores' internal accumulate rounding (t_acc assumes IEEE round-to-nearest adds) and
the error of erf_fast / __expf / rcpf.  Measured on an MI355X (parity log, gemm.kernels): the fp32 outputs use 0.015 and the TN
accumulations 0.04 of t_acc, and no activation output exceeds its bound - neither allowance was widened.

The emulation (``emu_nt`` / ``emu_tn``) restates the rounding points in torch fp32 on the CPU with blocked K accumulation; it validates
the bounds (tests/test_gemm_ref_cpu.py) and is NOT the reference.
"""
import math
from dataclasses import dataclass
from typing import Optional, Tuple

import torch

U = 2.0 ** -24                       # fp32 unit roundoff


def half_ulp(x):
    """Half an ulp of bf16 (8 significant bits) at magnitude x >= 0: 2^(floor(log2 x) - 8); 0 at 0."""
    return torch.where(x > 0, torch.exp2(torch.floor(torch.log2(x.clamp_min(1e-300))) - 8.0), torch.zeros_like(x))

FN = 2.0 ** -20                      # activation term (tests/test_fp32_kernels_gpu.py uses the same constant)
LIP = dict(gelu=1.13, tanh=1.0, silu=1.10)      # Lipschitz constants: max |gelu'| = 1.1290, |tanh'| = 1, max |silu'| = 1.0998

NT_DEFAULT = 9 + 256                 # fm_set_gemm_nt_config: automatic, raised priority
NT_FLAT = NT_DEFAULT + (1 << 29)     # + the flattened persistent kernel where it applies
LAB_DEFAULT = {2: 3, 3: 0, 4: 1, 9: 1}
TN_DEFAULT = 1
SPLITK_MAX_OUT = 128 * 128 * 128     # ops.SPLITK_MAX_OUT
SPLITK_WS_BYTES = 16 * SPLITK_MAX_OUT * 4


def gamma(n):
    return n * U / (1.0 - n * U)


def ru(x, m):
    return (x + m - 1) // m * m


def cdiv(a, b):
    return (a + b - 1) // b


# ------------------------------------------------------------------------------------------------
# dispatch restatement
# ------------------------------------------------------------------------------------------------
def lends_splitk(M, N, K, epi, fixed=False):
    """ops.gemm_nt lends its split-K scratch for FM_EPI_BF16 launches with M N <= SPLITK_MAX_OUT and K >= 512 (never under fixed_tiling)."""
    return SPLITK_WS_BYTES if (not fixed and epi == "bf16" and M * N <= SPLITK_MAX_OUT and K >= 512) else 0


def nt4_takes(M, N, K, mode, *, cus=256, bias=False, epi="bf16", ldo=None, aligned128=True):
    """fm_launch_nt4's own answer (gemm_nt4.hip:311-329): None when it declines, else the variant it launches."""
    ldo = N if ldo is None else ldo
    if not mode or bias or epi != "bf16":
        return None
    if M % 256 != 0 or M < 2048 or K % 64 != 0 or K < 192 or ldo % 64 != 0 or not aligned128:
        return None
    stg = "staged" if not (mode & 4) else "unstaged"
    xt = M // 256
    if (mode & 1) and N % 384 == 0:
        c4 = cdiv((N // 384) * xt, cus) * 384
        c256 = cdiv(cdiv(N, 256) * xt, cus) * 256
        c192 = cdiv((N // 192) * xt, cus) * 192 if N % 192 == 0 else c256
        forced = c4 > min(c256, c192)
        if forced and not (mode & 8):
            return None
        tiles = (N // 384) * xt
        return f"nt4.384.{stg}" + (".forced" if forced else "") + (".wrap" if tiles > cus else "")
    if (mode & 2) and N % 256 == 0:
        return f"nt4.256.{stg}" + (".wrap" if (N // 256) * xt > cus else "")
    return None


def _nt3(M, N, K, epi, mode, *, bias, out2, res, ldo, ldo2, ldr, Hp, aligned128, aligned16, lab3, cus, m_dev=False):
    if not mode:
        return None
    if m_dev:
        if epi != "bf16" or bias or K % 64 or K < 128 or N % 8 or ldo % 64 or not aligned128 or (lab3 & (16 | 1024)):
            return None
        return "nt3.devm.192" if (N % 192 == 0 and N % 256 != 0) else "nt3.devm.256"
    if bias and epi not in ("bf16", "gelu", "quick_gelu"):
        return None
    if bias and (lab3 & (16 | 1024)):
        return None
    if M < 2048 or K % 64 or K < 128 or N % 8:
        return None
    if not aligned16:
        return None
    xt = cdiv(M, 256)
    t256, t192 = cdiv(N, 256) * xt, cdiv(N, 192) * xt
    fits192 = N % 192 == 0
    c256, c192 = cdiv(t256, cus) * 256, cdiv(t192, cus) * 192
    use192 = fits192 if mode == 2 else (fits192 and c192 < c256) if mode == 3 else False
    tw = 192 if use192 else 256
    wrap = ".wrap" if (t192 if use192 else t256) > cus else ""
    if epi in ("gelu", "quick_gelu"):
        return None if not (lab3 & 131072) else f"nt3.{tw}.{epi}.lab"
    if epi == "bf16":
        if ldo % 8:
            return None
        if bias:
            if ldo % 64 or not aligned128:
                return None
            return f"nt3.{tw}.staged.bias{wrap}"
        if not (lab3 & 1024) and not (lab3 & 16) and ldo % 64 == 0 and aligned128:
            return f"nt3.{tw}.staged{wrap}"
        return f"nt3.{tw}.unstaged{wrap}" if not (lab3 & 16) else f"nt3.{tw}.nosplit.lab"
    if epi == "res":
        return None if not (lab3 & 256) else f"nt3.{tw}.res.lab"
    if epi == "swiglu_bwd":
        if N % 16 or Hp % 8 or ldo % 8 or ldr % 8 or not res or Hp < N:
            return None
        return "nt3.swiglu_bwd" + (".wrap" if t256 > cus else "")
    if epi == "swiglu":
        if N % 64 or Hp % 8 or ldo % 8 or (out2 and ldo2 % 8):
            return None
        if not (lab3 & 1024) and not (lab3 & 16) and ldo % 64 == 0 and (not out2 or ldo2 % 64 == 0) and Hp % 64 == 0:
            return "nt3.swiglu.staged"
        return "nt3.swiglu.unstaged"
    return None


def _flat(M, N, K, epi, flat_on, *, bias, out2, ldo, ldo2, Hp, aligned16):
    if not flat_on or bias:
        return None
    if M < 2048 or K % 64:
        return None
    if epi == "bf16":
        return None if (N % 128 or ldo % 8 or not aligned16 or K // 64 < 8) else "flat.bf16"
    if epi == "swiglu":
        return None if (N % 64 or Hp % 8 or ldo % 8 or (out2 and ldo2 % 8) or not aligned16 or K // 64 < 12) else "flat.swiglu"
    return None


def _tiled(M, N, K, epi, cfg_full, fixed, cus):
    if fixed:
        return "tiled.fixed"
    if M <= 128:
        return "tiled.m128"
    cfg = cfg_full & 0xff
    auto = [11, 10]
    swiglu = 12
    if (cfg_full >> 16) & 0xff:
        auto = [(cfg_full >> 16) & 0xf, (cfg_full >> 20) & 0xf]
    if (cfg_full >> 24) & 0xf:
        swiglu = (cfg_full >> 24) & 0xf
    name = "tiled"
    if cfg == 9:
        if epi == "swiglu":
            cfg, name = swiglu, "tiled.swiglu"
        else:
            cfg = auto[1 if (K >= 1536 or epi in ("res", "swiglu_bwd", "gelu_bwd")) else 0]
        t256 = cdiv(N, 256) * cdiv(M, 256)
        if cfg == auto[0] and auto[0] == 11 and N % 256 == 0 and t256 % cus == 0:
            cfg = 12
    suffix = ""
    geo = {10: (128, 256, 64), 11: (128, 256, 32), 12: (256, 256, 32)}
    if cfg in geo:                                        # persistent: one resident workgroup per LDS slot
        tw, tx, kb = geo[cfg]
        npt = tw // 2 if epi == "swiglu" else tw
        tiles = cdiv(N, npt) * cdiv(M, tx)
        slots = cus * (160 * 1024 // (3 * (tw + tx) * kb * 2)) // 8 * 8
        suffix = ".wrap" if tiles > slots else ".gtcus" if tiles > cus else ""
    return f"{name}.cfg{cfg}{suffix}"


def nt_route(M, N, K, epi, *, bias=False, out2=False, res=False, ldo=None, ldo2=0, ldr=0, Hp=0, aligned128=True, aligned16=True,
             splitk_ws_bytes=0, fixed=False, lab=None, nt_config=NT_DEFAULT, cus=256, m_dev=False, grouped=False):
    """The kernel and variant fm_gemm_nt selects (gemm.hip: fm_gemm_nt).  epi: bf16 | gelu | quick_gelu | res | swiglu | f32 | tanh |
    swiglu_bwd | gelu_bwd.  lab: {key: value} overrides of fm_lab_set (defaults LAB_DEFAULT); nt_config: the fm_set_gemm_nt_config word."""
    lb = dict(LAB_DEFAULT)
    lb.update(lab or {})
    ldo = ru(N, 4) if ldo is None else ldo
    kw3 = dict(bias=bias, out2=out2, res=res, ldo=ldo, ldo2=ldo2, ldr=ldr, Hp=Hp, aligned128=aligned128, aligned16=aligned16, lab3=lb[3], cus=cus)
    if m_dev:
        r = _nt3(M, N, K, epi, lb[2] or 3, m_dev=True, **kw3)
        return r or "refused"
    if grouped:
        return "grouped.k64pp" if K >= 1536 else "grouped.k32"
    if M <= 32 and not fixed and K % 16 == 0 and K >= 64:
        if epi == "bf16" or (epi == "res" and res) or epi == "swiglu" or epi == "quick_gelu":
            return f"skinny.{epi}"
    if not fixed and lb[9] and epi == "bf16" and M > 32 and not out2 and not res and N % 4 == 0:
        t256 = cdiv(M, 256) * cdiv(N, 256)
        if t256 * 2 <= cus:
            t128 = cdiv(M, 128) * cdiv(N, 128)
            kt = K // 64
            S = 1
            ldp = ru(N, 4)
            if splitk_ws_bytes and t128 * 2 <= cus and kt >= 8 and K % 64 == 0:
                S = min(cus // t128, kt // 4, 16, splitk_ws_bytes // (M * ldp * 4))
            if S >= 2:
                ks = cdiv(kt, S) * 64
                S = cdiv(K, ks)
                return f"splitk.{S}" + (".short_last" if K % ks else "")
            return "small128.k64" if K >= 1536 else "small128.k32"
    if not fixed and lb[4]:
        r = nt4_takes(M, N, K, lb[4], cus=cus, bias=bias, epi=epi, ldo=ldo, aligned128=aligned128)
        if r:
            return r
    if not fixed and lb[2]:
        r = _nt3(M, N, K, epi, lb[2], **kw3)
        if r:
            return r
    if not fixed and (nt_config & 0xff) == 9:
        r = _flat(M, N, K, epi, (nt_config >> 29) & 1, bias=bias, out2=out2, ldo=ldo, ldo2=ldo2, Hp=Hp, aligned16=aligned16)
        if r:
            return r
    return _tiled(M, N, K, epi, nt_config, fixed, cus)


def tn_route(R, N, K, force_tr=-1, cfg=TN_DEFAULT, splits=0, cus=256):
    """fm_gemm_tn (dense): -> (ping-pong schedule?, K-step, rows masked?, splits)."""
    pp = cfg in (1, 3, 4) and force_tr != 0
    kb = 64 if pp else 32
    slots = (1 if pp else 2) * cus
    if splits <= 0:
        tiles = cdiv(N, 128) * cdiv(K, 256)
        nt = cdiv(R, kb)
        splits = 1 if tiles >= slots else slots // tiles
        while splits > 1 and nt // splits < 8:
            splits -= 1
        splits = min(splits, 64)
        if nt < 16:
            splits = 1
    return pp, kb, R % kb != 0, splits


# ------------------------------------------------------------------------------------------------
# case tables
# ------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class NTCase:
    M: int
    N: int
    K: int
    epi: str
    route: str                                    # the kernel / variant the row is meant to reach (nt_route's name)
    bias: bool = False
    out2: bool = False
    res: str = ""                                 # "" | "sep" | "inplace" (RES: fp32; F32: fp32, optional; *_bwd: the saved bf16 rows)
    Hp: int = 0
    ldo: int = 0                                  # 0: roundup64(roundup4(width) + 1): whole lines, at least one spare column
    col0: int = 0                                 # first column of the out view inside its buffer
    ldo2: int = 0
    ldx_pad: int = 8                              # NaN columns behind K in X / W
    ldw_pad: int = 8
    lab: Tuple[Tuple[int, int], ...] = ()         # fm_lab_set(key, value) for the launch (restored afterwards)
    cfg: int = NT_DEFAULT                         # fm_set_gemm_nt_config word
    fixed: bool = False                           # under ops.fixed_tiling()

    @property
    def width(self):                              # columns of the out view
        return 2 * self.Hp if self.epi == "swiglu_bwd" else ru(self.N, 4)

    @property
    def ld_out(self):
        return self.ldo or ru(self.width + 1, 64)

    @property
    def ld_out2(self):
        if not self.out2:
            return 0
        return self.ldo2 or (ru(2 * self.Hp + 1, 64) if self.epi == "swiglu" else ru(ru(self.N, 4) + 1, 64))

    @property
    def ld_res(self):
        if not self.res:
            return 0
        if self.res == "inplace":
            return self.ld_out
        return ru((2 * self.Hp if self.epi == "swiglu_bwd" else ru(self.N, 4)) + 1, 8)

    @property
    def out_f32(self):
        return self.epi in ("res", "f32")

    @property
    def id(self):
        s = f"{self.M}x{self.N}x{self.K}-{self.epi}"
        s += "-b" if self.bias else ""
        s += "-o2" if self.out2 else ""
        s += f"-{self.res}" if self.res else ""
        s += f"-ld{self.ldo}" if self.ldo else ""
        s += f"-c{self.col0}" if self.col0 else ""
        s += "".join(f"-lab{k}={v}" for k, v in self.lab)
        s += "-flat" if self.cfg != NT_DEFAULT else ""
        s += "-fixed" if self.fixed else ""
        return s

    @property
    def math_key(self):                           # cases with the same key share inputs
        return (self.M, self.N, self.K, self.epi in ("swiglu_bwd", "gelu_bwd"), self.Hp if self.epi == "swiglu_bwd" else 0)


def case_route(c: NTCase, cus=256):
    """nt_route at the row's shape, layout and settings (what ops.gemm_nt passes for the buffers of tests/test_gemm_kernels_gpu.py)."""
    esz = 4 if c.out_f32 else 2
    a128 = (c.col0 * esz) % 128 == 0
    return nt_route(c.M, c.N, c.K, c.epi, bias=c.bias, out2=c.out2, res=bool(c.res), ldo=c.ld_out, ldo2=c.ld_out2, ldr=c.ld_res, Hp=c.Hp,
                    aligned128=a128, aligned16=(c.col0 * esz) % 16 == 0, splitk_ws_bytes=lends_splitk(c.M, c.N, c.K, c.epi, c.fixed),
                    fixed=c.fixed, lab=dict(c.lab), nt_config=c.cfg, cus=cus)


S0 = ((9, 0),)                                    # small-grid policy off for the launch (see the module docstring)


def build_nt_cases():
    C = NTCase
    out = []
    # ---- gemm_skinny.hip: M <= 32 ------------------------------------------------------------------------------------------------
    for M, N, K in ((7, 44, 64), (32, 42, 128)):
        for b in (False, True):
            out.append(C(M, N, K, "bf16", "skinny.bf16", bias=b))                       # gemm_skinny_kernel<EPI_BF16>
            out.append(C(M, N, K, "res", "skinny.res", bias=b, res="sep"))              # gemm_skinny_kernel<EPI_RES>
            out.append(C(M, N, K, "swiglu", "skinny.swiglu", bias=b, out2=True, Hp=64))  # gemm_skinny_kernel<EPI_SWIGLU> (bias and bias2)
    out.append(C(7, 44, 64, "swiglu", "skinny.swiglu", Hp=64))                          # ... inference: no (g | u) copy
    # ---- small-grid policy: gemm_nt_kernel<128,128,2,2,KB,3,EPI_BF16> / split-K -------------------------------------------------------
    out.append(C(200, 132, 128, "bf16", "small128.k32"))                                # K-step 32
    out.append(C(200, 132, 1536, "bf16", "splitk.6"))                                   # ops.gemm_nt lends its scratch at this shape: 6 slices of 4 K-tiles, NOT the K-step 64 form
    out.append(C(2050, 1024, 1536, "bf16", "small128.k64"))                             # K-step 64 needs a launch the lending rule refuses: M N > SPLITK_MAX_OUT, 36 tiles of 256 x 256
    for b in (False, True):
        out.append(C(200, 132, 576, "bf16", "splitk.2.short_last", bias=b))             # 9 K-tiles: slices of 5 and 4; splitk_reduce_kernel adds the bias
    out.append(C(200, 132, 4096, "bf16", "splitk.16"))                                  # 16 slices of 4 K-tiles
    # ---- gemm_nt_kernel, tile at a time ----------------------------------------------------------------------------------------------
    out.append(C(100, 75, 64, "bf16", "tiled.m128"))                                    # <128,128,2,2,32,3>: N % 4 != 0 skips the small-grid rule
    out.append(C(200, 130, 128, "bf16", "tiled.cfg11"))                                 # <128,256,2,4,32,3,.,PP,PERSIST>, N % 4 != 0
    out.append(C(200, 320, 128, "gelu", "tiled.cfg11", bias=True, out2=True))
    out.append(C(200, 320, 128, "tanh", "tiled.cfg11", bias=True))
    out.append(C(200, 320, 128, "f32", "tiled.cfg11", bias=True))
    out.append(C(200, 320, 128, "f32", "tiled.cfg11", bias=True, res="sep"))
    out.append(C(200, 136, 1536, "gelu", "tiled.cfg10", bias=True))                     # <128,256,2,4,64,3,.,PP,PERSIST>: long K
    out.append(C(200, 320, 128, "res", "tiled.cfg10", bias=True, res="inplace"))        # reading epilogue
    out.append(C(300, 176, 128, "swiglu_bwd", "tiled.cfg10", res="sep", Hp=192))
    out.append(C(300, 200, 128, "gelu_bwd", "tiled.cfg10", res="sep"))
    out.append(C(192, 170, 128, "swiglu", "tiled.swiglu.cfg12", out2=True, Hp=192))     # <256,256,2,4,32,3,EPI_SWIGLU,.,PP,PERSIST>, H % 4 != 0
    out.append(C(192, 170, 128, "swiglu", "tiled.swiglu.cfg12", Hp=192))
    out.append(C(255 * 256 + 20, 256, 64, "bf16", "tiled.cfg12"))                       # 256 tiles of 256 x 256 = one whole round (nt3 declines K < 128)
    out.append(C(33100, 260, 64, "gelu", "tiled.cfg11.gtcus", bias=True, out2=True))    # 390 tiles on 512 slots: two workgroups per CU
    out.append(C(22100, 260, 64, "res", "tiled.cfg10.wrap", res="sep"))                 # 261 tiles on 256 slots: a workgroup's SECOND tile (added: the row above never wraps)
    out.append(C(300, 260, 192, "bf16", "tiled.fixed", fixed=True))                     # <128,128,2,2,32,3> whatever the shape
    out.append(C(2100, 256, 128, "bf16", "tiled.fixed", fixed=True))
    # ---- gemm_nt3.hip ---------------------------------------------------------------------------------------------------------------
    out.append(C(2050, 256, 128, "bf16", "nt3.256.staged", lab=S0))                     # gemm_nt3_kernel<256,EPI_BF16,SPLIT,STG>
    out.append(C(2050, 192, 128, "bf16", "nt3.192.staged", lab=S0))                     # <192,...>
    out.append(C(2050, 200, 128, "bf16", "nt3.256.unstaged", ldo=200, lab=S0))          # ldo % 64 != 0: <256,EPI_BF16,SPLIT>
    out.append(C(2050, 256, 128, "bf16", "nt3.256.staged.bias", bias=True, lab=S0))     # <256,EPI_BF16,SPLIT,STG,BIAS>
    out.append(C(2050, 192, 128, "bf16", "nt3.192.staged.bias", bias=True, lab=S0))
    out.append(C(2050, 128, 128, "swiglu", "nt3.swiglu.staged", out2=True, Hp=128))     # <256,EPI_SWIGLU,SPLIT,STG>
    out.append(C(2050, 192, 128, "swiglu", "nt3.swiglu.unstaged", out2=True, Hp=192, ldo=200))      # act ld = 200: <256,EPI_SWIGLU,SPLIT>
    out.append(C(2050, 176, 128, "swiglu_bwd", "nt3.swiglu_bwd", res="sep", Hp=192))    # <256,EPI_SWIGLU_BWD,SPLIT>
    out.append(C(66000, 256, 128, "bf16", "nt3.256.staged.wrap"))                       # 258 tiles: the reverse walk reaches a second round
    # ---- gemm_nt4.hip ---------------------------------------------------------------------------------------------------------------
    out.append(C(33024, 384, 192, "bf16", "nt4.384.staged"))                            # default mode, 129 tiles: one round
    out.append(C(102400, 384, 192, "bf16", "nt4.384.staged.wrap"))                      # 400 tiles: a partial second round
    out.append(C(2048, 384, 192, "bf16", "nt4.384.staged.forced", lab=S0 + ((4, 9),)))  # mode 9: 8 tiles, 3 K-tiles (G = 3: the shortest stream)
    out.append(C(2304, 768, 256, "bf16", "nt4.384.staged.forced", lab=S0 + ((4, 9),)))  # 18 tiles, 4 K-tiles
    out.append(C(2048, 384, 192, "bf16", "nt4.384.unstaged.forced", lab=S0 + ((4, 13),)))
    out.append(C(2048, 256, 192, "bf16", "nt4.256.staged", lab=S0 + ((4, 2),)))         # gemm_nt4_kernel<256,256,2,2,STG>
    out.append(C(2048, 384, 192, "bf16", "nt4.384.staged.forced", lab=S0 + ((4, 9),), ldo=384 + 256, col0=128, ldx_pad=64, ldw_pad=128))
    # ---- gemm_nt_flat.hip (lab 2 = lab 4 = 0, config bit 29) --------------------------------------------------------------------------
    FL = S0 + ((2, 0), (4, 0))
    out.append(C(2050, 128, 512, "bf16", "flat.bf16", lab=FL, cfg=NT_FLAT))             # gemm_nt_flat_kernel<128,256,64,EPI_BF16>, 8 K-tiles = its 8 deferred stores
    out.append(C(2050, 128, 768, "swiglu", "flat.swiglu", out2=True, Hp=128, lab=FL, cfg=NT_FLAT))      # <..,EPI_SWIGLU>, 12 K-tiles = 12 stores
    out.append(C(2050, 128, 768, "swiglu", "flat.swiglu", Hp=128, lab=FL, cfg=NT_FLAT))  # inference: only the activation's 4 stores
    return out


NT_CASES = build_nt_cases()

# routes reached through their own entry points (tests/test_gemm_kernels_gpu.py: test_nt_heads_device_rows, test_nt_grouped)
HEADS_VOCABS, HEADS_COUNTS, HEADS_D = [512, 192, 1000, 64], [700, 0, 300, 5], 192
GROUP_NS, GROUP_KS = [40, 200, 520], [64, 1536]


@dataclass(frozen=True)
class TNCase:
    R: int
    N: int
    K: int
    cfg: int
    force_tr: int
    splits: int                                   # what the caller passes (0: automatic)
    route: tuple                                  # (ping-pong, K-step, masked, splits) of tn_route

    @property
    def id(self):
        return f"{self.R}x{self.N}x{self.K}-cfg{self.cfg}-tr{self.force_tr}-s{self.splits}"


def build_tn_cases():
    out = []
    for cfg, tr in ((1, 1), (1, 0), (0, 1)):      # gemm_tn_kernel<true,.,64,PP> / <false,.,32> / <true,.,32>
        for R, N, K, s in ((64, 128, 128, 0),                # one tile, unmasked for both K-steps
                           (37, 136, 264, 0),                # R < one K-step, N and K ragged
                           (1000, 200, 264, 0),              # masked last K-step
                           (1030, 136, 264, 0),              # automatic splits (2 on the ping-pong schedule)
                           (4100, 136, 520, 3)):             # 3 splits, 3 B tiles
            out.append(TNCase(R, N, K, cfg, tr, s, tn_route(R, N, K, tr, cfg, s)))
    return out


TN_CASES = build_tn_cases()
TN_MULTI_LISTS = {"one_small": [(64, 128, 128)], "ragged": [(1000, 200, 264), (37, 136, 520), (4100, 768, 136), (300, 64, 64)]}


# ------------------------------------------------------------------------------------------------
# inputs (CPU tensors; the GPU test moves them)
# ------------------------------------------------------------------------------------------------
def _gen(seed):
    return torch.Generator().manual_seed(seed)


@dataclass
class NTInputs:
    x: torch.Tensor                               # (M, K) bf16
    w: torch.Tensor                               # (N, K) bf16
    w2: torch.Tensor                              # (N, K) bf16 (SwiGLU)
    bias: torch.Tensor                            # (N,) fp32, NOT bf16-representable
    bias2: torch.Tensor
    res32: torch.Tensor                           # (M, N) fp32
    saved: Optional[torch.Tensor] = None          # swiglu_bwd: (M, 2 Hp) bf16 g | u; gelu_bwd: (M, N) bf16 pre-activation

    def to(self, dev):
        return NTInputs(*[None if t is None else t.to(dev) for t in (self.x, self.w, self.w2, self.bias, self.bias2, self.res32, self.saved)])


_NT_IN = {}


def nt_inputs(c: NTCase) -> NTInputs:
    """Seeded asymmetric operands: noise + ramps along K (x) and along N (w), so that transposed or shifted outputs fail."""
    if c.math_key in _NT_IN:
        return _NT_IN[c.math_key]
    M, N, K = c.M, c.N, c.K
    g = _gen(1000003 * (M % 9973) + 1009 * N + K)
    kr = (torch.arange(K) % 13).float() * 0.03 - 0.15
    nr = (torch.arange(N) % 11).float() * 0.01 - 0.04
    x = (torch.randn(M, K, generator=g) * 0.7 + kr[None]).bfloat16()
    w = (torch.randn(N, K, generator=g) * 0.1 + nr[:, None]).bfloat16()
    w2 = (torch.randn(N, K, generator=g) * 0.1 - nr[:, None]).bfloat16()
    bias = torch.randn(N, generator=g) * 2.0
    bias2 = torch.randn(N, generator=g) * 2.0
    res32 = torch.randn(M, N, generator=g) * 3.0 if M * N <= (1 << 23) else torch.zeros(1, 1)
    saved = None
    if c.epi == "swiglu_bwd":
        saved = torch.zeros(M, 2 * c.Hp)
        saved[:, :N] = torch.randn(M, N, generator=g) * 2.0
        saved[:, c.Hp:c.Hp + N] = torch.randn(M, N, generator=g) * 1.5
        saved = saved.bfloat16()
    elif c.epi == "gelu_bwd":
        saved = (torch.randn(M, N, generator=g) * 2.0).bfloat16()
    _NT_IN[c.math_key] = NTInputs(x, w, w2, bias, bias2, res32, saved)
    return _NT_IN[c.math_key]


def tn_inputs(R, N, K, seed=0):
    g = _gen(7919 * R + 31 * N + K + seed)
    a = (torch.randn(R, N, generator=g) + (torch.arange(N) % 17).float()[None] * 0.05).bfloat16()
    b = (torch.randn(R, K, generator=g) + (torch.arange(R) % 5).float()[:, None] * 0.1).bfloat16()
    out0 = torch.randn(N, K, generator=g) * 4.0
    return a, b, out0


# ------------------------------------------------------------------------------------------------
# float64 reference and bounds
# ------------------------------------------------------------------------------------------------
def bfr(t):
    """Round to bf16 and back (the dtype of ``t`` is kept)."""
    return t.bfloat16().to(t.dtype)


def _sig(x):
    return torch.sigmoid(x)


def f_gelu(x):
    return 0.5 * x * (1.0 + torch.erf(x * math.sqrt(0.5)))


def f_silu(x):
    return x * _sig(x)


def f_dsilu(x):                                   # d silu / dx = s (1 + x (1 - s))
    s = _sig(x)
    return s * (1.0 + x * (1.0 - s))


def f_dgelu(x):                                   # Phi(x) + x phi(x)
    return 0.5 * (1.0 + torch.erf(x * math.sqrt(0.5))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


def acc_ref(x, w, bias=None, bias_rounded=True):
    """-> v, S, t_acc (float64): v = x w^T (+ bias), S the same over absolute values.
    t_acc = gamma(K + 4) S: K products (exact: bf16 x bf16 fits fp32) summed in ANY order in fp32 - K - 1 additions, the bias, up to 16
    split-K partial sums ... each addition at most one rounding of a partial sum bounded by S; K + 4 covers a tree of any shape whose
    depth per term is at most K + 4 (sequential K-steps + 4 partial sums of the skinny kernel / log2(16) levels of split-K + the bias)."""
    K = x.shape[1]
    xd, wd = x.double(), w.double()
    v = xd @ wd.t()
    S = xd.abs() @ wd.abs().t()
    if bias is not None:
        b = (bfr(bias) if bias_rounded else bias).double()
        v = v + b[None]
        S = S + b.abs()[None]
    return v, S, gamma(K + 4) * S


def tol_bf16(v, t):
    """One round-to-nearest to bf16 of a value within t of v: half an ulp at |v| + t (the ulp grows with the magnitude), + t."""
    return half_ulp(v.abs() + t) + t


def e_act(fv, p):
    return FN * (fv.abs() + p.abs())


def prod_err(a, ea, b, eb):
    """|a' b' - a b| for |a' - a| <= ea, |b' - b| <= eb, plus the fp32 rounding of the product."""
    return a.abs() * eb + b.abs() * ea + ea * eb + U * (a.abs() + ea) * (b.abs() + eb)


def nt_reference(c: NTCase, inp: NTInputs, got=None):
    """-> {name: (ref, tol)} in float64 for every output of the row.  ``got``: the kernel's own outputs (dict name -> tensor), needed where a
    later stage is judged as a function of an earlier output (gelu with out2: "pre"; swiglu with out2: "g", "u")."""
    N = c.N
    epi = c.epi
    if epi == "swiglu":
        vg, Sg, tg = acc_ref(inp.x, inp.w, inp.bias if c.bias else None)
        vu, Su, tu = acc_ref(inp.x, inp.w2, inp.bias2 if c.bias else None)
        r = {}
        if c.out2:
            r["g"], r["u"] = (vg, tol_bf16(vg, tg)), (vu, tol_bf16(vu, tu))
            g, u = got["g"].double(), got["u"].double()              # act as a function of the saved g | u
            eg = eu = torch.zeros_like(vg)
        else:
            g, u, eg, eu = vg, vu, tol_bf16(vg, tg), tol_bf16(vu, tu)
        s = f_silu(g)
        es = tol_bf16(s, e_act(s, g) + (2.2 * FN + LIP["silu"]) * eg)      # bf16(silu_f(g')): activation error at g', slope, one rounding
        pe = prod_err(s, es, u, eu)
        r["act"] = (s * u, tol_bf16(s * u, pe))
        return r
    if epi in ("swiglu_bwd", "gelu_bwd"):
        v, S, t = acc_ref(inp.x, inp.w)
        ed = tol_bf16(v, t)                                           # d = bf16(acc)
        if epi == "gelu_bwd":
            xs = inp.saved.double()[:, :N]
            k = f_dgelu(xs)
            ek = e_act(k, xs)                                         # cdf (erf_fast) + x pdf (__expf), both within FN of (|k| + |x|)
            return {"out": (v * k, tol_bf16(v * k, prod_err(v, ed, k, ek)))}
        g, u = inp.saved.double()[:, :N], inp.saved.double()[:, c.Hp:c.Hp + N]
        sl = f_silu(g)
        esl = tol_bf16(sl, e_act(sl, g))                              # sl = bf16(g * sg)
        du = v * sl
        r = {"du": (du, tol_bf16(du, prod_err(v, ed, sl, esl)))}
        ds = v * u                                                    # ds = bf16(d * u)
        eds = tol_bf16(ds, prod_err(v, ed, u, torch.zeros_like(u)))
        h = f_dsilu(g)
        eh = e_act(h, g)
        r["dg"] = (ds * h, tol_bf16(ds * h, prod_err(ds, eds, h, eh)))
        return r
    v, S, t = acc_ref(inp.x, inp.w, inp.bias if c.bias else None, bias_rounded=(epi != "f32"))
    if epi == "bf16":
        return {"out": (v, tol_bf16(v, t))}
    if epi == "f32":
        if c.res:
            rr = inp.res32.double()
            return {"out": (v + rr, t + U * (rr.abs() + v.abs() + t))}
        return {"out": (v, t)}
    if epi == "res":
        rr = inp.res32.double()
        tb = tol_bf16(v, t)
        return {"out": (v + rr, tb + U * (rr.abs() + v.abs() + tb))}
    if epi in ("gelu", "tanh"):
        f = f_gelu if epi == "gelu" else torch.tanh
        r = {}
        tp = tol_bf16(v, t)
        if c.out2:
            r["pre"] = (v, tp)
            p, ep = got["pre"].double(), torch.zeros_like(v)
        else:
            p, ep = v, tp
        fp = f(p)
        ef = e_act(fp, p) + (2.2 * FN + LIP[epi]) * ep               # activation error at p', the slope carries the error of p' 
        r["out"] = (fp, tol_bf16(fp, ef))
        return r
    raise ValueError(epi)


def tn_reference(a, b, out0, R, splits):
    """out0 + a[:R]^T b[:R] and gamma(R + splits + 4) (|out0| + S): R products per element in any order, one fp32 atomic per split."""
    ad, bd = a[:R].double(), b[:R].double()
    v = out0.double() + ad.t() @ bd
    S = out0.double().abs() + ad.abs().t() @ bd.abs()
    return v, gamma(R + splits + 4) * S


class OutsideBound(AssertionError):
    def __init__(self, msg, index):
        super().__init__(msg)
        self.index = index


def within(name, got, ref, tol):
    """Every element of ``got`` within ``tol`` of ``ref`` (NaN fails, no element excluded); -> the worst err / tol."""
    err = (got.double() - ref).abs()
    tol = tol.expand_as(err)
    bad = ~(err <= tol)
    ratio = float(torch.where(err == 0, torch.zeros_like(err), err / (tol + 1e-300)).max()) if err.numel() else 0.0
    if bool(bad.any()):
        i = tuple(bad.nonzero()[0].tolist())
        raise OutsideBound(f"{name}: {int(bad.sum())} of {bad.numel()} outside the bound, worst err/tol {ratio:.3g}, first at {list(i)}: "
                           f"got {float(got[i])!r}, want {float(ref[i])!r} +- {float(tol[i]):.3g}", i)
    return ratio


# ------------------------------------------------------------------------------------------------
# CPU emulation of the kernels' rounding points (validates the bounds; not the reference)
# ------------------------------------------------------------------------------------------------
def emu_acc(x, w, order=0, k0=0, k1=None, drop_tile=None):
    """fp32 x w^T over k in [k0, k1) accumulated K-block by K-block.  order 0: blocks of 64 ascending (the tiled kernels' K-steps);
    order 1: blocks of 32 descending.  drop_tile = (r0, r1, c0, c1): the LAST 64-wide block is left out in that output tile (a mutation)."""
    K = x.shape[1] if k1 is None else k1
    kb = 64 if order == 0 else 32
    blocks = list(range(k0, K, kb))
    if order == 1:
        blocks = blocks[::-1]
    xf, wf = x.float(), w.float()
    acc = torch.zeros(x.shape[0], w.shape[0], dtype=torch.float32)
    last64 = (K - 1) // 64 * 64
    for s in blocks:
        e = min(s + kb, K)
        part = xf[:, s:e] @ wf[:, s:e].t()
        if drop_tile is not None and s >= last64:
            r0, r1, c0, c1 = drop_tile
            part[r0:r1, c0:c1] = 0.0
        acc = acc + part
    return acc


def trunc_bf16(t):
    """fp32 -> bf16 by dropping the low 16 bits (the WRONG conversion)."""
    return (t.float().contiguous().view(torch.int32) & -65536).view(torch.float32)


def emu_nt(c: NTCase, inp: NTInputs, order=0, mut=None, splits=0):
    """The row's outputs with the kernels' rounding points in fp32 / bf16 torch.  splits > 1: fp32 partial sums per K-slice + the
    reduction pass.  mut: a deliberately WRONG variant (tests/test_gemm_ref_cpu.py)."""
    M, N, K = c.M, c.N, c.K
    mut = mut or {}
    rnd = trunc_bf16 if mut.get("truncate") else (lambda t: t.bfloat16().float())

    def acc_of(w):
        if splits > 1:
            ks = cdiv(K // 64, splits) * 64
            parts = [emu_acc(inp.x, w, order, z * ks, min(K, (z + 1) * ks)) for z in range(cdiv(K, ks))]
            if mut.get("slice_twice"):
                parts.append(parts[-1])
            a = parts[0]
            for p in parts[1:]:
                a = a + p
            return a
        a = emu_acc(inp.x, w, order, drop_tile=mut.get("drop_tile"))
        if mut.get("swap_rows"):
            r = mut["swap_rows"]
            a[[r, r + 1]] = a[[r + 1, r]]
        return a

    def with_bias(a, b):
        if not c.bias:
            return a
        bb = b if (c.epi == "f32" or mut.get("bias_unrounded")) else b.bfloat16().float()
        bb = bb.clone()
        if mut.get("bias_skip_last4"):
            bb[ru(N, 4) - 4:] = 0.0
        return a + bb[None]

    epi = c.epi
    if epi == "swiglu":
        g, u = rnd(with_bias(acc_of(inp.w), inp.bias)), rnd(with_bias(acc_of(inp.w2), inp.bias2))
        if mut.get("swap_gu"):
            g, u = u, g
        act = rnd(rnd(f_silu(g)) * u)
        r = {"act": act}
        if c.out2:
            r["g"], r["u"] = g, u
        return r
    if epi == "gelu_bwd":
        d = rnd(acc_of(inp.w))
        return {"out": rnd(d * f_dgelu(inp.saved.float()[:, :N]))}
    if epi == "swiglu_bwd":
        d = rnd(acc_of(inp.w))
        g, u = inp.saved.float()[:, :N], inp.saved.float()[:, c.Hp:c.Hp + N]
        sg = torch.sigmoid(g)
        sl = rnd(g * sg)
        ds = rnd(d * u)
        return {"du": rnd(d * sl), "dg": rnd(ds * (sg * (1.0 + g * (1.0 - sg))))}
    a = with_bias(acc_of(inp.w), inp.bias)
    if epi == "bf16":
        return {"out": rnd(a)}
    if epi == "f32":
        return {"out": a + inp.res32 if c.res else a}
    if epi == "res":
        return {"out": inp.res32 + rnd(a)}
    if epi in ("gelu", "tanh"):
        p = rnd(a)
        r = {"out": rnd(f_gelu(p) if epi == "gelu" else torch.tanh(p))}
        if c.out2:
            r["pre"] = p
        return r
    raise ValueError(epi)


def emu_tn(a, b, out0, R, kb, splits, include_row_R=False):
    """out0 + a^T b as fm_gemm_tn adds it: each split accumulates its K-steps of kb rows in fp32 and is added to out once."""
    Rr = R + 1 if include_row_R else R
    af, bf_ = a.float(), b.float()
    nt = cdiv(R, kb)
    per = cdiv(nt, splits)
    out = out0.float().clone()
    for z in range(splits):
        acc = torch.zeros_like(out)
        for t in range(z * per, min(nt, (z + 1) * per)):
            s, e = t * kb, min((t + 1) * kb, Rr if t == nt - 1 else R)
            acc = acc + af[s:e].t() @ bf_[s:e]
        out = out + acc
    return out


def check_nt(c: NTCase, inp: NTInputs, got, label=""):
    """``within`` on every output of the row; -> {name: worst err / tol}."""
    refs = nt_reference(c, inp, got)
    assert set(refs) == set(got), (sorted(refs), sorted(got))
    return {name: within(f"{c.id}{label} {name}", got[name], ref, tol) for name, (ref, tol) in refs.items()}
