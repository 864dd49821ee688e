"""Builders and a plain reference for the selection / embedding stage (csrc/select_embed.hip), shared by tests/test_select_embed_cpu.py
(which proves the reference against the upstream fixtures and the oracle, no GPU) and tests/test_select_embed_kernels_gpu.py.

A ``Side`` describes one call: the modalities in concatenation order with their tables, ids and masks, plus B, D, n_keep, n_reg, is_decoder
and raw.  From it come
  * ``reference(side)``: upstream's formulation, the long way (fm.py:245-438 and the embedding modules' forward / forward_embed): embed EVERY
    position of every modality, concatenate (decoder sequences shifted for teacher forcing), ``argsort(mask + arange * 1e-6)``, gather the
    first n_keep, prepend registers, zero the masked slots, cumsum the gathered decoder_attention_mask.  It shares neither the kernel's
    integer-rank partition nor the oracle's ``stable_partition_keep``;
  * ``reference_backward(side, dx)``: the same forward in float64 under torch autograd;
  * ``DeviceCall(side)``: hand-filled ``_lib.SelectDesc`` / ``_lib.EmbedBwdDesc`` over padded, sentinel-guarded device buffers.  It does not
    go through ``engine.select`` / ``fill_mod_desc``: the tests must not share the engine's descriptor code."""
from dataclasses import dataclass
from typing import List, Optional

import torch
import torch.nn.functional as F

TOK, PATCH, SEQ, SEQ_EMB = 0, 1, 2, 3
SENT = 7.0               # float sentinel of output rows that must stay untouched
ISENT = 77               # integer sentinel


@dataclass
class Mod:
    kind: int
    L: int                                  # positions contributed to the concatenation (decoder sequences: tensor length - 1)
    vocab: int = 0
    max_len: int = 0                        # decoder sequences: position ids >= max_len collapse to 0
    mod_id: int = 0
    head_index: int = 0
    learned_pos: bool = False               # pos_emb is a parameter (receives gradient) rather than a fixed sin-cos buffer
    padding_idx: Optional[int] = None
    patch: int = 1
    channels: int = 1
    grid_w: int = 1
    orig_dim: int = 0
    ids: torch.Tensor = None                # TOK / SEQ: (B, T) int32 or int64; PATCH: (B, C, H, W) f32; SEQ_EMB: (B, L, orig_dim) f32
    mask: torch.Tensor = None               # (B, T) bool: input_mask (encoder) / target_mask (decoder), True = masked
    dam: torch.Tensor = None                # (B, T) int32 decoder_attention_mask
    table: torch.Tensor = None              # (vocab, D)
    pos: torch.Tensor = None                # (rows, D)
    mod_emb: torch.Tensor = None            # (D,)
    proj_bias: torch.Tensor = None          # (D,)  SEQ_EMB


@dataclass
class Side:
    mods: List[Mod]
    B: int
    D: int
    n_keep: int
    n_reg: int = 0
    is_decoder: bool = False
    raw: int = 0
    reg_tokens: torch.Tensor = None         # (n_reg, D)
    mask_token: torch.Tensor = None         # (D,)
    patch_ld: int = 0
    seqemb_ld: int = 0
    rows_f32: bool = False

    @property
    def total_len(self):
        return sum(m.L for m in self.mods)

    @property
    def Nt(self):
        return self.n_reg + self.n_keep

    def shifted(self, m: Mod) -> bool:
        return self.is_decoder and m.kind == SEQ and self.raw != 2


def gen(seed):
    return torch.Generator(device="cpu").manual_seed(seed)


def make_mod(g, kind, L, B, D, *, shifted=False, vocab=11, id_dtype=torch.int64, max_len=0, mod_id=1, head_index=0, learned_pos=False,
             padding_idx=None, patch=2, channels=3, grid_w=None, orig_dim=6, p_mask=0.5):
    """One modality with fresh random tables, ids and Bernoulli(p_mask) masks from the seeded CPU generator ``g``."""
    T = L + (1 if shifted else 0)
    m = Mod(kind=kind, L=L, max_len=max_len, mod_id=mod_id, head_index=head_index, learned_pos=learned_pos, padding_idx=padding_idx)
    m.mask = torch.rand(B, T, generator=g) < p_mask
    m.dam = torch.randint(0, 3, (B, T), generator=g, dtype=torch.int32)
    m.mod_emb = torch.randn(D, generator=g)
    # sequences: one row per possible rank (the encoder does not collapse positions) and one to spare
    m.pos = torch.randn(T + 1 if kind in (SEQ, SEQ_EMB) else L, D, generator=g)
    if kind in (TOK, SEQ):
        m.vocab = vocab
        m.ids = torch.randint(0, vocab, (B, T), generator=g).to(id_dtype)
        m.table = torch.randn(vocab, D, generator=g)
    elif kind == PATCH:
        gw = grid_w or L
        assert L % gw == 0
        m.patch, m.channels, m.grid_w = patch, channels, gw
        m.ids = torch.randn(B, channels, (L // gw) * patch, gw * patch, generator=g)
    else:
        m.orig_dim = orig_dim
        m.ids = torch.randn(B, L, orig_dim, generator=g)
        m.proj_bias = torch.randn(D, generator=g)
    return m


def make_side(seed, specs, B, D, n_keep=None, *, is_decoder=False, raw=0, n_reg=0, rows_f32=False, p_mask=0.5, extra_ld=4):
    """``specs``: list of (kind, L, options of make_mod).  mod_id / head_index default to distinct values that are NOT the list position."""
    g = gen(seed)
    side = Side(mods=[], B=B, D=D, n_keep=0, n_reg=n_reg, is_decoder=is_decoder, raw=raw, rows_f32=rows_f32)
    n = len(specs)
    for i, (kind, L, opt) in enumerate(specs):
        o = dict(p_mask=p_mask, mod_id=100 + 7 * i, head_index=(n - 1 - i) if is_decoder else 0)
        o.update(opt)
        side.mods.append(make_mod(g, kind, L, B, D, shifted=is_decoder and kind == SEQ and raw != 2, **o))
    side.n_keep = side.total_len if (raw or n_keep is None) else n_keep
    side.reg_tokens = torch.randn(n_reg, D, generator=g) if n_reg else None
    side.mask_token = torch.randn(D, generator=g) if is_decoder else None
    feats = [m.patch * m.patch * m.channels for m in side.mods if m.kind == PATCH]
    if feats:
        side.patch_ld = (max(feats) + 3) // 4 * 4 + extra_ld
    odims = [m.orig_dim for m in side.mods if m.kind == SEQ_EMB]
    if odims:
        side.seqemb_ld = (max(odims) + 3) // 4 * 4 + extra_ld
    return side


# ------------------------------------------------------------------------------------------------
# the reference
# ------------------------------------------------------------------------------------------------
def params_of(side: Side, dtype=torch.float32, requires_grad=False):
    """The embedding parameters as a dict of (fresh) tensors of ``dtype``: what autograd differentiates."""
    def c(t):
        return None if t is None else t.detach().to(dtype).clone().requires_grad_(requires_grad)
    return dict(mods=[dict(table=c(m.table), pos=c(m.pos), mod_emb=c(m.mod_emb), proj_bias=c(m.proj_bias)) for m in side.mods],
                mask_token=c(side.mask_token), reg_tokens=c(side.reg_tokens))


def _patchify(img, p):
    """(B, C, H, W) -> (B, H/p * W/p, p*p*C), feature (py * p + px) * C + c   (encoder_embeddings.py:301)"""
    B, C, H, W = img.shape
    return img.reshape(B, C, H // p, p, W // p, p).permute(0, 2, 4, 3, 5, 1).reshape(B, (H // p) * (W // p), p * p * C)


def _gather(t, idx):
    return torch.gather(t, 1, idx[..., None].expand(-1, -1, t.shape[2])) if t.dim() == 3 else torch.gather(t, 1, idx)


def reference(side: Side, params=None, dtype=torch.float32):
    """Every field of fm_select_desc's outputs, (B, Nt, ...) CPU tensors.  slot_src / slot_pos are defined where the slot uses them
    (slot_valid / pos_used); elsewhere the header gives them no meaning and they are 0 / -1 here."""
    P = params if params is not None else params_of(side, dtype)
    B, D, dec, raw = side.B, side.D, side.is_decoder, side.raw
    X, E, CM, TG, DAM, MID, MIX, HEAD, SRC, POS, PUSED, PR, SR = ([] for _ in range(13))
    for i, m in enumerate(side.mods):
        p = P["mods"][i]
        T = m.mask.shape[1]
        mk = m.mask.bool()
        # ---- 1. embed every position of the modality ------------------------------------------------------------------
        if m.kind in (TOK, PATCH):
            pos_ids = torch.arange(T).expand(B, T)
            pused = torch.ones(B, T, dtype=torch.bool)
            emb = (p["pos"][:T] + p["mod_emb"])[None].expand(B, T, D)
        else:
            pos_ids = (~mk).long().cumsum(1) - 1
            pos_ids = pos_ids.masked_fill(mk, 0)
            if dec:
                pos_ids = pos_ids.masked_fill(pos_ids >= m.max_len, 0)          # decoder_embeddings.py:128
            pe = F.embedding(pos_ids, p["pos"]).masked_fill(mk[..., None], 0.0)
            pused = ~mk
            emb = pe + p["mod_emb"]
        if m.kind in (TOK, SEQ):
            ids = m.ids.long()
            if dec and m.kind == TOK and raw != 2:
                x = P["mask_token"].expand(B, T, D)                             # grid targets are queried with the mask token (fm.py:322)
            else:
                x = F.embedding(ids, p["table"], padding_idx=m.padding_idx)
            src, tgt = ids, ids
        elif m.kind == PATCH:
            x = torch.zeros(B, T, D, dtype=emb.dtype)                           # the projection GEMM adds the rest
            src = tgt = torch.arange(T).expand(B, T)
        else:
            x = p["proj_bias"].expand(B, T, D)
            src = tgt = torch.arange(T).expand(B, T)
        pr = torch.zeros(B, T, side.patch_ld)
        sr = torch.zeros(B, T, side.seqemb_ld)
        if m.kind == PATCH:
            f = m.patch * m.patch * m.channels
            pr[:, :, :f] = _patchify(m.ids.float(), m.patch)
        if m.kind == SEQ_EMB:
            sr[:, :, :m.orig_dim] = m.ids.float()
        dam = m.dam if m.dam is not None else torch.zeros(B, T, dtype=torch.int32)
        cm = mk
        # ---- 2. teacher forcing: input j, target j + 1, mask m[j] | m[j+1], dam[:, :-1]   (fm.py:309-319) --------------
        if side.shifted(m):
            x, emb, tgt, src = x[:, :-1], emb[:, :-1], tgt[:, 1:], src[:, :-1]
            cm, dam = mk[:, :-1] | mk[:, 1:], dam[:, :-1]
            pos_ids, pused, pr, sr = pos_ids[:, :-1], pused[:, :-1], pr[:, :-1], sr[:, :-1]
        Lm = x.shape[1]
        assert Lm == m.L, (Lm, m.L)
        X.append(x); E.append(emb); CM.append(cm); TG.append(tgt); DAM.append(dam.int())
        MID.append(torch.full((B, Lm), m.mod_id, dtype=torch.int16)); MIX.append(torch.full((B, Lm), i, dtype=torch.int32))
        HEAD.append(torch.full((B, Lm), m.head_index, dtype=torch.int32))
        SRC.append(src); POS.append(pos_ids); PUSED.append(pused); PR.append(pr); SR.append(sr)
    X, E, CM, TG, DAM, MID, MIX, HEAD, SRC, POS, PUSED, PR, SR = (torch.cat(t, 1) for t in (X, E, CM, TG, DAM, MID, MIX, HEAD, SRC, POS, PUSED, PR, SR))
    Ptot = X.shape[1]
    # ---- 3. stable partition through the float key, first n_keep (fm.py:364-367) -----------------------------------------
    if raw:
        keep = torch.arange(Ptot).expand(B, Ptot)
    else:
        key = CM.float() + torch.arange(Ptot, dtype=torch.float32) * 1e-6
        keep = torch.argsort(key, dim=1)[:, :side.n_keep]
    # ---- 4. gather --------------------------------------------------------------------------------------------------------
    tok, emb, msk, tgt, dam, mod, mix, head, src, pos, pused, pr, sr = (_gather(t, keep) for t in (X, E, CM, TG, DAM, MID, MIX, HEAD, SRC, POS, PUSED, PR, SR))
    mod_pre = mod.clone()
    cs = dam.cumsum(1).int() if not raw else torch.zeros_like(dam)              # 7. (fm.py:459-468 consumes the cumsum)
    head = head.masked_fill(msk, -1)
    if not raw:
        # ---- 6. zero the masked slots ---------------------------------------------------------------------------------
        tok = tok.masked_fill(msk[..., None], 0.0)
        emb = emb.masked_fill(msk[..., None], 0.0)
        pr, sr = pr.masked_fill(msk[..., None], 0.0), sr.masked_fill(msk[..., None], 0.0)
        mod, mix, tgt = mod.masked_fill(msk, -1), mix.masked_fill(msk, -1), tgt.masked_fill(msk, 0)
    valid = mix >= 0
    src = torch.where(valid, src, torch.zeros_like(src))
    pos = torch.where(valid & pused, pos, torch.full_like(pos, -1))
    # ---- 5. registers in front (fm.py:375-381) ------------------------------------------------------------------------------
    if side.n_reg:
        R = side.n_reg
        reg = P["reg_tokens"][None].expand(B, R, D)
        z = lambda t, v=0: torch.full((B, R) + tuple(t.shape[2:]), v, dtype=t.dtype)
        tok, emb = torch.cat([reg, tok], 1), torch.cat([torch.zeros_like(reg), emb], 1)
        msk, mod, mod_pre, mix = torch.cat([z(msk), msk], 1), torch.cat([z(mod, -1), mod], 1), torch.cat([z(mod_pre, -1), mod_pre], 1), torch.cat([z(mix, -2), mix], 1)
        src = torch.cat([torch.arange(R).expand(B, R), src], 1)
        pos, pr, sr = torch.cat([z(pos), pos], 1), torch.cat([z(pr), pr], 1), torch.cat([z(sr), sr], 1)
        tgt, cs, head = torch.cat([z(tgt), tgt], 1), torch.cat([z(cs), cs], 1), torch.cat([z(head, -1), head], 1)
    return dict(tokens=tok, emb=emb, x0=tok + emb, out_mask=msk.to(torch.uint8), out_mod=mod, out_mod_pre=mod_pre, out_mod_index=head,
                target_ids=tgt.long(), out_cs=cs, slot_mod=mix, slot_src=src.int(), slot_pos=pos.int(), patch_rows=pr, seqemb_rows=sr,
                ids_keep=keep, dam=dam)


def dense_mask_reference(cs, mod, causal, use_cs, use_sep):
    """FourM.adapt_decoder_attention_mask (fm.py:440-475) from the already accumulated ``cs``: (B, M, M) bool, True = blocked."""
    B, M = cs.shape[0], cs.shape[1]
    col = torch.arange(M)
    if causal:
        blk = torch.ones(M, M, dtype=torch.bool).triu(1)[None].expand(B, M, M)
    elif use_cs:
        blk = col[None, None, :] >= cs[:, :, None]
    else:
        blk = torch.zeros(B, M, M, dtype=torch.bool)
    if use_sep:
        blk = blk | (mod[:, :, None] != mod[:, None, :])
    return blk


def reference_backward(side: Side, dx, zero_masked=False):
    """Gradients of sum(x0 * dx) in float64 autograd, x0 = tokens + emb of ``reference``; ``zero_masked`` drops the masked slots of a raw
    view (their slot_mod is then -1 for the kernel).  Returns {name: (grad, n, S)}: for every gradient element, n = number of contributing
    slots (the gradient of dx = 1) and S = sum of |dx| over them (the gradient of |dx|).  Names: ('table', i), ('pos', i) (learned tables
    only), ('mod_emb', i), ('proj_bias', i), 'mask_token', 'reg_tokens'."""
    P = params_of(side, torch.float64, requires_grad=True)
    r = reference(side, P, torch.float64)
    x0 = r["x0"]
    leaves = {}
    for i, m in enumerate(side.mods):
        p = P["mods"][i]
        if p["table"] is not None and not (side.is_decoder and m.kind == TOK):
            leaves[("table", i)] = p["table"]
        if m.learned_pos:
            leaves[("pos", i)] = p["pos"]
        leaves[("mod_emb", i)] = p["mod_emb"]
        if p["proj_bias"] is not None:
            leaves[("proj_bias", i)] = p["proj_bias"]
    if side.is_decoder:
        leaves["mask_token"] = P["mask_token"]
    if side.n_reg:
        leaves["reg_tokens"] = P["reg_tokens"]
    dx = dx.double()
    if zero_masked:
        dx = dx.masked_fill(r["out_mask"].bool()[..., None], 0.0)
    w_one = torch.ones_like(dx) if not zero_masked else (~r["out_mask"].bool())[..., None].expand_as(dx).double()
    names, ts = list(leaves), list(leaves.values())
    out = []
    for w in (dx, w_one, dx.abs()):
        gs = torch.autograd.grad((x0 * w).sum(), ts, retain_graph=True, allow_unused=True)
        out.append([torch.zeros_like(t) if g_ is None else g_ for g_, t in zip(gs, ts)])
    return {n: (out[0][k], out[1][k], out[2][k]) for k, n in enumerate(names)}, r


def masked_slot_tables(r):
    """The slot tables of a raw = 1 reference with the masked positions marked -1: slots of one modality separated by masked ones."""
    dead = r["out_mask"].bool()
    return r["slot_mod"].masked_fill(dead, -1), r["slot_src"].masked_fill(dead, 0), r["slot_pos"].masked_fill(dead, 0).clamp(min=0)


# ------------------------------------------------------------------------------------------------
# golden cases and the oracle
# ------------------------------------------------------------------------------------------------
_KINDS = {"tok": TOK, "patch": PATCH, "seq": SEQ, "seq_emb": SEQ_EMB}


def side_from_case(case, is_decoder, order):
    """One side of a tests.golden.cases case: its weights and batch as a ``Side`` (modalities in ``order``)."""
    cfg, sd, md = case["cfg"], case["sd"], case["mod_dict"]
    pre = "decoder_embeddings." if is_decoder else "encoder_embeddings."
    heads = [n for n in md if cfg.mod(n).in_dec]
    mods = []
    for n in order:
        s, d = cfg.mod(n), md[n]
        B = d["tensor"].shape[0]
        kind = _KINDS[s.kind]
        m = Mod(kind=kind, L=0, vocab=s.vocab, max_len=s.n_pos if s.is_seq else 0, mod_id=s.id, head_index=heads.index(n) if is_decoder else 0,
                learned_pos=n in case["learned_pos"], padding_idx=s.padding_idx if kind == SEQ else None)
        m.mask = d["target_mask" if is_decoder else "input_mask"].reshape(B, -1).bool()
        m.dam = d["decoder_attention_mask"].reshape(B, -1).int()
        m.pos, m.mod_emb = sd[pre + n + ".pos_emb"][0], sd[pre + n + ".mod_emb"][0, 0]
        if kind in (TOK, SEQ):
            m.ids, m.table = d["tensor"].reshape(B, -1), sd[pre + n + ".token_emb.weight"]
            m.L = m.ids.shape[1] - (1 if is_decoder and kind == SEQ else 0)
        elif kind == PATCH:
            m.ids, m.patch, m.channels = d["tensor"], s.patch, s.channels
            m.grid_w = d["tensor"].shape[3] // s.patch
            m.L = s.n_pos
        else:
            m.ids, m.orig_dim, m.proj_bias = d["tensor"], s.orig_dim, sd[pre + n + ".emb_proj.bias"]
            m.L = s.n_pos
        mods.append(m)
    B = mods[0].mask.shape[0]
    side = Side(mods=mods, B=B, D=cfg.dim, n_keep=case["M"] if is_decoder else case["N"], n_reg=0 if is_decoder else cfg.registers,
                is_decoder=is_decoder)
    side.reg_tokens = sd["register_tokens"][0] if side.n_reg else None
    side.mask_token = sd["mask_token"][0, 0] if is_decoder else None
    feats = [m.patch * m.patch * m.channels for m in mods if m.kind == PATCH]
    side.patch_ld = (max(feats) + 3) // 4 * 4 if feats else 0
    odims = [m.orig_dim for m in mods if m.kind == SEQ_EMB]
    side.seqemb_ld = (max(odims) + 3) // 4 * 4 if odims else 0
    return side


def to_oracle(side: Side):
    """The same data in oracle.fourm_oracle's terms: (P, cfg, mod_dict, order).  The dense projections get zero weights, so the oracle's
    token rows of PATCH / SEQ_EMB are 0 / the bias, as the kernel's are before the projection GEMM."""
    from oracle import fourm_oracle as O
    names = {TOK: "tok", PATCH: "patch", SEQ: "seq", SEQ_EMB: "seq_emb"}
    specs, Pd, md, order = [], {}, {}, []
    pre = "decoder_embeddings." if side.is_decoder else "encoder_embeddings."
    for i, m in enumerate(side.mods):
        n = f"m{i}"
        order.append(n)
        specs.append(O.ModSpec(n, names[m.kind], vocab=m.vocab, n_pos=m.max_len if (m.kind == SEQ and side.is_decoder) else m.L, patch=m.patch,
                               channels=m.channels, orig_dim=m.orig_dim, id=m.mod_id, tensor_len=m.mask.shape[1]))
        Pd[pre + n + ".pos_emb"], Pd[pre + n + ".mod_emb"] = m.pos[None], m.mod_emb[None, None]
        if m.table is not None:
            Pd[pre + n + ".token_emb.weight"] = m.table
        if m.kind == PATCH:
            Pd[pre + n + ".proj.weight"] = torch.zeros(side.D, m.patch * m.patch * m.channels)
        if m.kind == SEQ_EMB:
            Pd[pre + n + ".emb_proj.weight"], Pd[pre + n + ".emb_proj.bias"] = torch.zeros(side.D, m.orig_dim), m.proj_bias
        md[n] = dict(tensor=m.ids, input_mask=m.mask, target_mask=m.mask, decoder_attention_mask=m.dam)
    if side.is_decoder:
        Pd["mask_token"] = side.mask_token[None, None]
    if side.n_reg:
        Pd["register_tokens"] = side.reg_tokens[None]
    cfg = O.TrunkCfg(dim=side.D, registers=side.n_reg, mods=specs)
    return Pd, cfg, md, order


# ------------------------------------------------------------------------------------------------
# the kernel inputs (device)
# ------------------------------------------------------------------------------------------------
class DeviceCall:
    """Hand-filled descriptors over fresh device buffers.  mask / dam / ids are views of wider buffers (mask_stride, id_stride > L): the
    gap of the masks holds 1, of the ids an id outside the vocabulary, of the dense sources NaN.  The tables carry one extra NaN row - the
    row an id outside the vocabulary would select - so a wrong stride or index is a wrong answer, never a wild read.  Every output has one
    sentinel row past B * Nt."""

    def __init__(self, side: Side, dev="cuda", want_x0=True, gap=3):
        from fourm.hip import _lib as L
        self.L, self.side, self.dev = L, side, dev
        self.keep = []
        B, D, Nt = side.B, side.D, side.Nt
        d = self.desc = L.SelectDesc()
        nan = float("nan")

        def up(t):
            t = t.to(dev)
            self.keep.append(t)
            return t

        def table(t):
            return up(torch.cat([t.float(), torch.full((1, t.shape[1]), nan)], 0))

        for i, m in enumerate(side.mods):
            md = d.mods[i]
            T = m.mask.shape[1]
            mk = torch.ones(B, T + gap, dtype=torch.uint8)
            mk[:, :T] = m.mask.to(torch.uint8)
            md.mask, md.mask_stride = up(mk).data_ptr(), T + gap
            if side.is_decoder and m.dam is not None:
                dam = torch.full((B, T + gap), 1000, dtype=torch.int32)
                dam[:, :T] = m.dam
                md.dam = up(dam).data_ptr()
            md.kind, md.L, md.mod_id, md.head_index, md.max_len = m.kind, m.L, m.mod_id, m.head_index, m.max_len
            md.shifted = 1 if side.shifted(m) else 0
            md.pos, md.mod_emb = table(m.pos).data_ptr(), up(m.mod_emb.float()).data_ptr()
            if m.kind in (TOK, SEQ):
                ids = torch.full((B, T + gap + 2), m.vocab, dtype=m.ids.dtype)
                ids[:, :T] = m.ids
                md.ids, md.id_stride, md.ids_are_i64 = up(ids).data_ptr(), T + gap + 2, 1 if m.ids.dtype == torch.int64 else 0
                md.table = table(m.table).data_ptr()
            else:
                flat = m.ids.float().reshape(B, -1)
                src = torch.full((B, flat.shape[1] + gap), nan)
                src[:, :flat.shape[1]] = flat
                md.ids, md.id_stride = up(src).data_ptr(), flat.shape[1] + gap
                if m.kind == PATCH:
                    md.patch, md.channels, md.grid_w = m.patch, m.channels, m.grid_w
                else:
                    md.orig_dim, md.proj_bias = m.orig_dim, up(m.proj_bias.float()).data_ptr()
        d.n_mods, d.batch, d.dim, d.n_keep, d.n_reg, d.total_len = len(side.mods), B, D, side.n_keep, side.n_reg, side.total_len
        d.is_decoder, d.raw = int(side.is_decoder), side.raw
        if side.n_reg:
            d.reg_tokens = up(side.reg_tokens.float()).data_ptr()
        if side.is_decoder:
            d.mask_token = up(side.mask_token.float()).data_ptr()
        R = B * Nt
        self.out = {}

        def out(name, dtype, cols=None, fill=ISENT):
            t = torch.full((R + 1,) if cols is None else (R + 1, cols), fill, dtype=dtype, device=dev)
            self.out[name] = t
            return t.data_ptr()

        d.tokens, d.emb = out("tokens", torch.float32, D, SENT), out("emb", torch.float32, D, SENT)
        if want_x0:
            d.x0 = out("x0", torch.float32, D, SENT)
        d.out_mask, d.out_mod = out("out_mask", torch.uint8), out("out_mod", torch.int16)
        d.slot_mod, d.slot_src, d.slot_pos = out("slot_mod", torch.int32), out("slot_src", torch.int32), out("slot_pos", torch.int32)
        if side.is_decoder:
            d.target_ids, d.out_cs = out("target_ids", torch.int64), out("out_cs", torch.int32)
            d.out_mod_pre, d.out_mod_index = out("out_mod_pre", torch.int16), out("out_mod_index", torch.int32)
        rdt = torch.float32 if side.rows_f32 else torch.bfloat16
        if side.patch_ld:
            d.patch_rows, d.patch_ld = out("patch_rows", rdt, side.patch_ld, SENT), side.patch_ld
        if side.seqemb_ld:
            d.seqemb_rows, d.seqemb_ld = out("seqemb_rows", rdt, side.seqemb_ld, SENT), side.seqemb_ld
        d.rows_f32 = int(side.rows_f32)

    def launch(self):
        import ctypes as C
        return self.L.select_embed(C.byref(self.desc), C.c_void_p(torch.cuda.current_stream().cuda_stream))

    def results(self):
        """({name: (B, Nt, ...) CPU tensor}, every sentinel row intact)"""
        torch.cuda.synchronize()
        s, res, intact = self.side, {}, True
        for k, t in self.out.items():
            c = t.cpu()
            intact = intact and bool((c[-1] == (SENT if c.is_floating_point() else ISENT)).all())
            res[k] = c[:-1].reshape((s.B, s.Nt) + tuple(c.shape[1:]))
        return res, intact


class DeviceBwd:
    """A hand-filled ``_lib.EmbedBwdDesc``.  ``names``: the gradients to ask for (keys of ``reference_backward``); every other pointer stays
    NULL.  Each buffer is (rows + 1, D), pre-filled with seeded random values (the kernel accumulates), the last row a guard that no slot
    addresses.  dx is (B * Nt, D + pad) with NaN in the padding columns.  Slot tables: CPU or device int32 (B, Nt)."""

    def __init__(self, side: Side, slot_mod, slot_src, slot_pos, dx, names, dev="cuda", seed=0, pad=4, dim=None, lddx=None):
        from fourm.hip import _lib as L
        self.L, self.side = L, side
        B, D, Nt = side.B, side.D, side.Nt
        g = gen(1000 + seed)
        d = self.desc = L.EmbedBwdDesc()
        self.keep = [t.to(dev).int().contiguous() for t in (slot_mod, slot_src, slot_pos)]
        d.slot_mod, d.slot_src, d.slot_pos = (t.data_ptr() for t in self.keep)
        buf = torch.full((B * Nt, D + pad), float("nan"))
        buf[:, :D] = dx.reshape(B * Nt, D).float()
        self.dx = buf.to(dev)
        d.dx, d.lddx = self.dx.data_ptr(), lddx if lddx is not None else D + pad
        d.n_mods, d.batch, d.dim, d.Nt, d.is_decoder = len(side.mods), B, dim if dim is not None else D, Nt, int(side.is_decoder)
        self.pre, self.buf = {}, {}
        rows = {"table": lambda m: m.vocab, "pos": lambda m: m.pos.shape[0], "mod_emb": lambda m: 1, "proj_bias": lambda m: 1}
        for i, m in enumerate(side.mods):
            md = d.mods[i]
            md.kind = m.kind
            md.has_padding_idx, md.padding_idx = (1, m.padding_idx) if m.padding_idx is not None else (0, 0)
        for n in names:
            r = (1 if n == "mask_token" else side.n_reg) if isinstance(n, str) else rows[n[0]](side.mods[n[1]])
            self.pre[n] = torch.randn(r + 1, D, generator=g)
            self.buf[n] = self.pre[n].to(dev)
            ptr = self.buf[n].data_ptr()
            if n == "mask_token":
                d.d_mask_token = ptr
            elif n == "reg_tokens":
                d.d_reg_tokens = ptr
            else:
                setattr(d.mods[n[1]], "d_" + n[0], ptr)

    def launch(self):
        import ctypes as C
        return self.L.embed_bwd(C.byref(self.desc), C.c_void_p(torch.cuda.current_stream().cuda_stream))

    def results(self):
        torch.cuda.synchronize()
        return {n: (self.buf[n].cpu(), self.pre[n]) for n in self.buf}
