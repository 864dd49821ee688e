"""The engine behind ``fourm.models.fm_vit.FourMViT``: the 4M encoder on one dense RGB input, forward and backward between an image
batch and a gradient that arrives from outside (any torch head on top).

Everything but the front end is FourMEngine's: the flat parameter / gradient stores, the bf16 weight shadows, ``encoder_block_fwd`` /
``encoder_block_bwd`` with their queued dW launches, the LayerNorm kernels.  The front end is dense: every patch of every image in grid
order (fm_vit_patch_rows), the (position + modality) rows (fm_vit_emb_rows) and the projection GEMM that adds onto them in place.
"""
import torch
import torch.nn as nn

from . import _lib as L
from . import ops
from .engine import FourMEngine, ru

_NO_MASK = dict(mask_kind=L.MASK_NONE)


class ViTEngine(FourMEngine):
    def untouched_params(self):
        return []            # one modality, always present

    def _embedding(self):
        m = self.model
        return m.encoder_embeddings[f"rgb@{m.img_size}"]

    def vit_forward(self, x: torch.Tensor, save: bool) -> torch.Tensor:
        """x (B, C, H, W) -> encoder_norm(blocks(proj(patches) + pos_emb + mod_emb)) as a new fp32 (B, Np, D) tensor.
        ``save`` keeps what ``vit_backward`` needs (one forward at a time: the saved state lives in the named workspace)."""
        m, emb = self.model, self._embedding()
        self.prepare()
        if save:
            self._ensure_flat()
        px = x.float().contiguous()
        B, C, H, W = px.shape
        P = emb.patch_size[0]
        Np, D = (H // P) * (W // P), self.D
        R, Rp = B * Np, ru(B * Np, 128)
        ws = self.ws
        rows = ws.get("vit.patch_rows", (Rp, ru(P * P * C, 64)), self.adt)
        ops.vit_patch_rows(px, rows, P)
        x0 = ws.get("vit.x0", (Rp, D), torch.float32)
        ops.vit_emb_rows(emb.pos_emb, emb.mod_emb, x0, B, Np)
        ops.gemm_nt(rows, self.w(emb.proj.weight), x0, epilogue=L.EPI_RESIDUAL, res=x0, M=R, N=D)
        layers, cur = [], x0
        for i, blk in enumerate(m.encoder):
            sv = {} if save else None
            cur = self.encoder_block_fwd(blk, cur, B, Np, _NO_MASK, sv, f"enc{i}" if save else f"enc{i % 2}", defer_out=True)
            if save:
                layers.append(sv)
        out = torch.empty(R, D, dtype=torch.float32, device=px.device)
        top = {} if save else None
        if isinstance(m.encoder_norm, nn.Identity):
            self._settle()
            out.copy_(cur[:R])
        else:
            self._ln(m.encoder_norm, cur, out, R, top, "en", "top")
        self._ctx = dict(B=B, Np=Np, layers=layers, top=top, x_final=cur, rows=rows, live=P * P * C) if save else None
        return out.view(B, Np, D)

    def vit_backward(self, ctx, grad_out: torch.Tensor):
        """Backward of the ``vit_forward`` that returned ``ctx``: encoder_norm, every block (queued dW launches), the embedding.
        Accumulates into the flat gradient store; frozen parameters get nothing.  The block loop stops above the lowest layer that
        has anything trainable at or below it."""
        if ctx is None or ctx is not self._ctx:
            raise RuntimeError("FourMViT backward: the engine keeps the state of the most recent training forward only "
                               "(run forward and backward of one batch before the next forward)")
        self._ctx, self._dw_jobs = None, None
        m, emb, ws = self.model, self._embedding(), self.ws
        B, Np, D = ctx["B"], ctx["Np"], self.D
        R, Rp = B * Np, ctx["x_final"].shape[0]
        g = ws.get("bwd.g_enc", (Rp, D), torch.float32)
        g_bf = ws.get("bwd.g_enc_bf", (Rp, D), self.adt)
        go = grad_out.reshape(R, D).float().contiguous()
        if isinstance(m.encoder_norm, nn.Identity):
            g[:R].copy_(go)
            ops.f32_to_bf16(g, g_bf)
        else:
            norm, top = m.encoder_norm, ctx["top"]
            if self.fp32:
                self._ln_bwd(norm, go, ctx["x_final"], top, "en", g, g_bf, R, dres=None)
            else:       # the LayerNorm backward of the bf16 path takes a bf16 output gradient, as behind the context projection of FourM.
                # The bias gradient is the plain column sum of the head's fp32 gradient: it is taken from that, not from the rounded copy
                # (upstream's autocast keeps this norm in fp32, so its bias gradient carries no bf16 rounding either), summed in double
                # in a fixed order (fm_vit_colsum) rather than by fp32 atomics.
                dy = ws.get("bwd.vit_dy", (Rp, D), torch.bfloat16)
                ops.f32_to_bf16(go, dy[:R])
                ops.layernorm_bwd(dy, ctx["x_final"], norm.weight, top["en.mu"], top["en.rs"], g, dx_bf16=g_bf, dw=self._g(norm.weight),
                                  R=R, h=top.get("en.h"))
                if isinstance(norm.bias, nn.Parameter) and norm.bias.requires_grad:
                    ops.vit_colsum(go, self.grad_view(norm.bias), ws.get("bwd.vit_colsum", (64 * D,), torch.float64), R=R)
        emb_live = emb.proj.weight.requires_grad or emb.mod_emb.requires_grad
        live = [any(p.requires_grad for p in blk.parameters()) for blk in m.encoder]
        stop = 0 if emb_live else (live.index(True) if True in live else len(live))
        for i in reversed(range(stop, len(m.encoder))):
            self.encoder_block_bwd(m.encoder[i], ctx["layers"][i], g, g_bf, B, Np, _NO_MASK)
        if emb.proj.weight.requires_grad:
            ops.gemm_tn(g_bf, ctx["rows"], self.grad_view(emb.proj.weight), N=D, K=ctx["live"], R=R)
        if emb.mod_emb.requires_grad:
            ops.colsum(g, self.grad_view(emb.mod_emb).view(-1), D, R=R)
