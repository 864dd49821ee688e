#!/usr/bin/env python3
"""Time FourMViT fine-tuning on one MI355X: fm_vit_base_12e_swiglu_nobias, batch 256 at 224 x 224.

Prints ms per forward, ms per forward + backward + FusedAdamW step, images/s, and the dense front end alone: fm_vit_patch_rows as GB/s
over its algorithmic bytes (B*3*224^2*4 read + B*196*768*2 written) next to the raw fm_select_embed path producing the same rows.

    python tools/time_fm_vit.py [--batch 256] [--iters 10]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "ml-4m_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402


def timed(fn, iters, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(iters + 1)]
    ev[0].record()
    for i in range(iters):
        fn()
        ev[i + 1].record()
    torch.cuda.synchronize()
    ms = sorted(ev[i].elapsed_time(ev[i + 1]) for i in range(iters))
    return ms[len(ms) // 2], ms[0], ms[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--iters", type=int, default=10)
    a = ap.parse_args()
    from fourm.hip import _lib as L, ops
    from fourm.hip.engine import fill_mod_desc, ru
    from fourm.models import fm_vit
    from fourm.utils.optim_factory import FusedAdamW
    B = a.batch
    model = fm_vit.fm_vit_base_12e_swiglu_nobias(output_head=None).cuda().train()
    fc = torch.nn.Linear(768, 1000).cuda()
    x = torch.randn(B, 3, 224, 224, device="cuda")
    y = torch.randint(0, 1000, (B,), device="cuda")
    opt = FusedAdamW([{"params": [p for p in model.parameters()], "weight_decay": 0.05}], lr=1e-4, betas=(0.9, 0.95))
    hopt = torch.optim.AdamW(fc.parameters(), lr=1e-4)

    def fwd():
        with torch.no_grad():
            return model(x)

    def train():
        loss = torch.nn.functional.cross_entropy(fc(model(x).mean(1)), y)
        loss.backward()
        opt.step(); hopt.step()
        opt.zero_grad(); hopt.zero_grad()
    res = {"batch": B}
    res["forward_ms"], _, _ = timed(fwd, a.iters)
    res["train_step_ms"], res["train_step_ms_min"], res["train_step_ms_max"] = timed(train, a.iters)
    res["train_images_per_s"] = B / res["train_step_ms"] * 1e3
    res["forward_images_per_s"] = B / res["forward_ms"] * 1e3
    # the dense front end alone against the selection kernel producing the same rows
    Np, ld = 196, 768
    R, Rp = B * Np, ru(B * Np, 128)
    rows = torch.zeros(Rp, ld, dtype=torch.bfloat16, device="cuda")
    nbytes = B * 3 * 224 * 224 * 4 + B * Np * ld * 2
    ms, lo, hi = timed(lambda: ops.vit_patch_rows(x, rows, 16), 50)
    res["patch_rows_us"], res["patch_rows_GBps"] = ms * 1e3, nbytes / ms / 1e6
    emb = model.encoder_embeddings["rgb@224"]
    desc = L.SelectDesc()
    md = {"tensor": x, "input_mask": torch.zeros(B, Np, dtype=torch.bool, device="cuda")}
    keep = fill_mod_desc(desc.mods[0], md, emb, False, 0, 0, raw=0, name="rgb@224")
    f32, i32 = torch.float32, torch.int32
    bufs = dict(tokens=torch.zeros(Rp, 768, dtype=f32, device="cuda"), emb=torch.zeros(Rp, 768, dtype=f32, device="cuda"),
                x0=torch.zeros(Rp, 768, dtype=f32, device="cuda"), mask=torch.zeros(B, Np, dtype=torch.bool, device="cuda"),
                mod=torch.zeros(B, Np, dtype=torch.int16, device="cuda"), smod=torch.zeros(B, Np, dtype=i32, device="cuda"),
                ssrc=torch.zeros(B, Np, dtype=i32, device="cuda"), spos=torch.zeros(B, Np, dtype=i32, device="cuda"),
                rows=torch.zeros(Rp, ld, dtype=torch.bfloat16, device="cuda"))
    desc.n_mods, desc.batch, desc.dim, desc.n_keep, desc.n_reg, desc.total_len = 1, B, 768, Np, 0, Np
    desc.tokens, desc.emb, desc.x0 = bufs["tokens"].data_ptr(), bufs["emb"].data_ptr(), bufs["x0"].data_ptr()
    desc.out_mask, desc.out_mod = bufs["mask"].data_ptr(), bufs["mod"].data_ptr()
    desc.slot_mod, desc.slot_src, desc.slot_pos = bufs["smod"].data_ptr(), bufs["ssrc"].data_ptr(), bufs["spos"].data_ptr()
    desc.patch_rows, desc.patch_ld = bufs["rows"].data_ptr(), ld
    ms, lo, hi = timed(lambda: L.check(L.select_embed(ops.C.byref(desc), ops._stream())), 50)
    assert torch.equal(bufs["rows"][:R], rows[:R]), "the two front ends disagree"
    # (the selection kernel also writes tokens / emb / x0 and the slot tables: its own traffic is larger than the rows alone)
    res["select_embed_us"], res["select_embed_rows_GBps"] = ms * 1e3, nbytes / ms / 1e6
    x0 = bufs["x0"]
    ms, _, _ = timed(lambda: ops.vit_emb_rows(emb.pos_emb, emb.mod_emb, x0, B, Np), 50)
    res["emb_rows_us"] = ms * 1e3
    del keep
    print(json.dumps(res))


if __name__ == "__main__":
    main()
