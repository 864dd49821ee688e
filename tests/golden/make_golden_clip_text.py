#!/usr/bin/env python3
"""Generate tests/golden/clip_text_micro.npz from the UNMODIFIED upstream ``fourm/utils/clip/model.py::CLIP`` on the CPU.

The file is loaded by path through the oracle's import stubs (it imports only torch and numpy).  Two micro text towers (tests/clip_text_util.py
CASES) inside a ``CLIP`` with a throw-away one-layer vision tower; weights and token ids come from seeds.  Stored per case: the state-dict key
list of the text half and its shapes, an integer checksum of the regenerated inputs, and per result of ``encode_text`` (default,
return_all_tokens, return_patch_tokens): upstream's output in float64, in fp32 and under ``torch.autocast('cpu', bfloat16)``, and the distances
of the last two from the first (max |a - ref| / max |ref|).

The float64 run is upstream's class too: ``CLIP.double()``, with the instances of its ``LayerNorm`` subclass re-classed to ``nn.LayerNorm``.
That subclass only casts its input to float32 and back (the fp16 guard; the identity in an fp32 run, and what keeps the class from running in
float64 at all); nothing else of the model is touched.  Runs only where the upstream checkout exists.

    python tests/golden/make_golden_clip_text.py
"""
import copy
import importlib.util
import os
import sys

import numpy as np
import torch
from torch import nn

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)

import ref_stubs  # noqa: E402

from tests import clip_text_util as U  # noqa: E402


def load_upstream():
    ref_stubs.install()
    path = os.path.join(ref_stubs.REFERENCE_ROOT, "fourm", "utils", "clip", "model.py")
    spec = importlib.util.spec_from_file_location("upstream_clip_model", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def is_text_key(k):
    return not k.startswith("visual.") and k != "logit_scale"


def main():
    ref = load_upstream()
    out = {}
    for case, c in U.CASES.items():
        model = ref.CLIP(embed_dim=c["embed_dim"], image_resolution=16, vision_layers=1, vision_width=64, vision_patch_size=8,
                         context_length=c["context_length"], vocab_size=c["vocab_size"], transformer_width=c["width"],
                         transformer_heads=c["heads"], transformer_layers=c["layers"])
        sd = U.seeded_state_dict(case)
        res = model.load_state_dict(sd, strict=False)
        assert not res.unexpected_keys and all(not is_text_key(k) for k in res.missing_keys), res
        model.eval()
        keys = [k for k in model.state_dict().keys() if is_text_key(k)]
        assert keys == list(sd.keys()), (keys, list(sd.keys()))
        out[f"{case}/keys"] = np.array(keys)
        out[f"{case}/shapes"] = np.array([",".join(map(str, model.state_dict()[k].shape)) for k in keys])
        out[f"{case}/checksum"] = np.array(U.checksum(case), dtype=np.int64)
        m64 = copy.deepcopy(model).double()
        for mod in m64.modules():
            if type(mod) is ref.LayerNorm:
                mod.__class__ = nn.LayerNorm
        ids = U.token_ids(case)
        for flag in U.FLAGS:
            kw = U.flag_kwargs(flag)
            with torch.no_grad():
                o64 = m64.encode_text(ids, **kw)
                o32 = model.encode_text(ids, **kw)
                with torch.autocast("cpu", dtype=torch.bfloat16):
                    oac = model.encode_text(ids, **kw)
                mine = U.text_forward(sd, ids, flag, torch.float64)
            assert o64.dtype == torch.float64 and o32.dtype == torch.float32 and o32.shape == o64.shape == mine.shape
            e32, eac, eme = U.rel_max(o32, o64), U.rel_max(oac.float(), o64), U.rel_max(mine, o64)
            pre = f"{case}/{flag}"
            out[pre + "/out64"] = o64.numpy()
            out[pre + "/out32"] = o32.numpy()
            # (autocast returns bf16 for the two projected results: kept as the 16-bit patterns, clip_text_util.autocast_output widens them)
            out[pre + "/out_ac"] = oac.view(torch.int16).numpy() if oac.dtype == torch.bfloat16 else oac.numpy()
            out[pre + "/err32"] = np.array(e32)
            out[pre + "/err_ac"] = np.array(eac)
            print(f"[{pre}] shape {tuple(o32.shape)} autocast dtype {oac.dtype}: fp32 vs float64 {e32:.2e}, autocast vs float64 {eac:.2e}, "
                  f"restatement vs float64 {eme:.2e}")
    path = os.path.join(HERE, "clip_text_micro.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({os.path.getsize(path) / 1024:.0f} KiB)")


if __name__ == "__main__":
    torch.set_num_threads(min(16, os.cpu_count()))
    main()
