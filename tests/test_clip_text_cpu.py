"""CLIP's text tower without a GPU: the float64 yardstick of the GPU tests (tests/clip_text_util.py::text_forward) is pinned to upstream's
``CLIP.encode_text`` through tests/golden/clip_text_micro.npz, the module has upstream's parameter tree for the text half and loads its
checkpoints strictly, ``build_text`` reads the sizes off a state dict, what the HIP path does not do is refused in Python, and the new C symbols
are declared, exported and bound."""
import ctypes
import os
import re

import pytest
import torch

from tests import clip_text_util as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["fm_clip_text_embed", "fm_clip_pair_score_scratch", "fm_clip_pair_score", "fm_l2_normalize_rows"]


def build(case, **over):
    from fourm.utils.clip.text import TextTransformer
    return TextTransformer(**{**U.CASES[case], **over})


@pytest.fixture(scope="module")
def gold():
    return U.load_golden()


@pytest.mark.parametrize("case", list(U.CASES))
def test_inputs_are_the_ones_the_fixture_was_made_from(case, gold):
    assert int(gold[f"{case}/checksum"]) == U.checksum(case)
    ids = U.token_ids(case)
    assert ids.dtype == torch.int64 and tuple(ids.shape) == (U.BATCH[case], U.CASES[case]["context_length"])
    assert ids.argmax(dim=-1).tolist() == U.eot_positions(case) and int(ids.max()) == U.CASES[case]["vocab_size"] - 1
    top = (ids == ids.max(dim=-1, keepdim=True).values).sum(-1).tolist()
    assert sorted(top) == sorted([2 if second is not None else 1 for _, second in U.EOT[case]])      # one row carries its maximum twice
    # position 1, the middle and Lc - 1 all occur over the two cases
    Lc_a, Lc_b = U.CASES["text_a"]["context_length"], U.CASES["text_b"]["context_length"]
    assert U.eot_positions("text_a") == [1, Lc_a // 2, Lc_a - 1] and U.eot_positions("text_b") == [Lc_b // 2, Lc_b - 1]


@pytest.mark.parametrize("case", list(U.CASES))
def test_restatement_reproduces_upstreams_float64_and_fp32_outputs(case, gold):
    """text_forward in float64 against upstream's float64 run: 1e-12 relative.  In float32 against upstream's fp32 run: within 8 x the distance
    of that run from float64 (the rule of tests/test_clip_cpu.py: two fp32 evaluations of one function differ by about that distance; a wrong
    formula - mask, eps, head split, QuickGELU constant, the row that is picked - is off by 1e-3 or more)."""
    sd, ids = U.seeded_state_dict(case), U.token_ids(case)
    for flag in U.FLAGS:
        ref64 = torch.from_numpy(gold[f"{case}/{flag}/out64"])
        got64 = U.text_forward(sd, ids, flag, torch.float64)
        assert got64.shape == ref64.shape and got64.dtype == torch.float64
        err64 = U.rel_max(got64, ref64)
        assert err64 <= 1e-12, (case, flag, err64)
        ref32 = torch.from_numpy(gold[f"{case}/{flag}/out32"])
        got32 = U.text_forward(sd, ids, flag, torch.float32)
        assert got32.shape == ref32.shape and got32.dtype == torch.float32
        err, bound = U.rel_max(got32, ref32), 8 * float(gold[f"{case}/{flag}/err32"])
        assert err <= bound, (case, flag, err, bound)
        # the recorded distances are those of the stored arrays
        assert U.rel_max(ref32, ref64) == pytest.approx(float(gold[f"{case}/{flag}/err32"]), rel=1e-6)
        assert U.rel_max(U.autocast_output(gold, case, flag), ref64) == pytest.approx(float(gold[f"{case}/{flag}/err_ac"]), rel=1e-6)


def test_fixture_shapes_are_the_documented_ones(gold):
    assert gold["text_a/default/out64"].shape == (3, 40) and gold["text_a/return_all_tokens/out32"].shape == (3, 12, 40)
    assert gold["text_a/return_patch_tokens/out32"].shape == (3, 12, 128)
    assert gold["text_b/default/out64"].shape == (2, 64) and gold["text_b/return_all_tokens/out32"].shape == (2, 77, 64)
    assert gold["text_b/return_patch_tokens/out64"].shape == (2, 77, 64)


@pytest.mark.parametrize("case", list(U.CASES))
def test_state_dict_layout_and_strict_load(case, gold):
    model = build(case)
    keys = [str(k) for k in gold[f"{case}/keys"]]
    sd = model.state_dict()
    assert list(sd.keys()) == keys == [k for k, _ in U.expected_shapes(case)]
    assert len(keys) == 5 + 12 * U.CASES[case]["layers"]
    assert [",".join(map(str, sd[k].shape)) for k in keys] == [str(s) for s in gold[f"{case}/shapes"]]
    filled = U.seeded_state_dict(case)
    model.load_state_dict(filled, strict=True)                                 # an upstream-keyed dict into this module ...
    assert all(torch.equal(model.state_dict()[k], filled[k]) for k in keys)
    other = build(case)
    other.load_state_dict(model.state_dict(), strict=True)                     # ... and this module's own dict back
    assert all(torch.equal(other.state_dict()[k], filled[k]) for k in keys)
    assert set(n for n, _ in model.named_parameters()) == set(keys)            # every entry is a parameter, as upstream


def test_initialisation_is_upstreams():
    """CLIP.initialize_parameters: token rows std 0.02, position rows 0.01, in_proj width^-0.5, out_proj / c_proj width^-0.5 (2 layers)^-0.5,
    c_fc (2 width)^-0.5, text_projection width^-0.5; LayerNorms at (1, 0) with eps 1e-5, in_proj_bias zero."""
    torch.manual_seed(0)
    m = build("text_a", vocab_size=4000)
    w, layers = U.CASES["text_a"]["width"], U.CASES["text_a"]["layers"]
    blk = m.transformer.resblocks[1]
    for p, std in ((m.token_embedding.weight, 0.02), (m.positional_embedding, 0.01), (blk.attn.in_proj_weight, w ** -0.5),
                   (blk.attn.out_proj.weight, w ** -0.5 * (2 * layers) ** -0.5), (blk.mlp.c_fc.weight, (2 * w) ** -0.5),
                   (blk.mlp.c_proj.weight, w ** -0.5 * (2 * layers) ** -0.5), (m.text_projection, w ** -0.5)):
        assert 0.9 * std < float(p.detach().std()) < 1.1 * std, (tuple(p.shape), float(p.detach().std()), std)
    for ln in (m.ln_final, blk.ln_1, blk.ln_2):
        assert ln.eps == 1e-5 and bool((ln.weight == 1).all()) and bool((ln.bias == 0).all())
    assert bool((blk.attn.in_proj_bias == 0).all())
    assert (m.embed_dim, m.context_length, m.vocab_size, m.width, m.heads) == (40, 12, 4000, 128, 2)


@pytest.mark.parametrize("full", [True, False])
def test_build_text_recovers_the_sizes(full):
    from fourm.utils.clip.text import build_text
    for case, cfg in U.CASES.items():
        sd = {k: v.half() for k, v in U.seeded_state_dict(case).items()}
        if full:                                                               # a full CLIP dict carries the vision tower and the scalars too
            sd.update({"visual.proj": torch.zeros(8, 8), "visual.transformer.resblocks.0.attn.in_proj_weight": torch.zeros(24, 8),
                       "visual.transformer.resblocks.5.ln_1.weight": torch.zeros(8), "logit_scale": torch.tensor(2.0),
                       "input_resolution": torch.tensor(1), "context_length": torch.tensor(1), "vocab_size": torch.tensor(1)})
        m = build_text(sd)
        assert (m.embed_dim, m.context_length, m.vocab_size, m.width, m.heads, len(m.transformer.resblocks)) == \
            (cfg["embed_dim"], cfg["context_length"], cfg["vocab_size"], cfg["width"], cfg["heads"], cfg["layers"])
        assert not m.training and all(p.dtype == torch.float32 and not p.requires_grad for p in m.parameters())
        assert torch.equal(m.text_projection, sd["text_projection"].float())
    with pytest.raises(NotImplementedError, match="text tower"):
        build_text({"visual.proj": torch.zeros(4, 4)})


def test_from_upstream_adopts_the_text_half_of_a_clip_module():
    from fourm.utils.clip.text import TextTransformer

    class FakeClip(torch.nn.Module):                                           # the state dict of a CLIP: text half, vision half, logit_scale
        def __init__(self, text):
            super().__init__()
            self.positional_embedding, self.text_projection = text.positional_embedding, text.text_projection
            self.logit_scale = torch.nn.Parameter(torch.ones([]))
            self.visual = torch.nn.Linear(4, 4)
            self.transformer, self.token_embedding, self.ln_final = text.transformer, text.token_embedding, text.ln_final

    src = build("text_a")
    src.load_state_dict(U.seeded_state_dict("text_a"))
    got = TextTransformer.from_upstream(FakeClip(src))
    assert got is not src and not got.training and not any(p.requires_grad for p in got.parameters())
    assert list(got.state_dict().keys()) == list(src.state_dict().keys())
    assert all(torch.equal(a, b) for a, b in zip(got.state_dict().values(), src.state_dict().values()))


def test_refusals():
    from fourm.utils.clip.text import TextTransformer, clip_logits
    with pytest.raises(NotImplementedError, match="head_dim"):
        TextTransformer(40, 12, 50, 128, 4, 1)                                 # head_dim 32
    with pytest.raises(NotImplementedError, match="head_dim"):
        TextTransformer(40, 12, 50, 96, 1, 1)                                  # head_dim 96
    m = build("text_a")
    assert m.compute_precision == "bf16"
    m.compute_precision = "fp32"
    with pytest.raises(ValueError, match="compute_precision"):
        m.compute_precision = "fp16"
    assert m.compute_precision == "fp32"
    ids = U.token_ids("text_a")
    with pytest.raises(NotImplementedError, match="inference only"):           # gradients enabled, trainable parameters
        m(ids)
    m.requires_grad_(False)
    with pytest.raises(ValueError, match=r"\(B, 12\)"):                        # a wrong context length
        m(ids[:, :11])
    with pytest.raises(ValueError, match="int64 or int32"):
        m(ids.float())
    with pytest.raises(TypeError, match="tokenize"):
        m(["a photo of a cat"])
    with pytest.raises(RuntimeError, match="GPU"):                             # a CPU model says where it computes: no torch fall-back
        m(ids)
    with pytest.raises(RuntimeError, match="GPU"):
        m.encode_text(ids.int(), return_all_tokens=True)
    with torch.no_grad(), pytest.raises(RuntimeError, match="GPU"):
        build("text_a")(ids)
    with pytest.raises(RuntimeError, match="no CPU path"):
        clip_logits(torch.zeros(5, 40), torch.zeros(7, 40), 1.0)
    with pytest.raises(ValueError, match="clip_logits"):
        clip_logits(torch.zeros(5, 40), torch.zeros(7, 41), 1.0)


def test_clip_score_refuses_strings_and_cpu_tensors():
    from fourm.utils.clip.score import ClipScore
    metric = ClipScore(None, build("text_a").requires_grad_(False))
    with pytest.raises(TypeError, match=r"fourm\.utils\.clip\.tokenize"):
        metric.update(torch.zeros(1, 3, 32, 32), "a photo of a cat")
    with pytest.raises(TypeError, match=r"fourm\.utils\.clip\.tokenize"):
        metric.update(torch.zeros(2, 3, 32, 32), ["a photo of a cat", "a dog"])
    with pytest.raises(TypeError, match=r"fourm\.utils\.clip\.tokenize"):
        metric.update_features(torch.zeros(1, 40), ["a photo of a cat"])
    with pytest.raises(ValueError, match="one shape"):
        metric.update_features(torch.zeros(2, 40), torch.zeros(3, 40))
    with pytest.raises(RuntimeError, match="no CPU path"):
        metric.update_features(torch.zeros(2, 40), torch.zeros(2, 40))
    assert metric.compute() != metric.compute()                                # nothing seen: nan


def test_new_symbols_are_declared_exported_and_bound():
    from fourm.hip import _lib
    header = open(os.path.join(ROOT, "include", "fourm_hip.h")).read()
    assert re.search(r"#define FM_ABI_VERSION 11\b", header) and _lib.ABI_VERSION == 11 and _lib.lib.fm_abi_version() == 11
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint %s\(" % name, header), name
        assert name in _lib.EXPORTS and hasattr(_lib.lib, name), name
        assert getattr(_lib.lib, name).restype is ctypes.c_int
    assert len(_lib.clip_text_embed.argtypes) == 13 and len(_lib.clip_pair_score.argtypes) == 11 and len(_lib.l2_normalize_rows.argtypes) == 9
    assert _lib.l2_normalize_rows.argtypes[7] is ctypes.c_float
    assert "clip_text.hip" in open(os.path.join(ROOT, "ml-4m_amd", "build_ext.py")).read()
    # host-side refusals need no GPU: null pointers and non-positive sizes come back as -1 with a message
    assert _lib.clip_text_embed(None, None, None, None, 0, None, None, None, 1, 1, 4, 1, None) == -1
    assert b"fm_clip_text_embed" in _lib.lib.fm_last_error()
    assert _lib.clip_pair_score_scratch(0) == -1 and _lib.clip_pair_score_scratch(5) == 2
    assert _lib.clip_pair_score(None, 1, None, 1, None, None, None, None, 1, 1, None) == -1
    assert _lib.l2_normalize_rows(None, 1, None, 1, 1, 1, None, 1.0, None) == -1


def test_package_exports_and_default_launches_of_the_block_loop():
    import inspect

    from fourm.utils import clip
    from fourm.utils.clip import score, text
    from fourm.vq import engine
    assert clip.TextTransformer is text.TextTransformer and clip.build_text is text.build_text and clip.clip_logits is text.clip_logits
    assert clip.ClipScore is score.ClipScore and clip.TextTransformer.encode_text is clip.TextTransformer.forward
    sig = inspect.signature(engine._blocks_fwd)
    assert sig.parameters["mask"].default is None and list(sig.parameters)[:7] == ["eng", "vit", "stream", "B", "G", "st", "prefix"]
