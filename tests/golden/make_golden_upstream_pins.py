#!/usr/bin/env python3
"""Fixtures for the tests that pin this package's oracle and host helpers against the UNMODIFIED upstream code (container only:
needs the upstream tree, see ref_stubs.py).  Upstream runs here once on fixed inputs; its results go to

    tests/golden/upstream_pins.npz    tensors: image masks, codebook EMA / k-means, DropPath / zero-attention loss and gradient sketches, schedules
    tests/golden/upstream_pins.json   host values: span-masking merges, get_args() namespaces and their YAML inputs, run names

so that the tests run anywhere.          python tests/golden/make_golden_upstream_pins.py"""
import importlib.util
import json
import os
import random
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
import ref_stubs  # noqa: E402

ref_stubs.install()
REF = ref_stubs.REFERENCE_ROOT

from tests.golden.cases import CODEBOOK_EMA_CASES, build_case, codebook_ema_inputs, grad_projections  # noqa: E402

T, J = {}, {}


def load(rel, name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(REF, rel))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def merge_span():
    """tests/test_generate_cpu.py::test_merge_matches_upstream_helpers (inputs: its FakeTokenizer and random.Random(0) draws)."""
    from tests.test_generate_cpu import FakeTokenizer
    ref = load("fourm/utils/tokenizer/text_tokenizer.py", "ref_text_tokenizer")
    tok = FakeTokenizer()
    sent = set(ref.get_sentinel_to_id_mapping(tok).values())
    rng = random.Random(0)
    cases = []
    for _ in range(200):
        inp = [rng.choice(list(range(5, 10)) + list(range(20, 40))) for _ in range(rng.randint(1, 12))]
        dec = [rng.choice(list(range(5, 10)) + list(range(20, 40))) for _ in range(rng.randint(0, 16))]
        cases.append([inp, dec, ref.merge_span_masking(inp, dec, sent)])
    J["merge_span"] = {"sentinel_ids": sorted(sent), "cases": cases}


IMAGE_MASK_CASES = ((196, 40, 60, 0), (196, 0, 196, 1), (196, 196, 0, 2), (64, 10, None, 3), (196, 128, 68, 4), (16, 3, 0, 5))


def image_mask():
    """tests/test_masking.py::test_image_mask_oracle_matches_upstream: UnifiedMasking.image_mask after torch.manual_seed(seed)."""
    from fourm.data.masking import UnifiedMasking
    for i, (L_, kin, kt, seed) in enumerate(IMAGE_MASK_CASES):
        torch.manual_seed(seed)
        ref = UnifiedMasking.image_mask(None, torch.zeros(L_), L_, kin, kt)
        for k in ("input_mask", "target_mask", "decoder_attention_mask"):
            T[f"image_mask.{i}.{k}"] = ref[k].numpy()


def codebook_ema():
    """tests/test_vq_ema_oracle.py: CosineSimCodebook in training mode on the inputs of cases.codebook_ema_inputs; the forward runs after
    torch.manual_seed(123)."""
    from fourm.vq.quantizers.quantize_lucid import CosineSimCodebook
    for K, R, thr in CODEBOOK_EMA_CASES:
        cb = CosineSimCodebook(dim=32, codebook_size=K, decay=0.9, threshold_ema_dead_code=thr, code_replacement_policy="batch_random")
        e0, c0, z = codebook_ema_inputs(K, R)
        cb.embed.copy_(e0)
        cb.cluster_size.copy_(c0)
        cb.train()
        torch.manual_seed(123)
        _, ind = cb(z)
        T[f"codebook_ema.{K}.ind"] = ind.detach().numpy().astype(np.int16)
        T[f"codebook_ema.{K}.embed"], T[f"codebook_ema.{K}.cluster"] = cb.embed.detach().numpy(), cb.cluster_size.detach().numpy()


def kmeans():
    """tests/test_vq.py::test_kmeans_oracle_matches_upstream (inputs: its _clustered point sets)."""
    from fourm.vq.quantizers.quantize_lucid import kmeans as ref_kmeans, l2norm
    from tests.test_vq import _clustered
    for K, per, seed in ((16, 20, 0), (64, 3, 1), (8, 2, 2)):
        x = l2norm(_clustered(K, per, 32, seed))
        idx = torch.randperm(x.shape[0], generator=torch.Generator().manual_seed(seed))[:K + 3]
        means, bins = ref_kmeans(x, K + 3, 10, use_cosine_sim=True, sample_fn=lambda s, n: s[idx])
        T[f"kmeans.{seed}.means"], T[f"kmeans.{seed}.bins"] = means.numpy(), bins.numpy()


def _loss_and_grads(tag, model, case):
    random.seed(case["order_seed"])
    from make_golden import clone_mod_dict
    loss, _ = model(clone_mod_dict(case["mod_dict"]), case["N"], case["M"], loss_type=case["loss_type"])
    loss.sum().backward()
    T[f"{tag}.loss"] = np.float64(float(loss.detach().sum()))
    names = [k for k, p in model.named_parameters() if p.grad is not None and float(p.grad.norm()) > 1e-8]
    grads = dict(model.named_parameters())
    J.setdefault("grad_params", {})[tag] = names                 # row i of grad_norm / grad_proj = names[i]
    T[f"{tag}.grad_norm"] = np.array([float(grads[k].grad.double().norm()) for k in names])
    T[f"{tag}.grad_proj"] = np.stack([grad_projections(k, grads[k].grad) for k in names])
    return loss


def drop_path():
    """tests/test_model_cpu.py::test_oracle_drop_path_matches_upstream: upstream blocks with DropPath(p) replaying seeded draws."""
    import make_golden as MG
    case = build_case("micro_swiglu")
    cfg, sd = case["cfg"], case["sd"]
    model = MG.upstream_model(cfg, case["share_embedding"], case["norm_bias"], case["learned_pos"])
    model.load_state_dict(sd, strict=True)
    model.train()
    B = next(iter(case["mod_dict"].values()))["tensor"].shape[0]
    pe = [0.2 + 0.1 * i for i in range(cfg.enc_depth)]
    pd = [0.3 + 0.1 * i for i in range(cfg.dec_depth)]
    for blk, p in zip(list(model.encoder) + list(model.decoder), pe + pd):
        blk.drop_path = MG.ref_utils.DropPath(p)
    g = torch.Generator().manual_seed(4)
    draws = [torch.rand(B, generator=g) for _ in range(2 * cfg.enc_depth + 3 * cfg.dec_depth)]
    it = iter(draws)
    real = torch.rand

    def fake(*a, **k):
        shape = a[0] if a and isinstance(a[0], (tuple, list, torch.Size)) else a
        if len(shape) == 3 and tuple(shape[1:]) == (1, 1):
            return next(it).reshape(shape).to(k.get("dtype", torch.float32))
        return real(*a, **k)
    torch.rand = fake
    try:
        _loss_and_grads("drop_path", model, case)
    finally:
        torch.rand = real
    assert next(it, None) is None


def zero_attn():
    """tests/test_model_cpu.py::test_oracle_zero_attn_matches_upstream: upstream attention modules with allow_zero_attn set."""
    import make_golden as MG
    for name in ("micro_swiglu", "micro_qknorm"):
        case = build_case(name)
        model = MG.upstream_model(case["cfg"], case["share_embedding"], case["norm_bias"], case["learned_pos"])
        model.load_state_dict(case["sd"], strict=True)
        for mod in model.modules():
            if hasattr(mod, "allow_zero_attn"):
                mod.allow_zero_attn = True
        model.train()
        _loss_and_grads(f"zero_attn.{name}", model, case)


SCHEDULES = {
    "cosine": ((dict(base_value=1e-3, final_value=1e-6, epochs=5, niter_per_ep=37, warmup_epochs=1),
                dict(base_value=2e-4, final_value=0.0, epochs=3, niter_per_ep=50, warmup_epochs=-1, warmup_steps=40),
                dict(base_value=0.05, final_value=0.05, epochs=4, niter_per_ep=11))),
    "inverse_sqrt": ((dict(base_value=1e-3, final_value=1e-5, epochs=6, niter_per_ep=40, warmup_epochs=1, cooldown_epochs=1, timescale=100),
                      dict(base_value=1e-3, final_value=1e-3, epochs=2, niter_per_ep=40, warmup_steps=7, cooldown_steps=9),
                      dict(base_value=4e-4, final_value=0.0, epochs=3, niter_per_ep=25))),
}
RUN_NAMES = (dict(run_name="auto", config_path="cfgs/default/4m/models/main/4m-b_mod7_500b.yaml", wandb_run_name="auto",
                  output_dir="output/auto", s3_save_dir="s3://bucket/auto/x"),
             dict(run_name="mine", config_path="", wandb_run_name="auto", output_dir="out/auto"),
             dict(run_name="auto", config_path="/abs/cfgs/a/b/c.yaml", output_dir=""))
CONFIGS = ("cfgs/default/4m/models/main/4m-b_mod7_500b.yaml", "cfgs/default/4m/models/main/4m-l_mod21_500b.yaml")
GET_ARGS = (["-c", "{0}"],
            ["-c", "{0}", "--batch_size", "64", "--no_fixed_eval", "--opt_betas", "0.9", "0.99", "--clip_grad", "3.0", "--dtype", "bf16"],
            ["--epochs", "3", "--scheduler", "inverse_sqrt-10000", "--no_auto_resume", "--eval", "--log_wandb", "--find_unused_params"],
            ["-c", "{1}", "--no_pin_mem", "--no_compute_grad_norm"])


def trainer():
    """tests/test_trainer_cpu.py: upstream's schedules, setup_run_name and get_args() (the YAMLs it reads are stored as data: the
    test writes them back to a file and gives our get_args the same command line)."""
    from argparse import Namespace
    import yaml
    S = load("fourm/utils/scheduler.py", "upstream_scheduler")
    for kind, kws in SCHEDULES.items():
        for i, kw in enumerate(kws):
            T[f"schedule.{kind}.{i}"] = np.asarray(getattr(S, f"{kind}_scheduler")(**kw))
    T["schedule.constant"] = np.asarray(S.constant_scheduler(0.3, 2, 5))
    R = load("fourm/utils/run_name.py", "upstream_run_name")
    names = []
    for kw in RUN_NAMES:
        a = Namespace(**kw)
        R.setup_run_name(a)
        names.append([kw, vars(a)])
    J["run_name"] = names
    U = load("run_training_4m.py", "upstream_trainer")
    paths = [os.path.join(REF, c) for c in CONFIGS]
    J["configs"] = [[os.path.basename(c), yaml.safe_load(open(p))] for c, p in zip(CONFIGS, paths)]        # "{i}" in argv = configs[i]
    J["get_args"] = []
    for argv in GET_ARGS:
        sys.argv = ["run_training_4m.py"] + [x.format(*paths) for x in argv]
        ns = vars(U.get_args())
        for p, c in zip(paths, CONFIGS):          # the config paths are placeholders: the test substitutes where it wrote the YAML
            ns = {k: ("{%d}" % CONFIGS.index(c) if v == p else v) for k, v in ns.items()}
        J["get_args"].append([argv, json.loads(json.dumps(ns))])


if __name__ == "__main__":
    for f in (merge_span, image_mask, codebook_ema, kmeans, drop_path, zero_attn, trainer):
        f()
    np.savez_compressed(os.path.join(HERE, "upstream_pins.npz"), **T)
    with open(os.path.join(HERE, "upstream_pins.json"), "w") as fh:
        json.dump(J, fh, indent=0, sort_keys=True)
    print(f"{len(T)} arrays, {len(J)} host records")
