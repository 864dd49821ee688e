"""ml-4m_amd/save_vq_tokens.py end to end on a small folder: upstream's file names, shapes and dtypes; tokens equal to ``model.tokenize`` of
crops made by the numpy restatement of Pillow (tests/pil_resize_util.py) with the saved settings; replay with --force_load_crop; --dryrun."""
import argparse
import os

import numpy as np
import pytest
import torch

from tests import pil_resize_util as U

pytestmark = pytest.mark.gpu
SIZES = [(40, 56), (64, 33), (32, 32), (70, 50), (45, 45), (38, 90)]


def _folder(root, task="rgb"):
    from PIL import Image
    rng = np.random.default_rng(12)
    images = {}
    for i, (H, W) in enumerate(SIZES):
        cls = f"class_{i % 2}"
        os.makedirs(os.path.join(root, "train", task, cls), exist_ok=True)
        a = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        Image.fromarray(a, mode="RGB").save(os.path.join(root, "train", task, cls, f"img{i:03d}.png"))
        images[(cls, f"img{i:03d}")] = a
    return images


def _tokenizer(tmp_path):
    from fourm.vq import VQVAE
    torch.manual_seed(0)
    m = VQVAE(image_size=32, n_channels=3, enc_type="vit_s_enc", dec_type="vit_s_dec", patch_size=8, codebook_size=64, latent_dim=8, post_mlp=True)
    args = dict(domain="rgb", input_size=32, encoder_type="vit_s_enc", decoder_type="vit_s_dec", quantizer_type="lucid", patch_size=8, codebook_size=64,
                latent_dim=8, num_codebooks=1, norm_codes=True, norm_latents=False, post_mlp=True, quantizer_ema_decay=0.97, lr=1e-4, batch_size=32)
    path = tmp_path / "tok_rgb.pth"
    torch.save({"model": m.state_dict(), "args": argparse.Namespace(**args)}, path)
    return str(path)


def _tree(root):
    return sorted(os.path.relpath(os.path.join(d, f), root) for d, _, fs in os.walk(root) for f in fs)


@pytest.mark.parametrize("task", ["rgb", "normal"])
def test_script_writes_upstreams_files_and_the_restatements_tokens(tmp_path, task):
    pytest.importorskip("PIL")
    import save_vq_tokens as S
    root = str(tmp_path / "data")
    images = _folder(root, task)
    ckpt = _tokenizer(tmp_path)
    argv = ["--data_root", root, "--split", "train", "--task", task, "--n_crops", "3", "--min_crop_scale", "0.2", "--input_size", "32", "--tokenizer_ckpt", ckpt,
            "--folder_suffix", "tok", "--batch_size", "4", "--batch_size_dataloader", "4", "--num_workers", "2", "--seed", "3"]
    before = _tree(root)
    S.main(S.get_args(argv + ["--dryrun"]))
    assert _tree(root) == before                                                         # a dry run writes nothing
    done, _ = S.main(S.get_args(argv))
    assert done == 6
    model = S.load_tokenizer(S.get_args(argv)).cuda().eval()
    inv = (0,) if task == "normal" else ()
    tokens, crops = {}, []
    order = sorted(images)                                                               # the script's order: classes, then files
    for (cls, name) in order:
        img = images[(cls, name)]
        st = np.load(os.path.join(root, "train", "crop_settings", cls, f"{name}.npy"))
        tk = np.load(os.path.join(root, "train", f"{task}_tok", cls, f"{name}.npy"))
        assert st.shape == (3, 5) and np.issubdtype(st.dtype, np.integer) and tk.shape == (3, 16) and tk.dtype == np.int16
        H, W = img.shape[:2]
        side = min(H, W)
        assert tuple(st[0]) == (((H - side) // 2 if H > W else 0), (0 if H > W else (W - side) // 2), side, side, 0)
        crops.append(np.stack([U.crop_resize(img, s, 32, "bicubic", inv) for s in st]))
        tokens[(cls, name)] = tk
    # model.tokenize of the restatement's crops, in the script's sub-batches (4 images per loader batch, 4 crops per sub-batch)
    for b in range(0, 6, 4):
        x = torch.from_numpy(np.concatenate(crops[b:b + 4])).permute(0, 3, 1, 2).contiguous().to(torch.float32).div(255).sub_(0.5).div_(0.5).cuda()
        with torch.no_grad():
            want = torch.cat([model.tokenize(sub).reshape(sub.shape[0], -1) for sub in x.split(4, dim=0)]).cpu().numpy().astype(np.int16)
        for i, key in enumerate(order[b:b + 4]):
            assert np.array_equal(tokens[key], want[3 * i:3 * i + 3]), key
    assert len({t.tobytes() for t in tokens.values()}) > 1
    assert len(_tree(root)) == len(before) + 12
    # a second run skips what exists; after the tokens are deleted, --force_load_crop replays the saved settings to the same tokens
    assert S.main(S.get_args(argv))[0] == 0
    for (cls, name) in images:
        os.remove(os.path.join(root, "train", f"{task}_tok", cls, f"{name}.npy"))
    assert S.main(S.get_args(argv + ["--force_load_crop", "--seed", "99"]))[0] == 6
    for (cls, name), tk in tokens.items():
        assert np.array_equal(np.load(os.path.join(root, "train", f"{task}_tok", cls, f"{name}.npy")), tk)
    os.remove(os.path.join(root, "train", "crop_settings", "class_0", "img000.npy"))
    os.remove(os.path.join(root, "train", f"{task}_tok", "class_0", "img000.npy"))
    with pytest.raises(FileNotFoundError):
        S.main(S.get_args(argv + ["--force_load_crop"]))


def test_script_tokenizes_class_maps(tmp_path):
    """semseg_coco: palette PNGs, ``convert('P')``, shifted up by one, nearest whatever --resample_mode says, int64 into the tokenizer's class
    embedding."""
    pytest.importorskip("PIL")
    from PIL import Image
    import save_vq_tokens as S
    from fourm.vq import VQVAE
    root = str(tmp_path / "data")
    rng = np.random.default_rng(13)
    maps = {}
    for i, (H, W) in enumerate(SIZES[:3]):
        os.makedirs(os.path.join(root, "val", "semseg_coco", "c"), exist_ok=True)
        a = rng.integers(0, 10, (H // 4 + 1, W // 4 + 1), dtype=np.uint8).repeat(4, 0).repeat(4, 1)[:H, :W]
        im = Image.fromarray(np.ascontiguousarray(a), mode="P")
        im.putpalette([v for k in range(256) for v in (k, 255 - k, (7 * k) % 256)])
        im.save(os.path.join(root, "val", "semseg_coco", "c", f"m{i}.png"))
        maps[f"m{i}"] = a
    torch.manual_seed(1)
    m = VQVAE(image_size=32, n_channels=16, n_labels=11, enc_type="vit_s_enc", dec_type="vit_s_dec", patch_size=8, codebook_size=64, latent_dim=8, post_mlp=True)
    args = dict(domain="semseg_coco", input_size=32, encoder_type="vit_s_enc", decoder_type="vit_s_dec", quantizer_type="lucid", patch_size=8, codebook_size=64,
                latent_dim=8, num_codebooks=1, norm_codes=True, norm_latents=False, post_mlp=True, quantizer_ema_decay=0.97, lr=1e-4, batch_size=32)
    torch.save({"model": m.state_dict(), "args": argparse.Namespace(**args)}, tmp_path / "tok_seg.pth")
    argv = ["--data_root", root, "--split", "val", "--task", "semseg_coco", "--n_crops", "3", "--min_crop_scale", "0.2", "--input_size", "32", "--resample_mode", "bicubic",
            "--tokenizer_ckpt", str(tmp_path / "tok_seg.pth"), "--folder_suffix", "tok", "--batch_size", "16", "--seed", "4"]
    assert S.main(S.get_args(argv))[0] == 3
    model = S.load_tokenizer(S.get_args(argv)).cuda().eval()
    crops = []
    for name in sorted(maps):
        st = np.load(os.path.join(root, "val", "crop_settings", "c", f"{name}.npy"))
        crops.append(np.stack([U.crop_resize((maps[name] + 1)[:, :, None], s, 32, "nearest")[..., 0] for s in st]))
    x = torch.from_numpy(np.concatenate(crops).astype(np.int64)).cuda()
    assert int(x.min()) >= 1 and int(x.max()) <= 10
    with torch.no_grad():
        want = model.tokenize(x).reshape(9, -1).cpu().numpy().astype(np.int16)
    for i, name in enumerate(sorted(maps)):
        tk = np.load(os.path.join(root, "val", "semseg_coco_tok", "c", f"{name}.npy"))
        assert tk.shape == (3, 16) and tk.dtype == np.int16 and np.array_equal(tk, want[3 * i:3 * i + 3]), name
