#!/usr/bin/env python3
"""Dataset pre-tokenization: upstream's ``save_vq_tokens.py`` with the data stage on the device.

Same flags and folder layout as upstream: images under ``<data_root>/<split>/<task>/<class>/<id>.<ext>``, crop settings in
``<data_root>/<split>/crop_settings/<class>/<id>.npy`` (int (n_crops, 5) rows of top, left, h, w, flip; created when absent, replayed when
present, required with ``--force_load_crop``), tokens in ``<data_root>/<split>/<task>_<folder_suffix>/<class>/<id>.npy`` as int16
(n_crops, n_tokens); files that exist are skipped.

What differs is where the work happens.  Upstream makes every crop with Pillow on a loader worker; here a pool of at most 16 host threads
only decodes (``Image.open`` + ``convert``), and all crops of a loader batch are made in one call of ``fourm.data.crops.crop_resize``
- Pillow's bytes, flipped, normalised through a lookup table - and tokenized through ``fourm.vq.tokenize_sub_batches``.

Tasks: ``rgb`` (RGB, upstream's tokenizer statistics mean = std = 0.5, IMAGENET_INCEPTION_*), ``normal`` (RGB, mean = std = 0.5, channel 0
becomes 255 - v in flipped crops), ``semseg*`` (``convert('P')``, always nearest, int64 class maps; ``semseg_coco`` is shifted up by one
as upstream's registry does), and the feature tasks ``CLIP-B16``, ``DINOv2-B14``, ``DINOv2-B14-global``: the images are read from the ``rgb``
folder with rgb's crops and normalisation, the frozen tower (fourm/utils/clip, fourm/utils/dinov2) turns every crop into a feature map or a
global embedding, and the tokenizer reads that (fourm.data.features).  The tower's weights come from a local state-dict file named by the
environment variable FOURM_FEATURE_EXTRACTOR_CKPT (there is no flag for it: the command line stays upstream's); unset, the task is refused.
Refused by name: depth, --mask_value, SAM instances, ImageBind and any other feature task, and --corrupt_samples_log; see REFUSED.  ``--tokenizer_ckpt`` names a checkpoint file directly (``--tokenizer_id`` is resolved under
``--tokenizers_root`` as upstream does)."""
import argparse
import datetime
import os
import random
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

IMG_EXTENSIONS = (".bmp", ".gif", ".jpeg", ".jpg", ".jpx", ".pgm", ".png", ".ppm", ".tif", ".tiff", ".webp")          # the suffixes upstream's folder scan takes
MAX_DECODE_THREADS = 16
TASKS = {      # task -> (Pillow mode, mean, std, channels inverted on flip, output)
    "rgb": ("RGB", (0.5, 0.5, 0.5), (0.5, 0.5, 0.5), (), "float32"),
    "normal": ("RGB", (0.5, 0.5, 0.5), (0.5, 0.5, 0.5), (0,), "float32"),
}
FEATURE_TASKS = ("CLIP-B16", "DINOv2-B14", "DINOv2-B14-global")      # fourm.data.features.FEATURE_TASKS: the frozen tower runs in front of the tokenizer
REFUSED = {
    "depth": "16-bit depth maps do not go through Pillow's 8-bit resize path (and are standardised per crop)",
    "sam_instance": "SAM instances are sets of masks with boxes, not one image per file",
    "sam_mask": "SAM instances are sets of masks with boxes, not one image per file",
    "feature": "the feature tasks whose frozen feature extractor is built here are CLIP-B16, DINOv2-B14 and DINOv2-B14-global",
    "ImageBind-H14": "feature tasks need the frozen feature extractor in front of the tokenizer",
    "ImageBind-H14-global": "feature tasks need the frozen feature extractor in front of the tokenizer",
}


# The command line: upstream's flag names, types, defaults and actions (the interface; tests/golden/save_vq_tokens_flags.json records them),
# plus --tokenizer_ckpt.  (flag, type, default, what it does here)
VALUE_FLAGS = [
    ("--tokenizer_id", str, "cc12m/rgb_ViTB-UNetP4_16k_224-448", "tokenizer checkpoint to use: <tokenizers_root>/<tokenizer_id>.pth"),
    ("--tokenizers_root", str, "./tokenizer_ckpts", "folder that --tokenizer_id is resolved in"),
    ("--tokenizer_ckpt", str, None, "a checkpoint file given directly (.pth); takes precedence over --tokenizer_id (this script only)"),
    ("--data_root", str, "/path/to/dataset", "dataset folder; images are read from <data_root>/<split>/<task>/<class>/"),
    ("--split", str, "train", "sub-folder of the dataset to work on"),
    ("--n_crops", int, 1, "crops per image: the first is the unflipped centre crop, any further ones are random crops with a random flip"),
    ("--min_crop_scale", float, 0.8, "smallest area fraction of a random crop"),
    ("--input_size", int, 224, "side of the square every crop is resized to"),
    ("--task", str, "rgb", "modality to tokenize: rgb, normal, semseg*, CLIP-B16, DINOv2-B14 or DINOv2-B14-global"),
    ("--mask_value", float, None, "refused by this script (masking with the valid-mask modality is not built)"),
    ("--resample_mode", str, None, "Pillow filter of the resize: bilinear, bicubic, nearest; unset means Pillow's default (bicubic)"),
    ("--corrupt_samples_log", str, None, "refused by this script (delete the bad token files and run again)"),
    ("--device", None, "cuda", "device the crops and the tokenizer run on"),
    ("--seed", int, 0, "seed of the crop draws (the rank is added)"),
    ("--folder_suffix", str, "dvae_BUa_224", "tokens go to <data_root>/<split>/<task>_<folder_suffix>/"),
    ("--num_workers", int, 16, f"host threads that decode images, capped at {MAX_DECODE_THREADS}"),
    ("--batch_size_dataloader", int, 64, "images whose crops are made in one device call"),
    ("--batch_size", int, 64, "crops per tokenizer sub-batch"),
    ("--world_size", int, 1, "accepted for compatibility; sharding follows the RANK / WORLD_SIZE environment"),
    ("--local_rank", int, -1, "accepted for compatibility"),
    ("--dist_url", None, "env://", "accepted for compatibility"),
]
SWITCHES = [      # (flag, value when given, dest, default, what it does here)
    ("--verbose", True, "verbose", False, "print the running rate after every batch"),
    ("--dryrun", True, "dryrun", False, "go through every step but write neither crop settings nor tokens"),
    ("--pin_mem", True, "pin_mem", True, "accepted for compatibility: the upload buffer is always pinned"),
    ("--no_pin_mem", False, "pin_mem", True, "accepted for compatibility"),
    ("--dist_on_itp", True, "dist_on_itp", False, "accepted for compatibility"),
    ("--force_load_crop", True, "force_load_crop", False, "never draw crop settings: a missing crop_settings file is an error"),
]


def build_parser():
    parser = argparse.ArgumentParser(prog="save_vq_tokens", description="Pre-tokenize an image folder with the crops made on the device.")
    for flag, typ, default, text in VALUE_FLAGS:
        kw = {} if typ is None else {"type": typ}
        parser.add_argument(flag, default=default, help=f"{text} (default: {default})", **kw)
    for flag, value, dest, default, text in SWITCHES:
        parser.add_argument(flag, action="store_true" if value else "store_false", dest=dest, default=default, help=text)
    return parser


def get_args(argv=None):
    return build_parser().parse_args(argv)


def task_config(args):
    """(mode, mean, std, invert_on_flip, out, resample, shift) of the task, or NotImplementedError / ValueError naming what is refused and why.
    Nothing is loaded or launched before this has returned."""
    task = args.task
    if args.mask_value is not None:
        raise NotImplementedError("--mask_value is not supported here: the valid-mask modality and its masking are not part of this script")
    if args.corrupt_samples_log is not None:
        raise NotImplementedError("--corrupt_samples_log is not supported here: delete the corrupt token files and run again")
    for key, name in ((task, task), ("depth", "depth"), ("sam", "sam_instance"), ("CLIP", "feature"), ("DINO", "feature"), ("ImageBind", "ImageBind-H14")):
        if key in task and name in REFUSED and task not in FEATURE_TASKS:
            raise NotImplementedError(f"task {task!r} is not supported here: {REFUSED[name]}")
    if args.resample_mode not in (None, "bilinear", "bicubic", "nearest"):
        raise ValueError(f"--resample_mode {args.resample_mode}: one of bilinear, bicubic, nearest (or leave it unset)")
    if args.n_crops < 1 or args.input_size < 1 or args.batch_size < 1 or args.batch_size_dataloader < 1:
        raise ValueError("--n_crops, --input_size, --batch_size and --batch_size_dataloader are positive")
    if task in FEATURE_TASKS:
        # upstream's loader task of a feature task is rgb (save_vq_tokens.py:216): the same crops and (x - 0.5) / 0.5 normalisation go to the
        # extractor unchanged.  Its weights: a local state-dict file named by FOURM_FEATURE_EXTRACTOR_CKPT (refused here when unset or missing)
        from fourm.data.features import checkpoint_path
        checkpoint_path(task)
        return (*TASKS["rgb"], args.resample_mode, 0)
    if task in TASKS:
        return (*TASKS[task], args.resample_mode, 0)
    if task.startswith("semseg"):
        return ("P", None, None, (), "int64", "nearest", 1 if task == "semseg_coco" else 0)
    raise NotImplementedError(f"task {task!r} is not supported here: known tasks are {sorted(TASKS)} and semseg*")


def find_samples(root):
    """[(path, class, id)] under root/<class>/..., classes and files in sorted order (torchvision's DatasetFolder order)."""
    classes = sorted(e.name for e in os.scandir(root) if e.is_dir())
    if not classes:
        raise FileNotFoundError(f"{root} has no class sub-folders")
    out = []
    for cls in classes:
        for d, _, files in sorted(os.walk(os.path.join(root, cls), followlinks=True)):
            for f in sorted(files):
                if f.lower().endswith(IMG_EXTENSIONS):
                    out.append((os.path.join(d, f), os.path.basename(d), f.split(".")[0]))
    return out


def decode(path, mode, shift):
    """Pillow decode + convert -> uint8 (H, W, C)."""
    from PIL import Image
    with Image.open(path) as img:
        a = np.asarray(img.convert(mode))
    if a.ndim == 2:
        a = a[:, :, None]
    if shift:
        a = a + np.uint8(shift)          # uint8 arithmetic, as upstream's ``np.asarray(sample) + 1``
    return np.ascontiguousarray(a, dtype=np.uint8)


def load_tokenizer(args):
    from fourm.vq import get_image_tokenizer
    if args.tokenizer_ckpt is not None:
        root, name = os.path.split(os.path.abspath(args.tokenizer_ckpt))
        if not name.endswith(".pth"):
            raise ValueError(f"--tokenizer_ckpt {args.tokenizer_ckpt}: a .pth file expected")
        return get_image_tokenizer(name[:-4], tokenizers_root=root, encoder_only=True)[0]
    return get_image_tokenizer(args.tokenizer_id, tokenizers_root=args.tokenizers_root, encoder_only=True)[0]


def settings_for(sample, shape, root, args):
    """The crop settings of one image: loaded when present (or required), else drawn and saved."""
    from fourm.data.crops import make_crop_settings
    path = os.path.join(root, "crop_settings", sample[1], f"{sample[2]}.npy")
    if not os.path.isfile(path):
        if args.force_load_crop:
            raise FileNotFoundError(f"--force_load_crop: no crop settings at {path}")
        st = make_crop_settings(shape[0], shape[1], args.n_crops, args.min_crop_scale)
        if not args.dryrun:
            os.makedirs(os.path.dirname(path), exist_ok=True)
            np.save(path, st)
        return st
    return np.load(path)


def main(args, model=None, extractor=None):
    """Returns (images tokenized, seconds of the loop).  ``model``: a tokenizer already on the device (else loaded from the arguments);
    ``extractor``: the feature network of a feature task (else built from the file FOURM_FEATURE_EXTRACTOR_CKPT names)."""
    mode, mean, std, invert, out, resample, shift = task_config(args)
    feature = args.task in FEATURE_TASKS
    import torch
    from fourm.data.crops import crop_resize
    from fourm.vq import tokenize_sub_batches
    if not torch.cuda.is_available():
        raise RuntimeError("save_vq_tokens runs on the HIP kernels only (an MI355X is needed; there is no CPU path)")
    rank = int(os.environ.get("RANK", 0))
    world = int(os.environ.get("WORLD_SIZE", 1))
    seed = args.seed + rank
    torch.manual_seed(seed)
    np.random.seed(seed)
    random.seed(seed)
    device = torch.device(args.device)
    if model is None:
        model = load_tokenizer(args)
    model = model.to(device).eval()
    if feature:
        from fourm.data.features import feature_maps, load_feature_extractor
        if extractor is None:
            extractor = load_feature_extractor(args.task)
        extractor = extractor.to(device).eval().requires_grad_(False)
    root = os.path.join(args.data_root, args.split)
    tokens_root = os.path.join(root, f"{args.task}_{args.folder_suffix}")
    samples = find_samples(os.path.join(root, "rgb" if feature else args.task))[rank::world]
    samples = [s for s in samples if not os.path.exists(os.path.join(tokens_root, s[1], f"{s[2]}.npy"))]
    print(f"{len(samples)} images to tokenize ({args.task}, {args.n_crops} crops each); crop settings are {'only loaded' if args.force_load_crop else 'loaded or drawn'}")
    start, done = time.time(), 0
    workers = max(1, min(int(args.num_workers), MAX_DECODE_THREADS))
    batches = [samples[i:i + args.batch_size_dataloader] for i in range(0, len(samples), args.batch_size_dataloader)]
    with ThreadPoolExecutor(max_workers=workers) as pool, torch.cuda.device(device):
        ahead = pool.map(lambda s: decode(s[0], mode, shift), batches[0]) if batches else None
        for b, batch in enumerate(batches):
            images = list(ahead)
            if b + 1 < len(batches):          # the next batch decodes while this one is on the device
                ahead = pool.map(lambda s: decode(s[0], mode, shift), batches[b + 1])
            settings = [settings_for(s, im.shape, root, args) for s, im in zip(batch, images)]
            for s, st in zip(batch, settings):
                if st.shape != (args.n_crops, 5):
                    raise ValueError(f"crop settings of {s[1]}/{s[2]}: shape {st.shape}, expected {(args.n_crops, 5)}")
            crops = crop_resize(images, settings, args.input_size, resample=resample, mean=mean, std=std, invert_on_flip=invert, out=out)
            with torch.no_grad():
                subs = crops.split(args.batch_size, dim=0)
                if feature:          # (the towers run on the current stream; the tokenizer's sub-batches then overlap as for image tasks)
                    subs = [feature_maps(args.task, extractor, sb) for sb in subs]
                toks = tokenize_sub_batches(model, subs)
            toks = torch.cat([t.reshape(t.shape[0], -1) for t in toks]).cpu().numpy().astype(np.int16)
            toks = toks.reshape(len(batch), args.n_crops, -1)
            for s, t in zip(batch, toks):
                path = os.path.join(tokens_root, s[1], f"{s[2]}.npy")
                if args.dryrun:
                    print(f"[dry run] would write {path}")
                else:
                    os.makedirs(os.path.dirname(path), exist_ok=True)
                    np.save(path, t)
            done += len(batch)
            if args.verbose:
                print(f"{done} / {len(samples)} images, {done / max(time.time() - start, 1e-9):.1f} images/s", flush=True)
    total = time.time() - start
    print(f"done: {done} images in {datetime.timedelta(seconds=int(total))}")
    return done, total


if __name__ == "__main__":
    main(get_args())
