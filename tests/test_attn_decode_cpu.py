"""fm_attn_decode without a GPU: the symbol is declared, exported and bound with a matching prototype and struct layout, and
``autoregressive_generate`` no longer refuses qk_norm / fp32 models."""
import ctypes
import inspect
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    return open(os.path.join(ROOT, "include", "fourm_hip.h")).read()


def test_attn_decode_is_declared_exported_and_bound():
    from fourm.hip import _lib
    header = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    m = re.search(r"\bint\s+fm_attn_decode\s*\(([^)]*)\)\s*;", header)
    assert m, "fm_attn_decode is not declared in include/fourm_hip.h"
    params = [p.strip() for p in m.group(1).split(",")]
    assert len(params) == 2 and "fm_attn_decode_args*" in params[0].replace(" *", "*") and "*" in params[1], params
    assert "fm_attn_decode" in _lib.EXPORTS and hasattr(_lib.lib, "fm_attn_decode")
    fn = _lib.attn_decode
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == 2
    assert fn.argtypes[0]._type_ is _lib.AttnDecodeArgs and fn.argtypes[1] is ctypes.c_void_p
    assert int(re.search(r"#define FM_ATTN_DECODE_MAX_NK (\d+)", header).group(1)) == _lib.ATTN_DECODE_MAX_NK
    assert _lib.lib.fm_abi_version() == _lib.ABI_VERSION == int(re.search(r"#define FM_ABI_VERSION (\d+)", header).group(1))
    with open(os.path.join(ROOT, "ml-4m_amd", "build_ext.py")) as f:
        assert '"attn_decode.hip"' in f.read()


def test_attn_decode_args_mirror_matches_the_header_layout(tmp_path):
    """sizeof and every field offset of fm_attn_decode_args as the C compiler lays it out, against the ctypes mirror."""
    from fourm.hip import _lib
    if shutil.which("gcc") is None:
        pytest.skip("no C compiler")
    body = re.search(r"typedef struct fm_attn_decode_args \{(.*?)\} fm_attn_decode_args;", _header(), re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [re.search(r"([A-Za-z_][A-Za-z0-9_]*)\s*$", part.strip()).group(1)
             for decl in body.split(";") if decl.strip() for part in decl.split(",")]
    assert names == [f[0] for f in _lib.AttnDecodeArgs._fields_]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "fourm_hip.h"', 'int main(void) {',
             '  printf("size %zu\\n", sizeof(fm_attn_decode_args));']
    lines += [f'  printf("{n} %zu\\n", offsetof(fm_attn_decode_args, {n}));' for n in names]
    lines += ["  return 0;", "}"]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines))
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = dict(l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert ctypes.sizeof(_lib.AttnDecodeArgs) == int(out["size"])
    for n in names:
        assert getattr(_lib.AttnDecodeArgs, n).offset == int(out[n]), n


def test_autoregressive_generate_no_longer_refuses_qk_norm_or_fp32():
    from fourm.hip import ops
    from fourm.models.generate import GenerationSampler
    src = inspect.getsource(GenerationSampler.autoregressive_generate)
    assert "covers the bf16 models without qk_norm" not in src
    assert not re.search(r"if eng\.qk_norm or eng\.fp32:\s*\n\s*raise", src)
    assert "ops.attn_decode(" in src and callable(ops.attn_decode)
    assert "ops.attn_fwd(" in src                                   # the bf16 trunks without qk_norm keep their launch sequence
