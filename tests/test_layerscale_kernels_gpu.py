"""fm_layernorm_fwd_res_ls, fm_layerscale_add (csrc/layerscale.hip) and fm_cls_pos_embed (csrc/dinov2.hip) on a real MI355X.

LayerScale's sum is eager torch's - the product gamma * float(delta) rounded to fp32, then the sum rounded to fp32 - so x_out is compared with
torch.equal against the CPU's x + gamma * delta.float().  The norm behind it is held to the rule tests/test_kernels_gpu.py::
test_layernorm_with_residual_add applies to the kernel it extends: y, mean and rstd are the bits of fm_layernorm_fwd run on that x_out.
Shapes: one row, row counts that are no multiple of the 4 rows of a workgroup, more than one workgroup, and every width class of the kernel
(2, 3 and 8 float4 chunks per lane; 192 and 1536 fill their last chunk partly)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
SHAPES = [(1, 128), (129, 192), (300, 768), (17, 1536)]


def _ops():
    from fourm.hip import _lib as L
    from fourm.hip import ops
    return ops, L


def _inputs(R, D, ld=None, seed=0):
    """CPU tensors: x (R, D) f32, delta bf16 and f32, gamma in [-1.5, 1.5], w, b."""
    g = torch.Generator().manual_seed(100 + seed)
    x = torch.randn(R, D, generator=g) * 2 + 0.5
    d32 = torch.randn(R, D, generator=g)
    gamma = 3.0 * torch.rand(D, generator=g) - 1.5
    w, b = torch.randn(D, generator=g) * 0.2 + 1, torch.randn(D, generator=g) * 0.1
    return x, d32.bfloat16(), d32, gamma, w, b


def _strided(t, ld):
    """The same values in a device buffer with row stride ld, the pad columns poisoned."""
    buf = torch.full((t.shape[0], ld), 9.0, dtype=t.dtype, device=DEV)
    buf[:, :t.shape[1]] = t.to(DEV)
    return buf[:, :t.shape[1]]


@pytest.mark.parametrize("R,D", SHAPES)
def test_layerscale_add_equals_the_cpu_sum(R, D):
    ops, L = _ops()
    x, d16, d32, gamma, _, _ = _inputs(R, D)
    for delta in (d16, d32):
        want = x + gamma * delta.float()                     # CPU: product rounded to fp32, sum rounded to fp32
        out = torch.full((R, D), 7.0, device=DEV)
        ops.layerscale_add(x.to(DEV), delta.to(DEV), gamma.to(DEV), out)
        assert torch.equal(out.cpu(), want), (R, D, delta.dtype)
        # not the fused multiply-add (one rounding): the inputs must be able to tell the two apart
        fused = torch.addcmul(x.double(), gamma.double(), delta.double()).float()
        if R * D >= 128:
            assert not torch.equal(fused, want)
        xs = x.to(DEV).clone()                                # in place
        ops.layerscale_add(xs, delta.to(DEV), gamma.to(DEV), xs)
        assert torch.equal(xs.cpu(), want)


@pytest.mark.parametrize("R,D", SHAPES)
def test_layernorm_res_ls(R, D):
    ops, L = _ops()
    x, d16, _, gamma, w, b = _inputs(R, D, seed=1)
    want = x + gamma * d16.float()
    xd, dd, gd, wd, bd = (t.to(DEV) for t in (x, d16, gamma, w, b))
    for ydt in (torch.bfloat16, torch.float32):
        xo = torch.full((R, D), 7.0, device=DEV)
        y = torch.zeros(R, D, device=DEV, dtype=ydt)
        mean, rstd = torch.zeros(R, device=DEV), torch.zeros(R, device=DEV)
        ops.layernorm_fwd(xd, wd, bd, y, mean, rstd, delta=dd, x_out=xo, gamma=gd)
        assert torch.equal(xo.cpu(), want)
        y2, m2, r2 = torch.zeros_like(y), torch.zeros_like(mean), torch.zeros_like(rstd)
        ops.layernorm_fwd(want.to(DEV), wd, bd, y2, m2, r2)
        assert torch.equal(y, y2) and torch.equal(mean, m2) and torch.equal(rstd, r2), (R, D, ydt)
    # gamma == 1: every output has the bits of fm_layernorm_fwd_res
    one = torch.ones(D, device=DEV)
    outs = []
    for gm in (one, None):
        xo, y = torch.full((R, D), 7.0, device=DEV), torch.zeros(R, D, device=DEV, dtype=torch.bfloat16)
        mean, rstd = torch.zeros(R, device=DEV), torch.zeros(R, device=DEV)
        ops.layernorm_fwd(xd, wd, None, y, mean, rstd, delta=dd, x_out=xo, gamma=gm)
        outs.append((xo, y, mean, rstd))
    assert all(torch.equal(a, c) for a, c in zip(*outs))
    # scattered rows with skipped ones: x_out is written for every row, y only where the map says
    perm = torch.randperm(R, generator=torch.Generator().manual_seed(5)).int()
    perm[::7] = -1
    perm = perm.to(DEV)
    xo = torch.full((R, D), 7.0, device=DEV)
    ys, yr = torch.full((R, D), 3.0, device=DEV, dtype=torch.bfloat16), torch.full((R, D), 3.0, device=DEV, dtype=torch.bfloat16)
    ops.layernorm_fwd(xd, wd, bd, ys, row_map=perm, delta=dd, x_out=xo, gamma=gd)
    ops.layernorm_fwd(want.to(DEV), wd, bd, yr, row_map=perm)
    assert torch.equal(ys, yr) and torch.equal(xo.cpu(), want)
    untouched = torch.ones(R, dtype=torch.bool)
    untouched[perm[perm >= 0].long().cpu()] = False
    assert bool((ys.cpu()[untouched] == 3.0).all())


@pytest.mark.parametrize("R,D", [(129, 192), (17, 1536)])
def test_strided_leading_dims(R, D):
    ops, L = _ops()
    x, d16, d32, gamma, w, b = _inputs(R, D, seed=2)
    want = x + gamma * d16.float()
    xs, ds, fs = _strided(x, D + 8), _strided(d16, D + 12), _strided(d32, D + 4)
    xo, y = _strided(torch.zeros(R, D), D + 16), _strided(torch.zeros(R, D, dtype=torch.bfloat16), D + 4)
    ops.layernorm_fwd(xs, w.to(DEV), b.to(DEV), y, delta=ds, x_out=xo, gamma=gamma.to(DEV))
    y2 = torch.zeros(R, D, device=DEV, dtype=torch.bfloat16)
    ops.layernorm_fwd(want.to(DEV), w.to(DEV), b.to(DEV), y2)
    assert torch.equal(xo.cpu(), want) and torch.equal(y, y2)
    for delta, wnt in ((ds, want), (fs, x + gamma * d32)):
        out = _strided(torch.zeros(R, D), D + 20)
        ops.layerscale_add(xs, delta, gamma.to(DEV), out)
        assert torch.equal(out.cpu(), wnt)
        base = out._base if out._base is not None else out
        assert bool((base[:, D:] == 9.0).all())                         # nothing written past a row
    with pytest.raises(RuntimeError, match="fm_layerscale_add"):          # a row stride shorter than the row is refused
        L.check(L.layerscale_add(ops._p(xs), D - 4, ops._p(ds), ds.stride(0), 0, ops._p(gamma.to(DEV)), ops._p(xo), xo.stride(0), R, D, ops._stream()))


@pytest.mark.parametrize("f32", [False, True], ids=["bf16", "f32"])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("n_reg", [0, 4])
def test_cls_pos_embed(B, n_reg, f32):
    ops, L = _ops()
    G, D = 24, 192
    g = torch.Generator().manual_seed(7)
    patches = torch.randn(B * G, D, generator=g)
    patches = patches if f32 else patches.bfloat16()
    cls, pos = torch.randn(1, 1, D, generator=g), torch.randn(1 + G, D, generator=g)
    reg = torch.randn(n_reg, D, generator=g) if n_reg else None
    t = torch.cat([cls.expand(B, 1, D), patches.float().view(B, G, D)], 1) + pos
    if n_reg:
        t = torch.cat([t[:, :1], reg.expand(B, n_reg, D), t[:, 1:]], 1)
    T = 1 + n_reg + G
    pbuf = _strided(patches, D + 8)
    out = _strided(torch.zeros(B * T, D), D + 4)
    ops.cls_pos_embed(pbuf, cls.to(DEV), None if reg is None else reg.to(DEV), pos.to(DEV), out, B, G, D)
    assert torch.equal(out.cpu(), t.reshape(B * T, D))
    assert bool((out._base[:, D:] == 9.0).all())
