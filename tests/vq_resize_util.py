"""Shared pieces of the resize tests (fourm.vq.resize, csrc/resize.hip): the size pairs, the float64 reference (F.interpolate on the CPU, the
contract) and the derived error bound.  Nothing here looks at what the kernels return.

Bound of a bilinear resize in fp32, per element: the kernels filter along the rows, then along the columns, with weights that are the double
weights rounded once to fp32 (1 U each, U = 2^-24), one fused multiply-add per tap (1 U) and no negative weight, so the standard bound of a
two-pass dot product applies: |got - ref| <= (T_h + T_w + 4) U R(|x|), T the tap count of the axis and R(|x|) the same resize of |x| in
float64.  With a per-channel affine a R(x) + b (one fused multiply-add): the bound times |a_c|, plus 2^-23 |ref|.  The adjoint: the same
with R^T(|dy|) and the transposed tap counts (the largest number of outputs that read one input pixel)."""
import torch
import torch.nn.functional as F

U = 2.0 ** -24
# (B, C), input (H, W), output (H, W): tile edges, non-square, up and down, a window over the whole image, identity
SHAPES = [((2, 3), (41, 41), (18, 18)), ((2, 3), (18, 18), (41, 41)), ((3, 1), (37, 53), (16, 24)), ((2, 4), (64, 64), (32, 32)), ((1, 3), (23, 29), (1, 1)),
          ((1, 2), (5, 7), (40, 3)), ((1, 3), (33, 47), (33, 47))]
# further shapes at which the kernels take another path: several tiles in both directions with ragged edges (forward: 3 x 5 tiles of 32 x 32
# outputs, adjoint: 2 x 2 tiles of 64 x 64 input pixels), and 61-tap windows whose input window fits the LDS only for a 2 x 2 tile of outputs
EXTRA_SHAPES = [((1, 2), (100, 70), (67, 130)), ((1, 1), (600, 600), (20, 20))]
# the pairs of the table test: the shapes above and upstream's 512 <-> 224
TABLE_PAIRS = [((41, 41), (18, 18)), ((18, 18), (41, 41)), ((37, 53), (16, 24)), ((64, 64), (32, 32)), ((33, 47), (33, 47)), ((23, 29), (1, 1)),
               ((5, 7), (40, 3)), ((512, 512), (224, 224)), ((224, 224), (512, 512))]


def shape_id(v):
    return "-".join("x".join(map(str, p)) for p in v) if isinstance(v, tuple) and isinstance(v[0], tuple) else str(v)


def gen(seed):
    return torch.Generator().manual_seed(seed)


def interp64(x, size, antialias):
    return F.interpolate(x.double(), size, mode="bilinear", align_corners=False, antialias=antialias)


def adjoint64(dy, in_size, antialias):
    """R^T(dy) in float64: the autograd gradient of F.interpolate (linear in x, so the point of evaluation does not matter)."""
    x = torch.zeros(*dy.shape[:2], *in_size, dtype=torch.float64, requires_grad=True)
    g, = torch.autograd.grad(interp64(x, tuple(dy.shape[-2:]), antialias), x, dy.double())
    return g


def affine_vectors(C, seed):
    g = gen(seed)
    return (torch.randn(C, generator=g) * 1.5 + 0.25).float(), torch.randn(C, generator=g).float()


def dense_matrix(table, n_in, weights="weights_f64"):
    """The (n_out, n_in) float64 matrix of one axis table (a dict as fourm.hip.ops.resize_axis_table returns it)."""
    n_out = table["start"].numel()
    M = torch.zeros(n_out, n_in, dtype=torch.float64)
    for o in range(n_out):
        s, c = int(table["start"][o]), int(table["count"][o])
        M[o, s:s + c] = table[weights][o, :c].double()
    return M
