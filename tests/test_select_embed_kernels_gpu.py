"""csrc/select_embed.hip on a real MI355X, kernel by kernel: fm_select_embed, fm_embed_bwd and fm_dense_decoder_mask against the plain
reference of tests/select_embed_util.py (proved against the upstream fixtures and the oracle by tests/test_select_embed_cpu.py).

fm_select_embed only copies rows and adds two fp32 numbers, so every output is compared exactly: the integers element by element, the float
rows bit for bit with the reference evaluated in fp32 with the same single add.  The batches are the irregular ones the whole-model
fixtures never contain: scattered sequence masks, truncation, padding, max_len collapse, the chunk edges of both scans, the limits, every
grid split.  mask / dam / ids are views of wider buffers whose gaps hold 1 / an id outside the vocabulary / NaN; each output has a sentinel
row past the end.

fm_embed_bwd adds in an arbitrary order (registers, LDS atomics, global atomics) onto pre-filled buffers.  For a gradient element with n
contributing slots, S = sum |dx| over them and prefill p, any summation order of the n + 1 fp32 terms stays within the first-order bound
(n + 1) u (|p| + S); the factor 2 below covers the higher-order terms:
    |got - (p + ref)| <= 2 (n + 2) u (|p| + S),   u = 2^-24,
with n and S from the float64 autograd reference.  Elements with n = 0 must keep their prefill bit for bit."""
import ctypes as C

import pytest
import torch

from tests import select_embed_util as S
from tests.parity_log import record
from tests.select_embed_util import PATCH, SEQ, SEQ_EMB, TOK

pytestmark = pytest.mark.gpu

U = 2.0 ** -24


def refused(rc, text):
    from fourm.hip import _lib as L
    assert rc == -1, f"the launcher returned {rc} for a bad argument"
    msg = L.lib.fm_last_error().decode()
    assert text in msg, msg


def bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def same_bits(name, got, ref):
    bad = bits(got) != bits(ref.to(got.dtype))
    assert not bool(bad.any()), f"{name}: {int(bad.sum())} of {bad.numel()} elements differ, first at {bad.nonzero()[0].tolist()}"


def run_and_compare(side, want_x0=True):
    """Launch fm_select_embed on ``side`` and compare every output with the reference.  Returns (device call, reference)."""
    from fourm.hip import _lib as L
    ref = S.reference(side)
    call = S.DeviceCall(side, want_x0=want_x0)
    L.check(call.launch())
    got, intact = call.results()
    assert intact, "a row past B * Nt was written"
    ints = ["out_mask", "out_mod", "slot_mod"] + (["target_ids", "out_cs", "out_mod_pre", "out_mod_index"] if side.is_decoder else [])
    for k in ints:
        bad = got[k] != ref[k].to(got[k].dtype)
        assert not bool(bad.any()), f"{k}: {int(bad.sum())} differ, first at {bad.nonzero()[0].tolist()}: got {got[k][bad][0]}, want {ref[k][bad][0]}"
    live = ref["slot_mod"] != -1                      # slot_src / slot_pos have a meaning where the slot is live / uses a position row
    assert torch.equal(got["slot_src"][live], ref["slot_src"][live]), "slot_src"
    used = ref["slot_pos"] >= 0
    assert torch.equal(got["slot_pos"][used], ref["slot_pos"][used]), "slot_pos"
    for k in ["tokens", "emb"] + (["x0"] if want_x0 else []):
        same_bits(k, got[k], ref[k])
    for k in ("patch_rows", "seqemb_rows"):
        if k in got:                                  # bf16: one round-to-nearest-even of the fp32 source; pad columns and non-dense rows 0
            same_bits(k, got[k], ref[k])
    return call, ref


ENC4 = [(SEQ, 9, {}), (TOK, 6, {}), (SEQ_EMB, 7, {}), (PATCH, 4, dict(grid_w=2))]
DEC3 = [(SEQ, 9, dict(max_len=20)), (TOK, 6, {}), (SEQ, 5, dict(max_len=20, id_dtype=torch.int32))]


def _set_selectable(side, per_sample):
    """Sample b: exactly the concatenated positions per_sample[b] are selectable (unshifted modalities only)."""
    for b, sel in enumerate(per_sample):
        off = 0
        for m in side.mods:
            m.mask[b] = True
            for p in sel:
                if off <= p < off + m.L:
                    m.mask[b, p - off] = False
            off += m.L


def case_scattered_enc():
    return S.make_side(11, ENC4, B=3, D=8, n_keep=26)


def case_scattered_dec():
    s = S.make_side(12, DEC3, B=3, D=8, n_keep=20, is_decoder=True)
    m = s.mods[0]                                   # scattered targets: m[j] | m[j+1] differs from m[j]
    assert bool(((m.mask[:, :-1] | m.mask[:, 1:]) != m.mask[:, :-1]).any())
    return s


def case_truncate_inside():
    return S.make_side(13, ENC4, B=3, D=8, n_keep=5, p_mask=0.2)


def case_truncate_on_boundary():
    s = S.make_side(14, ENC4, B=2, D=8, n_keep=9, p_mask=0.3)
    s.mods[0].mask[:] = False                       # all 9 sequence positions selectable: the cut falls exactly between two modalities
    return s


def case_truncate_dec():
    return S.make_side(15, DEC3, B=3, D=8, n_keep=4, is_decoder=True, p_mask=0.1)


def case_padding_enc():
    s = S.make_side(16, ENC4, B=3, D=8, n_keep=24, p_mask=0.7)
    for m in s.mods:
        m.mask[1] = True                            # sample 1: nothing selectable at all
    return s


def case_padding_dec():
    s = S.make_side(17, DEC3, B=3, D=8, n_keep=19, is_decoder=True, p_mask=0.6)
    for m in s.mods:
        m.mask[2] = True
    return s


def case_max_len_collapse():
    return S.make_side(18, [(SEQ, 12, dict(max_len=3)), (TOK, 4, {})], B=2, D=8, n_keep=14, is_decoder=True, p_mask=0.1)


def case_scan(total):
    def build():
        # total_len = total over three modalities; sample 0's first selectable position lies in the last 256-position chunk
        a = total // 3
        s = S.make_side(19 + total, [(SEQ, a, {}), (TOK, a, {}), (SEQ_EMB, total - 2 * a, {})], B=2, D=4, n_keep=min(total, 40), p_mask=0.8)
        last = (total - 1) // 256 * 256
        _set_selectable(s, [sorted({last + (total - 1 - last) // 2, total - 1})])
        return s
    return build


def case_cs(n_keep):
    return lambda: S.make_side(30 + n_keep, [(SEQ, 50, dict(max_len=60)), (TOK, 100, {})], B=2, D=4, n_keep=n_keep, is_decoder=True, p_mask=0.3)


def case_limit_keep():
    return S.make_side(40, [(SEQ, 5000, {}), (TOK, 3192, {})], B=1, D=4, n_keep=1024, p_mask=0.9)


def case_limit_raw():
    return S.make_side(41, [(SEQ, 5000, {}), (TOK, 3192, {})], B=1, D=4, raw=1)


def case_batch(B):
    return lambda: S.make_side(50 + B, [(SEQ, 5, {}), (TOK, 4, {}), (SEQ_EMB, 3, dict(orig_dim=2))], B=B, D=4, n_keep=7)


def case_dim(D):
    return lambda: S.make_side(60 + D, ENC4, B=2, D=D, n_keep=8, n_reg=2 if D == 260 else 0)


def case_registers():
    return S.make_side(70, ENC4, B=3, D=8, n_keep=10, n_reg=2)


def case_rows_f32():
    return S.make_side(71, ENC4, B=2, D=8, n_keep=20, n_reg=2, rows_f32=True)


def case_id_dtypes(dec):
    specs = [(TOK, 5, dict(id_dtype=torch.int32)), (TOK, 5, dict(id_dtype=torch.int64)),
             (SEQ, 6, dict(id_dtype=torch.int32, max_len=9)), (SEQ, 6, dict(id_dtype=torch.int64, max_len=9))]
    return lambda: S.make_side(72 + dec, specs, B=2, D=8, n_keep=15, is_decoder=bool(dec))


def case_most_mods(dec):
    kinds = [SEQ, TOK] if dec else [SEQ, TOK, SEQ_EMB, PATCH]
    specs = [(kinds[i % len(kinds)], 1, dict(max_len=4, grid_w=1, vocab=5 + i)) for i in range(24)]
    return lambda: S.make_side(74 + dec, specs, B=3, D=4, n_keep=20, is_decoder=bool(dec), p_mask=0.3)


def case_shuffled_dec():
    specs = [(TOK, 6, dict(head_index=2, mod_id=900)), (SEQ, 7, dict(head_index=0, max_len=5, mod_id=3)), (TOK, 4, dict(head_index=3, mod_id=31000)),
             (SEQ, 5, dict(head_index=1, max_len=9, mod_id=77))]
    return S.make_side(76, specs, B=3, D=8, n_keep=16, is_decoder=True)


def case_raw1(dec):
    return lambda: S.make_side(77 + dec, DEC3 if dec else ENC4, B=3, D=8, raw=1, is_decoder=bool(dec))


def case_raw2(kind, dec):
    opt = dict(max_len=4) if kind == SEQ else dict(grid_w=3) if kind == PATCH else {}
    return lambda: S.make_side(80 + 2 * kind + dec, [(kind, 9, opt)], B=2, D=8, raw=2, is_decoder=bool(dec))


CASES = {
    "scattered_enc": case_scattered_enc, "scattered_dec": case_scattered_dec,
    "truncate_inside": case_truncate_inside, "truncate_on_boundary": case_truncate_on_boundary, "truncate_dec": case_truncate_dec,
    "padding_enc": case_padding_enc, "padding_dec": case_padding_dec, "max_len_collapse": case_max_len_collapse,
    **{f"scan_{t}": case_scan(t) for t in (255, 256, 257, 700)},
    **{f"cs_{n}": case_cs(n) for n in (63, 64, 65, 130)},
    "limit_keep_1024_of_8192": case_limit_keep, "limit_raw_8192": case_limit_raw,
    **{f"batch_{b}": case_batch(b) for b in (1, 3, 1024, 2048)},
    **{f"dim_{d}": case_dim(d) for d in (4, 128, 260, 2048)},
    "registers": case_registers, "rows_f32": case_rows_f32,
    "id_dtypes_enc": case_id_dtypes(0), "id_dtypes_dec": case_id_dtypes(1),
    "most_mods_enc": case_most_mods(0), "most_mods_dec": case_most_mods(1), "shuffled_dec": case_shuffled_dec,
    "raw1_enc": case_raw1(0), "raw1_dec": case_raw1(1),
    "raw2_tok_enc": case_raw2(TOK, 0), "raw2_tok_dec": case_raw2(TOK, 1), "raw2_patch": case_raw2(PATCH, 0),
    "raw2_seq_enc": case_raw2(SEQ, 0), "raw2_seq_dec": case_raw2(SEQ, 1), "raw2_seq_emb": case_raw2(SEQ_EMB, 0),
}


@pytest.mark.parametrize("name", list(CASES))
def test_select_embed(name):
    side = CASES[name]()
    _, ref = run_and_compare(side)
    # each case really contains what it is named after
    live = ref["slot_mod"] >= 0
    if name.startswith("truncate"):
        assert not bool(ref["out_mask"].any())
    if name.startswith("padding"):
        b = 2 if side.is_decoder else 1
        assert bool(ref["out_mask"][b].all()) and bool((ref["slot_mod"][b] == -1).all()) and bool(ref["out_mask"][0].any()) and bool(live[0].any())
        if side.is_decoder:
            assert int(ref["out_cs"][b, -1]) > 0 and bool((ref["out_mod_index"][b] == -1).all())      # out_cs still accumulates the gathered dam
    if name == "max_len_collapse":
        pos0 = ref["slot_pos"][ref["slot_mod"] == 0]
        assert int(pos0.max()) == 2 and int((pos0 == 0).sum()) > side.B
    if name.startswith("scan_"):
        assert int(ref["ids_keep"][0, 0]) >= (side.total_len - 1) // 256 * 256 and int(live[0].sum()) in (1, 2)
    if name == "raw2_tok_dec":
        assert torch.equal(ref["tokens"], side.mods[0].table[side.mods[0].ids])                        # its ids, not the mask token


def test_select_embed_without_x0():
    run_and_compare(case_scattered_enc(), want_x0=False)


def _small_call(**kw):
    return S.DeviceCall(S.make_side(90, kw.pop("specs", ENC4), B=2, D=8, n_keep=kw.pop("n_keep", 10), **kw))


def test_select_embed_refusals():
    """Every one of these is rejected by the host launcher (-1, fm_last_error names the reason) before any launch."""
    for n in (0, 25):
        c = _small_call()
        c.desc.n_mods = n
        refused(c.launch(), f"n_mods={n}")
    c = _small_call()
    c.desc.dim = 6
    refused(c.launch(), "dim must be a multiple of 4")
    c = _small_call()
    c.desc.total_len += 1
    refused(c.launch(), "modalities sum to 26")
    c = _small_call()
    c.desc.n_keep = 27
    refused(c.launch(), "n_keep=27 exceeds the 26")
    c = _small_call()
    c.desc.n_keep = 1025
    refused(c.launch(), "n_keep=1025 out of range")
    c = _small_call()
    c.desc.mods[0].L += 8193 - 26
    c.desc.total_len = 8193
    refused(c.launch(), "8193 concatenated positions exceed 8192")
    c = _small_call(raw=1)
    c.desc.n_reg, c.desc.reg_tokens = 2, c.desc.tokens
    refused(c.launch(), "raw views cover every position")
    c = _small_call(raw=1)
    c.desc.n_keep = 25
    refused(c.launch(), "raw views cover every position")
    c = _small_call(specs=DEC3, is_decoder=True)
    c.desc.out_cs = None
    refused(c.launch(), "decoder outputs missing")
    c = _small_call()
    c.desc.patch_rows = None
    refused(c.launch(), "pixel modality needs patch_rows")
    c = _small_call()
    c.desc.patch_ld = 18
    refused(c.launch(), "side buffers need ld")
    # nothing ran: the outputs still hold their sentinels
    got, intact = c.results()
    assert intact and bool((got["tokens"] == S.SENT).all()) and bool((got["slot_mod"] == S.ISENT).all())


# ------------------------------------------------------------------------------------------------
# fm_embed_bwd
# ------------------------------------------------------------------------------------------------
def check_grads(label, bwd, grads):
    """|got - (p + ref)| <= 2 (n + 2) u (|p| + S) per element (module docstring); n = 0: bit-equal to the prefill.  Returns worst err/tol."""
    worst = 0.0
    for name, (got, pre) in bwd.results().items():
        g, n, s_abs = (t.reshape(-1, got.shape[1]) for t in grads[name])
        pad = lambda t: torch.cat([t, torch.zeros(got.shape[0] - t.shape[0], got.shape[1], dtype=t.dtype)], 0)     # the guard row: n = 0
        g, n, s_abs = pad(g), pad(n), pad(s_abs)
        tol = 2 * (n + 2) * U * (pre.double().abs() + s_abs)
        err = (got.double() - (pre.double() + g)).abs()
        bad = ~(err <= tol)
        ratio = float((err / tol).max())
        assert not bool(bad.any()), f"{label} {name}: {int(bad.sum())} of {bad.numel()} outside the bound, worst err/tol {ratio:.3g}, first at {bad.nonzero()[0].tolist()}"
        idle = n == 0
        assert torch.equal(bits(got)[idle], bits(pre)[idle]), f"{label} {name}: an element without contributing slots changed"
        worst = max(worst, ratio)
    return worst


def run_bwd(label, side, null=(), masked_raw=False, seed=0):
    from fourm.hip import _lib as L
    dx = torch.randn(side.B, side.Nt, side.D, generator=S.gen(500 + seed))
    grads, ref = S.reference_backward(side, dx, zero_masked=masked_raw)
    tables = S.masked_slot_tables(ref) if masked_raw else (ref["slot_mod"], ref["slot_src"], ref["slot_pos"].clamp(min=0))
    names = [n for n in grads if n not in null and (n[0] if isinstance(n, tuple) else n) not in null]
    bwd = S.DeviceBwd(side, *tables, dx, names, seed=seed)
    L.check(bwd.launch())
    return check_grads(label, bwd, grads), grads, ref


LEARN = dict(learned_pos=True)


def bwd_enc(seed, Nt, B=3, D=8, n_reg=0, p_mask=0.3):
    # modality runs of 9 / 1 / 7 / 4 / rest slots cross the slot ranges of the 16 waves; the second modality has a single slot
    rest = max(Nt, 24)
    specs = [(SEQ, 9, dict(learned_pos=True, padding_idx=1, vocab=5)), (TOK, 1, LEARN), (SEQ_EMB, 7, LEARN), (PATCH, 4, dict(grid_w=2, learned_pos=True)),
             (TOK, rest, dict(vocab=7))]
    s = S.make_side(seed, specs, B=B, D=D, n_keep=Nt - n_reg, n_reg=n_reg, p_mask=p_mask)
    s.mods[1].mask[:] = False
    return s


BWD_CASES = {
    # 130 slots over 16 ranges of 9: a ragged split; p_mask = 0.05 keeps the last slots live, so a short last range loses gradient
    **{f"Nt_{n}": (lambda n=n: bwd_enc(100 + n, n, p_mask=0.05 if n == 130 else 0.3)) for n in (5, 16, 17, 130)},
    "registers": lambda: bwd_enc(110, 17, n_reg=2),
    "duplicates": lambda: S.make_side(111, [(SEQ, 130, dict(vocab=3, padding_idx=1, learned_pos=True))], B=2, D=8, n_keep=130, p_mask=0.0),
    "decoder_mask_token_and_collapse": lambda: S.make_side(112, [(TOK, 6, LEARN), (SEQ, 12, dict(max_len=3, learned_pos=True, padding_idx=0)), (TOK, 5, {})],
                                                           B=3, D=8, n_keep=20, is_decoder=True, p_mask=0.15),
    "dim_4": lambda: bwd_enc(113, 17, D=4), "dim_260": lambda: bwd_enc(114, 17, D=260, n_reg=2), "dim_2048": lambda: bwd_enc(115, 9, B=2, D=2048),
    **{f"batch_{b}": (lambda b=b: bwd_enc(120 + b, 16, B=b, D=4)) for b in (1, 3, 1024, 2048)},
    "most_mods": lambda: S.make_side(116, [([SEQ, TOK, SEQ_EMB, PATCH][i % 4], 2, dict(grid_w=1, learned_pos=i % 3 == 0, vocab=3)) for i in range(24)],
                                     B=3, D=4, n_keep=40, p_mask=0.3),
}


@pytest.mark.parametrize("name", list(BWD_CASES))
def test_embed_bwd(name):
    side = BWD_CASES[name]()
    r, grads, ref = run_bwd(name, side, seed=len(name))
    if name == "duplicates":
        g, n, _ = grads[("table", 0)]
        assert bool((n[1] == 0).all()) and float(n[0, 0]) + float(n[2, 0]) > 150          # the padding_idx row is idle, two rows take the rest
    if name == "decoder_mask_token_and_collapse":
        assert ("table", 0) not in grads and float(grads["mask_token"][1].max()) > 5       # grid targets feed the mask token
        assert float(grads[("pos", 1)][1][0, 0]) > float(grads[("pos", 1)][1][1, 0])       # collapsed slots land on position row 0
    if name == "Nt_130":
        assert bool((ref["slot_mod"][:, -2:] >= 0).all())                                  # live slots up to the end of the last range
    if name == "Nt_17":
        assert int((ref["slot_mod"] == 1).sum()) == side.B                                 # a modality with a single slot per sample
    record(f"select_embed_kernels.embed_bwd[{name}]", worst_err_over_tol=r)


@pytest.mark.parametrize("dec", [0, 1])
def test_embed_bwd_interleaved_and_dead_sample(dec):
    """The raw = 1 slot tables with the masked positions marked -1: slots of one modality separated by masked ones, never a contiguous
    run per wave; sample 1 has every slot -1."""
    specs = [(SEQ, 20, dict(learned_pos=True, padding_idx=2, vocab=6, max_len=30)), (TOK, 15, LEARN), (SEQ, 11, dict(max_len=30, vocab=4))]
    side = S.make_side(130 + dec, specs, B=3, D=8, raw=1, is_decoder=bool(dec))
    for m in side.mods:
        m.mask[1] = True
    r, grads, ref = run_bwd(f"interleaved[{dec}]", side, masked_raw=True, seed=dec)
    sm = S.masked_slot_tables(ref)[0]
    assert bool((sm[1] == -1).all()) and bool(((sm[0, 1:] == -1) & (sm[0, :-1] >= 0)).any())
    record(f"select_embed_kernels.embed_bwd_interleaved[{dec}]", worst_err_over_tol=r)


def test_embed_bwd_null_pointers_second_call():
    """The engine's second call (the context gradient reaches pos_emb / mod_emb only): NULL d_table / d_proj_bias / d_reg_tokens are skipped,
    the others receive exactly what they receive in the full call; then every pointer NULL but one modality's d_mod_emb."""
    side = bwd_enc(140, 17, n_reg=2)
    r1, grads, _ = run_bwd("null second call", side, null=("table", "proj_bias", "reg_tokens"))
    r2, _, _ = run_bwd("null all but one", side, null=("table", "proj_bias", "reg_tokens", "pos", ("mod_emb", 0), ("mod_emb", 1), ("mod_emb", 3), ("mod_emb", 4)))
    dside = BWD_CASES["decoder_mask_token_and_collapse"]()
    r3, _, _ = run_bwd("null mask token", dside, null=("mask_token", "pos"))
    record("select_embed_kernels.embed_bwd_null", worst_err_over_tol=max(r1, r2, r3))


def test_embed_bwd_chained_after_the_forward_kernel():
    """fm_select_embed's own slot_mod / slot_src / slot_pos (device buffers, masked slots included) drive fm_embed_bwd."""
    from fourm.hip import _lib as L
    side = bwd_enc(150, 30, n_reg=2, p_mask=0.5)
    call, ref = run_and_compare(side)
    assert bool((ref["slot_mod"] == -1).any())
    dx = torch.randn(side.B, side.Nt, side.D, generator=S.gen(151))
    grads, _ = S.reference_backward(side, dx)
    R = side.B * side.Nt
    bwd = S.DeviceBwd(side, *(call.out[k][:R].reshape(side.B, side.Nt) for k in ("slot_mod", "slot_src", "slot_pos")), dx, list(grads))
    L.check(bwd.launch())
    record("select_embed_kernels.embed_bwd_chained", worst_err_over_tol=check_grads("chained", bwd, grads))


def test_embed_bwd_refusals():
    side = bwd_enc(160, 17)
    dx = torch.zeros(side.B, side.Nt, side.D)
    ref = S.reference(side)
    tables = (ref["slot_mod"], ref["slot_src"], ref["slot_pos"].clamp(min=0))
    names = [("mod_emb", 0)]
    refused(S.DeviceBwd(side, *tables, dx, names, dim=2052).launch(), "bad shape (dim <= 2048)")
    refused(S.DeviceBwd(side, *tables, dx, names, lddx=10).launch(), "bad shape")
    b = S.DeviceBwd(side, *tables, dx, names, dim=2048)
    b.desc.n_mods = 24                                  # 25 rows of 2048 floats = 204800 bytes of LDS > 150 KB
    refused(b.launch(), "204800 bytes of LDS needed")
    got, pre = b.results()[("mod_emb", 0)]
    assert torch.equal(got, pre)


# ------------------------------------------------------------------------------------------------
# fm_dense_decoder_mask
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,M", [(1, 1), (3, 1), (1, 64), (3, 64), (1, 257), (3, 257)])
def test_dense_decoder_mask(B, M):
    """Against arange(M) >= cs (or triu(1)) | mod_q != mod_k for every combination of causal / use_cs / use_sep; the input is the already
    accumulated cs; mod holds -1 entries; the byte after the end survives."""
    from fourm.hip import _lib as L
    g = S.gen(B * 1000 + M)
    cs = torch.randint(0, 3, (B, M), generator=g, dtype=torch.int32).cumsum(1).int()
    mod = torch.randint(-1, 3, (B, M), generator=g).to(torch.int16)
    assert M < 8 or bool((mod == -1).any())
    cs_d, mod_d = cs.cuda(), mod.cuda()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for causal in (0, 1):
        for use_cs in (0, 1):
            for use_sep in (0, 1):
                out = torch.full((B * M * M + 1,), S.ISENT, dtype=torch.uint8, device="cuda")
                L.check(L.dense_decoder_mask(cs_d.data_ptr() if use_cs or causal else None, mod_d.data_ptr() if use_sep else None, out.data_ptr(), B, M,
                                             causal, use_cs, use_sep, stream))
                ref = S.dense_mask_reference(cs, mod, causal, use_cs, use_sep)
                o = out.cpu()
                assert torch.equal(o[:-1].reshape(B, M, M), ref.to(torch.uint8)), (causal, use_cs, use_sep)
                assert int(o[-1]) == S.ISENT
    out = torch.zeros(B * M * M, dtype=torch.uint8, device="cuda")
    refused(L.dense_decoder_mask(cs_d.data_ptr(), None, out.data_ptr(), B, M, 0, 1, 1, stream), "fm_dense_decoder_mask: null pointer")
    refused(L.dense_decoder_mask(None, mod_d.data_ptr(), out.data_ptr(), B, M, 0, 1, 1, stream), "fm_dense_decoder_mask: null pointer")
