"""zsg_conv_igemm_bf16_m / zsg_conv_igemm_bf16_m_supported (csrc/igemm_bf16.hip) at the kernel level, on DATA-GRADIENT descriptors
(ops.dgrad_desc) with the weight operand made by the plan's own chain: zsg_transpose_w, then zsg_pack_w_bf16_batched with N = n,
T = k*k, wC = C = cred.

Bounds: those derived in tests/test_gpu_conv_bf16.py, none taken from what the code gives:
  * integer data in [-8, 8]: |sum| <= 9 * 256 * 64 (+ 8 for add_src) < 2^24, so the fp32 result is exact in any summation order: zero
    tolerance against int64 arithmetic;
  * standard-normal data: fp64 data gradient of the HOST-rounded bf16 operands (+ fp32 add_src); per element
    |out - ref| <= (K + 4) * 2^-23 * (S + |add_src|), S the same sum of absolute values, K = taps * cred.
Mask values are drawn from {-1, -0.0, 0, 0.5, 3}: the output is == 0 where the mask is <= 0 and the unmasked result elsewhere.  With
mask_src = NULL the result is bit-equal to zsg_conv_igemm_bf16 on the same operands.  Every case runs on the tile hints 0, 64x64,
128x64, 128x128."""
import ctypes as C
import functools
import struct

import pytest
import torch

pytestmark = pytest.mark.gpu

HINTS = (0, (64, 64), (128, 64), (128, 128))
MASK_VALUES = (-1.0, -0.0, 0.0, 0.5, 3.0)

# name -> (dx levels [(H, W)], B, cout (real dy channels), cred (dy.ld), n (dx channels), cpad (rows of the transposed image), k, stride, pad, extras)
CASES = {
    "head": ([(10, 10), (5, 5), (3, 3)], 2, 256, 256, 256, 256, 3, 1, 1, dict(mask=True)),
    "last_48": ([(10, 10), (5, 5), (3, 3)], 2, 45, 48, 256, 256, 3, 1, 1, dict(mask=True)),
    "add_alias": ([(9, 11)], 2, 256, 256, 256, 256, 3, 1, 1, dict(mask=True, add=True)),
    "rows_516": ([(10, 10)], 1, 256, 256, 256, 516, 3, 1, 1, {}),
    "stride2": ([(5, 5)], 2, 256, 256, 256, 256, 3, 2, 1, dict(mask=True)),
    "tail_1x1": ([(8, 8)], 3, 256, 256, 512, 512, 1, 1, 0, {}),
}


@pytest.fixture(scope="module")
def Z():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from zsgnet_pytorch_amd import _lib, ops
    return _lib, ops


def conv_out(n, k, s, p):
    return (n + 2 * p - (k - 1) - 1) // s + 1


def dgrad_ref(dy, w, H, W, k, s, p):
    """dy [B, Ho, Wo, co], w [co, k, k, c] (the FORWARD weight) of one dtype (int64 / float64) -> dx [B, H, W, c]: the transpose of the
    forward gather, tap by tap in that dtype's own arithmetic"""
    B, Ho, Wo, co = dy.shape
    buf = torch.zeros(B, H + 2 * p, W + 2 * p, w.shape[3], dtype=dy.dtype)
    for ty in range(k):
        for tx in range(k):
            buf[:, ty: ty + (Ho - 1) * s + 1: s, tx: tx + (Wo - 1) * s + 1: s] += torch.matmul(dy.reshape(-1, co), w[:, ty, tx]).view(B, Ho, Wo, -1)
    return buf[:, p:p + H, p:p + W].contiguous()


@functools.lru_cache(maxsize=None)
def make_case(name, kind):
    """operands (fp32, CPU) and the UNMASKED reference of one case, computed once and shared by the tests (never modified)"""
    levels, B, cout, cred, n, cpad, k, s, p, ex = CASES[name]
    g = torch.Generator().manual_seed(100 + sorted(CASES).index(name) * 2 + (kind == "int"))

    def draw(*shape):
        if kind == "int":
            return torch.randint(-8, 9, shape, generator=g).float()
        return torch.randn(*shape, generator=g)
    w = draw(cout, k, k, cpad)
    dys = []
    for (H, W) in levels:
        dy = draw(B, conv_out(H, k, s, p), conv_out(W, k, s, p), cred)
        dy[..., cout:] = 0                                   # (the padding channels of the 45 -> 48 output gradient)
        dys.append(dy)
    adds = [draw(B, H, W, n) for (H, W) in levels] if ex.get("add") else None
    masks = None
    if ex.get("mask"):
        mv = torch.tensor(MASK_VALUES)
        masks = [mv[torch.randint(0, len(MASK_VALUES), (B, H, W, n), generator=g)] for (H, W) in levels]
        assert all(bool(torch.signbit(m[m == 0]).any()) and bool((~torch.signbit(m[m == 0])).any()) for m in masks), "both zeros occur"
    refs, bounds = [], []
    for i, ((H, W), dy) in enumerate(zip(levels, dys)):
        wu, du = w[..., :n], dy[..., :cout]
        if kind == "int":
            r = dgrad_ref(du.to(torch.int64), wu.to(torch.int64), H, W, k, s, p)
            if adds is not None:
                r = r + adds[i].to(torch.int64)
            assert int(r.abs().max()) < 2 ** 24
            refs.append(r.float())
            bounds.append(None)
        else:
            db, wb = du.to(torch.bfloat16).double(), wu.to(torch.bfloat16).double()
            r = dgrad_ref(db, wb, H, W, k, s, p)
            S = dgrad_ref(db.abs(), wb.abs(), H, W, k, s, p)
            if adds is not None:
                r, S = r + adds[i].double(), S + adds[i].double().abs()
            refs.append(r)
            bounds.append((k * k * cred + 4) * 2.0 ** -23 * S)
    return dict(w=w, dys=dys, adds=adds, masks=masks, refs=refs, bounds=bounds)


def weight_operand(L, cs, name):
    """the plan's chain: zsg_transpose_w (OHWI -> [cpad][k*k][cred]), then ONE pack job over the first n rows.  The rows behind n (conv0's
    language / grid columns) are poisoned with NaN before packing: the packer and the kernel may only read the first n."""
    levels, B, cout, cred, n, cpad, k, s, p, ex = CASES[name]
    wd = cs["w"].cuda()
    wt = torch.full((cpad * k * k * cred,), float("nan"), device="cuda")
    L.check(L.lib.zsg_transpose_w(wd.data_ptr(), wt.data_ptr(), cout, k * k, cpad, cred, L.stream_ptr()), "transpose_w")
    torch.cuda.synchronize()
    got = wt.view(cpad, k * k, cred).cpu()
    want = torch.zeros(cpad, k * k, cred)
    want[..., :cout] = cs["w"].permute(3, 1, 2, 0).reshape(cpad, k * k, cout)
    assert torch.equal(got, want), "zsg_transpose_w"
    if cpad > n:
        wt.view(cpad, k * k, cred)[n:] = float("nan")
    c8 = (cred + 7) // 8 * 8
    wp = torch.full((n, k * k, c8), 0x5555, dtype=torch.int16, device="cuda")
    job = struct.pack("<qqiiiiiiii", wt.data_ptr(), wp.data_ptr(), n, k * k, cred, 0, cred, c8, 0, 0)
    dev = torch.frombuffer(bytearray(job), dtype=torch.uint8).cuda()
    L.check(L.lib.zsg_pack_w_bf16_batched(dev.data_ptr(), 1, (n * k * k * c8 // 8 + 255) // 256, L.stream_ptr()), "pack")
    torch.cuda.synchronize()
    assert torch.equal(wp.cpu().view(torch.bfloat16)[..., :cred].view(torch.int16), want[:n].to(torch.bfloat16).view(torch.int16)), "packed transposed image"
    return wp


def launch(Z, name, kind, hint, use_mask=True, entry="m"):
    """run one case; returns (per-level outputs on the CPU, rc).  entry "m": zsg_conv_igemm_bf16_m (mask_src NULL when the case has no
    mask or use_mask is False); "plain": zsg_conv_igemm_bf16 on the same operands"""
    L, ops = Z
    levels, B, cout, cred, n, cpad, k, s, p, ex = CASES[name]
    cs = make_case(name, kind)
    wp = weight_operand(L, cs, name)
    dy_flat = torch.cat([x.reshape(-1) for x in cs["dys"]]).cuda()
    lv_y, lv_x, yo, xo = [], [], 0, 0
    for (H, W) in levels:
        Ho, Wo = conv_out(H, k, s, p), conv_out(W, k, s, p)
        lv_y.append(ops.Level(yo, Ho, Wo, Ho * Wo * cred))
        lv_x.append(ops.Level(xo, H, W, H * W * n))
        yo += B * Ho * Wo * cred
        xo += B * H * W * n
    out = torch.full((xo,), float("nan"), device="cuda")
    add = None
    if cs["adds"] is not None:
        out.copy_(torch.cat([a.reshape(-1) for a in cs["adds"]]).cuda())
        add = out                                            # add_src aliases out: the accumulating data gradient
    mask = torch.cat([m.reshape(-1) for m in cs["masks"]]).cuda() if (cs["masks"] is not None and use_mask) else None
    desc = ops.dgrad_desc(ops.TView(dy_flat, B, cred, cred, lv_y), ops.TView(out, B, n, n, lv_x), cred, n, k, s, p, 1,
                          tile_hint=0 if hint == 0 else ops.tile_hint(hint[0], hint[1], 1))
    assert not desc.zero_fill
    if name == "stride2":
        assert desc.nseg == 4, "four parity segments"
    if entry == "m":
        ok = int(L.lib.zsg_conv_igemm_bf16_m_supported(C.byref(desc)))
        rc = L.lib.zsg_conv_igemm_bf16_m(C.byref(desc), dy_flat.data_ptr(), wp.data_ptr(), out.data_ptr(), None, add.data_ptr() if add is not None else None,
                                         mask.data_ptr() if mask is not None else None, L.stream_ptr())
        assert ok == (1 if rc == 0 else 0), f"_supported says {ok}, the entry returned {rc}"
    else:
        rc = L.lib.zsg_conv_igemm_bf16(C.byref(desc), dy_flat.data_ptr(), wp.data_ptr(), out.data_ptr(), None, add.data_ptr() if add is not None else None,
                                       L.stream_ptr())
    torch.cuda.synchronize()
    res, o = [], 0
    oc = out.cpu()
    for (H, W) in levels:
        res.append(oc[o:o + B * H * W * n].view(B, H, W, n))
        o += B * H * W * n
    return res, rc


def split_by_mask(cs, lvl, got):
    """(elements the mask passes, elements it blocks) of one level's output; without a mask everything passes"""
    if cs["masks"] is None:
        return torch.ones_like(got, dtype=torch.bool), torch.zeros_like(got, dtype=torch.bool)
    m = cs["masks"][lvl]
    return m > 0, ~(m > 0)


def test_rows_and_tiles_of_the_cases():
    """what each case is there for — a self-check of the table above (it needs neither the GPU nor the feature and is no part of the
    feature's coverage)"""
    rows = {name: sum(c[1] * h * w for h, w in c[0]) for name, c in CASES.items()}
    assert rows["tail_1x1"] == 192 and rows["tail_1x1"] % 128 == 64 and CASES["tail_1x1"][4] == 512      # a tile tail, four 128-wide N tiles
    assert rows["head"] == 268 and rows["head"] % 64 != 0 and len(CASES["head"][0]) == 3                 # several blocks, level tails
    assert CASES["last_48"][2:4] == (45, 48) and CASES["rows_516"][5] == 516


@pytest.mark.parametrize("name", sorted(CASES))
def test_integer_data_is_exact(Z, name):
    cs = make_case(name, "int")
    for hint in HINTS:
        res, rc = launch(Z, name, "int", hint)
        assert rc == 0, Z[0].lib.zsg_last_error().decode()
        for lvl, (got, ref) in enumerate(zip(res, cs["refs"])):
            on, off = split_by_mask(cs, lvl, got)
            assert bool((got[off] == 0).all()), f"{name} hint {hint} level {lvl}: a masked element is not zero"
            assert torch.equal(got[on].view(torch.int32), ref[on].view(torch.int32)), \
                f"{name} hint {hint} level {lvl}: {int((got[on] != ref[on]).sum())} of {int(on.sum())} elements differ"


@pytest.mark.parametrize("name", sorted(CASES))
def test_random_data_within_the_fp32_accumulation_bound(Z, name):
    cs = make_case(name, "rand")
    worst = 0.0
    for hint in HINTS:
        res, rc = launch(Z, name, "rand", hint)
        assert rc == 0, Z[0].lib.zsg_last_error().decode()
        for lvl, (got, ref, bound) in enumerate(zip(res, cs["refs"], cs["bounds"])):
            assert not torch.isnan(got).any(), f"{name} hint {hint}: unwritten output elements"
            on, off = split_by_mask(cs, lvl, got)
            assert bool((got[off] == 0).all()), f"{name} hint {hint} level {lvl}: a masked element is not zero"
            err = (got.double() - ref).abs()[on]
            frac = float((err / bound[on].clamp(min=1e-300)).max())
            worst = max(worst, frac)
            assert bool((err <= bound[on]).all()), f"{name} hint {hint} level {lvl}: max error / bound = {frac:.3f}"
    print(f"bf16_m dgrad {name}: largest |out - ref| / bound over all tile hints = {worst:.4f}")


@pytest.mark.parametrize("name", sorted(CASES))
def test_null_mask_is_bit_equal_to_the_entry_without_a_mask(Z, name):
    for hint in HINTS:
        a, rc = launch(Z, name, "rand", hint, use_mask=False)
        b, rc2 = launch(Z, name, "rand", hint, entry="plain")
        assert rc == 0 and rc2 == 0
        for u, v in zip(a, b):
            assert not torch.isnan(u).any()
            assert torch.equal(u.view(torch.int32), v.view(torch.int32)), f"{name} hint {hint}"


def test_masked_result_is_the_unmasked_result_where_the_mask_passes(Z):
    """untouched elsewhere: bit for bit the NULL-mask launch's value where mask > 0"""
    for name in ("head", "stride2", "add_alias"):
        cs = make_case(name, "rand")
        for hint in HINTS:
            a, _ = launch(Z, name, "rand", hint)
            b, _ = launch(Z, name, "rand", hint, use_mask=False)
            for lvl, (u, v) in enumerate(zip(a, b)):
                on, off = split_by_mask(cs, lvl, u)
                assert int(off.sum()) > 0 and torch.equal(u[on].view(torch.int32), v[on].view(torch.int32)), f"{name} hint {hint}"
                assert bool((u[off] == 0).all())


def test_refusals_launch_nothing(Z):
    L, ops = Z
    dy = torch.zeros(2 * 8 * 8 * 64, device="cuda")
    o = torch.full((2 * 8 * 8 * 64,), 3.0, device="cuda")
    m = torch.ones(2 * 8 * 8 * 64, device="cuda")
    wp = torch.zeros(64 * 9 * 64, dtype=torch.int16, device="cuda")
    lv = [ops.Level(0, 8, 8, 8 * 8 * 64)]

    def desc(**kw):
        d = ops.dgrad_desc(ops.TView(dy, 2, 64, 64, lv), ops.TView(o, 2, 64, 64, lv), 64, 64, 3, 1, 1, 1)
        for k_, v in kw.items():
            setattr(d, k_, v)
        return d
    bad = {
        "merge_x": desc(merge_x=1),
        "split-K": desc(tile_hint=ops.tile_hint(64, 64, 2)),
        "stream-K": desc(tile_hint=ops.tile_hint(64, 64, 1) | (1 << 28)),
        "8-wave bit": desc(tile_hint=ops.tile_hint(64, 64, 1, 1)),
        "unknown tile": desc(tile_hint=ops.tile_hint(32, 64, 1)),
        "C % 4": desc(C=62),
        "epi_flags": desc(epi_flags=1),
    }
    for what, d in bad.items():
        assert L.lib.zsg_conv_igemm_bf16_m_supported(C.byref(d)) == 0, what
        for mk in (m.data_ptr(), None):
            rc = L.lib.zsg_conv_igemm_bf16_m(C.byref(d), dy.data_ptr(), wp.data_ptr(), o.data_ptr(), None, None, mk, L.stream_ptr())
            msg = L.lib.zsg_last_error().decode()
            assert rc == -1 and "conv_igemm_bf16_m" in msg and len(msg) > 20, (what, rc, msg)
    good = desc()
    assert L.lib.zsg_conv_igemm_bf16_m(C.byref(good), None, wp.data_ptr(), o.data_ptr(), None, None, m.data_ptr(), L.stream_ptr()) == -1
    assert L.lib.zsg_conv_igemm_bf16_m(C.byref(good), dy.data_ptr(), wp.data_ptr(), o.data_ptr(), None, None, m.data_ptr() + 2, L.stream_ptr()) == -1
    torch.cuda.synchronize()
    assert float(o.min()) == 3.0 and float(o.max()) == 3.0, "a refused call must launch nothing"
    assert L.lib.zsg_conv_igemm_bf16_m_supported(C.byref(good)) == 1
    assert L.lib.zsg_conv_igemm_bf16_m(C.byref(good), dy.data_ptr(), wp.data_ptr(), o.data_ptr(), None, None, m.data_ptr(), L.stream_ptr()) == 0
    torch.cuda.synchronize()
    assert float(o.abs().max()) == 0.0


def test_unaligned_mask_takes_the_scalar_epilogue(Z):
    """a mask pointer that is only 4-byte aligned: the 4-byte epilogue gives the 16-byte epilogue's bits"""
    L, ops = Z
    g = torch.Generator().manual_seed(77)
    B, H, W, Cc = 2, 7, 9, 64
    dy = torch.randn(B * H * W * Cc, generator=g).cuda()
    w = torch.randn(Cc, 9, Cc, generator=g).to(torch.bfloat16).view(torch.int16).cuda()
    mv = torch.tensor(MASK_VALUES)[torch.randint(0, 5, (B * H * W * Cc + 1,), generator=g)].cuda()
    lv = [ops.Level(0, H, W, H * W * Cc)]
    outs = []
    for off in (0, 1):
        m = torch.empty(B * H * W * Cc + 4, device="cuda")
        m[off:off + B * H * W * Cc] = mv[:B * H * W * Cc]
        o = torch.full((B * H * W * Cc,), float("nan"), device="cuda")
        d = ops.dgrad_desc(ops.TView(dy, B, Cc, Cc, lv), ops.TView(o, B, Cc, Cc, lv), Cc, Cc, 3, 1, 1, 1, tile_hint=ops.tile_hint(64, 64, 1))
        L.check(L.lib.zsg_conv_igemm_bf16_m(C.byref(d), dy.data_ptr(), w.data_ptr(), o.data_ptr(), None, None, m.data_ptr() + 4 * off, L.stream_ptr()), "bf16_m")
        torch.cuda.synchronize()
        outs.append(o.cpu())
    assert not torch.isnan(outs[0]).any() and torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32))
    assert bool((outs[0][~(mv[:-1].cpu() > 0)] == 0).all())


def test_two_runs_write_identical_bits(Z):
    for hint in HINTS:
        a, rc = launch(Z, "head", "rand", hint)
        b, _ = launch(Z, "head", "rand", hint)
        assert rc == 0
        for u, v in zip(a, b):
            assert torch.equal(u.view(torch.int32), v.view(torch.int32))
