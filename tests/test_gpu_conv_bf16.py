"""zsg_pack_w_bf16_batched / zsg_conv_igemm_bf16 / zsg_conv_igemm_bf16_supported (csrc/igemm_bf16.hip) at the kernel level.

Bounds, none of them taken from what the code gives:
  * packer and activation rounding: bit-equality with torch.Tensor.to(torch.bfloat16) (round-to-nearest-even);
  * integer data in [-8, 8]: every product and partial sum stays below 2^24 (K <= 9 * 256, |sum| <= 147 456 + bias + add_src), so the
    fp32 result is exact in ANY summation order: zero tolerance against int64 arithmetic;
  * standard-normal data: fp64 convolution of the HOST-rounded bf16 operands (+ fp32 bias / add_src); per element
    |out - ref| <= (K + 4) * 2^-23 * (S + |bias| + |add_src|), S the same convolution of absolute values, K = taps * C — the worst
    case of any fp32 accumulation order with a relative error of at most 2^-23 per operation (derived, not measured).  A truncating
    conversion or a wrong rounding is off by about 2^-9 * S.
The entry has no mask_src operand (include/zsg.h), so there is no mask_src refusal to test; merge_x, split-K, stream-K and the
variant bits are refused."""
import ctypes as C
import functools
import struct

import pytest
import torch

pytestmark = pytest.mark.gpu

HINTS = (0, (64, 64), (128, 64), (128, 128))

# name -> (levels [(H, W)], B, C, N, k, stride, pad, dil, extras)
CASES = {
    "rows_tail": ([(19, 19)], 2, 64, 64, 1, 1, 0, 1, {}),
    "bias_relu": ([(20, 17)], 2, 64, 128, 3, 1, 1, 1, dict(bias=True, relu=True)),
    "stride2": ([(21, 21)], 2, 128, 128, 3, 2, 1, 1, {}),
    "strided_1x1": ([(9, 11)], 3, 256, 64, 1, 2, 0, 1, {}),
    "n45": ([(10, 10)], 2, 256, 45, 3, 1, 1, 1, dict(bias=True)),
    "dil6": ([(12, 12)], 1, 64, 96, 3, 1, 6, 6, {}),
    "c40": ([(7, 9)], 2, 40, 72, 3, 1, 1, 1, {}),
    "c36": ([(7, 9)], 2, 36, 72, 3, 1, 1, 1, {}),
    "conv0_516": ([(10, 10)], 1, 256, 256, 3, 1, 1, 1, dict(wC=516)),
    "residual": ([(16, 16)], 2, 64, 256, 1, 1, 0, 1, dict(add=True, relu=True)),
    "alias": ([(16, 16)], 2, 64, 256, 1, 1, 0, 1, dict(add=True, alias=True)),
    "shared_head": ([(10, 10), (5, 5), (3, 3)], 2, 256, 256, 3, 1, 1, 1, dict(bias=True, relu=True)),
}


@pytest.fixture(scope="module")
def Z():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from zsgnet_pytorch_amd import _lib, ops
    return _lib, ops


def conv_out(n, k, s, p, d):
    return (n + 2 * p - d * (k - 1) - 1) // s + 1


def conv_ref(src, w, k, s, p, d, Ho, Wo):
    """src [B, H, W, C], w [N, k, k, C] of one dtype (int64 or float64) -> [B, Ho, Wo, N], tap by tap in that dtype's own arithmetic"""
    B, H, W, Cc = src.shape
    pad = torch.zeros(B, H + 2 * p, W + 2 * p, Cc, dtype=src.dtype)
    pad[:, p:p + H, p:p + W] = src
    out = torch.zeros(B, Ho, Wo, w.shape[0], dtype=src.dtype)
    for ty in range(k):
        for tx in range(k):
            win = pad[:, ty * d: ty * d + (Ho - 1) * s + 1: s, tx * d: tx * d + (Wo - 1) * s + 1: s]
            out += torch.matmul(win.reshape(-1, Cc), w[:, ty, tx].t()).view(B, Ho, Wo, -1)
    return out


@functools.lru_cache(maxsize=None)
def make_case(name, kind):
    """operands (fp32, CPU) and the reference of one case, computed once and shared by the tests (never modified)"""
    levels, B, Cc, N, k, s, p, d, ex = CASES[name]
    g = torch.Generator().manual_seed(sorted(CASES).index(name) * 2 + (kind == "int"))

    def draw(*shape):
        if kind == "int":
            return torch.randint(-8, 9, shape, generator=g).float()
        return torch.randn(*shape, generator=g)
    wC = ex.get("wC", Cc)
    w = draw(N, k, k, wC)
    srcs = [draw(B, H, W, Cc) for (H, W) in levels]
    outs_hw = [(conv_out(H, k, s, p, d), conv_out(W, k, s, p, d)) for (H, W) in levels]
    bias = draw(N) if ex.get("bias") else None
    adds = [draw(B, Ho, Wo, N) for (Ho, Wo) in outs_hw] if ex.get("add") else None
    refs, bounds = [], []
    for i, (x, (Ho, Wo)) in enumerate(zip(srcs, outs_hw)):
        wu = w[..., :Cc]
        if kind == "int":
            r = conv_ref(x.to(torch.int64), wu.to(torch.int64), k, s, p, d, Ho, Wo)
            if bias is not None:
                r = r + bias.to(torch.int64)
            if adds is not None:
                r = r + adds[i].to(torch.int64)
            if ex.get("relu"):
                r = r.clamp(min=0)
            assert int(r.abs().max()) < 2 ** 24
            refs.append(r.float())
            bounds.append(None)
        else:
            xb, wb = x.to(torch.bfloat16).double(), wu.to(torch.bfloat16).double()
            r = conv_ref(xb, wb, k, s, p, d, Ho, Wo)
            S = conv_ref(xb.abs(), wb.abs(), k, s, p, d, Ho, Wo)
            if bias is not None:
                r, S = r + bias.double(), S + bias.double().abs()
            if adds is not None:
                r, S = r + adds[i].double(), S + adds[i].double().abs()
            if ex.get("relu"):
                r = r.clamp(min=0)
            refs.append(r)
            bounds.append((k * k * Cc + 4) * 2.0 ** -23 * S)
    return dict(w=w, srcs=srcs, outs_hw=outs_hw, bias=bias, adds=adds, refs=refs, bounds=bounds)


def pack_jobs(L, jobs):
    """one zsg_pack_w_bf16_batched launch; jobs: [(src fp32 tensor, N, T, wC, wc0, C)] -> [int16 [N, T, C8] tensors]"""
    blob, blk, outs = b"", 0, []
    for (src, N, T, wC, wc0, Cc) in jobs:
        c8 = (Cc + 7) // 8 * 8
        dst = torch.full((N, T, c8), 0x5555, dtype=torch.int16, device="cuda")
        blob += struct.pack("<qqiiiiiiii", src.data_ptr(), dst.data_ptr(), N, T, wC, wc0, Cc, c8, blk, 0)
        blk += (N * T * c8 // 8 + 255) // 256
        outs.append(dst)
    dev = torch.frombuffer(bytearray(blob), dtype=torch.uint8).cuda()
    L.check(L.lib.zsg_pack_w_bf16_batched(dev.data_ptr(), len(jobs), blk, L.stream_ptr()), "pack")
    torch.cuda.synchronize()
    return outs


def launch(Z, name, kind, hint, poison=float("nan")):
    """run one case; returns (per-level outputs on the CPU, rc, descriptor)"""
    L, ops = Z
    levels, B, Cc, N, k, s, p, d, ex = CASES[name]
    cs = make_case(name, kind)
    wC = ex.get("wC", Cc)
    wd = cs["w"].cuda()
    (wp,) = pack_jobs(L, [(wd, N, k * k, wC, 0, Cc)])
    src_flat = torch.cat([x.reshape(-1) for x in cs["srcs"]]).cuda()
    lv_s, lv_o, so, oo = [], [], 0, 0
    for (H, W), (Ho, Wo) in zip(levels, cs["outs_hw"]):
        lv_s.append(ops.Level(so, H, W, H * W * Cc))
        lv_o.append(ops.Level(oo, Ho, Wo, Ho * Wo * N))
        so += B * H * W * Cc
        oo += B * Ho * Wo * N
    out = torch.full((oo,), poison, device="cuda")
    add = None
    if cs["adds"] is not None:
        add_flat = torch.cat([a.reshape(-1) for a in cs["adds"]]).cuda()
        if ex.get("alias"):
            out.copy_(add_flat)
            add = out
        else:
            add = add_flat
    bias = cs["bias"].cuda() if cs["bias"] is not None else None
    th = 0 if hint == 0 else ops.tile_hint(hint[0], hint[1], 1)
    desc = ops.fwd_desc(ops.TView(src_flat, B, Cc, Cc, lv_s), ops.TView(out, B, N, N, lv_o), Cc, N, k, s, p, d, wC=wC,
                        relu=bool(ex.get("relu")), tile_hint=th)
    ok = int(L.lib.zsg_conv_igemm_bf16_supported(C.byref(desc)))
    rc = L.lib.zsg_conv_igemm_bf16(C.byref(desc), src_flat.data_ptr(), wp.data_ptr(), out.data_ptr(), bias.data_ptr() if bias is not None else None,
                                   add.data_ptr() if add is not None else None, L.stream_ptr())
    torch.cuda.synchronize()
    assert ok == (1 if rc == 0 else 0), f"_supported says {ok}, the entry returned {rc}"
    res, o = [], 0
    oc = out.cpu()
    for (Ho, Wo) in cs["outs_hw"]:
        res.append(oc[o:o + B * Ho * Wo * N].view(B, Ho, Wo, N))
        o += B * Ho * Wo * N
    return res, rc, desc


def special_values():
    """fp32 bit patterns: exact ties in both directions (to the even neighbour below / above), their negatives, +-0, +-inf, the
    overflow-to-inf cases (largest finite fp32; the tie between the largest bf16 and 2^128) and NaN"""
    bits = [0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000, 0x40FE8000, 0x40FF8000, 0x3F808001, 0x3F807FFF,
            0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x7F7FFFFF, 0xFF7FFFFF, 0x7F7F8000, 0x7F7F7FFF, 0x7FC00000, 0x7F800001]
    return torch.tensor([struct.unpack("<f", struct.pack("<I", b))[0] for b in bits], dtype=torch.float64).float()


def test_packer_bit_equal_to_torch_bfloat16(Z):
    L, _ = Z
    g = torch.Generator().manual_seed(5)
    sv = special_values()
    assert int(torch.isnan(sv).sum()) >= 1 and int(torch.isinf(sv).sum()) == 2
    specs = [(5, 9, 516, 0, 256), (3, 1, 48, 8, 36), (7, 9, 64, 0, 64), (2, 4, 72, 32, 36)]      # (N, T, wC, wc0, C): C < wC; wc0 > 0 with C = 36 -> C8 = 40
    jobs, srcs = [], []
    for (N, T, wC, wc0, Cc) in specs:
        x = torch.randn(N, T, wC, generator=g)
        for r in range(min(N * T, 3)):                      # the value table inside the channel window of a few rows, at shifting offsets
            n, t = divmod(r, T)
            m = min(len(sv), Cc - r)
            x[n, t, wc0 + r: wc0 + r + m] = sv[:m]
        srcs.append(x)
        jobs.append((x.cuda(), N, T, wC, wc0, Cc))
    outs = pack_jobs(L, jobs)
    for (N, T, wC, wc0, Cc), x, o in zip(specs, srcs, outs):
        c8 = (Cc + 7) // 8 * 8
        want = torch.zeros(N, T, c8, dtype=torch.bfloat16)
        want[..., :Cc] = x[..., wc0:wc0 + Cc].to(torch.bfloat16)
        got = o.cpu().view(torch.bfloat16)
        nan = torch.isnan(want)
        assert torch.equal(torch.isnan(got), nan), "NaN positions"
        assert torch.equal(got.view(torch.int16)[~nan], want.view(torch.int16)[~nan]), f"packed image differs {(N, T, wC, wc0, Cc)}"
        assert int((o.cpu()[..., Cc:] != 0).sum()) == 0, "padding channels must be zero"


def test_activation_rounding_is_torch_bfloat16(Z):
    """1x1, C = N = 64, identity weight: out must equal bf16(src) bit for bit (finite inputs, the tie cases among them; -0 is left
    out: +0 + -0 = +0 in the accumulator)"""
    L, ops = Z
    g = torch.Generator().manual_seed(9)
    sv = special_values()
    sv = sv[torch.isfinite(sv) & (sv.abs() < 1e30) & ~((sv == 0) & (torch.signbit(sv)))]
    B, H, W, Cc = 2, 9, 7, 64
    x = torch.randn(B, H, W, Cc, generator=g)
    x.view(-1, Cc)[3, :len(sv)] = sv
    x.view(-1, Cc)[77, 64 - len(sv):] = sv
    xd, wd = x.cuda(), torch.eye(64).view(64, 1, 1, 64).contiguous().cuda()
    (wp,) = pack_jobs(L, [(wd, 64, 1, 64, 0, 64)])
    want = x.to(torch.bfloat16).float()
    for hint in HINTS:
        out = torch.full((B, H, W, 64), float("nan"), device="cuda")
        lv = [ops.Level(0, H, W, H * W * 64)]
        desc = ops.fwd_desc(ops.TView(xd.view(-1), B, 64, 64, lv), ops.TView(out.view(-1), B, 64, 64, lv), 64, 64, 1, 1, 0, 1, wC=64,
                            tile_hint=0 if hint == 0 else ops.tile_hint(hint[0], hint[1], 1))
        L.check(L.lib.zsg_conv_igemm_bf16(C.byref(desc), xd.data_ptr(), wp.data_ptr(), out.data_ptr(), None, None, L.stream_ptr()), "bf16 1x1")
        torch.cuda.synchronize()
        assert torch.equal(out.cpu().view(torch.int32), want.view(torch.int32)), f"hint {hint}"


@pytest.mark.parametrize("name", sorted(CASES))
def test_integer_data_is_exact(Z, name):
    cs = make_case(name, "int")
    for hint in HINTS:
        res, rc, _ = launch(Z, name, "int", hint)
        assert rc == 0, Z[0].lib.zsg_last_error().decode()
        for lvl, (got, ref) in enumerate(zip(res, cs["refs"])):
            assert torch.equal(got.view(torch.int32), ref.view(torch.int32)), \
                f"{name} hint {hint} level {lvl}: {int((got != ref).sum())} of {ref.numel()} elements differ, max |diff| {float((got - ref).abs().max())}"


@pytest.mark.parametrize("name", sorted(CASES))
def test_random_data_within_the_fp32_accumulation_bound(Z, name):
    cs = make_case(name, "rand")
    worst = 0.0
    for hint in HINTS:
        res, rc, _ = launch(Z, name, "rand", hint)
        assert rc == 0, Z[0].lib.zsg_last_error().decode()
        for lvl, (got, ref, bound) in enumerate(zip(res, cs["refs"], cs["bounds"])):
            assert not torch.isnan(got).any(), f"{name} hint {hint}: unwritten output elements"
            err = (got.double() - ref).abs()
            frac = float((err / bound.clamp(min=1e-300)).max())
            worst = max(worst, frac)
            assert bool((err <= bound).all()), f"{name} hint {hint} level {lvl}: max error / bound = {frac:.3f}"
    print(f"bf16 conv {name}: largest |out - ref| / bound over all tile hints = {worst:.4f}")


def test_refusals_and_supported_agree(Z):
    L, ops = Z
    x = torch.zeros(2 * 8 * 8 * 64, device="cuda")
    o = torch.zeros(2 * 8 * 8 * 64, device="cuda")
    wp = torch.zeros(64 * 64, dtype=torch.int16, device="cuda")
    lv = [ops.Level(0, 8, 8, 8 * 8 * 64)]

    def desc(**kw):
        d = ops.fwd_desc(ops.TView(x, 2, 64, 64, lv), ops.TView(o, 2, 64, 64, lv), 64, 64, 1, 1, 0, 1, wC=64)
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
    o.fill_(3.0)
    for what, d in bad.items():
        assert L.lib.zsg_conv_igemm_bf16_supported(C.byref(d)) == 0, what
        rc = L.lib.zsg_conv_igemm_bf16(C.byref(d), x.data_ptr(), wp.data_ptr(), o.data_ptr(), None, None, L.stream_ptr())
        msg = L.lib.zsg_last_error().decode()
        assert rc == -1 and "conv_igemm_bf16" in msg and len(msg) > 20, (what, rc, msg)
    torch.cuda.synchronize()
    assert float(o.min()) == 3.0 and float(o.max()) == 3.0, "a refused call must launch nothing"
    good = desc()
    assert L.lib.zsg_conv_igemm_bf16_supported(C.byref(good)) == 1
    assert L.lib.zsg_conv_igemm_bf16(C.byref(good), x.data_ptr(), wp.data_ptr(), o.data_ptr(), None, None, L.stream_ptr()) == 0
    assert L.lib.zsg_conv_igemm_bf16(C.byref(good), None, wp.data_ptr(), o.data_ptr(), None, None, L.stream_ptr()) == -1
    torch.cuda.synchronize()


def test_two_runs_write_identical_bits(Z):
    for hint in HINTS:
        a, rc, _ = launch(Z, "shared_head", "rand", hint)
        b, _, _ = launch(Z, "shared_head", "rand", hint)
        assert rc == 0
        for u, v in zip(a, b):
            assert torch.equal(u.view(torch.int32), v.view(torch.int32))
